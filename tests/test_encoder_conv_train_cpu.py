"""The hand-written restatement of the conv stack's training forward / backward (tests/encoder_conv_train_ref.py) pinned to
torch autograd on the CPU, its mutants shown to be detectable at the GPU tests' inputs, the new entry points declared,
exported and bound, and train_encoder's argument parsing; the edge cases off the layer shapes (autograd pins, the yardstick
that must not rise, the mutants only they can see, the weight-gradient planner's sweep).  No GPU."""
import os
import re

import pytest
import torch
import torch.nn as nn

import encoder_conv_train_ref as R
import encoder_train_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["s2i_conv1d_dgrad", "s2i_conv1d_wgrad_workspace_bytes", "s2i_conv1d_wgrad", "s2i_bn_relu_forward",
               "s2i_bn_relu_bwd_reduce", "s2i_bn_relu_bwd_apply", "s2i_maxpool_w3s2_backward", "s2i_bn1_stats", "s2i_bn1_finalize",
               "s2i_bn1_bwd_reduce", "s2i_bn1_bwd_finalize"]

_CACHE = {}


def stock_run(B=4, T=128):
    """Autograd through the model's own nn.Sequential (.double().train(), NCHW) and, behind it, a stock nn.LSTM over packed
    sequences and the restated loss -> features, loss, every parameter gradient, the state after the call."""
    if "stock" in _CACHE:
        return _CACHE["stock"]
    net = R.stack_net(bidirectional=True, nhidden=64)
    mel, lens, image, label = R.trainer_case(B, T, H=64)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ref = R.stack_net(bidirectional=True, nhidden=64).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in before.items()})
    ref.Conv.train()
    feat = ref.Conv(mel[:, 0].transpose(1, 2).unsqueeze(1))                  # [B, 1, n_mels, T] -> [B, 1024, 1, T/64]
    feat_nhwc = feat.permute(0, 2, 3, 1)
    packed = nn.utils.rnn.pack_padded_sequence(feat_nhwc[:, 0], torch.tensor(lens), batch_first=True)
    out, _ = ref.RNN(packed)
    out, _ = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=feat_nhwc.shape[2])
    res = TR.encoder_loss(out.mean(1), image, label)
    res["loss"].backward()
    _CACHE["stock"] = dict(net=net, inputs=(mel, lens, image, label), feat=feat_nhwc.detach(), loss=res["loss"].detach(),
                           grads={n: p.grad.clone() for n, p in ref.named_parameters()},
                           state={k: v.detach().clone() for k, v in ref.state_dict().items()})
    return _CACHE["stock"]


def test_stack_restatement_equals_autograd():
    s = stock_run()
    mel, lens, image, label = s["inputs"]
    layers = R.stack_layers(s["net"])
    res, grads, cache = R.full_grads(layers, R.rnn_params(s["net"]), mel, lens, image, label)
    assert R.rel_err(cache[-1]["out"], s["feat"]) < 1e-10
    assert abs(float(res["loss"]) - float(s["loss"])) < 1e-10 * max(1.0, abs(float(s["loss"])))
    assert set(R.grad_names(grads)) == set(s["grads"])
    for n, g in s["grads"].items():
        e = R.grad_err(n, g, grads)
        assert e < 1e-10, (n, e)
    # the leading BatchNorm's bias gradient is structurally zero; its weight gradient is small but real
    assert float(s["grads"]["Conv.0.bias"].abs().max()) < 1e-12 * float(grads[R.MASS + "Conv.0.bias"])
    assert float(s["grads"]["Conv.0.weight"].abs().max()) > 1e-5
    assert float(s["grads"]["Conv.0.weight"].abs().max()) > 0 and float(s["grads"]["Conv.1.0.weight"].abs().max()) > 0
    run = R.running_state(layers, cache)
    assert len(run) == 3 * 9
    for n, v in run.items():
        if n.endswith("num_batches_tracked"):
            assert int(v) == int(s["state"][n]) == 1, n
        else:
            assert R.rel_err(v, s["state"][n]) < 1e-10, n


def test_replayed_own_decisions_change_nothing():
    s = stock_run()
    mel, lens, image, label = s["inputs"]
    layers = R.stack_layers(s["net"])
    feat, cache = R.stack_forward(layers, mel)
    g = torch.Generator().manual_seed(1)
    dfeat = torch.randn(feat.shape, generator=g, dtype=torch.float64)
    a, da = R.stack_backward(layers, cache, dfeat)
    b, db = R.stack_backward(layers, cache, dfeat, R.own_decisions(layers, cache))
    assert all(torch.equal(a[n], b[n]) for n in a) and torch.equal(da, db)


@pytest.mark.parametrize("cin,cout,geom", R.LAYER_GEOMS, ids=lambda v: str(v).replace(" ", ""))
def test_launch_restatements_equal_autograd(cin, cout, geom):
    """conv_dgrad / conv_wgrad against autograd through F.conv2d at Wo = 1 and Wo = 8 (B = 3)."""
    k, s, pad = geom
    for Wo in (1, 8):
        x, w, dy = R.conv_case(cin, cout, geom, 3, Wo)
        xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        wt = w.unsqueeze(2).clone().requires_grad_(True)
        y = torch.nn.functional.conv2d(xt, wt, None, (1, s), (0, pad))
        assert y.shape[3] == Wo
        gx, gw = torch.autograd.grad(y, [xt, wt], dy.permute(0, 3, 1, 2))
        assert R.rel_err(R.conv_dgrad(dy, w, geom, x.shape[2]), gx.permute(0, 2, 3, 1)) < 1e-12
        assert R.rel_err(R.conv_wgrad(x, dy, geom), gw) < 1e-12


def test_pool_restatement_equals_autograd_with_ties():
    for ties in (False, True):
        x, dy = R.pool_case(3, 16, 64, ties=ties)
        xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = torch.nn.functional.max_pool2d(xt, (1, 3), (1, 2), (0, 1))
        (gx,) = torch.autograd.grad(y, [xt], dy.permute(0, 3, 1, 2))
        got = R.pool_backward(x.shape, R.pool_argmax(x), dy)
        assert torch.equal(got, gx.permute(0, 2, 3, 1)), ties
        if ties:
            gap = R.pool_gap(x)
            assert bool((gap == 0).any()) and int(R.pool_argmax(x)[0, 0, 0, 0]) == 0 and float(gap[0, 0, 0, 0]) == 0.0


def test_bn_restatement_equals_batchnorm2d():
    y, gamma, beta, dout, running = R.bn_case(24, 64)
    bn = nn.BatchNorm2d(64).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(running[0])
        bn.running_var.copy_(running[1])
        bn.num_batches_tracked.fill_(running[2])
    yt = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    out = torch.relu(bn(yt))
    gy, gg, gb = torch.autograd.grad(out, [yt, bn.weight, bn.bias], dout.permute(0, 3, 1, 2))
    coef, new = R.bn_finalize(y, gamma, beta, running)
    z, o = R.bn_relu_forward(y, coef)
    dy, dgamma, dbeta = R.bn_relu_backward(y, o > 0, dout, coef)
    assert R.rel_err(o, out.permute(0, 2, 3, 1)) < 1e-12 and R.rel_err(dy, gy.permute(0, 2, 3, 1)) < 1e-11
    assert R.rel_err(dgamma, gg) < 1e-12 and R.rel_err(dbeta, gb) < 1e-12
    assert R.rel_err(new[0], bn.running_mean) < 1e-12 and R.rel_err(new[1], bn.running_var) < 1e-12
    assert new[2] == int(bn.num_batches_tracked) == 4
    assert R.margin_ok(z, 1e-4)


# ---- mutants: each differs from the truth by more than 10 x the class bound at the GPU tests' inputs ----------------------
def gpu_bounds():
    import test_encoder_conv_train_gpu as G
    return G.BOUNDS


def test_dgrad_mutants_differ():
    B = gpu_bounds()
    for cin, cout, geom in R.LAYER_GEOMS:
        x, w, dy = R.conv_case(cin, cout, geom, 3, 8)
        ref = R.conv_dgrad(dy, w, geom, x.shape[2])
        assert R.rel_err(R.conv_dgrad(dy, w, geom, x.shape[2], "pad_m1"), ref) > 10 * B["dgrad"], geom
        if geom[1] == 2:
            assert R.rel_err(R.conv_dgrad(dy, w, geom, x.shape[2], "no_parity"), ref) > 10 * B["dgrad"], geom


def test_bn_and_pool_mutants_differ():
    B = gpu_bounds()
    for M, C in ((24, 64), (6144, 1024)):
        y, gamma, beta, dout, running = R.bn_case(M, C)
        coef, new = R.bn_finalize(y, gamma, beta, running)
        mask = R.bn_relu_forward(y, coef)[1] > 0
        ref = R.bn_relu_backward(y, mask, dout, coef)[0]
        assert R.rel_err(R.bn_relu_backward(y, mask, dout, coef, "bn_no_xhat")[0], ref) > 10 * B["bn_dy"], (M, C)
        bad = R.bn_finalize(y, gamma, beta, running, "biased_var")[1]
        assert R.rel_err(bad[1], new[1]) > 10 * B["running"], (M, C)
    for W in (2, 16):
        x, dy = R.pool_case(3, W, 64, ties=True)
        idx = R.pool_argmax(x)
        ref = R.pool_backward(x.shape, idx, dy)
        if W > 2:       # one window at W = 2: nothing overlaps
            assert R.rel_err(R.pool_backward(x.shape, idx, dy, "pool_no_add"), ref) > 10 * B["pool_dx"], W


def test_stack_mutants_differ():
    """At the whole-stack GPU test's inputs every mutant moves some parameter gradient (or running variance) by more than
    10 x its bound."""
    B = gpu_bounds()
    s = stock_run()
    mel, lens, image, label = s["inputs"]
    layers = R.stack_layers(s["net"])
    feat, cache = R.stack_forward(layers, mel)
    g = torch.Generator().manual_seed(1)
    dfeat = torch.randn(feat.shape, generator=g, dtype=torch.float64)
    ref, _ = R.stack_backward(layers, cache, dfeat)
    for mutant in ("pad_m1", "no_parity", "bn_no_xhat", "pool_no_add", "bn0_dropped"):
        got, _ = R.stack_backward(layers, cache, dfeat, mutant=mutant)
        worst = max(R.grad_err(n, got[n], ref) for n in R.grad_names(ref))
        assert worst > 10 * B["stack_grad"], (mutant, worst)
    _, cache_b = R.stack_forward(layers, mel, "biased_var")
    a, b = R.running_state(layers, cache), R.running_state(layers, cache_b)
    assert max(R.rel_err(b[n], a[n]) for n in a if n.endswith("running_var")) > 10 * B["running"]


# ---- off the layer shapes ---------------------------------------------------------------------------------------------------
EDGE_GEOMS = R.CONV_EDGE_CASES + R.WGRAD_ONLY_CASES


@pytest.mark.parametrize("case", EDGE_GEOMS, ids=lambda c: str(c).replace(" ", ""))
def test_edge_restatements_equal_autograd(case):
    cin, cout, geom, B, Wo = case
    k, s, pad = geom
    x, w, dy = R.conv_case(*case)
    assert x.shape[2] == Wo * s and (x.shape[2] + 2 * pad - k) // s + 1 == Wo
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wt = w.unsqueeze(2).clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt, None, stride=(1, s), padding=(0, pad))
    assert y.shape[3] == Wo
    gx, gw = torch.autograd.grad(y, [xt, wt], dy.permute(0, 3, 1, 2))
    assert R.rel_err(R.conv_dgrad(dy, w, geom, x.shape[2]), gx.permute(0, 2, 3, 1)) < 1e-12
    assert R.rel_err(R.conv_wgrad(x, dy, geom), gw) < 1e-12


def yardsticks():
    if "yard" not in _CACHE:
        _CACHE["yard"] = R.measure_yardsticks(verbose=False)
    return _CACHE["yard"]


def as_written(value, bound):
    """`value` rounded to the number of significant digits `bound` is written with (BOUNDS holds two or three)."""
    digits = next(d for d in range(1, 17) if float("%.*e" % (d - 1, bound)) == bound)
    return float("%.*e" % (digits - 1, value))


def test_no_yardstick_rises_above_half_its_bound():
    """The bounds are twice the yardsticks, so over the old and the new cases no class may exceed BOUND / 2.  BOUNDS is
    written to two or three digits, rounded to nearest (2 x 6.22e-7 is 1.24e-6), so the comparison is made at the bound's
    own written precision; the block_* classes, new with the edge cases, are held to the exact statement."""
    B = gpu_bounds()
    Y = {k: v for k, v in yardsticks().items() if not k.startswith("_")}
    for k, v in sorted(Y.items()):
        print("%-18s %.3e" % (k, v))
    assert set(B) <= set(Y)
    bad = ["%s 2 x %.3e > %.3e" % (k, Y[k], B[k]) for k in B if not as_written(2 * Y[k], B[k]) <= B[k]]
    assert not bad, "; ".join(bad)
    for k in ("block_out", "block_running", "block_dx", "block_dw", "block_dparam"):
        assert Y[k] <= B[k] / 2, k


def test_fp32_block_restatement_flips_no_relu_decision():
    flips = yardsticks()["_block_flips"]
    assert [c for c, _ in flips] == R.BLOCK_CASES
    assert all(n == 0 for _, n in flips), flips


@pytest.mark.parametrize("mutant", sorted(R.MUTANT_KILLS))
def test_edge_mutants_are_inert_on_the_layer_cases_and_rejected_on_the_edge_cases(mutant):
    """The fp32 restatement stands in for the GPU: a kernel with this mistake would return bit-identical results at every
    old case (the gap) and leaves BOUNDS at the edge cases (how the gap is closed)."""
    B = gpu_bounds()
    f = lambda t: t.float()
    wgrad = mutant == "col_tail_zero"
    cls = "wgrad" if wgrad else "dgrad"

    def run(case, m, dtype=torch.float32):
        x, w, dy = (t.to(dtype) for t in R.conv_case(*case))
        return R.conv_wgrad(x, dy, case[2], m) if wgrad else R.conv_dgrad(dy, w, case[2], x.shape[2], m)

    for case in R.CONV_CASES:
        assert torch.equal(run(case, mutant), run(case, None)), case
    killed = []
    for case in R.CONV_EDGE_CASES + (R.WGRAD_ONLY_CASES if wgrad else []):
        if R.rel_err(run(case, mutant), run(case, None, torch.float64)) > B[cls]:
            killed.append(case)
    print(mutant, "rejected at", killed)
    assert R.MUTANT_KILLS[mutant] in killed
    # and against the fp64 truth the mutant itself is far outside: what the GPU test asserts of the GPU's result
    case = R.MUTANT_KILLS[mutant]
    assert R.rel_err(run(case, None), run(case, mutant, torch.float64)) > 10 * B[cls]


def wgrad_tiles(cin, cout, k):
    """Blocks of one split under the documented tile choice: 128 x 128, 128 x 64 (Cin <= 64) or 64 x 64 (Cout <= 64)."""
    bm, bn = (128, 128) if (cout > 64 and cin > 64) else ((128, 64) if cout > 64 else (64, 64))
    return -(-cout // bm) * -(-cin // bn) * k


def test_wgrad_planner_sweep():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    geoms = sorted(set([g for g in R.LAYER_GEOMS] + [c[:3] for c in EDGE_GEOMS]))
    widths = sorted(set(v for g in geoms for v in g[:2]))
    combos = set(geoms) | set((ci, co, g[2]) for g in geoms for ci in widths for co in widths
                              if (ci, co) in ((g[0], g[1]), (4, 1024), (1024, 4), (68, 36)))
    n = 0
    for cin, cout, (k, s, pad) in sorted(combos):
        for B in (1, 3, 33, 64):
            for Wo in (1, 8, 16, 32, 2048):
                W = Wo * s
                assert (W + 2 * pad - k) // s + 1 == Wo
                nbytes = lib.s2i_conv1d_wgrad_workspace_bytes(B, W, cin, cout, k, s, pad)
                slab = cout * k * cin * 4
                what = (cin, cout, k, s, pad, B, Wo)
                if max(B * Wo * cout, B * W * cin) * 4 >= 0x7ff00000:       # past the 2 GiB buffer-addressing window
                    assert nbytes == 0, what
                    continue
                assert nbytes > 0 and nbytes % slab == 0, what
                splits = nbytes // slab
                nchunks = -(-B * Wo // 32)
                lo = -(-nchunks // 16)
                hi = max(1, lo, min(768 // wgrad_tiles(cin, cout, k), nchunks // 4))
                assert lo <= splits <= hi, (what, splits, lo, hi)
                n += 1
    assert n >= 20 * len(geoms)
    # every clause of the guard
    ok = (3, 16, 64, 64, 3, 1, 1)
    assert lib.s2i_conv1d_wgrad_workspace_bytes(*ok) == 64 * 3 * 64 * 4
    refused = {"B = 0": (0, 16, 64, 64, 3, 1, 1), "W = 0": (3, 0, 64, 64, 3, 1, 1), "W = 48": (3, 48, 64, 64, 3, 1, 1),
               "Cin = 0": (3, 16, 0, 64, 3, 1, 1), "Cin = 6": (3, 16, 6, 64, 3, 1, 1), "Cout = 0": (3, 16, 64, 0, 3, 1, 1),
               "Cout = 34": (3, 16, 64, 34, 3, 1, 1), "kw = 0": (3, 16, 64, 64, 0, 1, 0), "kw = 32": (3, 16, 64, 64, 32, 1, 16),
               "stride 0": (3, 16, 64, 64, 3, 0, 1), "pad -1": (3, 16, 64, 64, 3, 1, -1), "Wo = 14": (3, 16, 64, 64, 3, 1, 0),
               "Wo = 0": (3, 2, 64, 64, 5, 1, 0), "dy over 2 GiB": (4096, 2048, 4, 64, 1, 1, 0),
               "x over 2 GiB": (4096, 2048, 64, 4, 1, 1, 0)}
    for why, args in refused.items():
        assert lib.s2i_conv1d_wgrad_workspace_bytes(*args) == 0, why
        assert b"conv1d wgrad" in lib.s2i_last_error(), why


def test_dgrad_guard_is_narrower_than_wgrads():
    """the two weight-gradient-only cases stay weight-gradient tests; the input gradient refuses them before
    it touches a pointer (no device here: the pointers are never followed)."""
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    for cin, cout, (k, s, pad), B, Wo in R.WGRAD_ONLY_CASES:
        assert lib.s2i_conv1d_wgrad_workspace_bytes(B, Wo * s, cin, cout, k, s, pad) > 0
        assert lib.s2i_conv1d_dgrad(1, 1, 1, B, Wo * s, cin, cout, cin, cout, k, s, pad, None) != 0
        assert b"conv1d dgrad" in lib.s2i_last_error()


def test_bn1_stats_refuses_bad_arguments():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    for args in ((None, 8, 1, 1), (1, 8, None, 1), (1, 0, 1, 1), (1, 6, 1, 1), (1, 8, 1, 0)):
        assert lib.s2i_bn1_stats(*args, None) != 0, args
        assert b"bn1_stats" in lib.s2i_last_error()


# ---- the C surface and the CLI ---------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    from speech_to_image_translation_without_text_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    makefile = open(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc", "Makefile")).read()
    assert "s2i_conv1d_train.hip" in makefile
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib._SIGNATURES, name
    assert _lib.ABI_VERSION == 7


def test_new_symbols_exported_and_refuse_bad_arguments():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    assert not [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert lib.s2i_version() == 7
    # host-side planning and argument checks, no device needed
    assert lib.s2i_conv1d_wgrad_workspace_bytes(64, 2048, 64, 64, 3, 1, 1) >= 64 * 64 * 3 * 4 * 256     # 131 072 rows: split
    assert lib.s2i_conv1d_wgrad_workspace_bytes(64, 64, 512, 1024, 5, 2, 2) == 4 * 1024 * 5 * 512 * 4     # 2 048 rows: 4 slabs
    assert lib.s2i_conv1d_wgrad_workspace_bytes(3, 2, 64, 128, 17, 2, 8) == 128 * 17 * 64 * 4             # Wo = 1: one slab
    assert lib.s2i_conv1d_wgrad_workspace_bytes(3, 48, 64, 64, 3, 1, 1) == 0
    assert b"power of two" in lib.s2i_last_error() or b"bad extent" in lib.s2i_last_error()
    assert lib.s2i_conv1d_dgrad(None, None, None, 3, 16, 64, 64, 64, 64, 3, 1, 1, None) != 0
    assert lib.s2i_conv1d_dgrad(1, 1, 1, 3, 16, 64, 48, 64, 48, 3, 1, 1, None) != 0
    assert b"multiple of 32" in lib.s2i_last_error()
    assert lib.s2i_conv1d_dgrad(1, 1, 1, 3, 16, 64, 64, 64, 64, 3, 3, 1, None) != 0
    assert lib.s2i_bn_relu_forward(None, 4, 64, None, None, None) != 0
    assert lib.s2i_maxpool_w3s2_backward(1, 1, 3, 1, 3, 64, 1, None) != 0


def test_train_encoder_arguments():
    from speech_to_image_translation_without_text_amd import train_encoder as T
    from speech_to_image_translation_without_text_amd import train_encoder_head as TH
    assert T.SplitData is TH.SplitData
    a = T.get_parser().parse_args(["--data_dir", "/data"])
    assert a.model == "" and a.seed == 1234 and a.dataset == "birds" and not a.bidirectional
    b = T.get_parser().parse_args(["--data_dir", "/data", "--model", "enc.pth", "--bidirectional", "--seed", "7", "--epoch", "3"])
    assert b.model == "enc.pth" and b.bidirectional and b.seed == 7 and b.epoch == 3
    head = TH.get_parser().parse_args(["--data_dir", "/data", "--model", "enc.pth"])
    assert set(vars(head)) | {"seed"} == set(vars(a))
    with pytest.raises(SystemExit):
        T.get_parser().parse_args(["--dataset", "cars"])                               # birds or flowers
    with pytest.raises(SystemExit):
        T.get_parser().parse_args(["--data_dir", "/data", "--rnn_layers", "2"])        # no such option: one LSTM layer only
    for bad in (["--batch_size", "0"], ["--epoch", "0"], ["--eval_every", "0"]):
        with pytest.raises(SystemExit):
            T.check_args(T.get_parser().parse_args(bad))
    with pytest.raises(SystemExit):
        TH.get_parser().parse_args(["--data_dir", "/data"])                            # the head CLI still requires --model


def test_train_encoder_builds_the_reference_initialisation():
    """Without --model the CLI's encoder is CNNRNN(40, 1024, nhidden=1024, nsent=1024) under torch.manual_seed(seed): the
    same tensors as building it by hand, and the reference's key set."""
    from speech_to_image_translation_without_text_amd import train_encoder as T
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    a = T.get_parser().parse_args(["--data_dir", "/data", "--bidirectional", "--seed", "5"])
    net = T.build_model(a)
    torch.manual_seed(5)
    ref = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True)
    sd, rd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rd) and all(torch.equal(sd[k], rd[k]) for k in sd)
    assert not net.training
