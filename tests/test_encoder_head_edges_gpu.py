"""The LSTM head's fused step kernels, its two-kernel path, the bias-gradient kernel and the encoder loss on the GPU against
fp64 at the shapes training runs and at their edges (encoder_train_ref.EDGE_HEAD_CASES, EDGE_LOSS_SHAPES): Hd = 512 with
all 32 batch slots of a block, the dynamic-LDS limit of both fused kernels from either side, B = 1, 31, 32 and 33, unsorted
lengths, max(lens) < L, all-equal lengths, L = 1, Hd % 8 != 0 and Hd = 520; every edge of the bias gradient's 64-row body
and 8-row tail; the loss at B > 256, ragged C, B = 1, one class, all classes distinct, and logits whose exp overflows fp32
unless the row maximum is subtracted.

Everything goes through the operators' public entries (ops.lstm_sentence, ops.encoder_loss) with the helpers, the metric
and the BOUNDS of tests/test_encoder_train_gpu.py: max|got - ref| / max|ref| per tensor against the fp64 restatement, the
bound twice the fp32 CPU restatement's worst value.  tests/test_encoder_head_edges_cpu.py keeps the tables and the yardstick
of these cases honest where there is no GPU.  NaN sentinels are on in every head run.

The refusals of s2i_lstm_bwd_step cover its extents only: it takes no row stride (dG and gates are dense by definition), so
"ldx != D * 4 * Hd" exists for s2i_lstm_train_step alone, as does h_in == h_out.

Measured on the MI355X (worst over the edge cases, all three cotangent patterns; bound beside it):
    class                bound     fused path                                two-kernel path
    out, sent, h_n, c_n  2.4e-6    2.46e-7  (1, 4, 32, 8, 1) full            3.07e-7  (4, 6, 32, 12, 2) std
    dX                   1.4e-6    5.33e-7  (6, 8, 32, 64, 2) short          5.19e-7  (6, 8, 32, 64, 2) short, fused=False
    weight gradients     1.0e-6    6.48e-7  (32, 6, 32, 512, 2) std          5.16e-7  (32, 6, 32, 512, 2) std, fused=False
    bias gradients       5.5e-7    4.33e-7  (9, 7, 32, 8, 2) ones            2.45e-7  (1, 4, 32, 8, 1) full, fused=False
    loss scalars         1.8e-4    1.19e-4  (37, 1000) distillation; hot logits 1.33e-7
    d audio              7.5e-6    2.56e-6  (257, 40) all terms weighted; hot logits 5.01e-7
    bias-gradient kernel alone: at most 0.29 of its derived bound (M = 7, N = 4096)

BOUNDS hold everywhere, so there are no bounds of this module's own.  No kernel changed.  One dispatcher change was needed:
ops.lstm_sentence refused every L that is no power of two (the table's L = 5, 6, 7) inside the matrix kernels' planner,
which tiles power-of-two images; the three 1x1 products around the recurrence see rows only, so such an L now enters
them as B * L one-pixel images (ops._step_rows).  A power-of-two L takes the form it took before.
"""
import math

import pytest
import torch

import encoder_train_ref as R
from encoder_ref import small_encoder
from test_encoder_train_gpu import BOUNDS, check_head, head_errors, head_ref, loss_errors, run_head, run_loss

pytestmark = pytest.mark.gpu

NAN = float("nan")
FUSED_CASES = [e for e in R.EDGE_HEAD_CASES if e[2] == "fused"]


def _lens(entry):
    (B, L, _, _, _), pattern, _ = entry
    return R.edge_lens(pattern, B, L)


def _all_finite(got):
    for k in ("out", "sent", "hn", "cn", "dx"):
        assert bool(torch.isfinite(got[k]).all()), "%s is not finite" % k
    assert all(bool(torch.isfinite(t).all()) for t in got["dparams"]), "a parameter gradient is not finite"


# ---- the head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("entry", R.EDGE_HEAD_CASES, ids=R.edge_case_id)
def test_edge_case_against_fp64(gpu, entry, pattern):
    """ops.LSTM_FUSED at its default: the path is the one the table names, by the rule ops.LstmSentence applies."""
    from speech_to_image_translation_without_text_amd import ops
    case, _, path = entry
    B, _, _, Hd, _ = case
    assert ops.LSTM_FUSED is True
    assert ("fused" if (B <= 32 and Hd % 8 == 0 and Hd <= 512) else "two-kernel") == path
    _all_finite(check_head(gpu, case, _lens(entry), pattern))


@pytest.mark.parametrize("entry", FUSED_CASES, ids=R.edge_case_id)
def test_two_kernel_path_at_the_fused_edge_cases(gpu, entry):
    """Both paths are held to the same reference at the same inputs."""
    _all_finite(check_head(gpu, entry[0], _lens(entry), "both", fused=False))


@pytest.mark.parametrize("mutant", ["mean_len", "rev_L", "reset"])
@pytest.mark.parametrize("entry", R.EDGE_MUTANT_CASES, ids=R.edge_case_id)
def test_mutants_are_rejected_at_short_unsorted_lens(gpu, entry, mutant):
    case, lens = entry[0], _lens(entry)
    got = run_head(gpu, case, lens, "both")
    errs = head_errors(got, head_ref(case, lens, "both", mutant))
    out_of_bounds = [(what, e) for cls, what, e in errs if not e <= BOUNDS[cls]]
    print(mutant, R.edge_case_id(entry), out_of_bounds)
    assert out_of_bounds, "mutant %s passes at %s" % (mutant, R.edge_case_id(entry))
    if mutant == "reset":
        names = {what for what, _ in out_of_bounds}      # nothing but the final state reads a finished sequence's state
        assert "h_n" in names and names <= {"h_n", "c_n"}, names


@pytest.mark.parametrize("B", [32, 5])
def test_forward_equals_the_inference_path_bit_for_bit_at_production_width(gpu, B):
    """Hd = 512, D = 2, L = 32: the training kernel repeats the inference kernel's recurrence statement for statement."""
    from speech_to_image_translation_without_text_amd import encoder_train, ops
    net = small_encoder(True, 1024).to(gpu)
    assert net.nhidden == 512 and net.num_direction == 2
    g = torch.Generator().manual_seed(12)
    mel = (torch.randn(B, 1, 2048, 40, generator=g) * 20 - 40).to(gpu)
    lens = R.edge_lens("short", B, 32)
    words, sent_i = net.forward_nhwc(mel, lens)
    tr = encoder_train.HeadTrainer(net)
    feat = tr.features(mel)
    assert tuple(feat.shape) == (B, 1, 32, 1024)
    out, sent = ops.lstm_sentence(feat, lens, net.RNN)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.0
    assert torch.equal(out, words.transpose(1, 2)), "out differs from the inference path"
    assert torch.equal(sent, sent_i), "sent differs from the inference path"


# ---- refusals ------------------------------------------------------------------------------------------------------------------
FWD_OK = dict(B=3, T=8, Hd=8, D=2, step=0)
REFUSED = [
    ("B = 33", dict(B=33)),
    ("Hd = 12", dict(Hd=12)),
    ("Hd = 520", dict(Hd=520)),
    ("D = 3", dict(D=3)),
    ("step = T", dict(step=8)),
]


def test_step_kernels_refuse_what_they_do_not_take(gpu):
    """Device buffers larger than any of the refused extents would need, NaN-prefilled outputs: a non-zero return, a message
    that names the entry, nothing written; and a valid call afterwards still matches the reference."""
    from speech_to_image_translation_without_text_amd import _lib
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream
    n = 1 << 21
    assert 33 * 8 * 3 * 4 * 520 <= n and 4 * 520 * 520 <= n
    g = torch.Generator().manual_seed(3)
    ins = [torch.randn(n, generator=g).to(gpu) for _ in range(5)]          # xproj / d_out, W_hh x 2, h_in / d_sent, gates
    lens = torch.randint(1, 9, (64,), generator=g).to(torch.int32).to(gpu)
    outs = [torch.full((n,), NAN, device=gpu) for _ in range(6)]           # h_out, c, out, gates, cst, hprev / dc, dG
    ins0, lens0 = [t.clone() for t in ins], lens.clone()

    def untouched(what):
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t.view(torch.int32) == outs[0].new_full((1,), NAN).view(torch.int32)).all()), \
                "%s: refused, yet an output was written" % what
        assert all(torch.equal(a, b) for a, b in zip(ins, ins0)) and torch.equal(lens, lens0), what

    def forward(B, T, Hd, D, step, ldx=None, h_out=None):
        return lib.s2i_lstm_train_step(p(ins[0]), D * 4 * Hd if ldx is None else ldx, p(ins[1]), p(ins[2]), p(lens), B, T, Hd, D,
                                       step, p(ins[3]), p(outs[0]) if h_out is None else h_out, p(outs[1]), p(outs[2]), D * Hd,
                                       p(outs[3]), p(outs[4]), p(outs[5]), st())

    def backward(B, T, Hd, D, step, first=1):
        return lib.s2i_lstm_bwd_step(p(ins[0]), p(ins[3]), p(ins[4]), p(ins[0]), p(ins[1]), p(ins[2]), p(lens), B, T, Hd, D,
                                     step, first, p(outs[0]), p(outs[1]), st())

    for what, change in REFUSED:
        for name, call in (("lstm_train_step", forward), ("lstm_bwd_step", backward)):
            assert call(**dict(FWD_OK, **change)) != 0, "%s took %s" % (name, what)
            err = lib.s2i_last_error()
            print("%s %s: %s" % (name, what, err.decode()))
            assert name.encode() in err and b"unsupported extents" in err, (what, err)
            untouched("%s %s" % (name, what))
    assert backward(**dict(FWD_OK, step=8, first=0)) != 0
    untouched("lstm_bwd_step step = T after the first launch")
    for what, kw, message in (("ldx = D * 4 * Hd + 4", dict(ldx=2 * 4 * 8 + 4), b"must be dense"),
                              ("ldx = 4 * Hd", dict(ldx=4 * 8), b"must be dense"),
                              ("h_in == h_out", dict(h_out=p(ins[3])), b"bad pointers")):
        assert forward(**FWD_OK, **kw) != 0, "lstm_train_step took %s" % what
        err = lib.s2i_last_error()
        print("lstm_train_step %s: %s" % (what, err.decode()))
        assert b"lstm_train_step" in err and message in err, (what, err)
        untouched("lstm_train_step " + what)
    check_head(gpu, (3, 8, 32, 8, 2), R.case_lens(3, 8), "both")


# ---- the bias gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 48, 4096])
@pytest.mark.parametrize("M", [1, 7, 8, 9, 63, 64, 65, 71, 72, 129, 1000])
def test_bias_grad_row_edges(gpu, M, N):
    """db[n] = sum_m dG[m][n].  A thread adds every 64th row of its lane into one of 8 partial sums (at most ceil(M / 64)
    running adds per element), then two three-level pairwise trees combine the 8 partial sums and the 8 row lanes: every
    element passes at most ceil(M / 64) + 6 roundings, so |got - ref| <= (ceil(M / 64) + 6) * 2^-24 * sum_m |dG[m][n]|."""
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(500 + M)
    dG = torch.randn(M, N, generator=g)
    ref, mass = dG.double().sum(0), dG.double().abs().sum(0)
    whole = torch.full((2, N), NAN, device=gpu)              # db, then a guard row
    dG_dev = dG.to(gpu)
    assert lib.s2i_lstm_bias_grad(_lib.ptr(dG_dev), M, N, _lib.ptr(whole), _lib.stream()) == 0
    torch.cuda.synchronize()
    db = whole[0].double().cpu()
    assert bool(torch.isfinite(db).all()), "db holds elements the kernel did not write"
    assert bool(torch.isnan(whole[1]).all()), "the kernel wrote behind db"
    bound = (math.ceil(M / 64) + 6) * 2.0 ** -24 * mass
    ratio = float(((db - ref).abs() / bound).max())
    print("M = %d, N = %d: worst |got - ref| / bound = %.3f" % (M, N, ratio))
    assert bool(((db - ref).abs() <= bound).all())


# ---- the loss ------------------------------------------------------------------------------------------------------------------
_LOSS = {}


def _loss_case(B, C):
    if (B, C) not in _LOSS:
        _LOSS[(B, C)] = R.loss_case(B, C)
    return _LOSS[(B, C)]


def _check_loss(gpu, name, audio, image, label, flags):
    ref, rgrad = R.loss_run(audio, image, label, **flags)
    got, ggrad = run_loss(gpu, audio, image, label, flags)
    errs = loss_errors(got, ggrad, ref, rgrad)
    for cls, what, e in errs:
        print("%s %s: %.3e (bound %.1e)" % (name, what, e, BOUNDS[cls]))
    assert all(bool(torch.isfinite(v)) for v in got.values()) and bool(torch.isfinite(ggrad).all())
    B = len(label)
    assert R.hits(got["accu"], B) == R.hits(ref["accu"], B), "accu %s against %s" % (float(got["accu"]), float(ref["accu"]))
    bad = ["%s %.3e > %.1e" % (what, e, BOUNDS[cls]) for cls, what, e in errs if not e <= BOUNDS[cls]]
    assert not bad, "; ".join(bad)
    return got, ggrad, ref


@pytest.mark.parametrize("flags", list(R.LOSS_FLAGS), ids=list(R.LOSS_FLAGS))
@pytest.mark.parametrize("B,C", R.EDGE_LOSS_SHAPES)
def test_encoder_loss_edge_shapes(gpu, B, C, flags):
    audio, image, label = _loss_case(B, C)
    assert R.loss_case_ok(audio, image, label)
    _check_loss(gpu, "(%d, %d) %s" % (B, C, flags), audio, image, label, R.LOSS_FLAGS[flags])


@pytest.mark.parametrize("flags", ["jel", "weights"])
def test_encoder_loss_with_one_class(gpu, flags):
    """Every pair is a same-class pair and every hinge argument is negative (the nearest is 0.22 from zero): the
    joint-embedding term and its gradient are exactly zero."""
    audio, image, label = R.label_case("one_class")
    got, ggrad, ref = _check_loss(gpu, "one class " + flags, audio, image, label, R.LOSS_FLAGS[flags])
    assert float(ref["loss_jel"]) == 0.0 and float(got["loss_jel"]) == 0.0 and float(got["accu"]) == 100.0
    if flags == "jel":
        assert float(got["loss"]) == 0.0 and float(ggrad.abs().sum()) == 0.0


@pytest.mark.parametrize("flags", ["jel", "weights"])
def test_encoder_loss_with_all_classes_distinct(gpu, flags):
    audio, image, label = R.label_case("distinct")
    got, _, _ = _check_loss(gpu, "distinct " + flags, audio, image, label, R.LOSS_FLAGS[flags])
    assert float(got["loss_jel"]) > 0.0


def test_encoder_loss_with_one_row(gpu):
    audio, image, label = R.single_row_case()
    got, _, _ = _check_loss(gpu, "B = 1", audio, image, label, R.LOSS_FLAGS["all"])
    assert float(got["loss_jel"]) == 0.0 and float(got["accu"]) == 100.0
    assert float(got["loss_l1"]) > 0.0 and float(got["loss_distill"]) > 0.0


@pytest.mark.parametrize("flags", list(R.HOT_LOSS_FLAGS))
def test_distillation_at_logits_whose_exp_overflows(gpu, flags):
    """audio near 100, image near 200: a kernel that lost the max subtraction of either softmax returns inf or NaN."""
    audio, image, label = R.hot_loss_case()
    got, _, _ = _check_loss(gpu, "hot " + flags, audio, image, label, R.HOT_LOSS_FLAGS[flags])
    assert float(got["loss_distill"]) > 0.0 and float(got["loss_jel"]) == 0.0 and float(got["loss_l1"]) == 0.0
