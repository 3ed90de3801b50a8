"""Gradient clipping, accumulation and the non-finite guard without a GPU (reference: tests/gradclip_ref.py): the
restatement against torch's own clip_grad_norm_ + Adam, the chunk table, every mutant of the restatement rejected at the
bounds and by the cases of tests/test_gradclip_gpu.py, the recorded yardstick, the CLI's flags and the C-ABI."""
import math
import os
import re

import pytest
import torch

import gradclip_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [G.TEST_WD, 0.0])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_restatement_is_clip_grad_norm_then_adam(wd, gscale):
    """Three steps over five tensors in fp64.  The restatement rounds `scale` to fp32 as the kernel stores it, which moves
    the effective gradient by at most 2**-24 relatively; m and v follow by at most twice that and p by less, so
    4 * 2**-24 of the largest element bounds all three.  Every mutant lies orders of magnitude outside
    (test_every_mutant_is_rejected...)."""
    sizes = G.MULTI
    ps, grads = G.update_case(sizes)
    max_norm = G.case_max_norm(sizes, gscale)
    params = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(params, lr=G.ADAM["lr"], betas=(G.ADAM["b1"], G.ADAM["b2"]), eps=G.ADAM["eps"], weight_decay=wd)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g * gscale
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        assert float(norm) > max_norm
        opt.step()
    got = G.update_ref(sizes, torch.float64, wd, gscale=gscale, max_norm=max_norm)
    assert got[3] == G.STEPS and all(i["coef"] < 1.0 for i in got[4])
    ref = ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])
    errs = G.buffer_errs(got[:3], ref, sizes)
    print(errs)
    assert all(e <= 4 * 2.0 ** -24 for e in errs.values()), errs
    assert all(int(opt.state[p]["step"]) == G.STEPS for p in params)


def test_without_clipping_and_with_finite_gradients_it_is_adam_l2_ref():
    sizes = G.MULTI
    ps, grads = G.update_case(sizes)
    a = G.update_ref(sizes, torch.float64, G.TEST_WD, max_norm=0.0)
    b = G.update_ref(sizes, torch.float64, G.TEST_WD, max_norm=1e30)
    for k in range(len(sizes)):
        p, m, v = ps[k], torch.zeros_like(ps[k]), torch.zeros_like(ps[k])
        for s in range(G.STEPS):
            p, m, v = G.adam_l2_ref(p, grads[s][k], m, v, wd=G.TEST_WD, step=s + 1, gscale=G.f32(G.GSCALE), **G.ADAM)
        for x in (a, b):
            assert torch.equal(x[0][k], p) and torch.equal(x[1][k], m) and torch.equal(x[2][k], v)
    assert all(i["coef"] == 1.0 and i["scale"] == G.GSCALE for i in a[4] + b[4])


def test_clip_coef_is_torchs_rule():
    assert G.clip_coef(2.0, 1.0) == 1.0 / (2.0 + 1e-6) and G.clip_coef(0.5, 1.0) == 1.0 and G.clip_coef(5.0, 0.0) == 1.0
    assert G.clip_coef(1.0, 1.0) < 1.0 and G.clip_coef(1.0, 1.0, "no_eps") == 1.0
    assert G.clip_coef(0.0, 1.0) == 1.0 and G.clip_coef(float("inf"), 1.0) == 0.0


# ---- the chunk table ------------------------------------------------------------------------------------------------------------
C = G.CHUNK
TABLE_LAYOUTS = [[1], [3], [4], [5], [C - 1], [C], [C + 1], [1, 3, 5, 4097, 7], [C + 1, 1, C - 1, 2 * C, 2 * C + 3],
                 [3 * C + 2, 5]]


def test_chunk_constant_is_the_headers():
    from speech_to_image_translation_without_text_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    assert "#define S2I_GRAD_CHUNK %d" % ops.GRAD_CHUNK in header
    assert "#define S2I_GRAD_STATS_HEAD %d" % ops.GRAD_STATS_HEAD in header
    assert ops.GRAD_CHUNK == G.CHUNK == _lib.GRAD_CHUNK and ops.GRAD_CHUNK % 4 == 0


@pytest.mark.parametrize("sizes", TABLE_LAYOUTS, ids=lambda s: "-".join(str(n) for n in s))
def test_chunk_table_covers_every_element_once_and_no_padding(sizes):
    from speech_to_image_translation_without_text_amd import ops
    offsets, total = G.layout(sizes)
    table = ops.grad_chunk_table(offsets, sizes)
    hits = [0] * total
    owner = [-1] * total
    for o, n, s in zip(offsets, sizes, range(len(sizes))):
        for e in range(o, o + n):
            owner[e] = s
    for start, length, s in table:
        assert 1 <= length <= ops.GRAD_CHUNK and start % 4 == 0          # every chunk starts 16-byte aligned
        for e in range(start, start + length):
            assert owner[e] == s, "chunk (%d, %d) of tensor %d covers element %d of %d" % (start, length, s, e, owner[e])
            hits[e] += 1
    assert all(h == (1 if w >= 0 else 0) for h, w in zip(hits, owner))
    assert len(table) == sum(-(-n // ops.GRAD_CHUNK) for n in sizes)
    assert [s for _, _, s in table] == sorted(s for _, _, s in table)       # tensor by tensor: chunk0 is a prefix sum


def test_chunk_table_refuses_what_is_no_flat_layout():
    from speech_to_image_translation_without_text_amd import ops
    for offsets, sizes in (([0], [0]), ([2], [4]), ([0, 4], [8, 4]), ([8, 0], [4, 4]), ([], []), ([0], [4, 4])):
        with pytest.raises(ValueError):
            ops.grad_chunk_table(offsets, sizes)


# ---- the mutants ----------------------------------------------------------------------------------------------------------------
def _rejected(got, ref, sizes):
    """What the GPU tests would say about `got` against the restatement `ref`: the coefficient test (scale within one fp32
    ulp at every step) and the update test (CLIP_BOUNDS per buffer)."""
    out = []
    for s, (a, b) in enumerate(zip(got[4], ref[4])):
        if a.get("apply") and b.get("apply") and abs(a["scale"] - b["scale"]) > G.ulp32(b["scale"]):
            out.append("scale at step %d" % s)
    errs = G.buffer_errs(got[:3], ref[:3], sizes)
    out += ["%s %.2e" % (k, e) for k, e in errs.items() if not e <= G.CLIP_BOUNDS[k]]
    if got[3] != ref[3]:
        out.append("step count %d != %d" % (got[3], ref[3]))
    return out


def _skip_grads(sizes, bad=float("inf")):
    """The skip test's gradients: the case's, the second step's last element replaced by `bad`."""
    _, grads = G.update_case(sizes)
    grads = [[g.clone() for g in gs] for gs in grads]
    grads[1][-1].reshape(-1)[-1] = bad
    return grads


@pytest.mark.parametrize("mutant", ["norm_before_gscale", "per_tensor", "no_eps", "coef_on_decay"])
def test_every_clip_mutant_is_rejected_at_the_gpu_bounds(mutant):
    said = {}
    for sizes in G.UPDATE_LAYOUTS[:-1]:
        for wd in (G.TEST_WD, 0.0):
            ref = G.update_ref(sizes, torch.float64, wd)
            got = G.update_ref(sizes, torch.float64, wd, mutant=mutant)
            r = _rejected(got, ref, sizes)
            if r:
                said[(tuple(sizes), wd)] = r
    print(mutant, {k: v for k, v in list(said.items())[:3]})
    assert said, "no case of the GPU tests tells %s from the restatement" % mutant
    if mutant != "per_tensor":          # a single tensor's own norm is the global one
        assert any(len(k[0]) == 1 for k in said)
    assert any(len(k[0]) > 1 for k in said)


@pytest.mark.parametrize("mutant", ["skip_advances_step", "skip_decays"])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_every_skip_mutant_is_rejected(mutant, bad):
    for sizes in ([5], G.MULTI):
        grads = _skip_grads(sizes, bad)
        ref = G.update_ref(sizes, torch.float64, G.TEST_WD, grads=grads)
        assert ref[3] == G.STEPS - 1 and [i["apply"] for i in ref[4]] == [1, 0, 1]
        # the skipped step left everything as the first step had it
        one = G.update_ref(sizes, torch.float64, G.TEST_WD, grads=grads[:1], max_norm=G.case_max_norm(sizes))
        two = G.update_ref(sizes, torch.float64, G.TEST_WD, grads=grads[:2], max_norm=G.case_max_norm(sizes))
        assert all(torch.equal(a, b) for x, y in zip(one[:3], two[:3]) for a, b in zip(x, y)) and one[3] == two[3] == 1
        got = G.update_ref(sizes, torch.float64, G.TEST_WD, grads=grads, mutant=mutant)
        assert _rejected(got, ref, sizes), (mutant, sizes)
        if mutant == "skip_decays":     # ... and bit-equality across the skipped step alone already tells
            bad2 = G.update_ref(sizes, torch.float64, G.TEST_WD, grads=grads[:2], mutant=mutant, max_norm=G.case_max_norm(sizes))
            assert not all(torch.equal(a, b) for a, b in zip(one[0], bad2[0]))


def test_accumulation_dividing_an_incomplete_group_by_n_is_rejected():
    """An incomplete group of one micro-batch out of accum = 2 is a plain step (gscale 1); dividing by N halves it."""
    assert G.accum_gscale(1, 2, 2) == 0.5 and G.accum_gscale(2, 2, 2) == 0.25 and G.accum_gscale(1, 1, 2) == 1.0
    assert G.accum_gscale(1, 1, 2, "accum_full_n") == 0.5
    sizes = G.MULTI
    ref = G.update_ref(sizes, torch.float64, G.TEST_WD, gscale=G.accum_gscale(1, 1, 2), max_norm=0.0)
    got = G.update_ref(sizes, torch.float64, G.TEST_WD, gscale=G.accum_gscale(1, 1, 2, "accum_full_n"), max_norm=0.0)
    assert _rejected(got, ref, sizes)


def test_clip_bounds_are_twice_the_fp32_yardstick():
    """Elementwise IEEE arithmetic behind an fp64 norm, the same on any CPU: the figures agree from both sides.  Measured
    on clipped steps; encoder_dp_ref.KERNEL_YARDSTICK (unclipped) is not borrowed."""
    got = G.measure_yardsticks()
    print(got)
    for k, y in G.CLIP_YARDSTICK.items():
        assert got[k] == pytest.approx(y, rel=0.01), (k, got[k], y)
        assert G.CLIP_BOUNDS[k] == 2 * y


def test_exact_norm_and_its_bound():
    flat = G.flat_case(G.MULTI, "mixed")
    norm, per = G.exact_norms(flat, G.MULTI, 0.5)
    offsets, _ = G.layout(G.MULTI)
    assert math.isfinite(norm) and norm > 0 and len(per) == 5 and bool(torch.isnan(flat[offsets[0] + 1]))
    assert per[0] == 0.5 * float(torch.tensor(1e25, dtype=torch.float32))       # one element: sqrt(x * x) |gscale|, exact
    n = sum(G.MULTI)
    assert G.norm_bound(n) == (n + 4) * 2.0 ** -53
    # an fp32 accumulation loses these outright
    tiny, huge = G.flat_case([5], "tiny")[:5], G.flat_case([5], "huge")[:5]
    assert float((tiny * tiny).sum()) == 0.0 and math.isinf(float((huge * huge).sum()))
    assert G.exact_norms(G.flat_case([5], "tiny"), [5])[0] > 0 and math.isfinite(G.exact_norms(G.flat_case([5], "huge"), [5])[0])


# ---- the CLI and the C-ABI ----------------------------------------------------------------------------------------------------
def test_parser_flags_and_trainer_kwargs():
    from speech_to_image_translation_without_text_amd import train_encoder, train_encoder_head as TH
    for mod in (TH, train_encoder):
        base = ["--model", "m.pt"]
        a = mod.get_parser().parse_args(base)
        assert (a.clip_grad, a.accum, a.skip_nonfinite) == (0.0, 1, False)
        mod.check_args(a)
        kw = TH.trainer_kwargs(a)
        assert kw["fused_adam"] is False and (kw["clip_grad"], kw["accum"], kw["skip_nonfinite"]) == (0.0, 1, False)
        for bad in (["--clip_grad", "-1"], ["--accum", "0"], ["--clip_grad", "nan"]):
            with pytest.raises(SystemExit):
                mod.check_args(mod.get_parser().parse_args(base + bad))
        for on in (["--clip_grad", "1.5"], ["--accum", "2"], ["--skip_nonfinite"]):
            b = mod.get_parser().parse_args(base + on)
            mod.check_args(b)
            kw = TH.trainer_kwargs(b)
            assert kw["fused_adam"] is True and not kw["distributed"], on
        b = mod.get_parser().parse_args(base + ["--clip_grad", "1.5", "--accum", "3", "--skip_nonfinite"])
        kw = TH.trainer_kwargs(b)
        assert (kw["clip_grad"], kw["accum"], kw["skip_nonfinite"]) == (1.5, 3, True)


def test_trainers_refuse_bad_options_before_touching_the_model():
    from speech_to_image_translation_without_text_amd import encoder_train

    class Net:
        rnn_layers = 1
    for kw in (dict(clip_grad=-1.0), dict(accum=0), dict(clip_grad=float("nan"))):
        with pytest.raises(ValueError):
            encoder_train.HeadTrainer(Net(), **kw)


def test_c_abi_declares_and_binds_the_new_entry_points():
    from speech_to_image_translation_without_text_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    lib = _lib.load()
    for name, nargs in (("s2i_grad_sumsq", 9), ("s2i_grad_clip_scale", 10), ("s2i_adam_step_dev", 13),
                        ("s2i_adam_l2_step_dev", 14)):
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._SIGNATURES[name][1]) == nargs
    assert lib.s2i_version() == _lib.ABI_VERSION
    for fn in ("grad_sumsq", "grad_clip_scale", "adam_step_dev", "adam_l2_step_dev", "grad_chunk_table", "GradLayout"):
        assert hasattr(ops, fn)
    # the existing entry points kept their signatures
    assert len(_lib._SIGNATURES["s2i_adam_l2_step"][1]) == 14 and len(_lib._SIGNATURES["s2i_adam_step"][1]) == 13


def test_library_refuses_null_pointers_without_a_gpu():
    """Argument checks are host code: they answer before any launch."""
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    assert lib.s2i_grad_sumsq(None, 8, None, None, None, 1, 1, None, None) != 0
    assert b"grad_sumsq" in lib.s2i_last_error()
    assert lib.s2i_grad_clip_scale(None, None, 1, 1.0, 1.0, None, None, None, None, None) != 0
    assert lib.s2i_adam_l2_step_dev(None, None, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, None, None, None) != 0
    assert lib.s2i_adam_step_dev(None, None, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, None, None, None, None) != 0
