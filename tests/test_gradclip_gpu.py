"""Gradient clipping, accumulation and the non-finite guard of the fused optimiser on the GPU (references:
tests/gradclip_ref.py).

    check                              bound                                          worst seen on the MI355X
    norm (44 cases)                    (n + 4) 2**-53 relative, derived               2.5e-4 of the bound (1.14e-16 / 4.55e-13); <= 1.87e-16
    per-tensor norms                   the same per tensor                            0.015 of the bound
    scale (96 cases)                   1 fp32 ulp of the restatement's                0 ulp
    _dev entry points, off path        bit for bit                                    equal
    clipped update p (18 cases)        3.06e-7 (2 x 1.53e-7, CPU fp32 against fp64)   1.53e-7
    clipped update m                   3.62e-7 (2 x 1.81e-7)                          1.58e-7
    clipped update v                   5.20e-7 (2 x 2.60e-7)                          2.41e-7
    skipped step                       bit for bit unchanged                          equal
    step after a skip p / m / v (21)   the clipped update's bounds                    6.94e-8 / 1.06e-7 / 1.65e-7
    EncoderTrainer.step, clip on       encoder_dp_ref.TRAJ_BOUNDS traj_update 1.27e-2 1.58e-3
    two gloo ranks, clip on            encoder_dp_ref.TRAJ_BOUNDS dp_update 1.11e-3   1.94e-4

The norm's bound is derived in gradclip_ref (exact squares, non-negative terms, one rounding per addition in any order); the
update's is twice the deviation of the restatement in fp32 from fp64 on the same clipped cases
(gradclip_ref.CLIP_YARDSTICK, re-measured by tests/test_gradclip_cpu.py).  Every test prints what it measured next to its
bound.  Every process started here has its own time limit and nothing is retried.
"""
import copy
import math
import os
import re
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

import encoder_conv_train_ref as R
import encoder_dp_ref as D
import encoder_ref
import gradclip_ref as G
from speech_loader_ref import make_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROCESS_LIMIT = 300
C = G.CHUNK
LAYOUTS = [[n] for n in G.SINGLE_SIZES] + [G.MULTI, "head", "encoder"]
KINDS = ["normal", "tiny", "huge", "mixed"]


def lid(x):
    return x if isinstance(x, str) else "-".join(str(n) for n in x)


def sizes_of(layout):
    return G.real_sizes(layout) if isinstance(layout, str) else layout


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def glayout(sizes, gpu):
    from speech_to_image_translation_without_text_amd import ops
    offsets, total = G.layout(sizes)
    return ops.GradLayout(offsets, sizes, total, gpu)


def norm_pass(flat_gpu, L, gscale=1.0, max_norm=0.0, step_dev=None):
    from speech_to_image_translation_without_text_amd import ops
    ops.grad_sumsq(flat_gpu, L)
    ops.grad_clip_scale(L, gscale, max_norm, step_dev)
    return L.read_stats()


# ---- 1. the norm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lid)
def test_norm_meets_the_derived_bound(gpu, layout, kind):
    sizes = sizes_of(layout)
    flat = G.flat_case(sizes, kind)
    offsets, total = G.layout(sizes)
    pads = total - sum(sizes)
    assert int(torch.isnan(flat).sum()) == pads          # the padding holds NaN: one read of it and the norm is NaN
    ref, ref_per = G.exact_norms(flat, sizes, G.GSCALE)
    L = glayout(sizes, gpu)
    g = flat.to(gpu)
    st = norm_pass(g, L, G.GSCALE)
    first = (L.stats.clone(), L.partials.clone())
    L.stats.zero_()
    L.partials.fill_(-1.0)
    st2 = norm_pass(g, L, G.GSCALE)
    assert same_bits(first[0], L.stats) and same_bits(first[1], L.partials), "two runs gave different bits"
    n = sum(sizes)
    err = abs(st["norm"] - ref) / ref
    worst_t = max(abs(a - b) / b / G.norm_bound(m) for a, b, m in zip(st["tensor_norms"], ref_per, sizes))
    print("%s %s: norm %.17g ref %.17g rel err %.3e (bound %.3e); per tensor worst err / bound %.3f"
          % (lid(layout), kind, st["norm"], ref, err, G.norm_bound(n), worst_t))
    assert math.isfinite(st["norm"]) and st["apply"] == 1 and st2["updates"] == 1 and st["skipped"] == 0
    assert err <= G.norm_bound(n)
    assert worst_t <= 1.0
    assert st["coef"] == 1.0 and st["scale"] == G.GSCALE


def test_fp32_accumulation_would_fail_the_extremes(gpu):
    """The control of the extremes: torch's fp32 norm of the same buffers is 0 and inf."""
    for kind, want in (("tiny", 0.0), ("huge", float("inf"))):
        x = G.flat_case([C + 1], kind)[:C + 1].to(gpu)
        assert float((x * x).sum().sqrt()) == want


@pytest.mark.parametrize("layout", [[1], [5], G.MULTI, [C + 1]], ids=lid)
def test_zero_gradient(gpu, layout):
    L = glayout(layout, gpu)
    step_dev = torch.zeros(1, dtype=torch.int32, device=gpu)
    st = norm_pass(G.flat_case(layout, "zero").to(gpu), L, 0.5, 1.0, step_dev)
    print(st["norm"], st["coef"], st["apply"])
    assert st["norm"] == 0.0 and st["coef"] == 1.0 and st["apply"] == 1 and st["scale"] == 0.5 and int(step_dev) == 1
    assert st["tensor_norms"] == [0.0] * len(layout)


def test_wrappers_refuse_what_the_kernels_refuse(gpu):
    from speech_to_image_translation_without_text_amd import _lib, ops
    L = glayout([5, 3], gpu)
    g = torch.zeros(L.total, device=gpu)
    with pytest.raises(_lib.S2IError):
        ops.grad_sumsq(g[:-1], L)                          # not the layout's buffer
    with pytest.raises(_lib.S2IError):
        ops.grad_sumsq(g.double(), L)
    with pytest.raises(_lib.S2IError):
        ops.grad_sumsq(g.cpu(), L)
    with pytest.raises(_lib.S2IError):
        ops.grad_clip_scale(L, 1.0, -1.0)
    with pytest.raises(_lib.S2IError):
        ops.grad_clip_scale(L, 1.0, float("nan"))
    with pytest.raises(ValueError):
        ops.GradLayout([0, 8], [5, 3], 10, gpu)            # ends behind the buffer
    t = torch.zeros(8, device=gpu)
    with pytest.raises(_lib.S2IError):
        ops.adam_l2_step_dev(t, t.clone(), t.clone(), t.clone(), 1e-3, 0.9, 0.999, 1e-8, 0.1, None, L.scale, L.apply)
    with pytest.raises(_lib.S2IError):
        ops.adam_step_dev(t, t.clone(), t.clone(), t.clone(), 1e-3, 0.9, 0.999, 1e-8, L.apply, L.scale, None)
    assert float(t.abs().sum()) == 0.0
    # a layout that leaves the buffer it is given is not read: the C entry point is handed a shorter n than the layout's
    lib = _lib.load()
    ops.check(lib.s2i_grad_sumsq(ops.ptr(g), 4, ops.ptr(L.offsets), ops.ptr(L.sizes), ops.ptr(L.chunk0), L.S, L.nchunks,
                                 ops.ptr(L.partials), ops.stream()), "s2i_grad_sumsq")
    torch.cuda.synchronize()
    assert bool(torch.isnan(L.partials).all())


# ---- 2. the coefficient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [0.5, 1.0 / 3.0])
@pytest.mark.parametrize("layout", G.SMALL_LAYOUTS, ids=lid)
def test_scale_is_within_one_ulp_of_the_restatement(gpu, layout, gscale):
    flat = G.flat_case(layout, "normal")
    offsets, _ = G.layout(layout)
    total = math.fsum(G.exact_sumsq(flat[o:o + n]) for o, n in zip(offsets, layout))
    norm = math.sqrt(total) * gscale
    L = glayout(layout, gpu)
    g = flat.to(gpu)
    worst = 0.0
    for what, max_norm in (("below", 0.5 * norm), ("far below", 1e-3 * norm), ("at", norm), ("above", 10 * norm),
                           ("just above", (norm + 1e-6) * (1 + 1e-12)), ("off", 0.0)):
        st = norm_pass(g, L, gscale, max_norm)
        _, coef, scale = G.clip_scale(total, gscale, max_norm)
        ulps = abs(st["scale"] - scale) / G.ulp32(scale)
        worst = max(worst, ulps)
        print("%s gscale %.3g max_norm %s the norm: scale %.9g ref %.9g (%.2f ulp, bound 1), coef %.6g"
              % (lid(layout), gscale, what, st["scale"], scale, ulps, st["coef"]))
        assert ulps <= 1.0 and float(L.scale) == st["scale"] and int(L.apply) == 1
        if what in ("below", "far below", "at"):
            assert st["coef"] < 1.0 and coef < 1.0
        else:                                   # norm + 1e-6 <= max_norm, or no clipping: exactly float32(gscale)
            assert st["coef"] == 1.0 and st["scale"] == G.f32(gscale)
    last = L.read_stats()
    assert (last["updates"], last["clipped"], last["skipped"]) == (6, 3, 0)


# ---- 3. bit for bit ------------------------------------------------------------------------------------------------------------
def flat_params(sizes, gpu):
    gen = torch.Generator().manual_seed(8100 + sum(sizes) % 9973)
    _, total = G.layout(sizes)
    return (0.05 + 0.1 * torch.rand(total, generator=gen)).to(gpu)


@pytest.mark.parametrize("wd", [G.TEST_WD, 0.0], ids=["l2", "plain"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lid)
def test_dev_entry_points_equal_the_host_value_ones_bit_for_bit(gpu, layout, wd):
    from speech_to_image_translation_without_text_amd import ops
    sizes = sizes_of(layout)
    a = G.ADAM
    L = glayout(sizes, gpu)
    p0 = flat_params(sizes, gpu)
    dev_set = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    host_set = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    sd_dev = torch.zeros(1, dtype=torch.int32, device=gpu)
    sd_host = torch.zeros(1, dtype=torch.int32, device=gpu)
    for step in range(2):
        g = torch.nan_to_num(G.flat_case(sizes, "normal", seed=step), nan=0.0).to(gpu)       # FlatNet keeps the padding zero
        ops.grad_sumsq(g, L)
        ops.grad_clip_scale(L, G.GSCALE, 1e-4, sd_dev)           # every case's norm is above 1e-3: coef < 1
        scale = float(L.scale)                      # the host value of the device scale
        assert 0.0 < scale < G.GSCALE
        ops.increment(sd_host)
        if wd:
            ops.adam_l2_step_dev(*dev_set[:1], g, *dev_set[1:], a["lr"], a["b1"], a["b2"], a["eps"], wd, sd_dev, L.scale, L.apply)
            ops.adam_l2_step(*host_set[:1], g, *host_set[1:], a["lr"], a["b1"], a["b2"], a["eps"], wd, step_dev=sd_host,
                             gscale=scale)
        else:
            ops.adam_step_dev(*dev_set[:1], g, *dev_set[1:], a["lr"], a["b1"], a["b2"], a["eps"], sd_dev, L.scale, L.apply)
            ops.adam_step(*host_set[:1], g, *host_set[1:], a["lr"], a["b1"], a["b2"], a["eps"], step_dev=sd_host, gscale=scale)
    torch.cuda.synchronize()
    assert int(sd_dev) == int(sd_host) == 2
    assert not torch.equal(dev_set[0], p0)
    for k, x, y in zip("pmv", dev_set, host_set):
        assert same_bits(x, y), "%s differs from the host-value entry point on %s" % (k, lid(layout))


def head_case(seed):
    """Conv features [3, 1, 2, 1024] (post-ReLU), lengths, image features [3, 64] and labels for small_encoder(True, 64)."""
    g = torch.Generator().manual_seed(4400 + seed)
    return (torch.randn(3, 1, 2, 1024, generator=g).abs() * 0.5, [2, 2, 1], torch.randn(3, 64, generator=g),
            torch.tensor([0, 1, 0]))


def head_trainer(gpu, **kw):
    from speech_to_image_translation_without_text_amd.encoder_train import HeadTrainer
    return HeadTrainer(encoder_ref.small_encoder(True, 64).to(gpu), weight_decay=G.TEST_WD, **kw)


def head_step(tr, case, gpu):
    feat, lens, image, label = case
    return tr.step_features(feat.to(gpu), lens, image, label)


def flat_state(tr):
    torch.cuda.synchronize()
    f = tr.flat
    return [f.p.clone(), f.m.clone(), f.v.clone(), f.step_dev.clone()]


def states_equal(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def test_a_clip_that_never_bites_is_the_run_without_the_option(gpu):
    plain, clipped, guarded = head_trainer(gpu, fused_adam=True), head_trainer(gpu, clip_grad=1e30), head_trainer(gpu, skip_nonfinite=True)
    assert plain.flat.clip is None and clipped.flat is not None and guarded.flat is not None and not plain.guarded
    for k in range(3):
        losses = [head_step(tr, head_case(k), gpu) for tr in (plain, clipped, guarded)]
        assert all(same_bits(losses[0]["loss"], l["loss"]) for l in losses[1:])
    ref = flat_state(plain)
    assert plain.flat.clip is None, "the off path built the clip state"
    assert not torch.equal(ref[0], head_trainer(gpu, fused_adam=True).flat.p) and int(ref[3]) == 3
    assert states_equal(ref, flat_state(clipped)) and states_equal(ref, flat_state(guarded))
    st = clipped.grad_stats()
    print("norms of the last step: %.6g, coef %.3g; per tensor %s" % (st["norm"], st["coef"], st["tensor_norms"]))
    assert (st["updates"], st["clipped"], st["skipped"]) == (3, 0, 0) and st["coef"] == 1.0 and plain.grad_stats() is None
    assert sorted(st["tensor_norms"]) == sorted(n for n, _ in clipped.model.named_parameters() if n.startswith("RNN."))
    assert clipped.flat.sync_step_count() == 3 == clipped.updates == clipped.steps


# ---- 4. the update against fp64 ------------------------------------------------------------------------------------------------
_UPDATE_REF = {}


def update_ref(sizes, wd, grads_key=None, grads=None):
    key = (tuple(sizes), wd, grads_key)
    if key not in _UPDATE_REF:
        _UPDATE_REF[key] = G.update_ref(sizes, torch.float64, wd, grads=grads)
    return _UPDATE_REF[key]


def run_guarded(gpu, sizes, wd, grads, max_norm):
    """Guarded steps on the layout's flat buffers from zero moments -> (p, m, v, step_dev, stats per step, L, snapshots)."""
    from speech_to_image_translation_without_text_amd import ops
    a = G.ADAM
    ps, _ = G.update_case(sizes)
    L = glayout(sizes, gpu)
    p = G.flatten([t.float() for t in ps], sizes).to(gpu)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step_dev = torch.zeros(1, dtype=torch.int32, device=gpu)
    stats, snaps = [], []
    for gs in grads:
        g = G.flatten([t.float() for t in gs], sizes).to(gpu)
        ops.grad_sumsq(g, L)
        ops.grad_clip_scale(L, G.GSCALE, max_norm, step_dev)
        if wd:
            ops.adam_l2_step_dev(p, g, m, v, a["lr"], a["b1"], a["b2"], a["eps"], wd, step_dev, L.scale, L.apply)
        else:
            ops.adam_step_dev(p, g, m, v, a["lr"], a["b1"], a["b2"], a["eps"], step_dev, L.scale, L.apply)
        stats.append(L.read_stats())
        snaps.append([p.clone(), m.clone(), v.clone(), step_dev.clone()])
    return p, m, v, step_dev, stats, L, snaps


@pytest.mark.parametrize("wd", [G.TEST_WD, 0.0], ids=["l2", "plain"])
@pytest.mark.parametrize("layout", G.UPDATE_LAYOUTS, ids=lid)
def test_three_clipped_steps_follow_the_fp64_restatement(gpu, layout, wd):
    ref = update_ref(layout, wd)
    _, grads = G.update_case(layout)
    p, m, v, step_dev, stats, L, _ = run_guarded(gpu, layout, wd, grads, G.case_max_norm(layout))
    assert int(step_dev) == G.STEPS == ref[3] and all(s["coef"] < 1.0 for s in stats) and stats[-1]["clipped"] == G.STEPS
    for s, info in zip(stats, ref[4]):
        assert abs(s["scale"] - info["scale"]) <= G.ulp32(info["scale"])
    errs = G.buffer_errs((p.cpu(), m.cpu(), v.cpu()), ref[:3], layout)
    for k, e in errs.items():
        print("%s wd %g %s: %.3e (bound %.2e)" % (lid(layout), wd, k, e, G.CLIP_BOUNDS[k]))
    bad = ["%s %.3e > %.2e" % (k, e, G.CLIP_BOUNDS[k]) for k, e in errs.items() if not e <= G.CLIP_BOUNDS[k]]
    assert not bad, "; ".join(bad)
    offsets, total = G.layout(layout)
    pad = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offsets, layout):
        pad[o:o + n] = False
    assert float(m.cpu()[pad].abs().sum()) == 0.0 and float(v.cpu()[pad].abs().sum()) == 0.0      # zero padding stays zero


# ---- 5. the skip ---------------------------------------------------------------------------------------------------------------
SKIP_PLACES = [([C], 0, 0), ([C], 0, C - 1), ([C + 6], 0, C + 5), ([5], 0, 4), (G.MULTI, 3, 4096), (G.MULTI, 4, 6),
               (G.MULTI, 0, 0)]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("place", SKIP_PLACES, ids=lambda p: "%s@%d.%d" % (lid(p[0]), p[1], p[2]))
def test_a_non_finite_gradient_is_skipped_and_the_next_step_counts_on(gpu, place, bad):
    sizes, tensor, index = place
    _, grads = G.update_case(sizes)
    grads = [[g.clone() for g in gs] for gs in grads]
    grads[1][tensor][index] = bad
    p, m, v, step_dev, stats, L, snaps = run_guarded(gpu, sizes, G.TEST_WD, grads, G.case_max_norm(sizes))
    assert [s["apply"] for s in stats] == [1, 0, 1]
    assert states_equal(snaps[0], snaps[1]), "the skipped step changed p, m, v or the step counter"
    assert not same_bits(snaps[1][0], snaps[2][0])
    assert (stats[1]["skipped"], stats[1]["updates"]) == (1, 1) and (stats[2]["skipped"], stats[2]["updates"]) == (1, 2)
    assert int(step_dev) == 2
    ref = G.update_ref(sizes, torch.float64, G.TEST_WD, grads=grads)
    assert ref[3] == 2
    errs = G.buffer_errs((p.cpu(), m.cpu(), v.cpu()), ref[:3], sizes)
    for k, e in errs.items():
        print("%s bad %s at tensor %d element %d, after the next step %s: %.3e (bound %.2e)"
              % (lid(sizes), bad, tensor, index, k, e, G.CLIP_BOUNDS[k]))
    assert all(e <= G.CLIP_BOUNDS[k] for k, e in errs.items()), errs


@pytest.mark.parametrize("layout", [[5], [C + 6], G.MULTI], ids=lid)
def test_squares_that_overflow_fp32_but_are_finite_are_not_skipped(gpu, layout):
    from speech_to_image_translation_without_text_amd import ops
    L = glayout(layout, gpu)
    g = torch.nan_to_num(G.flat_case(layout, "huge"), nan=0.0).to(gpu)
    assert math.isinf(float((g * g).sum()))
    p = flat_params(layout, gpu)
    p0, m, v = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    step_dev = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.grad_sumsq(g, L)
    ops.grad_clip_scale(L, 1.0, 1.0, step_dev)
    ops.adam_l2_step_dev(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, G.TEST_WD, step_dev, L.scale, L.apply)
    st = L.read_stats()
    ref = math.sqrt(sum(layout)) * float(torch.tensor(1e25, dtype=torch.float32))
    print("norm %.6g (ref %.6g), coef %.3g, apply %d" % (st["norm"], ref, st["coef"], st["apply"]))
    assert st["apply"] == 1 and st["skipped"] == 0 and int(step_dev) == 1 and abs(st["norm"] - ref) <= 1e-12 * ref
    offsets, _ = G.layout(layout)
    for o, n in zip(offsets, layout):
        assert bool((p[o:o + n] != p0[o:o + n]).all()) and bool(torch.isfinite(p[o:o + n]).all())
        assert bool(torch.isfinite(m[o:o + n]).all()) and bool(torch.isfinite(v[o:o + n]).all())


# ---- 6. the trainers -----------------------------------------------------------------------------------------------------------
def test_accumulation_sums_the_micro_batches_bit_for_bit(gpu):
    a, b = head_case(10), head_case(11)
    one, two = head_trainer(gpu, fused_adam=True), head_trainer(gpu, fused_adam=True)
    head_step(one, a, gpu)
    head_step(two, b, gpu)
    torch.cuda.synchronize()
    g_a, g_b = one.flat.g.clone(), two.flat.g.clone()
    assert float(g_a.abs().sum()) > 0 and not torch.equal(g_a, g_b)
    acc = head_trainer(gpu, accum=2)
    assert acc.flat is not None and not acc.guarded
    start = flat_state(acc)
    head_step(acc, a, gpu)
    assert (acc.steps, acc.updates, acc.pending) == (1, 0, 1) and states_equal(start, flat_state(acc))
    head_step(acc, b, gpu)
    assert (acc.steps, acc.updates, acc.pending) == (2, 1, 0)
    assert same_bits(acc.flat.g, g_a + g_b), "the flat gradient buffer is not g_a + g_b"
    manual = head_trainer(gpu, fused_adam=True)
    manual.flat.g.copy_(g_a + g_b)
    manual.flat.adam(0.5)
    assert states_equal(flat_state(manual), flat_state(acc)), "the update is not the fused step on the sum with gscale 0.5"
    assert not states_equal(start, flat_state(acc))
    # with the clip on top: the norm is that of (g_a + g_b) / 2
    clipped = head_trainer(gpu, accum=2, clip_grad=1e30)
    head_step(clipped, a, gpu)
    head_step(clipped, b, gpu)
    assert states_equal(flat_state(manual), flat_state(clipped))
    ref = G.exact_norms((g_a + g_b).cpu(), clipped.flat.sizes, 0.5)[0]
    got = clipped.grad_stats()["norm"]
    print("norm of the accumulated gradient: %.17g, exact %.17g" % (got, ref))
    assert abs(got - ref) <= G.norm_bound(sum(clipped.flat.sizes)) * ref


def test_an_incomplete_group_flushed_by_end_epoch_is_a_plain_step(gpu):
    a = head_case(10)
    plain, acc = head_trainer(gpu, fused_adam=True), head_trainer(gpu, accum=2)
    head_step(plain, a, gpu)
    plain.end_epoch()
    head_step(acc, a, gpu)
    assert acc.pending == 1
    with pytest.raises(ValueError, match="pending"):
        acc.state_dict()
    acc.end_epoch()
    assert (acc.pending, acc.updates, acc.steps, acc.epoch) == (0, 1, 1, 1)
    assert states_equal(flat_state(plain), flat_state(acc))
    acc.end_epoch()                                  # nothing pending: no further step
    assert states_equal(flat_state(plain), flat_state(acc)) and acc.updates == 1


def test_a_skipped_update_is_counted_and_the_state_resumes_bit_for_bit(gpu):
    from test_encoder_resume_gpu import first_difference
    cases = [head_case(20 + k) for k in range(4)]
    cases[1][2][1, 5] = float("inf")                                 # image_feature of the second update
    straight = head_trainer(gpu, skip_nonfinite=True, clip_grad=1.0)
    state = None
    for k, case in enumerate(cases):
        before = flat_state(straight)
        head_step(straight, case, gpu)
        if k == 1:
            assert states_equal(before, flat_state(straight)), "the update with an inf was not skipped"
            st = straight.grad_stats()
            assert (st["skipped"], st["updates"], st["apply"]) == (1, 1, 0)
        else:
            assert not states_equal(before, flat_state(straight))
        if k == 2:
            state = straight.state_dict()
    assert (state["steps"], state["updates"], state["skipped"]) == (3, 3, 1)
    assert {float(e["step"]) for e in state["optimizer"]["state"].values()} == {2.0}
    resumed = head_trainer(gpu, skip_nonfinite=True, clip_grad=1.0)
    resumed.load_state_dict(copy.deepcopy(state))
    assert (resumed.steps, resumed.updates, int(resumed.flat.step_dev)) == (3, 3, 2)
    # a state written before the resumed trainer's first guarded step keeps the cumulative count
    assert resumed.flat.clip is None and first_difference(resumed.state_dict(), state) is None
    head_step(resumed, cases[3], gpu)
    assert states_equal(flat_state(straight), flat_state(resumed))
    a, b = straight.state_dict(), resumed.state_dict()
    assert (a["updates"], a["skipped"], float(a["optimizer"]["state"][0]["step"])) == (4, 1, 3.0)
    assert first_difference(a, b) is None, first_difference(a, b)
    # the state loads into the unfused trainer as before
    from speech_to_image_translation_without_text_amd.encoder_train import HeadTrainer
    HeadTrainer(encoder_ref.small_encoder(True, 64).to(gpu), weight_decay=G.TEST_WD).load_state_dict(copy.deepcopy(state))


def test_encoder_trainer_clipped_step_follows_the_fp64_trajectory(gpu):
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer
    net = R.stack_net(bidirectional=True, nhidden=512)
    mel, lens, image, label = R.trainer_case(B=3)
    max_norm = ENCODER_MAX_NORM
    _, ref_state, norms = G.clipped_trajectory(net, mel, lens, image, label, 1, torch.float64, max_norm, **R.TRAINER_LOSS)
    assert norms[0] > 2 * max_norm
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    model = copy.deepcopy(net).to(gpu)
    tr = EncoderTrainer(model, clip_grad=max_norm, **R.TRAINER_LOSS)
    assert tr.flat is not None and tr.guarded
    tr.step(mel.float().contiguous().to(gpu), lens, image.float(), label)
    st = tr.grad_stats()
    after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    e = D.update_err(after, ref_state, start, list(start))
    bound = D.TRAJ_BOUNDS["traj_update"]
    print("gradient norm %.6g (fp64 trajectory %.6g), coef %.4g (fp64 %.4g); parameters, update_err %.3e (bound %.2e)"
          % (st["norm"], norms[0], st["coef"], G.clip_coef(norms[0], max_norm), e, bound))
    assert st["coef"] < 1.0 and (st["updates"], st["clipped"], st["skipped"]) == (1, 1, 0) and len(st["tensor_norms"]) == len(start)
    assert e <= bound


# the fp64 gradient norm of the one step of trainer_case(B=3) is 281.5
ENCODER_MAX_NORM = 100.0
# the data-parallel case runs at the trainers' default weight decay: at encoder_dp_ref.TEST_WD the first clipped step is
# decided by the decay term and the second step's gradient norm falls to 0.05, below any max_norm that still leaves the
# first step a gradient; at 1e-5 the fp64 norms are 244.2 and 47.8
DP_MAX_NORM = 2.0
DP_WD = 1e-5


# ---- 7. two gloo ranks on one GPU ----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn(fn, args, nprocs):
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + PROCESS_LIMIT
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a spawned rank ran past %d s" % PROCESS_LIMIT)


def _two_rank_worker(rank, world, port, out_dir, max_norm, wd):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import struct
    import encoder_conv_train_ref as R
    import encoder_dp_ref as D
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gpu = torch.device("cuda:0")
        torch.cuda.set_device(0)
        model = copy.deepcopy(R.stack_net(bidirectional=True, nhidden=512)).to(gpu)
        tr = EncoderTrainer(model, weight_decay=wd, distributed=True, clip_grad=max_norm, **R.TRAINER_LOSS)
        mel, lens, image, label = D.dp_case(rank)
        mel_d = mel.float().to(gpu)
        scales = []
        for _ in range(D.DP_STEPS):
            tr.step(mel_d, lens, image.float(), label)
            st = tr.grad_stats()
            scales.append([struct.unpack("<q", struct.pack("<d", st[k]))[0] for k in ("scale", "norm", "coef")] + [st["apply"]])
        torch.cuda.synchronize()
        mine = torch.tensor(scales, dtype=torch.int64)
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(gathered, mine)
        assert all(torch.equal(gathered[0], t) for t in gathered), "the ranks clipped by different coefficients"
        state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        stats = tr.grad_stats()
        # an inf on rank 1 alone reaches rank 0 through the sum: both skip
        before = [tr.flat.p.clone(), tr.flat.m.clone(), tr.flat.v.clone(), tr.flat.step_dev.clone()]
        bad = image.float().clone()
        if rank == 1:
            bad[0, 0] = float("inf")
        tr.step(mel_d, lens, bad, label)
        torch.cuda.synchronize()
        after = [tr.flat.p, tr.flat.m, tr.flat.v, tr.flat.step_dev]
        st = tr.grad_stats()
        assert st["apply"] == 0 and st["skipped"] == 1 and st["updates"] == D.DP_STEPS, (rank, st)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after)), "rank %d stepped" % rank
        assert tr.flat.sync_step_count() == D.DP_STEPS and tr.updates == D.DP_STEPS + 1
        if rank == 0:
            torch.save({"state": state, "norm": stats["norm"], "coef": stats["coef"], "scale": stats["scale"],
                        "clipped": stats["clipped"]}, os.path.join(out_dir, "rank0.pt"))
        with open(os.path.join(out_dir, "ok%d" % rank), "w") as fh:
            fh.write("ok")
    finally:
        torch.distributed.destroy_process_group()


def test_two_gloo_ranks_clip_alike_and_skip_together(gpu, tmp_path):
    world = D.DP_WORLD
    spawn(_two_rank_worker, (world, _free_port(), str(tmp_path), DP_MAX_NORM, DP_WD), world)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))
    out = torch.load(str(tmp_path / "rank0.pt"), map_location="cpu", weights_only=True)
    net = R.stack_net(bidirectional=True, nhidden=512)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    ref, infos = G.dp_clipped_steps(net, [D.dp_case(r) for r in range(world)], D.DP_STEPS, torch.float64, DP_MAX_NORM,
                                    wd=DP_WD, **R.TRAINER_LOSS)
    assert all(i["coef"] < 1.0 for i in infos) and out["clipped"] == D.DP_STEPS and out["coef"] < 1.0
    e = D.update_err(out["state"], ref, start, list(start))
    bound = D.TRAJ_BOUNDS["dp_update"]
    print("last step: norm %.6g (fp64 %.6g), scale %.6g (fp64 %.6g); rank 0's parameters, update_err %.3e (bound %.2e)"
          % (out["norm"], infos[-1]["norm"], out["scale"], infos[-1]["scale"], e, bound))
    assert e <= bound


# ---- 8. the CLI ----------------------------------------------------------------------------------------------------------------
CLIPS = [1.0, 1.25, 0.3, 1.5]
GNORM = re.compile(r"^epoch (\d+): loss -?\d+\.\d{4}, batch accu \d+\.\d{2}, gnorm mean/max \S+/\S+, clipped (\d+)/(\d+), skipped (\d+)$")
PLAIN = re.compile(r"^epoch (\d+): loss -?\d+\.\d{4}, batch accu \d+\.\d{2}$")


def _epoch_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("epoch ")]


def test_cli_clips_accumulates_and_resumes(gpu, tmp_path, capsys):
    from test_encoder_resume_gpu import first_difference
    from speech_to_image_translation_without_text_amd import train_encoder_head
    root = str(tmp_path)
    make_tree(root, "train", [CLIPS[k:] + CLIPS[:k] for k in range(4)] + [[1.1, 0.9]], seed=1)      # five items: three batches
    make_tree(root, "test", [CLIPS[k:] + CLIPS[:k] for k in range(2)], seed=2)
    start = os.path.join(root, "start.pt")
    torch.save({"state_dict": encoder_ref.build_encoder().state_dict()}, start)
    common = ["--model", start, "--dataset", "birds", "--data_dir", root, "--batch_size", "2", "--bidirectional", "--jel_flag",
              "--seed", "3", "--state_every", "1"]
    flags = ["--clip_grad", "1", "--accum", "2", "--skip_nonfinite"]
    out_s, out_r, out_p = (os.path.join(root, d) for d in ("straight", "stopped", "plain"))
    train_encoder_head.main(common + flags + ["--output_dir", out_s, "--epoch", "2"])
    straight = _epoch_lines(capsys.readouterr().out)
    assert len(straight) == 2 and all(GNORM.match(ln) for ln in straight), straight
    # three batches an epoch at --accum 2: one full group and one flushed by the epoch's end
    assert [GNORM.match(ln).groups()[2:] for ln in straight] == [("2", "0"), ("2", "0")]
    st = torch.load(os.path.join(out_s, "state.pth"), map_location="cpu", weights_only=True)
    assert st["meta"]["epoch"] == 2 and (st["meta"]["steps"], st["meta"]["updates"], st["meta"]["skipped"]) == (6, 4, 0)
    assert {float(e["step"]) for e in st["optimizer"]["state"].values()} == {4.0}
    train_encoder_head.main(common + flags + ["--output_dir", out_r, "--epoch", "1"])
    leg1 = _epoch_lines(capsys.readouterr().out)
    assert leg1 == straight[:1]
    train_encoder_head.main(common + flags + ["--output_dir", out_r, "--epoch", "2", "--resume", os.path.join(out_r, "state.pth")])
    leg2 = _epoch_lines(capsys.readouterr().out)
    assert leg2 == straight[1:], (leg2, straight)
    end = torch.load(os.path.join(out_r, "state.pth"), map_location="cpu", weights_only=True)
    assert first_difference(st, end) is None, first_difference(st, end)
    # without the flags: the lines and the state's fields of before
    train_encoder_head.main(common + ["--output_dir", out_p, "--epoch", "1"])
    plain = _epoch_lines(capsys.readouterr().out)
    assert len(plain) == 1 and PLAIN.match(plain[0]), plain
    sp = torch.load(os.path.join(out_p, "state.pth"), map_location="cpu", weights_only=True)
    assert sp["meta"] == {"epoch": 1, "best_accu": sp["meta"]["best_accu"]} and set(sp["meta"]) == {"epoch", "best_accu"}
    assert {float(e["step"]) for e in sp["optimizer"]["state"].values()} == {3.0}
    print("\n".join(straight + plain))
