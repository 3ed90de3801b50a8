"""The finishing passes behind the fp32 matrix kernels, at the smallest shapes that reach each of their branches and tails:
the split-K reductions of the forward convolution (launch_splitk_reduce, csrc/s2i_conv_fwd.hip) and the slab sums and the
OIHW transpose of the weight gradient (the tail of launch_wgrad, csrc/s2i_wgrad.hip).

Split-K forward.  After a launch the workspace still holds the S slabs the matrix kernel wrote, so the reduction has a
true reference: y must equal ((slab0 + slab1) + slab2) ... bit for bit, summed here in torch in fp32 (an elementwise fp32
add is exact in both); the plain reduction starts from 0, adds the bias and applies LeakyReLU the same way.  The partial
sums are held against fp64 sums of the fp64 convolution at conv_replay.GAMMA_STATS x the replay's denominators, and must be
bit-equal from run to run.  Power: y differs from the sums without the last slab, and the partial-sum bound rejects the
statistics of the convolution less its last slab.
  * statistics: [24,4,4,128] -> 136 (M = 384, Q = 34 quads: two blocks of 32 quads, the second with 2; 4 row lanes per
    quad; groups 1 and 3), [23,4,4,128] -> 136 (the last row chunk short), [72,4,4,64] -> 512 (2 row lanes per quad, row
    chunks of 8 rows: the 32-quad blocks), [17,32,32,64] -> 136 (M = 17408 in 512 chunks of 34 rows: the 16-quad blocks,
    a full turn of 32 rows and one of 2), [24,4,4,128] -> 40 (at most 16 quads: the narrow kernel), and bf16 output
    through s2i_conv_forward_dt.
  * without statistics: N = 6 (scalar kernel) and N = 8, 136 (16-byte kernel), with bias and LeakyReLU, ldy = N + 8 into
    a guarded buffer whose other columns must keep their fill, and [24,16,16,64] -> 520 (M = 6144: 798 720 quads against
    the 524 288 one pass of the grid holds, so threads take a second turn at a carried (row, column) that wraps).

Weight gradients, through conv_replay.replay_wgrad (fp64, GAMMA["fp32/wgrad"], the written slice only, the dropped-image
and dropped-channel mutants) with the wrong references of conv_edges.wgrad_mutants, "the last pixel split not summed" (one
slab dropped) among them; each record is then launched twice more on the same operands and must give the same bits.
  * [8,64,64,32] x [8,64,64,32] 3x3: 256 slabs of a 9 x 32 x 32 gradient, the tree sum and RT = 1
  * 1, 3 and 6 slabs of a 136 x 72 x 3 x 3 layer (summed by the finish itself, then twice behind slab_sum_kernel; a
    32-column tail: 136 = 4 x 32 + 8)
  * the up layer with 2 and 5 slabs (swap + fold, 16 taps in the tile, 72 input channels = 2 x 32 + 8), a 4 x 4 layer
    with 2 slabs (16 parameter taps, RT = 1, 40 input channels), a 1 x 1 layer (RT = 4)
  * accumulation into a slice [8, 8 + I) of a prefilled tensor
"""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_edges as E  # noqa: E402
import conv_replay as C  # noqa: E402
import launch_harness as LH  # noqa: E402
import launch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LEDGER = LH.Ledger()
ACT_LRELU = 2


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("reduction tails")


def _fwd_rec(B, H, Cx, N, *, stats, groups=1, bias=False, act=0):
    rec = E.fwd("k3s1", B, H, Cx, N, "reduce tails", [], stats=stats, groups=groups)
    rec.update(bias=N if bias else 0, act=act)
    return rec


def _run_fwd(gpu, rec, *, y16=False, ldy=None):
    """One forward launch of record rec on drawn operands.  Returns dict(y [M, N] as stored, part, nparts, slabs [S, M, N]
    (a copy of the workspace), plan, M, S and the operands x, w (OIHW), bias)."""
    from speech_to_image_translation_without_text_amd import _lib, ops
    lib = _lib.load()
    gen = LH.gen_rec(gpu, rec)
    op, layer = R.layer_op(rec)
    x = C._operand(rec["x"], gen, gpu)
    w = LH.dyadic(rec["w"]["oihw"], gen, gpu)
    packed = ops.pack_weight(w, R.pack_mode(op, layer))
    N = rec["N"]
    bias = torch.randn((N,), generator=gen, device=gpu) if rec["bias"] else None
    d = E.conv_desc(rec, **({} if ldy is None else dict(ldy=ldy)))
    plan = _lib.conv_plan(d, _lib.DT_F32, _lib.DT_BF16 if y16 else _lib.DT_F32, 0, bias is not None, False)
    assert plan is not None, lib.s2i_last_error()
    M, S = plan["M"], plan["splitk"]
    assert S > 1 and plan["kernel"].startswith("f32-"), plan
    assert plan["reduce"] == (_lib.FWD_REDUCE_STATS if rec["stats"] else _lib.FWD_REDUCE_PLAIN), plan
    out = dict(plan=plan, M=M, S=S, x=x, w=w, bias=bias)
    if not y16 and ldy is None:
        y, part, nparts = ops.conv_raw(rec["kind"], x, None, packed, N, wR=rec["wR"], ldw=rec["ldw"], bias=bias, act=rec["act"],
                                       stats=rec["stats"], groups=rec["groups"])
        ws = ops._ws.get(plan["ws_bytes"], gpu)
        torch.cuda.synchronize()
        out.update(y=y.view(M, N), part=part, nparts=nparts)
    else:
        ld = N if ldy is None else ldy
        esz = 2 if y16 else 4
        ybuf = torch.full((2 * LH.GUARD_BYTES + M * ld * esz,), LH.GUARD_BYTE, dtype=torch.uint8, device=gpu)
        nparts = lib.s2i_conv_stat_parts(ctypes.byref(d)) if rec["stats"] else 0
        part = torch.empty((2, nparts, N), device=gpu) if rec["stats"] else None
        ws = torch.empty(plan["ws_bytes"] // 4 + 64, device=gpu)
        rc = lib.s2i_conv_forward_dt(ctypes.byref(d), x.data_ptr(), _lib.DT_F32, None, packed.data_ptr(), LH.P(bias), None,
                                     ybuf.data_ptr() + LH.GUARD_BYTES, _lib.DT_BF16 if y16 else _lib.DT_F32, LH.P(part),
                                     ws.data_ptr(), ws.numel() * 4, _lib.stream())
        assert rc == 0, lib.s2i_last_error()
        torch.cuda.synchronize()
        inner = ybuf[LH.GUARD_BYTES:LH.GUARD_BYTES + M * ld * esz]
        out.update(ybuf=ybuf, yfull=inner.view(torch.bfloat16 if y16 else torch.float32).view(M, ld), part=part, nparts=nparts)
        out["y"] = out["yfull"][:, :N]
    out["slabs"] = ws[:S * M * N].view(S, M, N).clone()
    return out


def _slab_sum(slabs, upto, from_zero):
    v = torch.zeros_like(slabs[0]) + slabs[0] if from_zero else slabs[0].clone()
    for s in range(1, upto):
        v = v + slabs[s]
    return v


def _finish(v, bias, act):
    if bias is not None:
        v = v + bias
    if act == ACT_LRELU:
        v = torch.where(v > 0, v, v * 0.2)
    return v


def _check_stats(rec, r, what):
    """part against the fp64 statistics of the fp64 convolution, as conv_replay.replay_conv does; the mutant is the
    convolution less what the last slab holds."""
    N, G, M = rec["N"], max(rec["groups"], 1), r["M"]
    B = rec["x"][0][0]
    op, layer = R.layer_op(rec)
    xd, Wd = LH.nchw(r["x"].double()), r["w"].double()
    Op = rec["w"]["packed"][2]
    pre, _ = C.conv_ref(rec, op, layer, xd, None, Wd, Op, None, None)
    absref, _ = C.conv_ref(rec, op, layer, xd.abs(), None, Wd.abs(), Op, None, None)
    got = r["part"].double().view(2, G, r["nparts"] // G, N).sum(2)
    den = torch.stack((R.group_stats(absref, G)[0], 2 * (absref * pre.abs()).reshape(G, B // G, N, -1).sum((1, 3))))
    ratio, ok = LH.compare(got, R.group_stats(pre, G), den, 0.0, C.GAMMA_STATS)
    LEDGER.note("stats", ratio, what, C.GAMMA_STATS)
    print("%s: stats ratio %.3e (gamma %.3e)" % (what, ratio, C.GAMMA_STATS))
    assert ok, "%s: partial sums off by %.3e x den > %.3e" % (what, ratio, C.GAMMA_STATS)
    last = LH.nchw(r["slabs"][-1].double().view(B, pre.shape[2], pre.shape[3], N))
    assert LH.fails(got, R.group_stats(pre - last, G), den, 0.0, C.GAMMA_STATS), "%s: the partial-sum bound cannot see a dropped slab" % what
    LEDGER.reject("stats: the last slab dropped")


STATS_CASES = [
    # B, H, Cx, N, groups, quads per block of the kernel the reduction takes (0: the narrow kernel)
    pytest.param(24, 4, 128, 136, 1, 32, id="M384-N136-g1"),
    pytest.param(24, 4, 128, 136, 3, 32, id="M384-N136-g3"),
    pytest.param(23, 4, 128, 136, 1, 32, id="M368-N136-ragged"),
    pytest.param(72, 4, 64, 512, 1, 32, id="M1152-N512-2lanes"),
    pytest.param(17, 32, 64, 136, 1, 16, id="M17408-N136-two-turns"),
    pytest.param(24, 4, 128, 40, 1, 0, id="M384-N40-narrow"),
]


@pytest.mark.parametrize("B,H,Cx,N,groups,qb", STATS_CASES)
def test_splitk_stats_y_is_the_slab_sum_and_part_holds_fp64(gpu, B, H, Cx, N, groups, qb):
    rec = _fwd_rec(B, H, Cx, N, stats=True, groups=groups)
    what = "stats B%d H%d C%d N%d g%d" % (B, H, Cx, N, groups)
    with torch.no_grad():
        r = _run_fwd(gpu, rec)
        again = _run_fwd(gpu, rec)
    rows_per_chunk = -(-(r["M"] // groups) // (r["nparts"] // groups))
    print("%s: %d slabs, %d parts, %d rows per chunk" % (what, r["S"], r["nparts"], rows_per_chunk))
    if qb == 32:
        assert N > 64 and rows_per_chunk <= 16, (N, rows_per_chunk)
    elif qb == 16:
        assert N > 64 and rows_per_chunk > 32 and rows_per_chunk % 32, (N, rows_per_chunk)
    else:
        assert N <= 64, N
    assert torch.equal(r["y"], _slab_sum(r["slabs"], r["S"], False)), "%s: y is not the sequential fp32 sum of the slabs" % what
    assert not torch.equal(r["y"], _slab_sum(r["slabs"], r["S"] - 1, False)), "%s: the last slab does not show in y" % what
    _check_stats(rec, r, what)
    assert torch.equal(r["slabs"], again["slabs"]), "%s: the slabs differ between two runs" % what
    assert torch.equal(r["part"], again["part"]) and torch.equal(r["y"], again["y"]), "%s: not bit-equal between two runs" % what


def test_splitk_stats_bf16_output(gpu):
    rec = _fwd_rec(24, 4, 128, 136, stats=True, groups=3)
    what = "stats bf16 out"
    with torch.no_grad():
        r = _run_fwd(gpu, rec, y16=True)
        again = _run_fwd(gpu, rec, y16=True)
    ysum = _slab_sum(r["slabs"], r["S"], False)
    assert torch.equal(r["y"].view(torch.int16), ysum.bfloat16().view(torch.int16)), "%s: y is not the rounded slab sum" % what
    assert not torch.equal(r["y"], _slab_sum(r["slabs"], r["S"] - 1, False).bfloat16())
    assert bool((r["ybuf"][:LH.GUARD_BYTES] == LH.GUARD_BYTE).all()) and bool((r["ybuf"][-LH.GUARD_BYTES:] == LH.GUARD_BYTE).all())
    _check_stats(rec, r, what)
    assert torch.equal(r["part"], again["part"]) and torch.equal(r["y"].view(torch.int16), again["y"].view(torch.int16))


SMALL = (24, 4, 128)       # B, H, Cx: M = 384
GRID_QUADS = 2048 * 256    # quads one pass of the 16-byte kernel's grid holds (launch_splitk_reduce)
PLAIN_CASES = [
    pytest.param(SMALL, 6, False, 0, None, id="N6-scalar"),
    pytest.param(SMALL, 6, True, ACT_LRELU, None, id="N6-scalar-bias-lrelu"),
    pytest.param(SMALL, 8, False, 0, None, id="N8"),
    pytest.param(SMALL, 136, True, ACT_LRELU, None, id="N136-bias-lrelu"),
    pytest.param(SMALL, 136, True, ACT_LRELU, 144, id="N136-bias-lrelu-ldy144"),
    pytest.param(SMALL, 6, True, 0, 14, id="N6-scalar-bias-ldy14"),
    pytest.param((24, 16, 64), 520, True, ACT_LRELU, None, id="M6144-N520-two-grid-passes"),
]


@pytest.mark.parametrize("shape,N,bias,act,ldy", PLAIN_CASES)
def test_splitk_plain_y_is_the_slab_sum(gpu, shape, N, bias, act, ldy):
    B, H, Cx = shape
    rec = _fwd_rec(B, H, Cx, N, stats=False, bias=bias, act=act)
    what = "plain N%d bias%d act%d ldy%s" % (N, bias, act, ldy)
    with torch.no_grad():
        r = _run_fwd(gpu, rec, ldy=ldy)
        again = _run_fwd(gpu, rec, ldy=ldy)
    if shape != SMALL:
        # the second pass starts in the middle of a row: the carried column wraps
        assert r["M"] * N // 4 > GRID_QUADS and (GRID_QUADS * 4) % N, (r["M"], N)
    want = _finish(_slab_sum(r["slabs"], r["S"], True), r["bias"], act)
    assert torch.equal(r["y"], want), "%s: y is not act(0 + slab0 + slab1 ... + bias) in fp32 (%d elements differ)" % (
        what, int((r["y"] != want).sum()))
    assert not torch.equal(r["y"], _finish(_slab_sum(r["slabs"], r["S"] - 1, True), r["bias"], act)), "%s: last slab unseen" % what
    assert torch.equal(r["y"], again["y"])
    if ldy is not None:
        fill = torch.full((1,), LH.GUARD_BYTE, dtype=torch.uint8, device=gpu)
        assert bool((r["yfull"][:, N:].contiguous().view(torch.uint8) == fill).all()), "%s: columns [N, ldy) were written" % what
        assert bool((r["ybuf"][:LH.GUARD_BYTES] == LH.GUARD_BYTE).all()) and bool((r["ybuf"][-LH.GUARD_BYTES:] == LH.GUARD_BYTE).all())
    # the fp64 convolution, at the replay's bound
    op, layer = R.layer_op(rec)
    xd, Wd = LH.nchw(r["x"].double()), r["w"].double()
    bd = None if r["bias"] is None else r["bias"].double()
    Op = rec["w"]["packed"][2]
    _, ref = C.conv_ref(rec, op, layer, xd, None, Wd, Op, None, bd)
    absref, _ = C.conv_ref(rec, op, layer, xd.abs(), None, Wd.abs(), Op, None, None)
    if bd is not None:
        absref = absref + R.pad_channels(bd.abs().view(1, -1, 1, 1), N)
    out = LH.nchw(r["y"].contiguous().double().view(B, H, H, N))
    ratio, ok = LH.compare(out, R.act(ref, act), absref, 0.0, C.GAMMA["fp32/conv"])
    LEDGER.note("fp32/conv", ratio, what, C.GAMMA["fp32/conv"])
    assert ok, "%s: element error %.3e x absref" % (what, ratio)


# ---- weight gradients ------------------------------------------------------------------------------------------------
def _wg(layer, B, H, Cin, N, finish, slabs, **kw):
    return (E.wgrad(layer, B, H, Cin, N, "reduce tails", [], **kw), finish, slabs)


WGRAD_CASES = [
    _wg("k3s1", 8, 64, 32, 32, "rt1-tree", 256),
    _wg("k3s1", 2, 8, 72, 136, "rt2-direct-ctail", 1),
    _wg("up", 4, 8, 72, 136, "rt2-direct-ctail-swap", 2),
    _wg("k3s1", 6, 8, 72, 136, "rt2-stream-ctail", 3),
    _wg("k3s1", 12, 8, 72, 136, "rt2-stream-ctail", 6),
    _wg("up", 11, 8, 72, 136, "rt2-stream-ctail-swap", 5),
    _wg("k4s2", 4, 16, 40, 72, "rt1-direct-ctail", 2),
    _wg("k1", 11, 8, 160, 128, "rt4-stream", 5),
    _wg("k3s1", 6, 8, 72, 136, "rt2-stream-ctail", 3, accumulate=True, i_off=8),
    _wg("k3s1", 8, 64, 32, 32, "rt1-tree", 256, accumulate=True, i_off=8),
]


def _wg_id(case):
    rec, finish, slabs = case
    return "%s-%s-S%d%s" % (E.record_id(0, rec)[4:], finish, slabs, "-acc-slice" if rec["accumulate"] else "")


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[_wg_id(c) for c in WGRAD_CASES])
def test_wgrad_finish_holds_fp64_and_repeats(gpu, case):
    from speech_to_image_translation_without_text_amd import ops
    rec, finish, slabs = case
    what = _wg_id(case)
    plan = E.wgrad_plan(rec)
    assert plan["slabs"] == slabs and E.FIN + finish in plan["reach"], (plan["slabs"], sorted(plan["reach"]))

    def extra(ctx):
        mutants = E.wgrad_mutants(rec, plan, ctx["a"], ctx["g"], ctx["dw"], ctx["true"])
        bad = [] if slabs == 1 or any(k.startswith("slabs:") for k in mutants) else ["no wrong reference with a slab dropped"]
        for name, m in mutants.items():
            if LH.fails(ctx["got"], ctx["base"] + m, ctx["absref"], ctx["rnd"], ctx["gamma"]):
                LEDGER.reject("wgrad: " + name)
            else:
                bad.append("the bound cannot see: " + name)
        return bad

    with torch.no_grad():
        C.replay_wgrad(rec, LH.gen_rec(gpu, rec), gpu, what, LEDGER, extra=extra)
        # twice more on one set of operands: the same bits, outside the slice too
        gen = LH.gen_rec(gpu, rec)
        a, g = C._operand(rec["a"], gen, gpu), C._operand(rec["g"], gen, gpu)
        gs = list(rec["grad_shape"])
        full = list(gs)
        if rec["I_total"]:
            full[1] = rec["I_total"]
        prefill = torch.randn(full, generator=gen, device=gpu) if rec["out"] else None
        runs = []
        for _ in range(2):
            out = None if prefill is None else prefill.clone()
            runs.append(ops.wgrad_raw(rec["kind"], a, None, g, tuple(gs), swap=rec["swap"], fold=rec["fold"], out=out,
                                      accumulate=rec["accumulate"], i_off=rec["i_off"], I_total=rec["I_total"]))
        torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]), "%s: two runs differ in %d elements" % (what, int((runs[0] != runs[1]).sum()))
