"""The convolution kernels at partial tiles and ragged batches, against the fp64 reference of the launch-replay suites.

tests/test_step_launches_gpu.py replays every launch of the train step at its production shape; there every GEMM is a
whole number of row tiles, pixel chunks and bf16 image tiles (tests/test_conv_edges_cpu.py asserts that).  This module
points the same replay (conv_replay.replay_conv / replay_wgrad), the same element-wise bound gamma x absref and the
unchanged constants conv_replay.GAMMA / GAMMA_STATS at the shapes where tile kernels go wrong:

  * the hand-written table tests/conv_edges.py: partly filled row tiles under 96- and 128-row tiles and under the
    128 x 64 / 128 x 32 tiles, single partial tiles, column and K tails, short last K splits, tails in the 4 phases of the
    transposed convolution, grouped statistics on 96-row groups, weight-gradient pixel tails per tile shape, ragged image
    tiles of both bf16 kernels, short bf16 weight-gradient stages.  A record that forces a tile height or a planner knob
    runs under it; every other record under the default planner.
  * power, besides the replay's dropped-channel and dropped-image mutants: with statistics, the partial-sum comparison
    must FAIL against reference sums without the last row (a tail row leaking into or dropping out of the sums); for a
    forward launch with a short last K split, the element comparison must FAIL against a reference without the (tap,
    channel) pairs of that last split.
  * the ragged production batch: the last batch of a CUB epoch has 23 images (8855 % 24 = 8855 % 48 = 23).  One eager
    train_step of each workload at B = 23 is recorded into tests/ragged_launches.json (regenerate it with
    `python tests/test_conv_edges_gpu.py`), must hold no stacked (groups = 3) launch -- the trainer runs three separate
    discriminator passes when B % 8 != 0 -- and every record whose GEMM has at most 23 x 32 x 32 rows per phase is
    replayed.  Larger maps at B = 23 differ from production by one 96-row tail on a large grid, which the table covers
    at small size.

Measured on one MI355X (worst ratio per class: edge table | ragged census | production worst recorded in
conv_replay.py; bound):

    fp32 forward / input gradient   3.3e-7 | 4.2e-7 | 4.8e-7   (2^-20 = 9.5e-7)
    fp32 weight gradient            2.8e-7 | 4.1e-7 | 4.0e-7   (8e-7)
    bf16 forward / input gradient   1.1e-9 | 3.4e-8 | 5.1e-8   (1e-7)
    bf16 weight gradient            1.4e-7 | 1.2e-7 | 1.6e-7   (3.2e-7)
    BatchNorm partial sums          1.1e-7 | 6.0e-8 | 7.4e-8   (1.5e-7)

No class needed a wider bound.  The partial sums' worst edge ratio is the fc layer at batch 5 (five rows per column: the
fp32 rounding of each row's value is not averaged out over many rows, as it is at M >= 384 in production).  73 table
records and 2 x 65 census records (2 x 42 left out by the row cap) replay in about 12 s; the last-row mutant was rejected
in all 70 replays with statistics, the dropped last K split in all 7 forward replays that have one.

The branches of the bf16 planner (plan_bf16) that no production shape takes
---------------------------------------------------------------------------
tests/conv_edges.py::_bf16_branches adds 52 records (rows 072 to 123), each the smallest shape that takes its branch;
tests/test_conv_edges_cpu.py derives the branch of every record from s2i_conv_bf16_plan_query / s2i_wgrad_plan_query,
asserts that every name of _lib.B16_KERNELS is replayed with forward and with input-gradient weights and every b16 name of
_lib.WGRAD_KERNELS once, and that no census record reaches the column tail, the split 256-pixel kernel or the class bias
on a tile of several images.  (Grouped statistics on tiles of several images the census does reach, in one form: 3 groups
of 48 images on the 128-pixel kernel.  The table adds 2 groups, the 256-pixel kernel and groups of one or two tiles.)
They run through the same replay, bounds unchanged; the extra hook adds one wrong reference per branch that the
comparison has to reject.  Measured on one MI355X, worst ratio of the records of a branch (elements, bound 1e-7 | partial
sums, bound 1.5e-7 | wrong references rejected):

    b16-coltail (N % BN != 0: 24 conv records, each of the 16 kernels)
                                  1.5e-9 | 6.0e-9 | last valid column zeroed 24 of 24; sums of the Npad columns shifted
                                                    by one 21 of 21
    b16-v2-split (256-pixel kernel, splitk > 1: 9 records, all four instantiations)
                                  7.1e-9 | 1.1e-9 | last channel chunk dropped 15 of 15 (every bf16 record with a split)
    b16-short-last-split (4 records on the 256-pixel kernels)
                                  7.1e-9 | 9.8e-10
    b16-cls-multi-image (class bias, tb = 2, 4, 8; 4 records, one unsplit only through nosplit)
                                  3.7e-10 | 1.0e-8 | bias row of the tile's first image for the whole tile 4 of 4
    b16-groups-multi-image (groups = 2, 3 on tb = 2, 4; split and unsplit; 5 records)
                                  1.6e-9 | 5.0e-9 | groups cut one image late 5 of 5
    b16-tb>1 (recorded for the two above)         1.6e-9 | 1.0e-8
    b16-wg-split-overwrite (2 records; b16-64x64 runs in 3)   5.2e-8 (bound 3.2e-7)

The ratios are far below the bound because the replay's weights are dyadic (exact in bf16): what is left is the fp32
accumulation order.  Wrong references accepted: 0 (test_no_wrong_reference_was_accepted).  One record
(conv_edges.NO_KERNEL) plans to no kernel (B16_NO_KERNEL: transposed conv, BN 64, 32-channel chunks) and is replayed
through the any-dtype fp32 kernel that ops.conv_any falls back to, bf16 in and out, under the bf16 bound: ratio 0, the
error stays inside the output rounding.

Ten of the records are also launched through s2i_conv_forward_bf16 itself (test_direct_call_*): ldy = N + 8, and y, the
partial sums and the slab workspace each between sentinels.  Columns [N, ldy), the rows behind the last one and every guard
byte came back bit-identical in all ten, elements at most 1.5e-9, partial sums 3.9e-9; ldy = N + 4 and a tile that
straddles two BatchNorm groups are refused with their message and nothing written.

No kernel was found wrong.  Deliberate mutation, tried once and reverted: the class-bias image index taken from the tile
(b0) instead of the pixel (b0 + tb), in both kernels.  The four class-bias replays failed (element error 0.05 to 0.16 x
absref) and nothing else did; the census replays cannot see it (one image per tile in every class-bias launch).

Wall time of this module on one MI355X: the 204 tests of the parent commit 11.5 s, all 269 tests 10.9 to 11.7 s (the
6 s census step dominates and varies more than the 65 new tests take together, under 2 s).

The branches of the weight-gradient planner (plan_wgrad) and the finishing paths of launch_wgrad
---------------------------------------------------------------------------------------------
tests/conv_edges.py::_wgrad_branches adds 34 records (rows 124 to 157), each the smallest shape that takes its branch.
tests/test_conv_edges_cpu.py derives every tag from s2i_wgrad_plan_query (the finish tag from conv_edges.wgrad_finish, the
one rule the query does not export), asserts that every name of _lib.WGRAD_KERNELS but f32in-128x128 is the plan of a
replayed record, and that no census record reaches what the rows add.  They run through the same replay, constants
unchanged; replay_wgrad takes the class from the kernel family (f32-* and rows3-* are "fp32/wgrad" whatever the operands'
storage) and leaves the fp32 operand of a mixed launch on an f32-* kernel its full significand.  The extra hook holds every
weight-gradient record of the table, old and new, against the wrong references of conv_edges.wgrad_mutants, one per branch
its plan takes; tests/test_conv_edges_cpu.py shows without a GPU that each lies outside the bound of the true gradient.
Measured on one MI355X, records of the whole table per tag | worst ratio (bound 8e-7):

    rows3-64x32 (5 records: W = 32 and 64, 1, 3 and 9 images, 8 / 24 / 96 / 231 slabs, accumulated into a slice)
                                          5 | 5.0e-8
    wg-rows3-odd-batch                   10 | 3.5e-8    (each of the five instantiations off the census batches)
    wg-rows3-coltail                      2 | 3.1e-8    (rows3-32x64 with gy = 2, rows3-64x128 with 96 of 128 columns)
    wg-short-last-split-rows3             1 | 7.6e-9
    wg-pixtail-128x32                     3 | 2.3e-7
    wg-short-last-split-128x32 / -96x64 / -96x32 / -256x128 / -256x256 / -128x128
                              1 / 1 / 1 / 1 / 1 / 3 | 6.4e-8 / 7.1e-8 / 7.8e-8 / 8.6e-8 / 1.0e-7 / 8.9e-8
    wg-16-on-f32-a / -g / -ag     3 / 3 / 4 | 2.7e-7 / 2.1e-7 / 1.2e-7
    wg-finish-rt4-direct / rt4-stream 1 / 1 | 2.2e-7 / 6.6e-8
    wg-finish-rt8-stream / rt8-stream-ctail / rt2-stream-ctail-swap / rt1-stream-ctail
                              1 / 1 / 1 / 1 | 1.0e-7 / 8.9e-8 / 3.7e-8 / 4.4e-8
    wg-finish-rt1-tree / rt1-tree-ctail (accumulated; into a slice)
                                      3 / 1 | 1.2e-8 / 1.3e-8
    b16-wg-recut-fewer-slabs              1 | 2.0e-8    (bound 3.2e-7)

The other finish tags (rt1 / rt2 / rt8 direct, rt1 / rt2 stream) are those of the rows that were there before, 2.3e-7 to
2.8e-7.  No record came near its class constant, so none needed explaining from a summation order.  Wrong references
rejected over the 66 weight-gradient records (accepted: 0): the pixels of the last chunk dropped 37 of 37, the last pixel
split not summed 28 of 28, the last valid column not written 15 of 15, input row 0 read as padding 11 of 11 and the first
pixel of a row's second chunk read as padding 2 of 2 (row-segment kernels), the fp32 operand rounded to bf16 on an f32-*
kernel 3 of 3 (g) and 3 of 3 (a), ky and kx exchanged in the folded gradient 4 of 4.

Nine of the rows are also launched through s2i_conv_wgrad / s2i_conv_wgrad_dt themselves (test_direct_wgrad_*): g with row
stride N + 8 and NaN in columns [N, ldg), the workspace of exactly s2i_wgrad_workspace_bytes(_dt) bytes and the OIHW tensor
each between guard bytes, the tensor prefilled where the record accumulates or slices.  Every guard byte came back
unchanged, the input channels outside the slice bit-identical, the fourth slab of the bf16 row whose 64-pixel re-cut fills
three of four unwritten, every result finite; worst ratio 1.0e-7 on the fp32 cores (f32-256x256) and 2.0e-8 on the bf16
cores, the same figures as the replays of these rows, whose operands they share.  A workspace one byte short and ldg < N
are refused with their message and nothing written.

No kernel was found wrong; rows3-64x32, which had never executed, holds 5.0e-8.  Deliberate mutation, tried once and
reverted: the channel half of aoff exchanged in the 64 x 32 instantiation of wgrad_k3_rows_kernel (in bounds).  The five
replays and the two direct calls that planned to rows3-64x32 failed (element error 0.04 to 0.20 x absref) and none of the
other 305 tests did (the third direct call of that kernel, into a slice, was added after the trial); before this change no
test of the repository ran that kernel.

Wall time of this module on one MI355X, parent commit and this one run alternately, four times: the parent's 269 tests
11.2 to 12.6 s, the tests of this one (312, then all 313) 11.2 to 12.1 s.  The 44 new tests take under 1 s together (the
largest, 9 x 64 x 64 x 64 floats, 0.04 s for its replay and 0.02 s for its direct call); the spread between two runs of
the same commit is larger.
"""
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
from helpers import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

CENSUS_FILE = os.path.join(HERE, "ragged_launches.json")

RAGGED_MODES = {
    "fp32_b23": (dict(CASES["full3_fwd"], B=23), False),
    "bf16_b23": (dict(CASES["full3_fwd"], B=23), True),
}
ROW_CAP = 23 * 32 * 32

EDGE_LEDGER = LH.Ledger()
RAGGED_LEDGER = LH.Ledger()
LEFT_OUT = {}
ACCEPTED = []            # wrong references a comparison let through: (record, mutation)
GUARD_ROWS = 4           # sentinel rows behind the last row of a directly launched output


@pytest.fixture(scope="module", autouse=True)
def _report():
    EDGE_LEDGER.start()
    RAGGED_LEDGER.start()
    yield
    EDGE_LEDGER.report("edge table replay")
    RAGGED_LEDGER.report("ragged batch (B = 23) launch replay")
    for mode, (kept, cut) in sorted(LEFT_OUT.items()):
        print("ragged census %s: %d records replayed, %d left out by the cap of %d rows per phase" % (mode, kept, cut, ROW_CAP))
    print("wrong references accepted: %d %s" % (len(ACCEPTED), ACCEPTED[:8]))


def _default_planner():
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0, "the replay runs the default planner"
    assert os.environ.get("S2I_TUNE", "") == "", "the replay runs the default planner"


# ---- power checks ----------------------------------------------------------------------------------------------------
def _edge_extra(ledger, what=""):
    def extra(ctx):
        rec, bad = ctx["rec"], []
        if ctx["stats"] is not None:
            cut = ctx["pre"].clone()
            cut[-1, :, -1, -1] = 0                       # the last pixel of the last image: the last row of the GEMM
            if LH.fails(ctx["stats"]["got"], R.group_stats(cut, ctx["stats"]["groups"]), ctx["stats"]["den"], 0.0, C.GAMMA_STATS):
                ledger.reject("stats: last row left out of the sums")
            else:
                bad.append("the partial-sum bound cannot see the last row")
        if "short-last-split" in rec.get("reach", ()) and ctx["op"] == "fwd" and ctx["layer"] != "up":
            plan = E.conv_plan(rec)
            Ca = rec["x"][0][3] + rec["cvec"]
            k0 = (plan["splitk"] - 1) * plan["cps"] * 32     # K runs tap-major, channel-minor, in 32-deep chunks
            W = ctx["W"].clone()
            Wv = W.view(W.shape[0], W.shape[1], -1)
            for k in range(k0, plan["K"]):
                Wv[:, k % Ca, k // Ca] = 0
            _, mref = C.conv_ref(rec, ctx["op"], ctx["layer"], ctx["x"], ctx["cvec"], W, ctx["Op"], ctx["table"], ctx["bias"])
            if LH.fails(ctx["out"], R.act(mref, rec["act"]), ctx["absref"], ctx["rnd"], ctx["gamma"]):
                ledger.reject("%s: last K split dropped" % ctx["cls"])
            else:
                bad.append("the bound cannot see the short last K split")
        if rec.get("fast") and "reach" in rec:
            _bf16_branch_power(ledger, ctx, what, bad)
        return bad
    return extra


def _bf16_branch_power(ledger, ctx, what, bad):
    """The branches of the bf16 plan (tests/conv_edges.py, _bf16_branches): the worst ratio per branch, and for each branch
    a wrong reference of the kind that branch would produce, which the comparison has to reject."""
    rec, N = ctx["rec"], ctx["rec"]["N"]
    plan = E.conv_plan(rec)
    reach = plan["reach"]
    st = ctx["stats"]
    sref = None if st is None else R.group_stats(ctx["pre"], st["groups"])
    for tag in sorted(reach):
        ledger.note("branch " + tag, ctx["ratio"], what, ctx["gamma"])
        if st is not None:
            ledger.note("branch " + tag + " (stats)", LH.compare(st["got"], sref, st["den"], 0.0, C.GAMMA_STATS)[0], what, C.GAMMA_STATS)

    def verdict(rejected, name):
        if rejected:
            ledger.reject("bf16 branch: " + name)
        else:
            ACCEPTED.append((what, name))
            bad.append("the bound cannot see: " + name)

    def element(mref, name):
        verdict(LH.fails(ctx["out"], R.act(mref, rec["act"]), ctx["absref"], ctx["rnd"], ctx["gamma"]), name)

    def reference(x=None, table=None):
        return C.conv_ref(rec, ctx["op"], ctx["layer"], ctx["x"] if x is None else x, ctx["cvec"], ctx["W"], ctx["Op"],
                          ctx["table"] if table is None else table, ctx["bias"])[1]

    if "b16-coltail" in reach:
        mref = ctx["ref"].clone()
        mref[:, N - 1] = 0
        element(mref, "column tail: the last valid column not written")
        if st is not None:
            wide = torch.zeros(sref.shape[:2] + (plan["npad"],), dtype=sref.dtype, device=sref.device)
            wide[..., :N] = sref
            verdict(LH.fails(st["got"], torch.roll(wide, 1, -1)[..., :N], st["den"], 0.0, C.GAMMA_STATS),
                    "column tail: statistics of the padded columns, one column off")
    if "b16-cls-multi-image" in reach:
        first = torch.arange(ctx["table"].shape[0], device=ctx["table"].device) // plan["tb"] * plan["tb"]
        element(reference(table=ctx["table"][first]), "class bias: the tile's first image for every image of the tile")
    if "b16-groups-multi-image" in reach:
        verdict(LH.fails(st["got"], R.group_stats(torch.roll(ctx["pre"], -1, 0), st["groups"]), st["den"], 0.0, C.GAMMA_STATS),
                "groups: cut one image late")
    if plan["splitk"] > 1:
        xm = ctx["x"].clone()
        xm[:, xm.shape[1] - plan["CK"]:] = 0         # the K loop runs channel chunk by channel chunk, all taps of a chunk
        element(reference(x=xm), "K split: the last channel chunk dropped")


# ---- the edge table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(E.RECORDS)), ids=[E.record_id(i, r) for i, r in enumerate(E.RECORDS)])
def test_edge_replay_matches_fp64(gpu, index):
    from speech_to_image_translation_without_text_amd import _lib, ops
    _default_planner()
    rec = E.RECORDS[index]
    what = E.record_id(index, rec)
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp, _lib.tuning(**rec["tune"]):
        mp.setattr(ops, "TILE_ROWS", rec["tile_rows"])
        if rec["fn"].startswith("conv"):
            C.replay_conv(rec, LH.gen_rec(gpu, rec), gpu, what, EDGE_LEDGER, extra=_edge_extra(EDGE_LEDGER, what))
        else:
            C.replay_wgrad(rec, LH.gen_rec(gpu, rec), gpu, what, EDGE_LEDGER, extra=_wgrad_extra(EDGE_LEDGER, what))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("index", range(len(E.NO_KERNEL)))
def test_plan_without_a_kernel_falls_back_and_holds_the_bf16_bound(gpu, index):
    """B16_NO_KERNEL: the replay asserts that the fast path was not taken; bf16 in, bf16 out, GAMMA["bf16/conv"]."""
    _default_planner()
    rec = E.NO_KERNEL[index]
    what = "no-kernel-%d-%s" % (index, E.record_id(index, rec))
    with torch.no_grad():
        C.replay_conv(rec, LH.gen_rec(gpu, rec), gpu, what, EDGE_LEDGER, cls="bf16/conv")
    torch.cuda.empty_cache()


def _wgrad_extra(ledger, what):
    """The worst ratio per branch tag of the record's plan, and the wrong references of conv_edges.wgrad_mutants (one per
    branch the plan takes), each of which the comparison has to reject."""
    def extra(ctx):
        rec, bad = ctx["rec"], []
        plan = E.wgrad_plan(rec)
        for tag in sorted(plan["reach"]):
            ledger.note("branch " + tag, ctx["ratio"], what, ctx["gamma"])
        for name, m in E.wgrad_mutants(rec, plan, ctx["a"], ctx["g"], ctx["dw"], ctx["true"]).items():
            if LH.fails(ctx["got"], ctx["base"] + m, ctx["absref"], ctx["rnd"], ctx["gamma"]):
                ledger.reject("wgrad branch: " + name)
            else:
                ACCEPTED.append((what, name))
                bad.append("the bound cannot see: " + name)
        return bad
    return extra


# ---- the bf16 entry point itself: a strided destination, every buffer between sentinels ---------------------------------
DIRECT = [i for i, r in enumerate(E.RECORDS) if r.get("direct") and "x" in r]


def _guarded(nbytes, dev):
    """(buffer, address of its nbytes in the middle): GUARD_BYTE throughout, GUARD_BYTES of margin on both sides."""
    buf = torch.full((2 * LH.GUARD_BYTES + nbytes,), LH.GUARD_BYTE, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + LH.GUARD_BYTES


def _inner(buf, nbytes, dtype):
    return buf[LH.GUARD_BYTES:LH.GUARD_BYTES + nbytes].view(dtype)


def _direct_operands(rec, gpu, ldy):
    """x, the bf16 weights of the descriptor with row stride ldy, the descriptor, its plan and the OIHW weight."""
    from speech_to_image_translation_without_text_amd import _lib, ops
    gen = LH.gen_rec(gpu, rec)
    op, layer = R.layer_op(rec)
    x = C._operand(rec["x"], gen, gpu)
    w = LH.dyadic(rec["w"]["oihw"], gen, gpu)
    packed = ops.pack_weight(w, R.pack_mode(op, layer))
    assert list(packed.shape) == rec["w"]["packed"]
    d = E.conv_desc(rec, ldy=ldy)
    plan = _lib.conv_bf16_plan(d)
    assert plan is not None and plan["kernel"] is not None, _lib.load().s2i_last_error()
    return x, ops.bf16_weight(packed, d, rec["w_offset"]), d, plan, w, packed


@pytest.mark.parametrize("index", DIRECT, ids=[E.record_id(i, E.RECORDS[i]) for i in DIRECT])
def test_direct_call_keeps_to_its_columns_rows_and_workspace(gpu, index):
    """s2i_conv_forward_bf16 with ldy = N + 8: columns [0, N) hold the convolution (fp64, the replay's bound), columns
    [N, ldy) of every row, the rows behind the last one and the bytes around y, around the 2 x parts x N partial sums and
    around the ws_bytes of slabs the plan query names are the sentinel they were filled with."""
    import ctypes
    from speech_to_image_translation_without_text_amd import _lib
    _default_planner()
    rec = E.RECORDS[index]
    what = "direct " + E.record_id(index, rec)
    assert not rec["cls_bias"] and not rec["bias"] and not rec["act"]
    N, G = rec["N"], max(rec["groups"], 1)
    ldy = N + 8
    op, layer = R.layer_op(rec)
    with torch.no_grad(), _lib.tuning(**rec["tune"]):
        x, wb, d, plan, w, packed = _direct_operands(rec, gpu, ldy)
        rows, parts, ws_bytes = plan["rows"], plan["parts"], plan["ws_bytes"]
        ybytes = (rows + GUARD_ROWS) * ldy * 2
        ybuf, yptr = _guarded(ybytes, gpu)
        pbuf, pptr = _guarded(2 * parts * N * 4, gpu)
        sbuf, sptr = _guarded(ws_bytes, gpu)
        rc = _lib.load().s2i_conv_forward_bf16(ctypes.byref(d), x.data_ptr(), wb.data_ptr(), None, yptr, pptr if rec["stats"] else None,
                                               sptr, ws_bytes, _lib.stream())
        torch.cuda.synchronize()
    assert rc == 0, _lib.load().s2i_last_error()
    chk = LH.Check(what, {"direct bf16/conv": C.GAMMA["bf16/conv"], "direct stats": C.GAMMA_STATS}, EDGE_LEDGER)
    chk.watch(ybuf, LH.GUARD_BYTES, ybytes)
    chk.watch(pbuf, LH.GUARD_BYTES, 2 * parts * N * 4)
    chk.watch(sbuf, LH.GUARD_BYTES, ws_bytes)
    yv = _inner(ybuf, ybytes, torch.int16).view(rows + GUARD_ROWS, ldy)
    yb = _inner(ybuf, ybytes, torch.uint8).view(rows + GUARD_ROWS, ldy * 2)
    for name, t in (("columns [N, ldy)", yb[:rows, 2 * N:]), ("rows behind the last", yb[rows:])):
        hit = int((t != LH.GUARD_BYTE).sum())
        if hit:
            chk.bad.append("%d sentinel bytes of %s were written" % (hit, name))
    B, H, W, _ = rec["x"][0]
    Ho, Wo = E.ops._geom(rec["kind"], H, W)
    out = LH.nchw(yv[:rows, :N].contiguous().view(torch.bfloat16).view(B, Ho, Wo, N).double())
    xd, W64 = LH.nchw(x.double()), w.double()
    pre, ref = C.conv_ref(rec, op, layer, xd, None, W64, packed.shape[-1], None, None)
    absref, _ = C.conv_ref(rec, op, layer, xd.abs(), None, W64.abs(), packed.shape[-1], None, None)
    mutant = ref.clone()
    mutant[:, N - 1] = 0
    chk.close("direct bf16/conv", "y[:, :N]", out, ref, absref, LH.BF16_ROUND, {"the last valid column not written": mutant})
    if rec["stats"]:
        got = _inner(pbuf, 2 * parts * N * 4, torch.float32).double().view(2, G, parts // G, N).sum(2)
        den = torch.stack((R.group_stats(absref, G)[0], 2 * (absref * pre.abs()).reshape(G, B // G, N, -1).sum((1, 3))))
        chk.close("direct stats", "partial sums", got, R.group_stats(pre, G), den)
    chk.done()


def test_direct_call_refuses_before_any_launch(gpu):
    """A row stride that is no multiple of 8 and a tile that straddles two BatchNorm groups: error code and text, and no
    kernel ran -- the output keeps its fill."""
    import ctypes
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    rec = E.RECORDS[DIRECT[0]]
    cases = []
    with torch.no_grad(), _lib.tuning(**rec["tune"]):
        x, wb, d, plan, _, _ = _direct_operands(rec, gpu, rec["N"] + 8)
        cases.append((E.conv_desc(rec, ldy=rec["N"] + 4), x, wb, plan["rows"] * (rec["N"] + 8) * 2, plan["parts"], "multiples of 8"))
    for rec, text in E.REFUSED:
        (B, H, W, Cx), N = rec["x"][0], rec["N"]
        x = C._operand(rec["x"], LH.gen_rec(gpu, rec), gpu)
        wb = torch.zeros(rec["w"]["packed"][0] * ((N + 127) // 128 * 128) * Cx, dtype=torch.bfloat16, device=gpu)
        cases.append((E.conv_desc(rec), x, wb, B * H * W * 4 * N * 2, 64, text))
    for d, x, wb, ybytes, parts, text in cases:
        ybuf, yptr = _guarded(ybytes, gpu)
        pbuf, pptr = _guarded(2 * parts * d.N * 4, gpu)
        sbuf, sptr = _guarded(1 << 20, gpu)
        rc = lib.s2i_conv_forward_bf16(ctypes.byref(d), x.data_ptr(), wb.data_ptr(), None, yptr, pptr, sptr, 1 << 20, _lib.stream())
        err = lib.s2i_last_error().decode()
        torch.cuda.synchronize()
        assert rc == 1 and text in err, (rc, err)
        for buf in (ybuf, pbuf, sbuf):
            assert bool((buf == LH.GUARD_BYTE).all()), "a refused launch wrote: %s" % text


# ---- the weight-gradient entry points themselves: a strided g, the workspace and the gradient between sentinels ---------
WG_DIRECT = [i for i, r in enumerate(E.RECORDS) if r.get("direct") and "a" in r]


def _wgrad_direct(rec, gpu, *, ldg_pad=8, ws_short=0):
    """One call of s2i_conv_wgrad (fp32 operands) or s2i_conv_wgrad_dt on record rec: g with row stride N + ldg_pad and NaN in
    columns [N, ldg); the workspace of exactly the bytes the workspace query names (less ws_short) and the OIHW tensor each
    between guard bytes, the tensor prefilled where the record writes into one.  Returns everything the checks need."""
    import ctypes
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    gen = LH.gen_rec(gpu, rec)
    a, g = C._operand(rec["a"], gen, gpu), C._operand(rec["g"], gen, gpu)
    a16, g16 = a.dtype == torch.bfloat16, g.dtype == torch.bfloat16
    on_f32 = C.wgrad_on_f32(rec)
    if a16 != g16 and not on_f32:
        a, g = [t if t.dtype == torch.bfloat16 else t.bfloat16().float() for t in (a, g)]
    N = g.shape[-1]
    M = g.numel() // N
    gp = torch.full((M, N + max(ldg_pad, 0)), float("nan"), dtype=g.dtype, device=gpu)
    gp[:, :N] = g.reshape(M, N)
    good = E.wgrad_desc(rec)
    good.ldg = N + max(ldg_pad, 0)
    d = E.wgrad_desc(rec)
    d.ldg = N + ldg_pad
    fp32 = not (a16 or g16)
    ws_bytes = lib.s2i_wgrad_workspace_bytes(ctypes.byref(good)) if fp32 else \
        lib.s2i_wgrad_workspace_bytes_dt(ctypes.byref(good), int(a16), int(g16))
    plan = _lib.wgrad_plan(good, int(a16), int(g16))
    assert ws_bytes > 0 and plan is not None and plan["kernel"] == E.wgrad_plan(rec)["kernel"], (ws_bytes, plan, lib.s2i_last_error())
    assert ws_bytes == plan["ws_slabs"] * plan["K"] * N * 4
    full = list(rec["grad_shape"])
    if rec["I_total"]:
        full[1] = rec["I_total"]
    nel = 1
    for v in full:
        nel *= v
    gbuf, gptr = _guarded(nel * 4, gpu)
    prefill = torch.randn(full, generator=gen, device=gpu) if rec["out"] else None
    if prefill is not None:
        _inner(gbuf, nel * 4, torch.float32).copy_(prefill.view(-1))
    wbuf, wptr = _guarded(ws_bytes, gpu)
    if fp32:
        rc = lib.s2i_conv_wgrad(ctypes.byref(d), a.data_ptr(), None, gp.data_ptr(), gptr, wptr, ws_bytes - ws_short, _lib.stream())
    else:
        rc = lib.s2i_conv_wgrad_dt(ctypes.byref(d), a.data_ptr(), int(a16), None, gp.data_ptr(), int(g16), gptr, wptr,
                                   ws_bytes - ws_short, _lib.stream())
    err = lib.s2i_last_error().decode()
    torch.cuda.synchronize()
    return dict(rc=rc, err=err, a=a, g=g, gbuf=gbuf, wbuf=wbuf, nel=nel, ws_bytes=ws_bytes, full=full, prefill=prefill, plan=plan,
                cls=("bf16" if (a16 or g16) and not on_f32 else "fp32") + "/wgrad")


@pytest.mark.parametrize("index", WG_DIRECT, ids=[E.record_id(i, E.RECORDS[i]) for i in WG_DIRECT])
def test_direct_wgrad_keeps_to_its_workspace_slice_and_columns(gpu, index):
    """s2i_conv_wgrad / s2i_conv_wgrad_dt with ldg = N + 8: every guard byte around the workspace the query sized and
    around the OIHW tensor is unchanged, input channels outside [i_off, i_off + I) are bit-identical, the slabs a bf16
    re-cut does not write stay unwritten, and the result holds the bound of its class and is finite (the NaN columns
    [N, ldg) of g were not read)."""
    _default_planner()
    from speech_to_image_translation_without_text_amd import _lib
    rec = E.RECORDS[index]
    what = "direct " + E.record_id(index, rec)
    with torch.no_grad(), _lib.tuning(**rec["tune"]):
        r = _wgrad_direct(rec, gpu)
        eplan = E.wgrad_plan(rec)
    assert r["rc"] == 0, r["err"]
    cls = "direct " + r["cls"]
    chk = LH.Check(what, {cls: C.GAMMA[r["cls"]]}, EDGE_LEDGER)
    chk.watch(r["gbuf"], LH.GUARD_BYTES, r["nel"] * 4)
    chk.watch(r["wbuf"], LH.GUARD_BYTES, r["ws_bytes"])
    plan = r["plan"]
    if plan["slabs"] < plan["ws_slabs"]:
        spare = _inner(r["wbuf"], r["ws_bytes"], torch.uint8)[plan["slabs"] * (r["ws_bytes"] // plan["ws_slabs"]):]
        hit = int((spare != LH.GUARD_BYTE).sum())
        if hit:
            chk.bad.append("%d bytes of the slabs behind the %d the re-cut fills were written" % (hit, plan["slabs"]))
    res = _inner(r["gbuf"], r["nel"] * 4, torch.float32).view(r["full"])
    gs, i_off = rec["grad_shape"], rec["i_off"]
    sl = (slice(None), slice(i_off, i_off + gs[1])) if rec["I_total"] else (slice(None),)
    if rec["I_total"]:
        keep = torch.ones(r["full"], dtype=torch.bool, device=gpu)
        keep[sl] = False
        chk.equal("input channels outside [%d, %d)" % (i_off, i_off + gs[1]), res[keep], r["prefill"][keep])
    ad, gd = LH.nchw(r["a"].double()), LH.nchw(r["g"].double())
    dw = C.wgrad_dw(rec, R.layer_op(rec)[1], ad, gd)
    base = r["prefill"].double()[sl] if rec["accumulate"] else 0.0
    true = dw()
    got = res[sl]
    if not bool(torch.isfinite(got).all()):
        chk.bad.append("the result is not finite: columns [N, ldg) of g were read")
    mutants = {k: base + m for k, m in E.wgrad_mutants(rec, eplan, ad, gd, dw, true).items()}
    chk.close(cls, "grad", got, base + true, dw(absval=True), 2 * LH.U if rec["accumulate"] else 0.0, mutants)
    chk.done()


def test_direct_wgrad_refuses_before_any_launch(gpu):
    """A workspace one byte short and ldg < N: error code and text, and no kernel ran -- workspace and gradient keep their fill."""
    from speech_to_image_translation_without_text_amd import _lib
    rec = E.RECORDS[WG_DIRECT[0]]
    assert not rec["out"]
    with torch.no_grad(), _lib.tuning(**rec["tune"]):
        for kw, text in ((dict(ws_short=1), "workspace too small"), (dict(ldg_pad=-4), "ldg < N")):
            r = _wgrad_direct(rec, gpu, **kw)
            assert r["rc"] == 1 and text in r["err"], (r["rc"], r["err"])
            for buf in (r["gbuf"], r["wbuf"]):
                assert bool((buf == LH.GUARD_BYTE).all()), "a refused launch wrote: %s" % text



# ---- the ragged production batch -------------------------------------------------------------------------------------
def take_census(gpu):
    return LH.take_step_census(gpu, RAGGED_MODES, C.wrap_dispatchers)


def _rows(rec):
    B, H, W, _ = (rec["x"] if "x" in rec else rec["a"])[0]
    Ho, Wo = E._geom(rec["kind"], H, W)
    return B * Ho * Wo


def test_ragged_census_matches_committed_file(gpu):
    """One train step of each workload at B = 23."""
    live, calls = take_census(gpu)
    for mode, recs in live.items():
        print("census %s: %d dispatcher calls per step, %d distinct launches" % (mode, calls[mode], len(recs)))
        stacked = [r for r in recs if r.get("groups", 1) > 1]
        assert not stacked, "%s: a stacked discriminator pass at B = 23: %s" % (mode, stacked[:2])
    LH.assert_census_equal(live, LH.load_census(CENSUS_FILE), RAGGED_MODES, "ragged_launches.json")


def _ragged_cases():
    out = []
    for mode, recs in LH.load_census(CENSUS_FILE).items():
        kept = 0
        for i, rec in enumerate(recs):
            if _rows(rec) > ROW_CAP:
                continue
            kept += 1
            op, layer = R.layer_op(rec)
            out.append(pytest.param(mode, i, id="%s-%03d-%s-%s-%s" % (mode, i, rec["fn"], op, layer)))
        LEFT_OUT[mode] = (kept, len(recs) - kept)
    return out


@pytest.mark.parametrize("mode,index", _ragged_cases())
def test_ragged_launch_replay_matches_fp64(gpu, mode, index):
    _default_planner()
    rec = LH.load_census(CENSUS_FILE)[mode][index]
    assert rec.get("groups", 1) == 1, "a stacked launch in the ragged census"
    what = "%s[%d] %s %s" % (mode, index, rec["fn"], "%s/%s" % R.layer_op(rec))
    with torch.no_grad():
        if rec["fn"].startswith("conv"):
            C.replay_conv(rec, LH.gen_rec(gpu, rec), gpu, what, RAGGED_LEDGER,
                          extra=_edge_extra(RAGGED_LEDGER) if rec["stats"] else None)
        else:
            C.replay_wgrad(rec, LH.gen_rec(gpu, rec), gpu, what, RAGGED_LEDGER)
    torch.cuda.empty_cache()


def test_ragged_census_is_committed():
    census = LH.load_census(CENSUS_FILE)
    assert set(census) == set(RAGGED_MODES) and all(census[m] for m in RAGGED_MODES), "tests/ragged_launches.json is missing"


def test_no_wrong_reference_was_accepted(gpu):
    """Last in the module, after its replays: every wrong reference built for a bf16 plan branch was rejected."""
    assert not ACCEPTED, ACCEPTED


if __name__ == "__main__":
    # regenerate tests/ragged_launches.json (or the path given) from one eager step of each workload at B = 23
    from speech_to_image_translation_without_text_amd import _lib
    _lib.load()
    _lib.require_device()
    census, calls = take_census(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else CENSUS_FILE
    LH.write_census(path, census)
    for mode, recs in census.items():
        print("census %s: %d dispatcher calls per step, %d distinct launches -> %s" % (mode, calls[mode], len(recs), path))
