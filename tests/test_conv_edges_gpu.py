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
    fp32 weight gradient            3.2e-7 | 4.1e-7 | 4.0e-7   (8e-7)
    bf16 forward / input gradient   1.1e-9 | 3.4e-8 | 5.1e-8   (1e-7)
    bf16 weight gradient            1.2e-7 | 1.2e-7 | 1.6e-7   (3.2e-7)
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
    def extra(ctx):
        for tag in ctx["rec"]["reach"]:
            if tag.startswith("b16-"):
                ledger.note("branch " + tag, ctx["ratio"], what, ctx["gamma"])
        return []
    return extra


# ---- the bf16 entry point itself: a strided destination, every buffer between sentinels ---------------------------------
DIRECT = [i for i, r in enumerate(E.RECORDS) if r.get("direct")]


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
