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


@pytest.fixture(scope="module", autouse=True)
def _report():
    EDGE_LEDGER.start()
    RAGGED_LEDGER.start()
    yield
    EDGE_LEDGER.report("edge table replay")
    RAGGED_LEDGER.report("ragged batch (B = 23) launch replay")
    for mode, (kept, cut) in sorted(LEFT_OUT.items()):
        print("ragged census %s: %d records replayed, %d left out by the cap of %d rows per phase" % (mode, kept, cut, ROW_CAP))


def _default_planner():
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0, "the replay runs the default planner"
    assert os.environ.get("S2I_TUNE", "") == "", "the replay runs the default planner"


# ---- power checks ----------------------------------------------------------------------------------------------------
def _edge_extra(ledger):
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
        return bad
    return extra


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
            C.replay_conv(rec, LH.gen_rec(gpu, rec), gpu, what, EDGE_LEDGER, extra=_edge_extra(EDGE_LEDGER))
        else:
            C.replay_wgrad(rec, LH.gen_rec(gpu, rec), gpu, what, EDGE_LEDGER)
    torch.cuda.empty_cache()


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
