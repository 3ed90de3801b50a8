"""The edge table (tests/conv_edges.py) reaches what it claims, and the train step's census does not.

The planners are host code and the library loads without a device, so every record's plan is asked of them here: the
fp32 forward's tile, K split and chunk counts of s2i_conv_plan_query, the weight gradient's of s2i_wgrad_plan_query, the
bf16 unit's pixels and images per tile, tiles and (persistent) grid of s2i_conv_bf16_plan_query.  No GPU."""
import json
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

# every feature the table as a whole must reach
REQUIRED = (
    "rowtail-128", "rowtail-96", "rowtail-128x64", "rowtail-128x32", "single-partial-tile", "coltail", "ktail",
    "short-last-split", "rowtail-4phase", "groups-96", "wg-pixtail-128x128", "wg-pixtail-128x64", "wg-pixtail-64x64", "wg-pixtail-96x64",
    "wg-pixtail-96x32", "wg-pixtail-256x128", "wg-pixtail-256x256", "wg-rows3-odd-batch", "b16-ragged-128", "b16-ragged-256",
    "b16-wg-stagetail",
)

IDS = [E.record_id(i, r) for i, r in enumerate(E.RECORDS)]


def test_record_ids_and_records_are_distinct():
    assert len(set(IDS)) == len(IDS)
    canon = [LH.canon(r) for r in E.RECORDS]
    assert len(set(canon)) == len(canon)
    for rec in E.RECORDS:
        assert rec["why"] and set(rec["reach"]) <= set(E.REACH), rec


@pytest.mark.parametrize("index", range(len(E.RECORDS)), ids=IDS)
def test_record_reaches_what_it_claims(index):
    rec = E.RECORDS[index]
    plan = E.plan(rec)
    assert set(rec["reach"]) == plan["reach"], (IDS[index], plan)
    if rec["fn"].startswith("conv") and not rec["fast"]:
        # a forced tile height is run only where the planner honours it
        if rec["tile_rows"]:
            assert plan["bm"] == rec["tile_rows"], (IDS[index], plan)
        if rec["cls_bias"]:
            assert plan["splitk"] == 1, "the class-bias table needs an unsplit plan"
    B = (rec["x"] if "x" in rec else rec["a"])[0][0]
    chans = max((rec["x"][0][3], rec["N"]) if "x" in rec else (rec["a"][0][3], rec["g"][0][3]))
    assert B <= 11 and chans <= 2048, "the edge shapes stay small"


def test_table_reaches_every_edge():
    reached = set()
    for rec in E.RECORDS:
        reached |= set(rec["reach"])
    missing = [f for f in REQUIRED if f not in reached]
    assert not missing, "no record of tests/conv_edges.py reaches: %s" % missing
    # the forward row tails are run with BatchNorm statistics, under the planner's own choice and under both forced heights
    for f in ("rowtail-128", "rowtail-96", "rowtail-128x64", "rowtail-128x32", "rowtail-4phase", "single-partial-tile"):
        assert any(f in r["reach"] and r.get("stats") for r in E.RECORDS), "%s without statistics" % f
    assert any("short-last-split" in r["reach"] and r["wmode"] == 0 and r["stats"] for r in E.RECORDS if "x" in r)
    assert any(r.get("cls_bias") and "rowtail-96" in r["reach"] for r in E.RECORDS)
    for flag in ("swap", "fold", "accumulate", "i_off"):
        assert any(r.get(flag) and any(f.startswith(("wg-pixtail", "b16-wg")) for f in r["reach"]) for r in E.RECORDS), flag
    assert any(r["fn"] == "wgrad_any" and r["a"][1] != r["g"][1] for r in E.RECORDS if "a" in r), "the mixed weight gradient"


def test_step_census_reaches_none_of_the_tails():
    """The gap the edge table closes, stated as a test: it fails (and is to be updated) when a production shape starts to
    cover an edge.  On spatial maps no launch of tests/step_launches.json has a partly filled row tile, a short pixel
    chunk or a ragged bf16 image tile.  The K1 launches on 1 x 1 maps (the fc layers and the class-aware loss's matrix
    products, M = the batch) are the exception the census does hold: one partly filled tile, one short chunk."""
    census = LH.load_census(os.path.join(HERE, "step_launches.json"))
    assert set(census) == set(LH.STEP_MODES)
    seen = 0
    for mode, recs in census.items():
        for rec in recs:
            what = "%s %s" % (mode, json.dumps(rec, sort_keys=True))
            rec = dict(rec, tile_rows=0, tune={})
            if rec["fn"].startswith("conv"):
                B, H, W, _ = rec["x"][0]
                Ho, Wo = E._geom(rec["kind"], H, W)
                M = B * Ho * Wo
                if H * W == 1:
                    assert M in (24, 48), what
                    continue
                if rec["fast"]:
                    plan = E.conv_plan(rec)
                    assert not plan["reach"] and B % plan["tb"] == 0, (what, plan)
                else:
                    assert M % 128 == 0 and M % 96 == 0, what     # whole row tiles under either height
            else:
                B, H, W, _ = rec["a"][0]
                Ho, Wo = E.ops._geom(rec["kind"], H, W)
                M = B * Ho * Wo
                if H * W == 1:
                    assert M in (24, 48), what
                    continue
                assert M % 64 == 0, what                          # whole 32-pixel chunks and 64-pixel bf16 stages
            seen += 1
    assert seen > 100


def test_dropping_the_last_row_breaks_the_partial_sum_bound():
    """Power of the BatchNorm partial-sum check, with the reference alone: sums that leave out the single last row (the last
    pixel of the last image) are outside GAMMA_STATS x sum|.| of the full sums.  The dropped row changes a column's sum by
    its value v; the bound is 1.5e-7 x M x mean|absref| with M <= 6000 rows, at most a thousandth of mean|absref|, so only a
    column whose last-row value is that close to zero passes, and the comparison fails as soon as one column does not."""
    g = torch.Generator().manual_seed(11)
    for rec in (r for r in E.RECORDS if r.get("stats") and r["x"][0][0] * r["x"][0][1] ** 2 <= 6000):
        op, layer = R.layer_op(rec)
        B, H, W, Cx = rec["x"][0]
        N = rec["N"]
        x = torch.randn(B, Cx + rec["cvec"], H, W, generator=g, dtype=torch.float64)
        w = LH.dyadic(rec["w"]["oihw"], g, "cpu").double()[:, -x.shape[1]:]
        pre, apre = R.fwd(layer, x, w), R.fwd(layer, x.abs(), w.abs())
        G = rec["groups"]
        full = R.group_stats(pre, G)
        den = torch.stack((R.group_stats(apre, G)[0], 2 * (apre * pre.abs()).reshape(G, B // G, N, -1).sum((1, 3))))
        cut = pre.clone()
        cut[-1, :, -1, -1] = 0
        assert LH.compare(full, full, den, 0.0, C.GAMMA_STATS)[1]
        mutant = R.group_stats(cut, G)
        assert LH.fails(full, mutant, den, 0.0, C.GAMMA_STATS), rec
