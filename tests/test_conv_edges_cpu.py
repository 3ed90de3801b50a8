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
    "b16-wg-stagetail", "b16-coltail", "b16-v2-split", "b16-short-last-split", "b16-tb>1", "b16-cls-multi-image",
    "b16-groups-multi-image", "b16-wg-split-overwrite",
)
# the bf16 plan branches the edge table adds and no production shape takes
NEW_B16 = ("b16-coltail", "b16-v2-split", "b16-cls-multi-image")
CENSUS_FILES = ("step_launches.json", "ragged_launches.json")

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
    if rec["fn"].startswith("conv") and rec["fast"]:
        if rec["cls_bias"]:
            assert plan["splitk"] == 1, "the class-bias table needs an unsplit plan"
        assert rec["x"][0][1] <= 64 and rec["x"][0][3] <= 512, "the bf16 edge maps stay small"
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
                    # whole image tiles; tiles of several images and a short last split of the 128-pixel kernel are
                    # production shapes, every other bf16 feature of the table is not
                    assert plan["reach"] <= {"b16-tb>1", "b16-short-last-split", "b16-groups-multi-image"}, (what, plan)
                    assert B % plan["tb"] == 0, (what, plan)
                    assert "b16-short-last-split" not in plan["reach"] or plan["bm"] == 128, (what, plan)
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


# ---- the bf16 unit: every named kernel, every branch of plan_bf16 ----------------------------------------------------
def _census_records():
    for name in CENSUS_FILES:
        census = LH.load_census(os.path.join(HERE, name))
        assert census, name
        for recs in census.values():
            for rec in recs:
                yield dict(rec, tile_rows=0, tune={})


def _replayed():
    """(conv kernel, wmode) pairs, weight-gradient kernels and plan features of every bf16 launch the fp64 replays run: the
    edge table on one side, the two census files on the other."""
    out = {}
    for side, recs in (("table", E.RECORDS), ("census", list(_census_records()))):
        conv, wg, reach, plans = set(), set(), set(), []
        for rec in recs:
            if rec["fn"] == "conv_any" and rec["fast"]:
                plan = E.conv_plan(rec)
                conv.add((plan["kernel"], rec["wmode"]))
                reach |= plan["reach"]
                plans.append((rec, plan))
            elif rec["fn"] == "wgrad_any":
                plan = E.wgrad_plan(rec)
                wg.add(plan["kernel"])
                reach |= plan["reach"]
        out[side] = dict(conv=conv, wgrad=wg, reach=reach, plans=plans)
    return out


def _plannable_kernels():
    """(kernel, wmode) of every descriptor of a small grid the plan names a kernel for, under the default knobs and with the
    256-pixel kernel forced; the weight gradient's b16 kernels of a grid of its own."""
    from speech_to_image_translation_without_text_amd import _lib, ops
    conv, wg = set(), set()
    for knobs in ({}, dict(b16_v2=2, b16_persist=4)):
        with _lib.tuning(**knobs):
            for kind in (ops.CONV_K3S1, ops.CONV_K4S2, ops.TCONV_K4S2):
                for wmode in (0, 1):
                    for B in (1, 8):
                        for H in (4, 8, 16, 32, 64):
                            for Cx in (32, 64, 96):
                                for N in (32, 64, 128):
                                    f = dict(kind=kind, B=B, H=H, W=H, Cx=Cx, Cc=0, N=N, wmode=wmode, flip=0, wR=Cx, ldw=N, act=0,
                                             stats=0, ldy=N, groups=1, nosplit=0, kw=0, stride=0, pad=0, tile_rows=0, in_act=0,
                                             in_groups=0)
                                    told = _lib.conv_bf16_plan(_lib.ConvDesc(*[f[n] for n, _ in _lib.ConvDesc._fields_]))
                                    if told is not None and told["kernel"] is not None:
                                        conv.add((told["kernel"], wmode))
    for layer in ("k1", "k3s1", "k4s2"):
        for B in (1, 3, 48):
            for H in (4, 16, 64):
                for Cin in (32, 128, 512):
                    for N in (32, 64, 128, 512):
                        for knobs in ({}, dict(wgrad16_bm=256), dict(wgrad16_bm=512)):
                            rec = E.wgrad(layer, B, H, Cin, N, "grid", [], a16=True, g16=True, tune=knobs)
                            d = E.wgrad_desc(rec)
                            with _lib.tuning(**knobs):
                                told = _lib.wgrad_plan(d, 1, 1)
                            if told is not None:
                                wg.add(told["kernel"])
    for B in (1, 5, 48):              # the first discriminator conv: fp32 NHWC4 image x bf16 gradient
        told = _lib.wgrad_plan(E.wgrad_desc(E.wgrad("k4s2", B, 8, 4, 64, "grid", [], g16=True)), 0, 1)
        if told is not None:
            wg.add(told["kernel"])
    return conv, wg


def test_every_named_bf16_kernel_is_replayed_in_fp64():
    """Every name of _lib.B16_KERNELS, in each direction (forward weights, wmode 0; input-gradient weights, wmode 1) in which
    some descriptor plans to it, is the plan of an edge record or of a census record; so is every b16 name of
    _lib.WGRAD_KERNELS."""
    from speech_to_image_translation_without_text_amd import _lib
    conv, wg = _plannable_kernels()
    assert {k for k, _ in conv} == set(_lib.B16_KERNELS), "the grid plans to no: %s" % sorted(set(_lib.B16_KERNELS) - {k for k, _ in conv})
    b16_wg = {k for k in _lib.WGRAD_KERNELS if k.startswith("b16")}
    assert b16_wg <= wg, "the grid plans to no: %s" % sorted(b16_wg - wg)
    seen = _replayed()
    have = seen["table"]["conv"] | seen["census"]["conv"]
    assert not conv - have, "bf16 kernels (name, wmode) no fp64 replay runs: %s" % sorted(conv - have)
    have = seen["table"]["wgrad"] | seen["census"]["wgrad"]
    assert not b16_wg - have, "bf16 weight-gradient kernels no fp64 replay runs: %s" % sorted(b16_wg - have)


def test_the_new_bf16_branches_are_new():
    """The table adds what the census lacks: each of NEW_B16 is reached by a record of the table and by no census record.
    Grouped statistics on tiles of several images are the one branch production does take, in one form: 3 groups of 48
    images (batch 144) on the 128-pixel kernel, at least 6 tiles to a group.  The table adds the forms it lacks: the
    256-pixel kernel, 2 groups, and groups of one or two tiles, where a tile counted to the wrong group is a whole group's
    error and not a sixth of one."""
    seen = _replayed()
    for tag in NEW_B16:
        assert tag in seen["table"]["reach"], tag
        assert tag not in seen["census"]["reach"], "a production shape reaches %s: update NEW_B16" % tag
    gm = "b16-groups-multi-image"
    census_groups = [(r, p) for r, p in seen["census"]["plans"] if gm in p["reach"]]
    assert census_groups
    for r, p in census_groups:
        assert (p["bm"], r["groups"]) == (128, 3) and r["x"][0][0] // r["groups"] // p["tb"] >= 6, (r, p)
    table_groups = [(r, p) for r, p in seen["table"]["plans"] if gm in p["reach"]]
    assert any(p["bm"] == 256 for r, p in table_groups) and any(r["groups"] == 2 for r, p in table_groups)
    assert any(r["x"][0][0] // r["groups"] == p["tb"] for r, p in table_groups), "a group of one tile"
    assert all(r["x"][0][0] // r["groups"] // p["tb"] <= 2 for r, p in table_groups)
    # each with BatchNorm statistics in a forward launch, the split of the 256-pixel kernel on each of its four instantiations
    fast = [(r, E.conv_plan(r)) for r in E.RECORDS if r["fn"] == "conv_any" and r["fast"]]
    for tag in NEW_B16:
        assert any(tag in p["reach"] and r["stats"] and r["wmode"] == 0 for r, p in fast), tag
    for name in ("b16v2-k3s1", "b16v2-tconv", "b16v2-k4s2", "b16v2-k4s2-pw66"):
        assert any(p["kernel"] == name and "b16-v2-split" in p["reach"] for _, p in fast), name
        assert any(p["kernel"] == name and "b16-coltail" in p["reach"] for _, p in fast), name
    from speech_to_image_translation_without_text_amd import _lib
    for name in _lib.B16_KERNELS:
        assert any(p["kernel"] == name and "b16-coltail" in p["reach"] and r["stats"] for r, p in fast), name
    assert any({"b16-coltail", "b16-short-last-split", "b16-v2-split"} <= p["reach"] for _, p in fast)
    assert any("b16-coltail" in p["reach"] and p["splitk"] > 1 and r["wmode"] == 1 for r, p in fast)
    assert any("b16-groups-multi-image" in p["reach"] and p["splitk"] > 1 for _, p in fast), "the reducer's groups"
    for g in (2, 3):
        assert any("b16-groups-multi-image" in p["reach"] and r["groups"] == g for r, p in fast), g
    for bm in (128, 256):
        assert any("b16-cls-multi-image" in p["reach"] and p["bm"] == bm and "b16-ragged-%d" % bm in p["reach"] for _, p in fast), bm
        assert any("b16-groups-multi-image" in p["reach"] and p["bm"] == bm for _, p in fast), bm


def test_direct_rows_cover_both_kernel_generations():
    """The rows tests/test_conv_edges_gpu.py also launches through s2i_conv_forward_bf16 itself: each 256-pixel kernel, three
    128-pixel kernels, a split with a column tail in both directions, every one with a column tail."""
    rows = [(r, E.conv_plan(r)) for r in E.RECORDS if r.get("direct")]
    assert 8 <= len(rows) <= 12
    for r, p in rows:
        assert r["fast"] and "b16-coltail" in p["reach"] and not r["cls_bias"], r
    names = {p["kernel"] for _, p in rows}
    assert {"b16v2-k3s1", "b16v2-tconv", "b16v2-k4s2", "b16v2-k4s2-pw66"} <= names
    assert len({n for n in names if not n.startswith("b16v2")}) >= 3
    for wmode in (0, 1):
        assert any(p["splitk"] > 1 and r["wmode"] == wmode for r, p in rows), wmode
    assert any(p["splitk"] > 1 and r["stats"] and r["groups"] > 1 for r, p in rows), "the reducer's grouped statistics"
    assert any(p["bm"] == 256 and p["splitk"] > 1 for r, p in rows)


def test_class_bias_alone_keeps_a_layer_unsplit():
    """nosplit: a record whose plan is unsplit only because it carries a class bias."""
    from speech_to_image_translation_without_text_amd import _lib
    hit = 0
    for rec in (r for r in E.RECORDS if r["fn"] == "conv_any" and r["fast"] and r["cls_bias"]):
        with _lib.tuning(**rec["tune"]):
            free = _lib.conv_bf16_plan(E.conv_desc(rec, nosplit=0))
            held = _lib.conv_bf16_plan(E.conv_desc(rec))
        assert held["splitk"] == 1, rec
        hit += free["splitk"] > 1
    assert hit >= 1


def test_a_plan_without_a_kernel_is_not_the_fast_path():
    """B16_NO_KERNEL: the plan accepts the descriptor and names no kernel; the record says ops.conv_any takes the fp32 kernel."""
    from speech_to_image_translation_without_text_amd import _lib
    assert E.NO_KERNEL
    for rec in E.NO_KERNEL:
        # everything ops.conv_any asks before it plans the bf16 launch holds: only the missing kernel keeps it off the fast path
        assert (rec["fn"], rec["fast"], rec["x"][1], rec["out_dtype"], rec["bias"], rec["act"]) == ("conv_any", False, "bf16", "bf16", 0, 0)
        assert rec["N"] % 8 == 0
        told = _lib.conv_bf16_plan(E.conv_desc(rec))
        assert told is not None and told["kernel"] is None, (rec, told)
        assert set(rec["reach"]) == E.conv_plan(rec)["reach"], rec       # the fp32 plan it falls back to


def test_refused_records_are_refused_by_the_plan():
    from speech_to_image_translation_without_text_amd import _lib
    assert E.REFUSED
    for rec, text in E.REFUSED:
        with _lib.tuning(**rec["tune"]):
            assert _lib.conv_bf16_plan(E.conv_desc(rec)) is None, rec
        assert text in _lib.load().s2i_last_error().decode(), _lib.load().s2i_last_error()
