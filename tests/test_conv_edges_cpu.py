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
    "b16-groups-multi-image", "b16-wg-split-overwrite", "b16-wg-recut-fewer-slabs",
    # the branches of plan_wgrad and the finishing paths of launch_wgrad (conv_edges._wgrad_branches)
    "wg-pixtail-128x32", "wg-rows3-coltail", "wg-short-last-split-rows3", "wg-short-last-split-128x128", "wg-short-last-split-128x32",
    "wg-short-last-split-96x64", "wg-short-last-split-96x32", "wg-short-last-split-256x128", "wg-short-last-split-256x256",
    "wg-16-on-f32-a", "wg-16-on-f32-g", "wg-16-on-f32-ag",
    "wg-finish-rt1-direct", "wg-finish-rt2-direct", "wg-finish-rt4-direct", "wg-finish-rt8-direct", "wg-finish-rt1-direct-ctail",
    "wg-finish-rt2-direct-swap", "wg-finish-rt1-stream", "wg-finish-rt2-stream", "wg-finish-rt4-stream", "wg-finish-rt8-stream",
    "wg-finish-rt1-stream-ctail", "wg-finish-rt8-stream-ctail", "wg-finish-rt2-stream-ctail-swap", "wg-finish-rt1-tree",
    "wg-finish-rt1-tree-ctail",
)
# what conv_edges._wgrad_branches adds and no weight-gradient record of the two census files reaches
NEW_WGRAD = ("wg-rows3-coltail", "wg-16-on-f32-g", "wg-16-on-f32-ag", "wg-short-last-split-96x64", "wg-short-last-split-96x32",
             "wg-short-last-split-256x128", "wg-short-last-split-256x256", "wg-pixtail-128x32", "wg-finish-rt4-direct",
             "wg-finish-rt4-stream")
# named kernels no fp64 replay of a record runs, each with its reason
WGRAD_NOT_REPLAYED = {
    "f32in-128x128": "apply-on-load is off by default and the replay schema has no a_src; tests/test_parity_gpu.py holds it to the "
                     "separate BatchNorm + LeakyReLU pass",
}
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
    # a prefilled, an accumulated and a sliced destination each behind both slab sums
    for flag in ("accumulate", "i_off", "out"):
        for path in ("-stream", "-tree"):
            assert any(r.get(flag) and any(f.startswith(E.FIN) and path in f for f in r["reach"]) for r in E.RECORDS), (flag, path)
    # every row-segment instantiation off the census batches, the 128-thread one in every form the others have
    wg = [(r, E.wgrad_plan(r)) for r in E.RECORDS if "a" in r]
    for name in ("rows3-32x64", "rows3-32x32", "rows3-64x128", "rows3-64x64", "rows3-64x32"):
        assert any(p["kernel"] == name and "wg-rows3-odd-batch" in p["reach"] for _, p in wg), name
    for name in ("rows3-32x64", "rows3-64x128"):
        assert any(p["kernel"] == name and "wg-rows3-coltail" in p["reach"] for _, p in wg), name
    small = [(r, p) for r, p in wg if p["kernel"] == "rows3-64x32"]
    assert all(p["threads"] == 128 for _, p in small) and all(p["threads"] != 128 for _, p in wg if p["kernel"] != "rows3-64x32")
    assert {r["a"][0][2] for r, _ in small} == {32, 64} and any(r["a"][0][0] == 1 for r, _ in small)
    assert any("wg-short-last-split-rows3" in p["reach"] for _, p in small) and any(r["accumulate"] and r["i_off"] for r, _ in small)
    # a bf16 operand on each tile of the fp32-MFMA kernel that takes one, and under swap + fold
    for tag, tiles in (("wg-16-on-f32-a", ("f32-128x128", "f32-128x64", "f32-64x64")), ("wg-16-on-f32-g", ("f32-128x128", "f32-128x64")),
                       ("wg-16-on-f32-ag", ("f32-128x128", "f32-128x64", "f32-64x64", "f32-128x32"))):
        for name in tiles:
            assert any(tag in p["reach"] and p["kernel"] == name for _, p in wg), (tag, name)
    assert any("wg-16-on-f32-g" in p["reach"] and r["swap"] for r, p in wg)
    assert any("wg-16-on-f32-a" in p["reach"] and p["slabs"] > 2 for r, p in wg)


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
    rows = [(r, E.conv_plan(r)) for r in E.RECORDS if r.get("direct") and "x" in r]
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


# ---- the weight gradient: every named kernel, every branch of plan_wgrad, every finishing path of launch_wgrad ----------
def _wgrad_kernels_replayed():
    """{kernel name: where} over the weight-gradient records of every table a fp64 replay runs."""
    import image_layer_edges as IE
    import split_planes as S
    from speech_to_image_translation_without_text_amd import _lib
    seen = {}
    for rec in (r for r in E.RECORDS if "a" in r):
        seen.setdefault(E.wgrad_plan(rec)["kernel"], "conv_edges")
    for rec in (r for r in IE.RECORDS if "a" in r):
        told = _lib.wgrad_plan(E.wgrad_desc(rec), int(rec["a"][1] == "bf16"), int(rec["g"][1] == "bf16"))
        seen.setdefault(told["kernel"], "image_layer_edges")
    for index, planes in S.cases():
        rec = S.RECORDS[index]
        if not S.is_conv(rec):
            seen.setdefault(_lib.wgrad_plan(E.wgrad_desc(rec), planes=planes)["kernel"], "split_planes")
    return seen


def test_every_named_wgrad_kernel_is_replayed_in_fp64():
    """Every name of _lib.WGRAD_KERNELS is the plan of a record of tests/conv_edges.py, tests/image_layer_edges.py or
    tests/split_planes.py, each of which its GPU module replays against fp64; the exceptions are listed with their reason.
    A kernel added to plan_wgrad without a record fails here."""
    from speech_to_image_translation_without_text_amd import _lib
    seen = _wgrad_kernels_replayed()
    assert set(seen) <= set(_lib.WGRAD_KERNELS)
    assert all(why for why in WGRAD_NOT_REPLAYED.values())
    stale = sorted(set(WGRAD_NOT_REPLAYED) & set(seen))
    assert not stale, "replayed after all, take them off WGRAD_NOT_REPLAYED: %s" % stale
    missing = sorted(set(_lib.WGRAD_KERNELS) - set(seen) - set(WGRAD_NOT_REPLAYED))
    assert not missing, "weight-gradient kernels no fp64 replay runs: %s" % missing


def test_the_new_wgrad_branches_are_new():
    """The gap conv_edges._wgrad_branches closes, stated as a test (to be updated when production starts to cover one): no
    weight-gradient record of tests/step_launches.json or tests/ragged_launches.json plans to rows3-64x32 or reaches any of
    NEW_WGRAD; the table reaches each."""
    table = set()
    for rec in (r for r in E.RECORDS if "a" in r):
        table |= E.wgrad_plan(rec)["reach"]
    assert any(E.wgrad_plan(r)["kernel"] == "rows3-64x32" for r in E.RECORDS if "a" in r)
    for tag in NEW_WGRAD:
        assert tag in table, tag
    seen = 0
    for rec in (r for r in _census_records() if "a" in r):
        plan = E.wgrad_plan(rec, table=False)
        what = json.dumps(rec, sort_keys=True)
        assert plan["kernel"] != "rows3-64x32", "a production shape runs rows3-64x32: %s" % what
        hit = sorted(plan["reach"] & set(NEW_WGRAD))
        assert not hit, "a production shape reaches %s, update NEW_WGRAD: %s" % (hit, what)
        seen += 1
    assert seen > 50


def test_direct_wgrad_rows_cover_what_the_entry_points_decide():
    """The rows tests/test_conv_edges_gpu.py also launches through s2i_conv_wgrad / s2i_conv_wgrad_dt themselves."""
    rows = [(r, E.wgrad_plan(r)) for r in E.RECORDS if r.get("direct") and "a" in r]
    assert 8 <= len(rows) <= 10
    kernels = [p["kernel"] for _, p in rows]
    assert kernels.count("rows3-64x32") == 3 and "f32-256x256" in kernels
    assert any(r["accumulate"] and r["i_off"] for r, _ in rows), "a prefilled slice between the guard bytes"
    assert any(p["slabs"] == 231 for _, p in rows)
    assert any("wg-short-last-split-128x32" in p["reach"] for _, p in rows)
    assert any("wg-16-on-f32-ag" in p["reach"] and r["g"][0][3] % 8 for r, p in rows)
    assert any(E.FIN + "rt4-stream" in p["reach"] for _, p in rows)
    assert any(E.FIN + "rt1-tree" in p["reach"] and r["accumulate"] for r, p in rows)
    assert any(p["family"] == "b16" and p["slabs"] < p["ws_slabs"] for _, p in rows)
    assert not rows[0][0]["out"], "the refusals run on the first row and expect an untouched, unfilled gradient"


def _cpu_operand(desc, gen):
    shape, dt = desc
    t = torch.randn(shape, generator=gen)
    return (t.bfloat16() if dt == "bf16" else t).double().permute(0, 3, 1, 2)


def test_wrong_wgrad_references_lie_outside_the_bound():
    """Power of the wrong references of conv_edges.wgrad_mutants, with the reference alone: for every weight-gradient record
    of the table, each mutant is outside gamma x absref of the true fp64 gradient under the class constant its kernel family
    replays with, so a kernel that produced it could not pass.  Every record of _wgrad_branches has at least one."""
    g0 = torch.Generator().manual_seed(13)
    first = next(i for i, r in enumerate(E.RECORDS) if r["why"].startswith("rows3-64x32 (never run)"))
    names = set()
    for index, rec in enumerate(E.RECORDS):
        if "a" not in rec:
            continue
        plan = E.wgrad_plan(rec)
        layer = R.layer_op(rec)[1]
        a, g = _cpu_operand(rec["a"], g0), _cpu_operand(rec["g"], g0)
        cd = torch.randn((a.shape[0], rec["cvec"]), generator=g0).double() if rec["cvec"] else None
        dw = C.wgrad_dw(rec, layer, a, g, cd)
        true, absref = dw(), dw(absval=True)
        assert plan["family"] in ("f32", "rows3", "b16", "b16d1"), plan
        gamma = C.GAMMA[("bf16" if plan["family"].startswith("b16") else "fp32") + "/wgrad"]
        assert LH.compare(true, true, absref, 0.0, gamma)[1]
        mutants = E.wgrad_mutants(rec, plan, a, g, dw, true)
        assert mutants or index < first, IDS[index]
        for name, m in mutants.items():
            assert LH.fails(true, m, absref, 0.0, gamma), (IDS[index], name)
            names.add(name.split(":")[0])
    assert names == {"pixel tail", "slabs", "column tail", "row segment", "bf16 a", "bf16 g", "swap + fold"}, names


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
