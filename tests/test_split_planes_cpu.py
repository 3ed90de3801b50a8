"""The split-mode table (tests/split_planes.py) reaches what it claims, its plane reference and probe operands are what the
GPU module takes them for, and the train step's census reaches none of it.  Everything is derived from the planners' host
queries (conv_edges.conv_plan under tile_rows = 128, which asks s2i_conv_plan_query; s2i_conv_split_eligible;
s2i_wgrad_plan_query with planes).  No GPU."""
import ctypes
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
import split_planes as S  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib, ops  # noqa: E402

CASES = S.cases()
IDS = [S.case_id(i, p) for i, p in CASES]
ROW_TAILS = ("rowtail-128", "rowtail-128x64", "rowtail-128x32", "single-partial-tile")


def test_records_and_ids_are_distinct():
    assert len(set(IDS)) == len(IDS)
    canon = [LH.canon(r) for r in S.RECORDS]
    assert len(set(canon)) == len(canon)
    for rec in S.RECORDS:
        assert rec["why"] and set(rec["reach"]) <= set(S.REACH) and 3 in rec["planes"], rec
        assert set(rec["planes"]) <= {1, 3}


@pytest.mark.parametrize("index,planes", CASES, ids=IDS)
def test_record_reaches_what_it_claims(index, planes):
    rec = S.RECORDS[index]
    plan = S.split_plan(rec, planes)
    assert set(rec["reach"]) == plan["reach"], (IDS[index], plan)
    assert plan["split"] == ("fallback" not in rec["reach"]), plan
    if S.is_conv(rec):
        assert plan["tile"] in S.FWD_TILES
        if plan["split"] and rec["N"] > 64:
            assert plan["bm"] == 128, plan
        if rec["cls_bias"]:
            assert rec["w_offset"] != 0 and plan["splitk"] == 1
    elif plan["split"]:
        assert plan["tile"] in S.WG_TILES, plan
        # the fp32 plan of the same layer: the 96-row tiles and the row-segment kernel are fp32 only
        native = _lib.wgrad_plan(E.wgrad_desc(rec))
        if plan["K"] == 288 and plan["tile"] == "split-128x32":
            assert native["kernel"] == "f32-96x32", native
    else:
        assert plan["tile"] == "smalln-16" and plan["M"] == 32768, plan       # the fp32 stream kernel, planes = 0
    B = (rec["x"] if "x" in rec else rec["a"])[0][0]
    assert B <= 7, "the shapes stay small"


def test_table_covers_every_split_tile_with_a_tail():
    fwd, wg, flags = {}, {}, set()
    for i, rec in enumerate(S.RECORDS):
        if "fallback" in rec["reach"]:
            continue
        plan = S.split_plan(rec, 3)
        reach = set(rec["reach"])
        if S.is_conv(rec):
            fwd.setdefault(plan["tile"], set()).update(reach)
            flags.add("wmode%d" % rec["wmode"])
            if rec["wmode"] and rec["kind"] == ops.TCONV_K4S2:
                flags.add("wmode1-phases")
            if rec["stats"] and plan["splitk"] > 1:
                flags.add("stats-from-slabs")
            if rec["stats"] and plan["splitk"] == 1 and reach & set(ROW_TAILS):
                flags.add("stats-per-tile-rowtail")
            if rec["groups"] > 1:
                flags.add("groups")
            if rec["bias"] and rec["act"]:
                flags.add("bias-act")
        else:
            wg.setdefault(plan["tile"], set()).update(reach)
            flags.update(k for k in ("swap", "fold", "accumulate", "i_off") if rec[k])
        flags.update(reach & {"short-last-split", "wg-short-last-split", "rowtail-4phase", "cvec-chunks", "wg-from-vec"})
    assert set(fwd) == set(S.FWD_TILES), fwd
    for tile, reach in fwd.items():
        assert reach & set(ROW_TAILS) and "coltail" in reach, (tile, reach)
    assert set(wg) == set(S.WG_TILES), wg
    for tile, reach in wg.items():
        assert any(f.startswith("wg-pixtail") for f in reach), (tile, reach)
    for tile in ("split-128x128", "split-128x32"):
        assert {"wg-ktail", "wg-coltail"} <= wg[tile], (tile, wg[tile])
    need = {"wmode0", "wmode1", "wmode1-phases", "stats-from-slabs", "stats-per-tile-rowtail", "groups", "bias-act", "swap",
            "fold", "accumulate", "i_off", "short-last-split", "wg-short-last-split", "rowtail-4phase", "cvec-chunks",
            "wg-from-vec"}
    assert need <= flags, need - flags
    # the three ways out of the split mode
    fb = [r for r in S.RECORDS if "fallback" in r["reach"]]
    assert any(S.is_conv(r) and (r["x"][0][3] + r["cvec"]) % 32 for r in fb)
    assert any(S.is_conv(r) and r["w_offset"] for r in fb)
    assert any(not S.is_conv(r) for r in fb)


@pytest.mark.parametrize("planes", (1, 2, 3))
def test_probe_shapes_reach_every_instantiation(planes):
    lib = _lib.load()
    for bm, bn in S.FWD_TILES:
        s = S.probe_fwd(bn, planes)
        d = _lib.ConvDesc(ops.CONV_K1, s["B"], s["H"], s["H"], s["Cx"], 0, s["N"], 0, 0, s["Cx"], s["N"], 0, 0, s["N"], 1, 0, 0,
                          0, 0, 128, 0, 0)
        assert lib.s2i_conv_split_eligible(ctypes.byref(d)) == 1, lib.s2i_last_error()
        assert lib.s2i_conv_workspace_bytes(ctypes.byref(d)) == 0                  # K is not split: one launch, no reduction
        assert (128 if s["N"] > 64 else 64 if s["N"] > 32 else 32) == bn and s["Cx"] <= 64
    for tile in S.WG_TILES:
        s = S.probe_wgrad(tile, planes)
        plan = _lib.wgrad_plan(S.probe_wgrad_desc(s), planes=planes)
        assert plan["kernel"] == tile and plan["gz"] == 1 and plan["M"] <= 80, plan


# ---- the plane reference and the probe constants -----------------------------------------------------------------------
def test_split_reproduces_fp32_values_from_three_planes():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(4096, generator=g)
    planes, rest = S.split(v, 3)
    assert torch.equal(sum(p.double() for p in planes) + rest.double(), v.double())      # the residual is exact
    assert float((rest.abs() / v.abs()).max()) <= 2.0 ** -24                              # 3 x 8 significant bits
    for p in planes:
        assert torch.equal(p.bfloat16().float(), p)
    # round to nearest even: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 and goes to the even 1; 1 + 3 2^-8 to 1 + 2^-6
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)])
    (h,), r = S.split(ties, 1)
    assert h.tolist() == [1.0, 1 + 2.0 ** -6, -1.0] and r.tolist() == [2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8)]


def test_probe_operands_split_into_the_stated_planes():
    g = torch.Generator().manual_seed(7)
    v = S.probe_operand((64, 64), g, "cpu")
    assert float(v.min()) == S.PROBE_C / 4 and float(v.max()) == S.PROBE_C * 4
    assert torch.tensor(S.PROBE_C, dtype=torch.float32).double().item() == S.PROBE_C     # c is an fp32 number
    planes, rest = S.split(v, 3)
    assert not rest.any()
    scale = (v / S.PROBE_C).double()
    assert torch.equal(scale, torch.pow(2.0, torch.log2(scale).round()))
    for p, c in zip(planes, S.PROBE_PLANES):
        assert torch.equal(p.double(), c * scale)
    # every cross-product sum of a GEMM on such operands is probe_fraction(i, j) of every element of the result
    a, b = v.double(), S.probe_operand((64, 48), g, "cpu")
    pb, _ = S.split(b, 3)
    full = a @ b.double()
    for i in range(1, 4):
        for j in range(1, 4):
            part = planes[i - 1].double() @ pb[j - 1].double()
            assert torch.allclose(part.abs() / full, torch.full_like(full, S.probe_fraction(i, j)), rtol=1e-12, atol=0)


def test_probe_margins():
    """The fractions DESIGN.md section 5 quotes, and what makes the probe decisive: a kernel within gamma of the kept-product
    reference is further than gamma from every mutant as soon as the mutated term exceeds 2 gamma, and the terms a mode drops
    must not matter to the comparison of a mode that keeps them."""
    f = S.probe_fraction
    table = {(1, 1): 0.99, (1, 2): 2.9e-3, (2, 2): 8.6e-6, (1, 3): 3.8e-6, (2, 3): 1.1e-8, (3, 3): 1.4e-11}
    for (i, j), want in table.items():
        assert abs(f(i, j) / want - 1) < 0.07 and f(i, j) == f(j, i), (i, j, f(i, j))
    for planes in (1, 2, 3):
        g = max(C.GAMMA[S.probe_class(planes, "conv")], C.GAMMA[S.probe_class(planes, "wgrad")])
        assert min(f(i, j) for i, j in S.kept(planes)) > 2 * g, planes
        if planes < 3:
            assert sum(f(i, j) for i, j in S.next_order(planes)) > 2 * g, planes
    assert S.kept(3) == [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 1)] and S.next_order(3) == [(2, 3), (3, 2)]
    assert S.kept(2) == [(1, 1), (1, 2), (2, 1)] and S.next_order(2) == [(1, 3), (2, 2), (3, 1)]
    assert S.kept(1) == [(1, 1)] and S.next_order(1) == [(1, 2), (2, 1)]


# ---- the census --------------------------------------------------------------------------------------------------------
def test_step_census_in_split_mode_reaches_none_of_the_tails():
    """The gap the table closes, stated as a test (the argument of test_step_census_reaches_none_of_the_tails): planned with
    3 planes, no launch of the fp32 train step (tests/step_launches.json) on a spatial map has a partly filled row tile, a
    short pixel chunk or a column tail on a split tile.  The K1 launches on 1 x 1 maps (the fc layers, M = the batch; the
    fc's input gradient has N = 228) are the exception the census does hold, as there."""
    census = LH.load_census(os.path.join(HERE, "step_launches.json"))
    seen = {"conv": 0, "wgrad": 0}
    for rec in census["fp32_b24"]:
        what = json.dumps(rec, sort_keys=True)
        if rec["fn"] == "conv_raw":
            rec = dict(rec, tile_rows=128, tune={}, reach=[])
            if rec["w"]["oihw"] is None or not S.conv_eligible(rec):
                continue
            B, H, W, _ = rec["x"][0]
            Ho, Wo = E._geom(rec["kind"], H, W)
            if H * W == 1:
                continue
            BN = 128 if rec["N"] > 64 else (64 if rec["N"] > 32 else 32)
            assert rec["N"] % BN == 0 and (B * Ho * Wo) % 128 == 0, what
            seen["conv"] += 1
        elif rec["fn"] == "wgrad_raw":
            plan = _lib.wgrad_plan(E.wgrad_desc(rec), planes=3)
            if not plan["kernel"].startswith("split-"):
                continue
            B, H, W, _ = rec["a"][0]
            if H * W == 1:
                continue
            assert rec["g"][0][3] % plan["bn"] == 0 and plan["M"] % 32 == 0, what
            seen["wgrad"] += 1
    assert seen["conv"] > 20 and seen["wgrad"] > 20, seen
