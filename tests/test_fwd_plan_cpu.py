"""s2i_conv_plan_query names what every forward convolution launches, and says what the tests used to restate.

plan_fwd (csrc/s2i_conv_plan.hip) is host code and the library loads without a device.  Checked here, without a GPU:

  * every forward record of tests/conv_edges.py and tests/image_layer_edges.py reaches what tests/golden/fwd_record_plans.json
    recorded at the commit before the query existed, when the two helper modules still restated the dispatch in Python.  The
    query may only add information: where the parent could not tell 96-row from 128-row tiles (bm = null) the height is
    now known, must be 128 for N <= 64, and the record's reach may gain the row tail of that height and nothing else;
  * over GRID x KNOBS of tests/golden/make_golden_conv_plans.py, s2i_conv_workspace_bytes against the largest workspace the
    query reports over the operand modes (see test_workspace_query_covers_every_mode for the one family of layers where
    the two differ, and by how much), s2i_conv_stat_parts against the grid and reduction the query reports, and the refusals
    of the stored table against the query's;
  * every FwdKernel value is planned for some row, record or EXTRA descriptor, except the two that no plan names any more.
"""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_golden_conv_plans", os.path.join(GOLDEN, "make_golden_conv_plans.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

import conv_edges as E  # noqa: E402
import image_layer_edges as IE  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib  # noqa: E402

with open(os.path.join(GOLDEN, "fwd_record_plans.json")) as _f:
    STORED = json.load(_f)

F = {f: i for i, f in enumerate(_lib.FWD_PLAN_FIELDS)}
# operand modes of a descriptor: (x dtype, y dtype, planes); planes = 3 only where s2i_conv_split_eligible
DTYPE_MODES = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0))
MATRIX = tuple(k for k in _lib.FWD_KERNELS if k.startswith(("f32-", "f32in-", "split-")))
# every kernel the forward can launch is planned somewhere below ...
REQUIRED = tuple(k for k in _lib.FWD_KERNELS if k not in ("smalln-4", "smalln-8"))
# ... except small_n_conv_kernel<4> and <8>: 16 / 32 channels never split K (at most 9 chunks), so thin_out_kernel takes every
# layer they qualify for.  Before the plan stopped looking at the workspace they were what a caller who passed none got; the
# instantiations stay in the library (the device code is unchanged) and the launcher keeps their case.
UNPLANNED = ("smalln-4", "smalln-8")
# what neither the grid (its N are 4, 40, 64 and 136) nor a record reaches: apply-on-load on the 128 x 32 tile
EXTRA = (dict(kind=G.K3S1, B=8, H=16, W=16, Cx=32, Cc=0, N=16, wmode=0, flip=0, wR=32, ldw=16, act=0, stats=1, ldy=16, groups=1,
              nosplit=0, in_act=_lib.ACT_LRELU, in_groups=1),)


def _stored_rows(suite):
    return [pytest.param(row, id=row["id"]) for row in STORED[suite]]


def test_stored_file_names_its_parent_and_holds_every_forward_record():
    assert len(STORED["recorded_at"]) == 40 and int(STORED["recorded_at"], 16)
    for suite, mod in (("conv_edges", E), ("image_layer_edges", IE)):
        want = [i for i, r in enumerate(mod.RECORDS) if r["fn"].startswith("conv") and not r["fast"]]
        assert [row["i"] for row in STORED[suite]] == want, suite
        assert [row["id"] for row in STORED[suite]] == [mod.record_id(i, mod.RECORDS[i]) for i in want], suite


@pytest.mark.parametrize("row", _stored_rows("conv_edges"))
def test_conv_edge_record_plans_as_recorded(row):
    rec = E.RECORDS[row["i"]]
    plan = E.conv_plan(rec)
    for f in ("M", "nphases", "K", "nchunks", "splitk", "cps", "BN"):
        assert plan[f] == row[f], (f, plan, row)
    if row["bm"] is not None:
        assert plan["bm"] == row["bm"] and sorted(plan["reach"]) == row["reach"], (plan, row)
        return
    # the parent could not tell the height: the query does, and only the row tail of that height may be new
    assert plan["bm"] in (96, 128) and (rec["N"] > 64 or plan["bm"] == 128), plan
    gained = plan["reach"] - set(row["reach"])
    assert set(row["reach"]) <= plan["reach"] and gained <= {"rowtail-%d" % plan["bm"], "rowtail-4phase"}, (plan, row)
    assert not gained or plan["M"] % plan["bm"], (plan, row)


@pytest.mark.parametrize("row", _stored_rows("image_layer_edges"))
def test_image_layer_record_plans_as_recorded(row):
    plan = IE.conv_plan(IE.RECORDS[row["i"]])
    for f in ("branch", "M", "nphases", "splitk", "ppb", "blocks", "Ho", "Wo"):
        assert plan[f] == row[f], (f, plan, row)
    assert sorted(plan["reach"]) == row["reach"], (plan, row)


def _query(lib, d, mode, out):
    x16, y16, planes = mode
    return None if lib.s2i_conv_plan_query(d, x16, y16, planes, 0, 0, ctypes.byref(out)) else list(out)


@pytest.fixture(scope="module")
def sweep():
    """Over GRID x KNOBS: the fp32 plan (or the refusal text), the largest ws_bytes over the modes, the three queries, and the
    kernels seen; apply-on-load (d.in_act) is asked under the default knobs only."""
    lib = _lib.load()
    out = (ctypes.c_int * 15)()
    rows, seen = [], set()
    for k, knobs in enumerate(G.KNOBS):
        with _lib.tuning(**knobs):
            for i, row in enumerate(G.GRID):
                desc = G.descriptor(_lib, row)
                d = ctypes.byref(desc)
                f32 = _query(lib, d, DTYPE_MODES[0], out)
                if f32 is None:
                    rows.append((k, i, None, lib.s2i_last_error().decode(), 0, lib.s2i_conv_workspace_bytes(d),
                                 lib.s2i_conv_stat_parts(d)))
                    continue
                modes = DTYPE_MODES[1:] + (((0, 0, 3),) if lib.s2i_conv_split_eligible(d) else ())
                plans = [f32] + [p for p in (_query(lib, d, m, out) for m in modes) if p is not None]
                seen.update(p[F["kernel"]] for p in plans)
                rows.append((k, i, f32, "", max(p[F["ws_bytes"]] for p in plans), lib.s2i_conv_workspace_bytes(d),
                             lib.s2i_conv_stat_parts(d)))
                if k == 0 and row[5] == 0 and row[8] == 0:          # no broadcast vector, forward weight layout
                    desc.in_act, desc.in_groups = _lib.ACT_LRELU, 1
                    p = _query(lib, d, DTYPE_MODES[0], out)
                    if p is not None:
                        seen.add(p[F["kernel"]])
    return rows, {_lib.FWD_KERNELS[s] for s in seen}


def _stored_table():
    with np.load(os.path.join(GOLDEN, "conv_plans.npz")) as z:
        return {c: z[c] for c in G.COLUMNS}


def test_workspace_query_covers_every_mode(sweep):
    """s2i_conv_workspace_bytes(d) is never short of what any mode's plan asks for, and equals the largest of them on every
    row but one family: N <= 4 layers that a tile kernel (tconv_n4_tile / conv3_n4_tile) takes with bf16 input.  There the
    query has always also counted rgb_out_kernel's fragment buffer, which the dispatch order never reaches while the tile
    kernel qualifies (a 3x3 from Ca channels: 576 Ca bytes counted, 144 Ca asked for; the transposed conv from 64: 65536
    against 16384).  tests/golden/conv_plans.npz pins those values, so they stay: on those rows the query must equal that
    fragment buffer, nph x (K / 16) x 64 lanes x 8 bf16."""
    rows, _ = sweep
    table = _stored_table()
    over = 0
    for k, i, f32, _, modes_max, ws, _ in rows:
        assert ws == table["workspace"][k, i]
        if f32 is None:
            assert ws == 0
            continue
        assert ws >= modes_max, (G.describe(G.GRID[i], G.KNOBS[k]), ws, modes_max)
        if ws != modes_max:
            kind, B, HW, Cx, N, Cc = G.GRID[i][:6]
            name = _lib.FWD_KERNELS[f32[F["kernel"]]]
            assert name in ("tconv-n4-64", "conv3-n4-32") and N <= 4 and Cc == 0, (G.describe(G.GRID[i], G.KNOBS[k]), name)
            assert ws == (4 if kind == G.TCONV else 1) * (f32[F["K"]] // 16) * 64 * 8 * 2, (G.describe(G.GRID[i], G.KNOBS[k]), ws)
            over += 1
    assert over, "the grid holds tile-kernel layers"


def test_stat_parts_follow_from_the_planned_grid_and_reduction(sweep):
    """Unsplit, the matrix kernel's epilogue writes one statistics row per row tile and phase: grid x times grid z.  Split,
    the reduction writes them: per BatchNorm group one row per 8 output rows, 512 rows at most over all groups."""
    rows, _ = sweep
    for k, i, f32, _, _, _, parts in rows:
        if f32 is None:
            assert parts == -1
            continue
        stats, groups = G.GRID[i][6]
        if _lib.FWD_KERNELS[f32[F["kernel"]]] not in MATRIX:
            assert not stats                                          # the vector-unit kernels have no statistics epilogue
            continue
        if f32[F["reduce"]] == _lib.FWD_REDUCE_NONE:
            assert f32[F["splitk"]] == 1 and parts == f32[F["gx"]] * f32[F["gz"]], (G.describe(G.GRID[i], G.KNOBS[k]), f32, parts)
        else:
            want = (_lib.FWD_REDUCE_PLAIN if not stats else
                    _lib.FWD_REDUCE_STATS if G.GRID[i][4] % 4 == 0 else _lib.FWD_REDUCE_COLSTATS)
            mrows = f32[F["M"]] * f32[F["gz"]] // f32[F["splitk"]]
            per_group = max(1, min(-(-(mrows // groups) // 8), 512 // groups))
            assert f32[F["reduce"]] == want and f32[F["splitk"]] > 1 and parts == per_group * groups, \
                (G.describe(G.GRID[i], G.KNOBS[k]), f32, parts)


def test_refusals_are_the_recorded_ones(sweep):
    rows, _ = sweep
    error = _stored_table()["error"]
    for k, i, f32, msg, _, _, _ in rows:
        code = int(error[k, i])
        if code:
            assert f32 is None and G.ERRORS[code - 1] in msg, (G.describe(G.GRID[i], G.KNOBS[k]), code, msg)
        else:
            assert f32 is not None, (G.describe(G.GRID[i], G.KNOBS[k]), msg)


def test_every_kernel_is_planned_somewhere(sweep):
    _, seen = sweep
    seen = set(seen)
    for mod in (E, IE):
        for rec in mod.RECORDS:
            if rec["fn"].startswith("conv") and not rec["fast"]:
                d = E.conv_desc(rec, ldy=rec.get("ldy", rec["N"]))
                with _lib.tuning(**rec.get("tune", {})):
                    seen.add(_lib.conv_plan(d, int(rec["x"][1] == "bf16"), int(rec["out_dtype"] == "bf16"), 0, rec["bias"],
                                            rec["cls_bias"])["kernel"])
    for f in EXTRA:
        seen.add(_lib.conv_plan(_lib.ConvDesc(**f))["kernel"])
    assert set(REQUIRED) | set(UNPLANNED) == set(_lib.FWD_KERNELS)
    missing = [k for k in REQUIRED if k not in seen]
    assert not missing, "no grid row, record or EXTRA descriptor plans: %s" % missing
    assert not set(UNPLANNED) & seen, "planned after all: %s" % sorted(set(UNPLANNED) & seen)


def test_refused_query_zeroes_its_output():
    lib = _lib.load()
    out = (ctypes.c_int * 15)(*range(1, 16))
    bad = _lib.ConvDesc(_lib.CONV_K3S1, 2, 6, 6, 8, 0, 16, 0, 0, 8, 16, 0, 0, 16, 1, 0)       # 6 x 6 is no power of two
    assert lib.s2i_conv_plan_query(ctypes.byref(bad), 0, 0, 0, 0, 0, ctypes.byref(out)) != 0 and not any(out)
    assert b"powers of two" in lib.s2i_last_error()
    ok = _lib.ConvDesc(_lib.CONV_K3S1, 2, 8, 8, 64, 0, 128, 0, 0, 64, 128, 0, 1, 128, 1, 0)
    assert _lib.conv_plan(ok)["kernel"] == "f32-128x128"
    assert _lib.conv_plan(ok, _lib.DT_BF16, _lib.DT_F32, planes=2) is None                      # split planes take fp32 tensors
    assert _lib.conv_plan(ok, cls_bias=True) is None and b"class bias" in lib.s2i_last_error()   # the plan splits K


def test_planner_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/fwd_plan_host_check.cpp: the planner's host units linked into a stand-alone program with AddressSanitizer and
    UndefinedBehaviorSanitizer, asked some 700 000 questions (most of them refused) on the CPU.  It exits non-zero on a
    sanitizer report, on a kernel id outside the table, on a refusal that leaves its output set, or on a plan that asks for
    more workspace than s2i_conv_workspace_bytes reports."""
    import subprocess
    csrc = os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc")
    exe = str(tmp_path / "fwd_plan_host_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "fwd_plan_host_check.cpp"),
                           os.path.join(csrc, "s2i_conv_plan.hip"), os.path.join(csrc, "s2i_runtime.hip"), "-o", exe], cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "planned onto" in run.stdout, run.stdout
