"""The weight-gradient planner answers what it answered when tests/golden/wgrad_plans.npz was recorded.

plan_wgrad is host code and the library loads without a device: the three workspace queries, the apply-on-load
eligibility and the twelve outputs of s2i_wgrad_plan_query are recomputed over the grid of
tests/golden/make_golden_wgrad_plans.py (1x1, 3x3, stride-2 and the up layer's swapped and folded gradient, batches
1 - 144, maps 1 - 128, channel counts on and off every tile width, a broadcast vector, a gradient row stride wider than N;
fp32, one or both operands bf16, 1 - 3 split planes, apply-on-load with 1 and 3 groups; the default knobs and every forced
tile of wgrad_bm / wgrad16_bm) and must equal the stored table exactly, the refusing S2I_REQUIRE family included.  No GPU."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_golden_wgrad_plans", os.path.join(GOLDEN, "make_golden_wgrad_plans.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)  # defines functions only; the library is loaded by compute()


def _stored():
    with np.load(os.path.join(GOLDEN, "wgrad_plans.npz")) as z:
        assert set(z.files) == set(G.COLUMNS)
        return np.stack([z[c] for c in G.COLUMNS], axis=-1).astype(np.int64)


def test_plans_equal_the_recorded_table():
    want, got = _stored(), G.compute()
    assert want.shape == got.shape == (len(G.GRID), len(G.SETTINGS), len(G.COLUMNS))
    bad = np.argwhere((want != got).any(axis=-1))
    lines = ["%s: recorded %s, planned %s" % (G.describe(G.GRID[i], G.SETTINGS[k]), dict(zip(G.COLUMNS, want[i, k].tolist())),
                                              dict(zip(G.COLUMNS, got[i, k].tolist()))) for i, k in bad[:10]]
    assert not len(bad), "%d plans changed:\n%s" % (len(bad), "\n".join(lines))


def test_recorded_table_reaches_the_planner_branches():
    seen = G.reached(_stored())
    missing = [b for b in G.REQUIRED if b not in seen]
    assert not missing, missing


def test_kernel_names_follow_the_binding():
    from speech_to_image_translation_without_text_amd import _lib
    assert G.KERNELS == _lib.WGRAD_KERNELS and G.PLAN == _lib.WGRAD_PLAN_FIELDS
    d = _lib.WgradDesc(_lib.CONV_K4S2, 144, 64, 64, 128, 0, 256, 256, 0, 0, 256, 128, 4, 4, 1, 0, 0, 0, 0)
    plan = _lib.wgrad_plan(d, _lib.DT_BF16, _lib.DT_BF16)
    assert plan["kernel"] in ("b16-256x128", "b16-256x256") and plan["stage"] == 64 and plan["K"] == 2048
    assert plan["slabs"] == plan["gz"] <= plan["ws_slabs"]
    assert _lib.wgrad_plan(d, _lib.DT_BF16, _lib.DT_F32, planes=2) is None      # split planes take fp32 tensors
