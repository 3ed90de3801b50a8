"""The fp32 forward planner answers what it answered when tests/golden/conv_plans.npz was recorded.

plan_fwd is host code and the library loads without a device: the workspace, statistics-row and split-eligibility queries
are recomputed over the grid of tests/golden/make_golden_conv_plans.py (five kinds, batches 1 - 144, maps 1 - 128, channel
counts off every tile width, a broadcast vector, BatchNorm groups, nosplit, both weight layouts, under the default knobs,
fwd_bm = 96 / 128 and fwd_min_cps = 2) and must equal the stored table exactly, the refusing S2I_REQUIRE family included.
No GPU."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_golden_conv_plans", os.path.join(GOLDEN, "make_golden_conv_plans.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)  # defines functions only; the library is loaded by compute()


def _stored():
    with np.load(os.path.join(GOLDEN, "conv_plans.npz")) as z:
        assert set(z.files) == set(G.COLUMNS)
        return np.stack([z[c] for c in G.COLUMNS], axis=-1)


def test_plans_equal_the_recorded_table():
    want, got = _stored(), G.compute()
    assert want.shape == got.shape == (len(G.KNOBS), len(G.GRID), len(G.COLUMNS))
    bad = np.argwhere((want != got).any(axis=-1))
    lines = ["%s: recorded %s, planned %s" % (G.describe(G.GRID[i], G.KNOBS[k]), dict(zip(G.COLUMNS, want[k, i].tolist())),
                                              dict(zip(G.COLUMNS, got[k, i].tolist()))) for k, i in bad[:10]]
    assert not len(bad), "%d plans changed:\n%s" % (len(bad), "\n".join(lines))


def test_recorded_table_reaches_the_planner_branches():
    seen = G.reached(_stored())
    missing = [b for b in G.REQUIRED if b not in seen]
    assert not missing, missing
