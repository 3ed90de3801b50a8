"""The bf16 convolution planner answers what it answered when tests/golden/bf16_plans.npz was recorded.

plan_bf16 is host code and the library loads without a device: the five planner queries are recomputed over the grid of
tests/golden/make_golden_bf16_plans.py (three kinds, batches 1 - 144, maps 4 - 128, every tile width, with and without
BatchNorm groups and split-K, under the default knobs and b16_v2 = 0 / 2) and must equal the stored table exactly,
ineligible rows and the refusing S2I_REQUIRE family included.  No GPU."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_golden_bf16_plans", os.path.join(GOLDEN, "make_golden_bf16_plans.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)  # defines functions only; the library is loaded by compute()


def _stored():
    with np.load(os.path.join(GOLDEN, "bf16_plans.npz")) as z:
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
