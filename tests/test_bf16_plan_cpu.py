"""The bf16 convolution planner answers what it answered when tests/golden/bf16_plans.npz was recorded.

plan_bf16 is host code and the library loads without a device: s2i_conv_bf16_plan_query is asked over the grid of
tests/golden/make_golden_bf16_plans.py (three kinds, batches 1 - 144, maps 4 - 128, every tile width, with and without
BatchNorm groups and split-K, under the default knobs, b16_v2 = 0 / 2 and the knobs the GPU tests force) and must equal
the stored table exactly: kernel, grid and tile count, ineligible rows and the refusing S2I_REQUIRE family included.  What
the GPU suites launch reaches every instantiation the planner can name.  No GPU."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
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


def test_gpu_suites_launch_every_bf16_kernel():
    """The forward and input-gradient launches of test_bf16_gpu.CONV_CASES / V2_CASES (the latter under the knobs that test
    forces) and the bf16 records of the edge table that test_conv_edges_gpu replays plan onto every name of B16_KERNELS."""
    import conv_edges as E
    import test_bf16_gpu as T
    from speech_to_image_translation_without_text_amd import _lib
    seen = set()

    def note(rec):
        told = _lib.conv_bf16_plan(E.conv_desc(rec))
        assert told is not None and told["kernel"] is not None, (rec, told)
        # the name (B16_KERNELS follows the B16Kernel enum) says what the plan's own fields say
        kind = {_lib.CONV_K3S1: "k3s1", _lib.CONV_K4S2: "k4s2", _lib.TCONV_K4S2: "tconv"}[rec["kind"]]
        if told["pixels"] == 128:
            assert told["kernel"] == "b16-%s-%dx%d" % (kind, told["bn"], told["ck"]) and told["threads"] == 256, told
        else:
            assert told["kernel"] in ("b16v2-" + kind, "b16v2-%s-pw66" % kind) and (told["bn"], told["threads"]) == (128, 512), told
        seen.add(told["kernel"])

    for cases, knobs in ((T.CONV_CASES, {}), (T.V2_CASES, dict(b16_v2=2, b16_persist=4))):
        with _lib.tuning(**knobs):
            for kind, B, H, Cin, Cout in cases:
                note(E.fwd(kind, B, H, Cin, Cout, "forward", [], bf16=True))
                note(E.dgrad(kind, B, H, Cin, Cout, "input gradient", [], bf16=True))
    for rec in E.RECORDS:
        if rec.get("fast"):
            with _lib.tuning(**rec["tune"]):
                note(rec)
    missing = [k for k in _lib.B16_KERNELS if k not in seen]
    assert not missing, "no bf16 GPU test launches: %s" % missing
