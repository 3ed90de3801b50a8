"""Every convolution launch of the train step, at its production shape, against a plain fp64 reference.

The kernels' variants (fp32 96 / 128-row tiles and split-K, weight-gradient tile shapes, the bf16 load-aware K split,
the persistent 256-pixel kernel, XCD remapping, BatchNorm partial sums per group) are chosen by the C planners from the
launch's shape, so they are tested here at the shapes the step really launches, with the default planner:

  * census: one eager train_step of each BASELINE workload (config 2: fp32, batch 24; config 4: bf16 activations,
    batch 48) with the four dispatchers of ops.py wrapped; each call's full argument description, deduplicated, is
    tests/step_launches.json.  test_census_matches_committed_file fails on any new or vanished launch, so a new shape
    shows up as a diff of that file.  Regenerate it with `python tests/test_step_launches_gpu.py`.
  * replay: every census entry re-run through the same dispatcher on fresh seeded operands.  Weights are integers in
    [-16, 16] times 2^-6, so their bf16 rounding and the up-block's 4-tap fold sums are exact; bf16 activations are
    drawn as bf16.  The reference (tests/launch_ref.py) sees exactly the values the kernel sees.
  * bound, element-wise: |out - ref| <= rnd * |ref| + gamma * absref, rnd = 2^-8 for a bf16 output and 0 for fp32,
    absref = the same operation on |operands| in fp64, gamma one constant per (matrix-core type, forward | weight
    gradient), at about 2x the worst ratio measured.  BatchNorm partial sums (summed per group) and accumulation into a
    prefilled gradient (the written slice = prefill + gradient, every other element bit-identical) are checked too.
  * power: the same comparison must FAIL against a reference with one input channel's contribution removed (a dropped
    K chunk) and, for weight gradients, one image's contribution removed (a dropped pixel-range split).

At these shapes every GEMM is a whole number of row tiles, pixel chunks and bf16 image tiles; partly filled tiles, tails
and the ragged 23-image batch are tests/test_conv_edges_gpu.py's.
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

import conv_replay as C  # noqa: E402
import launch_harness as LH  # noqa: E402
import launch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CENSUS_FILE = os.path.join(HERE, "step_launches.json")

MODES = LH.STEP_MODES

LEDGER = LH.Ledger()


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("step launch replay")


# ---- census ----------------------------------------------------------------------------------------------------------
def take_census(gpu):
    """{mode: deduplicated, sorted list of launch records}, and {mode: launches per step}: one eager train_step of each
    workload with the dispatchers of ops.py wrapped."""
    return LH.take_step_census(gpu, MODES, C.wrap_dispatchers)


def test_census_matches_committed_file(gpu):
    live, calls = take_census(gpu)
    for mode, recs in live.items():
        print("census %s: %d dispatcher calls per step, %d distinct launches" % (mode, calls[mode], len(recs)))
    LH.assert_census_equal(live, LH.load_census(CENSUS_FILE), MODES, "step_launches.json")


# ---- replay ----------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for mode, recs in LH.load_census(CENSUS_FILE).items():
        for i, rec in enumerate(recs):
            op, layer = R.layer_op(rec)
            out.append(pytest.param(mode, i, id="%s-%03d-%s-%s-%s" % (mode, i, rec["fn"], op, layer)))
    return out


@pytest.mark.parametrize("mode,index", _cases())
def test_launch_replay_matches_fp64(gpu, mode, index):
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0, "the replay runs the default planner"
    assert os.environ.get("S2I_TUNE", "") == "", "the replay runs the default planner"
    rec = LH.load_census(CENSUS_FILE)[mode][index]
    what = "%s[%d] %s %s" % (mode, index, rec["fn"], "%s/%s" % R.layer_op(rec))
    with torch.no_grad():
        (C.replay_conv if rec["fn"].startswith("conv") else C.replay_wgrad)(rec, LH.gen_rec(gpu, rec), gpu, what, LEDGER)
    torch.cuda.empty_cache()


def test_fp64_reference_gpu_equals_cpu(gpu):
    """The fp64 reference computed by torch on the GPU equals the CPU one (small shapes, every operation and layer)."""
    g = torch.Generator().manual_seed(5)
    for layer in R.LAYERS:
        kh = {"k1": 1, "k3s1": 3, "k4s2": 4, "up": 3}[layer]
        x = torch.randn(3, 6, 8, 8, generator=g, dtype=torch.float64)
        w = torch.randn(5, 6, kh, kh, generator=g, dtype=torch.float64)
        y = R.fwd(layer, x, w)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        for name, fn, args in (("fwd", R.fwd, (x, w)), ("dgrad", R.dgrad, (dy, w)), ("wgrad", R.wgrad, (x, dy, kh))):
            c = fn(layer, *args)
            d = fn(layer, *[t.to(gpu) if torch.is_tensor(t) else t for t in args]).cpu()
            assert torch.allclose(c, d, rtol=1e-12, atol=1e-12), (layer, name, float((c - d).abs().max()))


if __name__ == "__main__":
    # regenerate tests/step_launches.json (or the path given) from one eager step of each workload
    from speech_to_image_translation_without_text_amd import _lib
    _lib.load()
    _lib.require_device()
    census, calls = take_census(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else CENSUS_FILE
    LH.write_census(path, census)
    for mode, recs in census.items():
        print("census %s: %d dispatcher calls per step, %d distinct launches -> %s" % (mode, calls[mode], len(recs), path))
