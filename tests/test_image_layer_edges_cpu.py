"""The image-layer table (tests/image_layer_edges.py) reaches the dispatch branches it claims, and the censuses do not.

image_layer_edges.conv_plan / wgrad_plan ask the library which kernel a launch takes (s2i_conv_plan_query,
s2i_wgrad_plan_query: the library loads and plans without a device) and only rename it and describe the input: pixel tail
and strided grid from the reported pixels per block and grid, H != W, bias, N = 3, the gate M.  What the Python restatement
of the dispatch said of every forward record before the query existed is kept in tests/golden/fwd_record_plans.json and
compared in tests/test_fwd_plan_cpu.py.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_edges as E  # noqa: E402
import image_layer_edges as IE  # noqa: E402
import launch_harness as LH  # noqa: E402

IDS = [IE.record_id(i, r) for i, r in enumerate(IE.RECORDS)]

# what no launch of the step census or the B = 23 census reaches
NEVER_LAUNCHED = ("thin-out", "thin-out-4phase", "rgb-out-k4", "rgb-out-k8", "rgb-out-k16", "rgb-out-k9", "rgb-out-k18",
                  "rgb-out-k36", "rgb-in-1x4", "small-n-16", "n4-igemm")
# ... and what the operator tests aimed at these layers (test_kernels_gpu.CONVACT in fp32, test_bf16_gpu.IMAGE_LAYERS in bf16
# activation mode) do not reach either: they do launch rgb_out_kernel<8> and <36>, rgb_in_kernel<1,4> and
# small_n_conv_kernel<16>, at 1.5e-2 relative L2 or close()
NO_OPERATOR_TEST = ("thin-out", "thin-out-4phase", "rgb-out-k4", "rgb-out-k16", "rgb-out-k9", "rgb-out-k18")


def test_record_ids_and_records_are_distinct():
    assert len(set(IDS)) == len(IDS)
    canon = [LH.canon(r) for r in IE.RECORDS]
    assert len(set(canon)) == len(canon)
    for rec in IE.RECORDS:
        assert rec["why"] and set(rec["reach"]) <= set(IE.REACH), rec
    # the conv-edge table is untouched by the constructors here
    assert not any("ldy" in r for r in E.RECORDS)


@pytest.mark.parametrize("index", range(len(IE.RECORDS)), ids=IDS)
def test_record_reaches_what_it_claims(index):
    rec = IE.RECORDS[index]
    plan = IE.plan(rec)
    assert set(rec["reach"]) == plan["reach"], (IDS[index], plan)
    # the shapes stay small: operands and result of a record under about 40 MB
    if "x" in rec:
        B, H, W, C = rec["x"][0]
        nbytes = B * H * W * C * (2 if rec["x"][1] == "bf16" else 4) + plan["M"] * plan["nphases"] * rec.get("ldy", rec["N"]) * 4
    else:
        B, H, W, C = rec["a"][0]
        nbytes = B * H * W * (C * (2 if rec["a"][1] == "bf16" else 4) + 16)
    assert nbytes <= 40 << 20, (IDS[index], nbytes)


def test_table_claims_every_branch_and_edge():
    claimed = set()
    for rec in IE.RECORDS:
        claimed |= set(rec["reach"])
    missing = [f for f in IE.REACH if f not in claimed]
    assert not missing, "no record of tests/image_layer_edges.py reaches: %s" % missing

    def has(branch, edge):
        return any(branch in r["reach"] and edge in r["reach"] for r in IE.RECORDS)

    for branch in IE.BRANCHES:
        if branch == "wg-n4-igemm":
            continue                                     # the matrix tiles: tests/conv_edges.py
        if branch != "n4-igemm":
            assert has(branch, "nonsquare"), "%s without a record on a map with H != W" % branch
        if branch in IE.PIXEL_LOOP:
            assert has(branch, "pixtail"), "%s without a pixel tail" % branch
        if branch.startswith("wg-small-n"):
            assert has(branch, "odd-trip") and has(branch, "threshold"), branch
            for dt in ("f32", "bf16"):
                assert any(branch in r["reach"] and r["a"][1] == dt for r in IE.RECORDS), (branch, dt)
    # both input dtypes of the tile kernels; both forms of the 4-phase kernels; bias, n3 and the gate on each epilogue family
    for branch in ("tile3-16", "tile3-32", "tile3-64", "tile-tconv64"):
        for dt in ("f32", "bf16"):
            assert any(branch in r["reach"] and r["x"][1] == dt for r in IE.RECORDS), (branch, dt)
    for branch in ("thin-out", "rgb-out-k9"):
        assert has(branch, "n3") and has(branch, "threshold"), branch
    for prefix in ("thin-out", "thin-in", "rgb-out", "small-n", "tile3"):
        assert any("bias" in r["reach"] and any(b.startswith(prefix) for b in r["reach"]) for r in IE.RECORDS), prefix
    assert any("thin-in-16" in r["reach"] and "bias" in r["reach"] and r.get("out_dtype") == "bf16" for r in IE.RECORDS), \
        "the biased bf16 launch that rgb_in declines"
    for branch in ("rgb-out-k4", "small-n-16"):
        assert has(branch, "grid-cap"), branch


@pytest.mark.parametrize("census", ["step_launches.json", "ragged_launches.json"])
def test_censuses_reach_none_of_the_never_launched_kernels(census):
    """The gap the table closes, stated as a test: it fails (and is to be updated) when a production shape starts to
    launch one of these kernels.  Maps of 64 x 64 and larger go to the tile kernels (fp32 or bf16 input), 64 output channels
    of the first discriminator conv to rgb_in_kernel<2, 4>, GET_IMAGE_G's input gradient at 64 channels to <2, 3>."""
    data = LH.load_census(os.path.join(HERE, census))
    assert data
    seen, edges = {}, set()
    for mode, recs in data.items():
        for rec in recs:
            if not IE.in_family(rec):
                continue
            plan = IE.plan(dict(rec, tile_rows=0, tune={}))
            seen.setdefault(plan["branch"], []).append(mode)
            edges |= plan["reach"] & set(IE.EDGES)
            shape = (rec["x"] if "x" in rec else rec["a"])[0]
            assert shape[1] == shape[2] and shape[1] >= 32, rec
    print("%s: %s" % (census, {k: len(v) for k, v in sorted(seen.items())}))
    hit = sorted(set(seen) & set(NEVER_LAUNCHED))
    assert not hit, "%s launches %s" % (census, hit)
    assert {"tile3-16", "tile3-32", "tile3-64", "tile-tconv64", "rgb-in-2x4"} <= set(seen), sorted(seen)
    # large maps do stride the grid, and 23 images end the weight-gradient stream on a single-group trip
    edges -= {"grid-cap", "odd-trip"}
    assert not edges, "%s reaches the edges %s" % (census, sorted(edges))


def test_operator_tests_reach_none_of_the_unlaunched_kernels():
    """The same derivation over the ConvAct cases of the two operator tests that aim at the image layers.  thin_in_kernel
    writes bf16 only where rgb_in declines a bias, and small_n_wgrad_kernel reads bf16 activations only for a direct caller
    of ops.wgrad_any (ops._wgrad pads the image gradient and takes the matrix cores): no case has either."""
    import test_bf16_gpu
    import test_kernels_gpu
    act = test_kernels_gpu.ACT
    seen = {}
    cases = [(c[0], c[1], c[2], c[3], c[5], c[6], act[c[7]], c[8], False) for c in test_kernels_gpu.CONVACT if c[0] != "k1"]
    cases += [(c[0], c[1], c[2], c[3], c[5], c[6], act[c[7]], False, True) for c in test_bf16_gpu.IMAGE_LAYERS]
    for case in cases:
        for rec in IE.convact_launches(*case):
            plan = IE.plan(rec)
            seen.setdefault(plan["branch"], set()).add((rec.get("out_dtype"), (rec.get("a") or [0, 0])[1]))
            print(case, rec["why"], plan["branch"])
    hit = sorted(set(seen) & set(NO_OPERATOR_TEST))
    assert not hit, "an operator test launches %s" % hit
    assert {"rgb-out-k8", "rgb-out-k36", "rgb-in-1x4", "small-n-16"} <= set(seen), sorted(seen)
    assert all(o == "f32" for b in ("thin-in-16", "thin-in-32") for o, _ in seen.get(b, ())), seen
    assert all(a == "f32" for b in seen if b.startswith("wg-small-n") for _, a in seen[b]), seen
