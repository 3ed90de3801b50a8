"""The split-bf16 matrix kernels (ops.MATH_PLANES; igemm_fwd_split_kernel, igemm_wgrad_split_kernel, split_packed_kernel)
against fp64, launch by launch and plane by plane.

The launch-replay and edge suites run with MATH_PLANES = 0, and the tests that do run the mode (the [bf16x3] whole-step
tests, test_split_bf16_products_against_fp64) bound a mean or a relative error of 2e-4 and more: a three-plane kernel
that runs as two planes, or drops one of a1 b3, a2 b2, a3 b1, passes them.  This module has four parts.

  * Replay.  Every record of tests/split_planes.py (tests/test_split_planes_cpu.py derives what each one reaches) runs
    through conv_replay.replay_conv / replay_wgrad under MATH_PLANES = 3 with N(0, 1) / (k sqrt(I)) weights of full 24-bit
    significands, and under MATH_PLANES = 1 with every operand on the bf16 grid (there each product is exact, as on the bf16
    matrix path), with the replay's dropped-channel and dropped-image mutants, the last row left out of the BatchNorm sums
    and the dropped short last K split of tests/test_conv_edges_gpu.py.  A spy on the library asserts that the split entry
    point ran exactly once and the native one not at all; for the fallback records, which hold the native fp32 bound, the
    opposite.  (The <= 4 channel weight gradient falls back inside s2i_conv_wgrad_split, which ops.wgrad_raw calls for every
    layer in a split mode: there the plan query names the fp32 stream kernel and the spy sees the split entry point.)
  * Plane probe.  Random operands cannot find a missing third-order product: its largest contribution to an output element
    falls from 2.4e-6 x absref at K = 64 to 3e-7 at K = 4608, inside the bound above a few hundred K.  The probe operands are
    c 2^e > 0, c = 1 + 3 2^-10 + 3 2^-18 with the planes (1, 3 2^-10 + 2^-16, -2^-18), so every cross-product sum is a fixed
    fraction of every output element (a1 b2 2.9e-3, a2 b2 8.6e-6, a1 b3 3.8e-6, a2 b3 1.1e-8).  One K1 launch per
    instantiation (3 forward and 4 weight-gradient tiles x 1, 2, 3 planes) is compared with the fp64 sum of exactly the
    products the mode keeps; the comparison must FAIL against that reference without any one kept product, and for 1 and 2
    planes against the reference with the next order added.
  * Weight splitter.  s2i_split_packed_weight at three shapes, 1 to 3 planes, both outputs together and each alone, bit for
    bit against split_planes.split, with +-0 and round-to-even ties among the values and a sentinel guard behind each buffer.
  * Cache.  ops.split_weight keeps the planes on the packed tensor: after a re-pack into the same tensor, after a device-side
    re-pack followed by ops.invalidate_derived, and after a switch from 3 planes to 1, the forward equals bit for bit the
    forward on a freshly packed tensor.

Measured on one MI355X (worst ratio per class: replay | probe | native fp32 or bf16 class on tests/conv_edges.py; bound):

    3 planes forward / input gradient   2.7e-7 | 4.6e-7 | 3.3e-7   (2^-20 = 9.5e-7, the fp32 constant)
    3 planes weight gradient            2.9e-7 | 5.0e-7 | 3.7e-7   (8e-7, the fp32 constant)
    1 plane forward / input gradient    3.3e-8 | 0      | 1.1e-9   (7e-8)
    1 plane weight gradient             9.3e-8 | 0      | 1.2e-7   (1.9e-7)
    BatchNorm partial sums              8.6e-8                     (1.5e-7, GAMMA_STATS unchanged)
    fallback records (native kernels)   2.5e-7 forward, 3.5e-9 weight gradient, under the fp32 constants

Every class started at its native constant and none needed more; the one-plane constants were then set to about twice the
worst.  The three-plane classes stay at the fp32 constants (1.9x and 1.6x the probe's worst, whose coherent sums of positive
terms are harder on the fp32 accumulation than random operands): on random operands three planes are slightly more
accurate than the native instruction, as DESIGN.md section 9 says.  The two-plane probe launches, bounded by the three-plane
constants, measured at most 3.3e-7; the one-plane probe sums are powers of two times small integers and came out exact.
All 84 probe mutants were rejected (7 instantiations x (2 + 4 + 6)), the last-row mutant in all 24 replays with
statistics, the dropped short last K split in all 4 forward replays that have one; the spy saw the split entry points in all
54 eligible replays and all 21 probe launches.  No kernel and no dispatch was found wrong.  30 records, 88 tests, about 4 s.
"""
import contextlib
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
import split_planes as S  # noqa: E402
from launch_harness import P  # noqa: E402
from test_conv_edges_gpu import _edge_extra  # noqa: E402  (the last-row and short-last-split mutants)

pytestmark = pytest.mark.gpu

LEDGER = LH.Ledger()
SPLIT_LAUNCHES = {}

# the entry points the spy records (argument names in include/s2i_hip.h order, the stream left out)
ARGS = {
    "s2i_conv_forward_split": "d x cvec wsplit planes np kp bias cls_bias y part ws ws_bytes",
    "s2i_conv_forward_cls": "d x cvec w bias cls_bias y part ws ws_bytes",
    "s2i_conv_wgrad_split": "d planes a cvec g grad ws ws_bytes",
    "s2i_conv_wgrad": "d a cvec g grad ws ws_bytes",
}
SPLIT_ENTRY = {"conv": "s2i_conv_forward_split", "wgrad": "s2i_conv_wgrad_split"}
NATIVE_ENTRY = {"conv": "s2i_conv_forward_cls", "wgrad": "s2i_conv_wgrad"}


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("split-mode replay and plane probe")
    print("launches of the split entry points seen by the spy: %s" %
          ", ".join("%s %d" % kv for kv in sorted(SPLIT_LAUNCHES.items())))


@contextlib.contextmanager
def _mode(planes, tune=None):
    """ops.MATH_PLANES = planes for the body, with every call of the four entry points of ARGS recorded."""
    from speech_to_image_translation_without_text_amd import _lib, ops
    assert os.environ.get("S2I_TUNE", "") == "", "the replay runs the default planner"
    calls = []
    proxy = LH.LibRecorder(_lib.load(), calls, ARGS, lambda name: name not in ARGS, skip=("ws_bytes",))
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp, _lib.tuning(**(tune or {})):
        mp.setattr(ops, "MATH_PLANES", planes)
        mp.setattr(ops, "TILE_ROWS", 0)
        LH.install(mp, proxy)
        yield calls


def _assert_launched(what, calls, kind, split, planes):
    names = [c["fn"] for c in calls]
    want = SPLIT_ENTRY[kind] if split else NATIVE_ENTRY[kind]
    assert names == [want], "%s: expected one call of %s, the library saw %s" % (what, want, names)
    if split:
        assert calls[0]["planes"] == planes, (what, calls[0])
        SPLIT_LAUNCHES[want] = SPLIT_LAUNCHES.get(want, 0) + 1


def _on_grid(shape, gen, dev):
    return torch.randn(tuple(shape), generator=gen, device=dev).bfloat16().float()


# ---- replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,planes", S.cases(), ids=[S.case_id(i, p) for i, p in S.cases()])
def test_split_replay_matches_fp64(gpu, index, planes):
    rec = S.RECORDS[index]
    what = S.case_id(index, planes)
    gen = LH.gen_key(gpu, LH.canon(rec), planes)
    plan = S.split_plan(rec, planes)
    cls = S.class_of(rec, planes)
    B = (rec["x"] if "x" in rec else rec["a"])[0][0]
    given = {}
    if planes == 1:
        # one plane is bf16 operand rounding: with the operands on the bf16 grid (LH.dyadic weights are) every product is exact
        given = {k: _on_grid(rec[k][0], gen, gpu) for k in ("x", "a", "g") if k in rec}
        if rec["cvec"]:
            given["cvec"] = _on_grid((B, rec["cvec"]), gen, gpu)
    with _mode(planes, rec["tune"]) as calls:
        if S.is_conv(rec):
            C.replay_conv(rec, gen, gpu, what, LEDGER, extra=_edge_extra(LEDGER), weights="randn" if planes == 3 else "dyadic",
                          operands=given, cls=cls)
        else:
            C.replay_wgrad(rec, gen, gpu, what, LEDGER, operands=given, cls=cls)
    if S.is_conv(rec) or plan["split"]:
        _assert_launched(what, calls, "conv" if S.is_conv(rec) else "wgrad", plan["split"], planes)
    else:
        # ops.wgrad_raw hands every layer to s2i_conv_wgrad_split in a split mode; plan_wgrad keeps this one on the stream kernel
        assert [c["fn"] for c in calls] == ["s2i_conv_wgrad_split"] and plan["tile"].startswith("smalln-"), (what, calls, plan)
    torch.cuda.empty_cache()


# ---- plane probe -------------------------------------------------------------------------------------------------------
PROBES = [("fwd", "%dx%d" % t, p) for t in S.FWD_TILES for p in (1, 2, 3)] + \
         [("wgrad", t[len("split-"):], p) for t in S.WG_TILES for p in (1, 2, 3)]


@pytest.mark.parametrize("kind,tile,planes", PROBES, ids=["%s-%s-p%d" % c for c in PROBES])
def test_plane_probe(gpu, kind, tile, planes):
    from speech_to_image_translation_without_text_amd import ops
    what = "probe %s %s planes %d" % (kind, tile, planes)
    gen = LH.gen_key(gpu, "probe", kind, tile, planes)
    if kind == "fwd":
        s = S.probe_fwd(int(tile.split("x")[1]), planes)
        a = S.probe_operand((s["B"], s["H"], s["H"], s["Cx"]), gen, gpu)         # activations: split while they are staged
        b = S.probe_operand((s["N"], s["Cx"]), gen, gpu)                         # weights: split by s2i_split_packed_weight
        with _mode(planes) as calls:
            packed = ops.pack_weight(b, ops.PACK_PLAIN)
            y = ops.conv_raw(ops.CONV_K1, a, None, packed, s["N"], wR=packed.shape[1], ldw=packed.shape[2])[0]
        torch.cuda.synchronize()
        _assert_launched(what, calls, "conv", True, planes)
        out = y.view(-1, s["N"]).double()
        product = lambda ai, bj: ai.view(-1, s["Cx"]).double() @ bj.double().t()
        fam = S.probe_class(planes, "conv")
    else:
        s = S.probe_wgrad("split-" + tile, planes)
        a = S.probe_operand((s["B"], s["H"], s["H"], s["Ca"]), gen, gpu)         # the layer input
        b = S.probe_operand((s["B"], s["H"], s["H"], s["N"]), gen, gpu)          # the output gradient
        with _mode(planes) as calls:
            dw = ops.wgrad_raw(ops.CONV_K1, a, None, b, (s["N"], s["Ca"]))
        torch.cuda.synchronize()
        _assert_launched(what, calls, "wgrad", True, planes)
        assert (calls[0]["d"]["B"] * s["H"] * s["H"]) <= 80
        out = dw.double()
        product = lambda ai, bj: bj.view(-1, s["N"]).double().t() @ ai.view(-1, s["Ca"]).double()
        fam = S.probe_class(planes, "wgrad")
    (pa, ra), (pb, rb) = S.split(a, 3), S.split(b, 3)
    assert not ra.any() and not rb.any()
    prod = {(i, j): product(pa[i - 1], pb[j - 1]) for i in (1, 2, 3) for j in (1, 2, 3)}
    kept = S.kept(planes)
    ref = sum(prod[k] for k in kept)
    absref = sum(prod[k].abs() for k in kept)
    mutants = {"without a%d b%d" % k: ref - prod[k] for k in kept}
    if planes < 3:
        mutants["with the next order (%s)" % " + ".join("a%d b%d" % k for k in S.next_order(planes))] = \
            ref + sum(prod[k] for k in S.next_order(planes))
    chk = LH.Check(what, {fam + " probe": C.GAMMA[fam]}, LEDGER)
    chk.close(fam + " probe", "vs kept products", out, ref, absref, mutants=mutants)
    print("%s: %d mutants: %s" % (what, len(mutants), "all rejected" if not chk.bad else chk.bad))
    chk.done()


# ---- weight splitter ---------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 256, 0x5A5A


@pytest.mark.parametrize("planes", (1, 2, 3))
@pytest.mark.parametrize("T,R,Cw", [(9, 40, 136), (16, 4, 64), (1, 228, 2048)])
def test_weight_splitter_is_bit_exact(gpu, T, R, Cw, planes):
    gen = LH.gen_key(gpu, "splitter", T, R, Cw)
    v = torch.randn((T, R, Cw), generator=gen, device=gpu)
    special = torch.tensor([0.0, -0.0, 1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, (1 + 2.0 ** -8) * 2.0 ** -9,
                            1 + 2.0 ** -8 + 2.0 ** -16, 1 + 2.0 ** -8 + 2.0 ** -23, S.PROBE_C, -S.PROBE_C], device=gpu)
    v.view(-1)[:special.numel()] = special
    v[-1, -1, -special.numel():] = special
    ref, _ = S.split(v, planes)
    bits = lambda t: t.contiguous().bfloat16().view(torch.int16).view(-1)
    ref_rc = torch.cat([bits(p) for p in ref])                            # [plane][T][R][C]
    ref_cr = torch.cat([bits(p.transpose(1, 2)) for p in ref])            # [plane][T][C][R]
    n = planes * T * R * Cw
    chk = LH.Check("splitter %dx%dx%d planes %d" % (T, R, Cw, planes), {}, LEDGER)
    for use_rc, use_cr in ((True, True), (True, False), (False, True)):
        rc = torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device=gpu)
        cr = torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device=gpu)
        LH.call("s2i_split_packed_weight", P(v), T, R, Cw, planes, P(rc) if use_rc else None, P(cr) if use_cr else None)
        tag = "rc %d cr %d" % (use_rc, use_cr)
        chk.equal(tag + ": out_rc", rc[:n], ref_rc if use_rc else torch.full_like(ref_rc, SENTINEL))
        chk.equal(tag + ": out_cr", cr[:n], ref_cr if use_cr else torch.full_like(ref_cr, SENTINEL))
        chk.equal(tag + ": guards", torch.cat((rc[n:], cr[n:])), torch.full((2 * GUARD,), SENTINEL, dtype=torch.int16, device=gpu))
    chk.done()


# ---- the cache of ops.split_weight -------------------------------------------------------------------------------------
def test_split_weight_cache_follows_repacks(gpu):
    from speech_to_image_translation_without_text_amd import ops
    gen = LH.gen_key(gpu, "split cache")
    x = torch.randn((5, 8, 8, 64), generator=gen, device=gpu)
    w1, w2, w3 = (C.randn_weight((128, 64, 3, 3), gen, gpu) for _ in range(3))

    def run(packed, planes):
        with _mode(planes) as calls:
            y = ops.conv_raw(ops.CONV_K3S1, x, None, packed, 128, wR=packed.shape[1], ldw=packed.shape[2])[0]
        torch.cuda.synchronize()
        _assert_launched("cache", calls, "conv", True, planes)
        return y.clone()

    fresh = lambda w, planes: run(ops.pack_weight(w, ops.PACK_PLAIN), planes)
    chk = LH.Check("split cache", {}, LEDGER)
    packed = ops.pack_weight(w1, ops.PACK_PLAIN)
    y1 = run(packed, 3)
    chk.equal("first use", y1, fresh(w1, 3))
    chk.equal("second use (cached planes)", run(packed, 3), y1)
    # re-packed in place
    assert ops.pack_weight(w2, ops.PACK_PLAIN, out=packed) is packed
    y2 = run(packed, 3)
    assert not torch.equal(y2, y1)
    chk.equal("after pack_weight(out=packed)", y2, fresh(w2, 3))
    # a parameter's cached pack, re-packed on the device without the host bookkeeping (what a hipGraph replay does), then
    # ops.invalidate_derived
    p = torch.nn.Parameter(w1.clone())
    pk = ops.packed_weight(p)
    chk.equal("parameter pack", run(pk, 3), y1)
    LH.call("s2i_pack_conv_weight", P(w3), P(pk), 128, 64, 3, 3, pk.shape[1], ops.PACK_PLAIN)
    ops.invalidate_derived([p])
    y3 = run(pk, 3)
    assert not torch.equal(y3, y1)
    chk.equal("after invalidate_derived", y3, fresh(w3, 3))
    # 3 planes -> 1 on the same tensor
    y4 = run(pk, 1)
    assert not torch.equal(y4, y3)
    chk.equal("3 planes -> 1", y4, fresh(w3, 1))
    chk.equal("1 plane -> 3", run(pk, 3), y3)
    chk.done()
