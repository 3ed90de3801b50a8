"""What tests/test_weight_pack_gpu.py rests on, checked without a GPU: the plain references of tests/weight_pack_ref.py on
hand-written examples and against the element formula of the stage layout, the reach of the two case tables (derived from
the shapes and from s2i_conv_bf16_plan_query: a record that stops reaching its branch after a planner change fails here),
the strip geometry s2i_pack16_item_fill writes into a table item (host code), and the refusals of the pack entry points
that return before any launch."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import weight_pack_ref as W  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import (CONV_K3S1, CONV_K4S2, PACK_PLAIN, PACK_UPFOLD,  # noqa: E402
                                                               TCONV_K4S2)

F32_IDS = [W.f32_id(i) for i in range(len(W.CASES_F32))]
B16_IDS = [W.b16_id(i) for i in range(len(W.CASES_B16))]


def _last_error():
    msg = _lib.load().s2i_last_error()
    return msg.decode() if msg else ""


# ---- the references against themselves -------------------------------------------------------------------------------
def test_pack_ref_plain_on_a_hand_written_example():
    w = torch.arange(16, dtype=torch.float32).view(2, 2, 2, 2)          # w[o][i][ky][kx] = 8 o + 4 i + 2 ky + kx
    z = [0.0] * 4
    want = torch.tensor([[[0, 8, 0, 0], [4, 12, 0, 0], z, z],           # P[t][i][o], Ip = Op = 4
                         [[1, 9, 0, 0], [5, 13, 0, 0], z, z],
                         [[2, 10, 0, 0], [6, 14, 0, 0], z, z],
                         [[3, 11, 0, 0], [7, 15, 0, 0], z, z]], dtype=torch.float64)
    val, mag = W.pack_ref(w, PACK_PLAIN)
    assert val.dtype == torch.float64 and torch.equal(val, want) and torch.equal(mag, want)
    # a 2-D matrix is a 1x1 weight
    val2, _ = W.pack_ref(torch.tensor([[1.0, 2.0], [3.0, 4.0]]), PACK_PLAIN)
    assert torch.equal(val2, torch.tensor([[[1, 3, 0, 0], [2, 4, 0, 0], z, z]], dtype=torch.float64))


def test_pack_ref_upfold_on_a_hand_written_example():
    # w[o][i][ky][kx] = m(o, i) 2^(3 ky + kx), m = (-1)^o (1 + o + 2 i): an effective tap is m times the sum of the bits of
    # the parameter taps it folds.  By hand, with rows 0:{2} 1:{1,2} 2:{0,1} 3:{0} along each axis:
    S = [256, 384, 192, 64, 288, 432, 216, 72, 36, 54, 27, 9, 4, 6, 3, 1]
    w = torch.empty(2, 2, 3, 3)
    m = [[1.0, 3.0], [-2.0, -4.0]]
    for o in range(2):
        for i in range(2):
            for ky in range(3):
                for kx in range(3):
                    w[o, i, ky, kx] = m[o][i] * 2.0 ** (3 * ky + kx)
    val, mag = W.pack_ref(w, PACK_UPFOLD)
    assert val.shape == (16, 4, 4)
    for t in range(16):
        for i in range(4):
            for o in range(4):
                want = m[o][i] * S[t] if i < 2 and o < 2 else 0.0
                assert float(val[t, i, o]) == want and float(mag[t, i, o]) == abs(want), (t, i, o)


@pytest.mark.parametrize("index", range(len(W.CASES_B16)), ids=B16_IDS)
def test_pack_bf16_ref_has_the_planned_size_and_obeys_the_element_formula(index):
    c = W.CASES_B16[index]
    plan = W.b16_plan(c)
    Tsrc, R, C = W.b16_source_shape(c)
    P = torch.arange(Tsrc * R * C, dtype=torch.float32).view(Tsrc, R, C)         # index coded; bf16 rounding applies
    Npad, CK, off = plan["npad"], plan["ck"], W.b16_w_offset(c)
    out = W.pack_bf16_ref(P, c.kind, c.wmode, c.flip, c.Cx, c.N, Npad, CK, w_offset=off)
    assert out.dtype == torch.bfloat16 and out.numel() == plan["w_elems"], (out.numel(), plan)
    T, nphases, _ = W.TAPS[c.kind]
    nchunk = c.Cx // CK
    assert nchunk == plan["nchunks"]
    # the element formula, element by element on a sample (first, last and 200 drawn ones)
    gen = torch.Generator().manual_seed(index)
    picks = [0, out.numel() - 1] + torch.randint(0, out.numel(), (200,), generator=gen).tolist()
    flat = P.view(-1)
    for e in picks:
        kc, r = e % CK, e // CK
        n, r = r % Npad, r // Npad
        t, r = r % T, r // T
        cc, phase = r % nchunk, r // nchunk
        k = cc * CK + kc
        if c.kind == TCONV_K4S2:
            ts = W.PARITY_TAPS[phase >> 1][t >> 1] * 4 + W.PARITY_TAPS[phase & 1][t & 1]
        else:
            ts = T - 1 - t if c.flip else t
        if n >= c.N:
            want = torch.zeros((), dtype=torch.bfloat16)
        else:
            r_, c_ = (n, k) if c.wmode else (k, n)
            want = flat[off + ts * R * C + r_ * C + c_].to(torch.bfloat16)
        assert out[e].view(torch.int16) == want.view(torch.int16), (e, phase, cc, t, n, kc)


def test_mutated_bf16_references_differ_where_they_can():
    """Each wrong layout of pack_bf16_ref differs from the right one on every record where it can (the GPU module requires
    the kernels' output to differ from each)."""
    seen = {}
    for i, c in enumerate(W.CASES_B16):
        plan = W.b16_plan(c)
        Tsrc, R, C = W.b16_source_shape(c)
        P = torch.randn((Tsrc, R, C), generator=torch.Generator().manual_seed(i))
        args = (P, c.kind, c.wmode, c.flip, c.Cx, c.N, plan["npad"], plan["ck"])
        ref = W.pack_bf16_ref(*args, w_offset=W.b16_w_offset(c)).view(torch.int16)
        for m in W.b16_mutations(c, plan):
            bad = W.pack_bf16_ref(*args, w_offset=W.b16_w_offset(c), mutate=m).view(torch.int16)
            assert bad.shape == ref.shape and not torch.equal(bad, ref), (W.b16_id(i), m)
            seen[m] = seen.get(m, 0) + 1
    assert set(seen) == set(W.B16_MUTATIONS), seen


# ---- reach -----------------------------------------------------------------------------------------------------------
# which records reach a branch whose reach depends on the planner's answer (CK, the block width): stated, not derived
PLANNED_REACH = {
    "ck-16": [5, 6, 8, 21],
    "ck-16-on-4x4-maps": [8],
    "ck-32": [0, 1, 3, 4, 7, 9, 10, 11, 14, 15, 16, 17, 18, 19, 20, 22],
    "ck-64": [2, 12, 13],
    "npad>n-bn128": [5, 6, 14],
    "npad>n-bn32": [3, 4, 18, 20],
    "npad>n-bn64": [7, 19],
    "empty-tiles-along-n": [0, 2, 3, 7, 9, 11, 12, 16, 18, 19],
    "smallest-item": [3, 11, 15, 18],
}


def _reach_table(cases, reach):
    table = {}
    for i, c in enumerate(cases):
        for tag in reach(c):
            table.setdefault(tag, []).append(i)
    return table


def test_fp32_table_reaches_every_branch():
    table = _reach_table(W.CASES_F32, W.reach_f32)
    print("\nfp32 packer, branch: records")
    for tag in W.REQUIRED_F32:
        print("  %-30s %s" % (tag, ", ".join(F32_IDS[i] for i in table.get(tag, []))))
    missing = [t for t in W.REQUIRED_F32 if t not in table]
    assert not missing, "no record of CASES_F32 reaches: %s" % missing
    for c in W.CASES_F32:
        assert c.why and c.O * c.I * c.KH * c.KW <= 1 << 20, c
        assert not (c.two_d and (c.KH, c.KW) != (1, 1)), c
    shapes = [(W.f32_shape(c), c.misaligned) for c in W.CASES_F32]
    both = [s for s in set(shapes) if {c.mode for c in W.CASES_F32 if (W.f32_shape(c), c.misaligned) == s} ==
            {PACK_PLAIN, PACK_UPFOLD}]
    assert len(both) >= 2, "at least two masters are packed in both modes"
    # the half empty tile is met with 16 and with 9 taps, the alignment fallback with both
    for tag in ("vector-load-half-empty-tile", "scalar-load-by-alignment"):
        assert {W.CASES_F32[i].KH for i in table[tag]} == {3, 4}, tag


def test_bf16_table_reaches_every_branch():
    table = _reach_table(W.CASES_B16, W.reach_b16)
    print("\nbf16 packer, branch: records")
    for tag in sorted(set(W.REQUIRED_B16) | set(PLANNED_REACH)):
        print("  %-30s %s" % (tag, ", ".join(B16_IDS[i] for i in table.get(tag, []))))
    missing = [t for t in W.REQUIRED_B16 if t not in table]
    assert not missing, "no record of CASES_B16 reaches: %s" % missing
    for tag, want in PLANNED_REACH.items():
        assert table.get(tag, []) == want, "%s: reached by %s, stated %s" % (tag, table.get(tag, []), want)
    # the combinations the kernels treat differently
    assert {W.CASES_B16[i].N for i in table["npad>n-bn128"]} == {192}
    assert {W.CASES_B16[i].N for i in table["npad>n-bn32"]} >= {8, 24}
    for tag in ("npad>n-bn128", "several-chunks", "flip=1", "w_offset-R>rows"):
        assert {W.CASES_B16[i].wmode for i in table[tag]} == {0, 1}, tag
    for kind in ("k3s1", "k4s2", "tconv"):
        assert {W.CASES_B16[i].wmode for i in table[kind]} == {0, 1}, kind
    assert any(W.CASES_B16[i].wmode and W.CASES_B16[i].flip for i in table["square"]), "the record of the wmode mutant"
    for c in W.CASES_B16:
        assert c.why and W.b16_plan(c)["w_elems"] <= 1 << 20, c
        Tsrc, R, C = W.b16_source_shape(c)
        assert R % 4 == 0 and C % 4 == 0, "a packed source has rows and columns in multiples of 4"
    # both directions on one weight wherever the bf16 kernels take both
    pairs = [i for i, c in enumerate(W.CASES_B16) if W.b16_counterpart(c) is not None]
    print("  %-30s %s" % ("forward + input gradient", ", ".join(B16_IDS[i] for i in pairs)))
    assert len(pairs) >= 8 and {W.CASES_B16[i].kind for i in pairs} == {CONV_K3S1, CONV_K4S2, TCONV_K4S2}


@pytest.mark.parametrize("index", range(len(W.CASES_B16)), ids=B16_IDS)
def test_network_master_packs_to_the_source_of_its_record(index):
    c = W.CASES_B16[index]
    if not W.b16_in_network(c):
        assert c.Cextra or c.misaligned
        return
    (O, I, KH, KW), mode = W.b16_master(c)
    T = 16 if mode == PACK_UPFOLD else KH * KW
    assert (T, W.roundup4(I), W.roundup4(O)) == W.b16_source_shape(c)
    o = W.b16_counterpart(c)
    if o is not None:
        assert W.b16_master(o) == W.b16_master(c) and W.b16_source_shape(o)[1:] == W.b16_source_shape(c)[1:]


# ---- s2i_pack16_item_fill --------------------------------------------------------------------------------------------
def _fill(d, R, C, packed=0x10000, out=0x20000):
    item = _lib.Pack16Item()
    nb = _lib.load().s2i_pack16_item_fill(ctypes.byref(d), packed, R, C, out, ctypes.byref(item))
    return nb, item


def _all_b16():
    recs = list(W.CASES_B16)
    return recs + [o for o in map(W.b16_counterpart, W.CASES_B16) if o is not None]


def test_item_fill_geometry_agrees_with_the_plan():
    for c in _all_b16():
        plan = W.b16_plan(c)
        T, nphases, _ = W.TAPS[c.kind]
        _, R, C = W.b16_source_shape(c)
        nb, it = _fill(W.b16_desc(c), R, C)
        assert nb == it.gx * it.gy * nphases * T and nb > 0, (c, nb)
        assert (it.P, it.out, it.R, it.C, it.block0) == (0x10000, 0x20000, R, C, 0)
        assert (it.transpose, it.T, it.nphase, it.Nn, it.Npad, it.Kk, it.CK, it.flip) == \
            (int(c.wmode != 0), T, nphases, c.N, plan["npad"], c.Cx, plan["ck"], c.flip), c
        assert it.kind == {CONV_K3S1: 0, CONV_K4S2: 1, TCONV_K4S2: 2}[c.kind]
        assert (it.gx, it.gy) == W.b16_strips(c, plan)[:2], c
        # the strips cover the Npad / 32 x Cx / 32 tiles, with less than one strip of slack along the strip axis
        tn, tk = plan["npad"] // 32, c.Cx // 32
        if it.transpose:
            assert it.gx == tn and 0 <= it.gy * W.PACK16_KT - tk < W.PACK16_KT
        else:
            assert it.gy == tk and 0 <= it.gx * W.PACK16_KT - tn < W.PACK16_KT
        # every 16-byte segment the strips write lies inside the planned tensor
        assert nphases * T * plan["npad"] * c.Cx == plan["w_elems"]


def test_item_fill_refuses_a_small_source_a_null_pointer_and_an_unplanned_layer():
    c = W.CASES_B16[0]
    _, R, C = W.b16_source_shape(c)
    for cc in (c, W.CASES_B16[1]):
        rows, cols = (cc.N, cc.Cx) if cc.wmode else (cc.Cx, cc.N)
        for r, cl in ((rows - 1, cols), (rows, cols - 1)):
            nb, _ = _fill(W.b16_desc(cc), r, cl)
            assert nb == 1 and _last_error() == "pack(bf16): P is %d x %d, need rows >= %d cols >= %d" % (r, cl, rows, cols)
    for kw in (dict(packed=None), dict(out=None)):
        nb, _ = _fill(W.b16_desc(c), R, C, **kw)
        assert nb == 1 and _last_error() == "pack(bf16): null pointer"
    nb = _lib.load().s2i_pack16_item_fill(ctypes.byref(W.b16_desc(c)), 0x10000, R, C, 0x20000, None)
    assert nb == 1 and _last_error() == "pack(bf16): null pointer"
    # 48 input channels: the plan refuses, and says so
    d = W.b16_desc(c._replace(Cx=48))
    assert _lib.conv_bf16_plan(d) is None
    nb, _ = _fill(d, 64, 64)
    assert nb == -1 and "multiple of 32" in _last_error()


# ---- refusals before any launch --------------------------------------------------------------------------------------
def test_pack_entry_points_refuse_bad_arguments_before_launching():
    lib = _lib.load()
    w, p = 0x10000, 0x20000           # never dereferenced: every call returns from its argument checks
    for args, text in (((None, p, 8, 8, 3, 3, 8, PACK_PLAIN), "pack: null pointer"),
                       ((w, None, 8, 8, 3, 3, 8, PACK_PLAIN), "pack: null pointer"),
                       ((w, p, 8, 8, 3, 3, 4, PACK_PLAIN), "pack: bad shape"),               # Ip < I
                       ((w, p, 0, 8, 3, 3, 8, PACK_PLAIN), "pack: bad shape"),
                       ((w, p, 8, 8, 4, 4, 8, PACK_UPFOLD), "pack: UPFOLD needs a 3x3 parameter"),
                       ((w, p, 8, 8, 1, 1, 8, PACK_UPFOLD), "pack: UPFOLD needs a 3x3 parameter"),
                       ((w, p, 8, 8, 3, 3, 8, 7), "pack: unknown mode 7")):
        assert lib.s2i_pack_conv_weight(*args, None) != 0, args
        assert _last_error() == text, (args, _last_error())
    for args in ((None, 1, 1, 9), (w, 0, 1, 9), (w, 1, 0, 9), (w, 1, 1, 0), (w, 1, 1, 17)):
        assert lib.s2i_pack_conv_weights_batched(*args, None) != 0, args
        assert _last_error() == "pack(batched): bad args", (args, _last_error())
    for args in ((None, 1, 1), (w, 0, 1), (w, 1, 0)):
        assert lib.s2i_pack_conv_weights_bf16_batched(*args, None) != 0, args
        assert _last_error() == "pack(bf16, batched): empty table", (args, _last_error())
    # the single bf16 packer: the plan's refusal, a null pointer, a small source
    c = W.CASES_B16[0]
    _, R, C = W.b16_source_shape(c)
    assert lib.s2i_pack_conv_weight_bf16(ctypes.byref(W.b16_desc(c._replace(Cx=48))), w, 64, 64, p, None) != 0
    assert "multiple of 32" in _last_error()
    assert lib.s2i_pack_conv_weight_bf16(ctypes.byref(W.b16_desc(c)), None, R, C, p, None) != 0
    assert _last_error() == "pack(bf16): null pointer"
    assert lib.s2i_pack_conv_weight_bf16(ctypes.byref(W.b16_desc(c)), w, R - 1, C, p, None) != 0
    assert _last_error().startswith("pack(bf16): P is %d x %d" % (R - 1, C))
