"""Plain references of the weight re-pack kernels and the tables of cases tests/test_weight_pack_cpu.py and
tests/test_weight_pack_gpu.py run.  Nothing here launches a kernel; the planner is asked through its host query.

  pack_ref        OIHW master -> P[T][Ip][Op] (csrc/s2i_pack.hip: pack_weight_kernel, pack_weight_batched_kernel)
  pack_bf16_ref   P -> bf16 stage layout Wb[phase][chunk][tap][Npad][CK] (csrc/s2i_bf16_pack.hip: pack_bf16_kernel,
                  pack_bf16_batched_kernel), with the wrong layouts the GPU module must tell from the right one
  CASES_F32, CASES_B16   the records; reach_f32 / reach_b16 derive from the shapes and the plan query which branch of the
                  kernels a record runs

Both operations are permutations with zero padding; UPFOLD adds up to four taps, the bf16 layout rounds once to nearest
even.  The references are therefore compared bit for bit."""
import collections

import torch

from speech_to_image_translation_without_text_amd import _lib
from speech_to_image_translation_without_text_amd._lib import (CONV_K3S1, CONV_K4S2, PACK_PLAIN, PACK_UPFOLD, TCONV_K4S2,
                                                               ConvDesc)

PACK16_KT = 4          # 32 x 32 tiles per strip of the batched bf16 re-pack (csrc/s2i_bf16_pack.hip)
SENTINEL_B16 = 0x5A5A  # prefill of a bf16 destination
SENTINEL_F32 = 0x7FC5A5A5   # prefill of an fp32 destination: a quiet NaN with a payload, compared as integers

# effective tap k4 of the nearest-x2 + 3x3 fold sums these parameter taps, along each axis
FOLD = {0: (2,), 1: (1, 2), 2: (0, 1), 3: (0,)}
# transposed form: tap (a, b) of output parity (py, px) reads folded tap PARITY_TAPS[py][a] * 4 + PARITY_TAPS[px][b]
PARITY_TAPS = {0: (1, 3), 1: (2, 0)}
# taps and phases of the stage layout, taps of the source P
TAPS = {CONV_K3S1: (9, 1, 9), CONV_K4S2: (16, 1, 16), TCONV_K4S2: (4, 4, 16)}
KIND_NAME = {CONV_K3S1: "k3s1", CONV_K4S2: "k4s2", TCONV_K4S2: "tconv"}


def roundup4(v):
    return (v + 3) & ~3


# ---- fp32: OIHW -> P[T][Ip][Op] --------------------------------------------------------------------------------------
def pack_ref(w, mode):
    """(P, mag): P[t][i][o] in fp64 with Ip = roundup4(I) rows and Op = roundup4(O) columns, padding zero, and the sum of
    the absolute values of the terms of each element."""
    w = w.detach()
    if w.dim() == 2:
        w = w[:, :, None, None]
    O, I, KH, KW = w.shape
    wd = w.double()
    if mode == PACK_PLAIN:
        terms = [[(ky, kx)] for ky in range(KH) for kx in range(KW)]
    else:
        assert mode == PACK_UPFOLD and (KH, KW) == (3, 3), (mode, KH, KW)
        terms = [[(ky, kx) for ky in FOLD[t >> 2] for kx in FOLD[t & 3]] for t in range(16)]
    val = torch.zeros((len(terms), roundup4(I), roundup4(O)), dtype=torch.float64, device=w.device)
    mag = torch.zeros_like(val)
    for t, taps in enumerate(terms):
        for ky, kx in taps:
            val[t, :I, :O] += wd[:, :, ky, kx].t()
            mag[t, :I, :O] += wd[:, :, ky, kx].t().abs()
    return val, mag


# ---- bf16: P -> Wb[phase][chunk][tap][Npad][CK] ----------------------------------------------------------------------
def src_tap(kind, flip, T, t, phase, swap_parity=False):
    if kind == TCONV_K4S2:
        py, px = phase >> 1, phase & 1
        if swap_parity:
            py, px = 1 - py, 1 - px
        return PARITY_TAPS[py][t >> 1] * 4 + PARITY_TAPS[px][t & 1]
    return T - 1 - t if flip else t


def pack_bf16_ref(P, kind, wmode, flip, Cx, N, Npad, CK, w_offset=0, mutate=None):
    """The stage layout as a flat bf16 tensor of nphases * T * Npad * Cx elements: element
    ((((phase * nchunk + cc) * T + t) * Npad + n) * CK + kc) = bf16_rne(M[ts][cc * CK + kc][n]), zero for N <= n < Npad, where
    M[ts] is the Cx x N matrix of source tap ts: rows of P[ts] (from flat offset w_offset on) when wmode == 0, columns
    otherwise.  P is an fp32 tensor [Tsrc][R][C].

    mutate names one wrong layout: 'flip ignored', 'wmode ignored' (N == Cx only), 'parities exchanged', 'chunk and tap
    exchanged', 'padding left at the sentinel'."""
    assert mutate in (None, "flip ignored", "wmode ignored", "parities exchanged", "chunk and tap exchanged",
                      "padding left at the sentinel"), mutate
    T, nphases, Tsrc = TAPS[kind]
    assert P.dim() == 3 and P.shape[0] == Tsrc and P.dtype == torch.float32, (P.shape, P.dtype)
    assert Cx % CK == 0 and Npad >= N
    R, C = P.shape[1], P.shape[2]
    nchunk = Cx // CK
    flat = P.contiguous().reshape(-1)
    if mutate == "flip ignored":
        flip = 0
    transposed = wmode != 0
    if mutate == "wmode ignored":
        assert N == Cx
        transposed = not transposed
    out = torch.zeros((nphases, nchunk, T, Npad, CK), dtype=torch.float32, device=P.device)
    for phase in range(nphases):
        for t in range(T):
            ts = src_tap(kind, flip, T, t, phase, swap_parity=mutate == "parities exchanged")
            base = w_offset + ts * R * C
            if transposed:
                M = flat[base:base + (N - 1) * C + Cx].as_strided((N, Cx), (C, 1)).t()      # [k][n] = P[ts][n][k]
            else:
                M = flat[base:base + (Cx - 1) * C + N].as_strided((Cx, N), (C, 1))          # [k][n] = P[ts][k][n]
            out[phase, :, t, :N, :] = M.reshape(nchunk, CK, N).permute(0, 2, 1)
    bits = out.to(torch.bfloat16).view(torch.int16)
    if mutate == "padding left at the sentinel":
        bits[:, :, :, N:, :] = SENTINEL_B16
    if mutate == "chunk and tap exchanged":
        bits = bits.permute(0, 2, 1, 3, 4)
    return bits.contiguous().view(torch.bfloat16).reshape(-1)


B16_MUTATIONS = ("flip ignored", "wmode ignored", "parities exchanged", "chunk and tap exchanged",
                 "padding left at the sentinel")


def b16_mutations(c, plan):
    """The wrong layouts of pack_bf16_ref that differ from the right one on record c."""
    out = []
    if c.kind != TCONV_K4S2 and c.flip:
        out.append("flip ignored")
    if c.N == c.Cx:
        out.append("wmode ignored")
    if c.kind == TCONV_K4S2:
        out.append("parities exchanged")
    if plan["nchunks"] > 1:
        out.append("chunk and tap exchanged")
    if plan["npad"] > c.N:
        out.append("padding left at the sentinel")
    return out


# ---- fp32 records ----------------------------------------------------------------------------------------------------
# O, I, KH, KW, mode, why; two_d: the master is a 2-D [O, I] matrix; misaligned: the master is a view one float into a
# larger buffer, so its address is a multiple of 4 bytes only
F32Case = collections.namedtuple("F32Case", "O I KH KW mode why two_d misaligned", defaults=(False, False))

CASES_F32 = [
    F32Case(64, 32, 4, 4, PACK_PLAIN, "4x4, whole tiles, 16-byte loads"),
    F32Case(64, 32, 3, 3, PACK_PLAIN, "3x3, whole tiles; float4 groups straddle two input channels"),
    F32Case(64, 32, 3, 3, PACK_UPFOLD, "3x3 folded to 16 taps, whole tiles"),
    F32Case(100, 40, 1, 1, PACK_PLAIN, "linear weight [O, I]: the any-tap-count instantiation, scalar accesses", True),
    F32Case(96, 24, 1, 1, PACK_PLAIN, "1x1 convolution weight, the same instantiation from a 4-D master"),
    F32Case(3, 64, 3, 3, PACK_PLAIN, "image layer: O = 3, Op = 4"),
    F32Case(3, 32, 3, 3, PACK_UPFOLD, "image layer behind an upsampling, O = 3"),
    F32Case(64, 3, 4, 4, PACK_PLAIN, "first discriminator conv: I = 3 forces scalar loads, Ip = 4"),
    F32Case(64, 12, 4, 4, PACK_PLAIN, "I = 12: the last input-channel tile is half empty under 16-byte loads"),
    F32Case(32, 20, 3, 3, PACK_UPFOLD, "I = 20 under 16-byte loads with 9 taps: the half empty tile ends inside a float4"),
    F32Case(70, 16, 3, 3, PACK_PLAIN, "O = 70: neither a multiple of 64 nor of 4, Op = 72"),
    F32Case(70, 16, 3, 3, PACK_UPFOLD, "O = 70 folded"),
    F32Case(10, 5, 3, 3, PACK_PLAIN, "one block: O < 64, I < 8, both padded (Op = 12, Ip = 8)"),
    F32Case(10, 4, 4, 4, PACK_PLAIN, "one block under 16-byte loads: O < 64, I = 4"),
    F32Case(65, 8, 4, 4, PACK_PLAIN, "O = 65: two tiles, one channel and three padding columns in the second"),
    F32Case(16, 7, 3, 3, PACK_UPFOLD, "I = 7: scalar loads with 9 taps, Ip = 8"),
    F32Case(64, 16, 4, 4, PACK_PLAIN, "master 4-byte aligned: the alignment test alone keeps it off 16-byte loads", False, True),
    F32Case(40, 8, 3, 3, PACK_UPFOLD, "master 4-byte aligned, 9 taps folded", False, True),
    F32Case(512, 128, 4, 4, PACK_PLAIN, "the largest weight, 1 M elements: 8 x 16 blocks"),
]


def f32_id(i):
    c = CASES_F32[i]
    return "%d-%dx%d%s-%s%s" % (i, c.O, c.I, "" if c.two_d else "x%dx%d" % (c.KH, c.KW),
                                "upfold" if c.mode == PACK_UPFOLD else "plain", "-misaligned" if c.misaligned else "")


def f32_shape(c):
    return (c.O, c.I) if c.two_d else (c.O, c.I, c.KH, c.KW)


def reach_f32(c):
    """The branches of pack_tile a record runs, from its shape."""
    Tp = c.KH * c.KW
    tags = {"taps-%d" % Tp if Tp in (16, 9) else "taps-any", "upfold" if c.mode == PACK_UPFOLD else "plain"}
    templated = Tp in (16, 9)
    if templated and c.I % 4 == 0 and not c.misaligned:
        tags.add("vector-load")
        if c.I % 8:
            tags.add("vector-load-half-empty-tile")
    elif templated and c.I % 4 == 0:
        tags.add("scalar-load-by-alignment")
    elif templated:
        tags.add("scalar-load-by-I")
    if c.two_d:
        tags.add("linear-2d")
    if c.O == 3:
        tags.add("O=3")
    if c.I == 3 and Tp == 16:
        tags.add("I=3-4x4")
    if c.O % 64 and c.O % 4:
        tags.add("O-ragged")
    if c.O < 64 and c.I < 8:
        tags.add("single-block")
    if c.O == 65:
        tags.add("O=65")
    if roundup4(c.O) > 64 or roundup4(c.I) > 8:
        tags.add("several-blocks")
    if roundup4(c.I) > c.I:
        tags.add("Ip>I")
    return tags


REQUIRED_F32 = ("taps-16", "taps-9", "taps-any", "plain", "upfold", "linear-2d", "O=3", "I=3-4x4", "vector-load",
                "vector-load-half-empty-tile", "scalar-load-by-I", "scalar-load-by-alignment", "O-ragged", "single-block",
                "O=65", "several-blocks", "Ip>I")


# ---- bf16 records ----------------------------------------------------------------------------------------------------
# kind, wmode, flip, Cx, N, H, why; B: batch of the descriptor (it steers the planner with H); Cc: rows of P in front of the
# matrix (the class-bias fold of conv_any: R = rows + Cc, w_offset = Cc * C); Cextra: columns of P behind the matrix;
# misaligned: P is a view one float into a larger buffer.  Records with Cextra or misaligned are run through the C entry
# points only: no packed parameter has that form.
B16Case = collections.namedtuple("B16Case", "kind wmode flip Cx N H why B Cc Cextra misaligned", defaults=(4, 0, 0, False))

CASES_B16 = [
    B16Case(CONV_K3S1, 0, 0, 64, 64, 16, "3x3 forward, CK = 32; Npad / 32 = 2: two empty tiles in the one strip along n"),
    B16Case(CONV_K3S1, 1, 1, 64, 64, 16, "3x3 input gradient: transposed and flipped, N == Cx"),
    B16Case(CONV_K3S1, 0, 0, 128, 32, 8, "3x3 forward under the 32 block: CK = 64, Npad / 32 = 1"),
    B16Case(CONV_K3S1, 0, 0, 32, 8, 8, "the smallest item: Cx = 32, Npad / 32 = 1, N = 8 in a padded block of 32"),
    B16Case(CONV_K3S1, 1, 1, 96, 24, 8, "transposed, Cx / 32 = 3: one empty tile along k; N = 24 in a block of 32"),
    B16Case(CONV_K3S1, 0, 0, 64, 192, 8, "N = 192 under the 128 block: Npad = 256; CK = 16 on a 3x3", 2),
    B16Case(CONV_K3S1, 1, 1, 64, 192, 8, "the same padded block, transposed and flipped", 2),
    B16Case(CONV_K3S1, 0, 1, 64, 40, 8, "flip without transposition; N = 40 in a block of 64"),
    B16Case(CONV_K4S2, 0, 0, 64, 128, 8, "stride 2 onto 4x4 maps under the 128 block: CK = 16", 8),
    B16Case(CONV_K4S2, 0, 0, 160, 64, 16, "stride 2 forward, 16 taps, five chunks of 32"),
    B16Case(CONV_K4S2, 1, 0, 160, 32, 16, "stride 2 as the input gradient of an upsampling block: transposed, Cx / 32 = 5"),
    B16Case(CONV_K4S2, 0, 1, 32, 32, 16, "stride 2, flipped"),
    B16Case(TCONV_K4S2, 0, 0, 64, 64, 8, "transposed form forward (upsampling block): 4 phases x 4 taps, CK = 64"),
    B16Case(TCONV_K4S2, 1, 0, 128, 64, 8, "transposed form as the input gradient of a stride-2 conv: a full strip along k"),
    B16Case(TCONV_K4S2, 0, 0, 96, 192, 8, "transposed form under the 128 block, CK = 32, Npad = 256", 2),
    B16Case(TCONV_K4S2, 1, 0, 32, 32, 8, "transposed form, the smallest transposed item"),
    B16Case(CONV_K3S1, 0, 0, 64, 64, 8, "class-bias fold: 20 rows of P in front, R = 84 > Cx, w_offset = 20 C", 4, 20),
    B16Case(CONV_K3S1, 1, 1, 64, 64, 8, "input gradient of the class-bias fold: 20 rows in front, R = 84 > N", 4, 20),
    B16Case(CONV_K3S1, 0, 0, 32, 24, 8, "C = 36 > N = 24 with 12 rows in front (C entry points only)", 4, 12, 12),
    B16Case(CONV_K3S1, 0, 0, 32, 40, 8, "P 4-byte aligned: scalar loads in the strip (C entry points only)", 4, 0, 0, True),
    B16Case(TCONV_K4S2, 1, 0, 96, 24, 8, "P 4-byte aligned, transposed form, transposed strip (C entry points only)", 4, 0, 0, True),
    B16Case(CONV_K3S1, 0, 0, 256, 256, 8, "the largest bf16 weight, 590 k elements: two strips along n, eight chunk rows"),
    B16Case(CONV_K3S1, 1, 1, 160, 64, 8, "transposed, Cx / 32 = 5: a full strip and one with three empty tiles"),
]


def b16_id(i):
    return "%d-%s" % (i, b16_name(CASES_B16[i]))


def b16_name(c):
    return "%s%s%s-%dto%d-h%d%s%s%s" % (KIND_NAME[c.kind], "-T" if c.wmode else "", "-flip" if c.flip else "", c.Cx, c.N, c.H,
                                        "-cc%d" % c.Cc if c.Cc else "", "-ce%d" % c.Cextra if c.Cextra else "",
                                        "-misaligned" if c.misaligned else "")


def b16_source_shape(c):
    """(Tsrc, R, C) of the packed fp32 source of a record."""
    rows, cols = (c.N, c.Cx) if c.wmode else (c.Cx, c.N)
    return TAPS[c.kind][2], rows + c.Cc, cols + c.Cextra


def b16_w_offset(c):
    return c.Cc * b16_source_shape(c)[2]


def b16_desc(c, B=None):
    """The descriptor of a record, as ops.conv_any builds it."""
    _, R, C = b16_source_shape(c)
    return ConvDesc(c.kind, c.B if B is None else B, c.H, c.H, c.Cx, 0, c.N, c.wmode, c.flip, R, C, _lib.ACT_NONE, 0, c.N, 1,
                    0, 0, 0, 0)


def b16_plan(c):
    plan = _lib.conv_bf16_plan(b16_desc(c))
    assert plan is not None and plan["kernel"] is not None, (c, plan)
    return plan


def b16_in_network(c):
    """Whether a packed parameter can be the source of this record (through ops.packed_weight / ops.bf16_weight)."""
    return not c.Cextra and not c.misaligned


def b16_master(c):
    """(shape, mode) of the OIHW master whose pack is the source of a record."""
    assert b16_in_network(c)
    Tsrc, R, C = b16_source_shape(c)
    if c.kind == CONV_K3S1:
        k, mode = 3, PACK_PLAIN
    elif (c.kind == CONV_K4S2) == (c.wmode == 0):
        k, mode = 4, PACK_PLAIN          # a stride-2 conv forward, or its input gradient in the transposed form
    else:
        k, mode = 3, PACK_UPFOLD         # an upsampling block forward (transposed form), or its input gradient
    return (C, R, k, k), mode


def b16_counterpart(c):
    """The record of the other direction on the same packed weight (forward <-> input gradient), or None where the bf16
    kernels do not take that layer."""
    if not b16_in_network(c) or c.Cc:
        return None
    other = {CONV_K3S1: CONV_K3S1, CONV_K4S2: TCONV_K4S2, TCONV_K4S2: CONV_K4S2}[c.kind]
    o = c._replace(kind=other, wmode=0 if c.wmode else 1, flip=(0 if c.wmode else 1) if other == CONV_K3S1 else 0,
                   Cx=c.N, N=c.Cx, why="the other direction of: " + c.why)
    if o.Cx % 32 or o.N % 8:
        return None
    plan = _lib.conv_bf16_plan(b16_desc(o))
    return o if plan is not None and plan["kernel"] is not None else None


def b16_strips(c, plan):
    """(gx, gy, tiles along n, tiles along k) of the batched kernel's strip grid."""
    tn, tk = plan["npad"] // 32, c.Cx // 32
    if c.wmode:
        return tn, -(-tk // PACK16_KT), tn, tk
    return -(-tn // PACK16_KT), tk, tn, tk


def reach_b16(c):
    """The branches of pack_bf16_block / pack_bf16_strip a record runs, from the plan query and its shapes."""
    plan = b16_plan(c)
    _, R, C = b16_source_shape(c)
    tags = {KIND_NAME[c.kind], "wmode!=0" if c.wmode else "wmode=0", "flip=%d" % c.flip, "ck-%d" % plan["ck"]}
    tn, tk = plan["npad"] // 32, c.Cx // 32
    if plan["npad"] > c.N:
        tags.add("npad>n-bn%d" % plan["bn"])
    if not c.wmode and tn % PACK16_KT:
        tags.add("empty-tiles-along-n")
    if c.wmode and tk % PACK16_KT:
        tags.add("empty-tiles-along-k-%d" % c.Cx)
    if tn == 1 and c.Cx == 32:
        tags.add("smallest-item")
    if c.Cc and (R > (c.N if c.wmode else c.Cx)):
        tags.add("w_offset-R>rows")
    if c.Cextra:
        tags.add("C>cols")
    if c.misaligned:
        tags.add("scalar-strip-T" if c.wmode else "scalar-strip")
    elif C % 4 == 0:
        tags.add("vector-strip")
    if plan["ck"] == 16 and c.kind == CONV_K4S2 and c.H == 8:
        tags.add("ck-16-on-4x4-maps")
    if c.N == c.Cx and not c.Cc:
        tags.add("square")
    if plan["nchunks"] > 1:
        tags.add("several-chunks")
    if (tn > PACK16_KT and not c.wmode) or (tk > PACK16_KT and c.wmode):
        tags.add("several-strips")
    return tags


REQUIRED_B16 = ("k3s1", "k4s2", "tconv", "wmode=0", "wmode!=0", "flip=0", "flip=1", "ck-16", "ck-32", "ck-64", "ck-16-on-4x4-maps",
                "npad>n-bn128", "npad>n-bn32", "empty-tiles-along-n", "empty-tiles-along-k-32", "empty-tiles-along-k-96",
                "empty-tiles-along-k-160", "smallest-item", "w_offset-R>rows", "C>cols", "scalar-strip", "scalar-strip-T",
                "vector-strip", "square", "several-chunks", "several-strips")
