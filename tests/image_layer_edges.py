"""Hand-written launches of the image-layer convolutions -- 3 (4) channels on one side -- on every branch of their dispatch.

GET_IMAGE_G's conv3x3 -> RGB, the first discriminator conv, the input gradients of both and the RGB conv's weight gradient
do not run on the matrix tiles that tests/conv_edges.py covers but on a family of hand-written kernels, which plan_fwd()
(csrc/s2i_conv_plan.hip) and plan_wgrad() (csrc/s2i_wgrad_plan.hip) choose between on shape and dtype alone.
Every production shape has maps of 64 x 64 and larger, where the tile kernels and the matrix tiles win, so the step, ragged
and eval censuses launch only part of the family, and all of it on square maps with whole blocks.  The records below use
the census schema (conv_replay.replay_conv / replay_wgrad run them unchanged) with the extra keys of tests/conv_edges.py:

  why        one line on what the shape is for
  reach      the dispatch branch (BRANCHES) and the edges (EDGES) the record claims; tests/test_image_layer_edges_cpu.py
             derives both from the library's plan queries (conv_plan / wgrad_plan below) and asserts them;
             tests/test_image_layer_edges_gpu.py replays the record in fp64
  ldy        (n3 records only) the row stride of the output, 4 floats for N = 3: ops.py always launches with ldy = N, so
             these records are launched through the C ABI by the GPU test

Constructors: fwd() is ops.ConvAct's forward (n_out = the 4-padded channel count, as model.py passes it), dgrad() is
ops._dgrad (wmode = 1; flip = 1 for the 3x3, the transposed kind for the stride-2 layer), wgrad() is conv_edges.wgrad.
H and W are separate, and so are the input and output dtype: bf16 in / fp32 out is the RGB conv and the first
discriminator conv's input gradient in bf16 activation mode, fp32 NHWC4 in / bf16 out the first discriminator conv and
GET_IMAGE_G's input gradient.

small_n_conv_kernel<4> and <8> (16 and 32 channels) have no record: thin_out_kernel takes every such launch at or above
the M >= 4096 gate both sit behind, whatever the dtypes, bias or map size, so no plan names them (they used to be what a C
caller got who passed no workspace; such a call is refused now).  The tags small-n-4 / small-n-8 are not claimed.  The tile kernels own whole 8 x 8 / 16 x 16 tiles and the
weight-gradient stream whole pixel groups (W >= 16), so neither has a pixel tail; their edge is the odd batch and the
odd last trip."""
import conv_edges as E
from speech_to_image_translation_without_text_amd import ops
from speech_to_image_translation_without_text_amd._lib import ACT_LRELU, ACT_NONE, ACT_TANH

KH = E.KH

BRANCHES = (
    "n4-igemm",           # N <= 4 on the 128 x 32 matrix tiles: M < 4096
    "thin-out",           # thin_out_kernel, 3x3
    "thin-out-4phase",    # thin_out_kernel, transposed conv: one grid plane per output phase
    "thin-in-16", "thin-in-32",          # thin_in_kernel<N>
    "tile-tconv64",       # tconv_n4_tile_kernel<64>
    "tile3-16", "tile3-32", "tile3-64",  # conv3_n4_tile_kernel<16>, <32>, <32> in two passes
    "small-n-16",         # small_n_conv_kernel<16>
    "rgb-out-k4", "rgb-out-k8", "rgb-out-k16", "rgb-out-k9", "rgb-out-k18", "rgb-out-k36",   # rgb_out_kernel<KSTEPS>
    "rgb-in-1x3", "rgb-in-2x3", "rgb-in-1x4", "rgb-in-2x4",                                  # rgb_in_kernel<MT, KH>
    "wg-small-n-4", "wg-small-n-8", "wg-small-n-16",    # small_n_wgrad_kernel<LPP>
    "wg-n4-igemm",        # the RGB conv's weight gradient on the matrix tiles: M < 32768
)
EDGES = (
    "pixtail",            # M is no multiple of the kernel's pixels per block
    "nonsquare",          # H != W
    "odd-trip",           # small_n_wgrad_kernel's single-group tail executes
    "grid-cap",           # the grid-stride loop runs more than once
    "bias",
    "n3",                 # N = 3 in rows of ldy = 4
    "threshold",          # M is the first value that selects the kernel
)
REACH = BRANCHES + EDGES

# pixels per block of the kernels with a pixel loop (a tail is possible); the tile kernels and the weight-gradient stream
# have none
PIXEL_LOOP = ("n4-igemm", "thin-out", "thin-out-4phase", "thin-in-16", "thin-in-32", "small-n-16", "rgb-out-k4", "rgb-out-k8",
              "rgb-out-k16", "rgb-out-k9", "rgb-out-k18", "rgb-out-k36", "rgb-in-1x3", "rgb-in-2x3", "rgb-in-1x4", "rgb-in-2x4")


def _dt(bf16):
    return "bf16" if bf16 else "f32"


def _extra(rec, why, reach):
    """reach = None: a launch of another test, described only to derive its branch (convact_launches)."""
    assert reach is None or (set(reach) <= set(REACH) and len([r for r in reach if r in BRANCHES]) == 1), reach
    rec.update(why=why, reach=sorted(reach or ()), tile_rows=0, tune={})
    return rec


def _conv(kind, wmode, flip, x, x16, packed, oihw, N, y16, act, bias, ldy, why, reach):
    raw = not (x16 or y16)
    rec = dict(fn="conv_raw" if raw else "conv_any", kind=kind, wmode=wmode, flip=flip, x=[x, _dt(x16)],
               w=dict(packed=packed, oihw=oihw, mode=ops.PACK_PLAIN), N=N, out_dtype=_dt(y16), stats=False, groups=1,
               w_offset=0, cvec=0, cls_bias=False, bias=N if bias else 0, act=act, fast=False)
    if raw:
        rec.update(wR=packed[1], ldw=packed[2])
    if ldy is not None:
        rec["ldy"] = ldy
    return _extra(rec, why, reach)


def fwd(layer, B, H, W, Cx, O, why, reach, *, x16=False, y16=False, act=ACT_NONE, bias=False, N=None, ldy=None):
    """Forward of ops.ConvAct: x [B, H, W, Cx padded to 4] -> O channels in rows of N = the 4-padded count (N = 3, ldy = 4: n3)."""
    k = KH[layer]
    return _conv(ops._KIND[layer], 0, 0, [B, H, W, E._r4(Cx)], x16, [k * k, E._r4(Cx), E._r4(O)], [O, Cx, k, k],
                 E._r4(O) if N is None else N, y16, act, bias, ldy, why, reach)


def dgrad(layer, B, Hd, Wd, Cin, O, why, reach, *, x16=False, y16=False, bias=False):
    """Input gradient of a layer Cin -> O channels (ops._dgrad) from dy [B, Hd, Wd, O padded to 4] -> 4-padded Cin channels."""
    k = KH[layer]
    kind, flip = ops._DGRAD[layer]
    return _conv(kind, 1, flip, [B, Hd, Wd, E._r4(O)], x16, [k * k, E._r4(Cin), E._r4(O)], [O, Cin, k, k], E._r4(Cin), y16,
                 ACT_NONE, bias, None, why, reach)


def wgrad(B, H, W, Ca, why, reach, *, a16=False):
    """Weight gradient of the RGB conv Ca -> 3 (ops._wgrad in fp32 mode).  With bf16 activations ops._wgrad pads the image
    gradient to 8 bf16 channels and takes the matrix cores, so a16 records describe a launch that only a direct caller of
    ops.wgrad_any / the C ABI makes."""
    rec = dict(fn="wgrad_any" if a16 else "wgrad_raw", kind=ops.CONV_K3S1, a=[[B, H, W, Ca], _dt(a16)], cvec=0,
               g=[[B, H, W, 4], "f32"], grad_shape=[3, Ca, 3, 3], swap=0, fold=0, out=False, accumulate=False, i_off=0, I_total=0)
    return _extra(rec, why, reach)


def _table():
    t = []
    T, L = ACT_TANH, ACT_LRELU
    # ---- the M = 4096 boundary ---------------------------------------------------------------------------------------
    t.append(fwd("k3s1", 63, 8, 8, 16, 3, "M = 4032: the last shape below the gate, on the matrix tiles", ["n4-igemm", "pixtail"],
                 act=T))
    t.append(fwd("k3s1", 64, 8, 8, 16, 3, "M = 4096: the first shape thin_out takes", ["thin-out", "threshold"], act=T))
    t.append(fwd("k3s1", 63, 8, 8, 64, 3, "M = 4032 from 64 channels: matrix tiles, K split", ["n4-igemm", "pixtail"], act=T))
    t.append(fwd("k3s1", 64, 8, 8, 64, 3, "M = 4096 from 64 channels: 8x8 maps hold no 16 x 16 tile", ["small-n-16", "threshold"],
                 act=T))
    # ---- thin_out_kernel, fp32 ---------------------------------------------------------------------------------------
    for Ca, act in ((8, T), (16, ACT_NONE), (24, T), (32, ACT_NONE)):
        t.append(fwd("k3s1", 65, 8, 8, Ca, 3, "M = 4160 = 16 x 256 + 64, %d channels" % Ca, ["thin-out", "pixtail"], act=act))
    t.append(fwd("k3s1", 65, 8, 8, 16, 3, "three channels in rows of four floats: the fourth stays untouched",
                 ["thin-out", "pixtail", "n3"], act=T, N=3, ldy=4))
    t.append(fwd("k3s1", 65, 8, 8, 32, 3, "with bias", ["thin-out", "pixtail", "bias"], act=T, bias=True))
    t.append(fwd("k3s1", 9, 8, 64, 16, 3, "8 x 64 maps", ["thin-out", "nonsquare"], act=T))
    t.append(fwd("k3s1", 9, 64, 8, 32, 3, "64 x 8 maps", ["thin-out", "nonsquare"]))
    t.append(fwd("k3s1", 17, 16, 16, 8, 3, "8 channels on 16 x 16 maps (no tile kernel for 8 channels)", ["thin-out"], act=T))
    t.append(fwd("k3s1", 5, 16, 64, 24, 3, "24 channels on 16 x 64 maps, M = 5120", ["thin-out", "nonsquare"], act=T))
    t.append(dgrad("k4s2", 65, 8, 8, 3, 16, "input gradient of a stride-2 conv 3 -> 16: M = 4160 per phase",
                   ["thin-out-4phase", "pixtail"]))
    t.append(dgrad("k4s2", 65, 8, 8, 3, 32, "the same from 32 channels", ["thin-out-4phase", "pixtail"]))
    t.append(dgrad("k4s2", 9, 16, 32, 3, 32, "from 32 channels on 16 x 32 gradients", ["thin-out-4phase", "nonsquare"]))
    t.append(dgrad("k4s2", 9, 32, 16, 3, 16, "from 16 channels on 32 x 16 gradients", ["thin-out-4phase", "nonsquare"]))
    t.append(dgrad("k4s2", 64, 8, 8, 3, 16, "M = 4096 per phase", ["thin-out-4phase", "threshold"]))
    # ---- small_n_conv_kernel<16>, fp32 -------------------------------------------------------------------------------
    t.append(fwd("k3s1", 65, 8, 8, 64, 3, "64 channels on 8x8 maps, M = 4160", ["small-n-16"], act=T))
    t.append(fwd("k3s1", 17, 16, 16, 64, 3, "64 channels on 16 x 16 maps, M = 4352: the plan splits K, which the tile kernel "
                 "refuses", ["small-n-16"], act=T))
    t.append(fwd("k3s1", 9, 8, 64, 64, 3, "8 x 64 maps, with bias", ["small-n-16", "nonsquare", "bias"], bias=True, act=T))
    t.append(dgrad("k4s2", 257, 4, 4, 3, 64, "transposed conv from 64 channels on 4x4 gradients (no 8 x 8 tile), M = 4112",
                   ["small-n-16"]))
    t.append(dgrad("k4s2", 1025, 2, 2, 3, 64, "2x2 gradients, M = 4100 = 256 x 16 + 4: a wave's last group holds one pixel",
                   ["small-n-16", "pixtail"]))
    t.append(dgrad("k4s2", 513, 4, 4, 3, 64, "M = 8208 > 512 blocks x 16 pixels: the blocks stride", ["small-n-16", "grid-cap"]))
    t.append(dgrad("k4s2", 129, 4, 8, 3, 64, "4 x 8 gradients, M = 4128", ["small-n-16", "nonsquare"]))
    # ---- the tile kernels, fp32 and bf16 input -----------------------------------------------------------------------
    t.append(fwd("k3s1", 16, 16, 16, 16, 3, "one 16 x 16 tile per image, M = 4096", ["tile3-16", "threshold"], act=T))
    t.append(fwd("k3s1", 17, 16, 16, 16, 3, "17 images, bf16 input", ["tile3-16"], act=T, x16=True))
    t.append(fwd("k3s1", 9, 16, 32, 16, 3, "16 x 32 maps: two tiles side by side", ["tile3-16", "nonsquare"], x16=True))
    t.append(fwd("k3s1", 17, 16, 16, 32, 3, "32 channels, 17 images", ["tile3-32"], act=T))
    t.append(fwd("k3s1", 9, 16, 32, 32, 3, "32 channels on 16 x 32 maps", ["tile3-32", "nonsquare"], act=T))
    t.append(fwd("k3s1", 9, 32, 16, 32, 3, "32 channels on 32 x 16 maps, bf16 input, bias", ["tile3-32", "nonsquare", "bias"],
                 act=T, x16=True, bias=True))
    t.append(fwd("k3s1", 256, 16, 16, 64, 3, "64 channels in two passes; M = 65536 is the smallest unsplit plan",
                 ["tile3-64"], act=T))
    t.append(fwd("k3s1", 128, 16, 32, 64, 3, "64 channels on 16 x 32 maps, bf16 input", ["tile3-64", "nonsquare"], act=T,
                 x16=True))
    t.append(dgrad("k4s2", 64, 8, 8, 3, 64, "one 8 x 8 tile per image, M = 4096", ["tile-tconv64", "threshold"]))
    t.append(dgrad("k4s2", 65, 8, 8, 3, 64, "65 images", ["tile-tconv64"]))
    t.append(dgrad("k4s2", 65, 8, 8, 3, 64, "65 images, bf16 gradient", ["tile-tconv64"], x16=True))
    t.append(dgrad("k4s2", 33, 8, 16, 3, 64, "8 x 16 gradients, bf16", ["tile-tconv64", "nonsquare"], x16=True))
    t.append(dgrad("k4s2", 33, 16, 8, 3, 64, "16 x 8 gradients", ["tile-tconv64", "nonsquare"]))
    # ---- rgb_out_kernel: bf16 in, fp32 out ---------------------------------------------------------------------------
    for Ca, act in ((16, T), (32, ACT_NONE), (64, T)):
        t.append(fwd("k3s1", 65, 8, 8, Ca, 3, "M = 4160 = 32 x 128 + 64 from %d bf16 channels" % Ca,
                     ["rgb-out-k%d" % (9 * Ca // 16), "pixtail"], act=act, x16=True))
    for O in (16, 32):
        t.append(dgrad("k4s2", 65, 8, 8, 3, O, "transposed conv from %d bf16 channels, M = 4160 per phase" % O,
                       ["rgb-out-k%d" % (O // 4), "pixtail"], x16=True))
    t.append(dgrad("k4s2", 257, 4, 4, 3, 64, "transposed conv from 64 bf16 channels on 4x4 gradients, M = 4112",
                   ["rgb-out-k16", "pixtail"], x16=True))
    t.append(fwd("k3s1", 9, 8, 64, 16, 3, "8 x 64 maps", ["rgb-out-k9", "nonsquare"], act=T, x16=True))
    t.append(fwd("k3s1", 9, 64, 8, 32, 3, "64 x 8 maps", ["rgb-out-k18", "nonsquare"], act=T, x16=True))
    t.append(fwd("k3s1", 9, 8, 64, 64, 3, "8 x 64 maps from 64 channels", ["rgb-out-k36", "nonsquare"], x16=True))
    t.append(dgrad("k4s2", 33, 8, 16, 3, 32, "transposed conv on 8 x 16 gradients", ["rgb-out-k8", "nonsquare"], x16=True))
    t.append(dgrad("k4s2", 33, 16, 8, 3, 16, "transposed conv on 16 x 8 gradients", ["rgb-out-k4", "nonsquare"], x16=True))
    t.append(dgrad("k4s2", 129, 4, 8, 3, 64, "transposed conv from 64 channels on 4 x 8 gradients", ["rgb-out-k16", "nonsquare",
                                                                                                   "pixtail"], x16=True))
    t.append(dgrad("k4s2", 65, 32, 32, 3, 16, "M = 66560 > 512 blocks x 128 pixels per phase: the blocks stride",
                   ["rgb-out-k4", "grid-cap"], x16=True))
    t.append(fwd("k3s1", 65, 8, 8, 16, 3, "three channels in rows of four floats", ["rgb-out-k9", "pixtail", "n3"], act=T,
                 x16=True, N=3, ldy=4))
    t.append(fwd("k3s1", 65, 8, 8, 32, 3, "with bias", ["rgb-out-k18", "pixtail", "bias"], act=T, x16=True, bias=True))
    t.append(fwd("k3s1", 64, 8, 8, 16, 3, "M = 4096", ["rgb-out-k9", "threshold"], act=T, x16=True))
    # ---- rgb_in_kernel: fp32 NHWC4 in, bf16 out ----------------------------------------------------------------------
    for O, br in ((16, "rgb-in-1x3"), (32, "rgb-in-1x3"), (64, "rgb-in-2x3")):
        t.append(dgrad("k3s1", 65, 8, 8, O, 3, "GET_IMAGE_G's input gradient to %d channels, M = 4160" % O, [br, "pixtail"],
                       y16=True))
        t.append(fwd("k3s1", 17, 16, 16, 3, O, "3x3 from the image to %d channels, LeakyReLU, 17 images" % O, [br], act=L,
                     y16=True))
    for O, br in ((16, "rgb-in-1x4"), (32, "rgb-in-1x4"), (64, "rgb-in-2x4")):
        t.append(fwd("k4s2", 65, 16, 16, 3, O, "first discriminator conv to %d channels, M = 4160" % O, [br, "pixtail"],
                     act=L if O != 32 else ACT_NONE, y16=True))
    t.append(dgrad("k3s1", 5, 16, 64, 16, 3, "16 x 64 maps", ["rgb-in-1x3", "nonsquare"], y16=True))
    t.append(fwd("k3s1", 5, 64, 16, 3, 64, "64 x 16 maps", ["rgb-in-2x3", "nonsquare"], act=L, y16=True))
    t.append(fwd("k4s2", 33, 16, 64, 3, 32, "16 x 64 images", ["rgb-in-1x4", "nonsquare"], act=L, y16=True))
    t.append(fwd("k4s2", 33, 64, 16, 3, 64, "64 x 16 images", ["rgb-in-2x4", "nonsquare"], act=L, y16=True))
    t.append(fwd("k4s2", 64, 16, 16, 3, 16, "M = 4096", ["rgb-in-1x4", "threshold"], act=L, y16=True))
    t.append(fwd("k3s1", 65, 8, 8, 3, 16, "with bias rgb_in declines: the launch falls through to thin_in with a bf16 output",
                 ["thin-in-16", "pixtail", "bias"], act=L, y16=True, bias=True))
    # ---- thin_in_kernel, fp32 ----------------------------------------------------------------------------------------
    for O in (16, 32):
        t.append(dgrad("k3s1", 65, 8, 8, O, 3, "GET_IMAGE_G's input gradient to %d channels, M = 4160" % O,
                       ["thin-in-%d" % O, "pixtail"]))
        t.append(dgrad("k3s1", 17, 16, 16, O, 3, "16 x 16 maps, 17 images", ["thin-in-%d" % O]))
    t.append(dgrad("k3s1", 9, 8, 64, 16, 3, "8 x 64 maps", ["thin-in-16", "nonsquare"]))
    t.append(dgrad("k3s1", 9, 64, 8, 32, 3, "64 x 8 maps", ["thin-in-32", "nonsquare"]))
    t.append(dgrad("k3s1", 64, 8, 8, 32, 3, "M = 4096", ["thin-in-32", "threshold"]))
    # ---- small_n_wgrad_kernel ----------------------------------------------------------------------------------------
    for Ca in (16, 32, 64):
        br = "wg-small-n-%d" % (Ca // 4)
        for a16 in (False, True):
            # with 2048 pixel groups per stride: Ca = 16 has 2048 groups at M = 32768 (one stride: every wave takes the
            # single-group tail), Ca = 32 / 64 have 2 / 4 strides (paired trips only)
            t.append(wgrad(8, 64, 64, Ca, "M = 32768, the first the stream takes", [br, "threshold"] + (["odd-trip"] if Ca == 16
                                                                                                        else []), a16=a16))
            t.append(wgrad(9, 64, 64, Ca, "M = 36864: %s strides of pixel groups" % {16: "1.125", 32: "2.25", 64: "4.5"}[Ca],
                           [br, "odd-trip"], a16=a16))
        t.append(wgrad(17, 32, 64, Ca, "32 x 64 maps, 17 images", [br, "nonsquare", "odd-trip"]))
        t.append(wgrad(16, 64, 32, Ca, "64 x 32 maps, M = 32768", [br, "nonsquare", "threshold"] + (["odd-trip"] if Ca == 16
                                                                                                   else []), a16=True))
    t.append(wgrad(32, 32, 32, 32, "32 x 32 maps, M = 32768", ["wg-small-n-8", "threshold"]))
    t.append(wgrad(7, 64, 64, 16, "M = 28672: below the gate, the matrix tiles with N = 4", ["wg-n4-igemm"]))
    t.append(wgrad(7, 64, 64, 64, "M = 28672 from 64 channels", ["wg-n4-igemm"], a16=True))
    return t


RECORDS = _table()


def convact_launches(kind, B, H, Cin, Cout, n_out, act, bias, bf16):
    """The family's launches of ops.ConvAct.apply(x, w, bias, kind, act, n_out) forward and backward on H x H maps, as
    records without claims: what test_kernels_gpu.CONVACT (fp32) and test_bf16_gpu.IMAGE_LAYERS (bf16 activation mode: feature
    maps of 8 and more channels are bf16, NHWC4 images fp32) launch.  The bf16 mode's weight gradients go to the matrix cores
    (ops._wgrad) and are not of the family."""
    x16, y16 = bf16 and Cin >= 8, bf16 and n_out >= 8
    Ho = H // 2 if kind == "k4s2" else H
    out = [fwd(kind, B, H, H, Cin, Cout, "forward", None, x16=x16, y16=y16, act=act, bias=bias),
           dgrad(kind, B, Ho, Ho, Cin, Cout, "input gradient", None, x16=y16, y16=x16)]
    if not bf16 and kind == "k3s1" and n_out == 4:
        out.append(wgrad(B, H, H, Cin, "weight gradient", None))
    return out


def record_id(i, rec):
    shape, dt = rec["x"] if "x" in rec else rec["a"]
    return "%s-W%d-%s%s" % (E.record_id(i, rec), shape[2], dt, "-" + "-".join(r for r in rec["reach"] if r in BRANCHES))


def in_family(rec):
    """A census record that belongs to the image-layer family: 4 or fewer channels on one side of a spatial convolution."""
    if rec["fn"].startswith("conv"):
        return rec["w"]["oihw"] is not None and not rec["cvec"] and (rec["N"] <= 4 or rec["x"][0][3] == 4) and \
            rec["kind"] != ops.CONV_K1
    return rec["kind"] != ops.CONV_K1 and rec["g"][0][3] == 4 and not rec["swap"]


# ---- what a record's plan reaches, from the planners' host queries -----------------------------------------------------
# s2i_conv_plan_query / s2i_wgrad_plan_query (_lib.conv_plan / wgrad_plan) name the kernel, its pixels per block and its grid;
# the library loads and plans without a device.  The tags below only rename the kernels and describe the input.
def _cdiv(a, b):
    return -(-a // b)


def _branch(kernel, N, Ca, nph):
    """The BRANCHES tag of a FWD_KERNELS name."""
    if kernel.startswith("f32-"):
        return "n4-igemm" if N <= 4 else "igemm"
    if kernel == "thin-out":
        return "thin-out-4phase" if nph == 4 else "thin-out"
    if kernel == "tconv-n4-64":
        return "tile-tconv64"
    if kernel.startswith("conv3-n4-"):
        return "tile3-%d" % Ca                           # conv3-n4-32 runs 64 channels in two chunks
    for prefix, tag in (("rgb-out-", "rgb-out-k"), ("smalln-", "small-n-")):
        if kernel.startswith(prefix):
            return tag + kernel[len(prefix):]
    return kernel                                        # rgb-in-MTxKH, thin-in-N


def conv_plan(rec):
    """dict(branch, reach, M, nphases, splitk, ppb, blocks, Ho, Wo) of a conv_raw / conv_any record."""
    from speech_to_image_translation_without_text_amd import _lib
    B, H, W, Ca = rec["x"][0]
    kind, N = rec["kind"], rec["N"]
    ldy = rec.get("ldy", N)
    nph = 4 if kind == ops.TCONV_K4S2 else 1
    Ho, Wo = E._geom(kind, H, W)
    assert not rec["fast"] and not rec["cvec"] and not rec["cls_bias"], rec
    told = _lib.conv_plan(E.conv_desc(rec, ldy=ldy), int(rec["x"][1] == "bf16"), int(rec["out_dtype"] == "bf16"), 0, rec["bias"])
    assert told is not None, (_lib.load().s2i_last_error(), rec)
    M = told["M"]
    assert M == B * Ho * Wo, told
    branch = _branch(told["kernel"], N, Ca, nph)
    # pixels per block of the kernels with a pixel loop; the grid-stride loop runs more than once where the grid is capped
    ppb = told["bm"] if branch in PIXEL_LOOP else None
    blocks = None if ppb is None else _cdiv(M, ppb)
    reach = {branch}
    if ppb is not None and M % ppb:
        reach.add("pixtail")
    if ppb is not None and told["gx"] < blocks:
        reach.add("grid-cap")
    if H != W:
        reach.add("nonsquare")
    if rec["bias"]:
        reach.add("bias")
    if N == 3 and ldy == 4:
        reach.add("n3")
    if M == 4096 and branch not in ("n4-igemm", "igemm"):
        reach.add("threshold")
    return dict(branch=branch, reach=reach, M=M, nphases=nph, splitk=told["splitk"], ppb=ppb, blocks=blocks, Ho=Ho, Wo=Wo)


def wgrad_plan(rec):
    from speech_to_image_translation_without_text_amd import _lib
    d = E.wgrad_desc(rec)
    a16, g16 = rec["a"][1] == "bf16", rec["g"][1] == "bf16"
    B, H, W, Ca = rec["a"][0]
    N = rec["g"][0][3]
    told = _lib.wgrad_plan(d, int(a16), int(g16))
    assert told is not None, (_lib.load().s2i_last_error(), rec)
    M, K = told["M"], told["K"]
    reach = set()
    if told["kernel"].startswith("smalln-"):
        assert not g16
        branch = "wg-small-n-%d" % (Ca // 4)
        ppw = 64 // (Ca // 4)
        ngroups, stride = M // ppw, told["gx"] * 4
        assert M % ppw == 0
        # a wave starts at group g0 < stride, takes pairs (g, g + stride) while g + stride < ngroups, then one more if g < ngroups
        for g0 in range(stride):
            g = g0
            while g + stride < ngroups:
                g += 2 * stride
            if g < ngroups:
                reach.add("odd-trip")
                break
        if M == 32768:
            reach.add("threshold")
    else:
        branch = "wg-n4-igemm" if N == 4 else "wg-igemm"
    reach.add(branch)
    if H != W:
        reach.add("nonsquare")
    return dict(branch=branch, reach=reach, M=M, K=K, N=N, splitk=told["ws_slabs"])


def plan(rec):
    return conv_plan(rec) if rec["fn"].startswith("conv") else wgrad_plan(rec)
