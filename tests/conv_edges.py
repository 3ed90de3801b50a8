"""Hand-written convolution launches at the edges of the tile kernels: partly filled row tiles, column and K tails, short
last K splits, pixel-chunk tails of the weight gradients, ragged image tiles of the bf16 kernels, and every branch of the
bf16 planner (_bf16_branches) and of the weight-gradient planner and its finishing paths (_wgrad_branches) that no
production shape takes.

The train step's census (tests/step_launches.json) holds production shapes only: batches of 24 / 48 (72 / 144 stacked)
on power-of-two maps, where every GEMM is a whole number of row tiles and pixel chunks.  The records below use the
census schema, so conv_replay.replay_conv / replay_wgrad run them unchanged, and carry extra keys the replay ignores:

  why        one line on what the shape is for
  reach      the plan features the record claims (REACH below); tests/test_conv_edges_cpu.py derives them from the
             planners' host queries (conv_plan / wgrad_plan below) and asserts them, tests/test_conv_edges_gpu.py replays
             the record in fp64
  tile_rows  the value of ops.TILE_ROWS the replay runs under (0 = the planner's choice)
  tune       planner knobs (_lib.tuning) the replay runs under
  direct     (branch rows) the record is also launched through s2i_conv_forward_bf16 / s2i_conv_wgrad(_dt) itself, into
             guarded buffers

The constructors fill in the packed-weight shape, wR, ldw, w_offset and fast the way ops.ConvBnAct / ConvAct and
ops._dgrad / _wgrad launch the layer."""
from speech_to_image_translation_without_text_amd import ops

KH = {"k1": 1, "k3s1": 3, "k4s2": 4, "up": 3}

# the plan features a record may claim
REACH = (
    "rowtail-128",        # fp32 forward: 128 x 128 tiles, the last row tile partly filled
    "rowtail-96",         # 96 x 128 tiles, the last row tile partly filled
    "rowtail-128x64",     # 128 x 64 tiles (32 < N <= 64)
    "rowtail-128x32",     # 128 x 32 tiles (N <= 32)
    "single-partial-tile",  # one row tile per phase, partly filled
    "coltail",            # N is no multiple of the tile width
    "ktail",              # K = taps x channels is no multiple of the 32-deep chunk
    "short-last-split",   # split-K whose last split has fewer chunks than the others
    "rowtail-4phase",     # a partly filled row tile in each of the 4 phases of a transposed convolution
    "groups-96",          # grouped BatchNorm statistics on groups of whole 96-row (not 128-row) tiles
    "wg-pixtail-128x128", "wg-pixtail-128x64", "wg-pixtail-64x64", "wg-pixtail-96x64", "wg-pixtail-96x32", "wg-pixtail-256x128",
    "wg-pixtail-256x256",      # weight gradient: the pixel range ends on a short 32-pixel chunk, per tile shape of plan_wgrad
    "wg-rows3-odd-batch",  # the row-segment kernel (3x3, W >= 32) at its smallest map with a batch that is no power of two
    "b16-ragged-128",     # bf16 forward, 128-pixel kernel: the last tile holds fewer images than the others
    "b16-ragged-256",     # the same on the 256-pixel kernel
    "b16-persist-uneven",  # persistent 256-pixel kernel: the blocks walk different numbers of tiles
    "b16-wg-stagetail",   # bf16 weight gradient: the pixel range ends on a short 64-pixel stage
    "b16-coltail",        # bf16 convolution: N is no multiple of the kernel's column block (Npad > N)
    "b16-v2-split",       # 256-pixel kernel with a K split: raw slabs, then splitk_reduce_bf16_kernel
    "b16-short-last-split",  # bf16 K split whose last split has fewer channel chunks than the others
    "b16-tb>1",           # a pixel tile of more than one image
    "b16-cls-multi-image",   # class-bias table on a tile of more than one image
    "b16-groups-multi-image",  # grouped BatchNorm statistics on tiles of more than one image
    "b16-wg-split-overwrite",  # bf16 weight gradient: summed from more than one slab into a destination it overwrites
    "b16-wg-recut-fewer-slabs",  # bf16 weight gradient: the 64-pixel re-cut writes fewer slabs than the workspace was sized for
    "wg-pixtail-128x32",  # the pixel tail on the one fp32 tile the list above lacks
    "wg-rows3-coltail",   # row-segment kernel: N is no multiple of the column block (the gcolb == S2I_OOB loads)
    # fp32-MFMA and row-segment kernels: more than one slab and nchunks % cps != 0, the last pixel split is short
    "wg-short-last-split-128x128", "wg-short-last-split-128x64", "wg-short-last-split-128x32", "wg-short-last-split-64x64",
    "wg-short-last-split-96x64", "wg-short-last-split-96x32", "wg-short-last-split-256x128", "wg-short-last-split-256x256",
    "wg-short-last-split-rows3",
    # a bf16 operand read by a kernel named f32-* (bload4_any in igemm_wgrad_kernel): the GEMM's gathered operand a, its
    # plain operand g, or both (both bf16 but Cin % 8 or N % 8 keeps the layer off the bf16 cores)
    "wg-16-on-f32-a", "wg-16-on-f32-g", "wg-16-on-f32-ag",
) + tuple(
    # the finishing path of launch_wgrad (wgrad_finish below): rows per tile of the OIHW transpose, how the slabs were summed
    # before it, a partly filled last 32-column block, the swapped (and folded) form of the up block
    "wg-finish-rt%d-%s%s%s" % (rt, path, ctail, swap) for rt in (1, 2, 4, 8) for path in ("direct", "stream", "tree")
    for ctail in ("", "-ctail") for swap in ("", "-swap"))
FIN = "wg-finish-"


def _r4(v):
    return (v + 3) & ~3


def _packed(layer, O, I):
    return [16 if layer == "up" else KH[layer] ** 2, _r4(I), _r4(O)]


def _dt(bf16):
    return "bf16" if bf16 else "f32"


def _extra(rec, why, reach, tile_rows, tune):
    assert set(reach) <= set(REACH), reach
    rec.update(why=why, reach=sorted(reach), tile_rows=tile_rows, tune=dict(tune or {}))
    return rec


def fwd(layer, B, H, Cx, N, why, reach, *, Cc=0, cls=0, stats=True, groups=1, bf16=False, tile_rows=0, tune=None):
    """Forward of ops.ConvBnAct: x [B, H, H, Cx] (+ a broadcast vector of Cc channels, or cls leading weight rows folded
    into the class-bias table) -> N channels."""
    I = Cx + Cc + cls
    packed = _packed(layer, N, I)
    rec = dict(fn="conv_any" if bf16 else "conv_raw", kind=ops._KIND[layer], wmode=0, flip=0, x=[[B, H, H, Cx], _dt(bf16)],
               w=dict(packed=packed, oihw=[N, I, KH[layer], KH[layer]], mode=ops.PACK_UPFOLD if layer == "up" else
                      ops.PACK_PLAIN), N=N, out_dtype=_dt(bf16), stats=stats, groups=groups, w_offset=cls * packed[2],
               cvec=Cc, cls_bias=bool(cls), bias=0, act=0, fast=bf16)
    if not bf16:
        rec.update(wR=packed[1], ldw=packed[2])
    return _extra(rec, why, reach, tile_rows, tune)


def dgrad(layer, B, H, Cx, O, why, reach, *, bf16=False, fast=None, tile_rows=0, tune=None):
    """Input gradient of a layer Cx -> O channels on an H x H input (ops._dgrad): dy [B, Ho, Ho, Op] -> [B, H, H, Cx].
    fast=False with bf16: a layer the bf16 plan names no kernel for (NO_KERNEL below)."""
    kind, flip = ops._DGRAD[layer]
    packed = _packed(layer, O, Cx)
    Ho = {"k1": H, "k3s1": H, "k4s2": H // 2, "up": 2 * H}[layer]
    rec = dict(fn="conv_any" if bf16 else "conv_raw", kind=kind, wmode=1, flip=flip, x=[[B, Ho, Ho, packed[2]], _dt(bf16)],
               w=dict(packed=packed, oihw=[O, Cx, KH[layer], KH[layer]], mode=ops.PACK_UPFOLD if layer == "up" else
                      ops.PACK_PLAIN), N=Cx, out_dtype=_dt(bf16), stats=False, groups=1, w_offset=0, cvec=0, cls_bias=False,
               bias=0, act=0, fast=bf16 if fast is None else fast)
    if not bf16:
        rec.update(wR=packed[1], ldw=packed[2])
    return _extra(rec, why, reach, tile_rows, tune)


def wgrad(layer, B, H, Cin, N, why, reach, *, Cc=0, a16=False, g16=False, accumulate=False, out=False, i_off=0, tune=None,
          direct=False):
    """Weight gradient of a layer Cin (+ Cc broadcast) -> N channels on an H x H input (ops._wgrad); the up layer gathers dy
    by the k4s2 pattern against the layer input (swap, fold).  i_off > 0: the written slice of a wider tensor.  a16 / g16
    name the layer's input and its output gradient; under swap they are the GEMM's g and a (rec["g"], rec["a"])."""
    k = KH[layer]
    Ho = {"k1": H, "k3s1": H, "k4s2": H // 2, "up": 2 * H}[layer]
    fn = "wgrad_any" if (a16 or g16) else "wgrad_raw"
    if layer == "up":
        rec = dict(fn=fn, kind=ops.CONV_K4S2, a=[[B, Ho, Ho, N], _dt(g16)], cvec=0, g=[[B, H, H, Cin], _dt(a16)],
                   grad_shape=[N, Cin, 3, 3], swap=1, fold=1)
    else:
        rec = dict(fn=fn, kind=ops._KIND[layer], a=[[B, H, H, Cin], _dt(a16)], cvec=Cc, g=[[B, Ho, Ho, N], _dt(g16)],
                   grad_shape=[N, Cin + Cc, k, k] if k > 1 else [N, Cin + Cc], swap=0, fold=0)
    rec.update(out=bool(out or accumulate or i_off), accumulate=accumulate, i_off=i_off, I_total=i_off + Cin if i_off else 0)
    if direct:
        rec["direct"] = True
    return _extra(rec, why, reach, 0, tune)


def _tiles(make, heights):
    """One record per forced tile height (0 = the planner's choice)."""
    return [make(tr) for tr in heights]


def _table():
    t = []
    # ---- fp32 forward ------------------------------------------------------------------------------------------------
    t += _tiles(lambda tr: fwd("k3s1", 5, 8, 64, 128, "M = 320: 96-row tiles (the planner's choice) end on 32 rows, 128-row tiles on 64; "
                               "K split with a short last split", {0: ["rowtail-96", "short-last-split"], 96: ["rowtail-96", "short-last-split"],
                                                           128: ["rowtail-128", "short-last-split"]}[tr], tile_rows=tr),
                (0, 96, 128))
    t += _tiles(lambda tr: fwd("k3s1", 11, 8, 64, 256, "M = 704: row tail under both heights, two column tiles",
                               {0: ["rowtail-96", "short-last-split"], 96: ["rowtail-96", "short-last-split"],
                                128: ["rowtail-128", "short-last-split"]}[tr], tile_rows=tr), (0, 96, 128))
    t += _tiles(lambda tr: fwd("k3s1", 5, 8, 40, 136, "row tail, K = 360 (tail 8), N = 136 (tail 8); Cx % 32 != 0 takes the "
                               "general gather", {0: ["rowtail-96", "coltail", "ktail"], 96: ["rowtail-96", "coltail", "ktail"],
                                                  128: ["rowtail-128", "coltail", "ktail"]}[tr], tile_rows=tr), (0, 96, 128))
    t += _tiles(lambda tr: fwd("k4s2", 7, 16, 64, 128, "M = 448: five 96-row or four 128-row tiles, 64 rows in the last",
                               {0: ["rowtail-96"], 96: ["rowtail-96"], 128: ["rowtail-128"]}[tr], tile_rows=tr), (0, 96, 128))
    t.append(fwd("k4s2", 3, 16, 64, 64, "128 x 64 tile, M = 192: the second row tile half filled, K split", ["rowtail-128x64"]))
    t.append(fwd("k3s1", 5, 8, 32, 32, "128 x 32 tile, M = 320, unsplit: per-tile partial sums with a 64-row last tile",
                 ["rowtail-128x32"]))
    t.append(fwd("up", 5, 4, 64, 128, "transposed conv, M = 80: one partly filled tile in each of the 4 phases",
                 ["rowtail-4phase", "single-partial-tile"]))
    t.append(fwd("up", 3, 8, 64, 136, "transposed conv, M = 192, N = 136: column tail under phases", ["coltail"]))
    t.append(fwd("up", 5, 8, 64, 128, "transposed conv, M = 320, 128-row tiles: a 64-row last tile in each phase",
                 ["rowtail-4phase", "rowtail-128"], tile_rows=128))
    t.append(fwd("up", 5, 8, 64, 128, "transposed conv, M = 320, 96-row tiles: a 32-row last tile in each phase",
                 ["rowtail-4phase", "rowtail-96"], tile_rows=96))
    t.append(fwd("k3s1", 1, 4, 512, 128, "one image, M = 16, broadcast vector of 32 channels; deep K split with a short last "
                 "split", ["single-partial-tile", "short-last-split"], Cc=32))
    t.append(fwd("k3s1", 5, 4, 128, 64, "M = 80 on the 128 x 64 tile, broadcast vector, K split",
                 ["single-partial-tile", "rowtail-128x64"], Cc=32))
    t.append(fwd("k1", 5, 1, 100, 2048, "the generator's fc at batch 5: M = 5, K = 228 (tail 4), broadcast vector of 128",
                 ["single-partial-tile", "ktail"], Cc=128))
    t.append(fwd("k4s2", 9, 16, 64, 128, "three stacked BatchNorm batches of 3 images: groups of 192 rows = 2 x 96, no "
                 "multiple of 128", ["groups-96"], groups=3))
    t.append(fwd("k4s2", 9, 16, 16, 128, "the same groups with K = 256, unsplit: per-tile partial sums, two 96-row tiles per "
                 "group", ["groups-96"], groups=3))
    t.append(fwd("k3s1", 5, 16, 32, 64, "class-bias table (32 folded weight rows), unsplit as ops launches it, 5 images on "
                 "the 128 x 64 tile", [], cls=32))
    t.append(fwd("k3s1", 7, 16, 32, 128, "class-bias table, unsplit, M = 1792 = 18 x 96 + 64: the border classes of the tail "
                 "rows depend on their pixel position", ["rowtail-96"], cls=128, tile_rows=96))
    t.append(fwd("k3s1", 5, 16, 32, 128, "class-bias table, unsplit, M = 1280 = 13 x 96 + 32", ["rowtail-96"], cls=128,
                 tile_rows=96))
    # ---- fp32 input gradient -----------------------------------------------------------------------------------------
    t += _tiles(lambda tr: dgrad("k3s1", 5, 8, 128, 64, "flipped 3x3 input gradient, M = 320",
                                 {0: ["rowtail-96", "short-last-split"], 96: ["rowtail-96", "short-last-split"],
                                  128: ["rowtail-128", "short-last-split"]}[tr], tile_rows=tr), (0, 96, 128))
    t += _tiles(lambda tr: dgrad("k3s1", 11, 8, 136, 40, "flipped 3x3 input gradient, M = 704, N = 136 (column tail), K = "
                                 "360 (K tail)", {96: ["rowtail-96", "coltail", "ktail"],
                                                  128: ["rowtail-128", "coltail", "ktail"]}[tr], tile_rows=tr), (96, 128))
    t.append(dgrad("k4s2", 3, 16, 136, 64, "stride-2 input gradient = transposed conv on dy [3, 8, 8, 64]: M = 192 per "
                   "phase, N = 136", ["coltail"]))
    t.append(dgrad("k4s2", 5, 8, 128, 64, "stride-2 input gradient, M = 80 per phase", ["rowtail-4phase",
                                                                                        "single-partial-tile"]))
    t.append(dgrad("up", 5, 4, 64, 128, "up-block input gradient (stride-2 gather of dy on the folded weights), M = 80",
                   ["single-partial-tile", "rowtail-128x64"]))
    # ---- fp32 weight gradient ----------------------------------------------------------------------------------------
    t.append(wgrad("k3s1", 5, 4, 160, 64, "M = 80: chunks of 32 + 32 + 16 pixels; 128 x 64 tile; K = 1440 (tail 32)",
                   ["wg-pixtail-128x64", FIN + "rt2-direct"]))
    t.append(wgrad("k3s1", 3, 4, 40, 136, "M = 48, K = 360, N = 136: pixel, K and column tails together",
                   ["wg-pixtail-128x128", FIN + "rt1-direct-ctail"]))
    for bm, f in ((128, "wg-pixtail-128x128"), (256, "wg-pixtail-256x128")):
        t.append(wgrad("k4s2", 5, 8, 64, 128, "M = 80, K = 1024", [f, FIN + "rt2-direct"], tune=dict(wgrad_bm=bm)))
    for bm, f in ((128, "wg-pixtail-128x128"), (256, "wg-pixtail-256x128"), (512, "wg-pixtail-256x256")):
        t.append(wgrad("k3s1", 7, 4, 256, 512, "M = 112, K = 2304, N = 512", [f, FIN + "rt8-direct"], tune=dict(wgrad_bm=bm)))
    t.append(wgrad("k4s2", 1, 8, 4, 64, "the first discriminator conv's 64-row tile at one image, M = 16",
                   ["wg-pixtail-64x64", FIN + "rt1-direct"]))
    t.append(wgrad("k3s1", 5, 8, 32, 64, "K = 288 on 96 x 64 tiles, M = 320", [FIN + "rt1-direct"]))
    t.append(wgrad("k3s1", 5, 4, 32, 64, "K = 288 on 96 x 64 tiles, M = 80", ["wg-pixtail-96x64", FIN + "rt1-direct"]))
    t.append(wgrad("k3s1", 5, 8, 32, 32, "K = 288 on 96 x 32 tiles, M = 320", [FIN + "rt1-direct"]))
    t.append(wgrad("k3s1", 3, 4, 32, 32, "K = 288 on 96 x 32 tiles, M = 48", ["wg-pixtail-96x32", FIN + "rt1-direct"]))
    t.append(wgrad("k1", 5, 1, 100, 2048, "the fc's weight gradient at batch 5: one chunk of 5 pixels, broadcast vector",
                   ["wg-pixtail-128x128", FIN + "rt8-direct"], Cc=128))
    t.append(wgrad("k3s1", 3, 32, 32, 64, "row-segment kernel, W = 32, 3 images", ["wg-rows3-odd-batch", FIN + "rt1-stream"]))
    t.append(wgrad("k3s1", 3, 32, 64, 128, "row-segment kernel, 64 -> 128 channels, W = 32, 3 images",
                   ["wg-rows3-odd-batch", FIN + "rt2-stream"]))
    t.append(wgrad("up", 5, 4, 64, 128, "up-block weight gradient (swap, 4x4 taps folded to 3x3), M = 80, K = 2048",
                   ["wg-pixtail-128x64", FIN + "rt2-direct-swap"]))
    t.append(wgrad("k3s1", 5, 4, 160, 64, "M = 80, accumulated into a prefilled gradient", ["wg-pixtail-128x64", FIN + "rt2-direct"],
                   accumulate=True))
    t.append(wgrad("k3s1", 3, 4, 40, 136, "M = 48, written into input channels [32, 72) of a wider tensor",
                   ["wg-pixtail-128x128", FIN + "rt1-direct-ctail"], i_off=32))
    t.append(wgrad("k4s2", 5, 8, 64, 128, "M = 80, 256 x 128 tile, accumulated into a slice", ["wg-pixtail-256x128", FIN + "rt2-direct"],
                   accumulate=True, i_off=8, tune=dict(wgrad_bm=256)))
    # ---- bf16 --------------------------------------------------------------------------------------------------------
    t.append(fwd("k3s1", 5, 4, 256, 512, "4x4 maps: a 128-pixel tile spans 8 images, the batch has 5", ["b16-ragged-128", "b16-tb>1"],
                 bf16=True))
    t.append(fwd("k4s2", 9, 16, 64, 128, "8x8 outputs: 2 images per tile, 9 images", ["b16-ragged-128", "b16-tb>1"], bf16=True))
    t.append(fwd("up", 9, 4, 256, 256, "transposed conv on 4x4 maps: 8 images per tile, 9 images", ["b16-ragged-128", "b16-tb>1"],
                 bf16=True))
    t.append(dgrad("k3s1", 5, 4, 256, 512, "input gradient on 4x4 maps, 5 of 8 images", ["b16-ragged-128", "b16-tb>1"], bf16=True))
    t.append(dgrad("k4s2", 9, 8, 128, 64, "stride-2 input gradient (transposed conv of dy on 4x4 maps), 9 images",
                   ["b16-ragged-128", "b16-tb>1"], bf16=True))
    t.append(dgrad("up", 9, 4, 256, 256, "up-block input gradient: stride-2 gather of dy [9, 8, 8, 256]: 4x4 outputs, 8 images "
                   "per tile", ["b16-ragged-128", "b16-tb>1"], bf16=True))
    v2 = dict(b16_v2=2, b16_persist=4)
    t.append(fwd("k3s1", 5, 8, 96, 256, "256-pixel kernel on 8x8 maps: 4 images per tile, 5 images", ["b16-ragged-256", "b16-tb>1"],
                 bf16=True, tune=v2))
    t.append(fwd("k4s2", 5, 32, 96, 256, "persistent 256-pixel kernel: 5 one-image tiles over 2 block slots",
                 ["b16-persist-uneven"], bf16=True, tune=v2))
    t.append(fwd("up", 5, 8, 192, 256, "256-pixel transposed conv on 8x8 maps: 4 images per tile, 5 images",
                 ["b16-ragged-256", "b16-tb>1"], bf16=True, tune=v2))
    t.append(dgrad("k3s1", 5, 8, 256, 96, "256-pixel kernel, input gradient, 5 images on 8x8 maps", ["b16-ragged-256", "b16-tb>1"],
                   bf16=True, tune=v2))
    for bm in (128, 256, 512):
        t.append(wgrad("k3s1", 5, 4, 256, 256, "bf16 x bf16, M = 80: a 64-pixel stage and a 16-pixel one",
                       ["b16-wg-stagetail", FIN + "rt8-direct"], a16=True, g16=True, tune=dict(wgrad16_bm=bm)))
        t.append(wgrad("k3s1", 3, 4, 256, 256, "bf16 x bf16, M = 48: less than one stage", ["b16-wg-stagetail", FIN + "rt8-direct"],
                       a16=True, g16=True, tune=dict(wgrad16_bm=bm)))
    t.append(wgrad("k4s2", 5, 8, 64, 128, "bf16 x bf16 stride-2, M = 80, accumulated", ["b16-wg-stagetail", FIN + "rt2-direct"], a16=True,
                   g16=True, accumulate=True))
    t.append(wgrad("up", 5, 4, 64, 128, "bf16 x bf16 up-block (swap, fold), M = 80", ["b16-wg-stagetail", FIN + "rt2-direct-swap"],
                   a16=True, g16=True))
    t.append(wgrad("k4s2", 5, 8, 4, 64, "the first discriminator conv in bf16 mode: fp32 NHWC4 image x bf16 gradient, M = 80",
                   ["b16-wg-stagetail", FIN + "rt1-direct"], g16=True))
    t += _bf16_branches(v2)
    t += _wgrad_branches()
    return t


def _wgrad_branches():
    """The branches of plan_wgrad and the finishing paths of launch_wgrad that no production shape and no row above takes,
    each at the smallest shape that still takes it: the 128-thread row-segment kernel rows3-64x32 (never run before), the
    row-segment kernels off the census batches and with a column tail, the pixel tail of f32-128x32, a short last pixel
    split on the tiles that only ever ran whole ones, bf16 operands on the fp32-MFMA kernel, every (rows per tile, slab sum)
    pair of the OIHW finish that was missing.  direct=True: tests/test_conv_edges_gpu.py also calls s2i_conv_wgrad(_dt) itself
    with ldg = N + 8, the workspace of exactly s2i_wgrad_workspace_bytes(_dt) and the gradient each between sentinels."""
    t = []

    def w(*a, **k):
        t.append(wgrad(*a, **k))

    odd = "wg-rows3-odd-batch"
    # ---- row-segment kernels -------------------------------------------------------------------------------------------
    w("k3s1", 3, 32, 64, 32, "rows3-64x32 (never run): 128 threads, HPASS = 5, BPASS = 2; 24 slabs", [odd, FIN + "rt1-stream"], direct=True)
    w("k3s1", 3, 64, 64, 32, "rows3-64x32, W = 64: two chunks per image row, the left halo of the second is a real pixel; "
      "96 slabs, tree sum", [odd, FIN + "rt1-tree"])
    w("k3s1", 1, 32, 64, 32, "rows3-64x32, one image", [FIN + "rt1-stream"])
    w("k3s1", 9, 64, 64, 32, "rows3-64x32, 1152 chunks as 231 slabs of 5, the last of 2",
      [odd, "wg-short-last-split-rows3", FIN + "rt1-tree"], direct=True)
    w("k3s1", 3, 32, 32, 32, "rows3-32x32 off the census batches", [odd, FIN + "rt1-stream"])
    w("k3s1", 3, 32, 64, 64, "rows3-64x64 off the census batches", [odd, FIN + "rt1-stream"])
    w("k3s1", 3, 32, 32, 96, "rows3-32x64, gy = 2: the second column block half filled", [odd, "wg-rows3-coltail", FIN + "rt1-stream"])
    w("k3s1", 3, 32, 64, 96, "rows3-64x128 with 96 of 128 columns", [odd, "wg-rows3-coltail", FIN + "rt1-stream"])
    w("k3s1", 3, 32, 64, 32, "rows3-64x32 accumulated into input channels [8, 72) of a prefilled tensor", [odd, FIN + "rt1-stream"],
      accumulate=True, i_off=8, direct=True)
    # ---- f32-128x32 ----------------------------------------------------------------------------------------------------
    w("k3s1", 3, 4, 40, 32, "f32-128x32, M = 48: pixel tail (and K = 360: K tail)", ["wg-pixtail-128x32", FIN + "rt1-direct"])
    w("k3s1", 5, 4, 40, 24, "f32-128x32, M = 80, 24 of 32 columns", ["wg-pixtail-128x32", FIN + "rt1-direct-ctail"])
    w("k3s1", 11, 8, 40, 32, "f32-128x32, 22 chunks as 5 + 5 + 5 + 5 + 2", ["wg-short-last-split-128x32", FIN + "rt1-stream"], direct=True)
    # ---- a short last pixel split on the other tiles: 22 chunks in 5 slabs ------------------------------------------------
    w("k3s1", 11, 8, 32, 64, "f32-96x64, 22 chunks as 5 + 5 + 5 + 5 + 2", ["wg-short-last-split-96x64", FIN + "rt1-stream"])
    w("k3s1", 11, 8, 32, 32, "f32-96x32, 22 chunks as 5 + 5 + 5 + 5 + 2", ["wg-short-last-split-96x32", FIN + "rt1-stream"])
    w("k4s2", 11, 16, 64, 128, "f32-256x128, 22 chunks as 5 + 5 + 5 + 5 + 2", ["wg-short-last-split-256x128", FIN + "rt2-stream"],
      tune=dict(wgrad_bm=256))
    w("k3s1", 11, 8, 256, 256, "f32-256x256, 22 chunks as 5 + 5 + 5 + 5 + 2", ["wg-short-last-split-256x256", FIN + "rt8-stream"],
      tune=dict(wgrad_bm=512), direct=True)
    # ---- bf16 operands on the fp32-MFMA kernel ---------------------------------------------------------------------------
    A, G, AG = "wg-16-on-f32-a", "wg-16-on-f32-g", "wg-16-on-f32-ag"
    w("k3s1", 5, 4, 64, 128, "bf16 a x fp32 g on f32-128x128", [A, "wg-pixtail-128x128", FIN + "rt2-direct"], a16=True)
    w("k3s1", 5, 4, 64, 64, "fp32 a x bf16 g on f32-128x64", [G, "wg-pixtail-128x64", FIN + "rt1-direct"], g16=True)
    w("k3s1", 5, 4, 64, 36, "both bf16, N % 8 != 0 keeps them off the bf16 cores: f32-128x64 with 36 of 64 columns",
      [AG, "wg-pixtail-128x64", FIN + "rt1-direct-ctail"], a16=True, g16=True, direct=True)
    w("k3s1", 5, 4, 36, 128, "both bf16, Cin % 8 != 0: f32-128x128, K = 324 (K tail)", [AG, "wg-pixtail-128x128", FIN + "rt1-direct"],
      a16=True, g16=True)
    w("k4s2", 5, 8, 4, 72, "the first discriminator conv's shape with N = 72 > 64: not b16d1 but f32-128x128, fp32 image x bf16 "
      "gradient", [G, "wg-pixtail-128x128", FIN + "rt1-direct-ctail"], g16=True)
    w("k3s1", 3, 32, 32, 64, "a row-segment shape that a bf16 a keeps off that kernel: f32-128x64, 24 slabs", [A, FIN + "rt1-stream"],
      a16=True)
    w("up", 5, 4, 64, 128, "up block (swap, fold) with a bf16 layer input, which the swap makes the GEMM's g: f32-128x64",
      [G, "wg-pixtail-128x64", FIN + "rt2-direct-swap"], a16=True)
    w("k1", 3, 4, 64, 64, "bf16 a x fp32 g on f32-64x64", [A, "wg-pixtail-64x64", FIN + "rt1-direct"], a16=True)
    w("k1", 3, 4, 64, 36, "both bf16 on f32-64x64 with 36 of 64 columns", [AG, "wg-pixtail-64x64", FIN + "rt1-direct-ctail"], a16=True,
      g16=True)
    w("k3s1", 5, 4, 64, 20, "both bf16 on f32-128x32 with 20 of 32 columns", [AG, "wg-pixtail-128x32", FIN + "rt1-direct-ctail"], a16=True,
      g16=True)
    # ---- finishing paths of launch_wgrad -----------------------------------------------------------------------------------
    w("k1", 5, 4, 160, 128, "RT = 4 from one slab", ["wg-pixtail-128x128", FIN + "rt4-direct"])
    w("k1", 11, 8, 160, 128, "RT = 4 after slab_sum_kernel (5 slabs, the last of 2 chunks)",
      ["wg-short-last-split-128x128", FIN + "rt4-stream"], direct=True)
    w("k1", 11, 8, 640, 200, "RT = 8 with 8 of 32 columns in the last block, after slab_sum_kernel", ["wg-short-last-split-128x128",
                                                                                                      FIN + "rt8-stream-ctail"])
    w("up", 11, 8, 72, 136, "swap + fold with a column tail (72 input channels) after slab_sum_kernel", ["wg-short-last-split-128x128",
                                                                                                         FIN + "rt2-stream-ctail-swap"])
    w("k4s2", 8, 64, 4, 64, "64 slabs, tree sum, accumulated into a prefilled gradient", [FIN + "rt1-tree"], accumulate=True, direct=True)
    w("k1", 9, 32, 64, 36, "72 slabs, tree sum, into input channels [4, 68) of a wider tensor, 4 of 32 columns in the last block",
      [FIN + "rt1-tree-ctail"], i_off=4)
    w("k3s1", 5, 16, 40, 136, "10 slabs, stream sum, overwriting a prefilled tensor", [FIN + "rt1-stream-ctail"], out=True)
    # ---- bf16 cores: the 64-pixel re-cut of the 32-pixel split ------------------------------------------------------------
    w("k1", 9, 8, 32, 32, "b16-128x32, M = 576: the workspace holds 4 slabs (18 chunks of 32 pixels), the 9 stages of 64 fill 3",
      ["b16-wg-recut-fewer-slabs", "b16-wg-split-overwrite", FIN + "rt1-stream"], a16=True, g16=True, direct=True)
    return t


def _bf16_branches(v2):
    """The branches of plan_bf16 that no production shape takes, each at the smallest shape that still takes it: column
    blocks wider than N on every kernel, the 256-pixel kernels with a K split, the class-bias table and grouped statistics
    on tiles of several images, the kernels and directions no census record runs, the smallest weight-gradient tile.
    direct=True: tests/test_conv_edges_gpu.py also calls s2i_conv_forward_bf16 itself with ldy = N + 8 into guarded buffers."""
    t = []

    def f(*a, direct=False, **k):
        t.append(dict(fwd(*a, bf16=True, **k), direct=direct))

    def g(*a, direct=False, **k):
        t.append(dict(dgrad(*a, bf16=True, **k), direct=direct))

    def w(*a, **k):
        t.append(wgrad(*a, a16=True, g16=True, **k))

    tb, rag, ct = "b16-tb>1", "b16-ragged-128", "b16-coltail"
    # ---- kernels and directions the census never runs ----------------------------------------------------------------
    f("up", 2, 8, 64, 32, "tconv-32x64 (never run): 32 columns, 2 images in the one tile of each phase", [tb])
    f("up", 3, 16, 64, 32, "tconv-32x64: one image per tile, 6 tiles per phase", [])
    f("k3s1", 2, 16, 64, 32, "k3s1-32x64 forward (the census has its input gradient only)", [])
    f("k4s2", 3, 16, 32, 64, "k4s2-64x32 forward", [rag, tb])
    f("k4s2", 3, 16, 32, 32, "k4s2-32x32 forward", [rag, tb])
    g("k4s2", 3, 16, 32, 32, "tconv-32x32 as the stride-2 input gradient (the census has its forward only)", [rag, tb])
    g("k4s2", 3, 16, 32, 64, "tconv-32x64 as the stride-2 input gradient", [rag, tb])
    g("up", 3, 16, 128, 128, "256-pixel k4s2 as the up-block input gradient, K split in two", ["b16-v2-split"], tune=v2)
    g("up", 1, 32, 128, 32, "256-pixel k4s2 with the 66-pixel patch as the up-block input gradient: 32-column tiles of dy "
      "[1, 64, 64, 32]", [], tune=v2)
    g("up", 1, 32, 72, 32, "the same with 72 of 128 columns", [ct], tune=v2)
    # ---- column tail, 128-pixel kernels ------------------------------------------------------------------------------
    for N in (72, 136, 200):
        f("k3s1", 3, 8, 64, N, "k3s1-128x16 with N = %d: the last column block holds %d of 128" % (N, N % 128), [ct, rag, tb])
    f("k3s1", 3, 8, 64, 40, "k3s1-64x32 with 40 of 64 columns", [ct, rag, tb], direct=True)
    f("k3s1", 3, 8, 64, 24, "k3s1-32x64 with 24 of 32 columns", [ct, rag, tb])
    f("k3s1", 3, 4, 256, 72, "k3s1-128x16, 8 K splits, N = 72: the reduction with 18 column quads", [ct, rag, tb], direct=True)
    f("k4s2", 3, 16, 64, 72, "k4s2-128x32 with 72 of 128 columns", [ct, rag, tb], direct=True)
    f("k4s2", 3, 16, 64, 40, "k4s2-64x32 with 40 of 64 columns", [ct, rag, tb])
    f("up", 3, 8, 64, 72, "tconv-128x32 with 72 of 128 columns", [ct, rag, tb])
    f("up", 3, 8, 64, 40, "tconv-64x64 with 40 of 64 columns", [ct, rag, tb])
    f("up", 3, 8, 64, 24, "tconv-32x64 with 24 of 32 columns", [ct, rag, tb], direct=True)
    f("k3s1", 3, 8, 32, 24, "k3s1-32x32 (32 input channels) with 24 of 32 columns", [ct, rag, tb])
    f("k4s2", 3, 16, 32, 24, "k4s2-32x32 with 24 of 32 columns", [ct, rag, tb])
    f("up", 3, 8, 32, 24, "tconv-32x32 with 24 of 32 columns", [ct, rag, tb])
    f("k4s2", 9, 8, 64, 72, "k4s2-128x16 (8 maps of 4x4 outputs per tile) with 72 of 128 columns, 9 images", [ct, rag, tb])
    g("k3s1", 3, 8, 72, 64, "flipped 3x3 input gradient into 72 channels", [ct, rag, tb])
    g("k3s1", 3, 4, 72, 256, "flipped 3x3 input gradient into 72 channels, 8 K splits", [ct, rag, tb], direct=True)
    # ---- column tail, 256-pixel kernels ------------------------------------------------------------------------------
    f("k3s1", 5, 8, 96, 200, "v2-k3s1, 4 images per tile, 5 images, N = 200", [ct, "b16-ragged-256", tb], tune=v2, direct=True)
    f("k4s2", 3, 32, 64, 200, "v2-k4s2, persistent: 3 tiles over 2 block slots, N = 200", [ct, "b16-persist-uneven"], tune=v2)
    f("k4s2", 2, 64, 32, 136, "v2-k4s2-pw66, N = 136", [ct], tune=v2, direct=True)
    f("up", 3, 8, 64, 200, "v2-tconv, N = 200", [ct, "b16-ragged-256", tb], tune=v2, direct=True)
    # ---- 256-pixel kernels with a K split ----------------------------------------------------------------------------
    f("k3s1", 4, 8, 256, 128, "v2-k3s1, 4 K splits", ["b16-v2-split", tb], tune=v2)
    f("k3s1", 5, 8, 224, 128, "v2-k3s1, 7 chunks in splits of 3 + 3 + 1, 5 images on tiles of 4",
      ["b16-v2-split", "b16-short-last-split", "b16-ragged-256", tb], tune=v2)
    f("up", 4, 8, 256, 128, "v2-tconv, 2 K splits in each phase", ["b16-v2-split", tb], tune=v2)
    f("up", 5, 8, 320, 128, "v2-tconv, 5 chunks in splits of 3 + 2", ["b16-v2-split", "b16-short-last-split", "b16-ragged-256",
                                                                      tb], tune=v2)
    f("k4s2", 1, 32, 128, 128, "v2-k4s2, 2 K splits (split, so not persistent)", ["b16-v2-split"], tune=v2)
    f("k4s2", 3, 32, 160, 136, "v2-k4s2, 5 chunks in splits of 3 + 2, N = 136", ["b16-v2-split", "b16-short-last-split", ct],
      tune=v2, direct=True)
    f("k4s2", 1, 64, 160, 128, "v2-k4s2-pw66, 5 chunks in splits of 3 + 2", ["b16-v2-split", "b16-short-last-split"], tune=v2)
    # ---- class bias on tiles of several images (cls = 128 folded weight rows, as the census has them) -----------------
    cm = "b16-cls-multi-image"
    f("k3s1", 5, 4, 64, 64, "class bias, k3s1-64x32: 8 images per tile, 5 images", [cm, rag, tb], cls=128)
    f("k3s1", 5, 8, 64, 128, "class bias, k3s1-128x16: 2 images per tile, 5 images", [cm, rag, tb], cls=128)
    f("k3s1", 5, 4, 256, 128, "class bias, 16 chunks on one tile: unsplit only because the class bias forbids the split",
      [cm, rag, tb], cls=128)
    f("k3s1", 5, 8, 96, 256, "class bias, v2-k3s1: 4 images per tile, 5 images", [cm, "b16-ragged-256", tb], cls=128, tune=v2)
    # ---- grouped statistics on tiles of several images ---------------------------------------------------------------
    gm = "b16-groups-multi-image"
    f("k3s1", 8, 8, 128, 128, "2 groups of 4 images, 2 images per tile", [gm, tb], groups=2)
    f("k3s1", 6, 8, 128, 128, "3 groups of 2 images, 2 images per tile", [gm, tb], groups=3)
    f("k3s1", 8, 8, 96, 256, "v2-k3s1: 2 groups of 4 images, 4 images per tile", [gm, tb], groups=2, tune=v2)
    f("k4s2", 6, 32, 64, 128, "v2-k4s2, persistent: 6 one-image tiles of 3 groups over 4 block slots", ["b16-persist-uneven"],
      groups=3, tune=v2)
    f("k3s1", 6, 8, 256, 72, "3 groups of 2 images, 8 K splits, N = 72: the reduction's rows per group", [gm, tb, ct], groups=3, direct=True)
    f("k3s1", 8, 8, 256, 128, "v2-k3s1: 2 groups of 4 images, 4 K splits", [gm, tb, "b16-v2-split"], groups=2, tune=v2)
    # ---- bf16 weight gradient ----------------------------------------------------------------------------------------
    w("k1", 3, 4, 64, 64, "b16-64x64 (never run), M = 48: less than one stage", ["b16-wg-stagetail", FIN + "rt1-direct"])
    w("k1", 3, 8, 32, 40, "b16-64x64 with 40 of 64 columns", [FIN + "rt1-direct-ctail"])
    w("k1", 1, 16, 32, 40, "b16-64x64, 2 slabs summed into a prefilled gradient it overwrites",
      ["b16-wg-split-overwrite", FIN + "rt1-direct-ctail"], out=True)
    w("k3s1", 1, 16, 32, 32, "b16-128x32, 2 slabs summed into input channels [32, 64) of a wider tensor",
      ["b16-wg-split-overwrite", FIN + "rt1-direct"], i_off=32)
    return t


# planned by plan_bf16, which names no kernel for it (B16_NO_KERNEL): ops.conv_any takes the any-dtype fp32 kernel, bf16 in
# and out (fast=False), and the result holds the bound of the bf16 kernels
NO_KERNEL = [
    dgrad("k4s2", 3, 16, 64, 32, "transposed conv with BN 64 and 32-channel chunks", ["rowtail-128x64", "rowtail-4phase"],
          bf16=True, fast=False),
]

# refused by plan_bf16 before any launch: (record, text of the error)
REFUSED = [
    (fwd("k3s1", 8, 4, 128, 128, "2 groups of 4 images on 4x4 maps: the 128-pixel tile holds 8 images", [], groups=2, bf16=True),
     "a tile of 8 images straddles the 2 BatchNorm groups of batch 8"),
]


RECORDS = _table()


def record_id(i, rec):
    import launch_ref as R
    op, layer = R.layer_op(rec)
    shape = rec["x"][0] if "x" in rec else rec["a"][0]
    n = rec["N"] if "N" in rec else rec["g"][0][3]
    tag = "".join("-%s%d" % (k, v) for k, v in sorted(rec["tune"].items())) + ("-tr%d" % rec["tile_rows"] if rec["tile_rows"] else "")
    return "%03d-%s-%s-%s-B%dH%dC%dN%d%s" % (i, "b16" if "bf16" in (rec.get("out_dtype"), rec.get("a", [0, 0])[1],
                                                                     rec.get("g", [0, 0])[1]) else "f32", op, layer,
                                             shape[0], shape[1], shape[3], n, tag)


# ---- what a record's plan reaches, from the planners' host queries ---------------------------------------------------
# The library loads and plans without a device: s2i_conv_plan_query, s2i_conv_bf16_plan_query and s2i_wgrad_plan_query name
# the kernel, tile, grid and split of a launch, and nothing of the planners is restated here.
def _geom(kind, H, W):
    return ops._geom(kind, H, W) if kind != ops.TCONV_K4S2 else (H, W)     # the planners count rows per phase


def conv_desc(rec, **over):
    """The descriptor ops.conv_raw / conv_any builds for this record (tile_rows reaches conv_raw only)."""
    from speech_to_image_translation_without_text_amd import _lib
    B, H, W, Cx = rec["x"][0]
    raw = rec["fn"] == "conv_raw"
    wR, ldw = (rec["wR"], rec["ldw"]) if raw else rec["w"]["packed"][1:]
    f = dict(kind=rec["kind"], B=B, H=H, W=W, Cx=Cx, Cc=rec["cvec"], N=rec["N"], wmode=rec["wmode"], flip=rec["flip"], wR=wR,
             ldw=ldw, act=rec["act"], stats=int(rec["stats"]), ldy=rec["N"], groups=rec["groups"], nosplit=int(rec["cls_bias"]),
             kw=0, stride=0, pad=0, tile_rows=rec.get("tile_rows", 0) if raw else 0, in_act=0, in_groups=0)
    f.update(over)
    return _lib.ConvDesc(*[f[n] for n, _ in _lib.ConvDesc._fields_])


def wgrad_desc(rec):
    from speech_to_image_translation_without_text_amd import _lib
    B, H, W, Ca = rec["a"][0]
    N = rec["g"][0][3]
    gs = rec["grad_shape"]
    O, I, KH_, KW_ = gs if len(gs) == 4 else (gs[0], gs[1], 1, 1)
    return _lib.WgradDesc(rec["kind"], B, H, W, Ca, rec["cvec"], N, N, rec["swap"], rec["fold"], O, I, KH_, KW_,
                          int(rec["accumulate"]), rec["i_off"], rec["I_total"], 0, 0)


def conv_plan(rec):
    """dict(M, nphases, K, nchunks, splitk, cps, bm, BN, reach) of a conv_raw / conv_any record under its own tile_rows and
    knobs: the fp32 path's tile, K split and chunk counts are what s2i_conv_plan_query says."""
    import ctypes
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    B, H, W, Cx = rec["x"][0]
    kind, N = rec["kind"], rec["N"]
    nph = 4 if kind == ops.TCONV_K4S2 else 1
    Ho, Wo = _geom(kind, H, W)
    M = B * Ho * Wo
    K = ops._TAPS[kind] * (Cx + rec["cvec"])
    reach = set()
    with _lib.tuning(**rec.get("tune", {})):
        if rec["fast"]:
            return _bf16_plan(rec, M, nph)
        d = conv_desc(rec)
        told = _lib.conv_plan(d, int(rec["x"][1] == "bf16"), int(rec["out_dtype"] == "bf16"), 0, rec["bias"], rec["cls_bias"])
        assert told is not None, lib.s2i_last_error()
        assert told["kernel"].startswith("f32-") and (told["M"], told["K"]) == (M, K), told      # the matrix tiles at these sizes
        if rec["stats"]:
            assert lib.s2i_conv_stat_parts(ctypes.byref(d)) > 0, lib.s2i_last_error()
    bm, BN, sk, cps, nchunks = (told[f] for f in ("bm", "bn", "splitk", "cps", "nchunks"))
    one_tile = M < (96 if N > 64 else 128)
    tail = M % bm != 0 and not one_tile
    if tail:
        reach.add("rowtail-%d" % bm if N > 64 else "rowtail-128x%d" % BN)
    if one_tile:
        reach.add("single-partial-tile")
        if N <= 64:
            reach.add("rowtail-128x%d" % BN)
    if nph == 4 and (tail or one_tile):
        reach.add("rowtail-4phase")
    if N % BN:
        reach.add("coltail")
    if K % 32:
        reach.add("ktail")
    if sk > 1 and nchunks % cps:
        reach.add("short-last-split")
    if rec["stats"] and rec["groups"] > 1 and (M // rec["groups"]) % 128 != 0 and (M // rec["groups"]) % 96 == 0:
        reach.add("groups-96")
    return dict(M=M, nphases=nph, K=K, nchunks=nchunks, splitk=sk, cps=cps, bm=bm, BN=BN, reach=reach)


def _bf16_plan(rec, M, nph):
    """Pixels and images per tile, tiles, K splits and the grid are what s2i_conv_bf16_plan_query says."""
    from speech_to_image_translation_without_text_amd import _lib
    told = _lib.conv_bf16_plan(conv_desc(rec))
    assert told is not None and told["kernel"] is not None, (told, _lib.load().s2i_last_error())
    assert told["rows"] == M * nph, told
    B, bm, tb, gx, tiles = rec["x"][0][0], told["pixels"], told["tb"], told["gx"], told["tiles"]
    sk, cps, nchunks = told["splitk"], told["cps"], told["nchunks"]
    reach = set()
    if B % tb:
        reach.add("b16-ragged-%d" % bm)
    if gx < tiles and tiles % gx:         # persistent form: gx block slots walk the tiles, some one tile more than others
        reach.add("b16-persist-uneven")
    if rec["N"] % told["bn"]:
        assert told["npad"] > rec["N"], told
        reach.add("b16-coltail")
    if bm == 256 and sk > 1:
        reach.add("b16-v2-split")
    if sk > 1 and nchunks % cps:
        reach.add("b16-short-last-split")
    if tb > 1:
        reach.add("b16-tb>1")
        # declared on the record, checked against the plan's images per tile
        if rec["cls_bias"]:
            reach.add("b16-cls-multi-image")
        if rec["stats"] and rec["groups"] > 1:
            reach.add("b16-groups-multi-image")
    return dict(M=M, nphases=nph, splitk=sk, cps=cps, nchunks=nchunks, bm=bm, BN=told["bn"], CK=told["ck"], tb=tb, gridM=tiles,
                gx=gx, kernel=told["kernel"], npad=told["npad"], parts=told["parts"], ws_bytes=told["ws_bytes"], reach=reach)


def wgrad_plan(rec, table=True):
    """dict(M, K, N, tile, rows3, splitk, kernel, family, stage, nchunks, cps, slabs, ws_slabs, bn, threads, reach) from what
    s2i_wgrad_plan_query says: the tile is its (bm, bn), the row-segment and bf16 families are in the kernel's name, the pixel /
    stage tail is M % stage, a short last split nchunks % cps behind more than one slab; the finish tag is wgrad_finish's.
    table=False: a census record, which pins no tile."""
    import ctypes
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    d = wgrad_desc(rec)
    a16, g16 = rec["a"][1] == "bf16", rec["g"][1] == "bf16"
    B, H, W, Ca = rec["a"][0]
    Ho, Wo = ops._geom(rec["kind"], H, W)
    M, N = B * Ho * Wo, d.N
    K = ops._TAPS[rec["kind"]] * (Ca + rec["cvec"])
    tune = rec.get("tune", {})
    with _lib.tuning(**tune):
        ws = lib.s2i_wgrad_workspace_bytes_dt(ctypes.byref(d), int(a16), int(g16))
        if not (a16 or g16):
            assert ws == lib.s2i_wgrad_workspace_bytes(ctypes.byref(d))
        told = _lib.wgrad_plan(d, int(a16), int(g16))
    assert ws > 0 and ws == told["ws_slabs"] * K * N * 4 and (told["K"], told["M"]) == (K, M), (ws, told, lib.s2i_last_error())
    # the record itself: where the cost model may pick any of the 128- / 256-row fp32 tiles, the record pins one
    if table and told["kernel"] in ("f32-128x128", "f32-256x128", "f32-256x256") and K % 256 == 0:
        assert tune.get("wgrad_bm"), "a weight gradient that may take the 256-row tiles needs wgrad_bm set: %r" % (rec,)
    family = told["kernel"].split("-")[0]
    tile, rows3 = (told["bm"], told["bn"]), family == "rows3"
    # the pixel range in stages, and the stages per slab that cut it into told["slabs"] slabs (the query does not name cps:
    # every split the planner's search keeps satisfies cdiv(nchunks, cdiv(nchunks, split)) == split, the bf16 re-cut divides
    # by the workspace's slab count)
    nchunks = -(-M // told["stage"])
    cps = -(-nchunks // (told["ws_slabs"] if family in ("b16", "b16d1") else told["slabs"]))
    assert -(-nchunks // cps) == told["slabs"] == told["gz"] or family == "smalln", told
    reach = {wgrad_finish(d, told)}
    if family in ("b16", "b16d1"):
        if M % told["stage"]:
            reach.add("b16-wg-stagetail")
        if told["ws_slabs"] > 1 and not rec["accumulate"]:
            reach.add("b16-wg-split-overwrite")
        if told["slabs"] < told["ws_slabs"]:
            reach.add("b16-wg-recut-fewer-slabs")
    elif rows3:
        if B & (B - 1):
            reach.add("wg-rows3-odd-batch")
        if N % told["bn"]:
            reach.add("wg-rows3-coltail")
    elif M % told["stage"]:
        reach.add("wg-pixtail-%dx%d" % tile)
    if family in ("f32", "rows3") and told["slabs"] > 1 and nchunks % cps:
        reach.add("wg-short-last-split-" + ("rows3" if rows3 else "%dx%d" % tile))
    if family == "f32" and (a16 or g16):
        reach.add("wg-16-on-f32-" + "a" * a16 + "g" * g16)
    return dict(M=M, K=K, N=N, tile=tile, rows3=rows3, splitk=told["ws_slabs"], kernel=told["kernel"], reach=reach, family=family,
                stage=told["stage"], nchunks=nchunks, cps=cps, slabs=told["slabs"], ws_slabs=told["ws_slabs"], bn=told["bn"],
                threads=told["threads"])


def wgrad_finish(d, told):
    """The REACH tag of the finish launch_wgrad (csrc/s2i_wgrad.hip) runs behind the kernel of plan `told`.  The plan query
    does not export this rule, so it is restated here once, as the test side's oracle: the OIHW transpose takes the largest
    RT in 8, 4, 2, 1 rows per tile that leaves 128 blocks of 32 columns x RT rows (RT = 1 if none does); 32 or more slabs of
    fewer than 2^20 elements (and the stream kernels) are summed by slab_sum_tree_kernel first, else 3 or more by
    slab_sum_kernel, else the transpose sums them itself."""
    ncols, nrows = (d.I, d.O) if d.swap else (d.O, d.I)
    rt = 8
    while rt > 1 and -(-ncols // 32) * -(-nrows // rt) < 128:
        rt >>= 1
    S, kn = told["slabs"], told["K"] * d.N
    tree = told["kernel"].startswith("smalln") or (S >= 32 and kn % 4 == 0 and kn // 4 < (1 << 18))
    path = "tree" if tree else ("stream" if S > 2 and kn % 4 == 0 else "direct")
    return "%srt%d-%s%s%s" % (FIN, rt, path, "-ctail" if ncols % 32 else "", "-swap" if d.swap else "")


def wgrad_mutants(rec, plan, a, g, dw, true=None):
    """{name: gradient} of the wrong references the branches of `plan` (wgrad_plan) call for, each what a kernel that goes
    wrong on that branch would produce, accumulation order set aside.  a, g: the fp64 NCHW operands of rec["a"], rec["g"];
    dw(a=, g=) the fp64 gradient of the record with an operand replaced (conv_replay.wgrad_dw); true = dw().  Built from the
    reference alone, so tests/test_conv_edges_cpu.py can hold every one of them against the bound without a GPU."""
    import torch
    true = dw() if true is None else true
    reach, out = plan["reach"], {}
    B, _, Ho, Wo = g.shape                       # the GEMM's pixels are the rows of g, under swap too
    M, stage = plan["M"], plan["stage"]
    assert M == B * Ho * Wo, (plan, g.shape)

    def without(m0):
        return dw(g=g * (torch.arange(M, device=g.device) < m0).view(B, 1, Ho, Wo))

    def bf16(t):
        return t.float().bfloat16().double()

    if M % stage:
        out["pixel tail: the pixels of the last chunk dropped"] = without((plan["nchunks"] - 1) * stage)
    if plan["slabs"] > 1:
        out["slabs: the last pixel split not summed"] = without((plan["slabs"] - 1) * plan["cps"] * stage)
    finish = [f for f in reach if f.startswith(FIN)][0]
    if rec["g"][0][3] % plan["bn"] or "-ctail" in finish:
        m = true.clone()
        (m[:, -1] if rec["swap"] else m[-1]).zero_()
        out["column tail: the last valid column not written"] = m
    if plan["rows3"]:
        am = a.clone()
        am[:, :, 0] = 0
        out["row segment: input row 0 read as padding"] = dw(a=am)
        if a.shape[3] > 32:
            am = a.clone()
            am[:, :, :, 32] = 0
            out["row segment: the first pixel of the second chunk of a row read as padding"] = dw(a=am)
    if "wg-16-on-f32-a" in reach:
        out["bf16 a: the fp32 g rounded to bf16 too"] = dw(g=bf16(g))
    if "wg-16-on-f32-g" in reach:
        out["bf16 g: the fp32 a rounded to bf16 too"] = dw(a=bf16(a))
    if "-swap" in finish:
        out["swap + fold: ky and kx exchanged"] = true.transpose(2, 3)
    return out


def plan(rec):
    return conv_plan(rec) if rec["fn"].startswith("conv") else wgrad_plan(rec)
