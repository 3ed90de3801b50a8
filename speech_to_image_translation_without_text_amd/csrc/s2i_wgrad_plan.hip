// Host planner of the weight gradients (s2i_wgrad.hip launches what it decides): kernel, grid and pixel-range split per
// layer, and the entry points that only ask the plan a question.  No device code.
#include "s2i_igemm.h"

namespace {

// K rows x N columns of the result per block and the block size, indexed by WgKernel
const WgKernelInfo wg_kernels[WG_KERNEL_COUNT] = {
    {128, 128, 256}, {128, 64, 256}, {128, 32, 256}, {64, 64, 256}, {256, 128, 512}, {256, 256, 1024}, {96, 64, 192}, {96, 32, 192},
    {128, 128, 256},
    {128, 128, 256}, {128, 64, 256}, {128, 32, 256}, {64, 64, 256}, {256, 128, 512}, {256, 256, 1024},
    {64, 64, 256},
    {128, 128, 256}, {128, 64, 256}, {128, 32, 256}, {64, 64, 256},
    // row-segment 3x3: all 9 x 32 rows in one block, or 3 x 64 (one kernel row) per block
    {288, 64, 192}, {288, 32, 192}, {192, 128, 256}, {192, 64, 256}, {192, 32, 128},
    // <= 4 channel stream: every block covers the whole 9 Ca x 4 result
    {144, 4, 256}, {288, 4, 256}, {576, 4, 256},
};

// The pixel range is cut into `se` ranges of `cps` whole stages, each reduced by its own blocks into its own fp32 slab.
// Cost of one split in units of a stage round of the chip: tiles x splits fill rounds of the `slots` resident blocks, a block
// runs its stages plus a fixed prologue / epilogue share worth `fixed` stages, a stage of this tile takes `rel`, and every
// split writes a slab that the finish pass reads back (`slab` per split).
double split_cost(long long tiles, int slots, int cps, int se, double fixed, double rel, double slab) {
  return (double)((tiles * se + slots - 1) / slots) * (cps + fixed) * rel + slab * se;
}

// The cheapest split: every distinct effective split up to a quarter of the stages (256 at most), until the launch is past
// four rounds of blocks.  Ties go to the smaller split.
struct WgSplit { int split; double cost; };
WgSplit best_split(long long tiles, int slots, int nchunks, double fixed, double rel, double slab) {
  int smax = nchunks / 4;
  if (smax > 256) smax = 256;
  if (smax < 1) smax = 1;
  WgSplit best = {1, 1e300};
  for (int sc = 1; sc <= smax; ++sc) {
    const int cps = s2i_cdiv(nchunks, sc);
    if (s2i_cdiv(nchunks, cps) != sc) continue;   // same effective split as a smaller candidate
    const double cost = split_cost(tiles, slots, cps, sc, fixed, rel, slab);
    if (cost < best.cost) best = {sc, cost};
    if (tiles * sc > 4 * slots) break;
  }
  return best;
}

const WgSplit kNoSplit = {1, 1e300};   // a candidate the layer is not eligible for

// A tile candidate of the 256-row selections: resident block slots of the chip, fixed stages per block, time of a stage round
struct WgCand { WgKernel kernel; int slots; double fixed, rel; };
WgSplit price(const WgCand& c, int K, int N, int nchunks, double slab) {
  const WgKernelInfo& k = wg_kernels[c.kernel];
  return best_split((long long)s2i_cdiv(K, k.bm) * s2i_cdiv(N, k.bn), c.slots, nchunks, c.fixed, c.rel, slab);
}
// fp32, 32-pixel stages, in units of one stage round of the 128 x 128 tile (6.6 us).  Three resident 128 x 128 blocks per
// CU hide each other's load latency: 512 tiles x 1 = 0.67 of a round of the 768 slots ran at 108 TFLOP/s
// (profiles/r02_f32_per_launch_table.txt).
const WgCand kF32_128 = {WG_F32_128x128, 768, 3.0, 1.0};
// 256 x 128 tiles on 512-thread blocks (two per CU): half the `g` re-reads of the 128 x 128 form; a round of stages takes
// 1.26x as long for 1.33x the work (8.3 us against 6.6: tools/wgrad_bench.py, 103 -> 119 TFLOP/s on D_NET256's first
// stacked weight gradient)
const WgCand kF32_256x128 = {WG_F32_256x128, 512, 3.0, 1.26};
// 256 x 256 tiles on one 1024-thread block per CU where 256 divides N: a round of stages takes 1.22x the 128 x 128 round
// for 1.33x the work (D_NET256's three middle layers 0.650 -> 0.628 ms, profiles/r03_f32_wgrad_tile_heights.txt)
const WgCand kF32_256x256 = {WG_F32_256x256, 256, 3.0, 1.22};
// both operands bf16, 64-pixel stages, in us (measured on the config-4 layers, tools/wgrad16_bench.py): a round of stages
// takes ~2.5 us with 768 blocks of 128 x 128, ~2.7 us with 512 blocks of 256 x 128 and ~2.15 us with 256 blocks of
// 256 x 256; a block's prologue / epilogue is worth 3, 2 and 3 stages
const WgCand kB16_128 = {WG_B16_128x128, 768, 3.0, 2.5};
const WgCand kB16_256x128 = {WG_B16_256x128, 512, 2.0, 2.7};
const WgCand kB16_256x256 = {WG_B16_256x256, 256, 3.0, 2.15};

// Among the 128 x 128 plan `c128` and the two 256-row candidates: the knob's forced tile where the layer is eligible
// (128 never reaches here; 256; 512 = 256 x 256, else 256 x 128; 1 = the model without 256 x 256), else the cheapest.
// Returns the WgKernel offset from the family's 128 x 128 value.
int pick_256(int force, const WgSplit& c128, const WgSplit& c256, const WgSplit& c512, bool bf16) {
  const int k128 = 0, k256 = WG_F32_256x128 - WG_F32_128x128, k512 = WG_F32_256x256 - WG_F32_128x128;
  if (force == 512 && c512.cost < 1e300) return k512;
  if (force == 256 || force == 512) return k256;
  if (bf16) {
    // one model for the three: the cheaper 256-row candidate (256 x 128 on a tie) where it beats 128 x 128
    if (force != 0) return k128;
    const bool wide = c512.cost < c256.cost;
    return (wide ? c512.cost : c256.cost) < c128.cost ? (wide ? k512 : k256) : k128;
  }
  if (force == 0 && c512.cost < c256.cost && c512.cost < c128.cost) return k512;
  return c256.cost < c128.cost ? k256 : k128;
}

// apply-on-load: the generic 128 x 128 fp32 kernel only (the discriminator towers' layers); pl: the layer's fp32 plan
bool wgrad_in_ok(const s2i_wgrad_desc* d, const WgPlan& pl) {
  const int g = d->a_groups < 1 ? 1 : d->a_groups;
  return d->a_act == S2I_ACT_LRELU && d->Cc == 0 && !d->swap && pl.kernel == WG_F32_128x128 && g <= 3 && (d->B % g) == 0;
}

void set_kernel(WgPlan* pl, int kernel, int N) {
  const WgKernelInfo& k = wg_kernels[kernel];
  pl->kernel = (WgKernel)kernel;
  pl->threads = k.threads;
  pl->gx = s2i_cdiv(pl->K, k.bm);
  pl->gy = s2i_cdiv(N, k.bn);
}

// The 32-pixel plan: tile (named as the fp32 kernel of that shape, or the row-segment / stream kernel), grid and the
// split of the pixel range that sizes the workspace.  `mode` matters as "fp32 operands", "both bf16" or neither.
int plan_tiles(const s2i_wgrad_desc* d, WgMode mode, WgPlan* pl) {
  S2I_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->N > 0, "wgrad: non-positive extent");
  S2I_REQUIRE((d->Ca % 4) == 0 && (d->Cc % 4) == 0 && (d->N % 4) == 0 && d->Ca + d->Cc > 0,
              "wgrad: channel counts must be multiples of 4 (Ca=%d Cc=%d N=%d)", d->Ca, d->Cc, d->N);
  S2I_REQUIRE(s2i_is_pow2(d->H) && s2i_is_pow2(d->W), "wgrad: spatial extents must be powers of two");
  pl->Cin = d->Ca + d->Cc;
  switch (d->kind) {
    case S2I_CONV_K1: pl->T = 1; pl->Ho = d->H; pl->Wo = d->W; break;
    case S2I_CONV_K3S1: pl->T = 9; pl->Ho = d->H; pl->Wo = d->W; break;
    case S2I_CONV_K4S2: pl->T = 16; pl->Ho = d->H / 2; pl->Wo = d->W / 2; break;
    default: S2I_FAIL("wgrad: unsupported gather kind %d", d->kind);
  }
  const long long M = (long long)d->B * pl->Ho * pl->Wo;
  S2I_REQUIRE(M < (1ll << 30), "wgrad: too many rows");
  pl->M = (int)M;
  pl->K = pl->T * pl->Cin;
  S2I_REQUIRE(d->ldg >= d->N, "wgrad: ldg < N");
  // consistency of the OIHW target with the GEMM result
  const int taps_param = d->KH * d->KW;
  if (d->fold) S2I_REQUIRE(d->KH == 3 && d->KW == 3 && pl->T == 16, "wgrad: fold needs 3x3 param / 4x4 taps");
  else S2I_REQUIRE(taps_param == pl->T, "wgrad: taps mismatch (%d vs %d)", taps_param, pl->T);
  if (d->swap) S2I_REQUIRE(pl->Cin >= d->O && d->N == d->I, "wgrad(swap): shape mismatch");
  else S2I_REQUIRE(pl->Cin >= d->I && d->N >= d->O, "wgrad: shape mismatch");
  const bool f32 = mode == WG_MODE_F32 || mode == WG_MODE_F32_IN;
  const int K = pl->K, N = d->N;
  pl->planes = 0;
  pl->stage = 32;
  pl->nchunks = s2i_cdiv(M, 32);
  pl->gz = 1;

  int kernel = N > 64 ? WG_F32_128x128 : (N > 32 ? WG_F32_128x64 : WG_F32_128x32);
  if (K <= 64 && N > 32 && N <= 64) kernel = WG_F32_64x64;  // first discriminator conv: 16 taps x (3+1) channels
  // K = 288 (3x3 taps x 32 channels, the generator's last stage) wastes a quarter of three 128-row tiles: 96-row tiles
  // (they stage fp32 rows: fp32 operands only)
  if (f32 && K % 96 == 0 && N <= 64 && s2i_cdiv(K, 128) * 128 * 5 > K * 6) kernel = N > 32 ? WG_F32_96x64 : WG_F32_96x32;
  // slab write + read of the finish pass at ~4 TB/s, per split, in the units of each model
  const double slab32 = 3.0e-7 * (double)K * N, slab64 = 2.0e-6 * (double)K * N;
  WgCand base = kF32_128;
  base.kernel = (WgKernel)kernel;
  const WgSplit c0 = price(base, K, N, pl->nchunks, slab32);
  int splitk = c0.split;
  if (f32 && kernel == WG_F32_128x128 && (K % 256) == 0 && !d->a_act && s2i_tune(S2I_TUNE_WGRAD_BM, 0) != 128) {
    const WgSplit c8 = price(kF32_256x128, K, N, pl->nchunks, slab32);
    const WgSplit c9 = (N % 256) == 0 ? price(kF32_256x256, K, N, pl->nchunks, slab32) : kNoSplit;
    kernel += pick_256(s2i_tune(S2I_TUNE_WGRAD_BM, 0), c0, c8, c9, false);
    splitk = kernel == WG_F32_256x256 ? c9.split : (kernel == WG_F32_256x128 ? c8.split : splitk);
  }
  if (mode == WG_MODE_B16 && kernel == WG_F32_128x128 && (K % 256) == 0 && (pl->Cin % 8) == 0 && d->Cc == 0 && (N % 8) == 0 &&
      (d->ldg % 8) == 0 && s2i_tune(S2I_TUNE_WGRAD16_BM, 0) != 128) {
    // priced in the 64-pixel stages the bf16 kernels run; the 128 x 128 plan keeps the split found above
    const int nch64 = s2i_cdiv(M, 64);
    const int cps128 = s2i_cdiv(nch64, splitk), s128 = s2i_cdiv(nch64, cps128);
    const WgSplit c128 = {s128, split_cost((long long)s2i_cdiv(K, 128) * s2i_cdiv(N, 128), kB16_128.slots, cps128, s128,
                                           kB16_128.fixed, kB16_128.rel, slab64)};
    const WgSplit c6 = price(kB16_256x128, K, N, nch64, slab64);
    const WgSplit c7 = (N % 256) == 0 ? price(kB16_256x256, K, N, nch64, slab64) : kNoSplit;
    kernel += pick_256(s2i_tune(S2I_TUNE_WGRAD16_BM, 0), c128, c6, c7, true);
    splitk = kernel == WG_F32_256x256 ? c7.split : (kernel == WG_F32_256x128 ? c6.split : splitk);
  }
  set_kernel(pl, kernel, N);
  // thin 3x3 layers over wide maps: one kernel row per block, taps read from a staged row segment
  if (f32 && d->kind == S2I_CONV_K3S1 && d->Cc == 0 && (d->Ca == 32 || d->Ca == 64) && d->W >= 32 && (N % 32) == 0 && N <= 128) {
    if (d->Ca == 32) set_kernel(pl, N > 32 ? WG_ROWS3_32x64 : WG_ROWS3_32x32, N);
    else set_kernel(pl, N > 64 ? WG_ROWS3_64x128 : (N > 32 ? WG_ROWS3_64x64 : WG_ROWS3_64x32), N);
    // measured (24x128x128, 32->64): 512 / 768 / 1024 / 1536 blocks = 211 / 202 / 183 / 234 us; four 192-thread blocks or
    // three 256-thread blocks fill a CU, more only adds slab traffic
    splitk = (d->Ca == 32 ? 1024 : 768) / (pl->gx * pl->gy);
    if (splitk > pl->nchunks / 4) splitk = pl->nchunks / 4;
    if (splitk > 2048) splitk = 2048;
    if (splitk < 1) splitk = 1;
  }
  pl->cps = s2i_cdiv(pl->nchunks, splitk);
  pl->gz = pl->slabs = pl->ws_slabs = s2i_cdiv(pl->nchunks, pl->cps);
  // <= 4 output channels of a 3x3 conv: streamed on the vector units, one slab per block
  if (d->kind == S2I_CONV_K3S1 && d->Cc == 0 && N == 4 && d->ldg == 4 && (d->Ca == 16 || d->Ca == 32 || d->Ca == 64) &&
      d->W >= 16 && M >= (1 << 15)) {
    set_kernel(pl, d->Ca == 16 ? WG_SMALLN_16 : (d->Ca == 32 ? WG_SMALLN_32 : WG_SMALLN_64), N);
    pl->gx = pl->slabs = pl->ws_slabs = 512;
    pl->gy = pl->gz = 1;
  }
  return 0;
}

}  // namespace

int wg_mode(int a16, int g16, int planes, bool a_coef, WgMode* mode) {
  S2I_REQUIRE(planes >= 0 && planes <= 3, "wgrad(split): need 1 to 3 bf16 planes");
  S2I_REQUIRE(!(planes && (a16 || g16)), "wgrad(split): bf16 tensors go through s2i_conv_wgrad_dt");
  S2I_REQUIRE(!(a_coef && (planes || a16 || g16)), "wgrad(apply-on-load): fp32 operands only");
  if (planes) *mode = (WgMode)(WG_MODE_SPLIT1 + planes - 1);
  else if (a16 || g16) *mode = a16 && g16 ? WG_MODE_B16 : (a16 ? WG_MODE_A16 : WG_MODE_G16);
  else *mode = a_coef ? WG_MODE_F32_IN : WG_MODE_F32;
  return 0;
}

// The launch of the 32-pixel plan, in the order the kernel families claim a layer
int plan_wgrad(const s2i_wgrad_desc* d, WgMode mode, WgPlan* pl) {
  if (plan_tiles(d, mode, pl)) return 1;
  const bool g16 = mode == WG_MODE_G16 || mode == WG_MODE_B16;
  const bool stream = pl->kernel >= WG_SMALLN_16, matrix = pl->kernel < WG_F32IN_128x128;
  S2I_REQUIRE(!(stream && g16), "wgrad: the <= 4 channel gradient stream expects an fp32 output gradient");
  if (mode == WG_MODE_F32_IN)
    S2I_REQUIRE(wgrad_in_ok(d, *pl), "wgrad(apply-on-load): LeakyReLU producer, no broadcast vector, 128 x 128 tile plan (check "
                                     "s2i_conv_wgrad_in_eligible)");
  const bool chan8 = d->Cc == 0 && (d->N % 8) == 0 && (d->ldg % 8) == 0;
  const bool first_d = mode == WG_MODE_G16 && d->kind == S2I_CONV_K4S2 && d->Ca == 4 && pl->K == 64 && d->N <= 64 && chan8;
  if (first_d || (mode == WG_MODE_B16 && chan8 && (pl->Cin % 8) == 0)) {
    // the bf16 matrix cores (the first discriminator conv: fp32 NHWC4 image x bf16 output gradient, one block per split):
    // 64-pixel stages, re-cut from the split of the 32-pixel plan.  Fewer slabs may come out than the workspace was sized
    // for, and the finish must not sum slabs that nobody wrote.
    set_kernel(pl, first_d ? WG_B16D1_64x64 : WG_B16_128x128 + (pl->kernel - WG_F32_128x128), d->N);   // first_d: K = 64, N <= 64
    pl->stage = 64;
    pl->nchunks = s2i_cdiv(pl->M, 64);
    pl->cps = s2i_cdiv(pl->nchunks, pl->ws_slabs);
    pl->gz = pl->slabs = s2i_cdiv(pl->nchunks, pl->cps);
    S2I_REQUIRE(pl->slabs <= pl->ws_slabs, "wgrad(bf16): split plan mismatch");
  } else if (mode >= WG_MODE_SPLIT1 && matrix) {
    pl->planes = mode - WG_MODE_SPLIT1 + 1;
    set_kernel(pl, WG_SPLIT_128x128 + (pl->kernel - WG_F32_128x128), d->N);
  } else if (mode == WG_MODE_F32_IN) {
    pl->kernel = WG_F32IN_128x128;
  }
  return 0;
}

namespace {
size_t workspace_bytes(const s2i_wgrad_desc* d, int a16, int g16, int planes) {
  WgMode mode;
  WgPlan pl;
  if (wg_mode(a16, g16, planes, false, &mode) || plan_tiles(d, mode, &pl)) return 0;
  return wg_workspace_bytes(pl, d->N);
}
}  // namespace

extern "C" size_t s2i_wgrad_workspace_bytes(const s2i_wgrad_desc* d) { return workspace_bytes(d, 0, 0, 0); }

extern "C" size_t s2i_wgrad_workspace_bytes_dt(const s2i_wgrad_desc* d, int a_dtype, int g_dtype) {
  return workspace_bytes(d, a_dtype != 0, g_dtype != 0, 0);
}

extern "C" size_t s2i_wgrad_workspace_bytes_split(const s2i_wgrad_desc* d, int planes) { return workspace_bytes(d, 0, 0, planes); }

extern "C" int s2i_conv_wgrad_in_eligible(const s2i_wgrad_desc* d) {
  WgPlan pl;
  if (plan_tiles(d, WG_MODE_F32, &pl)) return 0;
  return wgrad_in_ok(d, pl) ? 1 : 0;
}

extern "C" int s2i_wgrad_plan_query(const s2i_wgrad_desc* d, int a_dtype, int g_dtype, int planes, int in_act, int out[12]) {
  for (int i = 0; i < 12; ++i) out[i] = 0;
  WgMode mode;
  WgPlan pl;
  if (wg_mode(a_dtype != 0, g_dtype != 0, planes, in_act != 0, &mode) || plan_wgrad(d, mode, &pl)) return 1;
  const WgKernelInfo& k = wg_kernels[pl.kernel];
  const int v[12] = {pl.kernel, k.bm, k.bn, pl.threads, pl.gx, pl.gy, pl.gz, pl.stage, pl.slabs, pl.ws_slabs, pl.K, pl.M};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
  return 0;
}
