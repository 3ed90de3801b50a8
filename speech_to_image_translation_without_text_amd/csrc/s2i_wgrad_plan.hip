// Host planner of the weight gradients (s2i_wgrad.hip launches what it decides): tile, grid and pixel-range split per layer,
// and the entry points that only ask the plan a question.  No device code.
#include "s2i_igemm.h"

// planes: 0 fp32 operands, 1..3 split-bf16 products (or one operand bf16), 16 both operands stored as bf16
int plan_wgrad(const s2i_wgrad_desc* d, WgPlan* pl, int planes) {
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
  pl->tile = d->N > 64 ? 0 : (d->N > 32 ? 1 : 2);
  if (pl->K <= 64 && d->N > 32 && d->N <= 64) pl->tile = 3;  // first discriminator conv: 16 taps x (3+1) channels
  // K = 288 (3x3 taps x 32 channels, the generator's last stage) wastes a quarter of three 128-row tiles: 96-row tiles
  if (!planes && pl->K % 96 == 0 && d->N <= 64 && s2i_cdiv(pl->K, 128) * 128 * 5 > pl->K * 6) pl->tile = d->N > 32 ? 4 : 5;
  const int BN = pl->tile == 0 ? 128 : ((pl->tile == 2 || pl->tile == 5) ? 32 : 64);
  const int BM = pl->tile == 3 ? 64 : (pl->tile >= 4 ? 96 : 128);
  pl->gridK = s2i_cdiv(pl->K, BM);
  pl->gridN = s2i_cdiv(d->N, BN);
  pl->nchunks = s2i_cdiv(M, 32);
  const long long tiles = (long long)pl->gridK * pl->gridN;
  // three resident blocks per CU hide each other's load latency: split the pixel range so that tiles x splits fill whole
  // rounds of the chip's 768 block slots (512 tiles x 1 = 0.67 of a round ran at 108 TFLOP/s, profiles/r02_f32_per_launch_table.txt),
  // priced as rounds x (chunks per block + a fixed share) + the fp32 slabs each split writes and the finish pass reads
  // (units: one chunk round of the chip, 6.6 us)
  int splitk = 1;
  {
    int smax = pl->nchunks / 4;
    if (smax > 256) smax = 256;
    if (smax < 1) smax = 1;
    double best = 1e300;
    for (int sc = 1; sc <= smax; ++sc) {
      const int cps = s2i_cdiv(pl->nchunks, sc), se = s2i_cdiv(pl->nchunks, cps);
      if (se != sc) continue;                       // same effective split as a smaller candidate
      const double rounds = (double)((tiles * se + 767) / 768);
      const double cost = rounds * (cps + 3.0) + 3.0e-7 * se * (double)pl->K * d->N;
      if (cost < best) { best = cost; splitk = se; }
      if (tiles * sc > 4 * 768) break;
    }
  }
  if (!planes && pl->tile == 0 && (pl->K % 256) == 0 && !d->a_act && s2i_tune(S2I_TUNE_WGRAD_BM, 0) != 128) {
    // fp32 256 x 128 tiles on 512-thread blocks (two per CU, 512 slots): half the `g` re-reads of the 128 x 128 form; a round
    // of chunks takes 1.26x as long for 1.33x the work (8.3 us against 6.6: tools/wgrad_bench.py, 103 -> 119 TFLOP/s on
    // D_NET256's first stacked weight gradient).  Taken where the same cost model prices it lower.
    const long long t2 = (long long)(pl->K / 256) * pl->gridN;
    int smax = pl->nchunks / 4, s8 = 1;
    if (smax > 256) smax = 256;
    if (smax < 1) smax = 1;
    double best8 = 1e300, cost0 = 1e300;
    for (int sc = 1; sc <= smax; ++sc) {
      const int cps = s2i_cdiv(pl->nchunks, sc), se = s2i_cdiv(pl->nchunks, cps);
      if (se != sc) continue;
      const double cost = (double)((t2 * se + 511) / 512) * (cps + 3.0) * 1.26 + 3.0e-7 * se * (double)pl->K * d->N;
      if (cost < best8) { best8 = cost; s8 = se; }
      if (t2 * sc > 4 * 512) break;
    }
    {
      const int cps = s2i_cdiv(pl->nchunks, splitk), se = s2i_cdiv(pl->nchunks, cps);
      cost0 = (double)((tiles * se + 767) / 768) * (cps + 3.0) + 3.0e-7 * se * (double)pl->K * d->N;
    }
    // 256 x 256 tiles on one 1024-thread block per CU (256 slots) where 256 divides N: a round of chunks takes 1.22x the
    // 128 x 128 round for 1.33x the work (D_NET256's three middle layers 0.650 -> 0.628 ms, profiles/r03_f32_wgrad_tile_heights.txt)
    int s9 = 1;
    double best9 = 1e300;
    if ((d->N % 256) == 0) {
      const long long t3 = (long long)(pl->K / 256) * (d->N / 256);
      for (int sc = 1; sc <= smax; ++sc) {
        const int cps = s2i_cdiv(pl->nchunks, sc), se = s2i_cdiv(pl->nchunks, cps);
        if (se != sc) continue;
        const double cost = (double)((t3 * se + 255) / 256) * (cps + 3.0) * 1.22 + 3.0e-7 * se * (double)pl->K * d->N;
        if (cost < best9) { best9 = cost; s9 = se; }
        if (t3 * sc > 4 * 256) break;
      }
    }
    const int force = s2i_tune(S2I_TUNE_WGRAD_BM, 0);   // 0 model, 128 / 256 / 512 (= 256 x 256) forced where eligible
    if ((force == 512 && best9 < 1e300) || (force == 0 && best9 < best8 && best9 < cost0)) {
      pl->tile = 9;
      pl->gridK = pl->K / 256;
      pl->gridN = d->N / 256;
      splitk = s9;
    } else if (best8 < cost0 || force == 256 || force == 512) {
      pl->tile = 8;
      pl->gridK = pl->K / 256;
      splitk = s8;
    }
  }
  pl->cps = s2i_cdiv(pl->nchunks, splitk);
  pl->splitk = s2i_cdiv(pl->nchunks, pl->cps);
  if (planes == 16 && pl->tile == 0 && (pl->K % 256) == 0 && (pl->Cin % 8) == 0 && d->Cc == 0 && (d->N % 8) == 0 &&
      (d->ldg % 8) == 0 && s2i_tune(S2I_TUNE_WGRAD16_BM, 0) != 128) {
    // both operands bf16: 256 x 128 tiles on 512-thread blocks, two per CU (512 slots), 64-pixel stages -- where that is
    // cheaper than the 128 x 128 plan above under one model for both (us; measured on the config-4 layers,
    // tools/wgrad16_bench.py: a round of 64-pixel stages takes ~2.5 us with 768 blocks of 128 x 128 and ~2.7 us with 512
    // blocks of 256 x 128; a block's prologue / epilogue is worth 3 resp. 2 stages; each split writes and re-reads a slab)
    const int nch64 = s2i_cdiv(M, 64);
    const double slab_us = 2.0e-6 * (double)pl->K * d->N;
    const int cps128 = s2i_cdiv(nch64, pl->splitk), se128 = s2i_cdiv(nch64, cps128);
    const double cost128 = (double)((tiles * se128 + 767) / 768) * (cps128 + 3.0) * 2.5 + slab_us * se128;
    const long long t2 = (long long)(pl->K / 256) * pl->gridN;
    int smax = nch64 / 4, best_s = 1;
    if (smax > 256) smax = 256;
    if (smax < 1) smax = 1;
    double best = 1e300;
    for (int sc = 1; sc <= smax; ++sc) {
      const int cps = s2i_cdiv(nch64, sc), se = s2i_cdiv(nch64, cps);
      if (se != sc) continue;
      const double cost = (double)((t2 * se + 511) / 512) * (cps + 2.0) * 2.7 + slab_us * se;
      if (cost < best) { best = cost; best_s = se; }
      if (t2 * sc > 4 * 512) break;
    }
    // 256 x 256 tiles, one 1024-thread block per CU (256 slots), where 256 divides N: ~2.15 us per round of stages
    int best3_s = 1;
    double best3 = 1e300;
    if ((d->N % 256) == 0) {
      const long long t3 = (long long)(pl->K / 256) * (d->N / 256);
      for (int sc = 1; sc <= smax; ++sc) {
        const int cps = s2i_cdiv(nch64, sc), se = s2i_cdiv(nch64, cps);
        if (se != sc) continue;
        const double cost = (double)((t3 * se + 255) / 256) * (cps + 3.0) * 2.15 + slab_us * se;
        if (cost < best3) { best3 = cost; best3_s = se; }
        if (t3 * sc > 4 * 256) break;
      }
    }
    const int force = s2i_tune(S2I_TUNE_WGRAD16_BM, 0);   // 0 model, 128 / 256 / 512 (= 256 x 256) forced where eligible
    int pick = 0;
    if (force == 512 && best3 < 1e300) pick = 7;
    else if (force == 256 || force == 512) pick = 6;
    else if (force == 0) {
      const double m = best3 < best ? best3 : best;
      if (m < cost128) pick = best3 < best ? 7 : 6;
    }
    if (pick) {
      const int bs = pick == 7 ? best3_s : best_s;
      pl->tile = pick;
      pl->gridK = pl->K / 256;
      if (pick == 7) pl->gridN = d->N / 256;
      // kept in 32-pixel chunks like the other plans (the launcher re-derives the 64-pixel stages from splitk)
      pl->cps = s2i_cdiv(pl->nchunks, bs);
      pl->splitk = s2i_cdiv(pl->nchunks, pl->cps);
    }
  }
  // thin 3x3 layers over wide maps: one kernel row per block, taps read from a staged row segment
  pl->rows3 = !planes && d->kind == S2I_CONV_K3S1 && d->Cc == 0 && (d->Ca == 32 || d->Ca == 64) && d->W >= 32 &&
              (d->N % 32) == 0 && d->N <= 128;
  if (pl->rows3) {
    pl->bn3 = (d->Ca == 64 && d->N > 64) ? 128 : (d->N > 32 ? 64 : 32);
    pl->gridN = s2i_cdiv(d->N, pl->bn3);
    // measured (24x128x128, 32->64): 512 / 768 / 1024 / 1536 blocks = 211 / 202 / 183 / 234 us; four 192-thread blocks or
    // three 256-thread blocks fill a CU, more only adds slab traffic
    const int target = d->Ca == 32 ? 1024 : 768;
    int sk = target / ((d->Ca == 32 ? 1 : 3) * pl->gridN);
    if (sk > pl->nchunks / 4) sk = pl->nchunks / 4;
    if (sk > 2048) sk = 2048;
    if (sk < 1) sk = 1;
    pl->cps = s2i_cdiv(pl->nchunks, sk);
    pl->splitk = s2i_cdiv(pl->nchunks, pl->cps);
  }
  // <= 4 output channels of a 3x3 conv: streamed on the vector units, one slab per block
  pl->small_n = d->kind == S2I_CONV_K3S1 && d->Cc == 0 && d->N == 4 && d->ldg == 4 &&
                (d->Ca == 16 || d->Ca == 32 || d->Ca == 64) && d->W >= 16 && M >= (1 << 15);
  if (pl->small_n) pl->splitk = 512;
  return 0;
}

// apply-on-load weight gradient: the generic 128 x 128 fp32 kernel only (the discriminator towers' layers)
bool wgrad_in_ok(const s2i_wgrad_desc* d, const WgPlan& pl) {
  const int g = d->a_groups < 1 ? 1 : d->a_groups;
  return d->a_act == S2I_ACT_LRELU && d->Cc == 0 && !d->swap && !pl.rows3 && !pl.small_n && pl.tile == 0 && g <= 3 &&
         (d->B % g) == 0;
}

extern "C" size_t s2i_wgrad_workspace_bytes(const s2i_wgrad_desc* d) {
  WgPlan pl;
  if (plan_wgrad(d, &pl)) return 0;
  return (size_t)pl.splitk * pl.K * d->N * sizeof(float);
}

extern "C" int s2i_conv_wgrad_in_eligible(const s2i_wgrad_desc* d) {
  WgPlan pl;
  if (plan_wgrad(d, &pl)) return 0;
  return wgrad_in_ok(d, pl) ? 1 : 0;
}

extern "C" size_t s2i_wgrad_workspace_bytes_dt(const s2i_wgrad_desc* d, int a_dtype, int g_dtype) {
  WgPlan pl;
  if (plan_wgrad(d, &pl, (a_dtype && g_dtype) ? 16 : ((a_dtype || g_dtype) ? 1 : 0))) return 0;
  return (size_t)pl.splitk * pl.K * d->N * sizeof(float);
}

extern "C" size_t s2i_wgrad_workspace_bytes_split(const s2i_wgrad_desc* d, int planes) {
  WgPlan pl;
  if (plan_wgrad(d, &pl, planes)) return 0;
  return (size_t)pl.splitk * pl.K * d->N * sizeof(float);
}
