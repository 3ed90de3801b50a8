// Host planner of the forward convolutions (s2i_conv.hip fills the parameter block and launches what it decides): the matrix
// tiling and K split of a layer, the kernel its operands select, grid, preparation launch, reduction and workspace, and the
// entry points that only ask the plan a question.  No device code.
#include "s2i_igemm.h"

namespace {

// output rows (pixels of one phase) x columns per block and the block size, indexed by FwdKernel
const FwdKernelInfo fwd_kernels[FWD_KERNEL_COUNT] = {
    {128, 128, 256}, {128, 64, 256}, {128, 32, 256}, {96, 128, 256},
    {128, 128, 256}, {128, 64, 256}, {128, 32, 256}, {96, 128, 256},
    {128, 128, 256}, {128, 64, 256}, {128, 32, 256},
    // 4 / 8 / 16 lanes per pixel: 64 / 32 / 16 pixels per block
    {64, 4, 256}, {32, 4, 256}, {16, 4, 256},
    // 8 x 8 input pixels per phase; 16 x 16 output pixels
    {64, 4, 256},
    {256, 4, 256}, {256, 4, 256},
    // pixels as columns of the bf16 matrix cores: 32 per wave
    {128, 4, 256}, {128, 4, 256}, {128, 4, 256}, {128, 4, 256}, {128, 4, 256}, {128, 4, 256},
    {128, 32, 256}, {128, 64, 256}, {128, 32, 256}, {128, 64, 256},
    // one lane per pixel
    {256, 4, 256},
    {256, 16, 256}, {256, 32, 256},
};

// K split of a launch of `blocks` output tiles: three 256-thread blocks fit per CU, so split K until about 768 blocks exist
int fwd_splitk(long long blocks, int nchunks, int nosplit, int min_cps) {
  int splitk = 1;
  if (blocks < 512 && nchunks >= 16 && !nosplit) {
    splitk = (int)(768 / blocks);
    if (splitk > nchunks / min_cps) splitk = nchunks / min_cps;
    if (splitk > 64) splitk = 64;
    if (splitk < 1) splitk = 1;
  }
  return splitk;
}

// The matrix plan of a descriptor, whatever its operands: geometry, tile (named as the fp32 kernel of that shape) and K split
int plan_fwd_tiles(const s2i_conv_desc* d, FwdPlan* pl) {
  S2I_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->N > 0, "conv: non-positive extent");
  S2I_REQUIRE(d->Cx >= 0 && d->Cc >= 0 && (d->Cx % 4) == 0 && (d->Cc % 4) == 0 && d->Cx + d->Cc > 0,
              "conv: channel counts must be multiples of 4 (Cx=%d Cc=%d)", d->Cx, d->Cc);
  S2I_REQUIRE(s2i_is_pow2(d->H) && s2i_is_pow2(d->W), "conv: spatial extents must be powers of two");
  pl->Ca = d->Cx + d->Cc;
  pl->nphases = 1;
  switch (d->kind) {
    case S2I_CONV_K1: pl->T = 1; pl->Ho = d->H; pl->Wo = d->W; break;
    case S2I_CONV_K3S1: pl->T = 9; pl->Ho = d->H; pl->Wo = d->W; break;
    case S2I_CONV_K4S2:
      S2I_REQUIRE(d->H >= 2 && d->W >= 2, "conv k4s2: extent < 2");
      pl->T = 16; pl->Ho = d->H / 2; pl->Wo = d->W / 2; break;
    case S2I_TCONV_K4S2: pl->T = 4; pl->Ho = d->H; pl->Wo = d->W; pl->nphases = 4; break;
    case S2I_CONV_1D:
      S2I_REQUIRE(d->kw >= 1 && d->kw <= 31 && d->stride >= 1 && d->pad >= 0, "conv1d: bad kw/stride/pad");
      S2I_REQUIRE(d->wmode == 0 && !d->flip, "conv1d: forward only");
      pl->T = d->kw; pl->Ho = d->H; pl->Wo = (d->W + 2 * d->pad - d->kw) / d->stride + 1;
      S2I_REQUIRE(pl->Wo >= 1 && s2i_is_pow2(pl->Wo), "conv1d: output width %d is not a power of two", pl->Wo);
      break;
    default: S2I_FAIL("conv: unknown kind %d", d->kind);
  }
  const long long M = (long long)d->B * pl->Ho * pl->Wo;
  S2I_REQUIRE(M * 4 < (1ll << 31), "conv: too many rows");
  pl->M = (int)M;
  pl->Mrows = M * pl->nphases;
  pl->K = pl->T * pl->Ca;
  if (d->wmode == 0) {
    S2I_REQUIRE(d->wR >= pl->Ca, "conv: wR (%d) smaller than the gathered channels (%d)", d->wR, pl->Ca);
    S2I_REQUIRE(d->ldw >= d->N && d->ldw % 4 == 0, "conv: ldw %d too small for N %d", d->ldw, d->N);
  } else {
    S2I_REQUIRE(d->wR >= d->N, "conv(T): wR (%d) < N (%d)", d->wR, d->N);
    S2I_REQUIRE(d->ldw >= pl->Ca, "conv(T): ldw (%d) < gathered channels (%d)", d->ldw, pl->Ca);
  }
  S2I_REQUIRE(d->ldy >= d->N, "conv: ldy < N");
  S2I_REQUIRE(!(d->stats && (d->act != S2I_ACT_NONE)), "conv: stats epilogue needs act NONE");
  if (d->stats && d->groups > 1) {
    // independent BatchNorm batches stacked along the rows: a row tile must not straddle two of them (tile heights are
    // checked per candidate below; 96-row tiles exist only for N > 64)
    S2I_REQUIRE(d->kind != S2I_TCONV_K4S2 && (M % d->groups) == 0 &&
                    (((M / d->groups) % 128) == 0 || (d->N > 64 && ((M / d->groups) % 96) == 0 && d->tile_rows != 128)),
                "conv: %lld rows do not split into %d BatchNorm groups of whole row tiles", M, d->groups);
    S2I_REQUIRE((d->N % 4) == 0, "conv: grouped statistics need N %% 4 == 0");
  }
  pl->kernel = d->N > 64 ? FWD_F32_128x128 : (d->N > 32 ? FWD_F32_128x64 : FWD_F32_128x32);
  pl->gridN = s2i_cdiv(d->N, fwd_kernels[pl->kernel].bn);
  pl->nchunks = s2i_cdiv(pl->K, 32);
  // Rows per tile.  The chip holds 768 blocks at a time (three per CU); a launch whose tiles x K-splits fill whole
  // rounds of them runs at 121 - 125 TFLOP/s, one that ends on 0.5 or 0.75 of a round at ~100
  // (profiles/r02_f32_per_launch_table.txt).  The discriminators' stacked passes have 72 = 8 x 9 images, so 128-row
  // tiles give 9 x 2^k of them (576, 1152: 0.75 / 1.5 rounds) where 96-row tiles give 3 x 2^k (768, 1536).  (192 x 128
  // tiles need 168+ registers: no third block per CU, and at two per CU a round holds the same rows as with 128.)
  // Candidates are priced as rounds x (chunks per block + a fixed prologue / epilogue share) x rows, the smaller
  // tile with the measured relative cost of its matrix loop.
  const int forced_bm = d->tile_rows ? d->tile_rows : s2i_tune(S2I_TUNE_FWD_BM, 0);
  S2I_REQUIRE(forced_bm == 0 || forced_bm == 96 || forced_bm == 128, "conv: tile_rows must be 0, 96 or 128");
  const int min_cps = s2i_tune(S2I_TUNE_FWD_MIN_CPS, 4);
  static const int cand_bm[2] = {128, 96};
  double best = 1e300;
  int best_bm = 128, best_split = 1;
  for (int c = 0; c < 2; ++c) {
    const int bm = cand_bm[c];
    if (forced_bm ? bm != forced_bm : false) continue;
    if (bm == 96 && pl->kernel != FWD_F32_128x128) continue;       // 96 x 128 only (four waves side by side)
    if (bm != 128 && (d->kind == S2I_CONV_1D || M < 2 * bm)) continue;
    if (d->stats && d->groups > 1 && ((M / d->groups) % bm) != 0) continue;
    const long long blocks = (long long)s2i_cdiv(M, bm) * pl->gridN * pl->nphases;
    const int sk0 = fwd_splitk(blocks, pl->nchunks, d->nosplit, min_cps);
    const int cps = s2i_cdiv(pl->nchunks, sk0), sk = s2i_cdiv(pl->nchunks, cps);
    const double rounds = (double)((blocks * sk + 767) / 768);
    const double rel = bm == 128 ? 1.0 : 0.80;   // time of one chunk of a block, 128 rows = 1
    // slab write + read at ~4 TB/s in units of one chunk round of the chip (768 x 128 x 128 x 32 MACs at 122 TFLOP/s = 6.6 us)
    const double slab = sk > 1 ? 3.0e-7 * sk * (double)pl->Mrows * d->N : 0.0;
    const double cost = rounds * (cps + 3.0) * rel + slab + (sk > 1 ? 2.0 : 0.0);
    if (cost < best * (bm == 128 ? 1.0 : 0.97)) { best = cost; best_bm = bm; best_split = sk; }
  }
  S2I_REQUIRE(best < 1e300 || !(d->stats && d->groups > 1 && ((M / d->groups) % 128) != 0),
              "conv: no tile height fits the %d BatchNorm groups of %lld rows", d->groups, M / (d->groups > 0 ? d->groups : 1));
  if (best == 1e300) { best_bm = 128; best_split = fwd_splitk((long long)s2i_cdiv(M, 128) * pl->gridN * pl->nphases, pl->nchunks, d->nosplit, min_cps); }
  pl->bm = best_bm;
  if (best_bm == 96) pl->kernel = FWD_F32_96x128;
  pl->gridM = s2i_cdiv(M, pl->bm);
  pl->cps = s2i_cdiv(pl->nchunks, best_split);
  pl->splitk = s2i_cdiv(pl->nchunks, pl->cps);
  return 0;
}

// <= 4 output channels of a 3x3 / transposed layer: small_n_conv_kernel where no thin kernel takes the layer
bool small_n_ok(const s2i_conv_desc* d, const FwdPlan& pl) {
  return d->N <= 4 && d->Cc == 0 && !d->stats && (d->kind == S2I_CONV_K3S1 || d->kind == S2I_TCONV_K4S2) &&
         (pl.Ca == 16 || pl.Ca == 32 || pl.Ca == 64) && pl.M >= 4096;
}
// the split-bf16 kernels gather 32 channels at a time
bool split_ok(const s2i_conv_desc* d, const FwdPlan& pl) { return (pl.Ca % 32) == 0 && (d->Cc % 32) == 0 && !small_n_ok(d, pl); }

// thin layers (one lane per output pixel, weights as a scalar table in the workspace): 1 = few outputs, 2 = 4 inputs
int thin_kind(const s2i_conv_desc* d, const FwdPlan& pl) {
  if (d->Cc != 0 || d->stats || pl.M < 4096 || pl.splitk != 1) return 0;
  // measured (bf16 mode, batch 48): few outputs from 16 / 32 channels 113 / 66 us against 273 / 135 us for the
  // lanes-per-pixel kernel; from 64 channels the lane-per-pixel reads (128-byte pixels, one 16-byte piece per instruction)
  // thrash L1: 703 against 280 us, so that case stays with small_n_conv_kernel.  4 inputs to 16 / 32 outputs 78 / 43 us
  // against 225 / 64 us on the matrix kernel; to 64 outputs (first discriminator conv, 4096 FMAs per pixel) the vector
  // units tie with the fp32 matrix kernel (310 vs 315 us) and lose at batch 48 (152 vs 113): not taken.
  if (d->N <= 4 && (d->kind == S2I_CONV_K3S1 || d->kind == S2I_TCONV_K4S2) && (pl.Ca % 8) == 0 && pl.Ca <= 32) return 1;
  if (pl.Ca == 4 && d->kind == S2I_CONV_K3S1 && (d->N == 16 || d->N == 32) && (d->ldy % 8) == 0) return 2;
  return 0;
}
// transposed conv to <= 4 channels from 64 stored channels on maps of whole 8 x 8 tiles: tconv_n4_tile_kernel
bool tile_n4_ok(const s2i_conv_desc* d, const FwdPlan& pl) {
  return d->kind == S2I_TCONV_K4S2 && d->N <= 4 && d->Cc == 0 && !d->stats && pl.Ca == 64 && (d->H % 8) == 0 && (d->W % 8) == 0 &&
         pl.M >= 4096 && pl.splitk == 1;
}
// conv3x3 to <= 4 channels from 16 / 32 / 64 stored channels on maps of whole 16 x 16 tiles: conv3_n4_tile_kernel
bool tile3_n4_ok(const s2i_conv_desc* d, const FwdPlan& pl) {
  return d->kind == S2I_CONV_K3S1 && d->N <= 4 && d->Cc == 0 && !d->stats && (pl.Ca == 16 || pl.Ca == 32 || pl.Ca == 64) &&
         (d->H % 16) == 0 && (d->W % 16) == 0 && pl.M >= 4096 && pl.splitk == 1;
}
// bf16-mode image layers on the matrix cores with pixels as columns: 1 = few outputs from bf16 input, 2 = fp32 NHWC4 input to
// bf16 output (the dtype combination decides: these are the edges of the bf16 activation mode only)
int rgb_kind(const s2i_conv_desc* d, const FwdPlan& pl, int x16, int y16) {
  if (d->Cc != 0 || d->stats || pl.M < 4096) return 0;
  if (x16 && !y16 && d->N <= 4 && (d->kind == S2I_CONV_K3S1 || d->kind == S2I_TCONV_K4S2) &&
      (pl.Ca == 16 || pl.Ca == 32 || pl.Ca == 64))
    return 1;
  if (!x16 && y16 && pl.Ca == 4 && (d->kind == S2I_CONV_K3S1 || d->kind == S2I_CONV_K4S2) &&
      (d->N == 16 || d->N == 32 || d->N == 64) && (d->ldy % 4) == 0)
    return 2;
  return 0;
}

// A kernel that takes the layer off the matrix tiles: its grid, and the table (4-byte) or fragment (2-byte) elements a
// preparation launch writes into the workspace for it
struct FwdCand { bool ok; FwdKernel kernel; int gx, gz, prep_elems, prep_bytes; };
int capped(int blocks, int cap) { return blocks > cap ? cap : blocks; }

// The candidates in dispatch order: the first that is ok runs.  All of them take fp32 weights, no class bias and no
// apply-on-load (plan_fwd asks only then).
void thin_candidates(const s2i_conv_desc* d, const FwdPlan& pl, const FwdMode& m, FwdCand (&c)[4]) {
  const int nph = pl.nphases;
  c[0] = {tile_n4_ok(d, pl) && !m.y16, FWD_TCONV_N4_64, (d->H / 8) * (d->W / 8) * d->B, 1, 4 * 4 * 64 * 4, 4};
  c[1] = {tile3_n4_ok(d, pl) && !m.y16, pl.Ca == 16 ? FWD_CONV3_N4_16 : FWD_CONV3_N4_32, (d->H / 16) * (d->W / 16) * d->B, 1,
          9 * pl.Ca * 4, 4};
  const int rk = rgb_kind(d, pl, m.x16, m.y16), r128 = capped(s2i_cdiv(pl.M, 128), 2048);
  if (rk == 1) {          // k-steps of 16: 3x3 from 16 / 32 / 64 channels 9 / 18 / 36, the transposed conv's 2x2 taps 4 / 8 / 16
    const int ks = pl.T * pl.Ca / 16;
    const FwdKernel k = ks == 4 ? FWD_RGB_OUT_4 : ks == 8 ? FWD_RGB_OUT_8 : ks == 9 ? FWD_RGB_OUT_9 : ks == 16 ? FWD_RGB_OUT_16 :
                        ks == 18 ? FWD_RGB_OUT_18 : FWD_RGB_OUT_36;
    c[2] = {true, k, capped(r128, 2048 / nph), nph, nph * ks * 64 * 8, 2};
  } else {                // a k-step per kernel row; with a bias rgb_in declines
    const int mt = rk == 2 ? (d->N + 31) / 32 : 1, kh = d->kind == S2I_CONV_K4S2 ? 4 : 3;   // rgb_kind: N = 16 / 32 / 64
    c[2] = {rk == 2 && !m.bias, (FwdKernel)(FWD_RGB_IN_1x3 + (mt - 1) + 2 * (kh - 3)), r128, 1, mt * kh * 64 * 8, 2};
  }
  const int tk = thin_kind(d, pl), r256 = s2i_cdiv(pl.M, 256);
  // thin_out's table has 4 columns per (tap, channel); columns beyond N read the zero padding of the packed weights.
  // thin_kind admits 16 and 32 outputs only for thin_in (64 ties with the matrix kernel, see there)
  if (tk == 2) c[3] = {true, d->N == 16 ? FWD_THIN_IN_16 : FWD_THIN_IN_32, capped(r256, 4096), 1, pl.T * 4 * d->N, 4};
  else c[3] = {tk == 1, FWD_THIN_OUT, capped(r256, 4096 / nph), nph, nph * pl.T * pl.Ca * 4, 4};
}

size_t slab_bytes(const FwdPlan& pl, int N) { return pl.splitk > 1 ? (size_t)pl.splitk * pl.Mrows * N * sizeof(float) : 0; }

// The launch of a tiled layer (pl: plan_fwd_tiles) in this operand mode, in the order the kernel families claim it
int plan_fwd_kernel(const s2i_conv_desc* d, const FwdMode& m, FwdPlan* pl) {
  S2I_REQUIRE(!m.cls_bias || (d->kind == S2I_CONV_K3S1 && pl->splitk == 1), "conv: class bias needs an unsplit 3x3 conv");
  if (m.planes) {
    S2I_REQUIRE(split_ok(d, *pl), "conv(split): layer not eligible (gathered channels must be multiples of 32)");
    S2I_REQUIRE(pl->bm == 128, "conv(split): the split-bf16 kernels have 128-row tiles (set tile_rows = 128)");
  }
  if (m.in_act) {
    const int g = d->in_groups < 1 ? 1 : d->in_groups;
    S2I_REQUIRE(d->in_act == S2I_ACT_LRELU, "conv(apply-on-load): the producer's activation must be LeakyReLU (in_act=%d)", d->in_act);
    S2I_REQUIRE(!m.planes && !m.x16 && !m.y16 && d->Cc == 0 && d->wmode == 0 && (pl->Ca % 32) == 0 && d->N > 4 && !m.bias && !m.cls_bias &&
                    d->kind != S2I_CONV_1D && d->kind != S2I_TCONV_K4S2,
                "conv(apply-on-load): fp32 forward of a stored tensor with 32 | Cx, no broadcast vector / bias");
    S2I_REQUIRE((pl->M % g) == 0 && (g == 1 || ((pl->M / g) % pl->bm) == 0),
                "conv(apply-on-load): %d rows do not split into %d producer groups of whole %d-row tiles", pl->M, g, pl->bm);
  }
  pl->wt = d->wmode != 0;
  pl->ca32 = (pl->Ca % 32) == 0 && (d->Cc % 32) == 0;
  pl->planes = m.planes;
  pl->gy = 1;
  pl->prep_elems = 0;
  pl->reduce = FWD_REDUCE_NONE;
  size_t prep_bytes = 0;
  const FwdCand* take = nullptr;
  FwdCand c[4];
  if (!m.planes && !m.cls_bias && !m.in_act) {
    thin_candidates(d, *pl, m, c);
    for (int i = 0; i < 4 && !take; ++i)
      if (c[i].ok) take = &c[i];
  }
  if (take) {
    pl->kernel = take->kernel;
    pl->gx = take->gx;
    pl->gz = take->gz;
    pl->prep_elems = take->prep_elems;
    prep_bytes = (size_t)take->prep_elems * take->prep_bytes;
  } else if (small_n_ok(d, *pl) && !m.planes && !m.cls_bias) {
    // HBM-bound RGB-sized layers: VALU kernel instead of a 32-wide MFMA tile that is 7/8 padding
    pl->kernel = pl->Ca == 16 ? FWD_SMALLN_4 : (pl->Ca == 32 ? FWD_SMALLN_8 : FWD_SMALLN_16);
    pl->gx = capped(s2i_cdiv(pl->M, fwd_kernels[pl->kernel].bm), 2048 / pl->nphases);   // 8 blocks per CU; the kernel strides over the rest
    pl->gz = pl->nphases;
  } else {
    const int shape = pl->kernel - FWD_F32_128x128;
    if (m.planes) pl->kernel = (FwdKernel)(FWD_SPLIT_128x128 + shape);
    else if (m.in_act) pl->kernel = (FwdKernel)(FWD_F32IN_128x128 + shape);
    pl->gx = pl->gridM;
    pl->gy = pl->gridN;
    pl->gz = pl->nphases * pl->splitk;
    if (pl->splitk > 1) {
      const bool quads = (d->N % 4) == 0 && (d->ldy % 4) == 0;
      pl->reduce = !d->stats ? FWD_REDUCE_PLAIN : (quads ? FWD_REDUCE_STATS : FWD_REDUCE_COLSTATS);
      S2I_REQUIRE(!(pl->reduce == FWD_REDUCE_COLSTATS && m.y16), "conv: bf16 output with statistics needs N %% 4 == 0 on a split-K layer");
    }
  }
  pl->threads = fwd_kernels[pl->kernel].threads;
  const size_t slab = slab_bytes(*pl, d->N);
  pl->ws_bytes = prep_bytes > slab ? prep_bytes : slab;
  return 0;
}

}  // namespace

int fwd_mode(int x16, int y16, int planes, bool bias, bool cls_bias, bool in_coef, FwdMode* mode) {
  S2I_REQUIRE(planes >= 0 && planes <= 3, "conv(split): need 1 to 3 bf16 planes");
  S2I_REQUIRE(!(planes && (x16 || y16)), "conv(split): bf16 tensors go through s2i_conv_forward_bf16 / _dt");
  *mode = {x16, y16, planes, bias, cls_bias, in_coef};
  return 0;
}

int plan_fwd(const s2i_conv_desc* d, const FwdMode& mode, FwdPlan* pl) { return plan_fwd_tiles(d, pl) || plan_fwd_kernel(d, mode, pl); }

// The caller does not say which dtypes it will launch with: the largest workspace over the four combinations, and in each
// the largest buffer among ALL the thin / RGB kernels the layer qualifies for, not only the one the dispatch order picks.
extern "C" size_t s2i_conv_workspace_bytes(const s2i_conv_desc* d) {
  FwdPlan pl;
  if (plan_fwd_tiles(d, &pl)) return 0;
  size_t need = slab_bytes(pl, d->N);
  for (int dt = 0; dt < 4; ++dt) {
    FwdCand c[4];
    thin_candidates(d, pl, FwdMode{dt & 1, dt >> 1, 0, false, false, false}, c);
    for (const FwdCand& k : c)
      if (k.ok && (size_t)k.prep_elems * k.prep_bytes > need) need = (size_t)k.prep_elems * k.prep_bytes;
  }
  return need;
}

extern "C" int s2i_conv_stat_parts(const s2i_conv_desc* d) {
  FwdPlan pl;
  if (plan_fwd_tiles(d, &pl)) return -1;
  return stat_parts(pl, d->groups);
}

extern "C" int s2i_conv_split_eligible(const s2i_conv_desc* d) {
  FwdPlan pl;
  if (plan_fwd_tiles(d, &pl)) return 0;
  return split_ok(d, pl) ? 1 : 0;
}

extern "C" int s2i_conv_plan_query(const s2i_conv_desc* d, int x_dtype, int y_dtype, int planes, int has_bias, int has_cls_bias,
                                   int out[15]) {
  for (int i = 0; i < 15; ++i) out[i] = 0;
  FwdMode mode;
  FwdPlan pl;
  if (fwd_mode(x_dtype != 0, y_dtype != 0, planes, has_bias != 0, has_cls_bias != 0, d->in_act != 0, &mode) || plan_fwd(d, mode, &pl))
    return 1;
  const FwdKernelInfo& k = fwd_kernels[pl.kernel];
  const int v[15] = {pl.kernel, k.bm, k.bn, pl.threads, pl.gx, pl.gy, pl.gz, pl.splitk, pl.cps, pl.nchunks, pl.prep_elems,
                     pl.reduce, (int)pl.ws_bytes, pl.M, pl.K};
  for (int i = 0; i < 15; ++i) out[i] = v[i];
  return 0;
}
