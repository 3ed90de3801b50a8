// Forward dispatch of the implicit-GEMM convolutions: the plan (tile, K split), the workspace and statistics-row queries,
// conv_forward_impl and the s2i_conv_forward* entry points.  The kernels live in s2i_conv_fwd.hip and s2i_conv_thin.hip
// and are reached through the launch_* functions of s2i_igemm.h.
#include "s2i_igemm.h"

namespace {

// K split of a launch of `blocks` output tiles: three 256-thread blocks fit per CU, so split K until about 768 blocks exist
static int fwd_splitk(long long blocks, int nchunks, int nosplit, int min_cps) {
  int splitk = 1;
  if (blocks < 512 && nchunks >= 16 && !nosplit) {
    splitk = (int)(768 / blocks);
    if (splitk > nchunks / min_cps) splitk = nchunks / min_cps;
    if (splitk > 64) splitk = 64;
    if (splitk < 1) splitk = 1;
  }
  return splitk;
}

int plan_fwd(const s2i_conv_desc* d, FwdPlan* pl) {
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
  pl->tile = d->N > 64 ? 0 : (d->N > 32 ? 1 : 2);
  const int BN = pl->tile == 0 ? 128 : (pl->tile == 1 ? 64 : 32);
  pl->gridN = s2i_cdiv(d->N, BN);
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
    if (bm == 96 && pl->tile != 0) continue;                       // 96 x 128 only (four waves side by side)
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
  pl->gridM = s2i_cdiv(M, pl->bm);
  const int splitk = best_split;
  pl->cps = s2i_cdiv(pl->nchunks, splitk);
  pl->splitk = s2i_cdiv(pl->nchunks, pl->cps);
  pl->small_n = d->N <= 4 && d->Cc == 0 && !d->stats && (d->kind == S2I_CONV_K3S1 || d->kind == S2I_TCONV_K4S2) &&
                (pl->Ca == 16 || pl->Ca == 32 || pl->Ca == 64) && pl->M >= 4096;
  return 0;
}

// bytes of the split-K slabs (0 when K is not split)
size_t slab_bytes(const FwdPlan& pl, int N) { return pl.splitk > 1 ? (size_t)pl.splitk * pl.Mrows * N * sizeof(float) : 0; }

}  // namespace

extern "C" size_t s2i_conv_workspace_bytes(const s2i_conv_desc* d) {
  FwdPlan pl;
  if (plan_fwd(d, &pl)) return 0;
  const size_t slab = slab_bytes(pl, d->N);
  const size_t thin = thin_workspace_bytes(d, pl);
  return thin > slab ? thin : slab;
}

extern "C" int s2i_conv_stat_parts(const s2i_conv_desc* d) {
  FwdPlan pl;
  if (plan_fwd(d, &pl)) return -1;
  return stat_parts(pl, d->groups);
}

static int conv_forward_impl(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                             const unsigned short* wsp, int planes, int np, int kp, const float* bias,
                             const float* cls_bias, float* y, float* part, void* ws, size_t ws_bytes, void* stream,
                             int x16 = 0, int y16 = 0, const float* in_coef = nullptr) {
  FwdPlan pl;
  if (plan_fwd(d, &pl)) return 1;
  S2I_REQUIRE(!cls_bias || (d->kind == S2I_CONV_K3S1 && pl.splitk == 1), "conv: class bias needs an unsplit 3x3 conv");
  S2I_REQUIRE(x != nullptr || d->Cx == 0, "conv: x is null");
  S2I_REQUIRE(d->Cc == 0 || cvec != nullptr, "conv: cvec is null but Cc > 0");
  S2I_REQUIRE((w || wsp) && y, "conv: null weight/output");
  S2I_REQUIRE(!d->stats || part, "conv: stats requested without a partial buffer");
  const size_t need = slab_bytes(pl, d->N);
  S2I_REQUIRE(ws_bytes >= need && (need == 0 || ws), "conv: workspace too small (%zu < %zu)", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  IgemmP p;
  p.x = x; p.cvec = cvec; p.w = w; p.bias = bias; p.cls_bias = cls_bias; p.y = y; p.part = part; p.slab = (float*)ws;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cx = d->Cx; p.Cc = d->Cc; p.Ca = pl.Ca;
  p.Ho = pl.Ho; p.Wo = pl.Wo; p.lgWo = s2i_ilog2(pl.Wo); p.lgHoWo = s2i_ilog2(pl.Ho * pl.Wo);
  p.M = pl.M; p.N = d->N; p.K = pl.K; p.T = pl.T;
  p.kind = d->kind; p.flip = d->flip; p.act = d->act; p.stats = d->stats;
  p.splitk = pl.splitk; p.cps = pl.cps; p.nchunks = pl.nchunks;
  p.ldw = d->ldw; p.wR = d->wR; p.ldy = d->ldy; p.nparts = pl.gridM * pl.nphases;
  p.g_kw = d->kw; p.g_s = d->stride; p.g_pad = d->pad; p.wt = d->wmode != 0;
  p.Mrows = pl.Mrows;
  p.x16 = x16; p.y16 = y16;
  S2I_REQUIRE(!(wsp && (x16 || y16)), "conv(split): bf16 tensors go through s2i_conv_forward_bf16 / _dt");
  S2I_REQUIRE(!wsp || pl.bm == 128, "conv(split): the split-bf16 kernels have 128-row tiles (set tile_rows = 128)");
  p.wsp = wsp; p.wsp_np = np; p.wsp_kp = kp; p.wsp_plane = 0; p.wsp_bytes = 0;
  p.in_coef = in_coef; p.in_rows_per_group = pl.M;
  if (in_coef) {
    const int g = d->in_groups < 1 ? 1 : d->in_groups;
    S2I_REQUIRE(d->in_act == S2I_ACT_LRELU, "conv(apply-on-load): the producer's activation must be LeakyReLU (in_act=%d)", d->in_act);
    S2I_REQUIRE(!wsp && !x16 && !y16 && d->Cc == 0 && d->wmode == 0 && (pl.Ca % 32) == 0 && d->N > 4 && !bias && !cls_bias &&
                    d->kind != S2I_CONV_1D && d->kind != S2I_TCONV_K4S2,
                "conv(apply-on-load): fp32 forward of a stored tensor with 32 | Cx, no broadcast vector / bias");
    S2I_REQUIRE((pl.M % g) == 0 && (g == 1 || ((pl.M / g) % pl.bm) == 0),
                "conv(apply-on-load): %d rows do not split into %d producer groups of whole %d-row tiles", pl.M, g, pl.bm);
    p.in_rows_per_group = pl.M / g;
  }
  {
    const int r = launch_thin(d, pl, p, ws, ws_bytes, st);
    if (r >= 0) return r;
  }
  if (pl.small_n && !wsp && !cls_bias) return launch_small_n_conv(d, pl, p, st);
  dim3 grid(pl.gridM, pl.gridN, pl.nphases * pl.splitk);
  const bool wt = d->wmode != 0;
  const int wtaps = d->kind == S2I_TCONV_K4S2 ? 16 : pl.T;
  const unsigned long long xb = (unsigned long long)d->B * d->H * d->W * d->Cx * (x16 ? 2ull : 4ull);
  const unsigned long long wb = (unsigned long long)wtaps * d->wR * d->ldw * 4ull;
  S2I_REQUIRE(xb < 0x7ff00000ull && wb < 0x7ff00000ull, "conv: tensor exceeds the 2 GiB buffer-addressing window");
  p.x_bytes = (unsigned)xb;
  p.c_bytes = (unsigned)((unsigned long long)d->B * d->Cc * 4ull);
  p.w_bytes = (unsigned)wb;
  const bool ca32 = (pl.Ca % 32) == 0 && (d->Cc % 32) == 0;
  if (wsp) {
    const unsigned long long pe = (unsigned long long)wtaps * np * kp;  // elements per plane
    S2I_REQUIRE(pe * planes * 2ull < 0x7ff00000ull, "conv(split): weight planes exceed the buffer window");
    S2I_REQUIRE(kp >= pl.Ca && np >= d->N, "conv(split): weight planes %d x %d too small for N=%d K=%d", np, kp, d->N, pl.Ca);
    p.wsp_plane = (int)pe;
    p.wsp_bytes = (unsigned)(pe * planes * 2ull);
    if (launch_igemm_fwd_split(pl, p, grid, planes, st)) return 1;
  } else {
    if (launch_igemm_fwd(pl, p, grid, wt, ca32, st)) return 1;
  }
  if (pl.splitk > 1) return launch_splitk_reduce(d, pl, bias, y, part, ws, y16, stream);
  return 0;
}

extern "C" int s2i_conv_forward(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                                const float* bias, float* y, float* part, void* ws, size_t ws_bytes,
                                void* stream) {
  return s2i_conv_forward_cls(d, x, cvec, w, bias, nullptr, y, part, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_forward_cls(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                                    const float* bias, const float* cls_bias, float* y, float* part, void* ws,
                                    size_t ws_bytes, void* stream) {
  S2I_REQUIRE(w != nullptr, "conv: null weight");
  return conv_forward_impl(d, x, cvec, w, nullptr, 0, 0, 0, bias, cls_bias, y, part, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_forward_in(const s2i_conv_desc* d, const float* x_raw, const float* in_coef, const float* w, float* y,
                                   float* part, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE(w != nullptr && in_coef != nullptr, "conv(apply-on-load): null weight / coefficient table");
  return conv_forward_impl(d, x_raw, nullptr, w, nullptr, 0, 0, 0, nullptr, nullptr, y, part, ws, ws_bytes, stream, 0, 0, in_coef);
}

extern "C" int s2i_conv_split_eligible(const s2i_conv_desc* d) {
  FwdPlan pl;
  if (plan_fwd(d, &pl)) return 0;
  return (pl.Ca % 32) == 0 && (d->Cc % 32) == 0 && !pl.small_n;
}

extern "C" int s2i_conv_forward_split(const s2i_conv_desc* d, const float* x, const float* cvec,
                                      const unsigned short* wsplit, int planes, int np, int kp, const float* bias,
                                      const float* cls_bias, float* y, float* part, void* ws, size_t ws_bytes,
                                      void* stream) {
  S2I_REQUIRE(wsplit != nullptr && planes >= 1 && planes <= 3, "conv(split): need 1 to 3 bf16 planes");
  S2I_REQUIRE(np > 0 && kp > 0 && (kp % 8) == 0, "conv(split): weight rows must be multiples of 8 bf16 (kp=%d)", kp);
  S2I_REQUIRE(s2i_conv_split_eligible(d), "conv(split): layer not eligible (gathered channels must be multiples of 32)");
  return conv_forward_impl(d, x, cvec, nullptr, wsplit, planes, np, kp, bias, cls_bias, y, part, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_forward_dt(const s2i_conv_desc* d, const void* x, int x_dtype, const float* cvec, const float* w,
                                   const float* bias, const float* cls_bias, void* y, int y_dtype, float* part, void* ws,
                                   size_t ws_bytes, void* stream) {
  S2I_REQUIRE(w != nullptr, "conv: null weight");
  S2I_REQUIRE((x_dtype == S2I_DT_F32 || x_dtype == S2I_DT_BF16) && (y_dtype == S2I_DT_F32 || y_dtype == S2I_DT_BF16),
              "conv: unknown dtype");
  return conv_forward_impl(d, (const float*)x, cvec, w, nullptr, 0, 0, 0, bias, cls_bias, (float*)y, part, ws, ws_bytes,
                           stream, x_dtype == S2I_DT_BF16, y_dtype == S2I_DT_BF16);
}
