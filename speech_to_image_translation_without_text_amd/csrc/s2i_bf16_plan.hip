// bf16 activation path: the launch plan -- tile, K split, kernel, grid and LDS size, decided here and nowhere else -- its
// query and the entry point of the convolution (no kernel: s2i_bf16_conv.hip, s2i_bf16_conv_v2.hip and s2i_bf16_pack.hip
// hold them; s2i_bf16.h says what the path is).
#include "s2i_bf16.h"

namespace {

// tile of bm output pixels: as wide as the map allows (up to 32), then rows, then images; and the input patch it reads
struct TileGeom { int tw, th, tb, PH, PW, npix; };

TileGeom tile_geom(int kb, int Ho, int Wo, int bm) {
  TileGeom g;
  g.tw = Wo < 32 ? Wo : 32;
  g.th = bm / g.tw;
  if (g.th > Ho) g.th = Ho;
  g.tb = bm / (g.tw * g.th);
  if (kb == KB_K3S1) { g.PH = g.th + 2; g.PW = g.tw + 2; }
  else if (kb == KB_K4S2) { g.PH = 2 * g.th + 2; g.PW = 2 * g.tw + 2; }
  else { g.PH = g.th + 1; g.PW = g.tw + 1; }
  g.npix = g.tb * g.PH * g.PW;
  return g;
}

size_t workspace_bytes(const s2i_conv_desc* d, const BPlan& pl) {
  return pl.splitk > 1 ? (size_t)pl.splitk * pl.Mrows * d->N * sizeof(float) : 0;
}

// the 66-pixel-wide stride-2 patch (32-column tiles) takes the padded-row instantiation
bool v2_padded(const BPlan& pl) { return pl.v2 && pl.kb == KB_K4S2 && pl.PW == 66 && pl.CK == 32; }

// one patch buffer in LDS
size_t patch_bytes(const BPlan& pl) {
  return ((size_t)pl.npix * (pl.CK * 2 + (v2_padded(pl) ? 16 : 0)) + 255) & ~(size_t)255;
}

// dynamic LDS: [patch | weight stage], or for the 256-pixel kernel [patch (x2) | weight stage x2 | 1 KB sink]; reused by the
// epilogue
size_t smem_bytes(const BPlan& pl) {
  const size_t ab = patch_bytes(pl), stage = (size_t)pl.TG * pl.BN * pl.CK * 2;
  const size_t main_b = pl.v2 ? (pl.kb == KB_K4S2 ? 1 : 2) * ab + 2 * stage + 1024 : ab + stage;
  const size_t epi = bf16_epilogue_bytes(pl.v2 ? 256 : 128, pl.BN);
  return main_b > epi ? main_b : epi;
}

// blocks along x for the second-generation kernel: persistent (one block per CU looping over its tiles) where the kernel
// supports it -- single patch buffer, no split-K, and a patch region large enough for the epilogue's transpose
int v2_grid_x(const BPlan& pl) {
  const int pers = s2i_tune(S2I_TUNE_B16_PERSIST, 1);
  if (!pers || pl.kb != KB_K4S2 || pl.splitk != 1 || patch_bytes(pl) < bf16_epilogue_bytes(256, 128)) return pl.gridM;
  int nblk = (pers > 1 ? pers : 256) / (pl.gridN * pl.nphases);   // knob b16_persist > 1: that many block slots (tests)
  if (nblk < 1) nblk = 1;
  if (pl.gridM <= nblk) return pl.gridM;
  // a block walks ceil(gridM / nblk) tiles: persistent only where that rounding costs little (measured: 144 tiles over
  // 64 slots -- 3 rounds for 2.25 rounds of work -- lost what the prefetch across tiles gained)
  if (pers == 1 && (pl.gridM % nblk) != 0 && pl.gridM < 6 * nblk) return pl.gridM;
  return nblk;
}

// the instantiation a finished tile plan runs on.  conv_bf16_kernel is matched on (kind, BN, CK): a TG its instantiation does
// not have is refused by launch_conv_bf16, not here
B16Kernel pick_kernel(const BPlan& pl) {
  if (pl.v2) return pl.kb == KB_K3S1 ? B16_V2_K3S1 : pl.kb == KB_TCONV ? B16_V2_TCONV : v2_padded(pl) ? B16_V2_K4S2_PW66 : B16_V2_K4S2;
#define S2I_CASE(K, bn, ck, tg) if (pl.kb == KB_##K && pl.BN == bn && pl.CK == ck) return B16_##K##_##bn##x##ck;
  S2I_BF16_TILES(S2I_CASE)
#undef S2I_CASE
  return B16_NO_KERNEL;
}

}  // namespace

const char* const b16_kernel_names[B16_KERNEL_COUNT] = {
#define S2I_NAME(K, bn, ck, tg) #K "_" #bn "x" #ck,
    S2I_BF16_TILES(S2I_NAME)
#undef S2I_NAME
#define S2I_NAME(id, K, ck, tg, pdb, pwc) #id,
    S2I_BF16_V2_TILES(S2I_NAME)
#undef S2I_NAME
};

int plan_bf16(const s2i_conv_desc* d, BPlan* pl) {
  S2I_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->N > 0, "conv(bf16): non-positive extent");
  S2I_REQUIRE(d->Cc == 0, "conv(bf16): broadcast vectors are concatenated by the caller");
  S2I_REQUIRE(s2i_is_pow2(d->H) && s2i_is_pow2(d->W), "conv(bf16): spatial extents must be powers of two");
  S2I_REQUIRE(d->Cx >= 32 && (d->Cx % 32) == 0, "conv(bf16): input channels must be a multiple of 32 (Cx=%d)", d->Cx);
  S2I_REQUIRE((d->N % 8) == 0 && (d->ldy % 8) == 0 && d->ldy >= d->N, "conv(bf16): N and ldy must be multiples of 8");
  S2I_REQUIRE(d->act == S2I_ACT_NONE, "conv(bf16): no activation epilogue");
  pl->nphases = 1;
  switch (d->kind) {
    case S2I_CONV_K3S1: pl->kb = KB_K3S1; pl->T = 9; pl->NG = 1; pl->Ho = d->H; pl->Wo = d->W; break;
    case S2I_CONV_K4S2:
      S2I_REQUIRE(d->H >= 2 && d->W >= 2, "conv(bf16) k4s2: extent < 2");
      pl->kb = KB_K4S2; pl->T = 16; pl->NG = 2; pl->Ho = d->H / 2; pl->Wo = d->W / 2; break;
    case S2I_TCONV_K4S2: pl->kb = KB_TCONV; pl->T = 4; pl->NG = 1; pl->Ho = d->H; pl->Wo = d->W; pl->nphases = 4; break;
    default: S2I_FAIL("conv(bf16): unsupported kind %d", d->kind);
  }
  // Stage shape: all 9 taps of a 3x3 / the 4 taps of a transposed-conv phase per stage; the stride-2 4x4 conv with BN = 128
  // takes 4 taps x 32 channels (64-byte pieces of a pixel instead of 32-byte ones: measured -10 % time, the 32-byte pieces
  // left half of every 64-byte memory request unused).
  pl->BN = d->N > 64 ? 128 : (d->N > 32 ? 64 : 32);
  pl->TG = pl->kb == KB_K4S2 ? 8 : pl->T;
  const bool wide_ck = pl->BN == 128 && pl->kb == KB_K4S2;
  if (wide_ck) pl->TG = 4;
  pl->NG = pl->T / pl->TG;
  int ck = (pl->kb == KB_TCONV ? 4096 : 2048) / pl->BN;
  if (ck > (pl->kb == KB_K4S2 ? 32 : 64)) ck = pl->kb == KB_K4S2 ? 32 : 64;  // the stride-2 patch is 5 pixels per output pixel
  if (wide_ck) ck = 32;
  while (ck > 16 && (d->Cx % ck) != 0) ck >>= 1;
  if (pl->BN == 32 && ck < 32) ck = 32;
  S2I_REQUIRE((d->Cx % ck) == 0, "conv(bf16): %d channels do not split into chunks of %d", d->Cx, ck);
  pl->CK = ck;
  pl->Npad = s2i_cdiv(d->N, pl->BN) * pl->BN;
  // second-generation kernel (256-pixel tiles); tuning knob b16_v2 = 0 never, 1 (default) where it was measured faster, 2
  // wherever it can run (tests)
  const int v2mode = s2i_tune(S2I_TUNE_B16_V2, 1);
  pl->v2 = 0;
  TileGeom g;
  if (v2mode && pl->BN == 128) {
    g = tile_geom(pl->kb, pl->Ho, pl->Wo, 256);
    const int ck2 = pl->kb == KB_TCONV ? 64 : 32;
    bool ok = (d->Cx % ck2) == 0 && g.npix <= bf16_v2_max_pix(pl->kb);
    if (d->stats && d->groups > 1) ok = ok && pl->kb != KB_TCONV && (d->B % d->groups) == 0 && ((d->B / d->groups) % g.tb) == 0;
    const long long blocks2 = (long long)(pl->Wo / g.tw) * (pl->Ho / g.th) * s2i_cdiv(d->B, g.tb) * (pl->Npad / 128) * pl->nphases;
    if (v2mode == 1) ok = ok && blocks2 >= 224;
    if (ok) {
      pl->v2 = 1;
      pl->CK = ck = ck2;
      pl->TG = pl->kb == KB_K4S2 ? 4 : (pl->kb == KB_K3S1 ? 3 : 2);
      pl->NG = pl->T / pl->TG;
    }
  }
  if (!pl->v2) g = tile_geom(pl->kb, pl->Ho, pl->Wo, 128);
  pl->lgTW = s2i_ilog2(g.tw); pl->lgTH = s2i_ilog2(g.th); pl->lgTB = s2i_ilog2(g.tb);
  pl->tilesX = pl->Wo / g.tw; pl->tilesY = pl->Ho / g.th; pl->tilesB = s2i_cdiv(d->B, g.tb);
  pl->PH = g.PH; pl->PW = g.PW; pl->npix = g.npix;
  if (!pl->v2 && wide_ck && pl->npix > bf16_max_pix(KB_K4S2, 32) && ck == 32) { pl->CK = ck = 16; pl->TG = 8; pl->NG = 2; }   // 8 maps of 4x4 outputs per tile
  S2I_REQUIRE(pl->v2 || pl->npix <= bf16_max_pix(pl->kb, ck),
              "conv(bf16): patch of %d pixels exceeds the LDS plan", pl->npix);
  pl->gridM = pl->tilesX * pl->tilesY * pl->tilesB;
  pl->gridN = pl->Npad / pl->BN;
  pl->nchunk = d->Cx / ck;
  const long long M = (long long)d->B * pl->Ho * pl->Wo;
  pl->Mrows = M * pl->nphases;
  S2I_REQUIRE(pl->Mrows * d->ldy < (1ll << 31), "conv(bf16): output too large");
  if (d->stats && d->groups > 1) {
    S2I_REQUIRE(pl->kb != KB_TCONV && (d->B % d->groups) == 0 && ((d->B / d->groups) % g.tb) == 0,
                "conv(bf16): a tile of %d images straddles the %d BatchNorm groups of batch %d", g.tb, d->groups, d->B);
  }
  const long long blocks = (long long)pl->gridM * pl->gridN * pl->nphases;
  int splitk = 1;
  const int slots = pl->v2 ? 256 : 512;                 // resident blocks of the chip
  if (blocks < slots * 3 / 4 && pl->nchunk >= 4 && !d->nosplit) {
    splitk = (int)(slots / blocks);
    if (splitk > pl->nchunk / 2) splitk = pl->nchunk / 2;
    if (splitk > 32) splitk = 32;
    if (splitk < 1) splitk = 1;
  }
  if (!pl->v2 && pl->nchunk >= 4 && !d->nosplit && blocks < 4 * slots) {
    // 128-pixel kernel, a launch of a few blocks per CU: the time is set by the CU that holds one block more than the others
    // (the discriminators' 8 -> 4 px layer at batch 48: 288 blocks on 256 CUs ran like 512).  Price every split by the work
    // of the most loaded CU plus the slab traffic it adds, in us: a CU does ~3.9 TFLOP/s with two resident blocks (0.6 of its
    // clocked bf16 peak, profiles/r03_bf16_conv_layers.txt), ~0.75 of that with one; slabs move at ~4 TB/s; the reduction is a
    // launch of its own (~12 us in its chain).
    const double tile_us = 2.0 * 128.0 * pl->BN * (double)pl->T * d->Cx / 3.9e6;
    const double slab_us = (double)pl->Mrows * d->N * 8.0 / 4.0e6;
    double best = 1e300;
    int best_s = splitk;
    const int smax = pl->nchunk / 2 < 32 ? pl->nchunk / 2 : 32;
    for (int sc = 1; sc <= smax; ++sc) {
      const int cps = s2i_cdiv(pl->nchunk, sc), se = s2i_cdiv(pl->nchunk, cps);
      if (se != sc) continue;
      const long long nb = blocks * se;
      const double per_cu = (double)((nb + 255) / 256);
      double cost = per_cu / se * tile_us * (nb <= 256 ? 1.0 / 0.75 : 1.0) + 2.5 * per_cu;   // + a block's prologue / epilogue
      if (se > 1) cost += se * slab_us + 12.0;
      if (cost < best) { best = cost; best_s = se; }
    }
    splitk = best_s;
  }
  pl->cps = s2i_cdiv(pl->nchunk, splitk);
  pl->splitk = s2i_cdiv(pl->nchunk, pl->cps);
  pl->kernel = pick_kernel(*pl);
  pl->threads = pl->v2 ? 512 : 256;
  pl->gx = pl->v2 ? v2_grid_x(*pl) : pl->gridM;
  pl->smem = (int)smem_bytes(*pl);
  return 0;
}

extern "C" int s2i_conv_bf16_plan_query(const s2i_conv_desc* d, long long out[21]) {
  for (int i = 0; i < 21; ++i) out[i] = 0;
  BPlan pl;
  if (plan_bf16(d, &pl)) return 1;
  const long long v[21] = {pl.kernel, pl.v2 ? 256 : 128, pl.BN, pl.CK, pl.threads, pl.gx, pl.gridN, pl.nphases * pl.splitk,
                           1 << pl.lgTW, 1 << pl.lgTH, 1 << pl.lgTB, pl.gridM, pl.splitk, pl.cps, pl.nchunk,
                           stat_parts(pl, d->groups), pl.Npad, (long long)pl.nphases * pl.T * pl.Npad * d->Cx, pl.smem,
                           (long long)workspace_bytes(d, pl), pl.Mrows};
  for (int i = 0; i < 21; ++i) out[i] = v[i];
  return 0;
}

extern "C" int s2i_conv_forward_bf16(const s2i_conv_desc* d, const unsigned short* x, const unsigned short* w,
                                     const float* cls_bias, unsigned short* y, float* part, void* ws, size_t ws_bytes,
                                     void* stream) {
  BPlan pl;
  if (plan_bf16(d, &pl)) return 1;
  S2I_REQUIRE(x && w && y, "conv(bf16): null operand");
  S2I_REQUIRE(!cls_bias || (d->kind == S2I_CONV_K3S1 && pl.splitk == 1), "conv(bf16): class bias needs an unsplit 3x3 conv");
  S2I_REQUIRE(!d->stats || part, "conv(bf16): stats requested without a partial buffer");
  const size_t need = workspace_bytes(d, pl);
  S2I_REQUIRE(ws_bytes >= need && (need == 0 || ws), "conv(bf16): workspace too small (%zu < %zu)", ws_bytes, need);
  ConvBP p;
  p.x = x; p.w = w; p.cls_bias = cls_bias; p.y = y; p.part = part; p.slab = (float*)ws;
  p.B = d->B; p.H = d->H; p.W = d->W; p.C = d->Cx; p.Ho = pl.Ho; p.Wo = pl.Wo;
  p.N = d->N; p.Npad = pl.Npad; p.ldy = d->ldy;
  p.lgTW = pl.lgTW; p.lgTH = pl.lgTH; p.lgTB = pl.lgTB; p.tilesX = pl.tilesX; p.tilesY = pl.tilesY;
  p.ntiles = pl.gridM;
  p.PH = pl.PH; p.PW = pl.PW; p.npix = pl.npix;
  p.nchunk = pl.nchunk; p.splitk = pl.splitk; p.cps = pl.cps;
  p.stats = d->stats; p.nparts = pl.gridM * pl.nphases; p.Mrows = pl.Mrows;
  const unsigned long long xb = (unsigned long long)d->B * d->H * d->W * d->Cx * 2ull;
  const unsigned long long wb = (unsigned long long)pl.nphases * pl.T * pl.Npad * d->Cx * 2ull;
  S2I_REQUIRE(xb < 0x7ff00000ull && wb < 0x7ff00000ull, "conv(bf16): tensor exceeds the 2 GiB buffer-addressing window");
  p.x_bytes = (unsigned)xb; p.w_bytes = (unsigned)wb;
#ifdef S2I_DIAG
  p.dbg = s2i_tune(S2I_TUNE_B16_DBG, 0);
#else
  p.dbg = 0;
#endif
  dim3 grid(pl.gx, pl.gridN, pl.nphases * pl.splitk);
  const hipStream_t st = (hipStream_t)stream;
  if (pl.v2 ? launch_conv_bf16_v2(pl, p, grid, st) : launch_conv_bf16(pl, p, grid, st)) return 1;
  S2I_LAUNCH_CHECK("conv_bf16");
  return pl.splitk > 1 ? launch_splitk_reduce_bf16(d, pl, y, part, (const float*)ws, st) : 0;
}
