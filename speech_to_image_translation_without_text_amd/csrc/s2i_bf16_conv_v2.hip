// bf16 activation path: the 256-pixel persistent convolution kernel (s2i_bf16.h says what the path is).
#include "s2i_bf16.h"

namespace {

// ---- second-generation kernel: 256 output pixels x 128 channels per tile, 8 waves, persistent over tiles ---------------
// What the in-kernel timelines showed (tools/conv16_timeline.py).  128-pixel kernel: the matrix loop
// was a quarter of a block's lifetime; the rest was the bulk issue of the next stage's loads (the CU's vector-memory path
// stalls the issuing wave), waiting for loads issued one matrix phase earlier, two barriers per stage, and a prologue /
// epilogue per 33 MFLOP.  First 256-pixel version (everything prefetched, one barrier per stage, one block per CU): the
// steady-state stage ran the matrix pipe at 82 %, but 37 % of a block's lifetime was its prologue -- every CU of the chip
// starts a tile at the same moment and asks HBM for its first patch chunk at once (36 MB per round: 7 us at 5 TB/s), then
// leaves HBM idle while it computes.  This kernel therefore
//   * keeps the 256-pixel tile (the 256 KB weight stream of a tile is amortised over twice the pixels),
//   * issues every global load BETWEEN matrix instructions, a few per k-step: weights two stages ahead (two register
//     sets that alternate), the next patch chunk a whole chunk ahead; the LDS stores of a later stage are interleaved too,
//   * keeps two weight stages (and two patch chunks where the patch is small: 3x3, transposed phases) in LDS: ONE barrier
//     per stage,
//   * is PERSISTENT where the launcher gives it fewer blocks than tiles (stride-2 4x4): the first patch chunk and the
//     first weight stages of the NEXT tile are prefetched during the last chunk of the current one exactly like any
//     other next chunk, so HBM is asked for data all the time instead of in bursts, and a tile boundary costs the
//     epilogue plus one patch store.
// The schedule is compile-time: the stages of a channel chunk are unrolled (tap group tg, weight register set parity P),
// so every vmcnt the compiler derives is exact; loads that must move nothing go through a descriptor of zero records.
// Geometry, LDS images, swizzle, fragment maps and the epilogue are those of conv_bf16_kernel.  A patch segment is
// described by its byte offset from the patch's pixel (0,0) plus four halo flags (left / right column, top / bottom
// row) that are tested against the tile's position, so moving to the next tile costs no per-lane index arithmetic.
template <int V> struct IC { static constexpr int value = V; };

// PWC != 0: the patch is PWC pixels wide (compile time) and its LDS rows are padded to 80 bytes instead of XOR-swizzled: a
// fragment address is then lane base + constant, i.e. the matrix loop spends NO vector instruction on addresses (with
// one k-step of read-ahead, a dependent address chain in front of every read starved the matrix pipe: +40 % per stage).
// 80 = 5 x 16 bytes and 5 is odd, so the 16 lanes of a ds_read_b128 group (consecutive patch rows) hit 16 distinct
// 16-byte bank groups.
template <int KIND, int CK, int TG, bool PDB, int DBG = 0, int PWC = 0>
__global__ __launch_bounds__(512, 1) void conv_bf16_v2_kernel(ConvBP p) {
  constexpr int BN = 128, BM = 256, NT = 512;
  constexpr int T = KIND == KB_K3S1 ? 9 : (KIND == KB_K4S2 ? 16 : 4);
  constexpr int NG = T / TG;
  static_assert(NG * TG == T && NG >= 2, "tap groups must tile the taps, at least two stages per channel chunk");
  constexpr int WAVES_N = 2, WAVES_M = 4, TM = 2, TN = 2;
  constexpr int SEGS = CK / 8, ROWB = CK * 2;
  constexpr bool PADA = PWC != 0;
  constexpr int AROWB = PADA ? ROWB + 16 : ROWB;              // bytes per patch row in LDS
  static_assert(!PADA || (KIND == KB_K4S2 && CK == 32), "padded patch rows: stride-2 4x4 with 32-channel chunks");
  constexpr int LGR = SEGS == 2 ? 3 : (SEGS == 4 ? 2 : 1);
  constexpr int KS = CK / 16, NS = TG * KS, HS = NS / 2;      // k-steps per stage; the first HS issue loads, the rest store
  static_assert((NS % 2) == 0, "even number of k-steps per stage");
  constexpr int BSEG = TG * BN * SEGS, NBL = BSEG / NT, B_BYTES = TG * BN * ROWB;
  static_assert(BSEG % NT == 0, "a weight stage is a whole number of 16-byte segments per thread");
  constexpr int MAXPIX = bf16_v2_max_pix(KIND);             // plan_bf16 checks the patch against this
  constexpr int NPL = (MAXPIX * SEGS + NT - 1) / NT;
  static_assert(NPL <= 16, "halo flags of a thread's patch segments fit two registers");
  constexpr int ALS = NG - 1;                                 // stages of a chunk that issue the next chunk's patch loads
  constexpr int AG = ALS * HS;                                // ... over this many k-step slots
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [patch (x2) | weight stage x2 | 1 KB sink]
  const int A_BYTES = (p.npix * AROWB + 255) & ~255;
  unsigned char* As = smem;
  unsigned char* Bs = smem + (PDB ? 2 : 1) * A_BYTES;
  const int sink = (PDB ? 2 : 1) * A_BYTES + 2 * B_BYTES;     // lanes without a patch segment store here (no exec masks)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l31 = lane & 31, lh = lane >> 5;
  int phase = 0, split = blockIdx.z;
  if (KIND == KB_TCONV) { phase = blockIdx.z / p.splitk; split = blockIdx.z - phase * p.splitk; }
  const int py = phase >> 1, px = phase & 1;
  const int n0 = blockIdx.y * BN;
  const int TW = 1 << p.lgTW, TH = 1 << p.lgTH;
  const int PW = PADA ? PWC : p.PW, PH = p.PH;
  const int ntiles = p.ntiles;

  auto stamp = [&](int i) { bf16_stamp<DBG>(p, tid, i); };
  stamp(0);

  // position of a tile: first image / output row / output column, byte offset of the patch's pixel (0,0) in x (may be
  // negative: the halo of the first image), and which of the patch's halo sides lie outside the image
  struct TilePos { int b0, oy0, ox0, base; unsigned edge; };
  auto tile_pos = [&](int tile) -> TilePos {
    TilePos t;
    const int tix = tile & (p.tilesX - 1);
    const int tiy = (tile / p.tilesX) & (p.tilesY - 1);
    const int tib = tile / (p.tilesX * p.tilesY);
    t.b0 = tib << p.lgTB; t.oy0 = tiy << p.lgTH; t.ox0 = tix << p.lgTW;
    int iy0, ix0;
    if (KIND == KB_K3S1) { iy0 = t.oy0 - 1; ix0 = t.ox0 - 1; }
    else if (KIND == KB_K4S2) { iy0 = 2 * t.oy0 - 1; ix0 = 2 * t.ox0 - 1; }
    else { iy0 = t.oy0 - (py ? 0 : 1); ix0 = t.ox0 - (px ? 0 : 1); }
    t.base = (((t.b0 * p.H + iy0) * p.W + ix0) * p.C) * 2;
    t.edge = (t.ox0 == 0 ? 1u : 0u) | (t.ox0 + TW == p.Wo ? 2u : 0u) | (t.oy0 == 0 ? 4u : 0u) | (t.oy0 + TH == p.Ho ? 8u : 0u);
    return t;
  };

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);

  // patch plan of this thread: byte offset of segment q from the patch's pixel (0,0), its halo flags (4 bits per q) and
  // its swizzled LDS offset.  The LDS offsets are kept in registers only where the matrix loop needs them (two patch
  // buffers); the single-buffer form recomputes them at the chunk boundary.
  const int nseg = p.npix * SEGS;
  const float inv_pw = 1.0f / (float)PW, inv_ph = 1.0f / (float)PH;
  int zv = 0;   // zero the optimiser cannot see through (re-made per chunk): keeps per-lane index arithmetic that is invariant
                // across chunks and tiles INSIDE the loops instead of hoisted into registers the matrix loop needs
  auto patch_slot = [&](int q, int& rel, unsigned& flags, int& lo) {
    const int e = tid + zv + q * NT;
    rel = S2I_OOB;
    flags = 0;
    lo = -1;
    if (e < nseg) {
      const int pix = e / SEGS, seg = e & (SEGS - 1);
      const int rest = (int)(((float)pix + 0.5f) * inv_pw);
      const int xl = pix - rest * PW;
      const int tb = (int)(((float)rest + 0.5f) * inv_ph);
      const int yl = rest - tb * PH;
      rel = (((tb * p.H + yl) * p.W + xl) * p.C + seg * 8) * 2;
      // halo sides: 3x3 and stride-2 4x4 (pad 1) have all four; a transposed-conv phase has the top row / left column
      // when its parity is 0 and the bottom row / right column when it is 1
      const bool hl = KIND == KB_TCONV ? px == 0 : true, hr = KIND == KB_TCONV ? px == 1 : true;
      const bool ht = KIND == KB_TCONV ? py == 0 : true, hb = KIND == KB_TCONV ? py == 1 : true;
      flags = (hl && xl == 0 ? 1u : 0u) | (hr && xl == PW - 1 ? 2u : 0u) | (ht && yl == 0 ? 4u : 0u) | (hb && yl == PH - 1 ? 8u : 0u);
      const int xs = KIND == KB_K4S2 ? (xl & 1) * (PW >> 1) + (xl >> 1) : xl;
      const int prow = (tb * PH + yl) * PW + xs;
      lo = PADA ? prow * AROWB + seg * 16 : prow * ROWB + ((seg ^ ((prow >> LGR) & (SEGS - 1))) << 4);
    }
  };
  // (the single-buffer form -- the stride-2 4x4, whose patch is the largest -- recomputes the LDS offsets at the chunk
  // boundary instead of keeping them: its matrix loop has no register to spare, and a spilled value comes back through a
  // scratch load whose vmcnt wait drains the whole prefetch queue)
  int rel[NPL], plo[PDB ? NPL : 1];
  unsigned fw0 = 0, fw1 = 0;
#pragma unroll
  for (int q = 0; q < NPL; ++q) {
    int r, lo;
    unsigned f;
    patch_slot(q, r, f, lo);
    rel[q] = r;
    if (q < 8) fw0 |= f << (4 * q);
    else fw1 |= f << (4 * (q - 8));
    if (PDB) plo[q] = lo;
  }
  auto plo_of = [&](int q) -> int {
    if (PDB) return plo[q];
    int r, lo;
    unsigned f;
    patch_slot(q, r, f, lo);
    return lo;
  };
  // vector offset of patch segment q for a tile at (base, edge): out of range where the segment is halo outside the image
  auto avoff = [&](int q, int base, unsigned edge) -> int {
    const unsigned hit = (q < 8 ? fw0 : fw1) & (edge << (4 * (q & 7)));
    return hit ? S2I_OOB : base + rel[q];
  };
  auto adst = [&](unsigned char* base, int lo) -> u32x4* {
    return reinterpret_cast<u32x4*>(lo >= 0 ? base + lo : smem + sink + lane * 16);
  };
  // A fragment rows of this lane (tile row -> patch row of tap (0,0)); the same for every tile
  int arow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int r = wm * TM * 32 + i * 32 + l31;
    const int tx = r & (TW - 1), ty = (r >> p.lgTW) & (TH - 1), tb = r >> (p.lgTW + p.lgTH);
    arow[i] = (tb * PH + (KIND == KB_K4S2 ? 2 * ty : ty)) * PW + tx;
    if (PADA) arow[i] = arow[i] * AROWB + lh * 16;           // padded rows: the lane's byte base, taps and k-steps add constants
  }
  int boffs[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int brow = wn * TN * 32 + j * 32 + l31;
    boffs[j] = brow * ROWB + ((lh ^ ((brow >> LGR) & (SEGS - 1))) << 4);
  }
  // weight stage segments of this thread: segment q is row (tid / SEGS) + q * (NT / SEGS) of the stage's [TG * BN][CK]
  // image, so both its global offset and its swizzled LDS offset are the q = 0 values plus a constant
  static_assert(BN % (NT / SEGS) == 0 && ((NT / SEGS) >> LGR) % SEGS == 0, "weight rows per load step keep the swizzle");
  const int bseg = tid & (SEGS - 1), brow0 = tid / SEGS;
  const int bgo0 = (brow0 * CK + bseg * 8) * 2;
  const int blo0 = brow0 * ROWB + ((bseg ^ ((brow0 >> LGR) & (SEGS - 1))) << 4);
  auto bgo_s = [&](int q) -> int {   // uniform part of the global byte offset of segment q
    const int row = q * (NT / SEGS), n = row & (BN - 1), t = row / BN;
    return ((t * p.Npad + n) * CK) * 2;
  };
  constexpr int BLO_STEP = (NT / SEGS) * ROWB;
  const int wstage = TG * p.Npad * CK;                        // elements per (chunk, tap group)
  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunk, c_begin + p.cps);
  const int ncl = c_end - c_begin;                            // chunks of this block's K range
  auto wbyte = [&](int cc, int tg) -> int { return (((phase * p.nchunk + cc) * NG + tg) * wstage + n0 * CK) * 2; };
  // loads: the per-lane offset goes in the vector offset (out of range where nothing is to be loaded), the uniform part in
  // the scalar offset
  auto bload16s = [&](__amdgpu_buffer_rsrc_t r, int voff, int soff) -> u32x4 {
    return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  };

  u32x4 ra[NPL], rb[2][NBL];
  f32x16 acc[TM][TN];
  zero_acc(acc);
  stamp(1);

  int tile = blockIdx.x;
  if (tile >= ntiles || ncl <= 0) return;
  TilePos cur = tile_pos(tile);
  // ---- prologue: patch chunk c_begin of the first tile, weight stages 0 (-> LDS) and 1 (stays in its register set) ----
  {
    const int coff = c_begin * CK * 2;
#pragma unroll
    for (int q = 0; q < NPL; ++q) ra[q] = bload16s(rx, avoff(q, cur.base, cur.edge), coff);
    const int w0 = wbyte(c_begin, 0), w1 = wbyte(c_begin, 1);
#pragma unroll
    for (int q = 0; q < NBL; ++q) rb[0][q] = bload16s(rw, bgo0, w0 + bgo_s(q));
#pragma unroll
    for (int q = 0; q < NBL; ++q) rb[1][q] = bload16s(rw, bgo0, w1 + bgo_s(q));
    stamp(2);
#pragma unroll
    for (int q = 0; q < NPL; ++q) *adst(As, plo_of(q)) = ra[q];
#pragma unroll
    for (int q = 0; q < NBL; ++q) *reinterpret_cast<u32x4*>(Bs + blo0 + q * BLO_STEP) = rb[0][q];
  }
  __syncthreads();
  stamp(3);

  // ---- epilogue of one tile: accumulators -> y (bf16, through an LDS transpose) or fp32 slabs, BatchNorm column sums ----
  auto epilogue = [&](const TilePos& tp, int tile_id) {
    // the lane / wave coordinates are re-derived from a value the optimiser cannot see through, so that none of the
    // epilogue's (tile-invariant) address arithmetic is hoisted above the tile loop into registers the matrix loop needs
    int z = 0;
    asm volatile("" : "+v"(z));
    const int tid = (int)threadIdx.x + z, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int l31 = lane & 31, lh = lane >> 5;
    const bool raw = p.splitk > 1;
    auto out_row = [&](int r, long long& row) { return tile_out_row<KIND>(p, tp.b0, tp.oy0, tp.ox0, py, px, r, row); };
    if (p.cls_bias && !raw)
      add_class_bias<TM, TN>(p.cls_bias, p.N, p.Ho, p.Wo, acc, lane, wm, wn, n0,
                             [&](int r, int& b, int& oy, int& ox) { return tile_pixel(p, tp.b0, tp.oy0, tp.ox0, r, b, oy, ox); });
    if (raw) {
      store_slab<TM, TN>(p.slab + (size_t)split * p.Mrows * p.N, p.N, acc, lane, wm, wn, n0, out_row);
      return;
    }
    transpose_tile_bf16<TM, TN, BN>(smem, acc, lane, wm, wn, l31, lh);
    constexpr int ERS = BN * 2 + 16;
    stamp(50);
    constexpr int SPR = BN / 8;
#pragma unroll
    for (int q = 0; q < BM * SPR / NT; ++q) {
      const int e = tid + q * NT;
      const int rr = e / SPR, sg = e & (SPR - 1);
      long long row;
      const bool live = out_row(rr, row);
      const int n = n0 + sg * 8;
      if (live && n < p.N)
        *reinterpret_cast<u32x4*>(p.y + row * p.ldy + n) = *reinterpret_cast<const u32x4*>(smem + rr * ERS + sg * 16);
    }
    stamp(51);
    if (p.stats)
      tile_col_stats<TM, TN, WAVES_M, BN>(p.part, p.nparts, p.N, reinterpret_cast<float*>(smem), acc, tid, lane, wm, wn, n0,
                                          phase * ntiles + tile_id);
    stamp(52);
  };

  // one channel chunk = NG stages, unrolled.  CP: parity of the chunk's first stage among the block's stages.
  // ci: index of the chunk inside [c_begin, c_end).  The chunk AFTER the last one of a tile is the first chunk of the
  // block's next tile (patch and weights alike); after the last tile nothing follows and the loads move nothing.
  int apar = 0;                                               // patch buffer in use (two-buffer form)
  auto run_chunk = [&](auto cp_tag, int ci, const TilePos& nxt, bool more_tiles) {
    constexpr int CP = decltype(cp_tag)::value;
    if (!PDB) asm volatile("" : "+v"(zv));
    const int cc = c_begin + ci;
    const bool last_chunk = ci + 1 == ncl;
    const bool nextc = !last_chunk || more_tiles;             // a patch chunk follows this one
    const int coff_next = (last_chunk ? c_begin : cc + 1) * CK * 2;
    const int nbase = last_chunk ? nxt.base : cur.base;
    const unsigned nedge = last_chunk ? nxt.edge : cur.edge;
    const unsigned char* Acur = As + apar * A_BYTES;
    unsigned char* Anext = As + (apar ^ 1) * A_BYTES;
    const __amdgpu_buffer_rsrc_t rxn = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, nextc ? p.x_bytes : 0u, 0x00020000);
#pragma unroll
    for (int tg = 0; tg < NG; ++tg) {
      const int P = (CP + tg) & 1;                             // constant after unrolling
      const unsigned char* Bcur = Bs + P * B_BYTES;
      unsigned char* Bnext = Bs + (P ^ 1) * B_BYTES;
      // the stage two ahead: (chunk, tap group), wrapping into the next tile
      const int tg2 = (tg + 2) % NG;
      int ci2 = ci + (tg + 2) / NG;
      bool have2 = true;
      if (ci2 >= ncl) { ci2 -= ncl; have2 = more_tiles; }
      const int w2 = wbyte(c_begin + ci2, tg2);
      const __amdgpu_buffer_rsrc_t rw2 = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, have2 ? p.w_bytes : 0u, 0x00020000);
      // LDS byte offset of this lane's A fragment rows for one tap (k-step 0; k-step ks is that XOR (ks << 5))
      int aad0[TM], aad1[TM];
      auto tap_addr = [&](int tl, int (&aad)[TM]) {
        const int t = tg * TG + tl;
        int toff;
        if (KIND == KB_K3S1) { toff = (t / 3) * PW + (t % 3); }
        else if (KIND == KB_K4S2) { const int dy = t >> 2, dx = t & 3; toff = dy * PW + (dx & 1) * (PW >> 1) + (dx >> 1); }
        else { const int ta = t >> 1, tb2 = t & 1; toff = (py ? ta : 1 - ta) * PW + (px ? tb2 : 1 - tb2); }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int prow = arow[i] + zv + toff;
          aad[i] = prow * ROWB + ((lh ^ ((prow >> LGR) & (SEGS - 1))) << 4);
        }
      };
      // k-step stp reads tap stp / KS; consecutive k-steps alternate between the two address sets only when a tap is a
      // single k-step (never: KS >= 2), so one set per fragment register set suffices
      auto ldfr = [&](int stp, bf16x8 (&a)[TM], bf16x8 (&b)[TN], int (&aad)[TM]) {
        const int tl = stp / KS, ks = stp % KS;
        if constexpr (PADA) {
          const int t = tg * TG + tl, dy = t >> 2, dx = t & 3;
          const int cst = (dy * PWC + (dx & 1) * (PWC >> 1) + (dx >> 1)) * AROWB + ks * 32;   // constant after unrolling
#pragma unroll
          for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8*>(Acur + arow[i] + cst);
        } else {
          if (ks < 2) tap_addr(tl, aad);            // the first use of this tap by this register set
#pragma unroll
          for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8*>(Acur + (aad[i] ^ (ks << 5)));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
          b[j] = *reinterpret_cast<const bf16x8*>(Bcur + tl * BN * ROWB + (boffs[j] ^ (ks << 5)));
      };
      auto mma = [&](const bf16x8 (&a)[TM], const bf16x8 (&b)[TN]) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      };
      // memory work of k-step slot k of this stage
      auto side = [&](int k) {
        if (k < HS) {
          // weights of stage + 2 into the set this stage's weights came from
#pragma unroll
          for (int q = 0; q < NBL; ++q)
            if (q * HS / NBL == k) rb[P][q] = bload16s(rw2, bgo0, w2 + bgo_s(q));
          if (tg < ALS) {
            const int g = tg * HS + k;
#pragma unroll
            for (int q = 0; q < NPL; ++q)
              if (q * AG / NPL == g) ra[q] = bload16s(rxn, avoff(q, nbase, nedge), coff_next);
          }
        } else {
          const int k2 = k - HS;
          // weights of stage + 1 (loaded during the previous stage) into the other LDS stage
#pragma unroll
          for (int q = 0; q < NBL; ++q)
            if (q * HS / NBL == k2) *reinterpret_cast<u32x4*>(Bnext + blo0 + q * BLO_STEP) = rb[P ^ 1][q];
          if (PDB && tg == NG - 1) {
#pragma unroll
            for (int q = 0; q < NPL; ++q)
              if (q * HS / NPL == k2) *adst(Anext, plo_of(q)) = ra[q];
          }
        }
      };
      bf16x8 a0[TM], b0[TN], a1[TM], b1[TN];
      ldfr(0, a0, b0, aad0);
#pragma unroll
      for (int s2 = 0; s2 < NS; s2 += 2) {
        ldfr(s2 + 1, a1, b1, aad1);
        side(s2);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (s2 + 2 < NS) ldfr(s2 + 2, a0, b0, aad0);
        side(s2 + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr ((DBG & 32) != 0) stamp(4 + 2 * min(ci * NG + tg, 22));
      __syncthreads();
      if constexpr ((DBG & 32) != 0) stamp(5 + 2 * min(ci * NG + tg, 22));
    }
    if (PDB) apar ^= 1;
  };

  auto chunk_boundary = [&](int ci) {
    if (!PDB && ci + 1 < ncl) {
      // single patch buffer: every wave is past its last read of this chunk
#pragma unroll
      for (int q = 0; q < NPL; ++q) *adst(As, plo_of(q)) = ra[q];
      __syncthreads();
    }
  };
  for (;;) {
    const int ntile = tile + (int)gridDim.x;
    const bool more_tiles = !PDB && ntile < ntiles;           // the two-patch-buffer forms are launched one block per tile
    const TilePos nxt = tile_pos(more_tiles ? ntile : tile);
    if constexpr ((NG & 1) == 0) {
      for (int ci = 0; ci < ncl; ++ci) {
        run_chunk(IC<0>{}, ci, nxt, more_tiles);
        chunk_boundary(ci);
      }
    } else {
      // odd number of stages per chunk: the weight register sets swap roles from one chunk to the next
      static_assert((NG & 1) == 0 || PDB, "the persistent form needs an even number of stages per tile");
      for (int ci = 0; ci < ncl; ci += 2) {
        run_chunk(IC<0>{}, ci, nxt, more_tiles);
        chunk_boundary(ci);
        if (ci + 1 < ncl) {
          run_chunk(IC<1>{}, ci + 1, nxt, more_tiles);
          chunk_boundary(ci + 1);
        }
      }
    }
    // every wave is past its last LDS read of this tile: the patch region is free for the epilogue's transpose.  The next
    // tile's first patch chunk is still in registers and its first weight stages sit behind the patch region.
    epilogue(cur, tile);
    if (!more_tiles) break;
    zero_acc(acc);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NPL; ++q) *adst(As, plo_of(q)) = ra[q];
    __syncthreads();
    tile = ntile;
    cur = nxt;
  }
}

template <int KIND, int CK, int TG, bool PDB, int PWC>
int launch_v2(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st) {
  S2I_REQUIRE(pl.smem <= 160 * 1024, "conv(bf16): %s needs %d bytes of LDS", b16_kernel_names[pl.kernel], pl.smem);
  static bool raised = false;
  if (bf16_raise_lds((const void*)conv_bf16_v2_kernel<KIND, CK, TG, PDB, 0, PWC>, 160 * 1024, &raised)) return 1;
  hipLaunchKernelGGL((conv_bf16_v2_kernel<KIND, CK, TG, PDB, 0, PWC>), grid, dim3(pl.threads), pl.smem, st, p);
  return 0;
}

#ifdef S2I_DIAG
#include "diag/s2i_bf16_conv_v2_diag.inc"
#endif

}  // namespace

// the kernel the plan names.  S2I_BF16_V2_TILES (s2i_bf16.h) lists the two-buffer forms first: the order of the cases is the
// order of the instantiations in the code object
int launch_conv_bf16_v2(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st) {
#ifdef S2I_DIAG   // libs2i_hip_diag.so only (make diag): the in-kernel timeline instantiations of tools/conv16_timeline.py
  int rc = 0;
  if (diag_launch_conv_bf16_v2(pl, p, grid, st, &rc)) return rc;
#endif
  switch (pl.kernel) {
#define S2I_CASE(id, K, ck, tg, pdb, pwc) \
  case B16_##id: return launch_v2<KB_##K, ck, tg, pdb, pwc>(pl, p, grid, st);
    S2I_BF16_V2_TILES(S2I_CASE)
#undef S2I_CASE
    default: break;
  }
  S2I_FAIL("conv(bf16): kernel %d is not a 256-pixel kernel", (int)pl.kernel);
}
