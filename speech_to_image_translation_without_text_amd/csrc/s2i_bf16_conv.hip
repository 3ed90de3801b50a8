// bf16 activation path: the 128-pixel convolution kernel (s2i_bf16.h says what the path is).
#include "s2i_bf16.h"

namespace {

// KIND: geometry; BN: output channels per block; CK: channels per LDS stage; waves 2x2 (BN >= 64) or 4x1 (BN = 32)
// TG: taps per LDS stage (T / TG stages per channel chunk); fragment reads are software-pipelined one k-step ahead with the
// order pinned (sched_barrier).  (Measured and removed: compiler-scheduled fragment reads, fewer taps per stage at three
// blocks per CU, weights by LDS-DMA into two buffers with one barrier per stage -- all within 5 %)
template <int KIND, int BN, int CK, int TG, int DBG = 0>
__global__ __launch_bounds__(256, 2) void conv_bf16_kernel(ConvBP p) {
  constexpr int T = KIND == KB_K3S1 ? 9 : (KIND == KB_K4S2 ? 16 : 4);
  constexpr int NG = T / TG;
  static_assert(NG * TG == T, "tap groups must tile the taps");
  constexpr int WAVES_N = BN >= 64 ? 2 : 1, WAVES_M = 4 / WAVES_N;
  constexpr int TM = 128 / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int SEGS = CK / 8;                      // 16-byte segments per LDS row
  constexpr int ROWB = CK * 2;
  constexpr int LGR = SEGS == 2 ? 3 : (SEGS == 4 ? 2 : 1);  // rows per 256-byte bank span = 16 / SEGS -> swizzle shift
  constexpr int KS = CK / 16;                       // k-steps per tap
  constexpr int BSEG = TG * BN * SEGS;              // 16-byte segments of one weight stage
  constexpr int NBL = (BSEG + 255) / 256;
  constexpr int MAXPIX = bf16_max_pix(KIND, CK);    // plan_bf16 checks the patch against this
  constexpr int NPL = (MAXPIX * SEGS + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [patch | weight stage], reused by the epilogue
  unsigned char* As = smem;
  unsigned char* Bs = smem + ((p.npix * ROWB + 255) & ~255);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l31 = lane & 31, lh = lane >> 5;
  // XCD-aware block order (round 3): the gridDim.y channel blocks and the gridDim.z phases / K splits of ONE pixel tile read
  // the same input patch and are its siblings
  int bx, sib;
  xcd_block_map(gridDim.x, gridDim.y * gridDim.z, bx, sib);
  const int by = sib % gridDim.y, bz = sib / gridDim.y;
  int phase = 0, split = bz;
  if (KIND == KB_TCONV) { phase = bz / p.splitk; split = bz - phase * p.splitk; }
  const int py = phase >> 1, px = phase & 1;
  const int n0 = by * BN;
  const int TW = 1 << p.lgTW, TH = 1 << p.lgTH;
  const int tix = bx & (p.tilesX - 1);
  const int tiy = (bx / p.tilesX) & (p.tilesY - 1);
  const int tib = bx / (p.tilesX * p.tilesY);
  const int b0 = tib << p.lgTB, oy0 = tiy << p.lgTH, ox0 = tix << p.lgTW;
  const int PW = p.PW, PH = p.PH;
  // input coordinate of patch pixel (0, 0)
  int iy0, ix0;
  if (KIND == KB_K3S1) { iy0 = oy0 - 1; ix0 = ox0 - 1; }
  else if (KIND == KB_K4S2) { iy0 = 2 * oy0 - 1; ix0 = 2 * ox0 - 1; }
  else { iy0 = oy0 - (py ? 0 : 1); ix0 = ox0 - (px ? 0 : 1); }

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);

  auto stamp = [&](int i) { bf16_stamp<DBG>(p, tid, i); };
  stamp(0);
  // ---- patch staging plan of this thread: global byte offset (chunk 0) and swizzled LDS offset per load ----
  int pgo[NPL], plo[NPL];
  const int nseg = p.npix * SEGS;
  const float inv_pw = 1.0f / (float)PW, inv_ph = 1.0f / (float)PH;
#pragma unroll
  for (int q = 0; q < NPL; ++q) {
    const int e = tid + q * 256;
    int go = S2I_OOB, lo = -1;
    if (e < nseg) {
      // pix < 1024: floor(pix / PW) = (int)((pix + 0.5) * (1 / PW)) exactly in fp32 (no integer-division sequences)
      const int pix = e / SEGS, seg = e & (SEGS - 1);
      const int rest = (int)(((float)pix + 0.5f) * inv_pw);
      const int xl = pix - rest * PW;
      const int tb = (int)(((float)rest + 0.5f) * inv_ph);
      const int yl = rest - tb * PH;
      const int b = b0 + tb, iy = iy0 + yl, ix = ix0 + xl;
      if (b < p.B && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) go = (((b * p.H + iy) * p.W + ix) * p.C + seg * 8) * 2;
      const int xs = KIND == KB_K4S2 ? (xl & 1) * (PW >> 1) + (xl >> 1) : xl;   // even / odd columns de-interleaved
      const int prow = (tb * PH + yl) * PW + xs;
      lo = prow * ROWB + ((seg ^ ((prow >> LGR) & (SEGS - 1))) << 4);
    }
    pgo[q] = go;
    plo[q] = lo;
  }
  // ---- A fragment rows of this lane: patch row of (tile row, tap (0,0)) ----
  int arow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int r = wm * TM * 32 + i * 32 + l31;
    const int tx = r & (TW - 1), ty = (r >> p.lgTW) & (TH - 1), tb = r >> (p.lgTW + p.lgTH);
    arow[i] = (tb * PH + (KIND == KB_K4S2 ? 2 * ty : ty)) * PW + tx;
  }
  // weight fragment rows of this lane inside one tap's [BN][CK] image (BN is a multiple of the swizzle period, so the
  // tap only adds tl * BN * ROWB)
  int boffs[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int brow = wn * TN * 32 + j * 32 + l31;
    boffs[j] = brow * ROWB + ((lh ^ ((brow >> LGR) & (SEGS - 1))) << 4);
  }
  // weight stage: segment e -> (tap, n, seg); global element offset inside the stage and swizzled LDS offset
  // (computed on the fly: BN and SEGS are powers of two)
  const int wstage = TG * p.Npad * CK;               // elements per (chunk, tap group)
  u32x4 ra[NPL], rb[NBL];
  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunk, c_begin + p.cps);
  const int s_begin = c_begin * NG, s_end = c_end * NG;

  auto fetch = [&](int st, bool with_a) {            // st = chunk * NG + group
    const int cc = st / NG, tg = st - cc * NG;
    if (with_a && !((DBG & 1) && st != s_begin)) {
      const int coff = cc * CK * 2;
#pragma unroll
      for (int q = 0; q < NPL; ++q) ra[q] = bload16(rx, pgo[q] == S2I_OOB ? S2I_OOB : pgo[q] + coff);
    }
    const int wbase = ((phase * p.nchunk + cc) * NG + tg) * wstage + n0 * CK;
    if ((DBG & 2) && st != s_begin) return;
    {
#pragma unroll
      for (int q = 0; q < NBL; ++q) {
        const int e = tid + q * 256;
        const int seg = e & (SEGS - 1), n = (e / SEGS) & (BN - 1), t = e / (SEGS * BN);
        rb[q] = bload16(rw, e < BSEG ? (wbase + (t * p.Npad + n) * CK + seg * 8) * 2 : S2I_OOB);
      }
    }
  };
  auto stage = [&](bool with_a) {
    if (with_a) {
#pragma unroll
      for (int q = 0; q < NPL; ++q)
        if (plo[q] >= 0) *reinterpret_cast<u32x4*>(As + plo[q]) = ra[q];
    }
    {
#pragma unroll
      for (int q = 0; q < NBL; ++q) {
        const int e = tid + q * 256;
        if (e < BSEG) {
          const int seg = e & (SEGS - 1), row = e / SEGS;  // row = t * BN + n
          *reinterpret_cast<u32x4*>(Bs + row * ROWB + ((seg ^ ((row >> LGR) & (SEGS - 1))) << 4)) = rb[q];
        }
      }
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  if (s_begin < s_end) fetch(s_begin, true);
  stamp(1);
  for (int st = s_begin; st < s_end; ++st) {
    const bool new_a = (st % NG) == 0;
    const int sb = 2 + 6 * min(st - s_begin, 7);
    stamp(sb);
    if (!((DBG & 4) && st != s_begin)) stage(new_a);
    stamp(sb + 1);
    __syncthreads();
    stamp(sb + 2);
    if (st + 1 < s_end) fetch(st + 1, ((st + 1) % NG) == 0);
    const int tg = st % NG;
    const unsigned char* Bcur = Bs;
    // LDS byte offsets of this lane's fragments, once per stage: the matrix loop below then spends no vector
    // instructions on addresses (row, swizzle and tap arithmetic per read had the address math competing with the MFMAs
    // for the SIMD's issue slots).  k-step ks of a tap is the ks = 0 offset XOR (ks << 5): the segment index is
    // (2 ks) ^ lh ^ swizzle(row).
    int aaddr[TM][TG];
#pragma unroll
    for (int tl = 0; tl < TG; ++tl) {
      const int t = tg * TG + tl;
      int toff;  // patch rows between tap (0,0) and tap t
      if (KIND == KB_K3S1) { toff = (t / 3) * PW + (t % 3); }
      else if (KIND == KB_K4S2) { const int dy = t >> 2, dx = t & 3; toff = dy * PW + (dx & 1) * (PW >> 1) + (dx >> 1); }
      else { const int ta = t >> 1, tb2 = t & 1; toff = (py ? ta : 1 - ta) * PW + (px ? tb2 : 1 - tb2); }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int prow = arow[i] + toff;
        aaddr[i][tl] = prow * ROWB + ((lh ^ ((prow >> LGR) & (SEGS - 1))) << 4);
      }
    }
    // fragments of k-step s+1 are read from LDS before the MFMAs of k-step s are issued (two named register sets,
    // order pinned): the LDS latency hides behind this wave's own MFMAs, and no more than two sets are ever live
    auto ldfr = [&](int stp, bf16x8 (&a)[TM], bf16x8 (&b)[TN]) {
      const int tl = stp / KS, ks = stp % KS;
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8*>(As + (aaddr[i][tl] ^ (ks << 5)));
#pragma unroll
      for (int j = 0; j < TN; ++j)
        b[j] = *reinterpret_cast<const bf16x8*>(Bcur + tl * BN * ROWB + (boffs[j] ^ (ks << 5)));
    };
    auto mma = [&](const bf16x8 (&a)[TM], const bf16x8 (&b)[TN]) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          if constexpr (!(DBG & 8)) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
          else asm volatile("" :: "v"(a[i]), "v"(b[j]));  // keeps the fragment reads alive
    };
    constexpr int NS = TG * KS;
    stamp(sb + 3);
    {
      bf16x8 a0[TM], b0[TN], a1[TM], b1[TN];
      ldfr(0, a0, b0);
#pragma unroll
      for (int s2 = 0; s2 < NS; s2 += 2) {
        if (s2 + 1 < NS) ldfr(s2 + 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (s2 + 2 < NS) ldfr(s2 + 2, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (s2 + 1 < NS) mma(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    stamp(sb + 4);
    __syncthreads();
    stamp(sb + 5);
  }

  // ---- epilogue ----
  const bool raw = p.splitk > 1;
  auto out_row = [&](int r, long long& row) { return tile_out_row<KIND>(p, b0, oy0, ox0, py, px, r, row); };
  if (p.cls_bias && !raw)
    add_class_bias<TM, TN>(p.cls_bias, p.N, p.Ho, p.Wo, acc, lane, wm, wn, n0,
                           [&](int r, int& b, int& oy, int& ox) { return tile_pixel(p, b0, oy0, ox0, r, b, oy, ox); });
  if (raw) {
    store_slab<TM, TN>(p.slab + (size_t)split * p.Mrows * p.N, p.N, acc, lane, wm, wn, n0, out_row);
    return;
  }
  // bf16 tile through LDS, rows leave as 16-byte row-contiguous stores: transpose_tile_bf16 (s2i_bf16.h) written out, see there
  constexpr int ERS = BN * 2 + 16;
  const bool odd = lane & 1;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float mine0 = acc[i][j][2 * q], mine1 = acc[i][j][2 * q + 1];
        const float give = odd ? mine0 : mine1;
        const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, give), 0xB1, 0xF, 0xF, true));
        const int reg = 2 * q + (odd ? 1 : 0);
        const int rr = acc_row(wm, TM, i, reg, lh);
        const int col = acc_col(wn, TN, j, l31 & ~1);
        const unsigned v = odd ? pack2(got, mine1) : pack2(mine0, got);
        *reinterpret_cast<unsigned*>(smem + rr * ERS + col * 2) = v;
      }
  __syncthreads();
  stamp(50);
  constexpr int SPR = BN / 8;                         // 16-byte segments per row
#pragma unroll
  for (int q = 0; q < 128 * SPR / 256; ++q) {
    const int e = tid + q * 256;
    const int rr = e / SPR, sg = e & (SPR - 1);
    long long row;
    const bool live = out_row(rr, row);
    const int n = n0 + sg * 8;
    if (live && n < p.N && !(DBG & 16))
      *reinterpret_cast<u32x4*>(p.y + row * p.ldy + n) = *reinterpret_cast<const u32x4*>(smem + rr * ERS + sg * 16);
  }
  stamp(51);
  // column sums of the fp32 accumulators over this block's valid rows (rows beyond the batch gathered zeros)
  if (p.stats)
    tile_col_stats<TM, TN, WAVES_M, BN>(p.part, p.nparts, p.N, reinterpret_cast<float*>(smem), acc, tid, lane, wm, wn, n0,
                                        phase * gridDim.x + bx);
  stamp(52);
  if constexpr ((DBG & 32) != 0) {
    if (tid == 0) {
      const size_t blk = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
      unsigned long long* o = reinterpret_cast<unsigned long long*>(p.slab) + blk * 64;
      o[60] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
      o[61] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // XCC_ID
      o[62] = __builtin_amdgcn_s_memrealtime();
    }
  }
}

template <int KIND, int BN, int CK, int TG>
int launch_one(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st) {
  static bool raised = false;
  if (bf16_raise_lds((const void*)conv_bf16_kernel<KIND, BN, CK, TG>, 96 * 1024, &raised)) return 1;
  hipLaunchKernelGGL((conv_bf16_kernel<KIND, BN, CK, TG>), grid, dim3(pl.threads), pl.smem, st, p);
  return 0;
}

#ifdef S2I_DIAG
#include "diag/s2i_bf16_conv_diag.inc"
#endif

}  // namespace

// the kernel the plan names (S2I_BF16_TILES of s2i_bf16.h, instantiated in its order), where its taps per stage are the planned ones
int launch_conv_bf16(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st) {
#ifdef S2I_DIAG   // libs2i_hip_diag.so only (make diag): ablation / in-kernel timeline instantiations of tools/conv16_*.py
  int rc = 0;
  if (diag_launch_conv_bf16(pl, p, grid, st, &rc)) return rc;
#endif
  switch (pl.kernel) {
#define S2I_CASE(K, bn, ck, tg)                                        \
  case B16_##K##_##bn##x##ck:                                          \
    if (pl.TG != tg) break;                                            \
    return launch_one<KB_##K, bn, ck, tg>(pl, p, grid, st);
    S2I_BF16_TILES(S2I_CASE)
#undef S2I_CASE
    default: break;
  }
  S2I_FAIL("conv(bf16): no kernel for kind %d BN=%d CK=%d TG=%d (the plan names %s)", pl.kb, pl.BN, pl.CK, pl.TG,
           pl.kernel < 0 ? "none" : b16_kernel_names[pl.kernel]);
}
