// fp32 and split-bf16 implicit-GEMM forward kernel templates (v_mfma_f32_32x32x2_f32, bit-exact f32 fma chain;
// v_mfma_f32_32x32x16_bf16 on bf16 planes) and their per-shape launch helpers.  Private to the forward matrix units
// s2i_conv_fwd_<BM>x<BN>.hip and s2i_conv_fwd_split.hip: each of them includes this header and compiles the instantiations
// of its own tile shapes, so every instantiation is compiled in exactly one unit.  Everything here stays in an unnamed
// namespace (the kernels' demangled names carry it).
// The gather formulation is described in s2i_igemm.h; the dispatcher is conv_forward_impl (s2i_conv.hip).
//
// Tile: 256 threads = 4 waves; block tile BM x BN x 32; each wave owns TM x TN MFMA tiles of 32x32.
// LDS holds A as [k][m] and B as [k][n] so a fragment read is 32 consecutive floats per half-wave
// (ds_read_b32, conflict-free).  Global->LDS staging goes through registers with the next chunk's
// loads in flight during the MFMA loop.
#pragma once
#include "s2i_igemm.h"

namespace {

// Row decode of the gather of igemm_fwd_kernel / igemm_fwd_split_kernel.  Thread (mrow, kq) stages channel quad kq of rows
// m0 + mrow + 32 i; per slot i: the byte offset of that quad in the row's base pixel (may be negative; only used when in
// bounds), the mask of taps that fall inside the tensor, and the byte offset of the quad in the row's image of cvec.
template <int ASLOTS>
__device__ __forceinline__ void gather_rows(const IgemmP& p, int m0, int mrow, int kq, int s, int pad, int kw, int py, int px,
                                            int (&aoff)[ASLOTS], unsigned (&amask)[ASLOTS], int (&acoff)[ASLOTS]) {
#pragma unroll
  for (int i = 0; i < ASLOTS; ++i) {
    const int m = m0 + mrow + 32 * i;
    unsigned mask = 0;
    int base = 0, coff = 0;
    if (m < p.M) {
      int b, oy, ox;
      row_pixel(p, m, b, oy, ox);
      const int by = p.kind == S2I_CONV_1D ? oy : oy * s - pad, bx = ox * s - pad;
      mask = tap_mask(p.kind, kw, by, bx, p.H, p.W, py, px);
      base = (((b * p.H + by) * p.W + bx) * p.Cx + kq * 4) * 4;
      coff = (b * p.Cc + kq * 4) * 4;
    }
    aoff[i] = base;
    amask[i] = mask;
    acoff[i] = coff;
  }
}

// CA32: gathered channel count (and the broadcast-vector part of it) is a multiple of 32, so a 32-deep K
// chunk lies inside ONE tap (and entirely in x or entirely in cvec): the tap decode is scalar work.
// Measured alternatives that lost (MI355X, 64->128 k4s2 on 24x128x128): two LDS stages with one barrier per
// chunk (2 blocks/CU: 79 vs 98 TFLOP/s), a start-up stagger of the blocks (no change).  Three resident blocks
// per CU with the plain two-barrier loop is the fastest structure found for v_mfma_f32_32x32x2_f32.
// INACT (CA32, no broadcast vector, forward weights only): see IgemmP::in_coef.  Padding taps stay zero AFTER the activation.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool WT, bool CA32, bool INACT = false>
__global__ __launch_bounds__(256, 3) void igemm_fwd_kernel(IgemmP p) {
  static_assert(!INACT || (CA32 && !WT), "apply-on-load: 32-channel chunks, forward weight layout");
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int LDA = BM + 1;
  constexpr int LDB = WT ? BN + 1 : BN;
  constexpr int ASLOTS = BM / 32;
  constexpr int BSLOTS = BN / 32;
  constexpr int BROWS_PER_PASS = 1024 / BN;
  // 96-row tiles are padded to the LDS footprint of a 128-row tile: exactly three blocks per CU either way, so that
  // 768 blocks are one round of the chip for both (plan_fwd counts rounds)
  constexpr int SMEM_FLOATS = 32 * LDA + 32 * LDB + 4;
  constexpr int SMEM_MIN = BM < 128 ? 32 * 129 + 32 * LDB + 4 : 0;
  __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS > SMEM_MIN ? SMEM_FLOATS : SMEM_MIN];
  float* As = smem + (WT ? 0 : 32 * LDB);  // keep the b128-written array 16-byte aligned
  float* Bs = smem + (WT ? 32 * LDA : 0);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  // XCD-aware block order (round 3): the column blocks, phases and K splits of ONE row tile are its siblings
  int bx, sib;
  xcd_block_map(gridDim.x, gridDim.y * gridDim.z, bx, sib);
  const int by = sib % gridDim.y, bz = sib / gridDim.y;
  int phase = 0, split = bz;
  if (p.kind == S2I_TCONV_K4S2) { phase = bz / p.splitk; split = bz - phase * p.splitk; }
  const int py = phase >> 1, px = phase & 1;
  const int m0 = bx * BM, n0 = by * BN;
  const int kq = tid & 7, mrow = tid >> 3;
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);

  // hardware-bounds-checked descriptors: an invalid element is fetched at S2I_OOB and reads as zero,
  // so the gather needs no exec-mask branches
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)p.cvec, 0, p.c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);

  int aoff[ASLOTS], acoff[ASLOTS];
  unsigned amask[ASLOTS];
  gather_rows<ASLOTS>(p, m0, mrow, kq, s, pad, kw, py, px, aoff, amask, acoff);
  // per-thread constant parts of the weight addresses
  const int bcol4 = tid % (BN / 4), brow = tid / (BN / 4);
  int wconst[BSLOTS];
#pragma unroll
  for (int j = 0; j < BSLOTS; ++j) {
    if (WT) {
      const int n = n0 + mrow + 32 * j;
      wconst[j] = n < p.N ? (n * p.ldw + kq * 4) * 4 : S2I_OOB;
    } else {
      const int n = n0 + bcol4 * 4;
      wconst[j] = n < p.ldw ? ((brow + j * BROWS_PER_PASS) * p.ldw + n) * 4 : S2I_OOB;
    }
  }

  f32x4 ra[ASLOTS], rb[BSLOTS];
  // apply-on-load state of the chunk held in ra: scale / shift of this thread's four channels and the chunk's tap
  f32x4 in_s = {1.f, 1.f, 1.f, 1.f}, in_t = {0.f, 0.f, 0.f, 0.f};
  int in_tap = 0;
  const float* in_cg = nullptr;
  if constexpr (INACT) in_cg = p.in_coef + (size_t)(m0 / p.in_rows_per_group) * 4 * p.Cx;   // a tile lies inside one group

  auto fetch = [&](int kc) {
    if (CA32) {
      // wave-uniform tap decode
      const int k0 = kc * 32;
      const int t = k0 / p.Ca;
      const int c0 = k0 - t * p.Ca;
      int dy, dx;
      tap_delta(p.kind, kw, t, py, px, dy, dx);
      const int tw = tap_weight(p.kind, p.flip, p.T, t, py, px);
      if constexpr (INACT) {
        in_tap = t;
        in_s = *reinterpret_cast<const f32x4*>(in_cg + 2 * p.Cx + c0 + kq * 4);
        in_t = *reinterpret_cast<const f32x4*>(in_cg + 3 * p.Cx + c0 + kq * 4);
      }
      if (c0 < p.Cc) {
#pragma unroll
        for (int i = 0; i < ASLOTS; ++i)
          ra[i] = bload4(rc, ((amask[i] >> t) & 1u) ? acoff[i] + c0 * 4 : S2I_OOB);
      } else {
        const int toff = ((dy * p.W + dx) * p.Cx + (c0 - p.Cc)) * 4;
#pragma unroll
        for (int i = 0; i < ASLOTS; ++i)
          ra[i] = bload4_any(rx, ((amask[i] >> t) & 1u) ? aoff[i] + toff : S2I_OOB, p.x16);
      }
      const int wbase = WT ? (tw * p.wR * p.ldw + c0) * 4 : (tw * p.wR + c0) * p.ldw * 4;
#pragma unroll
      for (int j = 0; j < BSLOTS; ++j) rb[j] = bload4(rw, wconst[j] == S2I_OOB ? S2I_OOB : wbase + wconst[j]);
    } else {
      const int k = kc * 32 + kq * 4;
      const bool kvalid = k < p.K;
      int t = 0, c = 0, tw = 0, toff = 0;
      if (kvalid) {
        t = k / p.Ca;
        c = k - t * p.Ca;
        int dy, dx;
        tap_delta(p.kind, kw, t, py, px, dy, dx);
        toff = ((dy * p.W + dx) * p.Cx + (c - kq * 4 - p.Cc)) * 4;
        tw = tap_weight(p.kind, p.flip, p.T, t, py, px);
      }
      const bool from_vec = c < p.Cc;
#pragma unroll
      for (int i = 0; i < ASLOTS; ++i) {
        const bool ok = kvalid && ((amask[i] >> t) & 1u);
        f32x4 vx = bload4_any(rx, (ok && !from_vec) ? aoff[i] + toff : S2I_OOB, p.x16);
        if (p.Cc > 0) vx += bload4(rc, (ok && from_vec) ? acoff[i] + (c - kq * 4) * 4 : S2I_OOB);
        ra[i] = vx;
      }
      if (WT) {
#pragma unroll
        for (int j = 0; j < BSLOTS; ++j)
          rb[j] = bload4(rw, (kvalid && wconst[j] != S2I_OOB) ? (tw * p.wR * p.ldw + c - kq * 4) * 4 + wconst[j] : S2I_OOB);
      } else {
#pragma unroll
        for (int q = 0; q < BSLOTS; ++q) {
          const int kb = kc * 32 + brow + q * BROWS_PER_PASS;
          int off = S2I_OOB;
          if (kb < p.K && wconst[q] != S2I_OOB) {
            const int tb = kb / p.Ca;
            const int cb = kb - tb * p.Ca;
            const int twb = tap_weight(p.kind, p.flip, p.T, tb, py, px);
            off = ((twb * p.wR + cb) * p.ldw + n0 + bcol4 * 4) * 4;
          }
          rb[q] = bload4(rw, off);
        }
      }
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  auto stage_store = [&](float* Asd, float* Bsd) {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = ra[i][j];
        if constexpr (INACT) {
          v = fmaf(v, in_s[j], in_t[j]);
          v = v > 0.f ? v : 0.2f * v;
          v = ((amask[i] >> in_tap) & 1u) ? v : 0.f;      // the padding is zero in the ACTIVATED tensor
        }
        Asd[(kq * 4 + j) * LDA + mrow + 32 * i] = v;
      }
    if (WT) {
#pragma unroll
      for (int i = 0; i < BSLOTS; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Bsd[(kq * 4 + j) * LDB + mrow + 32 * i] = rb[i][j];
    } else {
#pragma unroll
      for (int q = 0; q < BSLOTS; ++q)
        *reinterpret_cast<f32x4*>(Bsd + (brow + q * BROWS_PER_PASS) * LDB + bcol4 * 4) = rb[q];
    }
  };
  {
    if (c_begin < c_end) fetch(c_begin);
    for (int kc = c_begin; kc < c_end; ++kc) {
      stage_store(As, Bs);
      __syncthreads();
      if (kc + 1 < c_end) fetch(kc + 1);
      mma_chunk<TM, TN, LDA, LDB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
      __syncthreads();
    }
  }

  // ---- epilogue ----
  // This kernel keeps its own copy of the class bias, tile store and column sums that the other matrix kernels take from
  // s2i_tile.h: built on the shared pieces, its 3x3 forward launches ran 1 - 3.5 us (1.3 - 5 %) slower on the MI355X
  // (DESIGN.md section 4a).  A change to the shared epilogue pieces has to be repeated here.
  const int l31 = lane & 31, lh = lane >> 5;
  const bool tconv = p.kind == S2I_TCONV_K4S2;
  const bool raw = p.splitk > 1;
  if (p.cls_bias && !raw) {
    // contribution of a spatially constant operand (the broadcast c_code of model.py:277), pre-reduced per
    // border class: cls = 3 * (top | middle | bottom) + (left | middle | right)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= p.M) continue;
        const int b = m >> p.lgHoWo;
        const int rr = m & ((1 << p.lgHoWo) - 1);
        const int oy = rr >> p.lgWo, ox = rr & (p.Wo - 1);
        const int cls = 3 * (oy == 0 ? 0 : (oy == p.Ho - 1 ? 2 : 1)) + (ox == 0 ? 0 : (ox == p.Wo - 1 ? 2 : 1));
        const float* bp = p.cls_bias + ((size_t)b * 9 + cls) * p.N;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + wn * TN * 32 + j * 32 + l31;
          if (n < p.N) acc[i][j][r] += bp[n];
        }
      }
  }
  float* outp = raw ? p.slab + (size_t)split * p.Mrows * p.N : p.y;
  const int ldo = raw ? p.N : p.ldy;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ml = wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int m = m0 + ml;
      if (m >= p.M) continue;
      long long row = m;
      if (tconv) {
        const int b = m >> p.lgHoWo;
        const int rr = m & ((1 << p.lgHoWo) - 1);
        const int oy = rr >> p.lgWo, ox = rr & (p.Wo - 1);
        row = ((long long)b * (2 * p.Ho) + 2 * oy + py) * (2 * p.Wo) + 2 * ox + px;
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + l31;
        if (n < p.N) {
          float v = acc[i][j][r];
          if (!raw) {
            if (p.bias) v += p.bias[n];
            if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
            else if (p.act == S2I_ACT_TANH) v = tanhf(v);
            else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
          }
          if (!raw && p.y16) reinterpret_cast<unsigned short*>(outp)[row * ldo + n] = f2bf(v);
          else outp[row * ldo + n] = v;
        }
      }
    }
  }

  if (p.stats && !raw) {
    // column sums over this block's rows; rows >= M gathered zeros and contribute nothing
    float* red = smem;  // [2][WAVES_M][BN]
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float sv = 0.f, sq = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[i][j][r];
          sv += v;
          sq += v * v;
        }
      sv += __shfl_xor(sv, 32);
      sq += __shfl_xor(sq, 32);
      if (lh == 0) {
        const int col = wn * TN * 32 + j * 32 + l31;
        red[(0 * WAVES_M + wm) * BN + col] = sv;
        red[(1 * WAVES_M + wm) * BN + col] = sq;
      }
    }
    __syncthreads();
    if (tid < BN) {
      const int n = n0 + tid;
      if (n < p.N) {
        float sv = 0.f, sq = 0.f;
#pragma unroll
        for (int q = 0; q < WAVES_M; ++q) {
          sv += red[(0 * WAVES_M + q) * BN + tid];
          sq += red[(1 * WAVES_M + q) * BN + tid];
        }
        const int gm = phase * gridDim.x + bx;
        p.part[((size_t)0 * p.nparts + gm) * p.N + n] = sv;
        p.part[((size_t)1 * p.nparts + gm) * p.N + n] = sq;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Split-bf16 variant ("bf16xNP" math modes): every fp32 operand value v is written as the sum of NP bf16 numbers
// (v1 = bf16(v), v2 = bf16(v - v1), v3 = bf16(v - v1 - v2)) and the products a_i * b_j with i + j <= NP + 1 are
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16, which runs at 16x the rate of v_mfma_f32_32x32x2_f32.
//   NP = 2: 3 products, relative product error ~2^-16 (TF32, which the reference's cuDNN convolutions use by default on
//           NVIDIA hardware, is 2^-11);   NP = 3: 6 products, ~2^-23.
// Activations are split while they are staged into LDS (v_cvt_pk_bf16_f32 + two VALU ops per extra plane and pair);
// weights arrive pre-split in [plane][tap][n][k] order (s2i_split_packed_weight), so a B tile is a straight 16-byte copy.
// LDS: one [rows][32 k] bf16 image per plane and operand, 64-byte rows whose four 16-byte segments are XOR-swizzled
// with (row >> 2) & 3: a fragment is ONE ds_read_b128 per lane (row r = lane & 31, k = 8 * (lane >> 5) + j) and 16
// consecutive rows hit 16 distinct 4-bank groups; three planes of a 128x128 tile take 48 KB, so three blocks fit a CU.
// Gather, split-K, epilogue and statistics are those of igemm_fwd_kernel (CA32 case only).
template <int BM, int BN, int WAVES_M, int WAVES_N, int NP>
__global__ __launch_bounds__(256, 3) void igemm_fwd_split_kernel(IgemmP p) {
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int ROWB = 64;
  constexpr int APLANE = BM * ROWB, BPLANE = BN * ROWB;
  constexpr int ASLOTS = BM / 32;
  constexpr int BSEGS = NP * BN * 4;                 // 16-byte segments of the B tile
  constexpr int BLOADS = (BSEGS + 255) / 256;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NP * (APLANE + BPLANE)];
  unsigned char* As = smem;
  unsigned char* Bs = smem + NP * APLANE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  int phase = 0, split = blockIdx.z;
  if (p.kind == S2I_TCONV_K4S2) { phase = blockIdx.z / p.splitk; split = blockIdx.z - phase * p.splitk; }
  const int py = phase >> 1, px = phase & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kq = tid & 7, mrow = tid >> 3;
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc((void*)p.cvec, 0, p.c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wsp, 0, p.wsp_bytes, 0x00020000);

  int aoff[ASLOTS], acoff[ASLOTS];
  unsigned amask[ASLOTS];
  gather_rows<ASLOTS>(p, m0, mrow, kq, s, pad, kw, py, px, aoff, amask, acoff);
  int bconst[BLOADS], blds[BLOADS];
#pragma unroll
  for (int q = 0; q < BLOADS; ++q) {
    const int e = tid + q * 256;
    const int seg = e & 3, row = (e >> 2) % BN, pl = (e >> 2) / BN;
    const int n = n0 + row;
    bconst[q] = (e < BSEGS && n < p.N) ? (pl * p.wsp_plane + n * p.wsp_kp) * 2 + seg * 16 : S2I_OOB;
    blds[q] = e < BSEGS ? pl * BPLANE + row * ROWB + ((seg ^ ((row >> 2) & 3)) << 4) : -1;
  }

  f32x4 ra[ASLOTS];
  u32x4 rb[BLOADS];
  auto fetch = [&](int kc) {
    const int k0 = kc * 32;
    const int t = k0 / p.Ca;
    const int c0 = k0 - t * p.Ca;
    int dy, dx;
    tap_delta(p.kind, kw, t, py, px, dy, dx);
    const int tw = tap_weight(p.kind, p.flip, p.T, t, py, px);
    if (c0 < p.Cc) {
#pragma unroll
      for (int i = 0; i < ASLOTS; ++i)
        ra[i] = bload4(rc, ((amask[i] >> t) & 1u) ? acoff[i] + c0 * 4 : S2I_OOB);
    } else {
      const int toff = ((dy * p.W + dx) * p.Cx + (c0 - p.Cc)) * 4;
#pragma unroll
      for (int i = 0; i < ASLOTS; ++i)
        ra[i] = bload4(rx, ((amask[i] >> t) & 1u) ? aoff[i] + toff : S2I_OOB);
    }
    const int wbase = (tw * p.wsp_np * p.wsp_kp + c0) * 2;
#pragma unroll
    for (int q = 0; q < BLOADS; ++q)
      rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rw, bconst[q] == S2I_OOB ? S2I_OOB : wbase + bconst[q], 0, 0);
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  const int l31 = lane & 31, lh = lane >> 5;
  const int fsw = ((lh ^ ((l31 >> 2) & 3)) << 4);  // swizzled segment of k-step 0; k-step 1 is fsw ^ 32
  const unsigned char* ap = As + (wm * TM * 32 + l31) * ROWB;
  const unsigned char* bp = Bs + (wn * TN * 32 + l31) * ROWB;

  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  if (c_begin < c_end) fetch(c_begin);
  for (int kc = c_begin; kc < c_end; ++kc) {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i) {
      u32x2 sp[NP];
      split4<NP>(ra[i], sp);
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        *reinterpret_cast<u32x2*>(As + pl * APLANE + (mrow + 32 * i) * ROWB + ((((kq >> 1) ^ (mrow >> 2)) & 3) << 4) +
                                  (kq & 1) * 8) = sp[pl];
    }
#pragma unroll
    for (int q = 0; q < BLOADS; ++q)
      if (blds[q] >= 0) *reinterpret_cast<u32x4*>(Bs + blds[q]) = rb[q];
    // the MFMA phase of a split chunk is short (0.7 us): put the next chunk's loads in flight before the barrier wait
    if (kc + 1 < c_end) fetch(kc + 1);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int so = fsw ^ (ks << 5);
      bf16x8 a[NP][TM];
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int i = 0; i < TM; ++i)
          a[pl][i] = *reinterpret_cast<const bf16x8*>(ap + pl * APLANE + i * 32 * ROWB + so);
      // b plane by plane, the smallest cross terms first: (a1 b3) | (a2 b2, a1 b2) | (a3 b1, a2 b1, a1 b1)
#pragma unroll
      for (int pb = NP - 1; pb >= 0; --pb) {
        bf16x8 b[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
          b[j] = *reinterpret_cast<const bf16x8*>(bp + pb * BPLANE + j * 32 * ROWB + so);
#pragma unroll
        for (int pa = NP - 1 - pb; pa >= 0; --pa)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: class bias, the split-K slab or y, BatchNorm column sums (rows >= M gathered zeros) ----
  const bool raw = p.splitk > 1;
  if (p.cls_bias && !raw)
    add_class_bias<TM, TN>(p.cls_bias, p.N, p.Ho, p.Wo, acc, lane, wm, wn, n0,
                           [&](int r, int& b, int& oy, int& ox) {
                             if (m0 + r >= p.M) return false;
                             row_pixel(p, m0 + r, b, oy, ox);
                             return true;
                           });
  store_tile<TM, TN>(raw ? p.slab + (size_t)split * p.Mrows * p.N : p.y, raw ? p.N : p.ldy, p.N, raw, p.bias, p.act, 0 /* y is always fp32 here */, acc, lane,
                     wm, wn, n0, [&](int r, long long& row) {
                       const int m = m0 + r;
                       if (m >= p.M) return false;
                       row = m;
                       if (p.kind == S2I_TCONV_K4S2) {   // the rows of a phase interleave into the 2Ho x 2Wo map
                         int b, oy, ox;
                         row_pixel(p, m, b, oy, ox);
                         row = ((long long)b * (2 * p.Ho) + 2 * oy + py) * (2 * p.Wo) + 2 * ox + px;
                       }
                       return true;
                     });
  if (p.stats && !raw) tile_col_stats<TM, TN, WAVES_M, BN>(p.part, p.nparts, p.N, reinterpret_cast<float*>(smem), acc, tid, lane, wm, wn, n0, phase * gridDim.x + blockIdx.x);
}

// the instantiations of one tile shape: the fp32 kernel by its WT / CA32 flags, apply-on-load (plan_fwd admits it for
// !wt && ca32 only), or the split-bf16 kernel by its plane count
template <int BM, int BN, int WM, int WN>
void launch_fwd(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  if (pl.kernel >= FWD_F32IN_128x128) {
    hipLaunchKernelGGL((igemm_fwd_kernel<BM, BN, WM, WN, false, true, true>), grid, dim3(256), 0, st, p);
  } else if (pl.wt) {
    if (pl.ca32) hipLaunchKernelGGL((igemm_fwd_kernel<BM, BN, WM, WN, true, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((igemm_fwd_kernel<BM, BN, WM, WN, true, false>), grid, dim3(256), 0, st, p);
  } else {
    if (pl.ca32) hipLaunchKernelGGL((igemm_fwd_kernel<BM, BN, WM, WN, false, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((igemm_fwd_kernel<BM, BN, WM, WN, false, false>), grid, dim3(256), 0, st, p);
  }
}

template <int BM, int BN, int WM, int WN>
void launch_split(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  if (pl.planes == 1) hipLaunchKernelGGL((igemm_fwd_split_kernel<BM, BN, WM, WN, 1>), grid, dim3(256), 0, st, p);
  else if (pl.planes == 2) hipLaunchKernelGGL((igemm_fwd_split_kernel<BM, BN, WM, WN, 2>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((igemm_fwd_split_kernel<BM, BN, WM, WN, 3>), grid, dim3(256), 0, st, p);
}

}  // namespace
