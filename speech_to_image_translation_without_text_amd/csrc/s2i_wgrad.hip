// Weight gradients of the implicit-GEMM convolutions: the fp32, split-bf16 and bf16 matrix kernels, the row-segment and
// <= 4 channel kernels, the slab sums and the OIHW finish, their dispatcher and the s2i_conv_wgrad* entry points.  What to
// launch is decided by plan_wgrad (s2i_wgrad_plan.hip).
#include "s2i_igemm.h"

namespace {

// ------------------------------------------------------------------------------------------------
// weight gradient: slab[split][krow][n] = sum_{pixels in split} A(pixel, krow) * g[pixel][n]
struct WgradP {
  const float* __restrict__ a;
  const float* __restrict__ cvec;
  const float* __restrict__ g;
  float* __restrict__ slab;
  int B, H, W, Ca, Cc, Cin;
  int Ho, Wo, lgWo, lgHoWo;
  int M, N, ldg, K, T, kind;
  int cps, nchunks;
  int a16, g16;  // a / g hold bf16 instead of fp32
  unsigned a_bytes, c_bytes, g_bytes;
  // apply-on-load (AACT instantiation): `a` holds the RAW output of the producing convolution, a_coef its (groups, 4, Ca)
  // BatchNorm coefficient table; the gather computes LeakyReLU(scale * a + shift), padding taps staying zero
  const float* __restrict__ a_coef;
  int a_groups, a_ipg;   // BatchNorm groups of the producer, images per group
};

// (tap, channel) of gathered column kcol: fixed for a thread's whole pixel loop; false beyond K
__device__ __forceinline__ bool wgrad_col(const WgradP& p, int kcol, int kw, int& c, int& dy, int& dx) {
  c = 0;
  dy = 0;
  dx = 0;
  if (kcol >= p.K) return false;
  const int t = kcol / p.Cin;
  c = kcol - t * p.Cin;
  dy = t / kw;
  dx = t - dy * kw;
  return true;
}

// the block's tile -> the slab [K][N] of its pixel-range split; tile row -> slab row k0 + row = (tap, cin)
template <int TM, int TN>
__device__ __forceinline__ void store_wgrad_slab(const WgradP& p, int split, int k0, int n0, const f32x16 (&acc)[TM][TN], int lane,
                                                 int wm, int wn) {
  store_slab<TM, TN>(p.slab + (size_t)split * p.K * p.N, p.N, acc, lane, wm, wn, n0,
                     [&](int r, long long& row) { row = k0 + r; return k0 + r < p.K; });
}

// Never called.  Every kernel of this unit passes geom() the constant 1 x 1 geometry; when a unit has no other caller, hipcc
// folds those constants into geom() before it inlines it and the three matrix kernels come out with one to five more scalar
// instructions in their prologue than they had while the forward kernels, which pass run-time values, shared their unit.
// This device function is such a caller: with it the kernels compile to the instructions they had before the split
// (tools/compare_code_objects.py).  It is no kernel and costs a few bytes of code object.
__device__ __attribute__((used, noinline)) void geom_runtime_caller(int kind, int s1d, int pad1d, int kw1d, int* out) {
  geom(kind, s1d, pad1d, kw1d, out[0], out[1], out[2]);
}

// (HIP's second launch bound is waves per SIMD: 3 = three 256-thread blocks per CU, 4 = two 512-thread blocks or one of 1024)
template <int BM, int BN, int WAVES_M, int WAVES_N, bool AACT = false>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, (WAVES_M * WAVES_N > 4 ? 4 : 3)) void igemm_wgrad_kernel(WgradP p) {
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int LDA = BM, LDB = BN;
  constexpr int NT = 64 * WAVES_M * WAVES_N;  // 256, or 192 for the 96-row tiles (K = 9 * 32)
  constexpr int AROWS = NT * 4 / BM, BROWS = NT * 4 / BN;  // pixel rows of the 32-deep chunk staged per pass
  static_assert(AROWS * BM == NT * 4 && BROWS * BN == NT * 4, "a pass must cover whole rows");
  constexpr int APASS = (32 + AROWS - 1) / AROWS, BPASS = (32 + BROWS - 1) / BROWS;
  constexpr bool APRED = (32 % AROWS) != 0, BPRED = (32 % BROWS) != 0;  // last pass partly beyond the chunk
  __shared__ __attribute__((aligned(16))) float smem[32 * LDA + 32 * LDB];
  float* As = smem;
  float* Bs = smem + 32 * LDA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  // XCD-aware block order: the (k, n) tiles of ONE pixel-range split read the same pixels of both operands and are siblings
  int split, tile_;
  xcd_block_map(gridDim.z, gridDim.x * gridDim.y, split, tile_);
  const int k0 = (tile_ % gridDim.x) * BM, n0 = (tile_ / gridDim.x) * BN;
  int s, pad, kw;
  geom(p.kind, 1, 0, 1, s, pad, kw);

  const int acol4 = tid % (BM / 4), arow = tid / (BM / 4);
  const int bcol4 = tid % (BN / 4), brow = tid / (BN / 4);
  int c, dy, dx;
  const bool kvalid = wgrad_col(p, k0 + acol4 * 4, kw, c, dy, dx);   // this thread's 4 gathered columns
  const bool from_vec = c < p.Cc;
  const int nb = n0 + bcol4 * 4;
  const bool nvalid = nb < p.N;

  const __amdgpu_buffer_rsrc_t ra_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rc_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.cvec, 0, p.c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.g_bytes, 0x00020000);
  const int acolb = (c - p.Cc) * 4;            // byte offset of this thread's 4 channels inside a pixel of a
  const int ccolb = c * 4;                     // ... inside a row of cvec
  const int gcolb = nvalid ? nb * 4 : S2I_OOB;
  f32x4 ra[APASS], rb[BPASS];
  // apply-on-load: this thread's four channels are the same for the whole pixel loop, so their scale / shift (per producer
  // group: at most three, the stacked real / wrong / fake passes) sit in registers; per pass, which group the pixel's image
  // belongs to (2 bits) and whether the tap is inside the image (1 bit)
  f32x4 gs[3], gt[3];
  unsigned apass = 0;
  if constexpr (AACT) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int gg = g < p.a_groups ? g : 0;
      gs[g] = kvalid ? *reinterpret_cast<const f32x4*>(p.a_coef + ((size_t)gg * 4 + 2) * p.Ca + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      gt[g] = kvalid ? *reinterpret_cast<const f32x4*>(p.a_coef + ((size_t)gg * 4 + 3) * p.Ca + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  auto fetch = [&](int pc) {
    if constexpr (AACT) apass = 0;
#pragma unroll
    for (int q = 0; q < APASS; ++q) {
      const int m = pc * 32 + arow + q * AROWS;
      if (APRED && arow + q * AROWS >= 32) continue;
      int b, oy, ox;
      row_pixel(p, m, b, oy, ox);
      const int iy = oy * s - pad + dy, ix = ox * s - pad + dx;
      const bool ok = kvalid && m < p.M && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      if constexpr (AACT) {
        const unsigned grp = (unsigned)(b >= p.a_ipg) + (unsigned)(b >= 2 * p.a_ipg);
        apass |= ((ok ? 4u : 0u) | grp) << (3 * q);
      }
      if (from_vec) ra[q] = bload4(rc_rs, ok ? b * p.Cc * 4 + ccolb : S2I_OOB);
      else ra[q] = bload4_any(ra_rs, ok ? ((b * p.H + iy) * p.W + ix) * p.Ca * 4 + acolb : S2I_OOB, p.a16);
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      const int m = pc * 32 + brow + q * BROWS;
      if (BPRED && brow + q * BROWS >= 32) continue;
      rb[q] = bload4_any(rg_rs, (m < p.M && nvalid) ? m * p.ldg * 4 + gcolb : S2I_OOB, p.g16);
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  if (c_begin < c_end) fetch(c_begin);
  for (int pc = c_begin; pc < c_end; ++pc) {
#pragma unroll
    for (int q = 0; q < APASS; ++q)
      if (!APRED || arow + q * AROWS < 32) {
        f32x4 v = ra[q];
        if constexpr (AACT) {
          const unsigned bits = (apass >> (3 * q)) & 7u;
          const unsigned grp = bits & 3u;
          const f32x4 sc = grp == 0 ? gs[0] : (grp == 1 ? gs[1] : gs[2]);
          const f32x4 sh = grp == 0 ? gt[0] : (grp == 1 ? gt[1] : gt[2]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float z = fmaf(v[j], sc[j], sh[j]);
            z = z > 0.f ? z : 0.2f * z;
            v[j] = (bits & 4u) ? z : 0.f;
          }
        }
        *reinterpret_cast<f32x4*>(As + (arow + q * AROWS) * LDA + acol4 * 4) = v;
      }
#pragma unroll
    for (int q = 0; q < BPASS; ++q)
      if (!BPRED || brow + q * BROWS < 32) *reinterpret_cast<f32x4*>(Bs + (brow + q * BROWS) * LDB + bcol4 * 4) = rb[q];
    __syncthreads();
    if (pc + 1 < c_end) fetch(pc + 1);
    mma_chunk<TM, TN, LDA, LDB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
    __syncthreads();
  }

  store_wgrad_slab<TM, TN>(p, split, k0, n0, acc, lane, wm, wn);
}

// Split-bf16 weight gradient (see igemm_fwd_split_kernel).  The reduction index of this GEMM is the pixel, and both
// operands arrive pixel-major (NHWC), so the LDS images stay [pixel][row] -- a staged float4 becomes one 8-byte write per
// plane -- and the MFMA fragments (8 consecutive PIXELS of one row per lane) are fetched with the transposing read
// ds_read_b64_tr_b16: per 16-lane group it takes a 4-pixel x 16-row block and hands lane i column i.  16-byte chunks
// of a pixel row are XOR-swizzled with ((pixel & 3) << 2) | ((pixel >> 2) & 3) (cdna_hip_programming.md T10, image (b)).
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ s16x4 lds_tr_read(const unsigned char* ptr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(ptr));
}

// Transposed-read addressing of one operand ([pixel][row] image, ROWB bytes per pixel) for wave coordinate w and its T
// MFMA tiles: 16-lane group g = lane >> 4 -> (h = g >> 1, 16-row block g & 1); ad[i][f] is the byte offset inside a plane
// and a 16-pixel k-step of the 4-pixel half fragment f of tile i.
template <int T, int ROWB>
__device__ __forceinline__ void wgrad_tr_addr(int lane, int w, int (&ad)[T][2]) {
  constexpr int MASK = ROWB / 16 - 1;
  const int gi = lane & 15, gq = gi >> 2, gp = gi & 3;
  const int gh = lane >> 5, gcb = (lane >> 4) & 1;
  const int sw0 = (gq << 2) | (2 * gh);              // swizzle of pixel rows 8h + q (+ 16 ks); rows + 4: sw0 | 1
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int prow = 8 * gh + 4 * f + gq;
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const int ch = ((w * T + i) * 32 + 16 * gcb) / 8 + (gp >> 1);
      ad[i][f] = prow * ROWB + 16 * ((ch ^ (sw0 | f)) & MASK) + 8 * (gp & 1);
    }
  }
}

// one MFMA fragment (8 consecutive pixels of this lane's row) = two transposed 4-pixel reads
__device__ __forceinline__ bf16x8 lds_tr_frag(const unsigned char* kstep, const int (&ad)[2]) {
  const s16x4 lo = lds_tr_read(kstep + ad[0]);
  const s16x4 hi = lds_tr_read(kstep + ad[1]);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int BM, int BN, int WAVES_M, int WAVES_N, int NP>
__global__ __launch_bounds__(256, 3) void igemm_wgrad_split_kernel(WgradP p) {
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int AROWB = BM * 2, BROWB = BN * 2;
  constexpr int APLANE = 32 * AROWB, BPLANE = 32 * BROWB;
  constexpr int AMASK = BM / 8 - 1, BMASK = BN / 8 - 1;
  constexpr int APASS = BM / 32, BPASS = BN / 32;
  constexpr int AROWS = 1024 / BM, BROWS = 1024 / BN;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NP * (APLANE + BPLANE)];
  unsigned char* As = smem;
  unsigned char* Bs = smem + NP * APLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int k0 = blockIdx.x * BM, n0 = blockIdx.y * BN, split = blockIdx.z;
  int s, pad, kw;
  geom(p.kind, 1, 0, 1, s, pad, kw);

  const int acol4 = tid % (BM / 4), arow = tid / (BM / 4);
  const int bcol4 = tid % (BN / 4), brow = tid / (BN / 4);
  int c, dy, dx;
  const bool kvalid = wgrad_col(p, k0 + acol4 * 4, kw, c, dy, dx);
  const bool from_vec = c < p.Cc;
  const int nb = n0 + bcol4 * 4;
  const bool nvalid = nb < p.N;
  const __amdgpu_buffer_rsrc_t ra_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rc_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.cvec, 0, p.c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.g_bytes, 0x00020000);
  const int acolb = (c - p.Cc) * 4;
  const int ccolb = c * 4;
  const int gcolb = nvalid ? nb * 4 : S2I_OOB;
  f32x4 ra[APASS], rb[BPASS];
  auto fetch = [&](int pc) {
#pragma unroll
    for (int q = 0; q < APASS; ++q) {
      const int m = pc * 32 + arow + q * AROWS;
      int b, oy, ox;
      row_pixel(p, m, b, oy, ox);
      const int iy = oy * s - pad + dy, ix = ox * s - pad + dx;
      const bool ok = kvalid && m < p.M && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      if (from_vec) ra[q] = bload4(rc_rs, ok ? b * p.Cc * 4 + ccolb : S2I_OOB);
      else ra[q] = bload4(ra_rs, ok ? ((b * p.H + iy) * p.W + ix) * p.Ca * 4 + acolb : S2I_OOB);
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      const int m = pc * 32 + brow + q * BROWS;
      rb[q] = bload4(rg_rs, (m < p.M && nvalid) ? m * p.ldg * 4 + gcolb : S2I_OOB);
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  int aad[TM][2], bad[TN][2];
  wgrad_tr_addr<TM, AROWB>(lane, wm, aad);
  wgrad_tr_addr<TN, BROWB>(lane, wn, bad);

  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  if (c_begin < c_end) fetch(c_begin);
  for (int pc = c_begin; pc < c_end; ++pc) {
#pragma unroll
    for (int q = 0; q < APASS; ++q) {
      const int row = arow + q * AROWS;
      const int sw = ((row & 3) << 2) | ((row >> 2) & 3);
      u32x2 sp[NP];
      split4<NP>(ra[q], sp);
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        *reinterpret_cast<u32x2*>(As + pl * APLANE + row * AROWB + 16 * (((acol4 >> 1) ^ sw) & AMASK) + 8 * (acol4 & 1)) = sp[pl];
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      const int row = brow + q * BROWS;
      const int sw = ((row & 3) << 2) | ((row >> 2) & 3);
      u32x2 sp[NP];
      split4<NP>(rb[q], sp);
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        *reinterpret_cast<u32x2*>(Bs + pl * BPLANE + row * BROWB + 16 * (((bcol4 >> 1) ^ sw) & BMASK) + 8 * (bcol4 & 1)) = sp[pl];
    }
    if (pc + 1 < c_end) fetch(pc + 1);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[NP][TM];
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int i = 0; i < TM; ++i)
          a[pl][i] = lds_tr_frag(As + pl * APLANE + ks * 16 * AROWB, aad[i]);
#pragma unroll
      for (int pb = NP - 1; pb >= 0; --pb) {
        bf16x8 b[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = lds_tr_frag(Bs + pb * BPLANE + ks * 16 * BROWB, bad[j]);
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

  store_wgrad_slab<TM, TN>(p, split, k0, n0, acc, lane, wm, wn);
}

// Weight gradient with BOTH operands stored as bf16 (bf16 activation mode): the structure of igemm_wgrad_split_kernel
// with one plane, but the staged values are already bf16, so a 16-byte load (8 channels of one pixel) is copied to
// LDS as it is, and a stage is 64 pixels deep (4 k-steps, 16 MFMAs per wave between two barriers instead of 8).
// A32: the gathered operand is the fp32 NHWC4 image of the first discriminator conv (4x4 stride 2): 8 consecutive K columns
// are two horizontally adjacent taps x 4 channels = 32 contiguous bytes, converted to bf16 while they are staged.
// 256 x 128 tiles (8 waves, two blocks per CU; round 3): a tile of BM x BN moves (BM + BN) * 2 bytes per pixel from L2 into LDS
// for 2 * BM * BN FLOP -- 64 FLOP/B at 128 x 128, which at the ~70 GB/s a CU takes from L2 (MI355X_MICROARCH.md, gather into
// LDS) caps the chip near 0.65 PFLOP/s, where the 128 x 128 form sat (profiles/r03_roofline_bf16_wgrad_b48); 85 FLOP/B here.
// 256 x 256 tiles on 1024-thread blocks (one per CU) where N allows: 128 FLOP/B, 0.89 PFLOP/s on D_NET256's deep layers against
// 0.80 (256 x 128) and 0.70 (128 x 128); two LDS stages with one barrier per stage measured the same and were removed.
template <int BM, int BN, int WAVES_M, int WAVES_N, bool A32 = false>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, (WAVES_M * WAVES_N > 4 ? 4 : 3)) void igemm_wgrad_b16_kernel(WgradP p) {
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int PC = 64;                               // pixels per stage
  constexpr int AROWB = BM * 2, BROWB = BN * 2;
  constexpr int AMASK = BM / 8 - 1, BMASK = BN / 8 - 1;
  constexpr int ATPR = BM / 8, BTPR = BN / 8;          // threads per pixel row
  constexpr int AROWS = NT / ATPR, BROWS = NT / BTPR;  // pixel rows per pass
  static_assert(AROWS * ATPR == NT && BROWS * BTPR == NT && PC % AROWS == 0, "a pass covers whole pixel rows");
  constexpr int APASS = PC / AROWS, BPASS = (PC + BROWS - 1) / BROWS;
  constexpr int STAGE_BYTES = PC * (AROWB + BROWB);
  __shared__ __attribute__((aligned(16))) unsigned char smem[STAGE_BYTES];
  unsigned char* As = smem;
  unsigned char* Bs = smem + PC * AROWB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  // XCD-aware block order: the (k, n) tiles of ONE pixel-range split read the same pixels of both operands and are siblings
  int split, tile_;
  xcd_block_map(gridDim.z, gridDim.x * gridDim.y, split, tile_);
  const int k0 = (tile_ % gridDim.x) * BM, n0 = (tile_ / gridDim.x) * BN;
  int s, pad, kw;
  geom(p.kind, 1, 0, 1, s, pad, kw);
  const int acol8 = tid % ATPR, arow = tid / ATPR;
  const int bcol8 = tid % BTPR, brow = tid / BTPR;
  int c, dy, dx;
  const bool kvalid = wgrad_col(p, k0 + acol8 * 8, kw, c, dy, dx);
  const int nb = n0 + bcol8 * 8;
  const bool nvalid = nb < p.N;
  const __amdgpu_buffer_rsrc_t ra_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.g_bytes, 0x00020000);
  u32x4 ra[APASS], rb[BPASS];
  auto fetch = [&](int pc) {
#pragma unroll
    for (int q = 0; q < APASS; ++q) {
      const int m = pc * PC + arow + q * AROWS;
      int b, oy, ox;
      row_pixel(p, m, b, oy, ox);
      const int iy = oy * s - pad + dy, ix = ox * s - pad + dx;
      if constexpr (A32) {
        const bool rowok = kvalid && m < p.M && iy >= 0 && iy < p.H;
        const int o0 = ((b * p.H + iy) * p.W + ix) * 16;      // byte offset of pixel (iy, ix): 4 fp32 channels
        const f32x4 v0 = bload4(ra_rs, (rowok && ix >= 0 && ix < p.W) ? o0 : S2I_OOB);
        const f32x4 v1 = bload4(ra_rs, (rowok && ix + 1 >= 0 && ix + 1 < p.W) ? o0 + 16 : S2I_OOB);
        ra[q] = u32x4{(unsigned)f2bf(v0[0]) | ((unsigned)f2bf(v0[1]) << 16), (unsigned)f2bf(v0[2]) | ((unsigned)f2bf(v0[3]) << 16),
                      (unsigned)f2bf(v1[0]) | ((unsigned)f2bf(v1[1]) << 16), (unsigned)f2bf(v1[2]) | ((unsigned)f2bf(v1[3]) << 16)};
      } else {
        const bool ok = kvalid && m < p.M && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        ra[q] = __builtin_amdgcn_raw_buffer_load_b128(ra_rs, ok ? (((b * p.H + iy) * p.W + ix) * p.Ca + c) * 2 : S2I_OOB, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      const int row = brow + q * BROWS;
      const int m = pc * PC + row;
      rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rg_rs, (row < PC && m < p.M && nvalid) ? (m * p.ldg + nb) * 2 : S2I_OOB, 0, 0);
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  int aad[TM][2], bad[TN][2];
  wgrad_tr_addr<TM, AROWB>(lane, wm, aad);
  wgrad_tr_addr<TN, BROWB>(lane, wn, bad);

  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  auto stage_store = [&](unsigned char* A_, unsigned char* B_) {
#pragma unroll
    for (int q = 0; q < APASS; ++q) {
      const int row = arow + q * AROWS;
      const int sw = ((row & 3) << 2) | ((row >> 2) & 3);
      *reinterpret_cast<u32x4*>(A_ + row * AROWB + 16 * ((acol8 ^ sw) & AMASK)) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      const int row = brow + q * BROWS;
      const int sw = ((row & 3) << 2) | ((row >> 2) & 3);
      if (row < PC) *reinterpret_cast<u32x4*>(B_ + row * BROWB + 16 * ((bcol8 ^ sw) & BMASK)) = rb[q];
    }
  };
  auto stage_mma = [&](const unsigned char* A_, const unsigned char* B_) {
#pragma unroll
    for (int ks = 0; ks < PC / 16; ++ks) {
      bf16x8 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = lds_tr_frag(A_ + ks * 16 * AROWB, aad[i]);
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = lds_tr_frag(B_ + ks * 16 * BROWB, bad[j]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };
  if (c_begin < c_end) fetch(c_begin);
  for (int pc = c_begin; pc < c_end; ++pc) {
    stage_store(As, Bs);
    __syncthreads();
    if (pc + 1 < c_end) fetch(pc + 1);
    stage_mma(As, Bs);
    __syncthreads();
  }

  store_wgrad_slab<TM, TN>(p, split, k0, n0, acc, lane, wm, wn);
}

// Weight gradient of a 3x3 stride-1 convolution over a wide map with few channels (the generator at 64x64 and
// 128x128, Cin = 64 / 32).  The generic kernel above stages an im2col tile per chunk, i.e. it pulls every input pixel
// through the vector-memory path once per tap; with K x N this small that path, not the matrix cores, is the limit
// (57-78 TFLOP/s).  Here a block owns ONE kernel row dy and a chunk is 32 consecutive pixels of one image row: the
// block stages the 34-pixel input row segment (iy = y + dy - 1, halo of one pixel each side) ONCE and the three
// horizontal taps read their MFMA fragments from it at pixel offsets 0/1/2 -- a third of the loads, no wasted rows
// (block tile = (3 * CIN) x BN).  Slab rows are (tap, cin) as above, so the slab sum / OIHW finish are shared.
template <int CIN, int BN, int WAVES_M, int WAVES_N, int DYS>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, 3) void wgrad_k3_rows_kernel(WgradP p) {
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int BM = 3 * CIN * DYS, RT = BM / 32;  // DYS = 3: the block owns all three kernel rows (Cin = 32)
  constexpr int TM = RT / WAVES_M, TN = BN / (32 * WAVES_N);
  static_assert(TM * WAVES_M == RT && TN * WAVES_N * 32 == BN, "tile split");
  constexpr int LDH = CIN, LDB = BN;
  constexpr int CQ = CIN / 4, HQR = 34 * CQ, HQ = DYS * HQR;  // float4 per staged row segment / in total
  constexpr int HPASS = (HQ + NT - 1) / NT;
  constexpr int BROWS = NT * 4 / BN, BPASS = (32 + BROWS - 1) / BROWS;
  static_assert(BROWS * BN == NT * 4, "a pass must cover whole rows");
  __shared__ __attribute__((aligned(16))) float smem[DYS * 34 * LDH + 32 * LDB];
  float* Hs = smem;
  float* Bs = smem + DYS * 34 * LDH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int dy0 = DYS == 3 ? 0 : blockIdx.x, n0 = blockIdx.y * BN, split = blockIdx.z;
  const int bcol4 = tid % (BN / 4), brow = tid / (BN / 4);
  const int nb = n0 + bcol4 * 4;
  const int gcolb = nb < p.N ? nb * 4 : S2I_OOB;
  const __amdgpu_buffer_rsrc_t ra_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.g_bytes, 0x00020000);

  f32x4 rh[HPASS], rb[BPASS];
  auto fetch = [&](int pc) {
    const int m0 = pc * 32;
    const int b = m0 >> p.lgHoWo;
    const int r = m0 & ((1 << p.lgHoWo) - 1);
    const int y = r >> p.lgWo, x0 = r & (p.W - 1);
#pragma unroll
    for (int q = 0; q < HPASS; ++q) {
      const int e = tid + q * NT;
      if (e >= HQ) continue;
      const int dyl = e / HQR, er = e - dyl * HQR;
      const int iy = y + dy0 + dyl - 1;
      const int ix = x0 - 1 + er / CQ;
      const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      rh[q] = bload4(ra_rs, ok ? ((b * p.H + iy) * p.W + x0 - 1) * CIN * 4 + er * 16 : S2I_OOB);
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      const int row = brow + q * BROWS;
      if (row >= 32) continue;
      rb[q] = bload4(rg_rs, gcolb == S2I_OOB ? S2I_OOB : (m0 + row) * p.ldg * 4 + gcolb);
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  const int l31 = lane & 31, lh = lane >> 5;
  int aoff[TM];  // row tile -> (horizontal tap, channel half) -> offset inside the halo row segment
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int rt = wm * TM + i;                 // row tile -> (kernel row, horizontal tap, channel half)
    const int dyl = rt / (3 * CIN / 32), rr = rt % (3 * CIN / 32);
    aoff[i] = dyl * 34 * LDH + (rr / (CIN / 32)) * LDH + (rr % (CIN / 32)) * 32;
  }
  const float* hp = Hs + lh * LDH + l31;
  const float* bp = Bs + lh * LDB + wn * TN * 32 + l31;

  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  if (c_begin < c_end) fetch(c_begin);
  for (int pc = c_begin; pc < c_end; ++pc) {
#pragma unroll
    for (int q = 0; q < HPASS; ++q)
      if (tid + q * NT < HQ) *reinterpret_cast<f32x4*>(Hs + (tid + q * NT) * 4) = rh[q];
#pragma unroll
    for (int q = 0; q < BPASS; ++q)
      if (brow + q * BROWS < 32) *reinterpret_cast<f32x4*>(Bs + (brow + q * BROWS) * LDB + bcol4 * 4) = rb[q];
    __syncthreads();
    if (pc + 1 < c_end) fetch(pc + 1);
    {
      float a0[TM], b0[TN], a1[TM], b1[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a0[i] = hp[aoff[i]];
#pragma unroll
      for (int j = 0; j < TN; ++j) b0[j] = bp[j * 32];
#pragma unroll
      for (int kk = 0; kk < 16; kk += 2) {
#pragma unroll
        for (int i = 0; i < TM; ++i) a1[i] = hp[(2 * (kk + 1)) * LDH + aoff[i]];
#pragma unroll
        for (int j = 0; j < TN; ++j) b1[j] = bp[(2 * (kk + 1)) * LDB + j * 32];
        if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b0[j], acc[i][j], 0, 0, 0);
        if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
        if (kk + 2 < 16) {
#pragma unroll
          for (int i = 0; i < TM; ++i) a0[i] = hp[(2 * (kk + 2)) * LDH + aoff[i]];
#pragma unroll
          for (int j = 0; j < TN; ++j) b0[j] = bp[(2 * (kk + 2)) * LDB + j * 32];
        }
        if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b1[j], acc[i][j], 0, 0, 0);
        if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
  }

  // slab row (dy*3 + dx) * CIN + c; the block's 3 * CIN * DYS rows all exist
  store_slab<TM, TN>(p.slab + (size_t)split * p.K * p.N, p.N, acc, lane, wm, wn, n0,
                     [&](int r, long long& row) { row = dy0 * 3 * CIN + r; return true; });
}

// Weight gradient of a 3x3 convolution with at most 4 output channels (GET_IMAGE_G's conv3x3 -> RGB, model.py:287-298):
// K x N = (9 * Ca) x 4 is far too small for matrix cores and the operands are read exactly once, so this is an
// HBM stream.  LPP = Ca/4 lanes share one INPUT pixel (a wave reads 64 consecutive float4 = 1 KB of NHWC), each lane
// multiplies its 4 channels with the float4 output gradient of the 9 output pixels that see this input pixel and
// keeps all 9 x 4 x 4 products in registers across its pixel loop.  One slab [9*Ca][4] per block.
template <int LPP>
__global__ __launch_bounds__(256) void small_n_wgrad_kernel(WgradP p) {
  constexpr int PPW = 64 / LPP;
  __shared__ f32x4 red[4][9 * LPP * 4];  // [wave][tap][q][j]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane % LPP, pl = lane / LPP;
  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ngroups = p.M / PPW;  // W is a power of two >= PPW, so a group never straddles an image row
  const int wmask = p.W - 1;
  // two pixel groups per trip: both groups' loads (their input quads and the 2 x 9 output-gradient pixels) are issued before
  // the first product, which doubles the bytes each wave keeps in flight -- the kernel is a latency-bound stream at two waves
  // per SIMD (144 accumulators), 147 us for 125 MB with one group per trip
  auto load_a = [&](int m) -> f32x4 {
    if (p.a16) {
      const u32x2_t h = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const unsigned short*>(p.a) + (size_t)m * p.Ca + q * 4);
      return f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u),
                   __builtin_bit_cast(float, h[1] << 16), __builtin_bit_cast(float, h[1] & 0xffff0000u)};
    }
    return *reinterpret_cast<const f32x4*>(p.a + (size_t)m * p.Ca + q * 4);
  };
  auto load_g = [&](int m, f32x4 (&gv)[9]) {
    const int ix = m & wmask;
    const int iy = (m >> p.lgWo) & (p.H - 1);
    const float* gp = p.g + (size_t)m * 4;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int oy = iy + 1 - dy, ox = ix + 1 - dx;
        const bool ok = oy >= 0 && oy < p.H && ox >= 0 && ox < p.W;
        gv[dy * 3 + dx] = ok ? *reinterpret_cast<const f32x4*>(gp + ((1 - dy) * p.W + (1 - dx)) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };
  auto fma9 = [&](const f32x4& av, const f32x4 (&gv)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][j] += av[j] * gv[t];
  };
  const int stride = gridDim.x * 4;
  int grp = blockIdx.x * 4 + wave;
  for (; grp + stride < ngroups; grp += 2 * stride) {
    const int m0 = grp * PPW + pl, m1 = (grp + stride) * PPW + pl;
    f32x4 g0[9], g1[9];
    const f32x4 av0 = load_a(m0), av1 = load_a(m1);
    load_g(m0, g0);
    load_g(m1, g1);
    fma9(av0, g0);
    fma9(av1, g1);
  }
  if (grp < ngroups) {
    const int m0 = grp * PPW + pl;
    f32x4 g0[9];
    const f32x4 av0 = load_a(m0);
    load_g(m0, g0);
    fma9(av0, g0);
  }
  // lanes with equal q (different pixels) -> lane q
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v = acc[t][j];
#pragma unroll
      for (int sft = LPP; sft < 64; sft <<= 1)
#pragma unroll
        for (int n = 0; n < 4; ++n) v[n] += __shfl_xor(v[n], sft);
      if (pl == 0) red[wave][(t * LPP + q) * 4 + j] = v;
    }
  __syncthreads();
  float* outp = p.slab + (size_t)blockIdx.x * p.K * 4;
  for (int e = tid; e < 9 * LPP * 4; e += 256) {
    const f32x4 v = red[0][e] + red[1][e] + red[2][e] + red[3][e];
    *reinterpret_cast<f32x4*>(outp + (size_t)e * 4) = v;  // e = tap * Ca + channel: the slab's K row
  }
}

// slab[0] = sum_s slab[s] for a SMALL K x N (n4 float4) and many slabs: one block per 4 float4, 64 slab lanes each
__global__ __launch_bounds__(256) void slab_sum_tree_kernel(float* __restrict__ slab, int S, int n4) {
  __shared__ f32x4 sh[256];
  const int tid = threadIdx.x;
  const int e = blockIdx.x * 4 + (tid & 3), sl = tid >> 2;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (e < n4)
    for (int s = sl; s < S; s += 64) v += *reinterpret_cast<const f32x4*>(slab + ((size_t)s * n4 + e) * 4);
  sh[tid] = v;
  __syncthreads();
  for (int h = 32; h >= 1; h >>= 1) {
    if (sl < h) sh[tid] += sh[tid + h * 4];
    __syncthreads();
  }
  if (sl == 0 && e < n4) *reinterpret_cast<f32x4*>(slab + (size_t)e * 4) = sh[tid];
}

// slab[0] += slab[1..S-1]: a pure float4 stream over the split slabs (full-chip parallel, HBM-bound)
__global__ __launch_bounds__(256) void slab_sum_kernel(float* __restrict__ slab, int S, long long n4) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4;
       e += (long long)gridDim.x * blockDim.x) {
    f32x4 v = *reinterpret_cast<const f32x4*>(slab + e * 4);
    for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(slab + ((size_t)s * n4 + e) * 4);
    *reinterpret_cast<f32x4*>(slab + e * 4) = v;
  }
}

// Reduce the split slabs and write the reference's OIHW gradient tensor.  A [T][RT][32] tile goes through
// LDS so that both the slab reads (32 consecutive columns) and the OIHW writes (runs of (cin, ky, kx) for one
// cout) are coalesced.  fold: the 3x3 parameter tap (ky,kx) collects the 4 effective 4x4 taps it was summed into.
//   non-swap: slab rows (tap, cin), columns cout;   swap: slab rows (tap, cout), columns cin.
//   The tile is [T][TS] with rows of 33 floats inside a tap and TS = RT * 33 padded (wg_finish_tap_stride) so that the taps
// of the OIHW write loop, its fastest index, fall on different LDS banks.  RT is a power of two (lgRT); TP is the number
// of parameter taps as a constant (9, 16, 1) or 0 for any (Tp).
//   Each element is 0 + slab0 + slab1 ..., read 16 bytes wide where V4 (N % 4 == 0).
struct WgFinishP {
  const float* slab;
  float* grad;
  int S, K, N, Cg, O, I, Tp, T, swap, fold, accumulate, lgRT, TS, i_off, I_total;
};

template <int TP, bool V4>
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const WgFinishP p) {
  extern __shared__ float tile[];  // [T][TS]
  const int tid = threadIdx.x;
  const int Tp = TP > 0 ? TP : p.Tp;
  const int lgRT = p.lgRT, RT = 1 << lgRT, TS = p.TS, N = p.N, S = p.S;
  const int ncols = p.swap ? p.I : p.O, nrows = p.swap ? p.O : p.I;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * RT;
  const size_t sstride = (size_t)p.K * N;
  if (V4) {
    const int nload = (p.T << lgRT) * 8;
    for (int e = tid; e < nload; e += 256) {
      const int c_l = (e & 7) * 4;
      const int r_l = (e >> 3) & (RT - 1);
      const int t = (e >> 3) >> lgRT;
      const int c = c0 + c_l, r = r0 + r_l;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c < ncols && r < nrows) {
        const float* sp = p.slab + ((size_t)t * p.Cg + r) * N + c;
        for (int s = 0; s < S; ++s) v += *reinterpret_cast<const f32x4*>(sp + s * sstride);
      }
      float* tp = tile + t * TS + r_l * 33 + c_l;
#pragma unroll
      for (int j = 0; j < 4; ++j) tp[j] = c + j < ncols ? v[j] : 0.f;
    }
  } else {
    const int nload = (p.T << lgRT) * 32;
    for (int e = tid; e < nload; e += 256) {
      const int c_l = e & 31;
      const int r_l = (e >> 5) & (RT - 1);
      const int t = (e >> 5) >> lgRT;
      const int c = c0 + c_l, r = r0 + r_l;
      float v = 0.f;
      if (c < ncols && r < nrows) {
        const float* sp = p.slab + ((size_t)t * p.Cg + r) * N + c;
        for (int s = 0; s < S; ++s) v += sp[s * sstride];
      }
      tile[t * TS + r_l * 33 + c_l] = v;
    }
  }
  __syncthreads();
  const int nout = 32 * RT * Tp;
  for (int w = tid; w < nout; w += 256) {
    const int rest = w / Tp;
    const int tapo = w - rest * Tp;
    int o_l, i_l, r_l, c_l;
    if (p.swap) { i_l = rest & 31; o_l = rest >> 5; r_l = o_l; c_l = i_l; }
    else { i_l = rest & (RT - 1); o_l = rest >> lgRT; r_l = i_l; c_l = o_l; }
    const int o = p.swap ? r0 + o_l : c0 + o_l;
    const int i = p.swap ? c0 + i_l : r0 + i_l;
    if (o >= p.O || i >= p.I) continue;
    float v;
    if (p.fold) {
      const int ky = tapo / 3, kx = tapo - ky * 3;
      v = 0.f;
#pragma unroll
      for (int ay = 0; ay < 2; ++ay)
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) {
          const int t = ((2 - ky) + ay) * 4 + (2 - kx) + ax;  // ky=0:{2,3} ky=1:{1,2} ky=2:{0,1}
          v += tile[t * TS + r_l * 33 + c_l];
        }
    } else {
      v = tile[tapo * TS + r_l * 33 + c_l];
    }
    float* gp = p.grad + ((size_t)o * p.I_total + p.i_off + i) * Tp + tapo;
    *gp = p.accumulate ? *gp + v : v;
  }
}

// floats from one tap of the finish tile to the next: RT rows of 33, padded so that TS = 32 / Tp (rounded) mod 32.  The
// write loop's lanes run over the taps first, then over a few rows or columns (one bank each): 4 banks per tap for the 9 taps
// of a 3x3, 2 for the 16 of a 4x4.
static int wg_finish_tap_stride(int RT, int Tp) {
  int q = (32 + Tp / 2) / Tp;
  if (q < 1) q = 1;
  int ts = RT * 33;
  while ((ts & 31) != (q & 31)) ++ts;
  return ts;
}

template <bool V4>
static void launch_wgrad_finish(const WgFinishP& fp, dim3 grid, size_t shb, hipStream_t st) {
  if (fp.Tp == 9) hipLaunchKernelGGL((wgrad_finish_kernel<9, V4>), grid, dim3(256), shb, st, fp);
  else if (fp.Tp == 16) hipLaunchKernelGGL((wgrad_finish_kernel<16, V4>), grid, dim3(256), shb, st, fp);
  else if (fp.Tp == 1) hipLaunchKernelGGL((wgrad_finish_kernel<1, V4>), grid, dim3(256), shb, st, fp);
  else hipLaunchKernelGGL((wgrad_finish_kernel<0, V4>), grid, dim3(256), shb, st, fp);
}

}  // namespace

template <int BM, int BN, int WM, int WN>
static void launch_wgrad_split(const WgradP& p, dim3 grid, int planes, hipStream_t st) {
  if (planes == 1) hipLaunchKernelGGL((igemm_wgrad_split_kernel<BM, BN, WM, WN, 1>), grid, dim3(256), 0, st, p);
  else if (planes == 2) hipLaunchKernelGGL((igemm_wgrad_split_kernel<BM, BN, WM, WN, 2>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((igemm_wgrad_split_kernel<BM, BN, WM, WN, 3>), grid, dim3(256), 0, st, p);
}

// launches what plan_wgrad decided, then the finish: slab sum and the transpose into OIHW
static int launch_wgrad(const s2i_wgrad_desc* d, const WgPlan& pl, const float* a, const float* cvec, const float* g,
                        float* grad_oihw, void* ws, size_t ws_bytes, void* stream, int a16, int g16, const float* a_coef) {
  S2I_REQUIRE((a || d->Ca == 0) && g && grad_oihw, "wgrad: null operand");
  S2I_REQUIRE(d->Cc == 0 || cvec != nullptr, "wgrad: cvec is null but Cc > 0");
  const size_t need = wg_workspace_bytes(pl, d->N);
  S2I_REQUIRE(ws && ws_bytes >= need, "wgrad: workspace too small (%zu < %zu)", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  WgradP p;
  p.a = a; p.cvec = cvec; p.g = g; p.slab = (float*)ws;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Ca = d->Ca; p.Cc = d->Cc; p.Cin = pl.Cin;
  p.Ho = pl.Ho; p.Wo = pl.Wo; p.lgWo = s2i_ilog2(pl.Wo); p.lgHoWo = s2i_ilog2(pl.Ho * pl.Wo);
  p.M = pl.M; p.N = d->N; p.ldg = d->ldg; p.K = pl.K; p.T = pl.T; p.kind = d->kind;
  p.cps = pl.cps; p.nchunks = pl.nchunks;
  p.a16 = a16; p.g16 = g16;
  p.a_coef = a_coef; p.a_groups = d->a_groups < 1 ? 1 : d->a_groups; p.a_ipg = d->B / p.a_groups;
  {
    const unsigned long long ab = (unsigned long long)d->B * d->H * d->W * d->Ca * (a16 ? 2ull : 4ull);
    const unsigned long long gb = (unsigned long long)pl.M * d->ldg * (g16 ? 2ull : 4ull);
    S2I_REQUIRE(ab < 0x7ff00000ull && gb < 0x7ff00000ull, "wgrad: tensor exceeds the 2 GiB buffer-addressing window");
    p.a_bytes = (unsigned)ab; p.g_bytes = (unsigned)gb;
    p.c_bytes = (unsigned)((unsigned long long)d->B * d->Cc * 4ull);
  }
  const dim3 grid(pl.gx, pl.gy, pl.gz);
#define WG_LAUNCH(id, ...) case id: hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(pl.threads), 0, st, p); break
#define WG_LAUNCH_SPLIT(id, ...) case id: launch_wgrad_split<__VA_ARGS__>(p, grid, pl.planes, st); break
  switch (pl.kernel) {
    WG_LAUNCH(WG_F32_128x128, igemm_wgrad_kernel<128, 128, 2, 2>);
    WG_LAUNCH(WG_F32_128x64, igemm_wgrad_kernel<128, 64, 2, 2>);
    WG_LAUNCH(WG_F32_128x32, igemm_wgrad_kernel<128, 32, 4, 1>);
    WG_LAUNCH(WG_F32_64x64, igemm_wgrad_kernel<64, 64, 2, 2>);
    WG_LAUNCH(WG_F32_256x128, igemm_wgrad_kernel<256, 128, 4, 2>);
    WG_LAUNCH(WG_F32_256x256, igemm_wgrad_kernel<256, 256, 4, 4>);
    WG_LAUNCH(WG_F32_96x64, igemm_wgrad_kernel<96, 64, 3, 1>);
    WG_LAUNCH(WG_F32_96x32, igemm_wgrad_kernel<96, 32, 3, 1>);
    WG_LAUNCH(WG_F32IN_128x128, igemm_wgrad_kernel<128, 128, 2, 2, true>);
    WG_LAUNCH(WG_B16_128x128, igemm_wgrad_b16_kernel<128, 128, 2, 2>);
    WG_LAUNCH(WG_B16_128x64, igemm_wgrad_b16_kernel<128, 64, 2, 2>);
    WG_LAUNCH(WG_B16_128x32, igemm_wgrad_b16_kernel<128, 32, 4, 1>);
    WG_LAUNCH(WG_B16_64x64, igemm_wgrad_b16_kernel<64, 64, 2, 2>);
    WG_LAUNCH(WG_B16_256x128, igemm_wgrad_b16_kernel<256, 128, 4, 2>);
    WG_LAUNCH(WG_B16_256x256, igemm_wgrad_b16_kernel<256, 256, 4, 4>);
    WG_LAUNCH(WG_B16D1_64x64, igemm_wgrad_b16_kernel<64, 64, 2, 2, true>);
    WG_LAUNCH_SPLIT(WG_SPLIT_128x128, 128, 128, 2, 2);
    WG_LAUNCH_SPLIT(WG_SPLIT_128x64, 128, 64, 2, 2);
    WG_LAUNCH_SPLIT(WG_SPLIT_128x32, 128, 32, 4, 1);
    WG_LAUNCH_SPLIT(WG_SPLIT_64x64, 64, 64, 2, 2);
    WG_LAUNCH(WG_ROWS3_32x64, wgrad_k3_rows_kernel<32, 64, 3, 1, 3>);
    WG_LAUNCH(WG_ROWS3_32x32, wgrad_k3_rows_kernel<32, 32, 3, 1, 3>);
    WG_LAUNCH(WG_ROWS3_64x128, wgrad_k3_rows_kernel<64, 128, 2, 2, 1>);
    WG_LAUNCH(WG_ROWS3_64x64, wgrad_k3_rows_kernel<64, 64, 2, 2, 1>);
    WG_LAUNCH(WG_ROWS3_64x32, wgrad_k3_rows_kernel<64, 32, 2, 1, 1>);
    WG_LAUNCH(WG_SMALLN_16, small_n_wgrad_kernel<4>);
    WG_LAUNCH(WG_SMALLN_32, small_n_wgrad_kernel<8>);
    WG_LAUNCH(WG_SMALLN_64, small_n_wgrad_kernel<16>);
    default: S2I_FAIL("wgrad: the plan names no kernel (%d)", (int)pl.kernel);
  }
#undef WG_LAUNCH
#undef WG_LAUNCH_SPLIT
  S2I_LAUNCH_CHECK("igemm_wgrad");
  {
    const int ncols = d->swap ? d->I : d->O, nrows = d->swap ? d->O : d->I;
    int RT = 8;
    while (RT > 1 && (long long)s2i_cdiv(ncols, 32) * s2i_cdiv(nrows, RT) < 128) RT >>= 1;
    const int Tp = d->KH * d->KW;
    dim3 fgrid(s2i_cdiv(ncols, 32), s2i_cdiv(nrows, RT));
    WgFinishP fp;
    fp.slab = (const float*)ws; fp.grad = grad_oihw;
    fp.S = pl.slabs; fp.K = pl.K; fp.N = d->N; fp.Cg = pl.Cin; fp.O = d->O; fp.I = d->I; fp.Tp = Tp; fp.T = pl.T;
    fp.swap = d->swap; fp.fold = d->fold; fp.accumulate = d->accumulate; fp.lgRT = s2i_ilog2(RT);
    fp.TS = wg_finish_tap_stride(RT, Tp); fp.i_off = d->i_off; fp.I_total = d->I_total > 0 ? d->I_total : d->I;
    const size_t shb = (size_t)pl.T * fp.TS * sizeof(float);
    const long long kn = (long long)pl.K * d->N;
    // two passes (measured: 27 + 17 us against 53 us for one pass that walks the slabs tile by tile, and 215 against
    // 16 + 10 us with the tree sum inside the finish blocks of a small K x N): first the split slabs are folded into slab 0,
    // then the tile kernel transposes slab 0 into OIHW
    if (pl.kernel >= WG_SMALLN_16 || (fp.S >= 32 && (kn % 4) == 0 && kn / 4 < (1 << 18))) {
      // many slabs of a small K x N: the float4 stream below would run on a handful of blocks
      hipLaunchKernelGGL(slab_sum_tree_kernel, dim3(s2i_cdiv(kn / 4, 4)), dim3(256), 0, st, (float*)ws, fp.S, (int)(kn / 4));
      S2I_LAUNCH_CHECK("slab_sum_tree");
      fp.S = 1;
    } else if (fp.S > 2 && (kn % 4) == 0) {
      int sb = s2i_cdiv(kn / 4, 256);
      if (sb > 4096) sb = 4096;
      hipLaunchKernelGGL(slab_sum_kernel, dim3(sb), dim3(256), 0, st, (float*)ws, fp.S, kn / 4);
      S2I_LAUNCH_CHECK("slab_sum");
      fp.S = 1;
    }
    if ((d->N & 3) == 0 && ncols <= d->N) launch_wgrad_finish<true>(fp, fgrid, shb, st);
    else launch_wgrad_finish<false>(fp, fgrid, shb, st);
  }
  S2I_LAUNCH_CHECK("wgrad_finish");
  return 0;
}

static int conv_wgrad_impl(const s2i_wgrad_desc* d, int planes, const float* a, const float* cvec, const float* g,
                           float* grad_oihw, void* ws, size_t ws_bytes, void* stream, int a16 = 0, int g16 = 0, const float* a_coef = nullptr) {
  WgMode mode;
  WgPlan pl;
  if (wg_mode(a16, g16, planes, a_coef != nullptr, &mode) || plan_wgrad(d, mode, &pl)) return 1;
  return launch_wgrad(d, pl, a, cvec, g, grad_oihw, ws, ws_bytes, stream, a16, g16, a_coef);
}

extern "C" int s2i_conv_wgrad_in(const s2i_wgrad_desc* d, const float* a_raw, const float* a_coef, const float* g,
                                 float* grad_oihw, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE(a_coef != nullptr, "wgrad(apply-on-load): null coefficient table");
  return conv_wgrad_impl(d, 0, a_raw, nullptr, g, grad_oihw, ws, ws_bytes, stream, 0, 0, a_coef);
}

extern "C" int s2i_conv_wgrad_dt(const s2i_wgrad_desc* d, const void* a, int a_dtype, const float* cvec, const void* g,
                                 int g_dtype, float* grad_oihw, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE((a_dtype == S2I_DT_F32 || a_dtype == S2I_DT_BF16) && (g_dtype == S2I_DT_F32 || g_dtype == S2I_DT_BF16),
              "wgrad: unknown dtype");
  return conv_wgrad_impl(d, 0, (const float*)a, cvec, (const float*)g, grad_oihw, ws, ws_bytes, stream,
                         a_dtype == S2I_DT_BF16, g_dtype == S2I_DT_BF16);
}

extern "C" int s2i_conv_wgrad(const s2i_wgrad_desc* d, const float* a, const float* cvec, const float* g,
                              float* grad_oihw, void* ws, size_t ws_bytes, void* stream) {
  return conv_wgrad_impl(d, 0, a, cvec, g, grad_oihw, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_wgrad_split(const s2i_wgrad_desc* d, int planes, const float* a, const float* cvec,
                                    const float* g, float* grad_oihw, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE(planes >= 1 && planes <= 3, "wgrad(split): need 1 to 3 bf16 planes");
  return conv_wgrad_impl(d, planes, a, cvec, g, grad_oihw, ws, ws_bytes, stream);
}
