// General NHWC convolution (Inception-v3 scorer): any kernel extent, stride, padding, spatial size and channel count.
// Same tile machinery as igemm_fwd_kernel (256 threads, 2 x 2 waves, A as [k][m] and B as [k][n] in LDS, mma_chunk, buffer
// loads whose out-of-range offset reads zero).  The reduction index is k = (ky * kw + kx) * C + c.  The pixel of each
// gathered row is decoded once per thread (ordinary division: the extents are not powers of two); the tap of a 4-wide
// k group is decoded once per 32-deep chunk.  VEC: C and the pixel stride are multiples of 4, so a thread's four k lie
// in one tap and are one 16-byte load; otherwise (the 3-channel image) each k is its own 4-byte load.
#include "s2i_igemm.h"

namespace {

struct Conv2dP {
  const float* __restrict__ x;
  const float* __restrict__ w;
  const float* __restrict__ bias;
  float* __restrict__ y;
  int H, W, C, ldx, N, Np, kw, sh, sw, ph, pw, Wo, HoWo, ldy, coff, relu;
  int M, K, nchunks;
  unsigned x_bytes, w_bytes;
};

template <int BM, int BN, bool VEC>
__global__ __launch_bounds__(256, 3) void conv2d_fwd_kernel(Conv2dP p) {
  constexpr int WAVES_M = 2, WAVES_N = 2;
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int LDA = BM + 1, LDB = BN;
  constexpr int ASLOTS = BM / 32, BSLOTS = BN / 32, BROWS_PER_PASS = 1024 / BN;
  __shared__ __attribute__((aligned(16))) float smem[32 * LDB + 32 * LDA];
  float* Bs = smem;              // written with 16-byte stores: first, aligned
  float* As = smem + 32 * LDB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kq = tid & 7, mrow = tid >> 3;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);

  int pbase[ASLOTS], iy0[ASLOTS], ix0[ASLOTS];   // pixel index of tap (0, 0) (may lie outside) and its coordinates
#pragma unroll
  for (int i = 0; i < ASLOTS; ++i) {
    const int m = m0 + mrow + 32 * i;
    if (m < p.M) {
      const int b = m / p.HoWo, r = m - b * p.HoWo;
      const int oy = r / p.Wo, ox = r - oy * p.Wo;
      iy0[i] = oy * p.sh - p.ph;
      ix0[i] = ox * p.sw - p.pw;
      pbase[i] = (b * p.H + iy0[i]) * p.W + ix0[i];
    } else {
      iy0[i] = -(1 << 28);      // no tap of a row past M is in range: it gathers zeros
      ix0[i] = 0;
      pbase[i] = 0;
    }
  }
  const int bcol4 = tid % (BN / 4), brow = tid / (BN / 4);
  const int ncol = n0 + bcol4 * 4;
  const bool ncol_ok = ncol < p.Np;   // Np is a multiple of 4: the whole 16-byte group is inside the row

  f32x4 ra[ASLOTS], rb[BSLOTS];
  auto fetch = [&](int kc) {
    const int k = kc * 32 + kq * 4;
    if constexpr (VEC) {
      const int t = k / p.C, c = k - t * p.C;
      const int ky = t / p.kw, kx = t - ky * p.kw;
      const bool kv = k < p.K;
      const int toff = ky * p.W + kx;
#pragma unroll
      for (int i = 0; i < ASLOTS; ++i) {
        const bool ok = kv && (unsigned)(iy0[i] + ky) < (unsigned)p.H && (unsigned)(ix0[i] + kx) < (unsigned)p.W;
        ra[i] = bload4(rx, ok ? ((pbase[i] + toff) * p.ldx + c) * 4 : S2I_OOB);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ke = k + e;
        const int t = ke / p.C, c = ke - t * p.C;
        const int ky = t / p.kw, kx = t - ky * p.kw;
        const bool kv = ke < p.K;
        const int toff = ky * p.W + kx;
#pragma unroll
        for (int i = 0; i < ASLOTS; ++i) {
          const bool ok = kv && (unsigned)(iy0[i] + ky) < (unsigned)p.H && (unsigned)(ix0[i] + kx) < (unsigned)p.W;
          ra[i][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                   rx, ok ? ((pbase[i] + toff) * p.ldx + c) * 4 : S2I_OOB, 0, 0));
        }
      }
    }
#pragma unroll
    for (int q = 0; q < BSLOTS; ++q) {
      const int kb = kc * 32 + brow + q * BROWS_PER_PASS;
      rb[q] = bload4(rw, (kb < p.K && ncol_ok) ? (kb * p.Np + ncol) * 4 : S2I_OOB);
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);

  fetch(0);
  for (int kc = 0; kc < p.nchunks; ++kc) {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) As[(kq * 4 + j) * LDA + mrow + 32 * i] = ra[i][j];
#pragma unroll
    for (int q = 0; q < BSLOTS; ++q)
      *reinterpret_cast<f32x4*>(Bs + (brow + q * BROWS_PER_PASS) * LDB + bcol4 * 4) = rb[q];
    __syncthreads();
    if (kc + 1 < p.nchunks) fetch(kc + 1);
    mma_chunk<TM, TN, LDA, LDB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
    __syncthreads();
  }

  store_tile<TM, TN>(p.y + p.coff, p.ldy, p.N, false, p.bias, p.relu ? S2I_ACT_RELU : S2I_ACT_NONE, 0, acc, lane, wm, wn, n0,
                     [&](int r, long long& row) { row = m0 + r; return m0 + r < p.M; });
}

// Block tile from a round model: blocks are issued in rounds of 3 per CU; a round's time grows with the tile's work over
// its relative MFMA efficiency (fragment reads per MFMA grow as the tile shrinks).
struct Conv2dTile { int bm, bn; float eff; };
const Conv2dTile kConv2dTiles[4] = {{0, 0, 0.f}, {128, 128, 1.0f}, {128, 64, 0.85f}, {64, 64, 0.6f}};

int conv2d_validate(const s2i_conv2d_desc* d, int* tile_out) {
  S2I_REQUIRE(d, "conv2d: null descriptor");
  S2I_REQUIRE(d->B >= 1 && d->H >= 1 && d->W >= 1 && d->C >= 1 && d->N >= 1,
              "conv2d: B, H, W, C, N must be positive (got %d, %d, %d, %d, %d)", d->B, d->H, d->W, d->C, d->N);
  S2I_REQUIRE(d->kh >= 1 && d->kw >= 1 && d->kh <= 16 && d->kw <= 16, "conv2d: kernel %d x %d outside 1..16", d->kh, d->kw);
  S2I_REQUIRE(d->sh >= 1 && d->sw >= 1, "conv2d: stride %d x %d must be positive", d->sh, d->sw);
  S2I_REQUIRE(d->ph >= 0 && d->pw >= 0 && d->ph < d->kh && d->pw < d->kw, "conv2d: padding %d x %d outside [0, kernel)",
              d->ph, d->pw);
  const int ldx = d->ldx ? d->ldx : d->C;
  S2I_REQUIRE(ldx >= d->C, "conv2d: ldx %d < C %d", ldx, d->C);
  const int eh = d->H + 2 * d->ph - d->kh, ew = d->W + 2 * d->pw - d->kw;
  S2I_REQUIRE(eh >= 0 && ew >= 0, "conv2d: kernel larger than the padded input");
  S2I_REQUIRE(d->Ho == eh / d->sh + 1 && d->Wo == ew / d->sw + 1, "conv2d: output %d x %d, the geometry gives %d x %d",
              d->Ho, d->Wo, eh / d->sh + 1, ew / d->sw + 1);
  S2I_REQUIRE(d->coff >= 0 && d->ldy >= d->coff + d->N, "conv2d: channels [%d, %d) do not fit a pixel stride of %d",
              d->coff, d->coff + d->N, d->ldy);
  S2I_REQUIRE(d->relu == 0 || d->relu == 1, "conv2d: relu must be 0 or 1");
  S2I_REQUIRE(d->tile >= 0 && d->tile <= 3, "conv2d: tile %d outside 0..3", d->tile);
  // 32-bit offsets inside the kernel, and buffer records below the out-of-range offset
  const long long lim = 0x7fff0000LL;
  const long long K = (long long)d->kh * d->kw * d->C, Np = (d->N + 3) & ~3;
  S2I_REQUIRE((long long)d->B * d->H * d->W * ldx * 4 < lim, "conv2d: input larger than 2 GB: split the batch");
  S2I_REQUIRE((long long)d->B * d->Ho * d->Wo * d->ldy * 4 < lim, "conv2d: output larger than 2 GB: split the batch");
  S2I_REQUIRE(K * Np * 4 < lim, "conv2d: weight larger than 2 GB");
  if (tile_out) {
    int best = d->tile;
    if (!best) {
      const long long M = (long long)d->B * d->Ho * d->Wo;
      float cbest = 0.f;
      for (int t = 1; t <= 3; ++t) {
        const Conv2dTile& c = kConv2dTiles[t];
        const long long blocks = ((M + c.bm - 1) / c.bm) * ((d->N + c.bn - 1) / c.bn);
        const float cost = (float)((blocks + 767) / 768) * c.bm * c.bn / c.eff;
        if (!best || cost < cbest) { best = t; cbest = cost; }
      }
    }
    *tile_out = best;
  }
  return 0;
}

template <int BM, int BN>
void launch_conv2d(const Conv2dP& p, bool vec, hipStream_t st) {
  dim3 grid(s2i_cdiv(p.M, BM), s2i_cdiv(p.N, BN));
  if (vec) hipLaunchKernelGGL((conv2d_fwd_kernel<BM, BN, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((conv2d_fwd_kernel<BM, BN, false>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" int s2i_conv2d_plan(const s2i_conv2d_desc* d) {
  int tile = 0;
  if (conv2d_validate(d, &tile)) return -1;
  return tile;
}

extern "C" size_t s2i_conv2d_weight_elems(const s2i_conv2d_desc* d) {
  if (conv2d_validate(d, nullptr)) return 0;
  return (size_t)d->kh * d->kw * d->C * ((d->N + 3) & ~3);
}

extern "C" int s2i_conv2d_forward(const s2i_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y,
                                  void* stream) {
  int tile = 0;
  if (conv2d_validate(d, &tile)) return 1;
  S2I_REQUIRE(x && w && y, "conv2d: null pointer");
  Conv2dP p;
  p.x = x; p.w = w; p.bias = bias; p.y = y;
  p.H = d->H; p.W = d->W; p.C = d->C; p.ldx = d->ldx ? d->ldx : d->C;
  p.N = d->N; p.Np = (d->N + 3) & ~3;
  p.kw = d->kw; p.sh = d->sh; p.sw = d->sw; p.ph = d->ph; p.pw = d->pw;
  p.Wo = d->Wo; p.HoWo = d->Ho * d->Wo; p.ldy = d->ldy; p.coff = d->coff; p.relu = d->relu;
  p.M = d->B * d->Ho * d->Wo;
  p.K = d->kh * d->kw * d->C;
  p.nchunks = s2i_cdiv(p.K, 32);
  p.x_bytes = (unsigned)((size_t)d->B * d->H * d->W * p.ldx * 4);
  p.w_bytes = (unsigned)((size_t)p.K * p.Np * 4);
  const bool vec = p.C % 4 == 0 && p.ldx % 4 == 0 && ((uintptr_t)x & 15) == 0;
  S2I_REQUIRE(((uintptr_t)w & 15) == 0, "conv2d: the packed weight must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (tile == 1) launch_conv2d<128, 128>(p, vec, st);
  else if (tile == 2) launch_conv2d<128, 64>(p, vec, st);
  else launch_conv2d<64, 64>(p, vec, st);
  S2I_LAUNCH_CHECK("conv2d_fwd");
  return 0;
}
