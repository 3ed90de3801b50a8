// What the forward convolution launches that is no matrix tile: the lanes-per-pixel kernel for <= 4 output channels, the
// split-K reducers and the weight-plane splitter; and launch_igemm_fwd, the one door to the matrix tiles, which hands the
// plan to the unit that compiled its tile shape (s2i_conv_fwd_<BM>x<BN>.hip, s2i_conv_fwd_split.hip; the kernel templates
// are in s2i_conv_fwd.h, which this unit does not include).
// The gather formulation is described in s2i_igemm.h; the dispatcher is conv_forward_impl (s2i_conv.hip).
#include "s2i_igemm.h"

namespace {

// fp32 packed weights P[T][R][C] -> NP bf16 planes in BOTH operand layouts from one read:
//   dst_rc [plane][T][R][C] (input gradient: n = r, k = c) and dst_cr [plane][T][C][R] (forward: n = c, k = r); either may be null
__global__ __launch_bounds__(256) void split_packed_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst_rc,
                                                           unsigned short* __restrict__ dst_cr, int R, int C, int NP,
                                                           long long plane) {
  __shared__ float tile[32][33];
  const int t = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const float* sp = src + (size_t)t * R * C;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    tile[ty + 8 * k][tx] = (r < R && c < C) ? sp[(size_t)r * C + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (dst_rc) {
      const int r = r0 + ty + 8 * k, c = c0 + tx;
      if (r < R && c < C) {
        float v = tile[ty + 8 * k][tx];
        const size_t o = ((size_t)t * R + r) * C + c;
        for (int pl = 0; pl < NP; ++pl) {
          const __bf16 h = (__bf16)v;
          dst_rc[pl * plane + o] = __builtin_bit_cast(unsigned short, h);
          v -= (float)h;
        }
      }
    }
    if (dst_cr) {
      const int c = c0 + ty + 8 * k, r = r0 + tx;
      if (r < R && c < C) {
        float v = tile[tx][ty + 8 * k];
        const size_t o = ((size_t)t * C + c) * R + r;
        for (int pl = 0; pl < NP; ++pl) {
          const __bf16 h = (__bf16)v;
          dst_cr[pl * plane + o] = __builtin_bit_cast(unsigned short, h);
          v -= (float)h;
        }
      }
    }
  }
}

// Convolutions with at most 4 output channels (GET_IMAGE_G's conv3x3 -> RGB, model.py:287-298, and the input
// gradient of the discriminators' first conv): HBM-bound, so no matrix cores.  LPP = Ca/4 lanes share one output
// pixel, each multiplying its 4 input channels into the 4 outputs (weights [t][c][4] in LDS), then a shuffle
// reduction; a wave reads PPW = 64/LPP whole pixels per tap, i.e. contiguous NHWC bytes.
template <int LPP>
__global__ __launch_bounds__(256) void small_n_conv_kernel(IgemmP p) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [T][Ca][4]
  constexpr int PPW = 64 / LPP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int phase = blockIdx.z;
  const int py = phase >> 1, px = phase & 1;
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);
  // stage the 4 output columns of every (tap, channel) row
  for (int e = tid; e < p.T * p.Ca; e += 256) {
    const int t = e / p.Ca, c = e - t * p.Ca;
    const int tw = tap_weight(p.kind, p.flip, p.T, t, py, px);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p.wt) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (n < p.N) v[n] = p.w[((size_t)tw * p.wR + n) * p.ldw + c];
    } else {
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (n < p.N && n < p.ldw) v[n] = p.w[((size_t)tw * p.wR + c) * p.ldw + n];
    }
    *reinterpret_cast<f32x4*>(wl + e * 4) = v;
  }
  __syncthreads();
  const int q = lane % LPP, pl = lane / LPP;
  // grid-stride over groups of PPW pixels per wave: the weight table above is staged once per block, not once per 4 * PPW
  // pixels (the one-group-per-wave form ran the D_NET256 image gradient at 0.2 TB/s)
  const int ngroups = (p.M + PPW - 1) / PPW;
  for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
    const int m = grp * PPW + pl;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int b = 0, oy = 0, ox = 0;
    if (m < p.M) {
      b = m >> p.lgHoWo;
      const int r = m & ((1 << p.lgHoWo) - 1);
      oy = r >> p.lgWo;
      ox = r & (p.Wo - 1);
      const int by = oy * s - pad, bx = ox * s - pad;
      const unsigned mask = tap_mask(p.kind, kw, by, bx, p.H, p.W, py, px);
      const long long xo = (((long long)b * p.H + by) * p.W + bx) * p.Cx + q * 4;
      for (int t = 0; t < p.T; ++t) {
        if (!((mask >> t) & 1u)) continue;
        int dy, dx;
        tap_delta(p.kind, kw, t, py, px, dy, dx);
        const long long xe = xo + ((long long)dy * p.W + dx) * p.Cx;
        f32x4 xv;
        if (p.x16) {
          const u32x2_t h = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const unsigned short*>(p.x) + xe);
          xv = f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u),
                     __builtin_bit_cast(float, h[1] << 16), __builtin_bit_cast(float, h[1] & 0xffff0000u)};
        } else {
          xv = *reinterpret_cast<const f32x4*>(p.x + xe);
        }
        const float* wp = wl + ((size_t)t * p.Ca + q * 4) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += xv[j] * *reinterpret_cast<const f32x4*>(wp + j * 4);
      }
    }
#pragma unroll
    for (int sft = 1; sft < LPP; sft <<= 1)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[n] += __shfl_xor(acc[n], sft);
    if (q == 0 && m < p.M) {
      long long row = m;
      if (p.kind == S2I_TCONV_K4S2) row = ((long long)b * (2 * p.Ho) + 2 * oy + py) * (2 * p.Wo) + 2 * ox + px;
      f32x4 o;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        float v = acc[n];
        if (p.bias && n < p.N) v += p.bias[n];
        if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
        else if (p.act == S2I_ACT_TANH) v = tanhf(v);
        else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
        o[n] = v;
      }
      if (p.N == 4 && !p.y16 && (p.ldy & 3) == 0) {
        *reinterpret_cast<f32x4*>(p.y + row * p.ldy) = o;
      } else {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          if (n >= p.N) break;
          if (p.y16) reinterpret_cast<unsigned short*>(p.y)[row * p.ldy + n] = f2bf(o[n]);
          else p.y[row * p.ldy + n] = o[n];
        }
      }
    }
  }
}

__global__ void splitk_reduce_kernel(const float* __restrict__ slab, int S, long long rows, int N,
                                     const float* __restrict__ bias, int act, float* __restrict__ y,
                                     int ldy, int y16) {
  const long long total = rows * N;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / N;
    const int n = (int)(e - row * N);
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += slab[(size_t)s * total + e];
    if (bias) v += bias[n];
    if (act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
    else if (act == S2I_ACT_TANH) v = tanhf(v);
    else if (act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
    if (y16) reinterpret_cast<unsigned short*>(y)[row * ldy + n] = f2bf(v);
    else y[row * ldy + n] = v;
  }
}

// split-K reduction fused with the BatchNorm column statistics: y = sum_s slab[s], part = per-row-chunk column
// sums and sums of squares (the layout s2i_colstats writes).  256 threads = cpb column quads x 256/cpb row lanes.
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const float* __restrict__ slab, int S, long long rows,
                                                                  int N, float* __restrict__ y, int ldy,
                                                                  float* __restrict__ part, int nparts, int cpb,
                                                                  int ppg, long long Rg, int y16) {
  __shared__ f32x4 sh[2][256];
  const int tid = threadIdx.x;
  const int rpb = 256 / cpb;
  const int ql = tid % cpb, rl = tid / cpb;
  const int quad = blockIdx.y * cpb + ql;
  const int Q = N / 4;
  const int grp = blockIdx.x / ppg, pp = blockIdx.x - grp * ppg;  // BatchNorm group of this row chunk
  const long long chunk = (Rg + ppg - 1) / ppg;
  const long long r0 = grp * Rg + pp * chunk;
  const long long gend = (grp + 1) * Rg < rows ? (grp + 1) * Rg : rows;
  const long long r1 = r0 + chunk < gend ? r0 + chunk : gend;
  const size_t sstride = (size_t)rows * N;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  if (quad < Q) {
    for (long long row = r0 + rl; row < r1; row += rpb) {
      const float* sp = slab + row * N + quad * 4;
      f32x4 v = *reinterpret_cast<const f32x4*>(sp);
      for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(sp + s * sstride);
      if (y16) {
        unsigned short* yp = reinterpret_cast<unsigned short*>(y) + row * ldy + quad * 4;
        *reinterpret_cast<u32x2_t*>(yp) = u32x2_t{(unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16),
                                                 (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16)};
      } else {
        *reinterpret_cast<f32x4*>(y + row * ldy + quad * 4) = v;
      }
      s0 += v;
      s1 += v * v;
    }
  }
  sh[0][tid] = s0;
  sh[1][tid] = s1;
  __syncthreads();
  if (rl == 0 && quad < Q) {
    for (int r = 1; r < rpb; ++r) {
      s0 += sh[0][r * cpb + ql];
      s1 += sh[1][r * cpb + ql];
    }
    *reinterpret_cast<f32x4*>(part + ((size_t)0 * nparts + blockIdx.x) * N + quad * 4) = s0;
    *reinterpret_cast<f32x4*>(part + ((size_t)1 * nparts + blockIdx.x) * N + quad * 4) = s1;
  }
}

}  // namespace

int launch_igemm_fwd(const FwdPlan& pl, const IgemmP& p, hipStream_t st) {
  const dim3 grid(pl.gx, pl.gy, pl.gz);
  switch (pl.kernel) {
    case FWD_F32_128x128: case FWD_F32IN_128x128: launch_fwd_128x128(pl, p, grid, st); break;
    case FWD_F32_128x64: case FWD_F32IN_128x64: launch_fwd_128x64(pl, p, grid, st); break;
    case FWD_F32_128x32: case FWD_F32IN_128x32: launch_fwd_128x32(pl, p, grid, st); break;
    case FWD_F32_96x128: case FWD_F32IN_96x128: launch_fwd_96x128(pl, p, grid, st); break;
    case FWD_SPLIT_128x128: case FWD_SPLIT_128x64: case FWD_SPLIT_128x32: launch_fwd_split(pl, p, grid, st); break;
    default: S2I_FAIL("igemm_fwd: kernel %d is no matrix kernel", (int)pl.kernel);
  }
  S2I_LAUNCH_CHECK("igemm_fwd");
  return 0;
}

int launch_small_n_conv(const FwdPlan& pl, const IgemmP& p, hipStream_t st) {
  const dim3 grid(pl.gx, pl.gy, pl.gz);
  const size_t shb = (size_t)pl.T * pl.Ca * 4 * sizeof(float);
  if (pl.kernel == FWD_SMALLN_4) hipLaunchKernelGGL((small_n_conv_kernel<4>), grid, dim3(256), shb, st, p);
  else if (pl.kernel == FWD_SMALLN_8) hipLaunchKernelGGL((small_n_conv_kernel<8>), grid, dim3(256), shb, st, p);
  else hipLaunchKernelGGL((small_n_conv_kernel<16>), grid, dim3(256), shb, st, p);
  S2I_LAUNCH_CHECK("small_n_conv");
  return 0;
}

int launch_splitk_reduce(const s2i_conv_desc* d, const FwdPlan& pl, const float* bias, float* y, float* part, void* ws,
                         int y16, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (pl.reduce == FWD_REDUCE_STATS) {
    const int Q = d->N / 4;
    int cpb = 1;
    while (cpb < Q && cpb < 256) cpb <<= 1;
    const int groups = d->groups < 1 ? 1 : d->groups;
    const int nparts = stat_parts(pl, groups);
    hipLaunchKernelGGL(splitk_reduce_stats_kernel, dim3(nparts, (Q + cpb - 1) / cpb), dim3(256), 0, st,
                       (const float*)ws, pl.splitk, pl.Mrows, d->N, y, d->ldy, part, nparts, cpb, nparts / groups,
                       pl.Mrows / groups, y16);
    S2I_LAUNCH_CHECK("splitk_reduce_stats");
    return 0;
  }
  const long long total = pl.Mrows * d->N;
  int blocks = s2i_cdiv(total, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const float*)ws, pl.splitk,
                     pl.Mrows, d->N, bias, d->act, y, d->ldy, y16);
  S2I_LAUNCH_CHECK("splitk_reduce");
  if (pl.reduce == FWD_REDUCE_COLSTATS) return s2i_colstats(y, pl.Mrows, d->N, d->ldy, part, stat_parts(pl, 1), stream);
  return 0;
}

extern "C" int s2i_split_packed_weight(const float* packed, int T, int R, int C, int planes, unsigned short* out_rc,
                                       unsigned short* out_cr, void* stream) {
  S2I_REQUIRE(packed && (out_rc || out_cr) && T > 0 && R > 0 && C > 0 && planes >= 1 && planes <= 3,
              "split_packed_weight: bad args");
  dim3 grid(s2i_cdiv(C, 32), s2i_cdiv(R, 32), T);
  hipLaunchKernelGGL(split_packed_kernel, grid, dim3(256), 0, (hipStream_t)stream, packed, out_rc, out_cr, R, C, planes,
                     (long long)T * R * C);
  S2I_LAUNCH_CHECK("split_packed_weight");
  return 0;
}
