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

// splitk_reduce_kernel for N % 4 == 0 && ldy % 4 == 0: one column quad per thread and turn, 16-byte loads and stores, the
// (row, column) of the quad carried from turn to turn (srow, scol = the grid's stride in rows and columns).  Per element
// the same chain: 0 + slab0 + slab1 ..., bias, activation.
__global__ __launch_bounds__(256) void splitk_reduce_v4_kernel(const float* __restrict__ slab, int S, long long rows, int N,
                                                               const float* __restrict__ bias, int act,
                                                               float* __restrict__ y, int ldy, int y16, long long srow,
                                                               int scol) {
  const long long total = rows * N;
  const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (e0 >= total) return;
  long long row = e0 / N;
  int n = (int)(e0 - row * N);
  for (; row < rows;) {
    const float* sp = slab + row * N + n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) v += *reinterpret_cast<const f32x4*>(sp + (size_t)s * total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = v[j];
      if (bias) t += bias[n + j];
      if (act == S2I_ACT_LRELU) t = t > 0.f ? t : 0.2f * t;
      else if (act == S2I_ACT_TANH) t = tanhf(t);
      else if (act == S2I_ACT_RELU) t = fmaxf(t, 0.f);
      v[j] = t;
    }
    if (y16) {
      unsigned short* yp = reinterpret_cast<unsigned short*>(y) + row * ldy + n;
      *reinterpret_cast<u32x2_t*>(yp) = u32x2_t{(unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16),
                                               (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16)};
    } else {
      *reinterpret_cast<f32x4*>(y + row * ldy + n) = v;
    }
    row += srow;
    n += scol;
    if (n >= N) { n -= N; ++row; }
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

// The same reduction for cpb >= 32 (N > 64), spread over the chip: a block owns QB column quads of one row chunk, its 256
// threads are QB quads x 256 / QB row workers that load, sum over the slabs and store y for 512 / QB rows per turn (two
// each), and hand the sums through LDS to the QB x rpb threads that own the statistics (QB = 32, 16 rows per turn, for row
// chunks of at most 16 rows; 16 otherwise).  Those walk the rows as the kernel above does (rpb = 256 / cpb row lanes per
// quad, rows r0 + lane, + rpb, ...; then lanes 1 .. rpb-1 onto lane 0), so y and part come out bit for bit the same.  The
// first two slabs of the next turn are loaded before the walk and summed after it.
constexpr int RS_AHEAD = 2;
template <int RS_QB>
__global__ __launch_bounds__(256) void splitk_reduce_stats_wide_kernel(const float* __restrict__ slab, int S,
                                                                       long long rows, int N, float* __restrict__ y,
                                                                       int ldy, float* __restrict__ part, int nparts,
                                                                       int rpb, int ppg, long long Rg, int y16) {
  constexpr int RS_RW = 256 / RS_QB, RS_ROWS = 2 * RS_RW;
  __shared__ f32x4 vt[RS_ROWS][RS_QB];       // 8 KB: the turn's sums over the slabs
  __shared__ f32x4 sh[2][8 * RS_QB];         // 4 or 8 KB: the row lanes' statistics (rpb <= 8)
  const int tid = threadIdx.x;
  const int ql = tid % RS_QB, rw = tid / RS_QB;
  const int quad = blockIdx.y * RS_QB + ql;
  const int Q = N / 4;
  const int grp = blockIdx.x / ppg, pp = blockIdx.x - grp * ppg;  // BatchNorm group of this row chunk
  const long long chunk = (Rg + ppg - 1) / ppg;
  const long long r0 = grp * Rg + pp * chunk;
  const long long gend = (grp + 1) * Rg < rows ? (grp + 1) * Rg : rows;
  const long long r1 = r0 + chunk < gend ? r0 + chunk : gend;
  const size_t sstride = (size_t)rows * N;
  const bool colok = quad < Q;
  const bool owner = tid < RS_QB * rpb && colok;  // (quad ql, row lane rw) of the statistics
  const int ahead = S < RS_AHEAD ? S : RS_AHEAD;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  f32x4 t[2][RS_AHEAD];
  auto issue = [&](long long base) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long row = base + rw + h * RS_RW;
      if (colok && row < r1) {
        const float* sp = slab + row * N + quad * 4;
#pragma unroll
        for (int k = 0; k < RS_AHEAD; ++k)
          if (k < ahead) t[h][k] = *reinterpret_cast<const f32x4*>(sp + k * sstride);
      }
    }
  };
  if (r0 < r1) issue(r0);
  for (long long base = r0; base < r1; base += RS_ROWS) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long row = base + rw + h * RS_RW;
      if (colok && row < r1) {
        const float* sp = slab + row * N + quad * 4;
        f32x4 v = t[h][0];
#pragma unroll
        for (int k = 1; k < RS_AHEAD; ++k)
          if (k < ahead) v += t[h][k];
        for (int s = RS_AHEAD; s < S; ++s) v += *reinterpret_cast<const f32x4*>(sp + s * sstride);
        if (y16) {
          unsigned short* yp = reinterpret_cast<unsigned short*>(y) + row * ldy + quad * 4;
          *reinterpret_cast<u32x2_t*>(yp) = u32x2_t{(unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16),
                                                   (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16)};
        } else {
          *reinterpret_cast<f32x4*>(y + row * ldy + quad * 4) = v;
        }
        vt[rw + h * RS_RW][ql] = v;
      }
    }
    __syncthreads();
    if (base + RS_ROWS < r1) issue(base + RS_ROWS);
    if (owner) {
      const long long left = r1 - base;
      const int jend = left < RS_ROWS ? (int)left : RS_ROWS;
      for (int j = rw; j < jend; j += rpb) {  // RS_ROWS % rpb == 0: lane rw's rows of the chunk, in their order
        const f32x4 v = vt[j][ql];
        s0 += v;
        s1 += v * v;
      }
    }
    __syncthreads();
  }
  if (owner) {
    sh[0][tid] = s0;
    sh[1][tid] = s1;
  }
  __syncthreads();
  if (rw == 0 && colok) {
    for (int r = 1; r < rpb; ++r) {
      s0 += sh[0][r * RS_QB + ql];
      s1 += sh[1][r * RS_QB + ql];
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
    // cpb fixes the statistics' summation order (256 / cpb row lanes per quad) in both kernels; the wide one only spreads
    // the loads over more blocks
    const int ppg = nparts / groups;
    const long long Rg = pl.Mrows / groups;
    if (cpb >= 32 && s2i_cdiv(Rg, ppg) <= 16)
      hipLaunchKernelGGL(splitk_reduce_stats_wide_kernel<32>, dim3(nparts, (Q + 31) / 32), dim3(256), 0, st,
                         (const float*)ws, pl.splitk, pl.Mrows, d->N, y, d->ldy, part, nparts, 256 / cpb, ppg, Rg, y16);
    else if (cpb >= 32)
      hipLaunchKernelGGL(splitk_reduce_stats_wide_kernel<16>, dim3(nparts, (Q + 15) / 16), dim3(256), 0, st,
                         (const float*)ws, pl.splitk, pl.Mrows, d->N, y, d->ldy, part, nparts, 256 / cpb, ppg, Rg, y16);
    else
      hipLaunchKernelGGL(splitk_reduce_stats_kernel, dim3(nparts, (Q + cpb - 1) / cpb), dim3(256), 0, st,
                         (const float*)ws, pl.splitk, pl.Mrows, d->N, y, d->ldy, part, nparts, cpb, nparts / groups,
                         pl.Mrows / groups, y16);
    S2I_LAUNCH_CHECK("splitk_reduce_stats");
    return 0;
  }
  const long long total = pl.Mrows * d->N;
  if ((d->N & 3) == 0 && (d->ldy & 3) == 0) {
    int blocks = s2i_cdiv(total / 4, 256);
    if (blocks > 2048) blocks = 2048;
    const long long stride = (long long)blocks * 256 * 4;
    hipLaunchKernelGGL(splitk_reduce_v4_kernel, dim3(blocks), dim3(256), 0, st, (const float*)ws, pl.splitk, pl.Mrows,
                       d->N, bias, d->act, y, d->ldy, y16, stride / d->N, (int)(stride % d->N));
  } else {
    int blocks = s2i_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const float*)ws, pl.splitk,
                       pl.Mrows, d->N, bias, d->act, y, d->ldy, y16);
  }
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
