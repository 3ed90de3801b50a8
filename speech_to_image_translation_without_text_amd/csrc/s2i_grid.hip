// The snapshot image grid on gfx950 (StackGAN_v2/trainer.py:268-295: vutils.save_image(..., normalize=True)): min-max
// normalise a batch of three-channel fp32 images with ONE (lo, hi) pair, tile them nrow to a line with `padding` black
// pixels around every cell, and quantise to uint8 HWC.  Two launches on the caller's stream, no host round trip between
// them: the reduction leaves per-block (lo, hi) partials in the caller's workspace, and every block of the composition
// re-reduces those few hundred pairs before it writes one output pixel per thread (3-byte stores of consecutive lanes
// are consecutive in memory).  min and max do not depend on the order they are taken in, so the bytes do not depend on
// the block count.
#include "s2i_elementwise.h"
#include <limits.h>

namespace {

constexpr int GRID_PARTS = 512;      // most reduction blocks = most (lo, hi) partials in the workspace
constexpr int GRID_THREADS = 256;

struct GridSrc {
  const float* p;
  int N, H, W;
  long long sn, sy, sx, sc;          // element strides of image, row, column, channel
};

// (lo, hi) of the block's 256 threads in every thread: 64-lane shuffles, then the four waves through LDS
__device__ __forceinline__ void grid_block_minmax(float& lo, float& hi) {
  __shared__ float sh[2 * (GRID_THREADS / 64)];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, 64));
    hi = fmaxf(hi, __shfl_down(hi, off, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[2 * wave] = lo;
    sh[2 * wave + 1] = hi;
  }
  __syncthreads();
  lo = sh[0];
  hi = sh[1];
#pragma unroll
  for (int w = 1; w < GRID_THREADS / 64; ++w) {
    lo = fminf(lo, sh[2 * w]);
    hi = fmaxf(hi, sh[2 * w + 1]);
  }
}

// partials[2b] / partials[2b + 1] = min / max over the pixels block b strides over (every block has at least one)
__global__ __launch_bounds__(GRID_THREADS) void grid_minmax_kernel(GridSrc s, float* __restrict__ partials) {
  const long long HW = (long long)s.H * s.W, npix = (long long)s.N * HW;
  float lo = INFINITY, hi = -INFINITY;
  for (long long e = (long long)blockIdx.x * GRID_THREADS + threadIdx.x; e < npix;
       e += (long long)gridDim.x * GRID_THREADS) {
    const long long n = e / HW, r = e - n * HW;
    const int y = (int)(r / s.W), x = (int)(r - (long long)y * s.W);
    const float* px = s.p + n * s.sn + y * s.sy + x * s.sx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = px[c * s.sc];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  grid_block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = lo;
    partials[2 * blockIdx.x + 1] = hi;
  }
}

// (x - lo) / d * 255 + 0.5, clamped and truncated, every operation rounded on its own.  hipcc contracts a multiply and
// an add into one v_fma_f32 by default, through __fmul_rn / __fadd_rn as well (they are plain operators in HIP), and a
// float32 restatement then disagrees where v * 255 + 0.5 lies next to an integer: contraction is switched off for this
// function.  The division is the IEEE sequence (v_div_scale / v_div_fmas / v_div_fixup), hipcc's default for fp32.
__device__ __forceinline__ unsigned char grid_quantise(float x, float lo, float d) {
#pragma clang fp contract(off)
  const float v = (x - lo) / d;
  float q = v * 255.f;
  q = q + 0.5f;
  q = fminf(fmaxf(q, 0.f), 255.f);
  return (unsigned char)q;
}

// one output pixel per thread: d = max(hi - lo, 1e-5), then grid_quantise per channel
__global__ __launch_bounds__(GRID_THREADS) void grid_compose_kernel(GridSrc s, const float* __restrict__ partials,
                                                                    int nparts, int xmaps, int padding, int Hg, int Wg,
                                                                    unsigned char* __restrict__ dst) {
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nparts; i += GRID_THREADS) {
    lo = fminf(lo, partials[2 * i]);
    hi = fmaxf(hi, partials[2 * i + 1]);
  }
  grid_block_minmax(lo, hi);
  const float d = fmaxf(hi - lo, 1e-5f);
  const int ch = s.H + padding, cw = s.W + padding;
  const long long total = (long long)Hg * Wg;
  for (long long e = (long long)blockIdx.x * GRID_THREADS + threadIdx.x; e < total;
       e += (long long)gridDim.x * GRID_THREADS) {
    const int gy = (int)(e / Wg), gx = (int)(e - (long long)gy * Wg);
    const int ry = gy - padding, rx = gx - padding;
    unsigned char out[3] = {0, 0, 0};
    if (ry >= 0 && rx >= 0) {
      const int cy = ry / ch, iy = ry - cy * ch;
      const int cx = rx / cw, ix = rx - cx * cw;
      const long long k = (long long)cy * xmaps + cx;
      if (iy < s.H && ix < s.W && cx < xmaps && k < s.N) {
        const float* px = s.p + k * s.sn + iy * s.sy + ix * s.sx;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = grid_quantise(px[c * s.sc], lo, d);
      }
    }
    dst[e * 3 + 0] = out[0];
    dst[e * 3 + 1] = out[1];
    dst[e * 3 + 2] = out[2];
  }
}

}  // namespace

extern "C" size_t s2i_image_grid_workspace_bytes(void) { return (size_t)GRID_PARTS * 2 * sizeof(float); }

extern "C" int s2i_image_grid_u8(const float* src, int N, int H, int W, long long stride_n, long long stride_y,
                                 long long stride_x, long long stride_c, int nrow, int padding, float* workspace,
                                 unsigned char* dst, void* stream) {
  S2I_REQUIRE(src && workspace && dst, "image_grid_u8: null pointer");
  S2I_REQUIRE(N > 0 && H > 0 && W > 0, "image_grid_u8: bad batch %d x %d x %d", N, H, W);
  S2I_REQUIRE(nrow > 0 && padding >= 0, "image_grid_u8: bad nrow %d / padding %d", nrow, padding);
  const int xmaps = nrow < N ? nrow : N;
  const int ymaps = (N + xmaps - 1) / xmaps;
  const long long Hg = (long long)ymaps * ((long long)H + padding) + padding;
  const long long Wg = (long long)xmaps * ((long long)W + padding) + padding;
  S2I_REQUIRE(Hg <= INT_MAX && Wg <= INT_MAX, "image_grid_u8: grid of %lld x %lld pixels is too large", Hg, Wg);
  const GridSrc s = {src, N, H, W, stride_n, stride_y, stride_x, stride_c};
  const int nparts = grid_for((long long)N * H * W, GRID_THREADS, GRID_PARTS);
  hipLaunchKernelGGL(grid_minmax_kernel, dim3(nparts), dim3(GRID_THREADS), 0, ST, s, workspace);
  S2I_LAUNCH_CHECK("image_grid_u8 (min / max)");
  hipLaunchKernelGGL(grid_compose_kernel, dim3(grid_for(Hg * Wg, GRID_THREADS, 2048)), dim3(GRID_THREADS), 0, ST, s,
                     (const float*)workspace, nparts, xmaps, padding, (int)Hg, (int)Wg, dst);
  S2I_LAUNCH_CHECK("image_grid_u8 (compose)");
  return 0;
}
