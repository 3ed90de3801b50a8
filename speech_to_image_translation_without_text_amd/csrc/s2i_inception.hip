// Memory-bound pieces of the Inception-v3 scorer (StackGAN_v2/model.py:17-109): the input stage, the pools and the
// softmax.  The convolutions and the fc are s2i_conv2d_forward (s2i_conv2d.hip).  NHWC fp32 throughout.
#include "s2i_common.h"

namespace {

// one thread per output element (b, oy, ox, c)
__global__ __launch_bounds__(256) void pool_window_kernel(const float* __restrict__ x, float* __restrict__ y, int mode,
                                                          int H, int W, int C, int ldx, int Ho, int Wo, int ldy, int coff,
                                                          long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long pix = idx / C;
  const int ox = (int)(pix % Wo);
  const long long t = pix / Wo;
  const int oy = (int)(t % Ho);
  const int b = (int)(t / Ho);
  const float* xb = x + (size_t)b * H * W * ldx + c;
  float v;
  if (mode == S2I_POOL_MAX3S2) {
    v = -INFINITY;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) v = fmaxf(v, xb[((size_t)(2 * oy + ky) * W + 2 * ox + kx) * ldx]);
  } else {
    float s = 0.f;
    for (int ky = -1; ky <= 1; ++ky) {
      const int iy = oy + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = -1; kx <= 1; ++kx) {
        const int ix = ox + kx;
        if (ix >= 0 && ix < W) s += xb[((size_t)iy * W + ix) * ldx];
      }
    }
    v = s / 9.f;   // count_include_pad=True
  }
  y[pix * ldy + coff + c] = v;
}

// one thread per (b, c): the mean over the H x W map
__global__ __launch_bounds__(256) void pool_global_kernel(const float* __restrict__ x, float* __restrict__ y, int HW, int C,
                                                          int ldx, int ldy, int coff, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = idx % C, b = idx / C;
  const float* xb = x + (size_t)b * HW * ldx + c;
  float s = 0.f;
  for (int p = 0; p < HW; ++p) s += xb[(size_t)p * ldx];
  y[(size_t)b * ldy + coff + c] = s / (float)HW;
}

// one thread per output pixel: [-1, 1] -> [0, 1] -> ImageNet normalisation -> bilinear (align_corners=False) -> NHWC.
// The normalisation is applied to each source value before the interpolation, in the order of model.py:95-104, and the
// interpolation is upsample_bilinear2d's expression.
__global__ __launch_bounds__(256) void inception_prep_kernel(const float* __restrict__ img, int Hin, int Win, long long sb,
                                                             long long sc, long long sh, long long sw, float* __restrict__ y,
                                                             int S, int Cy, float rh, float rw, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = idx % S, t = idx / S, oy = t % S, b = t / S;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  float fy = rh * (oy + 0.5f) - 0.5f, fx = rw * (ox + 0.5f) - 0.5f;
  fy = fy < 0.f ? 0.f : fy;
  fx = fx < 0.f ? 0.f : fx;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < Hin - 1 ? 1 : 0), x1 = x0 + (x0 < Win - 1 ? 1 : 0);
  const float ly1 = fy - y0, ly0 = 1.f - ly1, lx1 = fx - x0, lx0 = 1.f - lx1;
  float* out = y + (size_t)idx * Cy;
  for (int c = 0; c < 3; ++c) {
    const float* p = img + b * sb + c * sc;
    auto at = [&](int yy, int xx) { return (fmaf(p[yy * sh + xx * sw], 0.5f, 0.5f) - mean[c]) / stdv[c]; };
    out[c] = ly0 * (lx0 * at(y0, x0) + lx1 * at(y0, x1)) + ly1 * (lx0 * at(y1, x0) + lx1 * at(y1, x1));
  }
  if (Cy == 4) out[3] = 0.f;
}

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  for (int o = 32; o > 0; o >>= 1) {
    const float u = __shfl_xor(v, o);
    v = is_max ? fmaxf(v, u) : v + u;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  v = red[0];
  for (int i = 1; i < 4; ++i) v = is_max ? fmaxf(v, red[i]) : v + red[i];
  return v;
}

// one block of 256 threads per row
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, int cols, int ldx,
                                                           float* __restrict__ y, int ldy) {
  __shared__ float red[4];
  const float* xr = x + (size_t)blockIdx.x * ldx;
  float* yr = y + (size_t)blockIdx.x * ldy;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < cols; i += 256) m = fmaxf(m, xr[i]);
  m = block_reduce(m, red, true);
  float s = 0.f;
  for (int i = threadIdx.x; i < cols; i += 256) s += expf(xr[i] - m);
  s = block_reduce(s, red, false);
  const float inv = 1.f / s;
  for (int i = threadIdx.x; i < cols; i += 256) yr[i] = expf(xr[i] - m) * inv;
}

}  // namespace

extern "C" int s2i_pool2d(int mode, const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy, int coff,
                          void* stream) {
  S2I_REQUIRE(x && y, "pool2d: null pointer");
  S2I_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && ldx >= C && coff >= 0 && ldy >= coff + C,
              "pool2d: bad shape (B %d, H %d, W %d, C %d, ldx %d, ldy %d, coff %d)", B, H, W, C, ldx, ldy, coff);
  hipStream_t st = (hipStream_t)stream;
  if (mode == S2I_POOL_GLOBAL) {
    const int total = B * C;
    hipLaunchKernelGGL(pool_global_kernel, dim3(s2i_cdiv(total, 256)), dim3(256), 0, st, x, y, H * W, C, ldx, ldy, coff,
                       total);
  } else {
    S2I_REQUIRE(mode == S2I_POOL_MAX3S2 || mode == S2I_POOL_AVG3S1, "pool2d: unknown mode %d", mode);
    S2I_REQUIRE(mode != S2I_POOL_MAX3S2 || (H >= 3 && W >= 3), "pool2d: a 3x3 max pool needs H, W >= 3");
    const int Ho = mode == S2I_POOL_MAX3S2 ? (H - 3) / 2 + 1 : H;
    const int Wo = mode == S2I_POOL_MAX3S2 ? (W - 3) / 2 + 1 : W;
    const long long total = (long long)B * Ho * Wo * C;
    hipLaunchKernelGGL(pool_window_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, y, mode, H, W, C,
                       ldx, Ho, Wo, ldy, coff, total);
  }
  S2I_LAUNCH_CHECK("pool2d");
  return 0;
}

extern "C" int s2i_inception_prep(const float* img, int B, int Hin, int Win, long long sb, long long sc, long long sh,
                                  long long sw, float* y, int S, int Cy, void* stream) {
  S2I_REQUIRE(img && y, "inception_prep: null pointer");
  S2I_REQUIRE(B >= 1 && Hin >= 1 && Win >= 1 && S >= 1 && (Cy == 3 || Cy == 4), "inception_prep: bad shape");
  const long long total = (long long)B * S * S;
  S2I_REQUIRE(total * Cy < (1LL << 31), "inception_prep: output too large: split the batch");
  hipLaunchKernelGGL(inception_prep_kernel, dim3(s2i_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, img, Hin, Win,
                     sb, sc, sh, sw, y, S, Cy, (float)Hin / (float)S, (float)Win / (float)S, (int)total);
  S2I_LAUNCH_CHECK("inception_prep");
  return 0;
}

extern "C" int s2i_softmax_rows(const float* x, int rows, int cols, int ldx, float* y, int ldy, void* stream) {
  S2I_REQUIRE(x && y, "softmax_rows: null pointer");
  S2I_REQUIRE(rows >= 1 && cols >= 1 && ldx >= cols && ldy >= cols, "softmax_rows: bad shape");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, cols, ldx, y, ldy);
  S2I_LAUNCH_CHECK("softmax_rows");
  return 0;
}
