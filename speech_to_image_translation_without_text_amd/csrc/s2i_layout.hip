// Layout conversion and casts at the edges of the NHWC path on gfx950: NCHW fp32 <-> NHWC fp32 / bf16 (one element per
// thread; the 3 -> 4 channel image form stores 16 bytes per pixel), uint8 HWC images <-> normalised fp32, per-image
// column sums of an NHWC tensor (16 bytes per lane, two stages) and the fp32 <-> bf16 cast (four elements per thread).
#include "s2i_elementwise.h"

namespace {
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int B, int C, int HW,
                                    int Cp) {
  const long long total = (long long)B * HW * Cp;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % Cp);
    const long long bp = e / Cp;
    const int pix = (int)(bp % HW);
    const int b = (int)(bp / HW);
    st1(dst + e, c < C ? src[((long long)b * C + c) * HW + pix] : 0.f);
  }
}
// image fast path: C = 3 -> Cp = 4, one pixel per thread
__global__ void nchw3_to_nhwc4_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int HW) {
  const long long total = (long long)B * HW;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int pix = (int)(e % HW);
    const long long b = e / HW;
    const float* s = src + b * 3 * HW + pix;
    f32x4 v = {s[0], s[HW], s[2 * (long long)HW], 0.f};
    st4(dst + e * 4, v);
  }
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ src, int lds, float* __restrict__ dst, int B, int C,
                                    int HW) {
  const long long total = (long long)B * C * HW;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int pix = (int)(e % HW);
    const long long bc = e / HW;
    const int c = (int)(bc % C);
    const long long b = bc / C;
    dst[e] = ld1(src + (b * HW + pix) * lds + c);
  }
}
}  // namespace
extern "C" int s2i_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int Cp, void* stream) {
  S2I_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && Cp >= C, "nchw_to_nhwc: bad args");
  if (C == 3 && Cp == 4) {
    hipLaunchKernelGGL(nchw3_to_nhwc4_kernel, dim3(grid_for((long long)B * H * W)), dim3(256), 0, ST, src, dst, B,
                       H * W);
  } else {
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(grid_for((long long)B * H * W * Cp)), dim3(256), 0, ST, src, dst, B,
                       C, H * W, Cp);
  }
  S2I_LAUNCH_CHECK("nchw_to_nhwc");
  return 0;
}
extern "C" int s2i_nhwc_to_nchw(const float* src, int lds, float* dst, int B, int C, int H, int W, void* stream) {
  S2I_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && lds >= C, "nhwc_to_nchw: bad args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(grid_for((long long)B * C * H * W)), dim3(256), 0, ST, src, lds, dst,
                     B, C, H * W);
  S2I_LAUNCH_CHECK("nhwc_to_nchw");
  return 0;
}
/* the same with the NHWC side stored as bf16 (the NCHW side stays fp32: the module boundary) */
extern "C" int s2i_nchw_to_nhwc_dt(int dtype, const float* src, void* dst, int B, int C, int H, int W, int Cp, void* stream) {
  S2I_DT_CHECK(dtype, "nchw_to_nhwc");
  if (dtype == S2I_DT_F32) return s2i_nchw_to_nhwc(src, (float*)dst, B, C, H, W, Cp, stream);
  S2I_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && Cp >= C, "nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, dim3(grid_for((long long)B * H * W * Cp)), dim3(256), 0, ST, src,
                     (bf16_t*)dst, B, C, H * W, Cp);
  S2I_LAUNCH_CHECK("nchw_to_nhwc");
  return 0;
}
extern "C" int s2i_nhwc_to_nchw_dt(int dtype, const void* src, int lds, float* dst, int B, int C, int H, int W, void* stream) {
  S2I_DT_CHECK(dtype, "nhwc_to_nchw");
  if (dtype == S2I_DT_F32) return s2i_nhwc_to_nchw((const float*)src, lds, dst, B, C, H, W, stream);
  S2I_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && lds >= C, "nhwc_to_nchw: bad args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3(grid_for((long long)B * C * H * W)), dim3(256), 0, ST,
                     (const bf16_t*)src, lds, dst, B, C, H * W);
  S2I_LAUNCH_CHECK("nhwc_to_nchw");
  return 0;
}

namespace {
__global__ void image_to_u8_kernel(const float* __restrict__ src, int lds, unsigned char* __restrict__ dst,
                                   long long npix) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < npix;
       e += (long long)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = ((src[e * lds + c] + 1.f) / 2.f) * 255.f;
      v = fminf(fmaxf(v, 0.f), 255.f);
      dst[e * 3 + c] = (unsigned char)v;  // .byte(): truncation
    }
  }
}

// HWC uint8 -> normalised NCHW float: consecutive threads take consecutive pixels, so the 3-byte reads and the three
// plane writes are all coalesced
__global__ void u8_to_image_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int HW,
                                   long long npix) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < npix;
       e += (long long)gridDim.x * blockDim.x) {
    const long long b = e / HW;
    const long long r = e - b * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = (float)src[e * 3 + c] / 255.f;          // ToTensor
      dst[(b * 3 + c) * HW + r] = (t - 0.5f) / 0.5f;          // Normalize
    }
  }
}
}  // namespace
extern "C" int s2i_image_to_u8(const float* src, int lds, unsigned char* dst, long long npix, void* stream) {
  S2I_REQUIRE(src && dst && lds >= 3 && npix > 0, "image_to_u8: bad args");
  hipLaunchKernelGGL(image_to_u8_kernel, dim3(grid_for(npix)), dim3(256), 0, ST, src, lds, dst, npix);
  S2I_LAUNCH_CHECK("image_to_u8");
  return 0;
}

extern "C" int s2i_u8_to_image(const unsigned char* src, float* dst, int B, int H, int W, void* stream) {
  S2I_REQUIRE(src && dst && B > 0 && H > 0 && W > 0, "u8_to_image: bad args");
  const long long npix = (long long)B * H * W;
  hipLaunchKernelGGL(u8_to_image_kernel, dim3(grid_for(npix)), dim3(256), 0, ST, src, dst, H * W, npix);
  S2I_LAUNCH_CHECK("u8_to_image");
  return 0;
}

namespace {
// per-image column sums, two stages: [B][S][C] partials then the S-sum
template <typename T>
__global__ __launch_bounds__(256) void spatial_sum_stage1(const T* __restrict__ src, int ld, int HW, int C,
                                                          int S, float* __restrict__ tmp, int cpb) {
  __shared__ f32x4 sh[256];
  const int tid = threadIdx.x;
  const int rpb = 256 / cpb;
  const int ql = tid % cpb, rl = tid / cpb;
  const int quad = blockIdx.z * cpb + ql;
  const int Q = C / 4;
  const int b = blockIdx.x, sidx = blockIdx.y;
  const int chunk = (HW + S - 1) / S;
  const int r0 = sidx * chunk, r1 = min(HW, r0 + chunk);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (quad < Q)
    for (int r = r0 + rl; r < r1; r += rpb) acc += ld4(src + ((long long)b * HW + r) * ld + quad * 4);
  sh[tid] = acc;
  __syncthreads();
  if (rl == 0 && quad < Q) {
    for (int r = 1; r < rpb; ++r) acc += sh[r * cpb + ql];
    st4(tmp + ((size_t)b * S + sidx) * C + quad * 4, acc);
  }
}
__global__ void spatial_sum_stage2(const float* __restrict__ tmp, int B, int S, int C, float* __restrict__ dst) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * C) return;
  const int b = e / C, c = e - b * C;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += tmp[((size_t)b * S + s) * C + c];
  dst[e] = v;
}
}  // namespace
static int spatial_segments(int HW) {
  int S = HW / 64;
  if (S > 64) S = 64;
  if (S < 1) S = 1;
  return S;
}
extern "C" size_t s2i_spatial_sum_workspace_bytes(int B, int HW, int C) {
  return (size_t)B * spatial_segments(HW) * C * sizeof(float);
}
template <typename T>
static int spatial_sum_impl(const T* src, int ld, int B, int HW, int C, float* dst, void* ws, size_t ws_bytes,
                            void* stream) {
  S2I_REQUIRE(src && dst && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && ld % 4 == 0 && ld >= C,
              "spatial_sum: bad args");
  const int S = spatial_segments(HW);
  S2I_REQUIRE(ws && ws_bytes >= (size_t)B * S * C * sizeof(float), "spatial_sum: workspace too small");
  RedGeom g = red_geom(C);
  hipLaunchKernelGGL(spatial_sum_stage1<T>, dim3(B, S, g.gy), dim3(256), 0, ST, src, ld, HW, C, S, (float*)ws, g.cpb);
  S2I_LAUNCH_CHECK("spatial_sum_stage1");
  hipLaunchKernelGGL(spatial_sum_stage2, dim3((B * C + 255) / 256), dim3(256), 0, ST, (const float*)ws, B, S, C, dst);
  S2I_LAUNCH_CHECK("spatial_sum_stage2");
  return 0;
}
extern "C" int s2i_spatial_sum(const float* src, int ld, int B, int HW, int C, float* dst, void* ws, size_t ws_bytes,
                               void* stream) {
  return spatial_sum_impl<float>(src, ld, B, HW, C, dst, ws, ws_bytes, stream);
}
extern "C" int s2i_spatial_sum_dt(int dtype, const void* src, int ld, int B, int HW, int C, float* dst, void* ws,
                                  size_t ws_bytes, void* stream) {
  S2I_DT_CHECK(dtype, "spatial_sum");
  if (dtype == S2I_DT_BF16) return spatial_sum_impl<bf16_t>((const bf16_t*)src, ld, B, HW, C, dst, ws, ws_bytes, stream);
  return spatial_sum_impl<float>((const float*)src, ld, B, HW, C, dst, ws, ws_bytes, stream);
}

namespace {
template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ src, D* __restrict__ dst, long long n4) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long long)gridDim.x * blockDim.x)
    st4(dst + e * 4, ld4(src + e * 4));
}
}  // namespace
/* element type conversion of a contiguous tensor: dst_dtype[n] = src_dtype[n] (n % 4 == 0) */
extern "C" int s2i_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long long n, void* stream) {
  S2I_DT_CHECK(src_dtype, "cast");
  S2I_DT_CHECK(dst_dtype, "cast");
  S2I_REQUIRE(src && dst && n > 0 && (n % 4) == 0 && src_dtype != dst_dtype, "cast: bad args");
  if (src_dtype == S2I_DT_F32)
    hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3(grid_for(n / 4)), dim3(256), 0, ST, (const float*)src, (bf16_t*)dst, n / 4);
  else
    hipLaunchKernelGGL((cast_kernel<bf16_t, float>), dim3(grid_for(n / 4)), dim3(256), 0, ST, (const bf16_t*)src, (float*)dst, n / 4);
  S2I_LAUNCH_CHECK("cast");
  return 0;
}
