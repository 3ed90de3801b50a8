// Differentiable augmentation of discriminator inputs on gfx950, fused into the image layout conversion: colour
// (brightness, saturation, contrast), translation and cutout (Zhao et al. 2020) applied while NCHW fp32 images become
// NHWC4, and the exact adjoint applied while the NHWC gradient becomes NCHW.  Per direction: one per-image reduction (only
// with the colour stage: the raw image's sum forward, the masked gradient's sum backward) and one apply launch that
// converts the layout itself; no augmented NCHW image exists in either direction.  The NHWC side is whole pixels, 16-byte
// (fp32) or 8-byte (bf16) units wherever a row stride of 4 elements allows it, and takes vector accesses in both directions.
// Forward, the translation moves the NCHW reads by `tx` floats, which breaks their 16-byte alignment: one pixel per thread,
// coalesced 4-byte reads, an aligned 16-byte store.  Backward, dx is written unshifted: four pixels per thread where the
// side is a multiple of 4, four pixel loads and one aligned 16-byte store per plane.
// Reductions run in a fixed order (a lane's strided partial, an xor tree over the wave, the four waves in order, then an
// xor tree over the per-segment partials): no atomics, the same bits on every run.
#include "s2i_elementwise.h"
#include <stdint.h>

namespace {
struct AugGeom {
  int H, HW;
  int shift;  // S = int(H / 8 + 0.5): translations are drawn from [-S, S]
  int nt;     // 2 S + 1
  int cut;    // c = int(H / 2 + 0.5): side of the cutout window
  int nc;     // H + 1 - c % 2 window positions per axis
  int segs;   // blocks per image of a reduction (<= 64)
};

struct AugImage {
  float b, s, k;           // brightness offset, saturation and contrast factors
  int tx, ty;              // out[r][q] = z[r + ty][q + tx]
  int r0, r1, q0, q1;      // the cutout window in output coordinates, clipped to the image (empty: all 0)
};

__device__ __forceinline__ int aug_draw(float u, int n) {
  const int v = (int)(u * (float)n);  // one fp32 multiply, truncated
  return max(0, min(v, n - 1));
}

__device__ __forceinline__ AugImage aug_image(const float* __restrict__ row, int policy, const AugGeom& g) {
  AugImage a = {0.f, 1.f, 1.f, 0, 0, 0, 0, 0, 0};
  if (policy & S2I_DIFFAUG_COLOR) {
    a.b = row[0] - 0.5f;
    a.s = 2.f * row[1];
    a.k = row[2] + 0.5f;
  }
  if (policy & S2I_DIFFAUG_TRANSLATION) {
    a.tx = aug_draw(row[3], g.nt) - g.shift;
    a.ty = aug_draw(row[4], g.nt) - g.shift;
  }
  if (policy & S2I_DIFFAUG_CUTOUT) {
    const int ox = aug_draw(row[5], g.nc), oy = aug_draw(row[6], g.nc);
    a.r0 = max(0, oy - g.cut / 2);
    a.r1 = min(g.H, oy - g.cut / 2 + g.cut);
    a.q0 = max(0, ox - g.cut / 2);
    a.q1 = min(g.H, ox - g.cut / 2 + g.cut);
  }
  return a;
}

// whether output pixel (r, q) takes a value: its source (r + ty, q + tx) lies inside the image and the cutout spares it
__device__ __forceinline__ bool aug_live(const AugImage& a, const AugGeom& g, int r, int q) {
  const bool inside = (unsigned)(r + a.ty) < (unsigned)g.H && (unsigned)(q + a.tx) < (unsigned)g.H;
  const bool cut = r >= a.r0 && r < a.r1 && q >= a.q0 && q < a.q1;
  return inside && !cut;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the 256 threads of a block, the same bits in every thread; `sh` holds 4 floats and is free again on return
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return v;
}

// the image's total from its `segs` partial sums (wave 0 adds them; every thread gets the result)
__device__ __forceinline__ float image_total(const float* __restrict__ part, int segs, float* sh) {
  if (threadIdx.x < 64) {
    const float v = wave_sum((int)threadIdx.x < segs ? part[threadIdx.x] : 0.f);
    if (threadIdx.x == 0) sh[0] = v;
  }
  __syncthreads();
  const float t = sh[0];
  __syncthreads();
  return t;
}

template <typename T, bool VEC>
__device__ __forceinline__ void load_rgb(const T* __restrict__ p, float& g0, float& g1, float& g2) {
  if constexpr (VEC) {
    const f32x4 v = ld4(p);
    g0 = v[0], g1 = v[1], g2 = v[2];
  } else {
    g0 = ld1(p), g1 = ld1(p + 1), g2 = ld1(p + 2);
  }
}

// part[n][seg] = the sum of segment `seg` of image n's 3 H W raw values (n4 = 3 H W / 4 sixteen-byte loads per image)
__global__ __launch_bounds__(256) void diffaug_image_sum_kernel(const float* __restrict__ x, int N, int n4, int segs,
                                                                float* __restrict__ part) {
  __shared__ float sh[4];
  const int chunk = (n4 + segs - 1) / segs;
  const int i0 = blockIdx.x * chunk, i1 = min(n4, i0 + chunk);
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float* p = x + (long long)n * n4 * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) acc += ld4(p + (long long)i * 4);
    const float v = block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]), sh);
    if (threadIdx.x == 0) part[(long long)n * segs + blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(256) void diffaug_forward_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                              int policy, float* __restrict__ y, int N, AugGeom g,
                                                              const float* __restrict__ part) {
  __shared__ float sh[4];
  const int H = g.H, HW = g.HW;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const AugImage a = aug_image(table + (long long)n * 8, policy, g);
    float mb = 0.f;  // the mean the contrast stage turns about: the raw image's mean moved by the brightness offset
    if (policy & S2I_DIFFAUG_COLOR) mb = image_total(part + (long long)n * g.segs, g.segs, sh) / (float)(3 * HW) + a.b;
    const float* xn = x + (long long)n * 3 * HW;
    float* yn = y + (long long)n * HW * 4;
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < HW; pix += gridDim.x * 256) {
      const int r = pix / H, q = pix - r * H;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (aug_live(a, g, r, q)) {
        const float* s = xn + (r + a.ty) * H + (q + a.tx);
        float x0 = s[0], x1 = s[HW], x2 = s[2 * HW];
        if (policy & S2I_DIFFAUG_COLOR) {
          const float pb = (x0 + x1 + x2) / 3.f + a.b;
          x0 = ((x0 + a.b) - pb) * a.s + pb;
          x1 = ((x1 + a.b) - pb) * a.s + pb;
          x2 = ((x2 + a.b) - pb) * a.s + pb;
          x0 = (x0 - mb) * a.k + mb;
          x1 = (x1 - mb) * a.k + mb;
          x2 = (x2 - mb) * a.k + mb;
        }
        v = f32x4{x0, x1, x2, 0.f};
      }
      st4(yn + (long long)pix * 4, v);
    }
  }
}

// part[n][seg] = the sum, over segment `seg` of image n's output pixels that took a value, of dy's three channels
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void diffaug_grad_sum_kernel(const T* __restrict__ dy, int ld,
                                                               const float* __restrict__ table, int policy, int N,
                                                               AugGeom g, float* __restrict__ part) {
  __shared__ float sh[4];
  const int H = g.H, HW = g.HW;
  const int chunk = (HW + g.segs - 1) / g.segs;
  const int p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const AugImage a = aug_image(table + (long long)n * 8, policy, g);
    const T* dn = dy + (long long)n * HW * ld;
    float acc = 0.f;
    for (int pix = p0 + (int)threadIdx.x; pix < p1; pix += 256) {
      const int r = pix / H, q = pix - r * H;
      if (aug_live(a, g, r, q)) {
        float g0, g1, g2;
        load_rgb<T, VEC>(dn + (long long)pix * ld, g0, g1, g2);
        acc += (g0 + g1) + g2;
      }
    }
    const float v = block_sum(acc, sh);
    if (threadIdx.x == 0) part[(long long)n * g.segs + blockIdx.x] = v;
  }
}

// PX input pixels of one row per thread: 4 where the side is a multiple of 4 (each plane of dx then takes one aligned
// 16-byte store; dx is not shifted, only the pixels read from dy are), else 1
template <typename T, bool VEC, int PX>
__global__ __launch_bounds__(256) void diffaug_backward_kernel(const T* __restrict__ dy, int ld,
                                                               const float* __restrict__ table, int policy,
                                                               float* __restrict__ dx, int N, AugGeom g,
                                                               const float* __restrict__ part) {
  __shared__ float sh[4];
  const int H = g.H, HW = g.HW;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const AugImage a = aug_image(table + (long long)n * 8, policy, g);
    float gm = 0.f;  // mean of g_z over the image's 3 H W values
    if (policy & S2I_DIFFAUG_COLOR) gm = image_total(part + (long long)n * g.segs, g.segs, sh) / (float)(3 * HW);
    const T* dn = dy + (long long)n * HW * ld;
    float* xn = dx + (long long)n * 3 * HW;
    for (int pix = (blockIdx.x * 256 + threadIdx.x) * PX; pix < HW; pix += gridDim.x * 256 * PX) {
      const int r = pix / H, q = pix - r * H;
      const int dr = r - a.ty;  // the output row these input pixels went to
      float o0[PX], o1[PX], o2[PX];
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const int dq = q + j - a.tx;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if ((unsigned)dr < (unsigned)H && (unsigned)dq < (unsigned)H && aug_live(a, g, dr, dq))
          load_rgb<T, VEC>(dn + (long long)(dr * H + dq) * ld, g0, g1, g2);
        if (policy & S2I_DIFFAUG_COLOR) {
          const float rest = (1.f - a.k) * gm;
          g0 = a.k * g0 + rest;
          g1 = a.k * g1 + rest;
          g2 = a.k * g2 + rest;
          const float pm = (1.f - a.s) * ((g0 + g1 + g2) / 3.f);
          g0 = a.s * g0 + pm;
          g1 = a.s * g1 + pm;
          g2 = a.s * g2 + pm;
        }
        o0[j] = g0, o1[j] = g1, o2[j] = g2;
      }
      if constexpr (PX == 4) {
        st4(xn + pix, f32x4{o0[0], o0[1], o0[2], o0[3]});
        st4(xn + HW + pix, f32x4{o1[0], o1[1], o1[2], o1[3]});
        st4(xn + 2 * HW + pix, f32x4{o2[0], o2[1], o2[2], o2[3]});
      } else {
        xn[pix] = o0[0];
        xn[HW + pix] = o1[0];
        xn[2 * HW + pix] = o2[0];
      }
    }
  }
}

int aug_segments(int H, int W) {
  int s = (int)(((long long)H * W) / 1024);
  return s < 1 ? 1 : (s > 64 ? 64 : s);
}

AugGeom aug_geom(int H) {
  AugGeom g;
  g.H = H;
  g.HW = H * H;
  g.shift = (int)(H * 0.125 + 0.5);
  g.nt = 2 * g.shift + 1;
  g.cut = (int)(H * 0.5 + 0.5);
  g.nc = H + 1 - (g.cut % 2);
  g.segs = aug_segments(H, H);
  return g;
}

dim3 aug_apply_grid(int N, int HW) { return dim3((unsigned)((HW + 255) / 256), (unsigned)(N < 65535 ? N : 65535)); }
dim3 aug_sum_grid(int N, int segs) { return dim3((unsigned)segs, (unsigned)(N < 65535 ? N : 65535)); }

template <typename T>
int backward_impl(const T* dy, int ld, const float* table, int policy, float* dx, int N, const AugGeom& g, float* part,
                  void* stream) {
  // a pixel is one aligned vector load where the row stride keeps every pixel on a 4-element boundary
  const bool vec = ld % 4 == 0 && (uintptr_t)dy % (4 * sizeof(T)) == 0;
  if (policy & S2I_DIFFAUG_COLOR) {
    if (vec)
      hipLaunchKernelGGL((diffaug_grad_sum_kernel<T, true>), aug_sum_grid(N, g.segs), dim3(256), 0, ST, dy, ld, table,
                         policy, N, g, part);
    else
      hipLaunchKernelGGL((diffaug_grad_sum_kernel<T, false>), aug_sum_grid(N, g.segs), dim3(256), 0, ST, dy, ld, table,
                         policy, N, g, part);
    S2I_LAUNCH_CHECK("diffaug_grad_sum");
  }
  const bool quad = g.H % 4 == 0 && (uintptr_t)dx % 16 == 0;
  const dim3 grid = aug_apply_grid(N, quad ? g.HW / 4 : g.HW);
#define S2I_DIFFAUG_BWD(V, PX) \
  hipLaunchKernelGGL((diffaug_backward_kernel<T, V, PX>), grid, dim3(256), 0, ST, dy, ld, table, policy, dx, N, g, part)
  if (vec && quad) S2I_DIFFAUG_BWD(true, 4);
  else if (vec) S2I_DIFFAUG_BWD(true, 1);
  else if (quad) S2I_DIFFAUG_BWD(false, 4);
  else S2I_DIFFAUG_BWD(false, 1);
#undef S2I_DIFFAUG_BWD
  S2I_LAUNCH_CHECK("diffaug_backward");
  return 0;
}
}  // namespace

#define S2I_DIFFAUG_ARGS(name)                                                                                        \
  S2I_REQUIRE(N >= 1 && H >= 2 && H == W && H % 2 == 0 && H <= 16384, name ": N >= 1 square images of even side, got N %d, %d x %d", N, H, W); \
  S2I_REQUIRE(policy >= 0 && (policy & ~S2I_DIFFAUG_ALL) == 0, name ": unknown policy bits in %d", policy)

extern "C" size_t s2i_diffaug_workspace_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return (size_t)N * aug_segments(H, W) * sizeof(float);
}

extern "C" int s2i_diffaug_forward(const float* x, const float* table, int policy, float* y, int N, int H, int W, void* ws,
                                   size_t ws_bytes, void* stream) {
  S2I_REQUIRE(x && table && y, "diffaug_forward: null pointer");
  S2I_DIFFAUG_ARGS("diffaug_forward");
  S2I_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0, "diffaug_forward: x and y must be 16-byte aligned");
  const AugGeom g = aug_geom(H);
  if (policy & S2I_DIFFAUG_COLOR) {
    S2I_REQUIRE(ws && ws_bytes >= s2i_diffaug_workspace_bytes(N, H, W), "diffaug_forward: workspace too small");
    hipLaunchKernelGGL(diffaug_image_sum_kernel, aug_sum_grid(N, g.segs), dim3(256), 0, ST, x, N, 3 * g.HW / 4, g.segs,
                       (float*)ws);
    S2I_LAUNCH_CHECK("diffaug_image_sum");
  }
  hipLaunchKernelGGL(diffaug_forward_kernel, aug_apply_grid(N, g.HW), dim3(256), 0, ST, x, table, policy, y, N, g,
                     (const float*)ws);
  S2I_LAUNCH_CHECK("diffaug_forward");
  return 0;
}

extern "C" int s2i_diffaug_backward(int dtype, const void* dy, int ld, const float* table, int policy, float* dx, int N,
                                    int H, int W, void* ws, size_t ws_bytes, void* stream) {
  S2I_DT_CHECK(dtype, "diffaug_backward");
  S2I_REQUIRE(dy && table && dx, "diffaug_backward: null pointer");
  S2I_DIFFAUG_ARGS("diffaug_backward");
  S2I_REQUIRE(ld >= 4, "diffaug_backward: pixel stride %d < 4", ld);
  const AugGeom g = aug_geom(H);
  if (policy & S2I_DIFFAUG_COLOR)
    S2I_REQUIRE(ws && ws_bytes >= s2i_diffaug_workspace_bytes(N, H, W), "diffaug_backward: workspace too small");
  if (dtype == S2I_DT_BF16) return backward_impl<bf16_t>((const bf16_t*)dy, ld, table, policy, dx, N, g, (float*)ws, stream);
  return backward_impl<float>((const float*)dy, ld, table, policy, dx, N, g, (float*)ws, stream);
}
