// Optimiser passes over flat fp32 parameter buffers on gfx950: fused Adam, plain and with L2 weight decay (16 bytes per
// lane per buffer, device-side step counter) and its counter increment, the gradient norm of a flat layout in fp64 with
// the clip coefficient and the skip decision kept on the device, EMA of the generator weights, y = x * a[0] and
// y = a x + b y.  The Adam, EMA and scaling passes are HBM-bound; what the norm pass reaches is measured in DESIGN.md 8b5a.
#include "s2i_elementwise.h"
#include <stdint.h>

namespace {
// one element's Adam update from its effective gradient gg; both kernels below end in it
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float gg, float b1, float b2, float eps,
                                            float step_size, float bc2s) {
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p -= step_size * m / (sqrtf(v) / bc2s + eps);
}

// L2 = false: gg = gscale g (torch.optim.Adam).  L2 = true: gg = gscale g + wd p (torch.optim.Adam(weight_decay=wd)).
// gscale_dev, where given, replaces gscale by a value on the device; apply_dev, where given and 0, ends the kernel before
// its first store (the _dev entry points: a step s2i_grad_clip_scale has decided to skip).
template <bool L2>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n4,
                                                   long long n, float lr, float b1, float b2, float eps, float wd, int step,
                                                   const int* __restrict__ step_dev, float gscale,
                                                   const float* __restrict__ gscale_dev,
                                                   const int* __restrict__ apply_dev) {
  if (apply_dev && apply_dev[0] == 0) return;
  if (gscale_dev) gscale = gscale_dev[0];
  __shared__ float bc[2];
  if (threadIdx.x == 0) {
    const int t = step_dev ? step_dev[0] : step;
    bc[0] = (float)(1.0 - pow((double)b1, (double)t));
    bc[1] = (float)sqrt(1.0 - pow((double)b2, (double)t));
  }
  __syncthreads();
  const float step_size = lr / bc[0];
  const float bc2s = bc[1];
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n4;
       e += (long long)gridDim.x * blockDim.x) {
    if (e * 4 + 3 < n) {
      f32x4 pv = ld4(p + e * 4), gv = ld4(g + e * 4), mv = ld4(m + e * 4), vv = ld4(v + e * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pp = pv[j], mm = mv[j], v2 = vv[j];
        float gg = gv[j] * gscale;
        if (L2) gg += wd * pp;
        adam_update(pp, mm, v2, gg, b1, b2, eps, step_size, bc2s);
        pv[j] = pp; mv[j] = mm; vv[j] = v2;
      }
      st4(p + e * 4, pv); st4(m + e * 4, mv); st4(v + e * 4, vv);
    } else {
      for (long long k = e * 4; k < n; ++k) {
        float pp = p[k], mm = m[k], vv = v[k];
        float gg = g[k] * gscale;
        if (L2) gg += wd * pp;
        adam_update(pp, mm, vv, gg, b1, b2, eps, step_size, bc2s);
        m[k] = mm; v[k] = vv; p[k] = pp;
      }
    }
  }
}
}  // namespace
extern "C" int s2i_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                             float beta2, float eps, int step, const int* step_dev, float gscale, void* stream) {
  S2I_REQUIRE(p && g && m && v && n > 0, "adam_step: bad args");
  S2I_REQUIRE(step_dev || step >= 1, "adam_step: step must be >= 1");
  const long long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(adam_kernel<false>, dim3(grid_for(n4)), dim3(256), 0, ST, p, g, m, v, n4, n, lr, beta1, beta2, eps,
                     0.f, step, step_dev, gscale, (const float*)nullptr, (const int*)nullptr);
  S2I_LAUNCH_CHECK("adam_step");
  return 0;
}
extern "C" int s2i_adam_l2_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int step, const int* step_dev, float gscale,
                                void* stream) {
  S2I_REQUIRE(p && g && m && v && n > 0, "adam_l2_step: bad args");
  S2I_REQUIRE(step_dev || step >= 1, "adam_l2_step: step must be >= 1");
  const long long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(adam_kernel<true>, dim3(grid_for(n4)), dim3(256), 0, ST, p, g, m, v, n4, n, lr, beta1, beta2, eps,
                     weight_decay, step, step_dev, gscale, (const float*)nullptr, (const int*)nullptr);
  S2I_LAUNCH_CHECK("adam_l2_step");
  return 0;
}
extern "C" int s2i_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                 float beta2, float eps, const int* step_dev, const float* gscale_dev,
                                 const int* apply_dev, void* stream) {
  S2I_REQUIRE(p && g && m && v && n > 0, "adam_step_dev: bad args");
  S2I_REQUIRE(step_dev && gscale_dev && apply_dev, "adam_step_dev: step_dev, gscale_dev and apply_dev are required");
  const long long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(adam_kernel<false>, dim3(grid_for(n4)), dim3(256), 0, ST, p, g, m, v, n4, n, lr, beta1, beta2, eps,
                     0.f, 0, step_dev, 0.f, gscale_dev, apply_dev);
  S2I_LAUNCH_CHECK("adam_step_dev");
  return 0;
}
extern "C" int s2i_adam_l2_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, const int* step_dev,
                                    const float* gscale_dev, const int* apply_dev, void* stream) {
  S2I_REQUIRE(p && g && m && v && n > 0, "adam_l2_step_dev: bad args");
  S2I_REQUIRE(step_dev && gscale_dev && apply_dev, "adam_l2_step_dev: step_dev, gscale_dev and apply_dev are required");
  const long long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(adam_kernel<true>, dim3(grid_for(n4)), dim3(256), 0, ST, p, g, m, v, n4, n, lr, beta1, beta2, eps,
                     weight_decay, 0, step_dev, 0.f, gscale_dev, apply_dev);
  S2I_LAUNCH_CHECK("adam_l2_step_dev");
  return 0;
}

// ---- gradient norm of a flat layout, clip coefficient and skip decision ----------------------------------------------------
// Tensor s of the layout is cut into chunks of S2I_GRAD_CHUNK elements from its first element on; chunk0[s] is the index
// of its first chunk among all chunks (chunk0[S] their number).  One block per chunk, 256 lanes:
//   lane t adds the squares of the 16-byte groups t, t + 256, ... of the chunk, elements in ascending order, then of the
//   scalar elements t, t + 256, ... behind the last whole group (all of them where the chunk is not 16-byte aligned);
//   the 64 lanes of a wave are added by the xor butterfly 32, 16, ..., 1; the block's sum is (w0 + w1) + (w2 + w3).
// Every square and every addition is fp64, so the order above, a function of the layout alone, fixes the bits.
namespace {
__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
  for (int o = 32; o; o >>= 1) a += __shfl_xor(a, o);
  return a;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n,
                                                         const long long* __restrict__ offsets,
                                                         const long long* __restrict__ sizes,
                                                         const long long* __restrict__ chunk0, int S,
                                                         double* __restrict__ partials) {
  __shared__ long long span[2];
  __shared__ double wsum[4];
  const int tid = threadIdx.x;
  if (tid == 0) {
    const long long b = blockIdx.x;
    int lo = 0, hi = S - 1;                       // the last tensor whose first chunk is not behind b
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (chunk0[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const long long c = b - chunk0[lo];
    const long long start = offsets[lo] + c * S2I_GRAD_CHUNK;
    long long len = sizes[lo] - c * S2I_GRAD_CHUNK;
    if (len > S2I_GRAD_CHUNK) len = S2I_GRAD_CHUNK;
    if (c < 0 || len < 1 || offsets[lo] < 0 || start + len > n) len = -1;      // a layout that leaves the buffer: read nothing
    span[0] = start;
    span[1] = len;
  }
  __syncthreads();
  const long long len = span[1];
  if (len < 0) {
    if (tid == 0) partials[blockIdx.x] = __builtin_nan("");
    return;
  }
  const float* x = g + span[0];
  const int len4 = ((uintptr_t)x & 15) == 0 ? (int)(len >> 2) : 0;
  double acc = 0.0;
  for (int e = tid; e < len4; e += 256) {
    const f32x4 q = ld4(x + 4 * e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)q[j];
      acc += d * d;
    }
  }
  for (int k = 4 * len4 + tid; k < (int)len; k += 256) {
    const double d = (double)x[k];
    acc += d * d;
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One block of four waves.  Wave w sums tensors w, w + 4, ...: lane l adds the tensor's chunk partials l, l + 64, ... in
// ascending order, then the butterfly.  Lane 0 of the block adds the tensors in ascending order and decides.
__global__ __launch_bounds__(256) void grad_clip_scale_kernel(const double* __restrict__ partials,
                                                              const long long* __restrict__ chunk0, int S, double gscale,
                                                              double max_norm, int* __restrict__ step_dev,
                                                              float* __restrict__ scale_dev, int* __restrict__ apply_dev,
                                                              double* stats) {
  double* seg_norm = stats + S2I_GRAD_STATS_HEAD;
  double* seg_sumsq = seg_norm + S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double ags = fabs(gscale);
  for (int s = wave; s < S; s += 4) {
    double acc = 0.0;
    for (long long c = chunk0[s] + lane; c < chunk0[s + 1]; c += 64) acc += partials[c];
    acc = wave_sum(acc);
    if (lane == 0) {
      seg_sumsq[s] = acc;
      seg_norm[s] = sqrt(acc) * ags;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int s = 0; s < S; ++s) total += seg_sumsq[s];
    const int apply = isfinite(total) ? 1 : 0;
    const double norm = sqrt(total) * ags;
    double coef = 1.0;
    if (max_norm > 0.0) {
      coef = max_norm / (norm + 1e-6);
      if (coef > 1.0) coef = 1.0;
    }
    const float scale = (float)(gscale * coef);
    scale_dev[0] = scale;
    apply_dev[0] = apply;
    if (apply && step_dev) step_dev[0] += 1;
    stats[0] = norm;
    stats[1] = coef;
    stats[2] = (double)scale;
    stats[3] = (double)apply;
    stats[9] = total;
    if (apply) {
      stats[4] += 1.0;
      if (coef < 1.0) stats[5] += 1.0;
      stats[7] += norm;
      if (norm > stats[8]) stats[8] = norm;
    } else {
      stats[6] += 1.0;
    }
  }
}
}  // namespace
extern "C" int s2i_grad_sumsq(const float* g, long long n, const long long* offsets, const long long* sizes,
                              const long long* chunk0, int S, long long nchunks, double* partials, void* stream) {
  S2I_REQUIRE(g && offsets && sizes && chunk0 && partials, "grad_sumsq: null pointer");
  S2I_REQUIRE(n > 0 && S >= 1 && nchunks >= S && nchunks <= 0x7fffffffLL, "grad_sumsq: bad sizes (n %lld, S %d, chunks %lld)",
              n, S, nchunks);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nchunks), dim3(256), 0, ST, g, n, offsets, sizes, chunk0, S, partials);
  S2I_LAUNCH_CHECK("grad_sumsq");
  return 0;
}
extern "C" int s2i_grad_clip_scale(const double* partials, const long long* chunk0, int S, double gscale, double max_norm,
                                   int* step_dev, float* scale_dev, int* apply_dev, double* stats, void* stream) {
  S2I_REQUIRE(partials && chunk0 && scale_dev && apply_dev && stats, "grad_clip_scale: null pointer");
  S2I_REQUIRE(S >= 1, "grad_clip_scale: S must be >= 1");
  S2I_REQUIRE(gscale == gscale && max_norm == max_norm && max_norm >= 0.0, "grad_clip_scale: max_norm must be >= 0 (0: no clipping)");
  hipLaunchKernelGGL(grad_clip_scale_kernel, dim3(1), dim3(256), 0, ST, partials, chunk0, S, gscale, max_norm, step_dev,
                     scale_dev, apply_dev, stats);
  S2I_LAUNCH_CHECK("grad_clip_scale");
  return 0;
}

namespace {
__global__ void increment_kernel(int* c) { c[0] += 1; }
}  // namespace
extern "C" int s2i_increment(int* counter, void* stream) {
  S2I_REQUIRE(counter, "increment: null");
  hipLaunchKernelGGL(increment_kernel, dim3(1), dim3(1), 0, ST, counter);
  S2I_LAUNCH_CHECK("increment");
  return 0;
}

namespace {
__global__ void ema_kernel(float* __restrict__ avg, const float* __restrict__ p, long long n, float decay) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (long long)gridDim.x * blockDim.x)
    avg[e] = decay * avg[e] + (1.f - decay) * p[e];
}
}  // namespace
extern "C" int s2i_ema_update(float* avg, const float* p, long long n, float decay, void* stream) {
  S2I_REQUIRE(avg && p && n > 0, "ema_update: bad args");
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n)), dim3(256), 0, ST, avg, p, n, decay);
  S2I_LAUNCH_CHECK("ema_update");
  return 0;
}

namespace {
__global__ void scale_dev_kernel(float* __restrict__ y, const float* __restrict__ x, long long n,
                                 const float* __restrict__ a) {
  const float av = a[0];
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (long long)gridDim.x * blockDim.x)
    y[e] = x[e] * av;
}
}  // namespace
extern "C" int s2i_scale_dev(float* y, const float* x, long long n, const float* a_dev, void* stream) {
  S2I_REQUIRE(y && x && a_dev && n > 0, "scale_dev: bad args");
  hipLaunchKernelGGL(scale_dev_kernel, dim3(grid_for(n)), dim3(256), 0, ST, y, x, n, a_dev);
  S2I_LAUNCH_CHECK("scale_dev");
  return 0;
}

namespace {
__global__ void axpby_kernel(float* __restrict__ y, const float* __restrict__ x, long long n, float a, float b) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (long long)gridDim.x * blockDim.x)
    y[e] = a * x[e] + (b != 0.f ? b * y[e] : 0.f);
}
}  // namespace
extern "C" int s2i_axpby(float* y, const float* x, long long n, float a, float b, void* stream) {
  S2I_REQUIRE(y && x && n > 0, "axpby: bad args");
  hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(256), 0, ST, y, x, n, a, b);
  S2I_LAUNCH_CHECK("axpby");
  return 0;
}
