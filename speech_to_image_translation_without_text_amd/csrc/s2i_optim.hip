// Optimiser passes over flat fp32 parameter buffers on gfx950: fused Adam, plain and with L2 weight decay (16 bytes per
// lane per buffer, device-side step counter) and its counter increment, EMA of the generator weights, y = x * a[0] and
// y = a x + b y.  HBM-bound.
#include "s2i_elementwise.h"

namespace {
// one element's Adam update from its effective gradient gg; both kernels below end in it
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float gg, float b1, float b2, float eps,
                                            float step_size, float bc2s) {
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  p -= step_size * m / (sqrtf(v) / bc2s + eps);
}

// L2 = false: gg = gscale g (torch.optim.Adam).  L2 = true: gg = gscale g + wd p (torch.optim.Adam(weight_decay=wd)).
template <bool L2>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n4,
                                                   long long n, float lr, float b1, float b2, float eps, float wd, int step,
                                                   const int* __restrict__ step_dev, float gscale) {
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
                     0.f, step, step_dev, gscale);
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
                     weight_decay, step, step_dev, gscale);
  S2I_LAUNCH_CHECK("adam_l2_step");
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
