// CA_NET and the loss heads of the step on gfx950: reparameterisation and KL term, the discriminators' logit heads (4x4
// NHWC fp32 maps), binary cross-entropy (single and all terms of one discriminator update) and the class-aware loss.  fp32
// scalars per thread, one block where the result is one number; latency-bound.
#include "s2i_elementwise.h"

namespace {
// ---- CA_NET ------------------------------------------------------------------------------------
__global__ void reparam_fwd_kernel(const float* __restrict__ h, const float* __restrict__ eps, int B, int E,
                                   float* __restrict__ c) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * E) return;
  const int b = e / E, j = e - b * E;
  const float mu = h[b * 2 * E + j], lv = h[b * 2 * E + E + j];
  c[e] = eps[e] * __expf(0.5f * lv) + mu;
}
__global__ void reparam_bwd_kernel(const float* __restrict__ h, const float* __restrict__ eps,
                                   const float* __restrict__ dc, const float* __restrict__ dmu,
                                   const float* __restrict__ dlv, int B, int E, float* __restrict__ dh) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * E) return;
  const int b = e / E, j = e - b * E;
  const float lv = h[b * 2 * E + E + j];
  const float g = dc ? dc[e] : 0.f;
  dh[b * 2 * E + j] = g + (dmu ? dmu[e] : 0.f);
  dh[b * 2 * E + E + j] = g * eps[e] * 0.5f * __expf(0.5f * lv) + (dlv ? dlv[e] : 0.f);
}
}  // namespace
extern "C" int s2i_reparam_forward(const float* h, const float* eps, int B, int E, float* c, void* stream) {
  S2I_REQUIRE(h && eps && c && B > 0 && E > 0, "reparam_forward: bad args");
  hipLaunchKernelGGL(reparam_fwd_kernel, dim3((B * E + 255) / 256), dim3(256), 0, ST, h, eps, B, E, c);
  S2I_LAUNCH_CHECK("reparam_forward");
  return 0;
}
extern "C" int s2i_reparam_backward(const float* h, const float* eps, const float* dc, const float* dmu,
                                    const float* dlogvar, int B, int E, float* dh, void* stream) {
  S2I_REQUIRE(h && eps && dh && B > 0 && E > 0, "reparam_backward: bad args");
  hipLaunchKernelGGL(reparam_bwd_kernel, dim3((B * E + 255) / 256), dim3(256), 0, ST, h, eps, dc, dmu, dlogvar, B, E,
                     dh);
  S2I_LAUNCH_CHECK("reparam_backward");
  return 0;
}

namespace {
__global__ __launch_bounds__(256) void kl_fwd_kernel(const float* __restrict__ mu, int ldmu,
                                                     const float* __restrict__ lv, int ldlv, int B, int E,
                                                     float* __restrict__ kl) {
  __shared__ float sh[256];
  float acc = 0.f;
  for (int e = threadIdx.x; e < B * E; e += 256) {
    const int b = e / E, j = e - b * E;
    const float m = mu[b * ldmu + j], l = lv[b * ldlv + j];
    acc += 1.f + l - m * m - __expf(l);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) kl[0] = -0.5f * sh[0] / (float)(B * E);
}
__global__ void kl_bwd_kernel(const float* __restrict__ mu, int ldmu, const float* __restrict__ lv, int ldlv, int B,
                              int E, const float* __restrict__ gout, float* __restrict__ dmu,
                              float* __restrict__ dlv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * E) return;
  const int b = e / E, j = e - b * E;
  const float g = gout[0] * (-0.5f) / (float)(B * E);
  dmu[e] = g * (-2.f * mu[b * ldmu + j]);
  dlv[e] = g * (1.f - __expf(lv[b * ldlv + j]));
}
}  // namespace
extern "C" int s2i_kl_forward(const float* mu, int ldmu, const float* logvar, int ldlv, int B, int E, float* kl,
                              void* stream) {
  S2I_REQUIRE(mu && logvar && kl && B > 0 && E > 0, "kl_forward: bad args");
  hipLaunchKernelGGL(kl_fwd_kernel, dim3(1), dim3(256), 0, ST, mu, ldmu, logvar, ldlv, B, E, kl);
  S2I_LAUNCH_CHECK("kl_forward");
  return 0;
}
extern "C" int s2i_kl_backward(const float* mu, int ldmu, const float* logvar, int ldlv, int B, int E,
                               const float* gout, float* dmu, float* dlogvar, void* stream) {
  S2I_REQUIRE(mu && logvar && gout && dmu && dlogvar && B > 0 && E > 0, "kl_backward: bad args");
  hipLaunchKernelGGL(kl_bwd_kernel, dim3((B * E + 255) / 256), dim3(256), 0, ST, mu, ldmu, logvar, ldlv, B, E, gout,
                     dmu, dlogvar);
  S2I_LAUNCH_CHECK("kl_backward");
  return 0;
}

namespace {
// ---- logit heads + BCE ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void logit_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int C,
                                                        float* __restrict__ prob) {
  __shared__ float sh[256];
  const int b = blockIdx.x;
  const int n = 16 * C;
  float acc = 0.f;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int pix = e / C, c = e - pix * C;
    acc += x[(size_t)b * n + e] * w[c * 16 + pix];
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) prob[b] = sigmoidf_(sh[0] + (bias ? bias[0] : 0.f));
}
__global__ __launch_bounds__(256) void logit_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ prob, const float* __restrict__ dprob,
                                                        int B, int C, float* __restrict__ dx, int acc_dx,
                                                        float* __restrict__ dw, float* __restrict__ dbias, int acc_dw) {
  // dl[b] = d loss / d logit once per block; then every thread owns one (pixel, channel) column of x and walks the
  // batch eight rows at a time so that eight independent loads are in flight (the serial walk was latency-bound: 39 us)
  __shared__ float dl_s[256];
  const int n = 16 * C;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < n;
  int pix = 0, c = 0;
  if (live) { pix = e / C; c = e - pix * C; }
  const float wv = live ? w[c * 16 + pix] : 0.f;
  float gw = 0.f, gb = 0.f;
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int nb = min(256, B - b0);
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      const float pr = prob[b0 + threadIdx.x];
      dl_s[threadIdx.x] = dprob[b0 + threadIdx.x] * pr * (1.f - pr);
    }
    __syncthreads();
    if (e == 0 && dbias)
      for (int b = 0; b < nb; ++b) gb += dl_s[b];
    if (!live) continue;
    for (int b1 = 0; b1 < nb; b1 += 8) {
      float xv[8], dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = b1 + j < nb;
        const size_t off = (size_t)(b0 + b1 + j) * n + e;
        xv[j] = ok ? x[off] : 0.f;
        dv[j] = (ok && dx && acc_dx) ? dx[off] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (b1 + j >= nb) break;
        const float dl = dl_s[b1 + j];
        gw += dl * xv[j];
        if (dx) dx[(size_t)(b0 + b1 + j) * n + e] = dv[j] + dl * wv;
      }
    }
  }
  if (live && dw) dw[c * 16 + pix] = acc_dw ? dw[c * 16 + pix] + gw : gw;
  if (e == 0 && dbias) dbias[0] = acc_dw ? dbias[0] + gb : gb;
}
}  // namespace
extern "C" int s2i_logit_forward(const float* x, const float* w, const float* bias, int B, int C, float* prob,
                                 void* stream) {
  S2I_REQUIRE(x && w && prob && B > 0 && C > 0, "logit_forward: bad args");
  hipLaunchKernelGGL(logit_fwd_kernel, dim3(B), dim3(256), 0, ST, x, w, bias, C, prob);
  S2I_LAUNCH_CHECK("logit_forward");
  return 0;
}
extern "C" int s2i_logit_backward(const float* x, const float* w, const float* prob, const float* dprob, int B, int C,
                                  float* dx, int acc_dx, float* dw, float* dbias, int acc_dw, void* stream) {
  S2I_REQUIRE(x && w && prob && dprob && B > 0 && C > 0, "logit_backward: bad args");
  hipLaunchKernelGGL(logit_bwd_kernel, dim3((16 * C + 255) / 256), dim3(256), 0, ST, x, w, prob, dprob, B, C, dx,
                     acc_dx, dw, dbias, acc_dw);
  S2I_LAUNCH_CHECK("logit_backward");
  return 0;
}

namespace {
__global__ __launch_bounds__(256) void bce_fwd_kernel(const float* __restrict__ prob, float target, int B,
                                                      float weight, float* __restrict__ loss, int accumulate) {
  __shared__ float sh[256];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float p = prob[b];
    const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
    acc += -(target * lp + (1.f - target) * lq);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float v = weight * sh[0] / (float)B;
    loss[0] = accumulate ? loss[0] + v : v;
  }
}
__global__ void bce_bwd_kernel(const float* __restrict__ prob, float target, int B, float weight,
                               const float* __restrict__ gout, float* __restrict__ dprob) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float p = prob[b];
  const float den = fmaxf((1.f - p) * p, 1e-12f);
  dprob[b] = weight * gout[0] * (p - target) / den / (float)B;
}
}  // namespace
extern "C" int s2i_bce_forward(const float* prob, float target, int B, float weight, float* loss, int accumulate,
                               void* stream) {
  S2I_REQUIRE(prob && loss && B > 0, "bce_forward: bad args");
  hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(256), 0, ST, prob, target, B, weight, loss, accumulate);
  S2I_LAUNCH_CHECK("bce_forward");
  return 0;
}
extern "C" int s2i_bce_backward(const float* prob, float target, int B, float weight, const float* gout,
                                float* dprob, void* stream) {
  S2I_REQUIRE(prob && gout && dprob && B > 0, "bce_backward: bad args");
  hipLaunchKernelGGL(bce_bwd_kernel, dim3((B + 255) / 256), dim3(256), 0, ST, prob, target, B, weight, gout, dprob);
  S2I_LAUNCH_CHECK("bce_backward");
  return 0;
}

namespace {
// all BCE terms of one discriminator update: H heads x G stacked batches (pointers passed by value)
struct MultiPtr { const float* p[4]; float* d[4]; };
__global__ __launch_bounds__(256) void bce_multi_fwd_kernel(MultiPtr mp, const float* __restrict__ target,
                                                            const float* __restrict__ weight, int G, int H, int B,
                                                            float* __restrict__ loss) {
  __shared__ float sh[256];
  float acc = 0.f;
  const int n = G * H * B;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int b = e % B, gh = e / B, h = gh % H, g = gh / H;
    const float p = mp.p[h][g * B + b];
    const float t = target[g * H + h];
    const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
    acc += weight[g * H + h] * -(t * lp + (1.f - t) * lq);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = sh[0] / (float)B;
}
__global__ void bce_multi_bwd_kernel(MultiPtr mp, const float* __restrict__ target, const float* __restrict__ weight,
                                     int G, int H, int B, const float* __restrict__ gout) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= G * H * B) return;
  const int b = e % B, gh = e / B, h = gh % H, g = gh / H;
  const float p = mp.p[h][g * B + b];
  const float den = fmaxf((1.f - p) * p, 1e-12f);
  mp.d[h][g * B + b] = weight[g * H + h] * gout[0] * (p - target[g * H + h]) / den / (float)B;
}
}  // namespace
extern "C" int s2i_bce_multi_forward(const float* const* probs, const float* target, const float* weight, int G, int H,
                                     int B, float* loss, void* stream) {
  S2I_REQUIRE(probs && target && weight && loss && G > 0 && H > 0 && H <= 4 && B > 0, "bce_multi_forward: bad args");
  MultiPtr mp = {};
  for (int h = 0; h < H; ++h) { S2I_REQUIRE(probs[h], "bce_multi_forward: null head"); mp.p[h] = probs[h]; }
  hipLaunchKernelGGL(bce_multi_fwd_kernel, dim3(1), dim3(256), 0, ST, mp, target, weight, G, H, B, loss);
  S2I_LAUNCH_CHECK("bce_multi_forward");
  return 0;
}
extern "C" int s2i_bce_multi_backward(const float* const* probs, const float* target, const float* weight, int G, int H,
                                      int B, const float* gout, float* const* dprobs, void* stream) {
  S2I_REQUIRE(probs && dprobs && target && weight && gout && G > 0 && H > 0 && H <= 4 && B > 0,
              "bce_multi_backward: bad args");
  MultiPtr mp = {};
  for (int h = 0; h < H; ++h) {
    S2I_REQUIRE(probs[h] && dprobs[h], "bce_multi_backward: null head");
    mp.p[h] = probs[h];
    mp.d[h] = dprobs[h];
  }
  hipLaunchKernelGGL(bce_multi_bwd_kernel, dim3((G * H * B + 255) / 256), dim3(256), 0, ST, mp, target, weight, G, H, B,
                     gout);
  S2I_LAUNCH_CHECK("bce_multi_backward");
  return 0;
}

namespace {
// ---- class-aware loss ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cal_loss_kernel(const float* __restrict__ S, const int* __restrict__ labels,
                                                       int B, int D, float* __restrict__ loss, int accumulate,
                                                       float* __restrict__ dS) {
  __shared__ float sh[3][256];
  float all = 0.f, pair = 0.f, cnt = 0.f;
  for (int e = threadIdx.x; e < B * B; e += 256) {
    const int i = e / B, j = e - i * B;
    const float v = S[e];
    all += v;
    if (i != j && labels[i] == labels[j]) { pair += v; cnt += 1.f; }
  }
  sh[0][threadIdx.x] = all; sh[1][threadIdx.x] = pair; sh[2][threadIdx.x] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
      sh[2][threadIdx.x] += sh[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  const float n = sh[2][0];
  const float diff = n > 0.f ? sh[0][0] / (float)(B * B) - sh[1][0] / n : 0.f;
  const bool active = n > 0.f && diff > 0.f;
  if (threadIdx.x == 0) {
    const float v = active ? diff / (float)D : 0.f;
    loss[0] = accumulate ? loss[0] + v : v;
  }
  if (dS) {
    // d loss / d S, symmetrised so that dX = dS_sym * X
    for (int e = threadIdx.x; e < B * B; e += 256) {
      const int i = e / B, j = e - i * B;
      float g = 0.f;
      if (active) {
        const float m = (i != j && labels[i] == labels[j]) ? 1.f : 0.f;
        g = 2.f * (1.f / (float)(B * B) - m / n) / (float)D;
      }
      dS[e] = g;
    }
  }
}
}  // namespace
extern "C" int s2i_cal_loss(const float* scores, const int* labels, int B, int D, float* loss, int accumulate,
                            float* dscores_sym, void* stream) {
  S2I_REQUIRE(scores && labels && loss && B > 0 && D > 0, "cal_loss: bad args");
  hipLaunchKernelGGL(cal_loss_kernel, dim3(1), dim3(256), 0, ST, scores, labels, B, D, loss, accumulate, dscores_sym);
  S2I_LAUNCH_CHECK("cal_loss");
  return 0;
}
