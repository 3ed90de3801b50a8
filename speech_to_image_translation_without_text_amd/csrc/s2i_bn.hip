// BatchNorm of the StackGAN-v2 step on gfx950, one op after the other as kernel, launcher, entry point: per-channel batch
// statistics and backward sums (colreduce_kernel) with their fp64 finalize, the eval-mode coefficients, BN-apply fused with
// GLU / LeakyReLU / residual add, its backward apply, and the plain activation backward and GLU passes.  Tensors are
// [M][C] rows of NHWC activations, fp32 or bf16 in HBM (T = float | bf16_t) with fp32 arithmetic; a thread moves 16 bytes
// per access (four fp32 channels; eight bf16 channels in the row-tiled forward).  All passes are HBM-bound.
#include "s2i_elementwise.h"

namespace {
// ---- per-quad value functors ------------------------------------------------------------------
// dz for BN-channel quad `quad` at `row`, un-doing the activation that followed BatchNorm
template <typename T>
__device__ __forceinline__ f32x4 act_dz(const T* __restrict__ y, const T* __restrict__ dout, int lddout,
                                        long long row, int C, int quad, const float* __restrict__ coef,
                                        int act, f32x4 yv) {
  const float* scale = coef + 2 * C;
  const float* shift = coef + 3 * C;
  f32x4 dz;
  if (act == S2I_ACT_GLU) {
    const int hq = C / 8;  // quads per half
    const bool first = quad < hq;
    const int pq = first ? quad + hq : quad - hq;
    const f32x4 yp = ld4(y + row * C + pq * 4);
    const f32x4 d = ld4(dout + row * lddout + (first ? quad : pq) * 4);
    const f32x4 sa = ld4(scale + (first ? quad : pq) * 4), ta = ld4(shift + (first ? quad : pq) * 4);
    const f32x4 sg = ld4(scale + (first ? pq : quad) * 4), tg = ld4(shift + (first ? pq : quad) * 4);
    const f32x4 ya = first ? yv : yp, yg = first ? yp : yv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float za = sa[j] * ya[j] + ta[j];
      const float sgm = sigmoid_gate_<T>(sg[j] * yg[j] + tg[j]);
      dz[j] = first ? d[j] * sgm : d[j] * za * sgm * (1.f - sgm);
    }
  } else {
    const f32x4 d = ld4(dout + row * lddout + quad * 4);
    if (act == S2I_ACT_LRELU) {
      const f32x4 sc = ld4(scale + quad * 4), sh = ld4(shift + quad * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) dz[j] = (sc[j] * yv[j] + sh[j]) > 0.f ? d[j] : 0.2f * d[j];
    } else {
      dz = d;
    }
  }
  return dz;
}

// ACT >= 0: the activation as a compile-time constant (the runtime form compiles every activation's path into one kernel:
// 127 registers = 4 waves per SIMD; specialised, the LeakyReLU form needs far fewer), RPT rows per trip
template <int MODE, typename T, int ACT = -1, int RPT = 4>  // 0: (y, y^2)   1: (dz, dz*xhat)
__global__ __launch_bounds__(256) void colreduce_kernel(const T* __restrict__ y, int ldy,
                                                        const T* __restrict__ dout, int lddout,
                                                        long long M, int C, const float* __restrict__ coef,
                                                        int act_rt, float* __restrict__ part, int nparts, int cpb,
                                                        int ppg, long long Rg) {
  const int act = ACT >= 0 ? ACT : act_rt;
  // rows are split into groups of Rg rows (independent BatchNorm batches); part p covers a row chunk of
  // group p / ppg and uses that group's coefficients
  __shared__ f32x4 sh[2][256];
  const int tid = threadIdx.x;
  const int rpb = 256 / cpb;
  const int ql = tid % cpb, rl = tid / cpb;
  const int quad = blockIdx.y * cpb + ql;
  const int Q = C / 4;
  const int grp = blockIdx.x / ppg, pp = blockIdx.x - grp * ppg;
  const long long chunk = (Rg + ppg - 1) / ppg;
  const long long r0 = grp * Rg + pp * chunk;
  const long long gend = (grp + 1) * Rg < M ? (grp + 1) * Rg : M;
  const long long r1 = r0 + chunk < gend ? r0 + chunk : gend;
  coef += (size_t)grp * 4 * C;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  if (quad < Q) {
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 1) { mean = ld4(coef + quad * 4); invstd = ld4(coef + C + quad * 4); }
    // four rows per trip: their loads are issued together (one row per trip left ~2 loads per lane in flight: 2.9 TB/s)
    long long row = r0 + rl;
    for (; row + (RPT - 1) * rpb < r1; row += RPT * rpb) {
      f32x4 yv[RPT], dz[RPT];
#pragma unroll
      for (int u = 0; u < RPT; ++u) yv[u] = ld4(y + (row + u * rpb) * ldy + quad * 4);
      if (MODE == 1) {
#pragma unroll
        for (int u = 0; u < RPT; ++u) dz[u] = act_dz(y, dout, lddout, row + u * rpb, C, quad, coef, act, yv[u]);
      }
#pragma unroll
      for (int u = 0; u < RPT; ++u) {
        if (MODE == 0) {
          s0 += yv[u];
          s1 += yv[u] * yv[u];
        } else {
          s0 += dz[u];
          s1 += dz[u] * ((yv[u] - mean) * invstd);
        }
      }
    }
    for (; row < r1; row += rpb) {
      const f32x4 yv = ld4(y + row * ldy + quad * 4);
      if (MODE == 0) {
        s0 += yv;
        s1 += yv * yv;
      } else {
        const f32x4 dz = act_dz(y, dout, lddout, row, C, quad, coef, act, yv);
        s0 += dz;
        s1 += dz * ((yv - mean) * invstd);
      }
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
    st4(part + ((size_t)0 * nparts + blockIdx.x) * C + quad * 4, s0);
    st4(part + ((size_t)1 * nparts + blockIdx.x) * C + quad * 4, s1);
  }
}
}  // namespace
extern "C" int s2i_colstats(const float* y, long long M, int C, int ldy, float* part, int nparts, void* stream) {
  S2I_REQUIRE(y && part && M > 0 && C > 0 && C % 4 == 0 && ldy % 4 == 0 && nparts > 0, "colstats: bad args");
  RedGeom g = red_geom(C);
  hipLaunchKernelGGL((colreduce_kernel<0, float>), dim3(nparts, g.gy), dim3(256), 0, ST, y, ldy, (const float*)nullptr, 0,
                     M, C, (const float*)nullptr, 0, part, nparts, g.cpb, nparts, M);
  S2I_LAUNCH_CHECK("colstats");
  return 0;
}

template <typename T>
static int bn_act_bwd_reduce_impl(const T* y, const T* dout, int lddout, long long M, int groups, int C,
                                  const float* coef4, int act, float* part, int nparts, void* stream) {
  S2I_REQUIRE(y && dout && coef4 && part && M > 0 && nparts > 0, "bn_act_bwd_reduce: bad args");
  S2I_REQUIRE(act == S2I_ACT_NONE || act == S2I_ACT_GLU || act == S2I_ACT_LRELU,
              "bn_act_bwd_reduce: activation %d is not NONE, GLU or LRELU", act);
  S2I_REQUIRE(groups >= 1 && M % groups == 0 && nparts % groups == 0, "bn_act_bwd_reduce: bad grouping");
  S2I_REQUIRE(act == S2I_ACT_GLU ? C % 8 == 0 : C % 4 == 0, "bn_act_bwd_reduce: C alignment");
  S2I_REQUIRE(lddout % 4 == 0, "bn_act_bwd_reduce: lddout alignment");
  RedGeom g = red_geom(C);
  // the activation as a template constant: see colreduce_kernel
#define S2I_RED(ACTV) hipLaunchKernelGGL((colreduce_kernel<1, T, ACTV, 4>), dim3(nparts, g.gy), dim3(256), 0, ST, y, C, \
                                         dout, lddout, M, C, coef4, act, part, nparts, g.cpb, nparts / groups, M / groups)
  if (act == S2I_ACT_LRELU) S2I_RED(S2I_ACT_LRELU);
  else if (act == S2I_ACT_GLU) S2I_RED(S2I_ACT_GLU);
  else S2I_RED(S2I_ACT_NONE);
#undef S2I_RED
  S2I_LAUNCH_CHECK("bn_act_bwd_reduce");
  return 0;
}
extern "C" int s2i_bn_act_bwd_reduce(const float* y, const float* dout, int lddout, long long M, int groups, int C,
                                     const float* coef4, int act, float* part, int nparts, void* stream) {
  return bn_act_bwd_reduce_impl<float>(y, dout, lddout, M, groups, C, coef4, act, part, nparts, stream);
}
extern "C" int s2i_bn_act_bwd_reduce_dt(int dtype, const void* y, const void* dout, int lddout, long long M, int groups,
                                        int C, const float* coef4, int act, float* part, int nparts, void* stream) {
  S2I_DT_CHECK(dtype, "bn_act_bwd_reduce");
  if (dtype == S2I_DT_BF16)
    return bn_act_bwd_reduce_impl<bf16_t>((const bf16_t*)y, (const bf16_t*)dout, lddout, M, groups, C, coef4, act, part, nparts, stream);
  return bn_act_bwd_reduce_impl<float>((const float*)y, (const float*)dout, lddout, M, groups, C, coef4, act, part, nparts, stream);
}

namespace {
// Reduce [2][G*ppg][C] partials in double.  Threads = qpb channel quads x `lanes` row lanes (tid = pl * qpb + ql); the G
// groups (independent BatchNorm batches sharing one set of parameters) own contiguous ranges of `lpg` row lanes and are
// reduced AT THE SAME TIME: per-lane sums, a shuffle reduction inside each wave over the lanes of equal quad (no barrier),
// one LDS exchange between waves, then one thread per quad walks the groups in order -- so the running statistics see G
// successive momentum updates exactly as G separate forwards would give.  (The earlier form ran a 10-level LDS tree with
// a barrier per level, once per group: 17 us for what is a few hundred KB.)
template <int MODE>  // 0: BN forward statistics   1: BN backward sums
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ part, int ppg, int G, int C,
                                                           double count, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ rmean,
                                                           float* __restrict__ rvar, float momentum, float eps,
                                                           float* __restrict__ out, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int accumulate, int qpb, int lpg,
                                                           long long* __restrict__ nbt) {
  extern __shared__ double shd[];  // [waves][qpb][8] partial sums, then [G][qpb][8] group sums
  if (MODE == 0 && nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += G;  // num_batches_tracked
  const int tid = threadIdx.x;
  const int NT = blockDim.x;
  const int ql = tid % qpb, pl = tid / qpb;
  const int quad = blockIdx.x * qpb + ql;
  const int Q = C / 4;
  const int nparts = ppg * G;
  const int grp = pl / lpg, pin = pl - grp * lpg;   // this lane's group and its lane index inside the group
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (quad < Q && grp < G) {
    for (int pi = grp * ppg + pin; pi < (grp + 1) * ppg; pi += lpg) {
      const f32x4 v0 = ld4(part + ((size_t)0 * nparts + pi) * C + quad * 4);
      const f32x4 v1 = ld4(part + ((size_t)1 * nparts + pi) * C + quad * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] += v0[j]; a[4 + j] += v1[j]; }
    }
  }
  // lanes of one wave that share the quad AND the group: xor offsets qpb .. 32 stay inside a group when lpg * qpb >= 64
  // (a group then covers whole waves); smaller blocks take the LDS path only
  const int wave = tid >> 6, lane = tid & 63, nwaves = (NT + 63) >> 6;
  const bool whole_waves = (lpg * qpb) % 64 == 0;
  if (whole_waves) {
    for (int off = 32; off >= qpb; off >>= 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += __shfl_xor(a[j], off);
    }
    if (lane < qpb) {
#pragma unroll
      for (int j = 0; j < 8; ++j) shd[((size_t)wave * qpb + lane) * 8 + j] = a[j];
    }
  } else {
    // few threads per group inside one wave: every lane publishes, the group leader sums
#pragma unroll
    for (int j = 0; j < 8; ++j) shd[(size_t)tid * 8 + j] = a[j];
  }
  __syncthreads();
  // group sums -> shd2[g][ql][8] (kept in registers of the group's first lane, then exchanged)
  double gs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (pin == 0 && grp < G && quad < Q) {
    if (whole_waves) {
      const int w0 = (grp * lpg * qpb) >> 6, w1 = (((grp + 1) * lpg * qpb) + 63) >> 6;
      for (int w = w0; w < w1 && w < nwaves; ++w)
#pragma unroll
        for (int j = 0; j < 8; ++j) gs[j] += shd[((size_t)w * qpb + ql) * 8 + j];
    } else {
      for (int k = 0; k < lpg; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) gs[j] += shd[((size_t)((grp * lpg + k) * qpb + ql)) * 8 + j];
    }
  }
  __syncthreads();
  if (pin == 0 && grp < G && quad < Q) {
#pragma unroll
    for (int j = 0; j < 8; ++j) shd[((size_t)grp * qpb + ql) * 8 + j] = gs[j];
  }
  __syncthreads();
  if (pl != 0 || quad >= Q) return;
  double g0[4] = {0, 0, 0, 0}, g1[4] = {0, 0, 0, 0};  // sums over groups (backward: dbeta, dgamma)
  float rm[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 0 && rmean) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { rm[j] = rmean[quad * 4 + j]; rv[j] = rvar[quad * 4 + j]; }
  }
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = quad * 4 + j;
      const double a0 = shd[((size_t)g * qpb + ql) * 8 + j], a1 = shd[((size_t)g * qpb + ql) * 8 + 4 + j];
      if (MODE == 0) {
        float* o = out + (size_t)g * 4 * C;
        const double mean = a0 / count;
        double var = a1 / count - mean * mean;
        if (var < 0) var = 0;
        const float invstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = gamma[c] * invstd;
        o[c] = (float)mean;
        o[C + c] = invstd;
        o[2 * C + c] = sc;
        o[3 * C + c] = beta[c] - (float)mean * sc;
        const double unb = count > 1 ? var * count / (count - 1) : var;
        rm[j] = (1.f - momentum) * rm[j] + momentum * (float)mean;
        rv[j] = (1.f - momentum) * rv[j] + momentum * (float)unb;
      } else {
        float* o = out + (size_t)g * 2 * C;
        o[c] = (float)(a0 / count);
        o[C + c] = (float)(a1 / count);
        g0[j] += a0;
        g1[j] += a1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = quad * 4 + j;
    if (MODE == 0) {
      if (rmean) { rmean[c] = rm[j]; rvar[c] = rv[j]; }
    } else {
      if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)g0[j] : (float)g0[j];
      if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)g1[j] : (float)g1[j];
    }
  }
}

// Same result for very short partial lists (<= 8 rows per group): one thread per channel, no LDS, no barriers.
template <int MODE>
__global__ __launch_bounds__(256) void bn_finalize_small_kernel(const float* __restrict__ part, int ppg, int G, int C,
                                                                double count, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ rmean,
                                                                float* __restrict__ rvar, float momentum, float eps,
                                                                float* __restrict__ out, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int accumulate,
                                                                long long* __restrict__ nbt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (MODE == 0 && nbt && c == 0) nbt[0] += G;
  if (c >= C) return;
  const int nparts = ppg * G;
  double g0 = 0, g1 = 0;
  float rm = 0.f, rv = 0.f;
  if (MODE == 0 && rmean) { rm = rmean[c]; rv = rvar[c]; }
  for (int grp = 0; grp < G; ++grp) {
    double a0 = 0, a1 = 0;
    for (int pi = grp * ppg; pi < (grp + 1) * ppg; ++pi) {
      a0 += part[((size_t)0 * nparts + pi) * C + c];
      a1 += part[((size_t)1 * nparts + pi) * C + c];
    }
    if (MODE == 0) {
      float* o = out + (size_t)grp * 4 * C;
      const double mean = a0 / count;
      double var = a1 / count - mean * mean;
      if (var < 0) var = 0;
      const float invstd = (float)(1.0 / sqrt(var + (double)eps));
      const float sc = gamma[c] * invstd;
      o[c] = (float)mean;
      o[C + c] = invstd;
      o[2 * C + c] = sc;
      o[3 * C + c] = beta[c] - (float)mean * sc;
      const double unb = count > 1 ? var * count / (count - 1) : var;
      rm = (1.f - momentum) * rm + momentum * (float)mean;
      rv = (1.f - momentum) * rv + momentum * (float)unb;
    } else {
      float* o = out + (size_t)grp * 2 * C;
      o[c] = (float)(a0 / count);
      o[C + c] = (float)(a1 / count);
      g0 += a0;
      g1 += a1;
    }
  }
  if (MODE == 0) {
    if (rmean) { rmean[c] = rm; rvar[c] = rv; }
  } else {
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)g0 : (float)g0;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)g1 : (float)g1;
  }
}
}  // namespace
static int launch_finalize(int mode, const float* part, int nparts, int groups, int C, long long count,
                           const float* gamma, const float* beta, float* rmean, float* rvar, float momentum, float eps,
                           float* out, float* dgamma, float* dbeta, int accumulate, void* stream,
                           long long* nbt = nullptr) {
  S2I_REQUIRE(part && out && nparts > 0 && C > 0 && C % 4 == 0 && count > 0, "bn finalize: bad args");
  S2I_REQUIRE(groups >= 1 && nparts % groups == 0, "bn finalize: %d partial rows do not split into %d groups", nparts,
              groups);
  const int ppg = nparts / groups;
  if (ppg <= 8) {
    const int grid = (C + 255) / 256;
    if (mode == 0)
      hipLaunchKernelGGL((bn_finalize_small_kernel<0>), dim3(grid), dim3(256), 0, ST, part, ppg, groups, C, (double)count,
                         gamma, beta, rmean, rvar, momentum, eps, out, dgamma, dbeta, accumulate, nbt);
    else
      hipLaunchKernelGGL((bn_finalize_small_kernel<1>), dim3(grid), dim3(256), 0, ST, part, ppg, groups, C, (double)count,
                         gamma, beta, rmean, rvar, momentum, eps, out, dgamma, dbeta, accumulate, nbt);
    S2I_LAUNCH_CHECK("bn_finalize_small");
    return 0;
  }
  const int Q = C / 4;
  // quads per block: few for narrow layers (their partial lists are the long ones), up to 32 for wide layers
  int qpb = 1;
  while (qpb < 32 && qpb * 32 < Q) qpb <<= 1;
  const int grid = (Q + qpb - 1) / qpb;
  // row lanes per group: a power of two, no more than the list is long, groups side by side in at most 256 threads.  (1024
  // threads and 64 KB of LDS until round 3: such a block cannot start on a CU that runs three matrix blocks of another stream
  // -- 123 KB of LDS, 12 of 16 wave slots -- and waited for the tail of that kernel: 44 us per finalize inside the step against
  // 10 us alone.  A 256-thread block with 16 KB fits beside them.)
  const int cap = s2i_tune(S2I_TUNE_FINALIZE_THREADS, 256);
  int lpg = 1;
  while (lpg < ppg && lpg * 2 * groups * qpb <= cap) lpg <<= 1;
  int nthreads = qpb * lpg * groups;
  nthreads = (nthreads + 63) & ~63;
  if (nthreads > 1024) nthreads = 1024;
  const int nwaves = nthreads / 64;
  size_t slots = (size_t)nthreads > (size_t)nwaves * qpb ? (size_t)nthreads : (size_t)nwaves * qpb;
  if (slots < (size_t)groups * qpb) slots = (size_t)groups * qpb;
  const size_t shbytes = slots * 8 * sizeof(double);
  if (mode == 0)
    hipLaunchKernelGGL((bn_finalize_kernel<0>), dim3(grid), dim3(nthreads), shbytes, ST, part, ppg, groups, C, (double)count,
                       gamma, beta, rmean, rvar, momentum, eps, out, dgamma, dbeta, accumulate, qpb, lpg, nbt);
  else
    hipLaunchKernelGGL((bn_finalize_kernel<1>), dim3(grid), dim3(nthreads), shbytes, ST, part, ppg, groups, C, (double)count,
                       gamma, beta, rmean, rvar, momentum, eps, out, dgamma, dbeta, accumulate, qpb, lpg, nbt);
  S2I_LAUNCH_CHECK("bn_finalize");
  return 0;
}

extern "C" int s2i_bn_finalize(const float* part, int nparts, int groups, int C, long long count, const float* gamma,
                               const float* beta, float* running_mean, float* running_var,
                               long long* num_batches_tracked, float momentum, float eps, float* out4, void* stream) {
  S2I_REQUIRE(gamma && beta, "bn_finalize: null affine parameters");
  S2I_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_finalize: running stats must come in pairs");
  return launch_finalize(0, part, nparts, groups, C, count, gamma, beta, running_mean, running_var, momentum, eps,
                         out4, nullptr, nullptr, 0, stream, num_batches_tracked);
}

extern "C" int s2i_bn_bwd_finalize(const float* part, int nparts, int groups, int C, long long count, float* dgamma,
                                   float* dbeta, int accumulate, float* red2, void* stream) {
  return launch_finalize(1, part, nparts, groups, C, count, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, red2, dgamma,
                         dbeta, accumulate, stream);
}

namespace {
__global__ void bn_eval_coeffs_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rmean, const float* __restrict__ rvar, float eps,
                                      float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float invstd = 1.f / sqrtf(rvar[c] + eps);
  const float sc = gamma[c] * invstd;
  out[c] = rmean[c];
  out[C + c] = invstd;
  out[2 * C + c] = sc;
  out[3 * C + c] = beta[c] - rmean[c] * sc;
}
}  // namespace
extern "C" int s2i_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, float* out4, void* stream) {
  S2I_REQUIRE(C > 0 && gamma && beta && running_mean && running_var && out4, "bn_eval_coeffs: bad args");
  hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((C + 255) / 256), dim3(256), 0, ST, C, gamma, beta, running_mean,
                     running_var, eps, out4);
  S2I_LAUNCH_CHECK("bn_eval_coeffs");
  return 0;
}

namespace {
template <typename T, int ACT = -1>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const T* __restrict__ y, long long M, int C,
                                                         const float* __restrict__ coef0, int act_rt,
                                                         const T* __restrict__ residual,
                                                         T* __restrict__ out, int G, unsigned Rg) {
  const int act = ACT >= 0 ? ACT : act_rt;
  const int Cout = act == S2I_ACT_GLU ? C / 2 : C;
  const int Qo = Cout / 4;
  const long long total = M * Qo;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / Qo;
    const int q = (int)(e - row * Qo);
    const float* coef = G > 1 ? coef0 + (size_t)((unsigned)row / Rg) * 4 * C : coef0;
    const float* scale = coef + 2 * C;
    const float* shift = coef + 3 * C;
    f32x4 o;
    if (act == S2I_ACT_GLU) {
      const f32x4 ya = ld4(y + row * C + q * 4), yg = ld4(y + row * C + Cout + q * 4);
      const f32x4 sa = ld4(scale + q * 4), ta = ld4(shift + q * 4);
      const f32x4 sg = ld4(scale + Cout + q * 4), tg = ld4(shift + Cout + q * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (sa[j] * ya[j] + ta[j]) * sigmoid_gate_<T>(sg[j] * yg[j] + tg[j]);
    } else {
      const f32x4 yv = ld4(y + row * C + q * 4);
      const f32x4 sc = ld4(scale + q * 4), sh = ld4(shift + q * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z = sc[j] * yv[j] + sh[j];
        if (act == S2I_ACT_LRELU) z = z > 0.f ? z : 0.2f * z;
        o[j] = z;
      }
      if (residual) o += ld4(residual + row * C + q * 4);
    }
    st4(out + row * Cout + q * 4, o);
  }
}

// ---- row-tiled BatchNorm / activation passes (round 2) --------------------------------------------------------------------
// The grid-stride forms above walk (row, channel quad) pairs: one 64-bit division, up to six coefficient loads and ONE
// 8- or 16-byte activation load in flight per thread and iteration.  Measured (tools/elementwise_bench.py, config 4 shapes):
// bf16 tensors moved at the same ROWS per second as fp32 ones, i.e. at half the bytes per second (1.8 - 3.6 TB/s in the
// backward passes), and the GLU forms at half of that again (both halves' threads load both halves and both compute the
// sigmoid).  These kernels fix a thread to V channels (8 for bf16: 16-byte loads; 4 for fp32) and let it walk rows: every
// coefficient lives in registers, there is no division, two rows' loads are issued before the first is used, and a GLU pair
// (value channel c, gate channel C/2 + c) is ONE thread's work.
// Row-tiled FORWARD kernel for bf16 tensors (measured: wins there; row-tiled backward forms lost to the walkers colreduce_kernel and bn_act_bwd_apply_walk_kernel and were removed).
typedef unsigned int u32x4e __attribute__((ext_vector_type(4)));
template <int V> struct fv { f32x4 v[V / 4]; };

template <int V> __device__ __forceinline__ fv<V> ldv(const float* p) {
  fv<V> r;
#pragma unroll
  for (int k = 0; k < V / 4; ++k) r.v[k] = *reinterpret_cast<const f32x4*>(p + 4 * k);
  return r;
}
template <int V> __device__ __forceinline__ fv<V> ldv(const bf16_t* p) {
  fv<V> r;
  if constexpr (V == 4) {
    r.v[0] = ld4(p);
  } else {
    const u32x4e h = *reinterpret_cast<const u32x4e*>(p);
#pragma unroll
    for (int k = 0; k < 2; ++k)
      r.v[k] = f32x4{__builtin_bit_cast(float, h[2 * k] << 16), __builtin_bit_cast(float, h[2 * k] & 0xffff0000u),
                     __builtin_bit_cast(float, h[2 * k + 1] << 16), __builtin_bit_cast(float, h[2 * k + 1] & 0xffff0000u)};
  }
  return r;
}
template <int V> __device__ __forceinline__ void stv(float* p, const fv<V>& a) {
#pragma unroll
  for (int k = 0; k < V / 4; ++k) *reinterpret_cast<f32x4*>(p + 4 * k) = a.v[k];
}
template <int V> __device__ __forceinline__ void stv(bf16_t* p, const fv<V>& a) {
  if constexpr (V == 4) {
    st4(p, a.v[0]);
  } else {
    u32x4e h;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const f32x2_ lo = {a.v[k][0], a.v[k][1]}, hi = {a.v[k][2], a.v[k][3]};
      h[2 * k] = __builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2_));
      h[2 * k + 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2_));
    }
    *reinterpret_cast<u32x4e*>(p) = h;
  }
}

// rows of this block: the rows are `G` independent BatchNorm batches of Rg rows, each walked by ppg blocks
struct RowSpan { long long r0, r1; int grp; };
__device__ __forceinline__ RowSpan row_span(long long M, int ppg, long long Rg) {
  RowSpan s;
  s.grp = blockIdx.x / ppg;
  const int pp = blockIdx.x - s.grp * ppg;
  const long long chunk = (Rg + ppg - 1) / ppg;
  s.r0 = s.grp * Rg + pp * chunk;
  const long long gend = (s.grp + 1) * Rg < M ? (s.grp + 1) * Rg : M;
  s.r1 = s.r0 + chunk < gend ? s.r0 + chunk : gend;
  return s;
}

template <typename T, int V, int ACT = -1>
__global__ __launch_bounds__(256) void bn_act_fwd_rows_kernel(const T* __restrict__ y, long long M, int C,
                                                              const float* __restrict__ coef0, int act_rt,
                                                              const T* __restrict__ residual, T* __restrict__ out,
                                                              int lgc, int ppg, long long Rg) {
  const int act = ACT >= 0 ? ACT : act_rt;
  const int cpb = 1 << lgc, rpb = 256 >> lgc;
  const int ql = threadIdx.x & (cpb - 1), rl = threadIdx.x >> lgc;
  const bool glu = act == S2I_ACT_GLU;
  const int Cout = glu ? C / 2 : C;
  const int c0 = (blockIdx.y * cpb + ql) * V;
  if (c0 >= Cout) return;
  const RowSpan sp = row_span(M, ppg, Rg);
  const float* scale = coef0 + (size_t)sp.grp * 4 * C + 2 * C;
  const float* shift = scale + C;
  const fv<V> sa = ldv<V>(scale + c0), ta = ldv<V>(shift + c0);
  fv<V> sg, tg;
  if (glu) { sg = ldv<V>(scale + Cout + c0); tg = ldv<V>(shift + Cout + c0); }
  auto one = [&](long long row, const fv<V>& ya, const fv<V>& yx) {   // yx: gate half (GLU) or residual
    fv<V> o;
#pragma unroll
    for (int k = 0; k < V / 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z = sa.v[k][j] * ya.v[k][j] + ta.v[k][j];
        if (glu) z *= sigmoid_gate_<T>(sg.v[k][j] * yx.v[k][j] + tg.v[k][j]);
        else if (act == S2I_ACT_LRELU) z = z > 0.f ? z : 0.2f * z;
        if (!glu && residual) z += yx.v[k][j];
        o.v[k][j] = z;
      }
    stv<V>(out + row * Cout + c0, o);
  };
  const bool two = glu || residual != nullptr;
  const T* second = glu ? y + Cout : residual;
  const long long ld2 = glu ? C : Cout;
  long long row = sp.r0 + rl;
  for (; row + rpb < sp.r1; row += 2 * rpb) {
    const fv<V> a0 = ldv<V>(y + row * C + c0), a1 = ldv<V>(y + (row + rpb) * C + c0);
    fv<V> x0 = a0, x1 = a1;
    if (two) { x0 = ldv<V>(second + row * ld2 + c0); x1 = ldv<V>(second + (row + rpb) * ld2 + c0); }
    one(row, a0, x0);
    one(row + rpb, a1, x1);
  }
  if (row < sp.r1) {
    const fv<V> a0 = ldv<V>(y + row * C + c0);
    fv<V> x0 = a0;
    if (two) x0 = ldv<V>(second + row * ld2 + c0);
    one(row, a0, x0);
  }
}

// host geometry of the row-tiled kernels: threads across the channel vectors (a power of two), the rest of the block
// down the rows; enough blocks along the rows to keep ~16 waves per CU busy with at least a few trips each
// blocks along the rows of one BatchNorm group: `want` rows per thread where the tensor is large, but never so few blocks
// that the chip is under-filled (small tensors: down to one row per thread -- a short kernel is all latency, and a
// thread that walks 8 rows one pair at a time takes four memory round trips where one would do), at most 4096 blocks
static int rows_ppg(long long Rg, int rpb, int groups, int gy, int want) {
  const long long per = (long long)groups * gy;
  long long ppg = (Rg + (long long)rpb * want - 1) / ((long long)rpb * want);
  const long long fill = (2048 + per - 1) / per;
  if (ppg < fill) ppg = fill;
  const long long most = (Rg + rpb - 1) / rpb;               // one row per thread
  if (ppg > most) ppg = most;
  const long long cap = 4096 / per > 0 ? 4096 / per : 1;
  if (ppg > cap) ppg = cap;
  if (ppg < 1) ppg = 1;
  return (int)ppg;
}
struct RowGeom { int lgc, gy, ppg; };
static RowGeom row_geom(int nvec, long long Rg, int groups, int want_parts) {
  RowGeom g;
  g.lgc = 0;
  while ((1 << g.lgc) < nvec && g.lgc < 8) ++g.lgc;
  const int cpb = 1 << g.lgc, rpb = 256 / cpb;
  g.gy = (nvec + cpb - 1) / cpb;
  if (want_parts > 0) { g.ppg = want_parts; return g; }
  g.ppg = rows_ppg(Rg, rpb, groups, g.gy, 8);
  return g;
}
}  // namespace
template <typename T>
static int bn_act_forward_impl(const T* y, long long M, int groups, int C, const float* coef4, int act,
                               const T* residual, T* out, void* stream) {
  S2I_REQUIRE(y && coef4 && out && M > 0 && C > 0, "bn_act_forward: bad args");
  S2I_REQUIRE(act == S2I_ACT_NONE || act == S2I_ACT_GLU || act == S2I_ACT_LRELU,
              "bn_act_forward: activation %d is not NONE, GLU or LRELU", act);
  S2I_REQUIRE(groups >= 1 && M % groups == 0 && M < (1ll << 31), "bn_act_forward: rows do not split into groups");
  S2I_REQUIRE(act == S2I_ACT_GLU ? C % 8 == 0 : C % 4 == 0, "bn_act_forward: C=%d not aligned for act %d", C, act);
  S2I_REQUIRE(!(residual && act == S2I_ACT_GLU), "bn_act_forward: residual with GLU unsupported");
  const int Cout = act == S2I_ACT_GLU ? C / 2 : C;
  constexpr bool is16 = sizeof(T) == 2;
  if (is16) {   // fp32 tensors: no gain from the row-tiled form
#define S2I_FWDR(VV, ACTV) hipLaunchKernelGGL((bn_act_fwd_rows_kernel<T, VV, ACTV>), dim3(groups * g.ppg, g.gy), dim3(256), 0, ST, \
                                              y, M, C, coef4, act, residual, out, g.lgc, g.ppg, M / groups)
    if (is16 && (Cout % 8) == 0) {
      const RowGeom g = row_geom(Cout / 8, M / groups, groups, 0);
      if (act == S2I_ACT_GLU) S2I_FWDR(8, S2I_ACT_GLU);
      else if (act == S2I_ACT_LRELU) S2I_FWDR(8, S2I_ACT_LRELU);
      else S2I_FWDR(8, S2I_ACT_NONE);
    } else {
      const RowGeom g = row_geom(Cout / 4, M / groups, groups, 0);
      S2I_FWDR(4, -1);
    }
#undef S2I_FWDR
    S2I_LAUNCH_CHECK("bn_act_forward(rows)");
    return 0;
  }
  const long long total = M * (Cout / 4);
#define S2I_FWD(ACTV) hipLaunchKernelGGL((bn_act_fwd_kernel<T, ACTV>), dim3(grid_for(total)), dim3(256), 0, ST, y, M, C, coef4, \
                                         act, residual, out, groups, (unsigned)(M / groups))
  if (act == S2I_ACT_GLU) S2I_FWD(S2I_ACT_GLU);
  else if (act == S2I_ACT_LRELU) S2I_FWD(S2I_ACT_LRELU);
  else S2I_FWD(S2I_ACT_NONE);
#undef S2I_FWD
  S2I_LAUNCH_CHECK("bn_act_forward");
  return 0;
}
extern "C" int s2i_bn_act_forward(const float* y, long long M, int groups, int C, const float* coef4, int act,
                                  const float* residual, float* out, void* stream) {
  return bn_act_forward_impl<float>(y, M, groups, C, coef4, act, residual, out, stream);
}
extern "C" int s2i_bn_act_forward_dt(int dtype, const void* y, long long M, int groups, int C, const float* coef4, int act,
                                     const void* residual, void* out, void* stream) {
  S2I_DT_CHECK(dtype, "bn_act_forward");
  if (dtype == S2I_DT_BF16)
    return bn_act_forward_impl<bf16_t>((const bf16_t*)y, M, groups, C, coef4, act, (const bf16_t*)residual, (bf16_t*)out, stream);
  return bn_act_forward_impl<float>((const float*)y, M, groups, C, coef4, act, (const float*)residual, (float*)out, stream);
}

namespace {
// The backward apply as a WALKER (round 2): a thread keeps one channel quad and walks the rows of its block's chunk, as
// colreduce_kernel does, with EVERY coefficient in registers (loaded by hand before the row loop: the stores to dy inside
// the loop keep the compiler from hoisting them).  The grid-stride form it replaced re-loaded seven to nine 16-byte coefficient
// vectors per quad -- L1 hits, but 168 bytes through the CU's 64 B/clk vector-memory path for 24 bytes of data: on the
// 32-channel GLU tensors of the generator that path, not HBM, set the 2.3 TB/s.
template <typename T, int ACT, int RPT = 4>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_walk_kernel(const T* __restrict__ y, const T* __restrict__ dout,
                                                                    int lddout, long long M, int C,
                                                                    const float* __restrict__ coef0,
                                                                    const float* __restrict__ red20, T* __restrict__ dy,
                                                                    int cpb, int ppg, long long Rg) {
  const int tid = threadIdx.x;
  const int rpb = 256 / cpb;
  const int ql = tid % cpb, rl = tid / cpb;
  const int quad = blockIdx.y * cpb + ql;
  if (quad >= C / 4) return;
  const int grp = blockIdx.x / ppg, pp = blockIdx.x - grp * ppg;
  const long long chunk = (Rg + ppg - 1) / ppg;
  const long long r0 = grp * Rg + pp * chunk;
  const long long gend = (grp + 1) * Rg < M ? (grp + 1) * Rg : M;
  const long long r1 = r0 + chunk < gend ? r0 + chunk : gend;
  const float* coef = coef0 + (size_t)grp * 4 * C;
  const float* red2 = red20 + (size_t)grp * 2 * C;
  const float* scale = coef + 2 * C;
  const float* shift = coef + 3 * C;
  const f32x4 mean = ld4(coef + quad * 4), invstd = ld4(coef + C + quad * 4), sc = ld4(scale + quad * 4);
  const f32x4 sh = ld4(shift + quad * 4);
  const f32x4 m0 = ld4(red2 + quad * 4), m1 = ld4(red2 + C + quad * 4);
  // GLU: this quad is in the value half (first) or the gate half; pq is its partner quad in the other half
  const int hq = C / 8;
  const bool first = quad < hq;
  const int pq = ACT == S2I_ACT_GLU ? (first ? quad + hq : quad - hq) : quad;
  const int dq = ACT == S2I_ACT_GLU ? (first ? quad : pq) : quad;          // quad of dout
  f32x4 sp = sc, tp = sh;                                                   // partner's scale / shift
  if (ACT == S2I_ACT_GLU) { sp = ld4(scale + pq * 4); tp = ld4(shift + pq * 4); }
  auto finish = [&](long long row, const f32x4& yv, const f32x4& yp, const f32x4& d) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float dz;
      if (ACT == S2I_ACT_GLU) {
        // value half: dz = d * sigmoid(gate);  gate half: dz = d * value * sigmoid(gate) * (1 - sigmoid(gate))
        const float za = first ? sc[j] * yv[j] + sh[j] : sp[j] * yp[j] + tp[j];
        const float zg = first ? sp[j] * yp[j] + tp[j] : sc[j] * yv[j] + sh[j];
        const float sgm = sigmoid_gate_<T>(zg);
        dz = first ? d[j] * sgm : d[j] * za * sgm * (1.f - sgm);
      } else if (ACT == S2I_ACT_LRELU) {
        dz = (sc[j] * yv[j] + sh[j]) > 0.f ? d[j] : 0.2f * d[j];
      } else {
        dz = d[j];
      }
      const float xh = (yv[j] - mean[j]) * invstd[j];
      o[j] = sc[j] * (dz - m0[j] - xh * m1[j]);
    }
    st4(dy + row * C + quad * 4, o);
  };
  long long row = r0 + rl;
  for (; row + (RPT - 1) * rpb < r1; row += RPT * rpb) {
    f32x4 yv[RPT], yp[RPT], d[RPT];
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      yv[u] = ld4(y + (row + u * rpb) * C + quad * 4);
      d[u] = ld4(dout + (row + u * rpb) * lddout + dq * 4);
      yp[u] = ACT == S2I_ACT_GLU ? ld4(y + (row + u * rpb) * C + pq * 4) : yv[u];
    }
#pragma unroll
    for (int u = 0; u < RPT; ++u) finish(row + u * rpb, yv[u], yp[u], d[u]);
  }
  for (; row < r1; row += rpb) {
    const f32x4 yv = ld4(y + row * C + quad * 4);
    const f32x4 d = ld4(dout + row * lddout + dq * 4);
    const f32x4 yp = ACT == S2I_ACT_GLU ? ld4(y + row * C + pq * 4) : yv;
    finish(row, yv, yp, d);
  }
}
}  // namespace
template <typename T>
static int bn_act_bwd_apply_impl(const T* y, const T* dout, int lddout, long long M, int groups, int C,
                                 const float* coef4, const float* red2, int act, T* dy, void* stream) {
  S2I_REQUIRE(y && dout && coef4 && red2 && dy && M > 0, "bn_act_bwd_apply: bad args");
  S2I_REQUIRE(act == S2I_ACT_NONE || act == S2I_ACT_GLU || act == S2I_ACT_LRELU,
              "bn_act_bwd_apply: activation %d is not NONE, GLU or LRELU", act);
  S2I_REQUIRE(groups >= 1 && M % groups == 0 && M < (1ll << 31), "bn_act_bwd_apply: rows do not split into groups");
  S2I_REQUIRE(act == S2I_ACT_GLU ? C % 8 == 0 : C % 4 == 0, "bn_act_bwd_apply: C alignment");
  S2I_REQUIRE(lddout % 4 == 0, "bn_act_bwd_apply: lddout alignment");
  RedGeom g = red_geom(C);
  const long long Rg = M / groups;
  const int rpb = 256 / g.cpb;
  const int ppg = rows_ppg(Rg, rpb, groups, g.gy, 16);
#define S2I_APPW(ACTV) hipLaunchKernelGGL((bn_act_bwd_apply_walk_kernel<T, ACTV>), dim3(groups * ppg, g.gy), dim3(256), 0, ST, y, \
                                          dout, lddout, M, C, coef4, red2, dy, g.cpb, ppg, Rg)
  if (act == S2I_ACT_GLU) S2I_APPW(S2I_ACT_GLU);
  else if (act == S2I_ACT_LRELU) S2I_APPW(S2I_ACT_LRELU);
  else S2I_APPW(S2I_ACT_NONE);
#undef S2I_APPW
  S2I_LAUNCH_CHECK("bn_act_bwd_apply(walk)");
  return 0;
}
extern "C" int s2i_bn_act_bwd_apply(const float* y, const float* dout, int lddout, long long M, int groups, int C,
                                    const float* coef4, const float* red2, int act, float* dy, void* stream) {
  return bn_act_bwd_apply_impl<float>(y, dout, lddout, M, groups, C, coef4, red2, act, dy, stream);
}
extern "C" int s2i_bn_act_bwd_apply_dt(int dtype, const void* y, const void* dout, int lddout, long long M, int groups,
                                       int C, const float* coef4, const float* red2, int act, void* dy, void* stream) {
  S2I_DT_CHECK(dtype, "bn_act_bwd_apply");
  if (dtype == S2I_DT_BF16)
    return bn_act_bwd_apply_impl<bf16_t>((const bf16_t*)y, (const bf16_t*)dout, lddout, M, groups, C, coef4, red2, act, (bf16_t*)dy, stream);
  return bn_act_bwd_apply_impl<float>((const float*)y, (const float*)dout, lddout, M, groups, C, coef4, red2, act, (float*)dy, stream);
}

namespace {
template <typename T, int ACT>  // S2I_ACT_LRELU | S2I_ACT_TANH
__global__ __launch_bounds__(256) void act_bwd_kernel(const T* __restrict__ out, const T* __restrict__ dout,
                                                      int lddout, long long M, int C, T* __restrict__ dy) {
  const int Q = C / 4;
  const long long total = M * Q;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / Q;
    const int q = (int)(e - row * Q);
    const f32x4 ov = ld4(out + row * C + q * 4);
    const f32x4 d = ld4(dout + row * lddout + q * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ACT == S2I_ACT_LRELU) o[j] = ov[j] > 0.f ? d[j] : 0.2f * d[j];
      else o[j] = d[j] * (1.f - ov[j] * ov[j]);
    }
    st4(dy + row * C + q * 4, o);
  }
}
}  // namespace
template <typename T>
static int act_backward_impl(const T* out, const T* dout, int lddout, long long M, int C, int act, T* dy, void* stream) {
  S2I_REQUIRE(out && dout && dy && M > 0 && C > 0 && C % 4 == 0 && lddout % 4 == 0, "act_backward: bad args");
  S2I_REQUIRE(act == S2I_ACT_LRELU || act == S2I_ACT_TANH, "act_backward: activation %d is not LRELU or TANH", act);
  if (act == S2I_ACT_LRELU)
    hipLaunchKernelGGL((act_bwd_kernel<T, S2I_ACT_LRELU>), dim3(grid_for(M * (C / 4))), dim3(256), 0, ST, out, dout, lddout, M, C, dy);
  else
    hipLaunchKernelGGL((act_bwd_kernel<T, S2I_ACT_TANH>), dim3(grid_for(M * (C / 4))), dim3(256), 0, ST, out, dout, lddout, M, C, dy);
  S2I_LAUNCH_CHECK("act_backward");
  return 0;
}
extern "C" int s2i_act_backward(const float* out, const float* dout, int lddout, long long M, int C, int act,
                                float* dy, void* stream) {
  return act_backward_impl<float>(out, dout, lddout, M, C, act, dy, stream);
}
extern "C" int s2i_act_backward_dt(int dtype, const void* out, const void* dout, int lddout, long long M, int C, int act,
                                   void* dy, void* stream) {
  S2I_DT_CHECK(dtype, "act_backward");
  if (dtype == S2I_DT_BF16)
    return act_backward_impl<bf16_t>((const bf16_t*)out, (const bf16_t*)dout, lddout, M, C, act, (bf16_t*)dy, stream);
  return act_backward_impl<float>((const float*)out, (const float*)dout, lddout, M, C, act, (float*)dy, stream);
}

namespace {
__global__ void glu_fwd_kernel(const float* __restrict__ x, long long M, int C, float* __restrict__ out) {
  const int H = C / 2;
  const long long total = M * H;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / H;
    const int c = (int)(e - row * H);
    out[e] = x[row * C + c] * sigmoidf_(x[row * C + H + c]);
  }
}

__global__ void glu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout, long long M, int C,
                               float* __restrict__ dx) {
  const int H = C / 2;
  const long long total = M * H;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = e / H;
    const int c = (int)(e - row * H);
    const float a = x[row * C + c];
    const float sg = sigmoidf_(x[row * C + H + c]);
    const float d = dout[e];
    dx[row * C + c] = d * sg;
    dx[row * C + H + c] = d * a * sg * (1.f - sg);
  }
}
}  // namespace
extern "C" int s2i_glu_forward(const float* x, long long M, int C, float* out, void* stream) {
  S2I_REQUIRE(x && out && M > 0 && C > 0 && C % 2 == 0, "glu_forward: bad args");
  hipLaunchKernelGGL(glu_fwd_kernel, dim3(grid_for(M * (C / 2))), dim3(256), 0, ST, x, M, C, out);
  S2I_LAUNCH_CHECK("glu_forward");
  return 0;
}
extern "C" int s2i_glu_backward(const float* x, const float* dout, long long M, int C, float* dx, void* stream) {
  S2I_REQUIRE(x && dout && dx && M > 0 && C > 0 && C % 2 == 0, "glu_backward: bad args");
  hipLaunchKernelGGL(glu_bwd_kernel, dim3(grid_for(M * (C / 2))), dim3(256), 0, ST, x, dout, M, C, dx);
  S2I_LAUNCH_CHECK("glu_backward");
  return 0;
}
