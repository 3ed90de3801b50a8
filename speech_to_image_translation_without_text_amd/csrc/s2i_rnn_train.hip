// Training of the speech encoder's recurrent head on gfx950, fp32: the LSTM time step that also stores what the backward
// needs (post-activation gates, cell state, previous hidden state), the backward-through-time step (gate gradients fused
// with the recurrent product dG_{t+1} . W_hh), their two-kernel forms for batches or hidden sizes the fused kernels do
// not take, and the encoder loss (joint-embedding + L1 + distillation) with its gradient for the audio embedding.
// The inference kernels of s2i_rnn.hip are not touched: the recurrence below repeats theirs statement for statement, so
// `out` is bit-identical to the inference path's.
#include "s2i_elementwise.h"

namespace {
// ---- forward ---------------------------------------------------------------------------------------------------------
// lstm_step_kernel (s2i_rnn.hip) plus the stores: gates [B][T][D*4*Hd] (i, f, g, o after their activations, the layout of
// xproj), cst [B][T][D*Hd] (c_t, the layout of out), hprev [D][B][T][Hd] (the h this step started from: the operand of
// dW_hh).  The first step also zeroes out and hprev at the padded positions t >= len, so neither has to be cleared by the
// caller; gates and cst are left unwritten there (the backward never reads them).
__global__ __launch_bounds__(256) void lstm_train_step_kernel(const float* __restrict__ xproj, int ldx,
                                                              const float* __restrict__ whh0, const float* __restrict__ whh1,
                                                              const int* __restrict__ lens, int B, int T, int Hd, int step,
                                                              const float* __restrict__ h_in, float* __restrict__ h_out,
                                                              float* __restrict__ c, float* __restrict__ out, int ldo,
                                                              float* __restrict__ gates, float* __restrict__ cst,
                                                              float* __restrict__ hprev) {
  extern __shared__ __attribute__((aligned(16))) float hs[];  // h: [32][Hd + 4], then W slice: [4 gates x 8 units][Hd + 4]
  const int d = blockIdx.y;
  const int tid = threadIdx.x;
  const int ul = tid & 7, u = blockIdx.x * 8 + ul, b = tid >> 3;
  const int LDH = Hd + 4, Q = Hd / 4;
  float* wsm = hs + 32 * LDH;
  const float* hin = h_in + (size_t)d * B * Hd;
  const float* w = d ? whh1 : whh0;
  for (int e = tid; e < 32 * Q; e += 256) {
    const int r = e / Q, q = e - r * Q;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < B) v = *reinterpret_cast<const f32x4*>(hin + (size_t)r * Hd + q * 4);
    *reinterpret_cast<f32x4*>(hs + r * LDH + q * 4) = v;
    const int grow = (r >> 3) * Hd + blockIdx.x * 8 + (r & 7);  // row r = gate * 8 + unit
    *reinterpret_cast<f32x4*>(wsm + r * LDH + q * 4) = *reinterpret_cast<const f32x4*>(w + (size_t)grow * Hd + q * 4);
  }
  __syncthreads();
  const float* w0 = wsm + (0 * 8 + ul) * LDH;
  const float* w1 = wsm + (1 * 8 + ul) * LDH;
  const float* w2 = wsm + (2 * 8 + ul) * LDH;
  const float* w3 = wsm + (3 * 8 + ul) * LDH;
  const float* hp = hs + b * LDH;
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 4
  for (int k = 0; k < Hd; k += 4) {
    const f32x4 hv = *reinterpret_cast<const f32x4*>(hp + k);
    a0 += hv * *reinterpret_cast<const f32x4*>(w0 + k);
    a1 += hv * *reinterpret_cast<const f32x4*>(w1 + k);
    a2 += hv * *reinterpret_cast<const f32x4*>(w2 + k);
    a3 += hv * *reinterpret_cast<const f32x4*>(w3 + k);
  }
  if (b >= B) return;
  const int D = gridDim.y;
  const size_t e = ((size_t)d * B + b) * Hd + u;
  const int len = lens[b];
  float* hpv = hprev + ((size_t)d * B + b) * T * Hd + u;
  if (step == 0)
    for (int t = len; t < T; ++t) {
      out[((size_t)b * T + t) * ldo + (size_t)d * Hd + u] = 0.f;
      hpv[(size_t)t * Hd] = 0.f;
    }
  if (step >= len) {  // finished sequence: the state is carried unchanged (packed-sequence rule)
    h_out[e] = h_in[e];
    return;
  }
  const int t = d ? len - 1 - step : step;
  const size_t row = (size_t)b * T + t;
  const float* xp = xproj + row * ldx + (size_t)d * 4 * Hd;
  const float gi = sigmoidf_(xp[u] + (a0[0] + a0[1] + a0[2] + a0[3]));
  const float gf = sigmoidf_(xp[Hd + u] + (a1[0] + a1[1] + a1[2] + a1[3]));
  const float gg = tanhf(xp[2 * Hd + u] + (a2[0] + a2[1] + a2[2] + a2[3]));
  const float go = sigmoidf_(xp[3 * Hd + u] + (a3[0] + a3[1] + a3[2] + a3[3]));
  const float cn = gf * c[e] + gi * gg;
  const float hn = go * tanhf(cn);
  c[e] = cn;
  h_out[e] = hn;
  out[row * ldo + (size_t)d * Hd + u] = hn;
  float* gp = gates + (row * D + d) * 4 * Hd + u;
  gp[0] = gi;
  gp[Hd] = gf;
  gp[2 * Hd] = gg;
  gp[3 * Hd] = go;
  cst[(row * D + d) * Hd + u] = cn;
  hpv[(size_t)t * Hd] = h_in[e];
}

// lstm_cell_kernel (s2i_rnn.hip) plus the same stores, one direction per launch; every pointer has its direction's column
// offset applied by the caller, hprev is this direction's [B][T][Hd].
__global__ void lstm_train_cell_kernel(const float* __restrict__ xproj, int ldx, const float* __restrict__ hproj,
                                       const int* __restrict__ lens, int B, int T, int Hd, int step, int reverse,
                                       float* __restrict__ h, float* __restrict__ c, float* __restrict__ out, int ldo,
                                       float* __restrict__ gates, float* __restrict__ cst, float* __restrict__ hprev) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * Hd) return;
  const int b = e / Hd, j = e - b * Hd;
  const int len = lens[b];
  if (step == 0)
    for (int t = len; t < T; ++t) {
      out[((size_t)b * T + t) * ldo + j] = 0.f;
      hprev[((size_t)b * T + t) * Hd + j] = 0.f;
    }
  if (step >= len) return;
  const int t = reverse ? len - 1 - step : step;
  const size_t row = (size_t)b * T + t;
  const float* xp = xproj + row * ldx;
  const float* hp = hproj + (size_t)b * 4 * Hd;
  const float gi = sigmoidf_(xp[j] + hp[j]);
  const float gf = sigmoidf_(xp[Hd + j] + hp[Hd + j]);
  const float gg = tanhf(xp[2 * Hd + j] + hp[2 * Hd + j]);
  const float go = sigmoidf_(xp[3 * Hd + j] + hp[3 * Hd + j]);
  const float cn = gf * c[e] + gi * gg;
  const float hn = go * tanhf(cn);
  hprev[row * Hd + j] = h[e];
  c[e] = cn;
  h[e] = hn;
  out[row * ldo + j] = hn;
  float* gp = gates + row * ldx + j;
  gp[0] = gi;
  gp[Hd] = gf;
  gp[2 * Hd] = gg;
  gp[3 * Hd] = go;
  cst[row * ldo + j] = cn;
}

// ---- backward through time ---------------------------------------------------------------------------------------------
// The cell's backward for one (b, unit) of one direction at recurrence step `step`, given dh_rec = dG_{step+1} . W_hh.
// first = this is the first launch of the backward (the LAST recurrence step): no recurrent gradient exists yet, dc is
// initialised here and the padded rows of dG are zeroed.  A sequence with step >= len has not started its backward: its
// recurrent gradients are zero (h_n and c_n receive none) and stay so.
struct CellBwdArgs {
  const float* d_out;   // [B][T][ldo] or null
  const float* d_sent;  // [B][ldo] or null: the time mean's backward, d_out[b][t] += d_sent[b] / T at t < len
  const float* gates;   // [B][T][ldg]
  const float* cst;     // [B][T][ldo]
  float* dG;            // [B][T][ldg]
  int ldo, ldg, T, Hd, step, reverse, first;
};
__device__ __forceinline__ void cell_backward(const CellBwdArgs& a, int b, int u, int len, float dh_rec, float* dcp,
                                              float* dgt) {
  if (a.first)
    for (int t = len; t < a.T; ++t) {
      float* z = a.dG + ((size_t)b * a.T + t) * a.ldg + u;
      z[0] = 0.f; z[a.Hd] = 0.f; z[2 * a.Hd] = 0.f; z[3 * a.Hd] = 0.f;
    }
  if (a.step >= len) {
    if (a.first) *dcp = 0.f;
    if (dgt) { dgt[0] = 0.f; dgt[a.Hd] = 0.f; dgt[2 * a.Hd] = 0.f; dgt[3 * a.Hd] = 0.f; }
    return;
  }
  const int Hd = a.Hd;
  const int t = a.reverse ? len - 1 - a.step : a.step;
  const size_t row = (size_t)b * a.T + t;
  const float* gp = a.gates + row * a.ldg + u;
  const float gi = gp[0], gf = gp[Hd], gg = gp[2 * Hd], go = gp[3 * Hd];
  const float ct = a.cst[row * a.ldo + u];
  const float cprev = a.step > 0 ? a.cst[((size_t)b * a.T + (a.reverse ? t + 1 : t - 1)) * a.ldo + u] : 0.f;
  float dh = a.d_out ? a.d_out[row * a.ldo + u] : 0.f;
  if (a.d_sent) dh += a.d_sent[(size_t)b * a.ldo + u] / (float)a.T;
  dh += dh_rec;
  const float tc = tanhf(ct);
  const float dc = (a.first ? 0.f : *dcp) + dh * go * (1.f - tc * tc);
  const float dai = dc * gg * gi * (1.f - gi);
  const float daf = dc * cprev * gf * (1.f - gf);
  const float dag = dc * gi * (1.f - gg * gg);
  const float dao = dh * tc * go * (1.f - go);
  *dcp = dc * gf;
  float* z = a.dG + row * a.ldg + u;
  z[0] = dai; z[Hd] = daf; z[2 * Hd] = dag; z[3 * Hd] = dao;
  if (dgt) { dgt[0] = dai; dgt[Hd] = daf; dgt[2 * Hd] = dag; dgt[3 * Hd] = dao; }
}

// One backward step for every direction in ONE launch, the mirror of the forward step: block = 8 hidden units x 32 batch
// slots.  dh_rec[b][u] = sum_k dG_{step+1}[b][k] W_hh[k][u] over the 4*Hd gate rows: 32 x 4*Hd floats of dG do not fit
// the LDS next to anything else at Hd = 512, so k runs in four chunks of Hd (one per gate): [32][Hd + 4] of dG and the
// [8][Hd + 4] slice of the TRANSPOSED W_hh (whht [Hd][4*Hd], made once per backward) per chunk, float4 along k.
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(CellBwdArgs a, const float* __restrict__ whht0,
                                                            const float* __restrict__ whht1, const int* __restrict__ lens,
                                                            int B, float* __restrict__ dcbuf) {
  extern __shared__ __attribute__((aligned(16))) float gs[];  // dG chunk: [32][Hd + 4], then W^T slice: [8][Hd + 4]
  const int d = blockIdx.y, D = gridDim.y;
  const int tid = threadIdx.x;
  const int ul = tid & 7, u = blockIdx.x * 8 + ul, b = tid >> 3;
  const int Hd = a.Hd, LDH = Hd + 4, Q = Hd / 4;
  float acc = 0.f;
  if (!a.first) {
    float* wsm = gs + 32 * LDH;
    const float* wt = d ? whht1 : whht0;
    f32x4 av = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < 4; ++g) {
      if (g) __syncthreads();
      for (int e = tid; e < 32 * Q; e += 256) {
        const int r = e / Q, q = e - r * Q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < B) {
          const int len = lens[r];
          if (a.step + 1 < len) {  // the position this sequence visited at recurrence step + 1
            const int tn = d ? len - 2 - a.step : a.step + 1;
            v = *reinterpret_cast<const f32x4*>(a.dG + ((size_t)r * a.T + tn) * a.ldg + (size_t)d * 4 * Hd + g * Hd + q * 4);
          }
        }
        *reinterpret_cast<f32x4*>(gs + r * LDH + q * 4) = v;
        if (r < 8)
          *reinterpret_cast<f32x4*>(wsm + r * LDH + q * 4) =
              *reinterpret_cast<const f32x4*>(wt + (size_t)(blockIdx.x * 8 + r) * 4 * Hd + g * Hd + q * 4);
      }
      __syncthreads();
      const float* gp = gs + b * LDH;
      const float* wp = wsm + ul * LDH;
#pragma unroll 4
      for (int k = 0; k < Hd; k += 4)
        av += *reinterpret_cast<const f32x4*>(gp + k) * *reinterpret_cast<const f32x4*>(wp + k);
    }
    acc = (av[0] + av[1]) + (av[2] + av[3]);
  }
  if (b >= B) return;
  // this direction's columns
  a.reverse = d;
  if (a.d_out) a.d_out += (size_t)d * Hd;
  if (a.d_sent) a.d_sent += (size_t)d * Hd;
  a.gates += (size_t)d * 4 * Hd;
  a.cst += (size_t)d * Hd;
  a.dG += (size_t)d * 4 * Hd;
  (void)D;
  cell_backward(a, b, u, lens[b], acc, dcbuf + ((size_t)d * B + b) * Hd + u, nullptr);
}

// One direction, dh_rec given (the K1 matrix kernel on dgt of the previous launch); dgt [B][4*Hd] is this step's dG in the
// compact form that product reads.
__global__ void lstm_bwd_cell_kernel(CellBwdArgs a, const float* __restrict__ dhrec, const int* __restrict__ lens, int B,
                                     float* __restrict__ dcbuf, float* __restrict__ dgt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * a.Hd) return;
  const int b = e / a.Hd, u = e - b * a.Hd;
  cell_backward(a, b, u, lens[b], (a.first || !dhrec) ? 0.f : dhrec[e], dcbuf + e, dgt + (size_t)b * 4 * a.Hd + u);
}

// db[n] = sum over the M rows of dG[.][n]: 32 columns x 8 row lanes per block, 8 interleaved partial sums per thread (64
// short sums per column, combined pairwise: one long running sum per column loses sqrt(M) more bits)
__global__ __launch_bounds__(256) void lstm_bias_grad_kernel(const float* __restrict__ dG, int M, int N, float* __restrict__ db) {
  __shared__ float sm[8][33];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, n = blockIdx.x * 32 + cl;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (n < N) {
    int m = rl;
    for (; m + 56 < M; m += 64)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += dG[(size_t)(m + 8 * k) * N + n];
    for (int k = 0; m < M; m += 8, ++k) acc[k] += dG[(size_t)m * N + n];
  }
  sm[rl][cl] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (rl == 0 && n < N)
    db[n] = ((sm[0][cl] + sm[1][cl]) + (sm[2][cl] + sm[3][cl])) + ((sm[4][cl] + sm[5][cl]) + (sm[6][cl] + sm[7][cl]));
}
}  // namespace

extern "C" int s2i_lstm_bias_grad(const float* dG, long long M, int N, float* db, void* stream) {
  S2I_REQUIRE(dG && db && M > 0 && M < (1ll << 31) && N > 0, "lstm_bias_grad: bad args");
  hipLaunchKernelGGL(lstm_bias_grad_kernel, dim3((N + 31) / 32), dim3(256), 0, ST, dG, (int)M, N, db);
  S2I_LAUNCH_CHECK("lstm_bias_grad");
  return 0;
}

extern "C" int s2i_lstm_train_step(const float* xproj, int ldx, const float* whh_fwd, const float* whh_rev, const int* lens,
                                   int B, int T, int Hd, int D, int step, const float* h_in, float* h_out, float* c,
                                   float* out, int ldo, float* gates, float* cst, float* hprev, void* stream) {
  S2I_REQUIRE(xproj && whh_fwd && lens && h_in && h_out && c && out && gates && cst && hprev && h_in != h_out,
              "lstm_train_step: bad pointers");
  S2I_REQUIRE((D == 1 || (D == 2 && whh_rev)) && B > 0 && B <= 32 && T > 0 && step >= 0 && step < T && Hd > 0 &&
                  (Hd % 8) == 0 && Hd <= 512, "lstm_train_step: unsupported extents (B=%d Hd=%d D=%d)", B, Hd, D);
  S2I_REQUIRE(ldx == D * 4 * Hd && ldo == D * Hd, "lstm_train_step: xproj / out rows must be dense (ldx=%d ldo=%d)", ldx, ldo);
  const size_t shb = (size_t)2 * 32 * (Hd + 4) * sizeof(float);
  S2I_REQUIRE(shb <= 160 * 1024, "lstm_train_step: Hd=%d needs %zu bytes of LDS", Hd, shb);
  static bool attr_set = false;
  if (shb > 65536 && !attr_set) {
    S2I_REQUIRE(hipFuncSetAttribute((const void*)lstm_train_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) == hipSuccess, "lstm_train_step: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  hipLaunchKernelGGL(lstm_train_step_kernel, dim3(Hd / 8, D), dim3(256), shb, ST, xproj, ldx, whh_fwd, whh_rev, lens, B, T,
                     Hd, step, h_in, h_out, c, out, ldo, gates, cst, hprev);
  S2I_LAUNCH_CHECK("lstm_train_step");
  return 0;
}

extern "C" int s2i_lstm_train_cell(const float* xproj, int ldx, const float* hproj, const int* lens, int B, int T, int Hd,
                                   int step, int reverse, float* h, float* c, float* out, int ldo, float* gates, float* cst,
                                   float* hprev, void* stream) {
  S2I_REQUIRE(xproj && hproj && lens && h && c && out && gates && cst && hprev && B > 0 && T > 0 && Hd > 0 && step >= 0 &&
                  step < T, "lstm_train_cell: bad args");
  S2I_REQUIRE(ldx >= 4 * Hd && ldo >= Hd, "lstm_train_cell: row strides too small");
  hipLaunchKernelGGL(lstm_train_cell_kernel, dim3((B * Hd + 255) / 256), dim3(256), 0, ST, xproj, ldx, hproj, lens, B, T,
                     Hd, step, reverse, h, c, out, ldo, gates, cst, hprev);
  S2I_LAUNCH_CHECK("lstm_train_cell");
  return 0;
}

extern "C" int s2i_lstm_bwd_step(const float* d_out, const float* d_sent, const float* gates, const float* cst,
                                 const float* whht_fwd, const float* whht_rev, const int* lens, int B, int T, int Hd, int D,
                                 int step, int first, float* dc, float* dG, void* stream) {
  S2I_REQUIRE(gates && cst && whht_fwd && lens && dc && dG, "lstm_bwd_step: bad pointers");
  S2I_REQUIRE((D == 1 || (D == 2 && whht_rev)) && B > 0 && B <= 32 && T > 0 && step >= 0 && step < T && Hd > 0 &&
                  (Hd % 8) == 0 && Hd <= 512, "lstm_bwd_step: unsupported extents (B=%d Hd=%d D=%d)", B, Hd, D);
  const size_t shb = (size_t)40 * (Hd + 4) * sizeof(float);
  static bool attr_set = false;
  if (shb > 65536 && !attr_set) {
    S2I_REQUIRE(hipFuncSetAttribute((const void*)lstm_bwd_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) == hipSuccess, "lstm_bwd_step: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  CellBwdArgs a{d_out, d_sent, gates, cst, dG, D * Hd, D * 4 * Hd, T, Hd, step, 0, first ? 1 : 0};
  hipLaunchKernelGGL(lstm_bwd_step_kernel, dim3(Hd / 8, D), dim3(256), shb, ST, a, whht_fwd, whht_rev, lens, B, dc);
  S2I_LAUNCH_CHECK("lstm_bwd_step");
  return 0;
}

extern "C" int s2i_lstm_bwd_cell(const float* d_out, const float* d_sent, int ldo, const float* gates, int ldg,
                                 const float* cst, const float* dhrec, const int* lens, int B, int T, int Hd, int step,
                                 int reverse, int first, float* dc, float* dG, float* dgt, void* stream) {
  S2I_REQUIRE(gates && cst && lens && dc && dG && dgt && B > 0 && T > 0 && Hd > 0 && step >= 0 && step < T,
              "lstm_bwd_cell: bad args");
  S2I_REQUIRE(first || dhrec, "lstm_bwd_cell: a step after the first needs the recurrent gradient");
  S2I_REQUIRE(ldg >= 4 * Hd && ldo >= Hd, "lstm_bwd_cell: row strides too small");
  CellBwdArgs a{d_out, d_sent, gates, cst, dG, ldo, ldg, T, Hd, step, reverse ? 1 : 0, first ? 1 : 0};
  hipLaunchKernelGGL(lstm_bwd_cell_kernel, dim3((B * Hd + 255) / 256), dim3(256), 0, ST, a, dhrec, lens, B, dc, dgt);
  S2I_LAUNCH_CHECK("lstm_bwd_cell");
  return 0;
}

// ---- the encoder loss ----------------------------------------------------------------------------------------------------
// total = [jel] JEL(audio, image, label) + [l1] lambda_l1 * mean|audio/|audio|_F - image/|image|_F|
//       + [distill] lambda_distill * kl_div(log_softmax(audio), softmax(image / T)) / (B*C)
// (Audio_to_Image/jel.py:17-43, train_audio_encoder.py:308-361) and d total / d audio, in up to five small launches.
// Workspace (floats): score [B][B], G [B][B] (d jel / d score), rowstat [B][6], rowpart [B][3], jel, accu.
namespace {
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
}
// sum / max over a 256-thread block, result in every thread
__device__ float block_sum(float v, float* sm) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
__device__ float block_max(float v, float* sm) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// score[i][j] = image_i . audio_j, one wave per pair
__global__ __launch_bounds__(256) void enc_score_kernel(const float* __restrict__ audio, const float* __restrict__ image,
                                                        int B, int C, float* __restrict__ score) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= B * B) return;
  const int i = p / B, j = p - i * B;
  const float* a = audio + (size_t)j * C;
  const float* m = image + (size_t)i * C;
  float acc = 0.f;
  for (int c = lane; c < C; c += 64) acc += m[c] * a[c];
  acc = wave_sum(acc);
  if (lane == 0) score[p] = acc;
}

// per row: sum a^2, sum m^2, max a, sum exp(a - max), max m/T, sum exp(m/T - max).  The softmaxes are formed as
// exp(v - max) / sum downstream: v - logsumexp would carry the rounding of a logsumexp near log C into every probability.
__global__ __launch_bounds__(256) void enc_rowstat_kernel(const float* __restrict__ audio, const float* __restrict__ image,
                                                          int C, float Tm, float* __restrict__ rowstat) {
  __shared__ float sm[4];
  const int b = blockIdx.x;
  const float* a = audio + (size_t)b * C;
  const float* m = image + (size_t)b * C;
  float ssa = 0.f, ssi = 0.f, ma = -INFINITY, mi = -INFINITY;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float av = a[c], mv = m[c];
    ssa += av * av;
    ssi += mv * mv;
    ma = fmaxf(ma, av);
    mi = fmaxf(mi, mv / Tm);
  }
  ssa = block_sum(ssa, sm);
  ssi = block_sum(ssi, sm);
  ma = block_max(ma, sm);
  mi = block_max(mi, sm);
  float ea = 0.f, ei = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    ea += expf(a[c] - ma);
    ei += expf(m[c] / Tm - mi);
  }
  ea = block_sum(ea, sm);
  ei = block_sum(ei, sm);
  if (threadIdx.x == 0) {
    float* r = rowstat + (size_t)b * 6;
    r[0] = ssa; r[1] = ssi; r[2] = ma; r[3] = ea; r[4] = mi; r[5] = ei;
  }
}

// The joint-embedding loss on score [B][B], one block: column j owns score_abs[., j] = score[., j] - score[j][j], so the
// diagonal's gradient (minus the column's sum) needs no atomics; row i owns its argmax (lowest index wins a tie).
__global__ __launch_bounds__(256) void enc_jel_kernel(const float* __restrict__ score, const int* __restrict__ label, int B,
                                                      float c_diff, float c_same, float* __restrict__ G,
                                                      float* __restrict__ res) {
  __shared__ float sm[4];
  const float inv = 1.f / ((float)B * (float)B);
  float loss = 0.f, hits = 0.f;
  for (int j = threadIdx.x; j < B; j += 256) {
    const float sjj = score[(size_t)j * B + j];
    const int lj = label[j];
    float colsum = 0.f;
    for (int i = 0; i < B; ++i) {
      const float s = score[(size_t)i * B + j] - sjj;
      const bool same = label[i] == lj;
      const float v = same ? s : s + 1.f;
      const float cf = same ? c_same : c_diff;
      const float w = v > 0.f ? cf : 0.f;
      loss += w * v;
      colsum += w;
      if (i != j) G[(size_t)i * B + j] = w * inv;
    }
    G[(size_t)j * B + j] = -colsum * inv;  // its own term is relu(0) = 0
  }
  for (int i = threadIdx.x; i < B; i += 256) {
    const float* r = score + (size_t)i * B;
    int arg = 0;
    float best = r[0];
    for (int j = 1; j < B; ++j)
      if (r[j] > best) { best = r[j]; arg = j; }
    hits += arg == i ? 1.f : 0.f;
  }
  loss = block_sum(loss, sm);
  hits = block_sum(hits, sm);
  if (threadIdx.x == 0) {
    res[0] = loss * inv;
    res[1] = 100.f * hits / (float)B;
  }
}

// per row, with the whole-tensor norms: sum |u|, sum sign(u) a (u = a/na - m/ni), sum q (log q - log p)
__global__ __launch_bounds__(256) void enc_rowpart_kernel(const float* __restrict__ audio, const float* __restrict__ image,
                                                          int B, int C, float Tm, const float* __restrict__ rowstat,
                                                          float* __restrict__ rowpart) {
  __shared__ float sm[4];
  const int b = blockIdx.x;
  float ssa = 0.f, ssi = 0.f;
  for (int r = 0; r < B; ++r) { ssa += rowstat[(size_t)r * 6]; ssi += rowstat[(size_t)r * 6 + 1]; }
  const float na = sqrtf(ssa), ni = sqrtf(ssi);
  const float ma = rowstat[(size_t)b * 6 + 2], ea = rowstat[(size_t)b * 6 + 3];
  const float mi = rowstat[(size_t)b * 6 + 4], ei = rowstat[(size_t)b * 6 + 5];
  const float dlog = logf(ei) - logf(ea);
  const float* a = audio + (size_t)b * C;
  const float* m = image + (size_t)b * C;
  float l1 = 0.f, dot = 0.f, kl = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float av = a[c], mv = m[c];
    const float u = av / na - mv / ni;
    l1 += fabsf(u);
    dot += u > 0.f ? av : (u < 0.f ? -av : 0.f);
    const float zq = mv / Tm - mi, q = expf(zq) / ei;
    if (q > 0.f) kl += q * ((zq - (av - ma)) - dlog);  // log q - log p
  }
  l1 = block_sum(l1, sm);
  dot = block_sum(dot, sm);
  kl = block_sum(kl, sm);
  if (threadIdx.x == 0) {
    float* r = rowpart + (size_t)b * 3;
    r[0] = l1; r[1] = dot; r[2] = kl;
  }
}

// grad[j][c] and, from block (0, 0), the five scalars
__global__ __launch_bounds__(256) void enc_grad_kernel(const float* __restrict__ audio, const float* __restrict__ image,
                                                       int B, int C, int flags, float lam_l1, float lam_d, float Tm,
                                                       const float* __restrict__ G, const float* __restrict__ rowstat,
                                                       const float* __restrict__ rowpart, const float* __restrict__ res,
                                                       float* __restrict__ grad, float* __restrict__ scal) {
  const int j = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  const bool jel = flags & 1, l1 = flags & 2, dis = flags & 4;
  const float invBC = 1.f / ((float)B * (float)C);
  float ssa = 0.f, ssi = 0.f, sabs = 0.f, sdot = 0.f, skl = 0.f;
  if (l1 || dis)
    for (int r = 0; r < B; ++r) {
      ssa += rowstat[(size_t)r * 6];
      ssi += rowstat[(size_t)r * 6 + 1];
      sabs += rowpart[(size_t)r * 3];
      sdot += rowpart[(size_t)r * 3 + 1];
      skl += rowpart[(size_t)r * 3 + 2];
    }
  if (blockIdx.x == 0 && j == 0 && threadIdx.x == 0) {
    const float vj = jel ? res[0] : 0.f, v1 = l1 ? sabs * invBC : 0.f, vd = dis ? skl * invBC : 0.f;
    scal[0] = vj + lam_l1 * v1 + lam_d * vd;
    scal[1] = vj;
    scal[2] = v1;
    scal[3] = vd;
    scal[4] = jel ? res[1] : 0.f;
  }
  if (c >= C) return;
  const float av = audio[(size_t)j * C + c], mv = image[(size_t)j * C + c];
  float g = 0.f;
  if (jel)
    for (int i = 0; i < B; ++i) g += G[(size_t)i * B + j] * image[(size_t)i * C + c];
  if (l1) {
    const float na = sqrtf(ssa), ni = sqrtf(ssi);
    const float u = av / na - mv / ni;
    const float s = u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f);
    g += lam_l1 * invBC * (s / na - sdot * av / (na * na * na));
  }
  if (dis) {
    const float* r = rowstat + (size_t)j * 6;
    const float p = expf(av - r[2]) / r[3], q = expf(mv / Tm - r[4]) / r[5];
    g += lam_d * invBC * (p - q);
  }
  grad[(size_t)j * C + c] = g;
}
}  // namespace

extern "C" size_t s2i_encoder_loss_workspace_bytes(int B) {
  return B > 0 ? ((size_t)2 * B * B + (size_t)9 * B + 2) * sizeof(float) : 0;
}

extern "C" int s2i_encoder_loss(const float* audio, const float* image, const int* label, int B, int C, float c_diff,
                                float c_same, int flags, float lambda_l1, float lambda_distill, float distill_T, void* ws,
                                size_t ws_bytes, float* grad, float* scal, void* stream) {
  S2I_REQUIRE(audio && image && label && grad && scal && B > 0 && C > 0 && B <= 65535, "encoder_loss: bad args");
  S2I_REQUIRE((flags & ~7) == 0, "encoder_loss: unknown flags %d", flags);
  S2I_REQUIRE(!(flags & 4) || distill_T > 0.f, "encoder_loss: the distillation temperature must be positive");
  S2I_REQUIRE(ws && ws_bytes >= s2i_encoder_loss_workspace_bytes(B), "encoder_loss: workspace too small (%zu < %zu)",
              ws_bytes, s2i_encoder_loss_workspace_bytes(B));
  float* score = (float*)ws;
  float* G = score + (size_t)B * B;
  float* rowstat = G + (size_t)B * B;
  float* rowpart = rowstat + (size_t)6 * B;
  float* res = rowpart + (size_t)3 * B;
  if (flags & 1) {
    hipLaunchKernelGGL(enc_score_kernel, dim3((B * B + 3) / 4), dim3(256), 0, ST, audio, image, B, C, score);
    hipLaunchKernelGGL(enc_jel_kernel, dim3(1), dim3(256), 0, ST, score, label, B, c_diff, c_same, G, res);
  }
  if (flags & 6) {
    hipLaunchKernelGGL(enc_rowstat_kernel, dim3(B), dim3(256), 0, ST, audio, image, C, distill_T, rowstat);
    hipLaunchKernelGGL(enc_rowpart_kernel, dim3(B), dim3(256), 0, ST, audio, image, B, C, distill_T, rowstat, rowpart);
  }
  hipLaunchKernelGGL(enc_grad_kernel, dim3((C + 255) / 256, B), dim3(256), 0, ST, audio, image, B, C, flags, lambda_l1,
                     lambda_distill, distill_T, G, rowstat, rowpart, res, grad, scal);
  S2I_LAUNCH_CHECK("encoder_loss");
  return 0;
}
