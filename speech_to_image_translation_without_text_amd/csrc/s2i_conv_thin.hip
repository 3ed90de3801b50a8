// Thin-layer and RGB kernels: convolutions with 3 (4) channels on one side, which the 32-wide matrix tiles would pad 7/8.
// Interface: launch_thin (s2i_igemm.h); which layer runs on which of them is decided in s2i_conv_plan.hip.
#include "s2i_igemm.h"

namespace {

// ---- thin layers: 3 (4) channels on one side --------------------------------------------------------------------------
// GET_IMAGE_G's conv3x3 -> RGB and the input gradient of the discriminators' first conv (few OUTPUT channels), the first
// discriminator conv itself and GET_IMAGE_G's input gradient (4 INPUT channels): ONE LANE PER OUTPUT PIXEL on the vector
// units, the weights as wave-uniform operands (scalar loads of a [phase][tap][k][n] fp32 table prepared by
// thin_table_kernel), so an FMA needs no LDS read and no cross-lane reduction.  HBM-bound by design; the 32-wide matrix
// tiles are 7/8 padding here and small_n_conv_kernel (s2i_conv_fwd.hip) spends most of its time in LDS weight reads and
// shuffles.
__global__ void thin_table_kernel(const float* __restrict__ P, float* __restrict__ table, int kind, int flip, int T, int wt,
                                  int wR, int ldw, int Kk, int Nn, int nphases) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = nphases * T * Kk * Nn;
  if (e >= total) return;
  const int n = e % Nn, k = (e / Nn) % Kk, t = (e / (Nn * Kk)) % T, ph = e / (Nn * Kk * T);
  const int tw = tap_weight(kind, flip, T, t, ph >> 1, ph & 1);
  float v = 0.f;
  if (wt) { if (n < wR && k < ldw) v = P[((size_t)tw * wR + n) * ldw + k]; }
  else { if (k < wR && n < ldw) v = P[((size_t)tw * wR + k) * ldw + n]; }
  table[e] = v;
}

__device__ __forceinline__ void load8(const IgemmP& p, long long xe, float (&v)[8]) {
  if (p.x16) {
    const u32x4 h = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(p.x) + xe);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __builtin_bit_cast(float, h[j] << 16);
      v[2 * j + 1] = __builtin_bit_cast(float, h[j] & 0xffff0000u);
    }
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p.x + xe), b = *reinterpret_cast<const f32x4*>(p.x + xe + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
}

// <= 4 output channels: y[pix][0..3] = act(sum_{t,c} x[pix + t][c] * table[phase][t][c][0..3] + bias)
__global__ __launch_bounds__(256) void thin_out_kernel(IgemmP p, const float* __restrict__ table) {
  const int phase = blockIdx.z, py = phase >> 1, px = phase & 1;
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);
  const float* __restrict__ wph = table + (size_t)phase * p.T * p.Ca * 4;
  for (int m = blockIdx.x * 256 + threadIdx.x; m < p.M; m += gridDim.x * 256) {
    const int b = m >> p.lgHoWo;
    const int r = m & ((1 << p.lgHoWo) - 1);
    const int oy = r >> p.lgWo, ox = r & (p.Wo - 1);
    const int by = oy * s - pad, bx = ox * s - pad;
    const unsigned mask = tap_mask(p.kind, kw, by, bx, p.H, p.W, py, px);
    const long long xo = (((long long)b * p.H + by) * p.W + bx) * p.Cx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int t = 0; t < p.T; ++t) {
      if (!((mask >> t) & 1u)) continue;
      int dy, dx;
      tap_delta(p.kind, kw, t, py, px, dy, dx);
      const long long xe = xo + ((long long)dy * p.W + dx) * p.Cx;
      for (int c0 = 0; c0 < p.Ca; c0 += 8) {
        float v[8];
        load8(p, xe + c0, v);
        const float* __restrict__ w = wph + ((size_t)t * p.Ca + c0) * 4;   // wave-uniform
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a0 = fmaf(v[j], w[j * 4 + 0], a0);
          a1 = fmaf(v[j], w[j * 4 + 1], a1);
          a2 = fmaf(v[j], w[j * 4 + 2], a2);
          a3 = fmaf(v[j], w[j * 4 + 3], a3);
        }
      }
    }
    long long row = m;
    if (p.kind == S2I_TCONV_K4S2) row = ((long long)b * (2 * p.Ho) + 2 * oy + py) * (2 * p.Wo) + 2 * ox + px;
    f32x4 o = {a0, a1, a2, a3};
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      float v = o[n];
      if (p.bias && n < p.N) v += p.bias[n];
      if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
      else if (p.act == S2I_ACT_TANH) v = tanhf(v);
      else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
      o[n] = v;
    }
    if (p.N == 4 && !p.y16 && (p.ldy & 3) == 0) {
      *reinterpret_cast<f32x4*>(p.y + row * p.ldy) = o;
    } else {
      for (int n = 0; n < p.N && n < 4; ++n) {
        if (p.y16) reinterpret_cast<unsigned short*>(p.y)[row * p.ldy + n] = f2bf(o[n]);
        else p.y[row * p.ldy + n] = o[n];
      }
    }
  }
}

// ---- transposed conv to <= 4 channels from 64 (the image gradient of the discriminators' first conv, model.py:383) ------
// small_n_conv_kernel (s2i_conv_fwd.hip) ran this layer at 12 TFLOP/s-equivalent (0.27 ms for a 125 MB stream: every input
// pixel is 256 bytes and four lanes-per-pixel groups re-read it per output phase).  Here a block owns 8 x 8 INPUT pixels (+ 1 halo):
// the 10 x 10 x C patch is staged in LDS once with coalesced 16-byte loads, each of the four waves computes the 8 x 8 outputs
// of ONE output phase (py, px), so its 2 x 2 taps' weights are wave-uniform and arrive as scalar loads from the
// [phase][tap][c][4] table of thin_table_kernel; a lane reads its pixel's channels from LDS as 16-byte pieces (rows padded
// to C + 4 floats: the 16 lanes of a read group hit distinct bank groups).  HBM-bound by construction: x read once, y written
// once.
template <int C>
__global__ __launch_bounds__(256) void tconv_n4_tile_kernel(IgemmP p, const float* __restrict__ table) {
  constexpr int LDP = C + 4;                       // floats per patch pixel in LDS
  __shared__ __attribute__((aligned(16))) float patch[100 * LDP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int phase = __builtin_amdgcn_readfirstlane(tid >> 6), py = phase >> 1, px = phase & 1;
  const int tilesX = p.W >> 3, tilesY = p.H >> 3;
  const int tix = blockIdx.x % tilesX, tiy = (blockIdx.x / tilesX) % tilesY, b = blockIdx.x / (tilesX * tilesY);
  const int iy0 = tiy * 8 - 1, ix0 = tix * 8 - 1;
  // stage the patch: 100 pixels x C/4 float4 pieces
  for (int e = tid; e < 100 * (C / 4); e += 256) {
    const int pix = e / (C / 4), q = e - pix * (C / 4);
    const int yl = pix / 10, xl = pix - yl * 10;
    const int iy = iy0 + yl, ix = ix0 + xl;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
      const long long xe = (((long long)b * p.H + iy) * p.W + ix) * p.Cx + q * 4;
      if (p.x16) {
        const u32x2_t h = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const unsigned short*>(p.x) + xe);
        v = f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u),
                  __builtin_bit_cast(float, h[1] << 16), __builtin_bit_cast(float, h[1] & 0xffff0000u)};
      } else {
        v = *reinterpret_cast<const f32x4*>(p.x + xe);
      }
    }
    *reinterpret_cast<f32x4*>(patch + pix * LDP + q * 4) = v;
  }
  __syncthreads();
  const int ly = lane >> 3, lx = lane & 7;                        // this lane's input pixel inside the tile
  const float* __restrict__ wph = table + (size_t)phase * 4 * C * 4;   // [tap][c][4], wave-uniform
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int dy, dx;
    tap_delta(S2I_TCONV_K4S2, 1, t, py, px, dy, dx);
    const float* xp = patch + ((ly + 1 + dy) * 10 + (lx + 1 + dx)) * LDP;
    const float* __restrict__ w = wph + (size_t)t * C * 4;
#pragma unroll 4
    for (int c0 = 0; c0 < C; c0 += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xp + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a0 = fmaf(v[j], w[(c0 + j) * 4 + 0], a0);
        a1 = fmaf(v[j], w[(c0 + j) * 4 + 1], a1);
        a2 = fmaf(v[j], w[(c0 + j) * 4 + 2], a2);
        a3 = fmaf(v[j], w[(c0 + j) * 4 + 3], a3);
      }
    }
  }
  const int oy = 2 * (tiy * 8 + ly) + py, ox = 2 * (tix * 8 + lx) + px;
  const long long row = ((long long)b * (2 * p.H) + oy) * (2 * p.W) + ox;
  f32x4 o = {a0, a1, a2, a3};
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    float v = o[n];
    if (p.bias && n < p.N) v += p.bias[n];
    if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
    else if (p.act == S2I_ACT_TANH) v = tanhf(v);
    else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
    o[n] = v;
  }
  if (p.N == 4 && !p.y16 && (p.ldy & 3) == 0) {
    *reinterpret_cast<f32x4*>(p.y + row * p.ldy) = o;
  } else {
    for (int n = 0; n < p.N && n < 4; ++n) {
      if (p.y16) reinterpret_cast<unsigned short*>(p.y)[row * p.ldy + n] = f2bf(o[n]);
      else p.y[row * p.ldy + n] = o[n];
    }
  }
}

// conv3x3 to <= 4 channels (GET_IMAGE_G, model.py:287-298) from 16 / 32 / 64 channels, the same construction: a block owns
// 16 x 16 output pixels, stages the 18 x 18 patch of (up to) 32 channels in LDS with coalesced 16-byte loads, one lane per
// output pixel, all nine taps' weights wave-uniform from the [tap][c][4] table.  x read once (+ 27 % halo), y written once.
template <int CCH>
__global__ __launch_bounds__(256) void conv3_n4_tile_kernel(IgemmP p, const float* __restrict__ table) {
  constexpr int LDP = CCH + 4;
  __shared__ __attribute__((aligned(16))) float patch[324 * LDP];
  const int tid = threadIdx.x;
  const int tilesX = p.W >> 4, tilesY = p.H >> 4;
  const int tix = blockIdx.x % tilesX, tiy = (blockIdx.x / tilesX) % tilesY, b = blockIdx.x / (tilesX * tilesY);
  const int iy0 = tiy * 16 - 1, ix0 = tix * 16 - 1;
  const int ly = tid >> 4, lx = tid & 15;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int cb = 0; cb < p.Ca; cb += CCH) {
    if (cb) __syncthreads();
    for (int e = tid; e < 324 * (CCH / 4); e += 256) {
      const int pix = e / (CCH / 4), q = e - pix * (CCH / 4);
      const int yl = pix / 18, xl = pix - yl * 18;
      const int iy = iy0 + yl, ix = ix0 + xl;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
        const long long xe = (((long long)b * p.H + iy) * p.W + ix) * p.Cx + cb + q * 4;
        if (p.x16) {
          const u32x2_t h = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const unsigned short*>(p.x) + xe);
          v = f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u),
                    __builtin_bit_cast(float, h[1] << 16), __builtin_bit_cast(float, h[1] & 0xffff0000u)};
        } else {
          v = *reinterpret_cast<const f32x4*>(p.x + xe);
        }
      }
      *reinterpret_cast<f32x4*>(patch + pix * LDP + q * 4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float* xp = patch + ((ly + t / 3) * 18 + lx + t % 3) * LDP;
      const float* __restrict__ w = table + ((size_t)t * p.Ca + cb) * 4;     // wave-uniform
#pragma unroll 4
      for (int c0 = 0; c0 < CCH; c0 += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xp + c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a0 = fmaf(v[j], w[(c0 + j) * 4 + 0], a0);
          a1 = fmaf(v[j], w[(c0 + j) * 4 + 1], a1);
          a2 = fmaf(v[j], w[(c0 + j) * 4 + 2], a2);
          a3 = fmaf(v[j], w[(c0 + j) * 4 + 3], a3);
        }
      }
    }
  }
  const long long row = ((long long)b * p.H + tiy * 16 + ly) * p.W + tix * 16 + lx;
  f32x4 o = {a0, a1, a2, a3};
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    float v = o[n];
    if (p.bias && n < p.N) v += p.bias[n];
    if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
    else if (p.act == S2I_ACT_TANH) v = tanhf(v);
    else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
    o[n] = v;
  }
  if (p.N == 4 && !p.y16 && (p.ldy & 3) == 0) {
    *reinterpret_cast<f32x4*>(p.y + row * p.ldy) = o;
  } else {
    for (int n = 0; n < p.N && n < 4; ++n) {
      if (p.y16) reinterpret_cast<unsigned short*>(p.y)[row * p.ldy + n] = f2bf(o[n]);
      else p.y[row * p.ldy + n] = o[n];
    }
  }
}

// 4 input channels, NOUT outputs: y[pix][n] = act(sum_{t,ci} x[pix + t][ci] * table[t][ci][n])
template <int NOUT>
__global__ __launch_bounds__(256) void thin_in_kernel(IgemmP p, const float* __restrict__ table) {
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);
  for (int m = blockIdx.x * 256 + threadIdx.x; m < p.M; m += gridDim.x * 256) {
    const int b = m >> p.lgHoWo;
    const int r = m & ((1 << p.lgHoWo) - 1);
    const int oy = r >> p.lgWo, ox = r & (p.Wo - 1);
    const int by = oy * s - pad, bx = ox * s - pad;
    const unsigned mask = tap_mask(p.kind, kw, by, bx, p.H, p.W, 0, 0);
    const long long xo = (((long long)b * p.H + by) * p.W + bx) * 4;
    float acc[NOUT];
#pragma unroll
    for (int n = 0; n < NOUT; ++n) acc[n] = 0.f;
    for (int t = 0; t < p.T; ++t) {
      if (!((mask >> t) & 1u)) continue;
      int dy, dx;
      tap_delta(p.kind, kw, t, 0, 0, dy, dx);
      const long long xe = xo + ((long long)dy * p.W + dx) * 4;
      f32x4 xv;
      if (p.x16) {
        const u32x2_t h = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const unsigned short*>(p.x) + xe);
        xv = f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u),
                   __builtin_bit_cast(float, h[1] << 16), __builtin_bit_cast(float, h[1] & 0xffff0000u)};
      } else {
        xv = *reinterpret_cast<const f32x4*>(p.x + xe);
      }
      const float* __restrict__ w = table + (size_t)t * 4 * NOUT;   // wave-uniform
#pragma unroll
      for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int n = 0; n < NOUT; ++n) acc[n] = fmaf(xv[ci], w[ci * NOUT + n], acc[n]);
    }
#pragma unroll
    for (int n = 0; n < NOUT; ++n) {
      float v = acc[n];
      if (p.bias) v += p.bias[n];
      if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
      else if (p.act == S2I_ACT_TANH) v = tanhf(v);
      else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
      acc[n] = v;
    }
    if (p.y16) {
      unsigned short* yp = reinterpret_cast<unsigned short*>(p.y) + (long long)m * p.ldy;
#pragma unroll
      for (int g = 0; g < NOUT / 8; ++g) {
        u32x4 o;
#pragma unroll
        for (int h = 0; h < 4; ++h) o[h] = (unsigned)f2bf(acc[g * 8 + 2 * h]) | ((unsigned)f2bf(acc[g * 8 + 2 * h + 1]) << 16);
        *reinterpret_cast<u32x4*>(yp + g * 8) = o;
      }
    } else {
      float* yp = p.y + (long long)m * p.ldy;
#pragma unroll
      for (int g = 0; g < NOUT / 4; ++g)
        *reinterpret_cast<f32x4*>(yp + g * 4) = f32x4{acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]};
    }
  }
}

// ---- bf16 mode: the 3-channel image layers on the bf16 matrix cores with PIXELS AS COLUMNS ---------------------------------
// D = W (32 output-channel rows x K) . X^T (K x 32 pixels): the weights are the A operand and stay in registers for the whole
// kernel (fragments prepared by rgb_afrag_kernel), the B fragment of a lane -- 8 consecutive K values of ITS pixel -- is 16
// (bf16) or 32 (fp32 NHWC4: two adjacent taps) contiguous bytes of global memory, so no LDS, no barriers and no cross-lane
// reduction; the result of a pixel sits in the registers of its own lane(s) and leaves as 8 / 16-byte stores.
//   rgb_out: few output channels (GET_IMAGE_G's conv3x3 -> RGB, input gradient of the first discriminator conv)
//   rgb_in : 4 input channels (first discriminator conv, input gradient of GET_IMAGE_G)
__global__ void rgb_afrag_kernel(const float* __restrict__ P, unsigned short* __restrict__ out, int mode, int kind, int flip, int T,
                                 int wt, int wR, int ldw, int CIN, int KW, int MT, int KSTEPS, int nphases, int Nreal) {
  // out[phase][mt][ks][lane][8]; mode 0 (rgb_out): k = t * CIN + c;  mode 1 (rgb_in): k-step = kernel row, j = dxl * 4 + c
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = nphases * MT * KSTEPS * 64 * 8;
  if (e >= total) return;
  const int j = e & 7, lane = (e >> 3) & 63, ks = (e >> 9) % KSTEPS, mt = ((e >> 9) / KSTEPS) % MT, ph = (e >> 9) / (KSTEPS * MT);
  const int n = mt * 32 + (lane & 31), kk = 8 * (lane >> 5) + j;
  int t, c;
  bool live = n < Nreal;
  if (mode == 0) {
    const int k = ks * 16 + kk;
    t = k / CIN;
    c = k - t * CIN;
  } else {
    const int dxl = kk >> 2;
    c = kk & 3;
    t = ks * KW + dxl;
    live = live && dxl < KW;
  }
  float v = 0.f;
  if (live) {
    const int tw = tap_weight(kind, flip, T, t, ph >> 1, ph & 1);
    if (wt) { if (n < wR && c < ldw) v = P[((size_t)tw * wR + n) * ldw + c]; }
    else { if (c < wR && n < ldw) v = P[((size_t)tw * wR + c) * ldw + n]; }
  }
  out[e] = f2bf(v);
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

template <int KSTEPS>
__global__ __launch_bounds__(256) void rgb_out_kernel(IgemmP p, const unsigned short* __restrict__ afrag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int phase = blockIdx.z, py = phase >> 1, px = phase & 1;
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);
  bf16x8_t A[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks)
    A[ks] = *reinterpret_cast<const bf16x8_t*>(afrag + ((size_t)(phase * KSTEPS + ks) * 64 + lane) * 8);
  const int kpt = p.Ca / 16;                      // k-steps per tap
  const unsigned short* xb = reinterpret_cast<const unsigned short*>(p.x);
  const int ngroups = (p.M + 31) / 32;
  for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
    const int m = grp * 32 + l31;
    const bool live = m < p.M;
    const int b = m >> p.lgHoWo;
    const int r = m & ((1 << p.lgHoWo) - 1);
    const int oy = r >> p.lgWo, ox = r & (p.Wo - 1);
    const int by = oy * s - pad, bx = ox * s - pad;
    const unsigned mask = live ? tap_mask(p.kind, kw, by, bx, p.H, p.W, py, px) : 0u;
    const long long xo = (((long long)b * p.H + by) * p.W + bx) * p.Cx + 8 * lh;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int t = ks / kpt, c0 = (ks - t * kpt) * 16;
      int dy, dx;
      tap_delta(p.kind, kw, t, py, px, dy, dx);
      u32x4 v = {0u, 0u, 0u, 0u};
      if ((mask >> t) & 1u) v = *reinterpret_cast<const u32x4*>(xb + xo + ((long long)dy * p.W + dx) * p.Cx + c0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[ks], __builtin_bit_cast(bf16x8_t, v), acc, 0, 0, 0);
    }
    if (lh == 0 && live) {                       // rows 0..3 of column l31 = registers 0..3 of this lane
      long long row = m;
      if (p.kind == S2I_TCONV_K4S2) row = ((long long)b * (2 * p.Ho) + 2 * oy + py) * (2 * p.Wo) + 2 * ox + px;
      f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        float v = o[n];
        if (p.bias && n < p.N) v += p.bias[n];
        if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
        else if (p.act == S2I_ACT_TANH) v = tanhf(v);
        else if (p.act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
        o[n] = v;
      }
      if (p.N == 4 && (p.ldy & 3) == 0) *reinterpret_cast<f32x4*>(p.y + row * p.ldy) = o;
      else
        for (int n = 0; n < p.N && n < 4; ++n) p.y[row * p.ldy + n] = o[n];
    }
  }
}

// MT = output-channel tiles of 32; KH = kernel rows = k-steps (a k-step holds the 4 horizontal taps x 4 channels of one row;
// the 3x3 has a zero fourth tap)
template <int MT, int KH>
__global__ __launch_bounds__(256) void rgb_in_kernel(IgemmP p, const unsigned short* __restrict__ afrag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  int s, pad, kw;
  geom(p.kind, p.g_s, p.g_pad, p.g_kw, s, pad, kw);
  bf16x8_t A[MT][KH];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ks = 0; ks < KH; ++ks)
      A[mt][ks] = *reinterpret_cast<const bf16x8_t*>(afrag + ((size_t)(mt * KH + ks) * 64 + lane) * 8);
  unsigned short* yb = reinterpret_cast<unsigned short*>(p.y);
  const int ngroups = (p.M + 31) / 32;
  for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
    const int m = grp * 32 + l31;
    const bool live = m < p.M;
    const int b = m >> p.lgHoWo;
    const int r = m & ((1 << p.lgHoWo) - 1);
    const int oy = r >> p.lgWo, ox = r & (p.Wo - 1);
    const int by = oy * s - pad, bx = ox * s - pad + 2 * lh;   // this lane's two taps: columns bx, bx + 1
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mt][q] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KH; ++ks) {
      const int iy = by + ks;
      const bool rowok = live && iy >= 0 && iy < p.H;
      const float* xp = p.x + (((long long)b * p.H + iy) * p.W + bx) * 4;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
      if (rowok && bx >= 0 && bx < p.W) v0 = *reinterpret_cast<const f32x4*>(xp);
      if (rowok && bx + 1 >= 0 && bx + 1 < p.W) v1 = *reinterpret_cast<const f32x4*>(xp + 4);
      bf16x8_t bv = {(__bf16)v0[0], (__bf16)v0[1], (__bf16)v0[2], (__bf16)v0[3],
                     (__bf16)v1[0], (__bf16)v1[1], (__bf16)v1[2], (__bf16)v1[3]};
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][ks], bv, acc[mt], 0, 0, 0);
    }
    if (!live) continue;
    // column l31 (this pixel): registers 4g..4g+3 of tile mt = channels mt*32 + 8g + 4lh + (0..3)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = mt * 32 + 8 * g + 4 * lh;
        if (n >= p.N) continue;
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = acc[mt][4 * g + q];
          if (p.act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
          else if (p.act == S2I_ACT_TANH) v = tanhf(v);
          o[q] = v;
        }
        *reinterpret_cast<u32x2_t*>(yb + (long long)m * p.ldy + n) =
            u32x2_t{(unsigned)f2bf(o[0]) | ((unsigned)f2bf(o[1]) << 16), (unsigned)f2bf(o[2]) | ((unsigned)f2bf(o[3]) << 16)};
      }
  }
}

}  // namespace


int launch_thin(const s2i_conv_desc* d, const FwdPlan& pl, const IgemmP& p, void* ws, hipStream_t st) {
  const dim3 grid(pl.gx, pl.gy, pl.gz), prep(s2i_cdiv(pl.prep_elems, 256));
  const int wt = d->wmode != 0 ? 1 : 0;
  if (pl.kernel >= FWD_RGB_OUT_4 && pl.kernel <= FWD_RGB_IN_2x4) {
    // A fragments [phase][mt][ks][lane][8]: rgb_out has one row tile and k-steps of 16 (tap, channel) pairs, rgb_in a k-step
    // per kernel row
    const unsigned short* afrag = (const unsigned short*)ws;
    const bool out = pl.kernel <= FWD_RGB_OUT_36;
    const int KW = d->kind == S2I_CONV_K4S2 ? 4 : 3;
    hipLaunchKernelGGL(rgb_afrag_kernel, prep, dim3(256), 0, st, p.w, (unsigned short*)ws, out ? 0 : 1, d->kind, d->flip, pl.T, wt,
                       d->wR, d->ldw, pl.Ca, KW, out ? 1 : (d->N + 31) / 32, out ? pl.T * pl.Ca / 16 : KW, pl.nphases, d->N);
    S2I_LAUNCH_CHECK("rgb_afrag");
    switch (pl.kernel) {
      case FWD_RGB_OUT_4: hipLaunchKernelGGL((rgb_out_kernel<4>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_OUT_8: hipLaunchKernelGGL((rgb_out_kernel<8>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_OUT_9: hipLaunchKernelGGL((rgb_out_kernel<9>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_OUT_16: hipLaunchKernelGGL((rgb_out_kernel<16>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_OUT_18: hipLaunchKernelGGL((rgb_out_kernel<18>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_OUT_36: hipLaunchKernelGGL((rgb_out_kernel<36>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_IN_1x3: hipLaunchKernelGGL((rgb_in_kernel<1, 3>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_IN_2x3: hipLaunchKernelGGL((rgb_in_kernel<2, 3>), grid, dim3(256), 0, st, p, afrag); break;
      case FWD_RGB_IN_1x4: hipLaunchKernelGGL((rgb_in_kernel<1, 4>), grid, dim3(256), 0, st, p, afrag); break;
      default: hipLaunchKernelGGL((rgb_in_kernel<2, 4>), grid, dim3(256), 0, st, p, afrag); break;
    }
    S2I_LAUNCH_CHECK("rgb_conv");
    return 0;
  }
  // the weight table [phase][tap][k][n]: 4 columns per gathered channel, or thin_in's N columns per input channel
  const float* table = (const float*)ws;
  const bool in = pl.kernel == FWD_THIN_IN_16 || pl.kernel == FWD_THIN_IN_32;
  hipLaunchKernelGGL(thin_table_kernel, prep, dim3(256), 0, st, p.w, (float*)ws, d->kind, d->flip, pl.T, wt, d->wR, d->ldw, pl.Ca,
                     in ? d->N : 4, pl.nphases);
  S2I_LAUNCH_CHECK("thin_table");
  switch (pl.kernel) {
    case FWD_TCONV_N4_64: hipLaunchKernelGGL((tconv_n4_tile_kernel<64>), grid, dim3(256), 0, st, p, table); break;
    case FWD_CONV3_N4_16: hipLaunchKernelGGL((conv3_n4_tile_kernel<16>), grid, dim3(256), 0, st, p, table); break;
    case FWD_CONV3_N4_32: hipLaunchKernelGGL((conv3_n4_tile_kernel<32>), grid, dim3(256), 0, st, p, table); break;
    case FWD_THIN_OUT: hipLaunchKernelGGL(thin_out_kernel, grid, dim3(256), 0, st, p, table); break;
    case FWD_THIN_IN_16: hipLaunchKernelGGL((thin_in_kernel<16>), grid, dim3(256), 0, st, p, table); break;
    default: hipLaunchKernelGGL((thin_in_kernel<32>), grid, dim3(256), 0, st, p, table); break;
  }
  S2I_LAUNCH_CHECK("thin_conv");
  return 0;
}
