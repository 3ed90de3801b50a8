// WAV `data` bytes at any rate -> 16 kHz mono fp32 (librosa.load(path, 16000), Audio_to_Image/utils.py:313): sample
// decode, mixdown and band-limited resampling of one group of clips (same rate, sample format and channel count) in one
// launch.  The method is resampy's `kaiser_best`, which librosa.load of the reference's era calls.
//
// Definition.  rate is the file's rate, g = gcd(16000, rate), L = 16000 / g, M = rate / g, scale = min(1, L / M),
// W = ceil(64 / scale), taps = 2 W + 2.  Prototype h(t) = r sinc(r t) I0(beta sqrt(1 - (t / 64)^2)) / I0(beta) for
// |t| <= 64 and 0 outside, r = 0.9475937167399596, beta = 14.769656459379492, sinc(x) = sin(pi x) / (pi x).
// table[p][j] = scale h(scale (W - j + p / L)) for p in [0, L), j in [0, taps): float64 on the host, rounded to fp32
// once.  For output m, in 64-bit integers, q = (m M) div L, p = (m M) mod L and
//   y[m] = sum_j x[q - W + j] table[p][j],     x = 0 outside [0, n).
// A clip of n frames gives n_out = ceil(n L / M) outputs; those with m >= floor(n L / M) are 0.0f (librosa's
// fix_length pads there).  rate = 16000 is L = M = 1, W = 0, table [1, 0]: the same kernel, which then only decodes and
// mixes down.  Decode (little-endian, interleaved): u8 (v - 128) / 128; s16, s24, s32 float(v) 2^-(bits - 1); f32 as is;
// f64 rounded to fp32.  Mono: the channels added in channel order in fp32, divided by float(C), correctly rounded.
// Order: decode, mono, resample, as librosa does.
//
// Device layout of the table: [L][tpad] fp32 with tpad = taps rounded up to a multiple of 4 and the pad zero, so every
// phase's row starts on a 16-byte boundary and is read as f32x4 (audio.pack_resample_table).  The pad is never read.
//
// One 256-thread block per tile-table entry (clip b, first output m0): the S2I_RESAMPLE_TILE = 1024 outputs from m0 on.
//   1. t0 = m0 M in 64 bits, once: q0 = t0 div L, p0 = t0 mod L.  Output m0 + i has q = q0 + (p0 + i M) div L and
//      p = (p0 + i M) mod L; p0 + i M < 16000 + 1023 * 192000 fits 32 bits.
//   2. The input window [q0 - W, q_last + W + 2) is decoded and mixed to mono fp32 into LDS.  Positions outside [0, n)
//      are stored as 0.0f: a block never reads another clip's bytes.
//   3. Each thread forms four outputs of one phase: outputs i and i + L read the same table row, so a work item owns
//      i = r + L (kg + KG u), u < 4 (r = i mod L, KG = ceil(ceil(count / L) / 4)), and one f32x4 of the row feeds four
//      outputs; with L = 1 that is i = t, t + 256, t + 512, t + 768.  For output i the operands are
//      lds[(p0 + i M) div L + j] and row p, four independent accumulators over j mod 4, summed as (a0 + a1) + (a2 + a3).
//      Neighbouring lanes own neighbouring i (stores coalesce) and read LDS M / L floats apart: conflict-free for an
//      odd step (48 kHz), 2-way at 32 and 96 kHz, 4-way at 192 kHz.
// No atomics, no scratch, no workspace; the window is dynamic LDS sized by the host from L, M and W (at most
// S2I_RESAMPLE_MAX_WINDOW floats, 54 KB).
#include "s2i_common.h"

namespace {

constexpr int TILE = S2I_RESAMPLE_TILE;
constexpr int OUT_RATE = 16000;
constexpr int MAX_RATIO = 12;                    // 192 kHz / 16 kHz
constexpr int MAX_W = 64 * MAX_RATIO;            // 768
constexpr int MAX_WINDOW = S2I_RESAMPLE_MAX_WINDOW;
static_assert(MAX_WINDOW == MAX_RATIO * TILE + 2 * MAX_W + 2, "window bound");

// sample k (frame * C + channel) of an interleaved little-endian clip -> fp32
template <int FMT>
__device__ __forceinline__ float decode_sample(const unsigned char* clip, long long k) {
  if (FMT == S2I_PCM_U8) return (float)((int)clip[k] - 128) * (1.f / 128.f);
  if (FMT == S2I_PCM_S16) return (float)((const short*)clip)[k] * (1.f / 32768.f);
  if (FMT == S2I_PCM_S24) {
    const unsigned char* p = clip + 3 * k;
    const int v = (int)((unsigned)p[0] << 8 | (unsigned)p[1] << 16 | (unsigned)p[2] << 24) >> 8;
    return (float)v * (1.f / 8388608.f);
  }
  if (FMT == S2I_PCM_S32) return (float)((const int*)clip)[k] * (1.f / 2147483648.f);
  if (FMT == S2I_PCM_F32) return ((const float*)clip)[k];
  return (float)((const double*)clip)[k];
}

// frame i -> mono: the channels added in channel order, then one correctly rounded division
template <int FMT>
__device__ __forceinline__ float decode_frame(const unsigned char* clip, long long i, int C) {
  float s = decode_sample<FMT>(clip, i * C);
  for (int c = 1; c < C; ++c) s += decode_sample<FMT>(clip, i * C + c);
  return __fdiv_rn(s, (float)C);
}

template <int FMT>
__global__ __launch_bounds__(256) void pcm_resample_kernel(
    const unsigned char* __restrict__ raw, const long long* __restrict__ boff, const int* __restrict__ frames, int B,
    int C, int L, int M, int W, int tpad, const float* __restrict__ table, const int* __restrict__ tiles,
    float* __restrict__ out, const long long* __restrict__ ooff, const int* __restrict__ olen, int window_cap) {
  extern __shared__ float win[];
  const int b = tiles[2 * blockIdx.x], m0 = tiles[2 * blockIdx.x + 1];
  if (b < 0 || b >= B) return;
  const int n = frames[b], nout = olen[b];
  if (n < 1 || m0 < 0 || m0 >= nout) return;
  const int cnt = min(TILE, nout - m0);
  const long long t0 = (long long)m0 * M;
  const long long q0 = t0 / L;
  const unsigned p0 = (unsigned)(t0 - q0 * L);
  const int taps = 2 * W + 2;
  const int wlen = min((int)((p0 + (unsigned)(cnt - 1) * (unsigned)M) / (unsigned)L) + taps, window_cap);
  const unsigned char* clip = raw + boff[b];
  const long long ws = q0 - W;
  for (int k = threadIdx.x; k < wlen; k += 256) {
    const long long src = ws + k;
    float v = 0.f;
    if (src >= 0 && src < n) v = decode_frame<FMT>(clip, src, C);
    win[k] = v;
  }
  __syncthreads();

  const long long nfull = (long long)n * L / M;       // outputs from here on are fix_length's padding
  float* ob = out + ooff[b] + m0;
  // Outputs i and i + L share a phase.  Work item w = (r, kg), r = w mod Lr the residue of i mod L (Lr = min(L, cnt))
  // and kg = w div Lr, owns the up to four outputs i_u = r + L (kg + KG u), u < 4, KG = ceil(ceil(cnt / L) / 4): one
  // f32x4 of the phase's row feeds all four.  With L = 1 this is i = t + 256 u.
  const int Lr = min(L, cnt);
  const int K = (cnt + L - 1) / L, KG = (K + 3) >> 2;
#pragma unroll 1
  for (int w = threadIdx.x; w < Lr * KG; w += 256) {
    const int kg = w / Lr, r = w - kg * Lr;
    const unsigned t = p0 + (unsigned)r * (unsigned)M;
    const unsigned dq0 = t / (unsigned)L, p = t - dq0 * (unsigned)L;
    const float* row = table + (size_t)p * tpad;
    const float* x[4];
    bool live[4];
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kg + KG * u;
      const int i = r + L * k;
      // output i reads win[dq0 + k M + j]; a dead slot (no such output, or fix_length's padding) reads output r's window
      live[u] = k < K && i < cnt && (long long)m0 + i < nfull && (int)dq0 + k * M + taps <= wlen;
      x[u] = win + dq0 + (live[u] ? k * M : 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[u][c] = 0.f;
    }
    if ((int)dq0 + taps <= wlen) {
      int j = 0;
      for (; j + 4 <= taps; j += 4) {
        const f32x4 h = *(const f32x4*)(row + j);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[u][0] = fmaf(x[u][j], h[0], acc[u][0]);
          acc[u][1] = fmaf(x[u][j + 1], h[1], acc[u][1]);
          acc[u][2] = fmaf(x[u][j + 2], h[2], acc[u][2]);
          acc[u][3] = fmaf(x[u][j + 3], h[3], acc[u][3]);
        }
      }
      if (j < taps) {                                   // taps is even: two taps are left when taps % 4 == 2
        const float h0 = row[j], h1 = row[j + 1];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc[u][0] = fmaf(x[u][j], h0, acc[u][0]);
          acc[u][1] = fmaf(x[u][j + 1], h1, acc[u][1]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kg + KG * u;
      const int i = r + L * k;
      if (k < K && i < cnt) ob[i] = live[u] ? (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]) : 0.f;
    }
  }
}

int gcd_int(int a, int b) {
  while (b) {
    const int r = a % b;
    a = b;
    b = r;
  }
  return a;
}

}  // namespace

extern "C" int s2i_pcm_resample(const void* raw, const long long* byte_offsets, const int* in_frames, int B, int format,
                                int channels, int L, int M, int W, const float* table, const int* tiles, int ntiles,
                                float* out, const long long* out_offsets, const int* out_lens, void* stream) {
  S2I_REQUIRE(raw && byte_offsets && in_frames && table && tiles && out && out_offsets && out_lens,
              "pcm_resample: null pointer");
  S2I_REQUIRE(B >= 1, "pcm_resample: bad clip count %d", B);
  S2I_REQUIRE(format >= S2I_PCM_U8 && format <= S2I_PCM_F64, "pcm_resample: unknown sample format %d", format);
  S2I_REQUIRE(channels >= 1 && channels <= 8, "pcm_resample: %d channels; need 1 to 8", channels);
  S2I_REQUIRE(L >= 1 && L <= OUT_RATE && M >= 1 && M <= MAX_RATIO * L && L <= 4 * M && gcd_int(L, M) == 1,
              "pcm_resample: L %d, M %d is not the reduced ratio of 16000 to a rate in [4000, 192000]", L, M);
  S2I_REQUIRE(W >= 0 && W <= MAX_W && (long long)L * (2 * W + 2) <= (1LL << 24),
              "pcm_resample: half width %d (L %d) is outside [0, %d] or its table is over 2^24 floats", W, L, MAX_W);
  S2I_REQUIRE(ntiles >= 1 && ntiles <= 0x7fffffff / 2, "pcm_resample: bad tile count %d", ntiles);
  S2I_REQUIRE(((uintptr_t)raw & 15) == 0, "pcm_resample: the byte buffer must be 16-byte aligned");
  S2I_REQUIRE((((uintptr_t)table | (uintptr_t)out) & 15) == 0, "pcm_resample: table and out must be 16-byte aligned");
  const int taps = 2 * W + 2, tpad = (taps + 3) & ~3;
  // the longest window of a tile: p0 <= L - 1, so (p0 + 1023 M) div L <= (L - 1 + 1023 M) div L
  const int window = (int)(((long long)(L - 1) + (long long)(S2I_RESAMPLE_TILE - 1) * M) / L) + taps;
  S2I_REQUIRE(window <= MAX_WINDOW, "pcm_resample: a tile's window of %d floats is over %d", window, MAX_WINDOW);
  const size_t lds = (size_t)window * sizeof(float);
  const unsigned char* r8 = (const unsigned char*)raw;
#define S2I_RESAMPLE_LAUNCH(F)                                                                                        \
  hipLaunchKernelGGL(pcm_resample_kernel<F>, dim3(ntiles), dim3(256), lds, (hipStream_t)stream, r8, byte_offsets,    \
                     in_frames, B, channels, L, M, W, tpad, table, tiles, out, out_offsets, out_lens, window)
  switch (format) {
    case S2I_PCM_U8: S2I_RESAMPLE_LAUNCH(S2I_PCM_U8); break;
    case S2I_PCM_S16: S2I_RESAMPLE_LAUNCH(S2I_PCM_S16); break;
    case S2I_PCM_S24: S2I_RESAMPLE_LAUNCH(S2I_PCM_S24); break;
    case S2I_PCM_S32: S2I_RESAMPLE_LAUNCH(S2I_PCM_S32); break;
    case S2I_PCM_F32: S2I_RESAMPLE_LAUNCH(S2I_PCM_F32); break;
    default: S2I_RESAMPLE_LAUNCH(S2I_PCM_F64); break;
  }
#undef S2I_RESAMPLE_LAUNCH
  S2I_LAUNCH_CHECK("pcm_resample");
  return 0;
}
