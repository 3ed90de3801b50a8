// Additive white noise and babble on a ragged batch of 16 kHz waveforms on gfx950, in place, each at a signal-to-noise
// ratio the host drew (include/s2i_hip.h has the definitions word for word).  x: the flat fp32 batch that s2i_pcm_resample
// wrote, clip b = x[offsets[b] .. offsets[b] + lens[b]); pool: the stored clips an interferer is read from; table: 32
// bytes per clip (WaveMixEntry).
//
//   y_i = (x_i + a_w e_i) + a_b v_i     every product and sum rounded to fp32 on its own (no fused multiply-add)
//   a_w = sqrtf(P_b g_white),  a_b = sqrtf(P_b g_babble),  P_b = S_b / (float)n,  n = lens[b]
//   e_i: Irwin-Hall of four 16-bit halves of Philox4x32-10 words, unit variance;  v_i = pool[src + (start + i) mod n_j]
//
// Power.  S_b is the fp32 sum of the clip's n squares (each square rounded, then added) in this fixed order, without
// atomics.  The clip is cut into runs of 8192 samples = 2048 four-sample pieces, counted from the clip's first sample.
// Thread j of a run's 256 adds pieces j, j + 256, ..., j + 1792 in that order, sample c of a piece into lane c of a four-lane
// accumulator that starts at 0 (a sample at or past n adds nothing); the lanes fold (a0 + a1) + (a2 + a3); the 64 lanes of
// a wave by an xor butterfly (offsets 32 .. 1); the four waves ((w0 + w1) + w2) + w3: the run sum, written to the
// workspace.  The second launch adds a clip's ceil(n / 8192) run sums: lane l of a wave adds runs l, l + 64, ... in that
// order starting at 0, then the same butterfly (every wave of every block repeats it and gets the same bits).  The run
// length is a constant, so S_b does not depend on the grid, on max_len, on the batch or on where the clip starts; a clip
// that starts on a 16-byte boundary is read and written in 16-byte pieces, any other one sample at a time, with the same
// sums.  P_b == 0 (or both gains 0) leaves the clip unwritten.
//
// Two launches, no LDS in the second, no synchronisation with the host.
#include "s2i_elementwise.h"
#include <stdint.h>

// every product and every sum below is rounded on its own: the definitions (and the bit-exact tests) say so.  The
// division and sqrtf must be the correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt, hipcc's default, which
// csrc/Makefile pins for this unit together with -ffp-contract=off); -ffast-math would break the header's wording.
#pragma clang fp contract(off)

namespace {
constexpr int WM_RUN_PIECES = 8;                      // pieces per thread of a run
constexpr int WM_RUN = 256 * WM_RUN_PIECES * 4;       // 8192 samples
constexpr int WM_TILE_PIECES = 4;                     // pieces per thread of a mix block
constexpr int WM_TILE = 256 * WM_TILE_PIECES * 4;     // 4096 samples
constexpr int WM_MAX_LEN = 0x7fffffff - 4;            // sample numbers and the noise counter 2 + i / 2 fit 32 bits
constexpr unsigned WM_KEY_XOR = 0x57415645u;          // into key word 1: no (key, counter) block is SpecAugment's

struct WaveMixEntry {  // the device table, 32 bytes per clip
  float g_white;       // 10^(-snr / 10); 0: no white noise
  float g_babble;      // 10^(-snr / 10) / Q_j; 0: no babble
  long long src;       // the interferer's first sample, in floats from `pool`
  int n_j;             // its length, >= 1 where g_babble != 0
  int start;           // in [0, n_j)
  unsigned uid;        // the clip's id in the noise counter
  int pad;
};
static_assert(sizeof(WaveMixEntry) == 32, "the table's layout is part of the ABI");

struct u32x4_ {
  unsigned v[4];
};

// s2i_specaug.hip's generator (Salmon et al. 2011)
__host__ __device__ inline u32x4_ philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0, c1 = (unsigned)p1, c2 = n2, c3 = (unsigned)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return u32x4_{{c0, c1, c2, c3}};
}

// ((float)h - 131070) c, h the sum of the four 16-bit halves of two words, c = fp32(1 / sqrt((2^32 - 1) / 3))
__device__ __forceinline__ float wm_noise(unsigned a, unsigned b) {
  const unsigned h = (a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16);
  return ((float)h - 131070.0f) * 0x1.bb67aep-16f;
}

__device__ __forceinline__ float wm_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int wm_len(const int* lens, int b, int max_len) {
  const int n = lens[b];
  return n < 0 ? 0 : (n > max_len ? max_len : n);
}

// the four samples from i0 on of a clip of n (zeros at and past n)
__device__ __forceinline__ f32x4 wm_load(const float* xb, bool aligned, unsigned i0, unsigned n) {
  if (aligned && i0 + 4 <= n) return ld4(xb + i0);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (i0 + c < n) v[c] = xb[i0 + c];
  return v;
}

// part[b * runs + r] = the sum of the squares of run r of clip b
__global__ __launch_bounds__(256) void wave_power_kernel(const float* __restrict__ x, const long long* __restrict__ offsets,
                                                         const int* __restrict__ lens, int B, int max_len, int runs,
                                                         float* __restrict__ part) {
  __shared__ float sh[4];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const unsigned n = (unsigned)wm_len(lens, b, max_len);
    const unsigned r0 = blockIdx.x * (unsigned)WM_RUN;
    if (r0 >= n) continue;  // the whole block leaves together
    const float* xb = x + offsets[b];
    const bool aligned = ((uintptr_t)xb & 15) == 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < WM_RUN_PIECES; ++k) {
      const unsigned i0 = r0 + (unsigned)(k * 256 + threadIdx.x) * 4;
      if (i0 >= n) break;
      const f32x4 v = wm_load(xb, aligned, i0, n);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = acc[c] + v[c] * v[c];
    }
    const float w = wm_wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)b * runs + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
  }
}

// a thread reads and writes its own pieces of x alone; pool is never written
__global__ __launch_bounds__(256) void wave_mix_kernel(float* x, const long long* __restrict__ offsets,
                                                       const int* __restrict__ lens, int B, int max_len, int runs,
                                                       const float* __restrict__ pool,
                                                       const WaveMixEntry* __restrict__ table, unsigned k0, unsigned k1,
                                                       unsigned c0, unsigned c1, const float* __restrict__ part) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const unsigned n = (unsigned)wm_len(lens, b, max_len);
    const unsigned t0 = blockIdx.x * (unsigned)WM_TILE;
    if (t0 >= n) continue;
    const WaveMixEntry e = table[b];
    const bool white = e.g_white != 0.f, babble = pool != nullptr && e.g_babble != 0.f && e.n_j >= 1;
    if (!white && !babble) continue;
    const unsigned nruns = (n + WM_RUN - 1) / WM_RUN;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (unsigned r = lane; r < nruns; r += 64) s = s + part[(long long)b * runs + r];
    s = wm_wave_sum(s);
    const float P = s / (float)n;
    if (P == 0.f) continue;
    const float aw = white ? sqrtf(P * e.g_white) : 0.f;
    const float ab = babble ? sqrtf(P * e.g_babble) : 0.f;
    float* xb = x + offsets[b];
    const bool aligned = ((uintptr_t)xb & 15) == 0;
    const float* pj = pool + e.src;
    const unsigned nj = babble ? (unsigned)e.n_j : 1u, start = babble ? (unsigned)e.start % nj : 0u;
#pragma unroll
    for (int k = 0; k < WM_TILE_PIECES; ++k) {
      const unsigned i0 = t0 + (unsigned)(k * 256 + threadIdx.x) * 4;
      if (i0 >= n) break;
      f32x4 v = wm_load(xb, aligned, i0, n);
      if (white) {
        const u32x4_ ra = philox4x32_10(c0, c1, e.uid, 2u + i0 / 2, k0, k1);
        const u32x4_ rb = philox4x32_10(c0, c1, e.uid, 3u + i0 / 2, k0, k1);
        v[0] = v[0] + aw * wm_noise(ra.v[0], ra.v[1]);
        v[1] = v[1] + aw * wm_noise(ra.v[2], ra.v[3]);
        v[2] = v[2] + aw * wm_noise(rb.v[0], rb.v[1]);
        v[3] = v[3] + aw * wm_noise(rb.v[2], rb.v[3]);
      }
      if (babble) {
        // start + i0 < 2^32: both are under 2^31
        unsigned q = (start + i0) % nj;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v[c] = v[c] + ab * pj[q];
          q = q + 1 == nj ? 0u : q + 1;
        }
      }
      if (aligned && i0 + 4 <= n) {
        st4(xb + i0, v);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (i0 + c < n) xb[i0 + c] = v[c];
      }
    }
  }
}

int wm_runs(int max_len) { return (int)(((long long)max_len + WM_RUN - 1) / WM_RUN); }
}  // namespace

extern "C" size_t s2i_wave_mix_workspace_bytes(int B, int max_len) {
  if (B < 1 || max_len < 1 || max_len > WM_MAX_LEN) return 0;
  return (size_t)B * (size_t)wm_runs(max_len) * sizeof(float);
}

extern "C" int s2i_wave_mix(float* x, const long long* offsets, const int* lens, int B, int max_len, const float* pool,
                            const void* table, unsigned long long seed, unsigned long long step, void* ws,
                            size_t ws_bytes, void* stream) {
  S2I_REQUIRE(x && offsets && lens && table, "wave_mix: null pointer");
  S2I_REQUIRE(B >= 1, "wave_mix: bad clip count %d", B);
  S2I_REQUIRE(max_len >= 1 && max_len <= WM_MAX_LEN, "wave_mix: max_len %d outside [1, 2^31 - 5]: a sample number must "
              "stay under 2^31 - 4", max_len);
  S2I_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)pool & 15) == 0, "wave_mix: x and pool must be 16-byte aligned");
  S2I_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)lens & 3) == 0 && ((uintptr_t)table & 15) == 0,
              "wave_mix: offsets must be 8-byte, lens 4-byte and the table 16-byte aligned");
  S2I_REQUIRE(ws && ((uintptr_t)ws & 3) == 0 && ws_bytes >= s2i_wave_mix_workspace_bytes(B, max_len),
              "wave_mix: workspace too small");
  const int runs = wm_runs(max_len);
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  hipLaunchKernelGGL(wave_power_kernel, dim3((unsigned)runs, gy), dim3(256), 0, ST, (const float*)x, offsets, lens, B,
                     max_len, runs, (float*)ws);
  S2I_LAUNCH_CHECK("wave_power");
  const unsigned tiles = (unsigned)(((long long)max_len + WM_TILE - 1) / WM_TILE);
  hipLaunchKernelGGL(wave_mix_kernel, dim3(tiles, gy), dim3(256), 0, ST, x, offsets, lens, B, max_len, runs, pool,
                     (const WaveMixEntry*)table, (unsigned)seed, (unsigned)(seed >> 32) ^ WM_KEY_XOR, (unsigned)step,
                     (unsigned)(step >> 32), (const float*)ws);
  S2I_LAUNCH_CHECK("wave_mix");
  return 0;
}
