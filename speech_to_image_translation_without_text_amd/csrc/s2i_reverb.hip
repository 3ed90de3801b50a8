// Room reverberation of a ragged batch of 16 kHz waveforms on gfx950: each clip convolved with a room impulse response
// (RIR) of up to 16000 taps that is written on the device from the host's draws (include/s2i_hip.h has the definitions
// word for word).  x, y: two flat fp32 batches with one set of offsets, clip b = [offsets[b] .. offsets[b] + lens[b]);
// table: 16 bytes per clip (ReverbEntry); h: [B][max_taps].
//
//   h[0] = 1,  h[k] = (alpha e_k) env_k for 1 <= k < taps,  env_k = exp2f((float)k slope),  0 from taps on
//   y_i = sum_k h[k] x_{i - k},  i in [0, n)                 (taps == 0: y_i = x_i bit for bit)
//
// The convolution is a block-Toeplitz product on v_mfma_f32_32x32x2_f32.  With X[m][a] = x[32 a + m] (a clip cut into
// blocks of 32 samples, zero outside [0, n)),
//   Y[:, a] = sum_{j = 0}^{taps / 32} W_j X[:, a - j],   W_j[b][m] = h[32 j + b - m]   (h zero outside [0, taps)):
// a dense 32 x 32 matrix per block of 32 taps, so no product is wasted apart from the two end blocks of h.  W_j is never
// stored: lane l of a wave reads the A fragment of the k-pair (m, m + 1) from the h chunk in LDS at index
// 32 j + (l & 31) - m - (l >> 5), consecutive addresses across 32 lanes.  The B fragment is X[m + (l >> 5)][a0 + (l & 31) - j],
// a stride of one block across lanes; the x window is staged with rows of 33 floats, which spreads the 32 lanes of a half
// over 32 banks (33 is odd).
//
// Order of the sum (part of the ABI): output 32 a + b has ONE accumulator that starts at 0 and takes
// fmaf(h[32 j + b - m], x[32 (a - j) + m], acc) for j = 0, 1, ..., taps / 32 and inside a j for m = 0, 1, ..., 31: the
// instruction's own two k in order, the sixteen k-pairs in order, the j in order.  Blocks with j > a multiply samples before
// the clip (zeros) and are skipped; a product with a zero of the padding adds +-0 and changes nothing.  Nothing in that
// order depends on the tile, the grid, max_len, the batch or where the clip starts.
//
// One workgroup of 4 waves per (clip, tile of 8192 outputs = 256 blocks); wave w owns the 64 block columns
// [64 w, 64 w + 64) of the tile in two 32 x 32 accumulators.  The taps are walked in chunks of 32 blocks (1024 taps): a
// chunk stages (256 + 31) blocks of x and 1024 + 64 taps of h, 42.3 KB of LDS together, then issues 32 x 16 x 2 MFMAs per
// wave: the staging is 36 floats per thread against 65 536 MFMA cycles.
#include "s2i_elementwise.h"
#include <stdint.h>

// the RIR's products are each rounded on their own (csrc/Makefile pins -ffp-contract=off for this unit as well)
#pragma clang fp contract(off)

namespace {
constexpr int RV_MAX_TAPS = 16000;
constexpr int RV_MAX_LEN = 0x7fffffff - 8192 - 32;    // a tile's last sample number fits 32 bits
constexpr unsigned RV_KEY_XOR = 0x52455642u;          // "REVB" into key word 1: no block is SpecAugment's or the mix's
constexpr int RV_NB = 256;                            // blocks of 32 outputs per tile
constexpr int RV_TILE = RV_NB * 32;                   // 8192 outputs
constexpr int RV_JC = 32;                             // tap blocks per chunk
constexpr int RV_TN = 2;                              // accumulators (groups of 32 block columns) per wave
constexpr int RV_XROWS = RV_NB + RV_JC - 1;           // blocks of x a chunk multiplies
constexpr int RV_LDX = 33;                            // floats per staged block: lanes one block apart, one bank apart
constexpr int RV_HS = 32 * RV_JC + 64;                // taps a chunk multiplies: 32 before its first block, 32 after its last
static_assert(RV_NB == 4 * RV_TN * 32, "four waves of RV_TN accumulators cover a tile");

struct ReverbEntry {  // the device table, 16 bytes per clip
  float alpha;        // gain of the tail
  float slope;        // log2 of the envelope per tap, < 0
  int taps;           // 0: the clip is copied; else a multiple of 32 in [32, 16000]
  unsigned uid;       // the clip's id in the counter
};
static_assert(sizeof(ReverbEntry) == 16, "the table's layout is part of the ABI");

struct u32x4_ {
  unsigned v[4];
};

// s2i_specaug.hip's generator (Salmon et al. 2011)
__device__ inline u32x4_ philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0, c1 = (unsigned)p1, c2 = n2, c3 = (unsigned)p0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return u32x4_{{c0, c1, c2, c3}};
}

// s2i_wave_mix's e: ((float)h - 131070) c, h the sum of the four 16-bit halves of two words
__device__ __forceinline__ float rv_noise(unsigned a, unsigned b) {
  const unsigned h = (a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16);
  return ((float)h - 131070.0f) * 0x1.bb67aep-16f;
}

__device__ __forceinline__ int rv_taps(const ReverbEntry& e, int max_taps) {
  return e.taps < 0 ? 0 : (e.taps > max_taps ? max_taps : e.taps);
}

// h[b][k], one thread per tap
__global__ __launch_bounds__(256) void reverb_rir_kernel(const ReverbEntry* __restrict__ table, int B, int max_taps,
                                                         float* __restrict__ h, unsigned k0, unsigned k1, unsigned c0,
                                                         unsigned c1) {
  const int k = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= max_taps) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const ReverbEntry e = table[b];
    const int taps = rv_taps(e, max_taps);
    float v = 0.f;
    if (k < taps) {
      if (k == 0) {
        v = 1.f;
      } else {
        const u32x4_ r = philox4x32_10(c0, c1, e.uid, 1u + (unsigned)k / 2, k0, k1);
        const float n = (k & 1) ? rv_noise(r.v[2], r.v[3]) : rv_noise(r.v[0], r.v[1]);
        const float env = exp2f((float)k * e.slope);
        v = (e.alpha * n) * env;
      }
    }
    h[(long long)b * max_taps + k] = v;
  }
}

__global__ __launch_bounds__(256) void reverb_kernel(const float* __restrict__ x, const long long* __restrict__ offsets,
                                                     const int* __restrict__ lens, int B, int max_len,
                                                     const ReverbEntry* __restrict__ table, const float* __restrict__ h,
                                                     int max_taps, float* __restrict__ y) {
  __shared__ float xs[RV_XROWS * RV_LDX];
  __shared__ float hs[RV_HS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    int n = lens[b];
    n = n < 0 ? 0 : (n > max_len ? max_len : n);
    const int t0 = (int)blockIdx.x * RV_TILE;  // the tile's first output
    if (t0 >= n) continue;                     // the whole block leaves together
    const long long off = offsets[b];
    const float* xb = x + off;
    float* yb = y + off;
    const int taps = rv_taps(table[b], max_taps);
    if (taps == 0) {
      for (int i = t0 + tid; i < n && i < t0 + RV_TILE; i += 256) yb[i] = xb[i];
      continue;
    }
    const float* hb = h + (long long)b * max_taps;
    const int a0 = t0 >> 5;                                        // the tile's first block
    const int last = ((n < t0 + RV_TILE ? n : t0 + RV_TILE) - 1) >> 5;  // its last block with an output
    const int J = taps >> 5;
    const int jend = (J < last ? J : last) + 1;                    // j in [0, jend)
    f32x16 acc[RV_TN];
#pragma unroll
    for (int t = 0; t < RV_TN; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    for (int j0 = 0; j0 < jend; j0 += RV_JC) {
      __syncthreads();  // the last chunk's (or clip's) reads are done
      // hs[t] = h[32 j0 - 32 + t]
      for (int t = tid; t < RV_HS; t += 256) {
        const int k = 32 * j0 - 32 + t;
        hs[t] = (k >= 0 && k < taps) ? hb[k] : 0.f;
      }
      // row r of xs = block a0 - (j0 + RV_JC - 1) + r of the clip
      const int s0 = (a0 - (j0 + RV_JC - 1)) * 32;  // its first sample, negative before the clip
      for (int t = tid; t < RV_XROWS * 32; t += 256) {
        const int i = s0 + t;
        xs[(t >> 5) * RV_LDX + (t & 31)] = (i >= 0 && i < n) ? xb[i] : 0.f;
      }
      __syncthreads();
      const int jc = jend - j0 < RV_JC ? jend - j0 : RV_JC;
      for (int jj = 0; jj < jc; ++jj) {
        const int j = j0 + jj;
        // A: h[32 j + i - m - k] = hs[32 jj + 32 + i - m - k], i = l31, k = lh, for m = 0, 2, ..., 30
        const float* ap = hs + 32 * jj + 32 + l31 - lh;
        float af[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) af[p] = ap[-2 * p];
#pragma unroll
        for (int t = 0; t < RV_TN; ++t) {
          const int g = wave * RV_TN + t;              // columns a0 + 32 g + (0 .. 31)
          if (j > a0 + 32 * g + 31) continue;          // every block a - j lies before the clip (wave-uniform)
          if (a0 + 32 * g > last) continue;            // no output in these columns
          // B: X[m + k][a - j] = xs[(32 g + l31 + RV_JC - 1 - jj) * RV_LDX + m + k]
          const float* bp = xs + (32 * g + l31 + RV_JC - 1 - jj) * RV_LDX + lh;
          float bf[16];
#pragma unroll
          for (int p = 0; p < 16; ++p) bf[p] = bp[2 * p];
#pragma unroll
          for (int p = 0; p < 16; ++p) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[p], bf[p], acc[t], 0, 0, 0);
        }
      }
    }
    // C: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of column l & 31
    const bool aligned = ((uintptr_t)yb & 15) == 0;
#pragma unroll
    for (int t = 0; t < RV_TN; ++t) {
      const int a = a0 + 32 * (wave * RV_TN + t) + l31;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 32 * a + 8 * q + 4 * lh;
        if (i >= n) continue;
        if (aligned && i + 4 <= n) {
          st4(yb + i, f32x4{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]});
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (i + c < n) yb[i + c] = acc[t][4 * q + c];
        }
      }
    }
  }
}
}  // namespace

extern "C" int s2i_reverb_rir(const void* table, int B, int max_taps, float* h, unsigned long long seed,
                              unsigned long long step, void* stream) {
  S2I_REQUIRE(table && h, "reverb_rir: null pointer");
  S2I_REQUIRE(B >= 1, "reverb_rir: bad clip count %d", B);
  S2I_REQUIRE(max_taps >= 32 && max_taps <= RV_MAX_TAPS && max_taps % 32 == 0,
              "reverb_rir: max_taps %d is not a multiple of 32 in [32, %d]", max_taps, RV_MAX_TAPS);
  S2I_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)h & 15) == 0, "reverb_rir: table and h must be 16-byte aligned");
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  hipLaunchKernelGGL(reverb_rir_kernel, dim3((unsigned)((max_taps + 255) / 256), gy), dim3(256), 0, ST,
                     (const ReverbEntry*)table, B, max_taps, h, (unsigned)seed, (unsigned)(seed >> 32) ^ RV_KEY_XOR,
                     (unsigned)step, (unsigned)(step >> 32));
  S2I_LAUNCH_CHECK("reverb_rir");
  return 0;
}

extern "C" int s2i_reverb(const float* x, const long long* offsets, const int* lens, int B, int max_len, const void* table,
                          const float* h, int max_taps, float* y, void* stream) {
  S2I_REQUIRE(x && offsets && lens && table && h && y, "reverb: null pointer");
  S2I_REQUIRE(B >= 1, "reverb: bad clip count %d", B);
  S2I_REQUIRE(max_len >= 1 && max_len <= RV_MAX_LEN, "reverb: max_len %d outside [1, %d]", max_len, RV_MAX_LEN);
  S2I_REQUIRE(max_taps >= 32 && max_taps <= RV_MAX_TAPS && max_taps % 32 == 0,
              "reverb: max_taps %d is not a multiple of 32 in [32, %d]", max_taps, RV_MAX_TAPS);
  S2I_REQUIRE(x != y && (const float*)y != h, "reverb: y must be apart from x and h");
  S2I_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)h & 15) == 0,
              "reverb: x, y and h must be 16-byte aligned");
  S2I_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)lens & 3) == 0 && ((uintptr_t)table & 15) == 0,
              "reverb: offsets must be 8-byte, lens 4-byte and the table 16-byte aligned");
  const unsigned tiles = (unsigned)(((long long)max_len + RV_TILE - 1) / RV_TILE);
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  hipLaunchKernelGGL(reverb_kernel, dim3(tiles, gy), dim3(256), 0, ST, x, offsets, lens, B, max_len,
                     (const ReverbEntry*)table, h, max_taps, y);
  S2I_LAUNCH_CHECK("reverb");
  return 0;
}
