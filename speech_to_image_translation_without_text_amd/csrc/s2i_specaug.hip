// SpecAugment (Park et al. 2019) of a log-mel training batch on gfx950: frequency and time masks drawn and applied on the
// device, the masked cells set to the utterance's own mean.  x, y: fp32 [B][T][40]; valid[b] = n: the leading rows of
// utterance b that the masks may touch (clamped to [0, T]); rows at or after n are copied unchanged.
//
// Draws.  Nothing is uploaded: utterance b has 2 (freq_masks + time_masks) uniforms u_0, u_1, ... from Philox4x32-10
// (Salmon et al. 2011).  Group g (g = 0, 1, ...) is the block
//   key k = (seed mod 2^32, seed div 2^32),  counter c = (step mod 2^32, step div 2^32, b, g)
// run through ten rounds; a round maps (c0, c1, c2, c3) to
//   (hi(0xCD9E8D57 c2) ^ c1 ^ k0,  lo(0xCD9E8D57 c2),  hi(0xD2511F53 c0) ^ c3 ^ k1,  lo(0xD2511F53 c0))
// with hi / lo the halves of the 64-bit product, and between two rounds (nine times) k0 += 0x9E3779B9, k1 += 0xBB67AE85
// mod 2^32.  The four output words r_0..r_3 of group g give u_{4g + i} = (float)(r_i >> 8) * 2^-24: 24 bits, exact in
// fp32, in [0, 1).  Mask k (the frequency masks first, k = 0 .. freq_masks - 1, then the time masks) takes u = u_{2k} and
// u' = u_{2k+1}.  The same (seed, step, b) gives the same masks on any grid, in any batch.
//
// Masks (int() truncates one fp32 product, as s2i_diffaug_forward's offsets):
//   frequency: f = min(int(u (float)(freq_width + 1)), freq_width);  f0 = min(int(u' (float)(40 - f + 1)), 40 - f);
//              bins [f0, f0 + f) of rows [0, n)
//   time:      W = min(time_width, int(time_ratio (float)n));  t = min(int(u (float)(W + 1)), W);
//              t0 = min(int(u' (float)(n - t + 1)), n - t);  rows [t0, t0 + t), all 40 bins.  n == 0 or W == 0: nothing.
//
// Masked value: m_b = S_b / (float)(40 n), S_b the fp32 sum of the utterance's 40 n unmasked inputs, in this fixed order
// (no atomics: the same inputs give the same bits).  The 10 n sixteen-byte pieces of rows [0, n) are cut into
// segs = min(64, max(1, 10 T div 1024)) runs of chunk = ceil(10 n / segs) consecutive pieces, one 256-thread block each.
// Thread j of a block adds pieces j, j + 256, ... of its run, in that order, into a four-lane accumulator that starts at 0;
// the lanes are folded (a0 + a1) + (a2 + a3); the 64 lanes of a wave by an xor butterfly (offsets 32, 16, 8, 4, 2, 1);
// the four waves as ((w0 + w1) + w2) + w3; the segs run sums, padded with zeros to 64, by the same butterfly in the
// second launch.  Depth: a term passes through at most d = ceil(chunk / 256) + 2 + 6 + 3 + 6 additions;
// over n <= T that is d(T) = ceil(ceil(10 T / segs) / 256) + 17  (22 at T = 128, 21 at T = 2048).  T <= 419430, so that
// 40 n < 2^24 and (float)n, (float)(40 n) are exact.
//
// Launches: the run sums into the workspace, then a copy-or-mask in 16-byte pieces (a 160-byte row is ten pieces, the bin
// test is per lane of the piece); with x == y only pieces that hold a masked cell are written.  A block of the second
// launch first draws its utterance's masks (wave 0, one Philox block per lane; the frequency masks become one 40-bit word
// by an or-butterfly, the time masks eight row ranges, unused ones empty) and folds the run sums (wave 1); a thread then
// takes four pieces, 256 apart, loaded before that prelude, and tests each without a branch or an LDS read: the eight row
// ranges sit in registers.  (Testing mask by mask out of LDS, with short-circuit compares, cost 21 - 23 us at B = 64,
// T = 2048 against 9.5 us for the gather launch that moves the same bytes: DESIGN.md 8b4a.)  Without masks the first
// launch is skipped, and with x == y both are.
#include "s2i_elementwise.h"
#include <stdint.h>

namespace {
constexpr int SA_BINS = 40;
constexpr int SA_ROW_PIECES = SA_BINS * 4 / 16;  // a 160-byte row is ten f32x4
constexpr int SA_MAX_MASKS = 8;                  // of each kind
constexpr int SA_MAX_SEGS = 64;
constexpr int SA_PIECES = 4;                     // pieces per thread of the apply launch
constexpr int SA_MAX_ROWS = ((1 << 24) - 1) / SA_BINS;  // 419430
static_assert(SA_ROW_PIECES * 16 == SA_BINS * 4, "a log-mel row must be whole 16-byte pieces");

struct SpecAugPolicy {
  int freq_masks, freq_width, time_masks, time_width;
  float time_ratio;
};

struct u32x4_ {
  unsigned v[4];
};

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

__host__ __device__ inline float sa_uniform(unsigned bits) { return (float)(bits >> 8) * 5.9604644775390625e-8f; }

__host__ __device__ inline int sa_draw(float u, int n) {
  const int v = (int)(u * (float)n);  // one fp32 multiply, truncated
  return v < n - 1 ? v : n - 1;
}

// mask k of utterance b, n rows of which may be touched -> [lo, hi): bins for k < freq_masks, rows for the rest
__host__ __device__ inline void sa_mask(const SpecAugPolicy& p, unsigned long long seed, unsigned long long step, int b,
                                        int n, int k, int& lo, int& hi) {
  const u32x4_ r = philox4x32_10((unsigned)step, (unsigned)(step >> 32), (unsigned)b, (unsigned)(k >> 1), (unsigned)seed,
                                 (unsigned)(seed >> 32));
  const float u = sa_uniform(k & 1 ? r.v[2] : r.v[0]), u2 = sa_uniform(k & 1 ? r.v[3] : r.v[1]);
  if (k < p.freq_masks) {
    const int f = sa_draw(u, p.freq_width + 1);
    lo = sa_draw(u2, SA_BINS - f + 1);
    hi = lo + f;
  } else {
    const int lim = (int)(p.time_ratio * (float)n);
    const int W = p.time_width < lim ? p.time_width : lim;
    const int t = sa_draw(u, W + 1);
    lo = sa_draw(u2, n - t + 1);
    hi = lo + t;
  }
}

__host__ __device__ inline int sa_rows(const int* valid, int b, int T) {
  const int n = valid[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

__device__ __forceinline__ float sa_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// part[b][seg] = the sum of run `seg` of utterance b's 10 n leading pieces
__global__ __launch_bounds__(256) void specaug_sum_kernel(const float* __restrict__ x, const int* __restrict__ valid, int B,
                                                          int T, int segs, float* __restrict__ part) {
  __shared__ float sh[4];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long n4 = (long long)sa_rows(valid, b, T) * SA_ROW_PIECES;
    const long long chunk = (n4 + segs - 1) / segs;
    const long long i0 = (long long)blockIdx.x * chunk, i1 = min(n4, i0 + chunk);
    const float* p = x + (long long)b * T * SA_BINS;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) acc += ld4(p + i * 4);
    float v = sa_wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)b * SA_MAX_SEGS + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
  }
}

// x and y may be one buffer (INPLACE): a thread reads and writes its own piece alone
template <bool INPLACE>
__global__ __launch_bounds__(256) void specaug_apply_kernel(const float* x, const int* __restrict__ valid, int B, int T,
                                                            float* y, SpecAugPolicy pol, unsigned long long seed,
                                                            unsigned long long step, int segs,
                                                            const float* __restrict__ part) {
  __shared__ int tlo[SA_MAX_MASKS], thi[SA_MAX_MASKS];  // the time masks' rows; an unused entry is empty
  __shared__ unsigned long long fbits;                  // bit i: bin i is inside a frequency mask
  __shared__ float mean;
  const int nmask = pol.freq_masks + pol.time_masks;
  const unsigned per = (unsigned)T * SA_ROW_PIECES;     // T <= SA_MAX_ROWS: a piece number fits 32 bits
  // this thread's SA_PIECES pieces of every utterance, 256 apart inside the block's run of 256 SA_PIECES
  const unsigned p0 = blockIdx.x * (256 * SA_PIECES) + threadIdx.x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* xb = x + (long long)b * per * 4;
    float* yb = y + (long long)b * per * 4;
    // every load goes out before the masks are known (a piece past the utterance's end re-reads its last one)
    f32x4 s[SA_PIECES];
#pragma unroll
    for (int j = 0; j < SA_PIECES; ++j) s[j] = ld4(xb + (long long)min(p0 + j * 256, per - 1) * 4);
    const int n = sa_rows(valid, b, T);
    if (threadIdx.x < 64) {  // wave 0 draws the masks, one per lane
      const int k = threadIdx.x;
      int lo = 0, hi = 0;
      if (k < nmask) sa_mask(pol, seed, step, b, n, k, lo, hi);
      unsigned long long bits = k < pol.freq_masks ? (1ull << hi) - (1ull << lo) : 0ull;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, 64);
      if (k == 0) fbits = bits;
      const int j = k - pol.freq_masks;
      if (j >= 0 && j < SA_MAX_MASKS) {
        tlo[j] = j < pol.time_masks ? lo : 0;
        thi[j] = j < pol.time_masks ? hi : 0;
      }
    } else if (threadIdx.x < 128 && nmask > 0) {  // wave 1 adds the run sums
      const int l = threadIdx.x - 64;
      const float sum = sa_wave_sum(l < segs ? part[(long long)b * SA_MAX_SEGS + l] : 0.f);
      if (l == 0) mean = n > 0 ? sum / (float)((long long)SA_BINS * n) : 0.f;
    }
    __syncthreads();
    const unsigned long long fb = fbits;
    const float m = mean;
    int lo[SA_MAX_MASKS], hi[SA_MAX_MASKS];
#pragma unroll
    for (int k = 0; k < SA_MAX_MASKS; ++k) lo[k] = tlo[k], hi[k] = thi[k];
#pragma unroll
    for (int j = 0; j < SA_PIECES; ++j) {
      const unsigned p = p0 + j * 256;
      if (p >= per) break;
      const int t = (int)(p / SA_ROW_PIECES), bin0 = (int)(p - (unsigned)t * SA_ROW_PIECES) * 4;
      bool row = false;  // inside a time mask (their rows lie in [0, n))
#pragma unroll
      for (int k = 0; k < SA_MAX_MASKS; ++k) row |= (t >= lo[k]) & (t < hi[k]);
      // bit c: bin bin0 + c of this row is masked
      const unsigned lanes = row ? 15u : (t < n ? (unsigned)(fb >> bin0) & 15u : 0u);
      if (INPLACE && lanes == 0) continue;
      f32x4 v = s[j];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (lanes >> c & 1) v[c] = m;
      st4(yb + p * 4, v);
    }
    __syncthreads();
  }
}

int sa_segments(int T) {
  const long long s = (long long)T * SA_ROW_PIECES / 1024;
  return s < 1 ? 1 : (s > SA_MAX_SEGS ? SA_MAX_SEGS : (int)s);
}
}  // namespace

extern "C" size_t s2i_specaug_workspace_bytes(int B) {
  if (B < 1) return 0;
  return (size_t)B * SA_MAX_SEGS * sizeof(float);
}

extern "C" int s2i_specaug(const float* x, const int* valid, int B, int T, float* y, int freq_masks, int freq_width,
                           int time_masks, int time_width, float time_ratio, unsigned long long seed,
                           unsigned long long step, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE(x && valid && y, "specaug: null pointer");
  S2I_REQUIRE(B >= 1 && T >= 1, "specaug: bad shape (B %d, T %d)", B, T);
  S2I_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "specaug: x and y must be 16-byte aligned");
  S2I_REQUIRE(freq_masks >= 0 && freq_masks <= SA_MAX_MASKS && time_masks >= 0 && time_masks <= SA_MAX_MASKS,
              "specaug: mask counts must lie in [0, %d], got %d and %d", SA_MAX_MASKS, freq_masks, time_masks);
  S2I_REQUIRE(freq_width >= 0 && freq_width <= SA_BINS / 2, "specaug: freq_width %d outside [0, %d]", freq_width,
              SA_BINS / 2);
  S2I_REQUIRE(time_width >= 0, "specaug: time_width %d < 0", time_width);
  S2I_REQUIRE(time_ratio > 0.f && time_ratio <= 1.f, "specaug: time_ratio %g outside (0, 1]", (double)time_ratio);
  // 40 T < 2^24: (float)n and (float)(40 n) are exact, and the ten pieces of T rows fit one grid
  S2I_REQUIRE(T <= SA_MAX_ROWS, "specaug: T %d is too large for one launch (at most %d rows)", T, SA_MAX_ROWS);
  const long long per = (long long)T * SA_ROW_PIECES;
  const bool masks = freq_masks + time_masks > 0;
  if (masks) S2I_REQUIRE(ws && ws_bytes >= s2i_specaug_workspace_bytes(B), "specaug: workspace too small");
  if (!masks && x == y) return 0;
  const int segs = sa_segments(T);
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  if (masks) {
    hipLaunchKernelGGL(specaug_sum_kernel, dim3((unsigned)segs, gy), dim3(256), 0, ST, x, valid, B, T, segs, (float*)ws);
    S2I_LAUNCH_CHECK("specaug_sum");
  }
  const SpecAugPolicy pol = {freq_masks, freq_width, time_masks, time_width, time_ratio};
  const dim3 grid((unsigned)((per + 256 * SA_PIECES - 1) / (256 * SA_PIECES)), gy);
  if (x == y)
    hipLaunchKernelGGL(specaug_apply_kernel<true>, grid, dim3(256), 0, ST, x, valid, B, T, y, pol, seed, step, segs,
                       (const float*)ws);
  else
    hipLaunchKernelGGL(specaug_apply_kernel<false>, grid, dim3(256), 0, ST, x, valid, B, T, y, pol, seed, step, segs,
                       (const float*)ws);
  S2I_LAUNCH_CHECK("specaug_apply");
  return 0;
}
