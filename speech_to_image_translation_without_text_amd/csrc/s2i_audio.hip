// Speech front end (Audio_to_Image/utils.py:292-340, load_one_audio_file): mean removal, pre-emphasis, reflect-padded
// Hamming STFT, power, 40-band Slaney mel projection and power_to_db(ref=max, top_db=80) over a ragged batch of
// utterances.  fp32 throughout; the DFT is one GEMM on v_mfma_f32_16x16x4_f32 against a window-folded basis.
#include "s2i_common.h"

namespace {

constexpr int NFFT = S2I_LOGMEL_NFFT;            // 400 samples per frame (n_fft = win_length)
constexpr int HOP = S2I_LOGMEL_HOP;              // 160
constexpr int NBIN = NFFT / 2 + 1;               // 201
constexpr int NMEL = S2I_LOGMEL_NMEL;            // 40
constexpr int FT = S2I_LOGMEL_TILE_FRAMES;       // 64 frames per block
constexpr int NPT = 13;                          // 16-wide pair tiles: pair q = (cos q, sin q), q = 1..199; q = 0 holds
                                                 // (cos 0, cos 200); q = 200..207 are zero columns
constexpr int NKG = NFFT / 16;                   // 25 groups of four 4-deep K steps
// LDS image of the padded signal: sample p of the tile sits at p + 2 * (p / HOP).  Frame f starts at f * 162, and
// 162 mod 32 = 2, so the 16 frames x 2 k of a 32-lane ds_read_b32 group land on 32 distinct banks (at a plain stride of
// 160 they would share one bank per k: 16-way).
constexpr int SEG = HOP + 2;
constexpr int SPAN = (FT - 1) * HOP + NFFT;      // samples a full tile reads
constexpr int LDS_SIG = (SPAN + HOP - 1) / HOP * SEG;
// power image [frame][PSTR]: PSTR = 4 mod 8, so a 32-lane write of 16 bins x rows {r, r + 4} is conflict-free
constexpr int PSTR = 204;
constexpr int LDS_POW = FT * PSTR;
constexpr int LDS_F = LDS_POW > LDS_SIG ? LDS_POW : LDS_SIG;

// np.pad(y, n, 'reflect') for any n: the even periodic extension of period 2 (L - 1)
__device__ __forceinline__ int reflect_index(int j, int L) {
  if (L == 1) return 0;
  const int P = 2 * (L - 1);
  j %= P;
  if (j < 0) j += P;
  return j < L ? j : P - j;
}

// one block per utterance: mean in fp64; also clears the utterance's max (consumed by logmel_power's atomicMax)
__global__ __launch_bounds__(256) void signal_mean_kernel(const float* __restrict__ x, const long long* __restrict__ off,
                                                          const int* __restrict__ lens, float* __restrict__ mean,
                                                          unsigned* __restrict__ maxbits) {
  __shared__ double red[4];
  const int b = blockIdx.x, L = lens[b];
  const float* xb = x + off[b];
  double s = 0.0;
  for (int i = threadIdx.x; i < L; i += 256) s += (double)xb[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    mean[b] = L > 0 ? (float)((red[0] + red[1] + red[2] + red[3]) / (double)L) : 0.f;
    maxbits[b] = 0u;
  }
}

// One block per tile-table entry (utterance b, first frame f0): up to 64 frames of one utterance.
//   1. the tile's span of the reflect-padded, mean-removed, pre-emphasised signal -> LDS (pre-emphasis is taken at the
//      reflected source index, i.e. before padding, as the reference does);
//   2. [64 frames x 400 samples] x basis [400 x 416] on v_mfma_f32_16x16x4_f32.  Wave w computes frames
//      [32 (w & 1), +32) against pair tiles [7 (w >> 1), +7 or +6); a pair tile's cos and sin accumulators hold the same
//      (frame, bin) in the same lane, so re^2 + im^2 forms in registers;
//   3. power -> LDS, the 40 mel sums over each filter's bin range, written for frames < T; every frame's sums go into
//      the utterance's max (atomicMax on the bits: the sums are >= 0).
__global__ __launch_bounds__(256) void logmel_power_kernel(
    const float* __restrict__ x, const long long* __restrict__ off, const int* __restrict__ lens, int B,
    const float* __restrict__ mean, const f32x4* __restrict__ basis, const float* __restrict__ bank,
    const int* __restrict__ mrange, const int* __restrict__ tiles, int T, float* __restrict__ melpow,
    unsigned* __restrict__ maxbits) {
  __shared__ float lds[LDS_F];
  __shared__ float red[4];
  const int b = tiles[2 * blockIdx.x], f0 = tiles[2 * blockIdx.x + 1];
  if (b < 0 || b >= B) return;
  const int L = lens[b];
  const int nf = 1 + L / HOP;
  if (L < 1 || f0 < 0 || f0 >= nf) return;
  const float* xb = x + off[b];
  const float m = mean[b];
  const int p0 = f0 * HOP - NFFT / 2;
  for (int p = threadIdx.x; p < SPAN; p += 256) {
    const int j = reflect_index(p0 + p, L);
    const float v = xb[j] - m;
    lds[p + 2 * (p / HOP)] = j == 0 ? v : v - 0.97f * (xb[j - 1] - m);
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int fbase = 32 * (wave & 1);
  const int t0 = 7 * (wave >> 1), nt = (wave >> 1) ? NPT - 7 : 7;
  f32x4 acc[7][2][2];
#pragma unroll
  for (int t = 0; t < 7; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) acc[t][h][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kg = 0; kg < NKG; ++kg) {
    // K step u of this group: lane group g supplies k = 16 kg + 4 u + g (the packed basis uses the same order)
    float a[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = 16 * kg + 4 * u + g;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[u][mt] = lds[(fbase + 16 * mt + i) * SEG + k + 2 * (k / HOP)];
    }
    const f32x4* bk = basis + (size_t)kg * (2 * NPT) * 64 + lane;
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      if (t < nt) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 bv = bk[(2 * (t0 + t) + h) * 64];
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
              acc[t][h][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][mt], bv[u], acc[t][h][mt], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();  // the signal image is dead: the power image reuses the buffer

#pragma unroll
  for (int t = 0; t < 7; ++t) {
    if (t < nt) {
      const int q = 16 * (t0 + t) + i;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* row = lds + (fbase + 16 * mt + 4 * g + r) * PSTR;   // C/D map: col = lane & 15, row = 4 (lane >> 4) + r
          const float c = acc[t][0][mt][r], s = acc[t][1][mt][r];
          if (q == 0) {
            row[0] = c * c;
            row[NBIN - 1] = s * s;
          } else if (q < NBIN - 1) {
            row[q] = fmaf(c, c, s * s);
          }
        }
    }
  }
  __syncthreads();

  const int nvalid = min(FT, nf - f0);
  float vmax = 0.f;
  for (int idx = threadIdx.x; idx < nvalid * NMEL; idx += 256) {
    const int fr = idx / NMEL, mm = idx - fr * NMEL;
    const float* prow = lds + fr * PSTR;
    const float* brow = bank + mm * NBIN;
    float sum = 0.f;
    const int lo = max(mrange[2 * mm], 0), hi = min(mrange[2 * mm + 1], NBIN);
    for (int k = lo; k < hi; ++k) sum = fmaf(brow[k], prow[k], sum);
    vmax = fmaxf(vmax, sum);
    if (f0 + fr < T) melpow[((size_t)b * T + f0 + fr) * NMEL + mm] = sum;
  }
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  if (lane == 0) red[wave] = vmax;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(maxbits + b, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// one thread per output element: power_to_db(ref=max over all frames, amin=1e-10, top_db=80), 0 dB past n_frames
__global__ __launch_bounds__(256) void logmel_finish_kernel(const float* __restrict__ melpow,
                                                            const unsigned* __restrict__ maxbits,
                                                            const int* __restrict__ lens, int T, int layout,
                                                            float* __restrict__ out, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  int t, mm;
  long long b;
  if (layout == S2I_LOGMEL_BFT) {
    t = (int)(idx % T);
    const long long r = idx / T;
    mm = (int)(r % NMEL);
    b = r / NMEL;
  } else {
    mm = (int)(idx % NMEL);
    const long long r = idx / NMEL;
    t = (int)(r % T);
    b = r / T;
  }
  const int L = lens[b];
  const int nf = L > 0 ? min(1 + L / HOP, T) : 0;
  float v = 0.f;
  if (t < nf) {
    const float p = melpow[((size_t)b * T + t) * NMEL + mm];
    const float ref = __uint_as_float(maxbits[b]);
    v = fmaxf(10.f * log10f(fmaxf(1e-10f, p)) - 10.f * log10f(fmaxf(1e-10f, ref)), -80.f);
  }
  out[idx] = v;
}

// A batch out of kept log-mel rows (speech_loader.py), standing for the padding and truncation to target_length of
// load_one_audio_file (Audio_to_Image/utils.py:329-340) applied to rows computed earlier: one thread per 16-byte piece of `out`.  Utterance b owns the
// T * 10 consecutive pieces [b * T * 10, +T * 10) of `out`; its first frames[b] * 10 of them are the consecutive pieces
// of the pool from row off[b] on, the rest are the 0 dB fill of logmel_finish_kernel.  Lane i of a wave stores piece
// base + i: 1 KiB per store instruction, and the loads are as contiguous inside an utterance.  Every address is a 64-bit
// piece index: a pool may hold more than 2^31 floats.
constexpr int ROW_PIECES = NMEL * 4 / 16;        // a 160-byte row is ten f32x4
static_assert(ROW_PIECES * 16 == NMEL * 4, "a log-mel row must be whole 16-byte pieces");

__global__ __launch_bounds__(256) void logmel_gather_kernel(const f32x4* __restrict__ pool,
                                                            const long long* __restrict__ off,
                                                            const int* __restrict__ frames, int T,
                                                            f32x4* __restrict__ out, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long per = (long long)T * ROW_PIECES;
  const long long b = idx / per;
  const long long p = idx - b * per;
  const long long o = off[b];
  const long long kept = o >= 0 ? (long long)min(max(frames[b], 0), T) * ROW_PIECES : 0;   // unstored: all fill
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (p < kept) v = pool[o * ROW_PIECES + p];
  out[idx] = v;
}

}  // namespace

extern "C" size_t s2i_logmel_basis_elems(void) { return (size_t)NKG * 2 * NPT * 64 * 4; }

extern "C" int s2i_signal_mean(const float* x, const long long* offsets, const int* lens, int B, float* mean,
                               unsigned* maxbits, void* stream) {
  S2I_REQUIRE(x && offsets && lens && mean && maxbits, "signal_mean: null pointer");
  S2I_REQUIRE(B >= 1 && B <= 65535 * 1024, "signal_mean: bad utterance count %d", B);
  hipLaunchKernelGGL(signal_mean_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, offsets, lens, mean, maxbits);
  S2I_LAUNCH_CHECK("signal_mean");
  return 0;
}

extern "C" int s2i_logmel_power(const float* x, const long long* offsets, const int* lens, int B, const float* mean,
                                const float* basis, const float* melbank, const int* mel_range, const int* tiles,
                                int ntiles, int T, float* melpow, unsigned* maxbits, void* stream) {
  S2I_REQUIRE(x && offsets && lens && mean && basis && melbank && mel_range && tiles && melpow && maxbits,
              "logmel_power: null pointer");
  S2I_REQUIRE(B >= 1, "logmel_power: bad utterance count %d", B);
  S2I_REQUIRE(ntiles >= 1 && ntiles <= 0x7fffffff / 2, "logmel_power: bad tile count %d", ntiles);
  S2I_REQUIRE(T >= 1, "logmel_power: bad target length %d", T);
  S2I_REQUIRE(((uintptr_t)basis & 15) == 0, "logmel_power: basis must be 16-byte aligned");
  hipLaunchKernelGGL(logmel_power_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)stream, x, offsets, lens, B, mean,
                     (const f32x4*)basis, melbank, mel_range, tiles, T, melpow, maxbits);
  S2I_LAUNCH_CHECK("logmel_power");
  return 0;
}

extern "C" int s2i_logmel_finish(const float* melpow, const unsigned* maxbits, const int* lens, int B, int T,
                                 int layout, float* out, void* stream) {
  S2I_REQUIRE(melpow && maxbits && lens && out, "logmel_finish: null pointer");
  S2I_REQUIRE(B >= 1 && T >= 1, "logmel_finish: bad shape (B %d, T %d)", B, T);
  S2I_REQUIRE(layout == S2I_LOGMEL_BFT || layout == S2I_LOGMEL_NHWC, "logmel_finish: unknown layout %d", layout);
  const long long total = (long long)B * NMEL * T;
  hipLaunchKernelGGL(logmel_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     melpow, maxbits, lens, T, layout, out, total);
  S2I_LAUNCH_CHECK("logmel_finish");
  return 0;
}

extern "C" int s2i_logmel_gather(const float* pool, const long long* row_offsets, const int* frames, int B, int T,
                                 float* out, void* stream) {
  S2I_REQUIRE(pool && row_offsets && frames && out, "logmel_gather: null pointer");
  S2I_REQUIRE(B >= 1 && T >= 1, "logmel_gather: bad shape (B %d, T %d)", B, T);
  S2I_REQUIRE((((uintptr_t)pool | (uintptr_t)out) & 15) == 0, "logmel_gather: pool and out must be 16-byte aligned");
  const long long total = (long long)B * T * ROW_PIECES;
  S2I_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "logmel_gather: B %d x T %d is too large for one launch", B, T);
  hipLaunchKernelGGL(logmel_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const f32x4*)pool, row_offsets, frames, T, (f32x4*)out, total);
  S2I_LAUNCH_CHECK("logmel_gather");
  return 0;
}
