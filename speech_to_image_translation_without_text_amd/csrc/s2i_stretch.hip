// Time stretch of a ragged batch of 16 kHz waveforms on gfx950: the short-time phase vocoder of
// librosa.effects.time_stretch (n_fft 512, hop 128, periodic Hann, zero centre padding) with the phase kept in turns
// (include/s2i_hip.h has the definitions word for word).  x, y: two flat fp32 batches, clip b = x[offsets[b] .. + lens[b])
// and y[out_offsets[b] .. + out_len); table: 16 bytes per clip (StretchEntry).
//
// Five launches, none of which waits on another block:
//   1. stretch_plan_kernel     one block: every clip's frame counts and where its frames start in the workspace (an integer
//                              prefix sum over the clips), 32 bytes per clip at the head of the workspace
//   2. stretch_analysis_kernel (clip, tile of 32 frames): [32 frames x 512 samples] x forward basis [512 x 512] on
//                              v_mfma_f32_16x16x4_f32, then (|X|, arg X / 2 pi) of the 257 bins -> workspace
//   3. stretch_phase_kernel    one thread per (clip, bin): the recursion over the output frames, sequential in t;
//                              Y_t = M_t (cos, sin)(2 pi theta_t) -> workspace, [re 0..256 | im 1..255] per frame
//   4. stretch_synthesis_kernel (clip, tile of 32 output frames): [32 x 512] x inverse basis [512 x 512] on the same
//                              instruction, the window and 1 / 512 folded in -> workspace, 512 samples per frame
//   5. stretch_overlap_kernel  one thread per output sample: the up to four frames that cover it gathered in ascending t,
//                              divided by the same sum of w^2; a clip with rate == 1 is copied here
// Both bases are [512][512] fp32, built in float64 by the host and rounded once; 1 MiB each, they stay in L2.
//
// Order of the sums (part of the ABI): a transform's output is summed in SIXTEEN runs of 32 consecutive k.  A run has an
// fp32 accumulator of its own that starts at 0 and takes its 32 products in ascending k, four per instruction (the
// instruction adds them one after the other, each an fmaf); the output is (((0 + p0) + p1) + ... ) + p15.  One accumulator
// over all 512 products deviated from float64 by 2.1 x what a float32 matrix product on the CPU does at n = 127, and four
// runs of 128 by 4.2 x at n = 1, whose 257 products are all equal, so that every run repeats the first one's rounding
// drift; runs of 32 stay at or under that yardstick in every case.  The signal tile in LDS holds zeros
// outside the clip, so a frame's sum is the same wherever its tile starts; tiles start at the clip's frame 0.  Nothing
// depends on the grid, max_len, the batch or where the clip starts.
#include "s2i_elementwise.h"
#include <stdint.h>

// (1 - a) |X_j| + a |X_j+1| and w w are rounded product by product (csrc/Makefile pins -ffp-contract=off for this unit as
// well, with the correctly rounded division of the overlap-add)
#pragma clang fp contract(off)

namespace {
constexpr int SV_NFFT = 512;
constexpr int SV_HOP = 128;
constexpr int SV_NBIN = 257;
constexpr int SV_MAX_LEN = 0x7fffffff / 4 - 1024;     // 4 max_len + 256 + a tile fits 32 bits
constexpr int SV_FT = 32;                             // frames per tile of either transform
constexpr int SV_SEG = SV_HOP + 2;                    // LDS row of 128 values: rows 2 banks apart, so the 16 rows x 2 k of a
                                                      // 32-lane read land on 32 banks (logmel_power_kernel's image)
constexpr int SV_NQ = SV_NFFT / SV_HOP;               // four chunks of 128 products staged at a time
constexpr int SV_RUN = 32;                            // products per accumulator run (a multiple of 16)
constexpr int SV_ROWS = SV_FT + SV_NQ - 1;            // 35 segments of the signal under 32 overlapping frames
constexpr int SV_POLAR = 2 * 260;                     // floats per analysed frame: |X| [260] then arg / 2 pi [260]
constexpr int SV_BASIS = SV_NFFT * SV_NFFT;           // floats per packed basis
constexpr int SV_OT = 2048;                           // outputs per block of the overlap-add

struct StretchEntry {  // the device table, 16 bytes per clip
  double rate;         // exactly 1: the clip is copied; else in [0.25, 4]
  int out_len;         // floor(n / rate + 0.5)
  int out_frames;      // ceil((1 + n div 128) / rate)
};
static_assert(sizeof(StretchEntry) == 16, "the table's layout is part of the ABI");

struct ClipInfo {      // what stretch_plan_kernel leaves for the other four, 32 bytes per clip
  long long in_base;   // first analysed frame of the clip in the workspace
  long long out_base;  // first output frame
  int F;               // analysed frames; 0: the clip is not stretched (copied, or skipped)
  int OF;              // output frames
  int n;               // samples, clamped to [0, max_len]
  int out_len;         // output samples, clamped to [0, max_out_len]; 0: nothing is written
};
static_assert(sizeof(ClipInfo) == 32, "eight infos per 256 bytes");

__global__ __launch_bounds__(256) void stretch_plan_kernel(const int* __restrict__ lens, int B, int max_len,
                                                           int max_out_len, const StretchEntry* __restrict__ table,
                                                           long long in_cap, long long out_cap,
                                                           ClipInfo* __restrict__ info) {
  __shared__ long long sum_in[256], sum_out[256];
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256;
  const int b0 = tid * per, b1 = b0 + per < B ? b0 + per : B;
  auto frames = [&](int b, int& n, int& F, int& OF, int& out_len) {
    n = lens[b];
    n = n < 0 ? 0 : (n > max_len ? max_len : n);
    const StretchEntry e = table[b];
    out_len = e.out_len < 0 ? 0 : (e.out_len > max_out_len ? max_out_len : e.out_len);
    const bool stretched = n >= 1 && e.rate != 1.0 && e.rate >= 0.25 && e.rate <= 4.0;
    F = stretched ? 1 + n / SV_HOP : 0;
    OF = stretched ? (e.out_frames < 0 ? 0 : (e.out_frames > 4 * F ? 4 * F : e.out_frames)) : 0;
    if (e.rate == 1.0) out_len = out_len < n ? out_len : n;    // a copy
    else if (!stretched) out_len = 0;                          // a rate outside [0.25, 4], NaN included: left alone
  };
  long long si = 0, so = 0;
  for (int b = b0; b < b1; ++b) {
    int n, F, OF, out_len;
    frames(b, n, F, OF, out_len);
    si += F, so += OF;
  }
  sum_in[tid] = si, sum_out[tid] = so;
  __syncthreads();
  long long bi = 0, bo = 0;
  for (int t = 0; t < tid; ++t) bi += sum_in[t], bo += sum_out[t];
  for (int b = b0; b < b1; ++b) {
    int n, F, OF, out_len;
    frames(b, n, F, OF, out_len);
    ClipInfo c{bi, bo, F, OF, n, out_len};
    // no room in the workspace: the clip is left alone.  A clip's place counts every stretched clip before it, fitted or
    // not, so the stretched clips behind one that did not fit are left alone too; a copied clip needs no room.
    if (F > 0 && (bi + F > in_cap || bo + OF > out_cap)) c.F = 0, c.OF = 0, c.out_len = 0;
    info[b] = c;
    bi += F, bo += OF;
  }
}

typedef f32x4 Acc[4][2][2];   // [t][h][mt]: column tile 2 t + h of the wave's eight, rows 16 mt .. 16 mt + 15

__device__ __forceinline__ void clear(Acc& acc) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) acc[t][h][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// sum += rows[32 x 128] x basis chunk [128 x 512], 32 products at a time: each run of 32 consecutive k has an accumulator of
// its own that starts at 0 (eight instructions), and the runs' accumulators are added to `sum` in ascending k.  Wave w
// takes the 32 rows against the eight 16-wide column tiles [8 w, +8).  rows: LDS, row stride SV_SEG; bk: the chunk's
// first fragment.
__device__ __forceinline__ void mfma_chunk(const float* rows, const f32x4* __restrict__ bk, Acc& sum, int lane, int wave) {
  const int i = lane & 15, g = lane >> 4;
  const int nt0 = 8 * wave;
#pragma unroll 1
  for (int run = 0; run < SV_HOP / SV_RUN; ++run) {
    Acc part;
    clear(part);
#pragma unroll
    for (int kk = 0; kk < SV_RUN / 16; ++kk) {
      const int kg = run * (SV_RUN / 16) + kk;
      float a[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) a[u][mt] = rows[(16 * mt + i) * SV_SEG + 16 * kg + 4 * u + g];
      const f32x4* bp = bk + ((size_t)kg * 32 + nt0) * 64 + lane;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x4 bv = bp[(2 * t + h) * 64];
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
              part[t][h][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][mt], bv[u], part[t][h][mt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) sum[t][h][mt] = sum[t][h][mt] + part[t][h][mt];
  }
}

__device__ __forceinline__ void store_polar(float* row, int k, float re, float im) {
  row[k] = hypotf(re, im);
  row[260 + k] = atan2f(im, re) * 0x1.45f306p-3f;   // 1 / (2 pi) rounded to fp32; atan2f(+-0, +x) = +-0: arg(0) = 0
}

// Column tile 2 t + h of the forward basis: h = 0 holds w cos of bins 16 t .. 16 t + 15, h = 1 their -w sin; bin 0 has no
// sine, its h = 1 column is bin 256's cosine.  So (re, im) of a (frame, bin) sit in one lane.
__global__ __launch_bounds__(256) void stretch_analysis_kernel(const float* __restrict__ x,
                                                               const long long* __restrict__ offsets, int B,
                                                               const ClipInfo* __restrict__ info,
                                                               const f32x4* __restrict__ basis, float* __restrict__ polar) {
  __shared__ float lds[SV_ROWS * SV_SEG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const ClipInfo c = info[b];
    const int f0 = (int)blockIdx.x * SV_FT;
    if (f0 >= c.F) continue;                  // the whole block leaves together
    const float* xb = x + offsets[b];
    __syncthreads();                          // the last clip's reads are done
    const int s0 = f0 * SV_HOP - SV_NFFT / 2; // the tile's first sample, negative in the padding
    for (int p = tid; p < SV_ROWS * SV_HOP; p += 256) {
      const int s = s0 + p;
      lds[p + 2 * (p >> 7)] = (s >= 0 && s < c.n) ? xb[s] : 0.f;
    }
    __syncthreads();
    Acc acc;
    clear(acc);
    // samples 128 q .. 128 q + 127 of frame r are segment r + q of the image
#pragma unroll 1
    for (int q = 0; q < SV_NQ; ++q) mfma_chunk(lds + q * SV_SEG, basis + (size_t)q * 8 * 32 * 64, acc, lane, wave);
    // C: register r of lane l is row 4 (l >> 4) + r of column l & 15
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 16 * (4 * wave + t) + i;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = f0 + 16 * mt + 4 * g + r;
          if (f >= c.F) continue;
          float* row = polar + (c.in_base + f) * SV_POLAR;
          const float re = acc[t][0][mt][r], im = acc[t][1][mt][r];
          if (k == 0) {
            store_polar(row, 0, re, 0.f);
            store_polar(row, 256, im, 0.f);
          } else {
            store_polar(row, k, re, im);
          }
        }
    }
  }
}

// One thread per (clip, bin), 64 bins per block.  Frames F and F + 1 are zeros: magnitude 0, phase 0.
__global__ __launch_bounds__(64) void stretch_phase_kernel(int B, const ClipInfo* __restrict__ info,
                                                           const StretchEntry* __restrict__ table,
                                                           const float* __restrict__ polar, float* __restrict__ Y) {
  const int k = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (k >= SV_NBIN) return;
  const float phi = 0.25f * (float)(k & 3);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const ClipInfo c = info[b];
    if (c.F == 0) continue;
    const double rate = table[b].rate;
    const float* pb = polar + c.in_base * SV_POLAR + k;
    float* yb = Y + c.out_base * SV_NFFT;
    float theta = pb[260];
#pragma unroll 4
    for (int t = 0; t < c.OF; ++t) {
      const double s = (double)t * rate;
      int j = (int)s;                         // floor: s >= 0
      const float a = (float)(s - (double)j);
      j = j < c.F ? j : c.F;
      const float* p0 = pb + (long long)j * SV_POLAR;
      const bool in0 = j < c.F, in1 = j + 1 < c.F;
      const float m0 = in0 ? p0[0] : 0.f, t0 = in0 ? p0[260] : 0.f;
      const float m1 = in1 ? p0[SV_POLAR] : 0.f, t1 = in1 ? p0[SV_POLAR + 260] : 0.f;
      const float m = (1.f - a) * m0 + a * m1;
      float sn, cs;
      sincospif(2.f * theta, &sn, &cs);
      float* yr = yb + (long long)t * SV_NFFT;
      yr[k] = m * cs;                         // re 0 .. 256
      if (k >= 1 && k <= 255) yr[256 + k] = m * sn;
      float d = (t1 - t0) - phi;
      d = d - rintf(d);
      theta = (theta + phi) + d;
      theta = theta - rintf(theta);
    }
  }
}

// y_t = Y_t [re 0..256 | im 1..255] x inverse basis [512 x 512] (w / 512 and c_k folded in), 32 output frames per tile
__global__ __launch_bounds__(256) void stretch_synthesis_kernel(int B, const ClipInfo* __restrict__ info,
                                                                const f32x4* __restrict__ basis, const float* __restrict__ Y,
                                                                float* __restrict__ frames) {
  __shared__ float lds[SV_FT * SV_SEG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const ClipInfo c = info[b];
    const int f0 = (int)blockIdx.x * SV_FT;
    if (f0 >= c.OF) continue;
    const float* yb = Y + (c.out_base + f0) * SV_NFFT;
    const int rows = c.OF - f0 < SV_FT ? c.OF - f0 : SV_FT;
    Acc acc;
    clear(acc);
    for (int q = 0; q < SV_NQ; ++q) {
      __syncthreads();                        // the last chunk's (or clip's) reads are done
      for (int p = tid; p < SV_FT * SV_HOP / 4; p += 256) {
        const int r = p >> 5, kk = 4 * (p & 31);
        const f32x4 v = r < rows ? ld4(yb + (long long)r * SV_NFFT + SV_HOP * q + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
        float* d = lds + r * SV_SEG + kk;
        d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
      }
      __syncthreads();
      mfma_chunk(lds, basis + (size_t)q * 8 * 32 * 64, acc, lane, wave);
    }
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int s = 16 * (8 * wave + 2 * t + h) + i;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = 16 * mt + 4 * g + r;
            if (f < rows) frames[(c.out_base + f0 + f) * SV_NFFT + s] = acc[t][h][mt][r];
          }
      }
  }
}

__global__ __launch_bounds__(256) void stretch_overlap_kernel(const float* __restrict__ x,
                                                              const long long* __restrict__ offsets, int B,
                                                              const ClipInfo* __restrict__ info,
                                                              const StretchEntry* __restrict__ table,
                                                              const float* __restrict__ w, const float* __restrict__ frames,
                                                              float* __restrict__ y, const long long* __restrict__ out_offsets) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const ClipInfo c = info[b];
    const int m0 = (int)blockIdx.x * SV_OT;
    if (m0 >= c.out_len) continue;
    const int m1 = m0 + SV_OT < c.out_len ? m0 + SV_OT : c.out_len;
    float* yb = y + out_offsets[b];
    if (c.F == 0) {                           // rate == 1 (stretch_plan_kernel zeroed out_len of every other such clip)
      const float* xb = x + offsets[b];
      for (int m = m0 + (int)threadIdx.x; m < m1; m += 256) yb[m] = xb[m];
      continue;
    }
    const float* fb = frames + c.out_base * SV_NFFT;
    for (int m = m0 + (int)threadIdx.x; m < m1; m += 256) {
      const int u = m + SV_NFFT / 2;
      const int lo = u >= SV_NFFT ? (u - (SV_NFFT - SV_HOP)) >> 7 : 0;   // ceil((u - 511) / 128)
      const int hi = (u >> 7) < c.OF - 1 ? (u >> 7) : c.OF - 1;
      float num = 0.f, den = 0.f;
      for (int t = lo; t <= hi; ++t) {
        const int idx = u - SV_HOP * t;
        const float wv = w[idx];
        num = num + fb[(long long)t * SV_NFFT + idx];
        den = den + wv * wv;
      }
      yb[m] = den > 1e-10f ? num / den : num;
    }
  }
}

__host__ size_t info_bytes(int B) { return ((size_t)B * sizeof(ClipInfo) + 255) / 256 * 256; }
}  // namespace

extern "C" size_t s2i_stretch_basis_elems(void) { return 2 * (size_t)SV_BASIS + SV_NFFT; }

extern "C" size_t s2i_time_stretch_workspace_bytes(int B, long long in_frames_total, long long out_frames_total) {
  if (B < 1 || in_frames_total < 0 || out_frames_total < 0 || in_frames_total > (1ll << 40) || out_frames_total > (1ll << 40)) {
    s2i_set_error("time_stretch_workspace_bytes: bad shape (B %d, %lld input and %lld output frames)", B, in_frames_total,
                  out_frames_total);
    return 0;
  }
  return info_bytes(B) + (size_t)in_frames_total * SV_POLAR * 4 + (size_t)out_frames_total * 2 * SV_NFFT * 4 + 16;
}

extern "C" int s2i_time_stretch(const float* x, const long long* offsets, const int* lens, int B, int max_len,
                                const void* table, const float* basis, float* y, const long long* out_offsets,
                                int max_out_len, long long in_frames_total, long long out_frames_total, void* ws,
                                size_t ws_bytes, void* stream) {
  S2I_REQUIRE(x && offsets && lens && table && basis && y && out_offsets && ws, "time_stretch: null pointer");
  S2I_REQUIRE(B >= 1, "time_stretch: bad clip count %d", B);
  S2I_REQUIRE(max_len >= 1 && max_len <= SV_MAX_LEN, "time_stretch: max_len %d outside [1, %d]", max_len, SV_MAX_LEN);
  S2I_REQUIRE(max_out_len >= 0 && max_out_len <= 4 * (long long)max_len,
              "time_stretch: max_out_len %d outside [0, 4 max_len]", max_out_len);
  S2I_REQUIRE(x != y, "time_stretch: y must be apart from x");
  S2I_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)basis & 15) == 0 && ((uintptr_t)ws & 15) == 0,
              "time_stretch: x, y, the basis and the workspace must be 16-byte aligned");
  S2I_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)out_offsets & 7) == 0 && ((uintptr_t)lens & 3) == 0 &&
                  ((uintptr_t)table & 15) == 0,
              "time_stretch: the offsets must be 8-byte, lens 4-byte and the table 16-byte aligned");
  const size_t need = s2i_time_stretch_workspace_bytes(B, in_frames_total, out_frames_total);
  S2I_REQUIRE(need != 0, "time_stretch: bad frame totals (%lld, %lld)", in_frames_total, out_frames_total);
  S2I_REQUIRE(ws_bytes >= need, "time_stretch: workspace of %zu bytes, need %zu", ws_bytes, need);
  ClipInfo* info = (ClipInfo*)ws;
  float* polar = (float*)((char*)ws + info_bytes(B));
  float* Y = polar + (size_t)in_frames_total * SV_POLAR;
  float* frames = Y + (size_t)out_frames_total * SV_NFFT;
  const StretchEntry* tab = (const StretchEntry*)table;
  const f32x4* fwd = (const f32x4*)basis;
  const f32x4* inv = (const f32x4*)(basis + SV_BASIS);
  const float* w = basis + 2 * (size_t)SV_BASIS;
  const unsigned gy = (unsigned)(B < 65535 ? B : 65535);
  const int fmax = 1 + max_len / SV_HOP;
  hipLaunchKernelGGL(stretch_plan_kernel, dim3(1), dim3(256), 0, ST, lens, B, max_len, max_out_len, tab, in_frames_total,
                     out_frames_total, info);
  S2I_LAUNCH_CHECK("time_stretch (plan)");
  if (in_frames_total > 0) {
    hipLaunchKernelGGL(stretch_analysis_kernel, dim3((unsigned)((fmax + SV_FT - 1) / SV_FT), gy), dim3(256), 0, ST, x, offsets,
                       B, info, fwd, polar);
    S2I_LAUNCH_CHECK("time_stretch (analysis)");
  }
  if (in_frames_total > 0 && out_frames_total > 0) {
    hipLaunchKernelGGL(stretch_phase_kernel, dim3((SV_NBIN + 63) / 64, gy), dim3(64), 0, ST, B, info, tab, polar, Y);
    S2I_LAUNCH_CHECK("time_stretch (phase)");
    // a clip has at most 4 F output frames, and no more than the workspace holds
    long long ofmax = 4ll * fmax < out_frames_total ? 4ll * fmax : out_frames_total;
    hipLaunchKernelGGL(stretch_synthesis_kernel, dim3((unsigned)((ofmax + SV_FT - 1) / SV_FT), gy), dim3(256), 0, ST, B, info,
                       inv, Y, frames);
    S2I_LAUNCH_CHECK("time_stretch (synthesis)");
  }
  if (max_out_len > 0) {
    hipLaunchKernelGGL(stretch_overlap_kernel, dim3((unsigned)((max_out_len + SV_OT - 1) / SV_OT), gy), dim3(256), 0, ST, x,
                       offsets, B, info, tab, w, frames, y, out_offsets);
    S2I_LAUNCH_CHECK("time_stretch (overlap-add)");
  }
  return 0;
}
