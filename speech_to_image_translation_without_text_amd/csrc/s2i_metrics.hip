// Streaming moments of feature rows for the Frechet distance (StackGAN_v2/trainer.py:103-144 fits a Gaussian to the pool3
// rows with np.mean / np.cov): the count is the caller's, the column sums and the Gram matrix X^T X are accumulated here
// in fp64, chunk by chunk, so no row has to be kept.  fp32 -> fp64 is exact and an fp32 x fp32 product fits in the fp64
// mantissa (48 <= 53 bits), so v_mfma_f64_16x16x4_f64 forms every product exactly; the only rounding is in the fp64 sums.
#include "s2i_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;        // Gram tile edge: one block per tile on or above the diagonal
constexpr int kRows = 32;        // rows staged in LDS per step
constexpr int kLd = kTile + 2;   // LDS row stride in doubles: the four k rows one MFMA operand read touches fall on
                                 // different banks
constexpr int kThreads = 256;    // four waves, each owning a 32 x 32 quarter of the tile (2 x 2 MFMA tiles of 16 x 16)
constexpr int kMaxD = 65536;
constexpr int kMaxRows = 1 << 30;

// Block b of the T (T + 1) / 2 upper tiles (row-major over the upper triangle) accumulates
//   gram[i0 .. i0 + 63][j0 .. j0 + 63] += X[:, i0 ..]^T X[:, j0 ..]   over rows 0 .. rows - 1 in order,
// starting its accumulators FROM the stored tile, so a chunk continues the running sums of the earlier chunks.  Each
// accumulator sums its k in a fixed order: the result does not depend on scheduling.  A diagonal block also owns the 64
// column sums of its strip.  Columns >= D and rows >= rows are staged as zeros (an exact no-op in the sums).
__global__ __launch_bounds__(kThreads) void moments_kernel(const float* __restrict__ x, int rows, int D, long long ldx,
                                                           int T, double* __restrict__ colsum,
                                                           double* __restrict__ gram) {
  __shared__ double sa[kRows][kLd];
  __shared__ double sb[kRows][kLd];
  int b = blockIdx.x, ti = 0;
  while (b >= T - ti) {
    b -= T - ti;
    ++ti;
  }
  const int tj = ti + b;
  const bool diag = ti == tj;
  const int i0 = ti * kTile, j0 = tj * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;

  // MFMA f64 16x16x4 C/D layout: register r of lane l is (row (l >> 4) + 4 r, col l & 15) of the 16 x 16 tile
  f64x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + wi + 16 * m + lk + 4 * r, col = j0 + wj + 16 * n + lr;
        acc[m][n][r] = (row < D && col < D) ? gram[(size_t)row * D + col] : 0.0;
      }
  const bool owns_sum = diag && tid < kTile && i0 + tid < D;
  double cs = owns_sum ? colsum[i0 + tid] : 0.0;

  // staging: thread (wave, lane) loads column lane of the strips at rows wave + 4 q, q = 0..7
  const int ca = i0 + lane, cb = j0 + lane;
  const bool va = ca < D, vb = !diag && cb < D;
  float fa[kRows / 4], fb[kRows / 4];
  auto load = [&](int r0) {
#pragma unroll
    for (int q = 0; q < kRows / 4; ++q) {
      const int r = r0 + wave + 4 * q;
      const float* p = x + (size_t)r * (size_t)ldx;
      fa[q] = (r < rows && va) ? p[ca] : 0.f;
      fb[q] = (r < rows && vb) ? p[cb] : 0.f;
    }
  };
  load(0);
  for (int r0 = 0; r0 < rows; r0 += kRows) {
    __syncthreads();   // the previous step's LDS reads are done
#pragma unroll
    for (int q = 0; q < kRows / 4; ++q) {
      sa[wave + 4 * q][lane] = (double)fa[q];
      sb[wave + 4 * q][lane] = (double)fb[q];
    }
    __syncthreads();
    if (r0 + kRows < rows) load(r0 + kRows);   // next step's rows are in flight during this step's MFMAs
    const double(*sbj)[kLd] = diag ? sa : sb;
    if (owns_sum) {
#pragma unroll 8
      for (int k = 0; k < kRows; ++k) cs += sa[k][tid];
    }
#pragma unroll
    for (int k = 0; k < kRows; k += 4) {
      const double a0 = sa[k + lk][wi + lr], a1 = sa[k + lk][wi + 16 + lr];
      const double b0 = sbj[k + lk][wj + lr], b1 = sbj[k + lk][wj + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + wi + 16 * m + lk + 4 * r, col = j0 + wj + 16 * n + lr;
        if (row < D && col < D) gram[(size_t)row * D + col] = acc[m][n][r];
      }
  if (owns_sum) colsum[i0 + tid] = cs;
}

}  // namespace

extern "C" int s2i_moments_accumulate(const float* x, int rows, int D, long long ldx, double* colsum, double* gram,
                                      void* stream) {
  S2I_REQUIRE(colsum && gram, "moments_accumulate: null pointer");
  S2I_REQUIRE(D >= 1 && D <= kMaxD, "moments_accumulate: D %d outside 1..%d", D, kMaxD);
  S2I_REQUIRE(rows >= 0 && rows <= kMaxRows, "moments_accumulate: rows %d outside 0..%d", rows, kMaxRows);
  S2I_REQUIRE(ldx >= D, "moments_accumulate: row stride %lld < D %d", ldx, D);
  if (rows == 0) return 0;
  S2I_REQUIRE(x, "moments_accumulate: null rows");
  const int T = s2i_cdiv(D, kTile);
  hipLaunchKernelGGL(moments_kernel, dim3(T * (T + 1) / 2), dim3(kThreads), 0, (hipStream_t)stream, x, rows, D, ldx, T,
                     colsum, gram);
  S2I_LAUNCH_CHECK("moments_accumulate");
  return 0;
}
