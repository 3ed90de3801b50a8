// Three folds of one [Q, N] block of chunked scores (ops.score_rows) behind the kernel inception distance and the
// k-nearest-neighbour manifold metrics (gan_metrics.kid, gan_metrics.prdc).  Like s2i_topk_rows and
// s2i_rank_rows they let two sets of feature rows be compared pair by pair without the [rows, rows] matrix ever existing.
//
//   s2i_polykernel_rows   sum[q] += sum_j (scores[q][j] * inv_d + 1)^3 in fp64, the own column left out on request
//   s2i_sqdist_rows       scores[q][j] <- -max(0, |q|^2 + |row_j|^2 - 2 scores[q][j]) in place, fp32; the own column -inf
//   s2i_ball_rows         count[q] += #{j : nd[q][j] >= row_bound[base + j]},  best[q] = max(best[q], max_j nd[q][j])
//
// One block per query row walks that row once, as s2i_rank.hip does: a lane loads four scores with one 16-byte load, four
// of them in flight; the row's first columns up to a 16-byte boundary and its last N mod 4 go through single loads (and
// single stores, where the fold rewrites the row).  The boundary is found from the row's own address, so any row stride,
// any base and any pointer are taken; the per-row vector that goes with the columns (row_norm2, row_bound) goes with a
// 16-byte load when its address reaches a boundary at the same column, and with four single loads otherwise.
//
// Each pass reads Q * N * 4 bytes of scores once (HBM; s2i_sqdist_rows writes them back once) and N floats per query that
// are the same for every query (L2).  No atomics, no workspace, no allocation, no synchronisation.
#include "s2i_common.h"
#include <limits.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kMaxWaves = 4;
constexpr int kMaxN = 1 << 30;           // as s2i_topk_rows: a column index stays inside int, and so does a counter
constexpr int kUnroll = 4;               // 16-byte loads a lane has in flight
constexpr int kWaveCols = 64 * 4 * kUnroll;

// The column of query q that is its own row of the other set, or -1: none, or not in this block.
__device__ __forceinline__ int own_column(long long own_base, long long q, int base, int N) {
  if (own_base < 0) return -1;
  const long long c = own_base + q - (long long)base;
  return (c >= 0 && c < (long long)N) ? (int)c : -1;
}

// Walks one row: body(col, score, aux[col]) for every column exactly once, each lane its own columns in a fixed order
// (head, tail, then the 16-byte groups by ascending address).  kAux: aux is read (else body gets 0).  kStore: the value
// body returns replaces the score.
template <bool kAux, bool kStore, class Body>
__device__ __forceinline__ void walk_row(float* __restrict__ row, const float* __restrict__ aux, int N, int tid,
                                         int nthreads, Body&& body) {
  // columns [0, head): up to the row's first 16-byte boundary; [head, head + 4 nvec): 16-byte loads; the rest: the tail
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > N) head = N;
  const int nvec = (N - head) >> 2;
  const int tail = head + 4 * nvec;
  const bool aux_vec = kAux && ((uintptr_t)(aux + head) & 15u) == 0;   // block-uniform

  if (tid < head) {
    const float r = body(tid, row[tid], kAux ? aux[tid] : 0.f);
    if (kStore) row[tid] = r;
  }
  if (tail + tid < N) {                                                // < 4 columns
    const float r = body(tail + tid, row[tail + tid], kAux ? aux[tail + tid] : 0.f);
    if (kStore) row[tail + tid] = r;
  }

  float4* __restrict__ row4 = reinterpret_cast<float4*>(row + head);
  const float4* __restrict__ aux4 = reinterpret_cast<const float4*>(aux + head);
  const float* __restrict__ aux1 = aux + head;
  for (int v0 = tid; v0 < nvec; v0 += nthreads * kUnroll) {
    float4 s[kUnroll], a[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = v0 + u * nthreads;
      s[u] = v < nvec ? row4[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = v0 + u * nthreads;
      if (!kAux || v >= nvec) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      else if (aux_vec) a[u] = aux4[v];
      else a[u] = make_float4(aux1[4 * v], aux1[4 * v + 1], aux1[4 * v + 2], aux1[4 * v + 3]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = v0 + u * nthreads;
      if (v < nvec) {                                                  // a group past the row takes no part at all
        const int c = head + 4 * v;
        float4 r;
        r.x = body(c, s[u].x, a[u].x);
        r.y = body(c + 1, s[u].y, a[u].y);
        r.z = body(c + 2, s[u].z, a[u].z);
        r.w = body(c + 3, s[u].w, a[u].w);
        if (kStore) row4[v] = r;
      }
    }
  }
}

// ---- sum of the cubic polynomial kernel --------------------------------------------------------------------------------
__global__ __launch_bounds__(kMaxWaves * 64) void polykernel_rows_kernel(const float* __restrict__ scores, int N,
                                                                         size_t lds, int base, long long own_base,
                                                                         double inv_d, double* __restrict__ sum) {
#pragma clang fp contract(off)   // every fp64 operation rounded on its own: k is the value a host restatement gets
  __shared__ double sAcc[kMaxWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const size_t q = blockIdx.x;
  const int own = own_column(own_base, (long long)q, base, N);
  double acc = 0.0;
  walk_row<false, false>(const_cast<float*>(scores) + q * lds, nullptr, N, tid, nthreads, [&](int c, float s, float) {
#pragma clang fp contract(off)
    const double p = (double)s * inv_d;
    const double t = p + 1.0;
    const double k = (t * t) * t;
    if (c != own) acc += k;
    return 0.f;
  });
  // lanes: butterfly, the same pairs in the same order every run; then the waves in order through LDS
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) sAcc[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < waves; ++w) acc += sAcc[w];
    sum[q] += acc;
  }
}

// ---- scores -> negated squared distances, in place ----------------------------------------------------------------------
__global__ __launch_bounds__(kMaxWaves * 64) void sqdist_rows_kernel(float* __restrict__ scores, int N, size_t lds, int base,
                                                                     long long own_base, const float* __restrict__ q_norm2,
                                                                     const float* __restrict__ chunk_norm2) {
  const size_t q = blockIdx.x;
  const int own = own_column(own_base, (long long)q, base, N);
  const float qn = q_norm2[q];
  walk_row<true, true>(scores + q * lds, chunk_norm2, N, threadIdx.x, blockDim.x, [&](int c, float s, float rn) {
    const float d = (qn + rn) - 2.f * s;                 // 2 s is exact: an FMA here gives the same bits
    const float nd = d != d ? d : -fmaxf(0.f, d);        // fmaxf alone would drop a NaN
    return c == own ? -INFINITY : nd;
  });
}

// ---- how many balls hold the query, and its nearest row ----------------------------------------------------------------
__global__ __launch_bounds__(kMaxWaves * 64) void ball_rows_kernel(const float* __restrict__ nd, int N, size_t lds,
                                                                   const float* __restrict__ chunk_bound,
                                                                   int* __restrict__ count, float* __restrict__ best) {
  __shared__ int sCnt[kMaxWaves];
  __shared__ float sBest[kMaxWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const size_t q = blockIdx.x;
  int cnt = 0;
  float top = -INFINITY;
  // comparisons only: a NaN entry or a NaN bound is false in both
  walk_row<true, false>(const_cast<float*>(nd) + q * lds, chunk_bound, N, tid, nthreads, [&](int, float s, float b) {
    cnt += s >= b ? 1 : 0;
    top = s > top ? s : top;
    return 0.f;
  });
  // wave, then LDS: an integer sum and a maximum, the same in any order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cnt += __shfl_down(cnt, d);
    const float o = __shfl_down(top, d);
    top = o > top ? o : top;
  }
  if (lane == 0) {
    sCnt[wave] = cnt;
    sBest[wave] = top;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < waves; ++w) {
      cnt += sCnt[w];
      top = sBest[w] > top ? sBest[w] : top;
    }
    if (count) count[q] += cnt;
    if (best) best[q] = top > best[q] ? top : best[q];
  }
}

// a wave per 1024 columns of a row, 4 at the most: the queries fill the chip, not the waves of one block
int row_waves(int N) {
  const int waves = s2i_cdiv(N, kWaveCols);
  return waves > kMaxWaves ? kMaxWaves : waves;
}

}  // namespace

#define S2I_BLOCK_ARGS(name)                                                                                            \
  S2I_REQUIRE(Q >= 1 && N >= 1 && N <= kMaxN, name ": Q %d must be positive and N %d lie in 1..%d", Q, N, kMaxN);       \
  S2I_REQUIRE(lds >= N, name ": row stride %d < N %d", lds, N);                                                         \
  S2I_REQUIRE(base >= 0 && (long long)base + N <= (long long)INT_MAX, name ": row ids %d + %d leave int", base, N)

extern "C" int s2i_polykernel_rows(const float* scores, int Q, int N, int lds, int base, int own_base, double inv_d,
                                   double* sum, void* stream) {
  S2I_REQUIRE(scores && sum, "polykernel_rows: null pointer");
  S2I_BLOCK_ARGS("polykernel_rows");
  S2I_REQUIRE(own_base >= -1, "polykernel_rows: own_base %d is neither -1 nor a row id",
              own_base);
  S2I_REQUIRE(inv_d == inv_d && fabs(inv_d) <= 1.79769313486231570e308, "polykernel_rows: inv_d is not finite");
  S2I_REQUIRE(((uintptr_t)scores & 3) == 0 && ((uintptr_t)sum & 7) == 0,
              "polykernel_rows: scores are not 4-byte or sums not 8-byte aligned");
  hipLaunchKernelGGL(polykernel_rows_kernel, dim3(Q), dim3(row_waves(N) * 64), 0, (hipStream_t)stream, scores, N,
                     (size_t)lds, base, own_base, inv_d, sum);
  S2I_LAUNCH_CHECK("polykernel_rows");
  return 0;
}

extern "C" int s2i_sqdist_rows(float* scores, int Q, int N, int lds, int base, int own_base, const float* q_norm2,
                               const float* row_norm2, int n_rows, void* stream) {
  S2I_REQUIRE(scores && q_norm2 && row_norm2, "sqdist_rows: null pointer");
  S2I_BLOCK_ARGS("sqdist_rows");
  S2I_REQUIRE(own_base >= -1, "sqdist_rows: own_base %d is neither -1 nor a row id",
              own_base);
  S2I_REQUIRE((long long)base + N <= (long long)n_rows, "sqdist_rows: rows %d + %d pass the %d row norms", base, N, n_rows);
  S2I_REQUIRE((((uintptr_t)scores | (uintptr_t)q_norm2 | (uintptr_t)row_norm2) & 3) == 0,
              "sqdist_rows: scores or norms are not 4-byte aligned");
  hipLaunchKernelGGL(sqdist_rows_kernel, dim3(Q), dim3(row_waves(N) * 64), 0, (hipStream_t)stream, scores, N, (size_t)lds,
                     base, own_base, q_norm2, row_norm2 + base);
  S2I_LAUNCH_CHECK("sqdist_rows");
  return 0;
}

extern "C" int s2i_ball_rows(const float* nd, int Q, int N, int lds, int base, const float* row_bound, int n_rows,
                             int* count, float* best, void* stream) {
  S2I_REQUIRE(nd && row_bound, "ball_rows: null pointer");
  S2I_REQUIRE(count || best, "ball_rows: null pointer (both count and best: nothing to write)");
  S2I_BLOCK_ARGS("ball_rows");
  S2I_REQUIRE((long long)base + N <= (long long)n_rows, "ball_rows: rows %d + %d pass the %d row bounds", base, N, n_rows);
  S2I_REQUIRE((((uintptr_t)nd | (uintptr_t)row_bound | (uintptr_t)count | (uintptr_t)best) & 3) == 0,
              "ball_rows: distances, bounds or outputs are not 4-byte aligned");
  hipLaunchKernelGGL(ball_rows_kernel, dim3(Q), dim3(row_waves(N) * 64), 0, (hipStream_t)stream, nd, N, (size_t)lds,
                     row_bound + base, count, best);
  S2I_LAUNCH_CHECK("ball_rows");
  return 0;
}
