// The rank of one designated candidate of every query among the candidates of other classes, folded chunk by chunk into
// per-query counters: the last stage of the speech-image consistency score (retrieval.Gallery.rank, gan_metrics.
// ConsistencyScorer), which never holds the [Q, N] scores of the whole gallery.  A top k does not answer this: the rank
// can be in the thousands.
//
// Two launches share one entry point.  Gather: one thread per query copies scores[q][own_row[q] - base] into own_score[q]
// when the own row lies in this chunk.  Count: one block per query walks its row of scores once and counts the columns
// whose gallery row has another label than the query and whose score is greater than (gt) or equal to (eq) the own
// score.  Scores are only compared, never computed with; the counters are integers, so the result does not depend on
// how the row was divided among lanes, waves or chunks: no atomics, no scratch, no workspace.
//
// The pass reads Q * N * 4 bytes of scores once (HBM) and N labels per query (the same for every query: L2).  A lane
// loads four scores with one 16-byte load, four of them in flight; the row's first columns up to a 16-byte boundary and
// its last N mod 4 go through single loads.  The boundary is found from the row's own address, so any row stride, any
// base and any pointer are taken; the labels go with a 16-byte load when their address reaches a boundary at the same
// column, and with four single loads otherwise.
#include "s2i_common.h"
#include <limits.h>
#include <stdint.h>

namespace {

constexpr int kMaxWaves = 4;
constexpr int kMaxN = 1 << 30;           // as s2i_topk_rows: a column index stays inside int, and so does a counter
constexpr int kUnroll = 4;               // 16-byte loads a lane has in flight
constexpr int kWaveCols = 64 * 4 * kUnroll;

// One candidate.  A NaN own score makes every candidate of another class count as greater; a NaN score is neither
// greater nor equal.
__device__ __forceinline__ void tally(float s, int label, float own, int qlabel, bool own_nan, int& gt, int& eq) {
  const bool other = label != qlabel;
  gt += (other && (own_nan || s > own)) ? 1 : 0;
  eq += (other && s == own) ? 1 : 0;
}

__global__ __launch_bounds__(256) void rank_gather_kernel(const float* __restrict__ scores, int Q, int N, size_t lds,
                                                           int base, const int* __restrict__ own_row,
                                                           float* __restrict__ own_score) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)Q) return;
  const int r = own_row[q];
  if (r < base || r - base >= N) return;         // -1 and rows of other chunks: untouched
  // bit copy: a NaN own score travels as it is
  reinterpret_cast<unsigned int*>(own_score)[q] = reinterpret_cast<const unsigned int*>(scores)[q * lds + (r - base)];
}

__global__ __launch_bounds__(kMaxWaves * 64) void rank_count_kernel(const float* __restrict__ scores, int N, size_t lds,
                                                                    const int* __restrict__ chunk_label,
                                                                    const int* __restrict__ query_label,
                                                                    const float* __restrict__ own_score,
                                                                    int* __restrict__ gt_out, int* __restrict__ eq_out) {
  __shared__ int sGt[kMaxWaves], sEq[kMaxWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
  const size_t q = blockIdx.x;
  const float* __restrict__ row = scores + q * lds;
  const float own = own_score[q];
  const int qlabel = query_label[q];
  const bool own_nan = own != own;

  // columns [0, head): up to the row's first 16-byte boundary; [head, head + 4 nvec): 16-byte loads; the rest: the tail
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);
  if (head > N) head = N;
  const int nvec = (N - head) >> 2;
  const int tail = head + 4 * nvec;
  const bool label_vec = ((uintptr_t)(chunk_label + head) & 15u) == 0;   // block-uniform

  int gt = 0, eq = 0;
  if (tid < head) tally(row[tid], chunk_label[tid], own, qlabel, own_nan, gt, eq);
  if (tail + tid < N) tally(row[tail + tid], chunk_label[tail + tid], own, qlabel, own_nan, gt, eq);   // < 4 columns

  const float4* __restrict__ row4 = reinterpret_cast<const float4*>(row + head);
  const int4* __restrict__ lab4 = reinterpret_cast<const int4*>(chunk_label + head);
  const int* __restrict__ lab1 = chunk_label + head;
  for (int v0 = tid; v0 < nvec; v0 += nthreads * kUnroll) {
    float4 s[kUnroll];
    int4 l[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = v0 + u * nthreads;
      s[u] = v < nvec ? row4[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int v = v0 + u * nthreads;
      if (v >= nvec) l[u] = make_int4(qlabel, qlabel, qlabel, qlabel);   // the query's own class: never counted
      else if (label_vec) l[u] = lab4[v];
      else l[u] = make_int4(lab1[4 * v], lab1[4 * v + 1], lab1[4 * v + 2], lab1[4 * v + 3]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      tally(s[u].x, l[u].x, own, qlabel, own_nan, gt, eq);
      tally(s[u].y, l[u].y, own, qlabel, own_nan, gt, eq);
      tally(s[u].z, l[u].z, own, qlabel, own_nan, gt, eq);
      tally(s[u].w, l[u].w, own, qlabel, own_nan, gt, eq);
    }
  }

  // wave, then LDS: integer sums, the same in any order
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    gt += __shfl_down(gt, d);
    eq += __shfl_down(eq, d);
  }
  if (lane == 0) {
    sGt[wave] = gt;
    sEq[wave] = eq;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < waves; ++w) {
      gt += sGt[w];
      eq += sEq[w];
    }
    gt_out[q] += gt;
    eq_out[q] += eq;
  }
}

}  // namespace

extern "C" int s2i_rank_rows(const float* scores, int Q, int N, int lds, int base, const int* own_row,
                             const int* query_label, const int* row_label, int n_labels, float* own_score, int* gt, int* eq,
                             int mode, void* stream) {
  S2I_REQUIRE(mode == S2I_RANK_GATHER || mode == S2I_RANK_COUNT, "rank_rows: mode %d is neither gather nor count", mode);
  S2I_REQUIRE(scores && own_score, "rank_rows: null pointer");
  S2I_REQUIRE(Q >= 1 && N >= 1 && N <= kMaxN, "rank_rows: Q %d must be positive and N %d lie in 1..%d", Q, N, kMaxN);
  S2I_REQUIRE(lds >= N, "rank_rows: row stride %d < N %d", lds, N);
  S2I_REQUIRE(base >= 0 && (long long)base + N <= (long long)INT_MAX, "rank_rows: row ids %d + %d leave int", base, N);
  S2I_REQUIRE((((uintptr_t)scores | (uintptr_t)own_score) & 3) == 0, "rank_rows: scores are not 4-byte aligned");
  if (mode == S2I_RANK_GATHER) {
    S2I_REQUIRE(own_row, "rank_rows: null pointer (own_row)");
    hipLaunchKernelGGL(rank_gather_kernel, dim3(s2i_cdiv(Q, 256)), dim3(256), 0, (hipStream_t)stream, scores, Q, N,
                       (size_t)lds, base, own_row, own_score);
    S2I_LAUNCH_CHECK("rank_rows(gather)");
    return 0;
  }
  S2I_REQUIRE(query_label && row_label && gt && eq, "rank_rows: null pointer (labels or counters)");
  S2I_REQUIRE((long long)base + N <= (long long)n_labels, "rank_rows: rows %d + %d pass the %d row labels", base, N,
              n_labels);
  S2I_REQUIRE(((uintptr_t)row_label & 3) == 0, "rank_rows: row labels are not 4-byte aligned");
  // a wave per 1024 columns of a row, 4 at the most: the queries fill the chip, not the waves of one block
  int waves = s2i_cdiv(N, kWaveCols);
  if (waves > kMaxWaves) waves = kMaxWaves;
  hipLaunchKernelGGL(rank_count_kernel, dim3(Q), dim3(waves * 64), 0, (hipStream_t)stream, scores, N, (size_t)lds,
                     row_label + base, query_label, own_score, gt, eq);
  S2I_LAUNCH_CHECK("rank_rows(count)");
  return 0;
}
