// The k best entries of every row of a score matrix, folded into a running [Q][k] result: the last stage of a chunked
// nearest-row search (retrieval.Gallery), which never holds the [Q, N] scores of the whole gallery.
//
// Order.  An entry is (score bits, row id).  Its rank key is the 64-bit word  ord(score) << 32 | ~row  compared as unsigned,
// larger first: ord() maps a float to a 32-bit word that ascends with the value (NaN taken as -inf, -0 as +0), and ~row
// makes the LOWER row id win among equal scores.  An empty slot is (-inf, -1): ~(-1) = 0, so it ranks behind every real
// row, real rows scored -inf or NaN included.  The key only ranks; the score bits travel next to it untouched.
//
// One block per query row, 1 to 16 waves.  Each wave keeps its k best in its own lanes, lane r = rank r, best first.  It
// walks the row 256 elements at a time (four coalesced loads in flight per lane); a ballot finds the lanes whose element
// beats the wave's k-th key, and each of those is inserted with one shift (__shfl_up) -- after the first few hundred
// elements of a row in random order almost every group passes with no insertion at all.  The waves' lists and, when
// merging, the k stored entries then meet in LDS, where every entry counts the entries ahead of it (ties on the key by
// position); that count is its output slot.  The keys of distinct rows differ, so the result does not depend on how the
// row was divided among waves or chunks: no atomics, no scratch, no workspace, nothing for the host to wait on.
#include "s2i_common.h"
#include <limits.h>

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kMaxK = 64;
constexpr int kMaxWaves = 16;
constexpr int kMaxN = 1 << 30;                     // the element index of a step stays inside int
constexpr int kGroup = 256;                        // elements one wave takes per step: 4 per lane
constexpr u32 kNegInf = 0xff800000u;
constexpr u64 kEmpty = (u64)0x007fffffu << 32;     // key of (-inf, row -1)

__device__ __forceinline__ u32 ord_bits(u32 b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) b = kNegInf;   // NaN ranks as -inf
  if (b == 0x80000000u) b = 0u;                       // -0 == +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u64 make_key(u32 bits, int row) { return ((u64)ord_bits(bits) << 32) | (u32)~(u32)row; }

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const u32 lo = __shfl((u32)v, src), hi = __shfl((u32)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_up64(u64 v) {
  const u32 lo = __shfl_up((u32)v, 1), hi = __shfl_up((u32)(v >> 32), 1);
  return ((u64)hi << 32) | lo;
}

// Insert every lane's candidate (ck, cb) that beats thr into the wave's sorted list (K, B); thr follows the k-th entry.
__device__ __forceinline__ void wave_insert(u64 ck, u32 cb, int lane, int k, u64& K, u32& B, u64& thr) {
  u64 mask = __ballot(ck > thr);
  while (mask) {                                      // wave-uniform
    const int src = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const u64 c = shfl64(ck, src);
    const u32 b = __shfl(cb, src);
    if (c > thr) {                                    // thr may have risen since the ballot
      const u64 upK = shfl_up64(K);
      const u32 upB = __shfl_up(B, 1);
      if (!(K > c)) {                                 // this lane's entry moves down, or the candidate lands here
        const bool here = lane == 0 || upK > c;
        K = here ? c : upK;
        B = here ? b : upB;
      }
      thr = shfl64(K, k - 1);
    }
  }
}

__global__ __launch_bounds__(kMaxWaves * 64) void topk_rows_kernel(const float* __restrict__ scores, int N, size_t lds,
                                                                   int base, int k, float* __restrict__ best_score,
                                                                   int* __restrict__ best_row, int merge) {
  __shared__ u64 sK[(kMaxWaves + 1) * kMaxK];
  __shared__ u32 sB[(kMaxWaves + 1) * kMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const size_t q = blockIdx.x;
  const u32* __restrict__ row = reinterpret_cast<const u32*>(scores) + q * lds;

  u64 K = kEmpty, thr = kEmpty;
  u32 B = kNegInf;
  for (int j0 = wave * kGroup; j0 < N; j0 += waves * kGroup) {
    u32 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 64 + lane;
      v[u] = j < N ? row[j] : kNegInf;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 64 + lane;
      const u64 ck = j < N ? make_key(v[u], base + j) : 0ull;   // 0 beats nothing
      wave_insert(ck, v[u], lane, k, K, B, thr);
    }
  }

  // the waves' lists, then the stored entries: E = waves * k (+ k) >= k entries
  if (lane < k) {
    sK[wave * k + lane] = K;
    sB[wave * k + lane] = B;
  }
  int E = waves * k;
  if (merge) {
    if (tid < k) {
      const u32 b = reinterpret_cast<const u32*>(best_score)[q * k + tid];
      sK[E + tid] = make_key(b, best_row[q * k + tid]);
      sB[E + tid] = b;
    }
    E += k;
  }
  __syncthreads();   // every read of the stored entries is done before any slot is written
  // An entry's slot is the number of entries ahead of it, ties on the key going to the earlier position.  Each wave's
  // list is sorted, so its share of that count is a binary search (6 probes for 64 entries); the stored entries are
  // counted one by one, so nothing is assumed about their order.  An entry already k deep stops counting.
  for (int e = tid; e < E; e += blockDim.x) {
    const u64 mine = sK[e];
    const int own = e / k;                            // 0 .. waves - 1: a wave's list; waves: the stored entries
    int ahead = own < waves ? e - own * k : 0;        // those before it in its own sorted list
    for (int l = 0; l < waves && ahead < k; ++l) {
      if (l == own) continue;
      const u64* list = sK + l * k;
      int lo = 0, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const u64 o = list[mid];
        if (o > mine || (o == mine && l < own)) lo = mid + 1;
        else hi = mid;
      }
      ahead += lo;
    }
    if (merge && ahead < k) {
      for (int j = waves * k; j < E; ++j) {
        const u64 o = sK[j];
        ahead += (o > mine || (o == mine && j < e)) ? 1 : 0;
      }
    }
    if (ahead < k) {
      reinterpret_cast<u32*>(best_score)[q * k + ahead] = sB[e];
      best_row[q * k + ahead] = (int)~(u32)mine;
    }
  }
}

}  // namespace

extern "C" int s2i_topk_rows(const float* scores, int Q, int N, int lds, int base, int k, float* best_score, int* best_row,
                             int merge, void* stream) {
  S2I_REQUIRE(scores && best_score && best_row, "topk_rows: null pointer");
  S2I_REQUIRE(k >= 1 && k <= kMaxK, "topk_rows: k %d outside 1..%d", k, kMaxK);
  S2I_REQUIRE(Q >= 1 && N >= 1 && N <= kMaxN, "topk_rows: Q %d must be positive and N %d lie in 1..%d", Q, N, kMaxN);
  S2I_REQUIRE(lds >= N, "topk_rows: row stride %d < N %d", lds, N);
  S2I_REQUIRE(base >= 0 && (long long)base + N <= (long long)INT_MAX, "topk_rows: row ids %d + %d leave int", base, N);
  // a wave per 1024 elements of a row, 16 at the most: short rows do not pay for a wide merge
  int waves = s2i_cdiv(N, 4 * kGroup);
  if (waves > kMaxWaves) waves = kMaxWaves;
  hipLaunchKernelGGL(topk_rows_kernel, dim3(Q), dim3(waves * 64), 0, (hipStream_t)stream, scores, N, (size_t)lds, base, k,
                     best_score, best_row, merge ? 1 : 0);
  S2I_LAUNCH_CHECK("topk_rows");
  return 0;
}
