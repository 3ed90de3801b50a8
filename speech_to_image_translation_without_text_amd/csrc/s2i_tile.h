// Tile pieces shared by the matrix kernels of the convolution units (s2i_conv_fwd.h, s2i_wgrad.hip, s2i_conv2d.hip) and
// of the bf16 units (s2i_bf16_conv.hip, s2i_bf16_conv_v2.hip) (internal).  Every kernel there keeps its result as f32x16 acc[TM][TN]: a wave owns TM x TN MFMA tiles of
// 32 x 32, wave (wm, wn) of the block's WAVES_M x WAVES_N.
// The helpers take plain arguments, no kernel parameter struct, and the caller supplies what differs between kernels (how a
// tile row becomes an output row) as a lambda.  All of them are __forceinline__: a kernel's accumulators stay in registers.
#pragma once
#include "s2i_common.h"

// tile row held by accumulator register r of MFMA tile i (v_mfma_*_32x32: four rows per register quad, the upper half-wave
// lh = lane >> 5 four rows further down), and tile column of lane l31 = lane & 31 in MFMA tile j
__device__ __forceinline__ int acc_row(int wm, int TM, int i, int r, int lh) {
  return wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
}
__device__ __forceinline__ int acc_col(int wn, int TN, int j, int l31) { return wn * TN * 32 + j * 32 + l31; }

__device__ __forceinline__ unsigned short f2bf(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// XCD-aware block order.  Blocks are dealt round-robin over the chip's 8 XCDs, each with an L2 of its own
// (MI355X_MICROARCH.md).  A grid is n_major x n_sibling blocks whose siblings read the same operand bytes: the column
// blocks, phases and K splits of one row tile of a convolution (they gather the same input pixels, but sit gridDim.x ids
// apart in launch order: another XCD's L2, another time), or the k-tiles of one pixel-range split of a weight gradient (in
// launch order the 8 k-tiles of a split land on 8 different XCDs and every one of them pulls the split's `g` rows through the
// fabric; profiles/r03_roofline_bf16_wgrad_b48: 1.25 GB fetched for 453 MB of operands).  Linear block id L -> (major,
// sibling) such that all siblings of a major index have the same L % 8 -- one XCD -- and consecutive ids on that XCD; a
// bijection for any grid (the last group of major indices uses its own modulus).
__device__ __forceinline__ void xcd_block_map(int n_major, int n_sibling, int& major, int& sibling) {
  const int L = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const int per_group = 8 * n_sibling;
  const int grp = L / per_group, Ll = L - grp * per_group;
  const int in_group = min(8, n_major - grp * 8);        // major indices of this group (the last one may hold fewer)
  major = grp * 8 + Ll % in_group;
  sibling = Ll / in_group;
}

// Contribution of a spatially constant operand (the broadcast c_code of model.py:277), pre-reduced per border class:
// cls = 3 * (top | middle | bottom) + (left | middle | right).  pixel(tile row, b, oy, ox) -> false for a row beyond the batch.
template <int TM, int TN, class PixelFn>
__device__ __forceinline__ void add_class_bias(const float* __restrict__ cls_bias, int N, int Ho, int Wo, f32x16 (&acc)[TM][TN],
                                               int lane, int wm, int wn, int n0, PixelFn pixel) {
  const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int b, oy, ox;
      if (!pixel(acc_row(wm, TM, i, r, lh), b, oy, ox)) continue;
      const int cls = 3 * (oy == 0 ? 0 : (oy == Ho - 1 ? 2 : 1)) + (ox == 0 ? 0 : (ox == Wo - 1 ? 2 : 1));
      const float* bp = cls_bias + ((size_t)b * 9 + cls) * N;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + acc_col(wn, TN, j, l31);
        if (n < N) acc[i][j][r] += bp[n];
      }
    }
}

// The tile leaves the registers: element (tile row, n) goes to out[row * ldo + n], row from out_row(tile row, row), which
// returns false for a row that does not exist.  raw: the accumulators as they are (a split-K or weight-gradient slab);
// otherwise bias, activation and, with y16, a bf16 store.
template <int TM, int TN, class RowFn>
__device__ __forceinline__ void store_tile(float* __restrict__ out, int ldo, int N, bool raw, const float* __restrict__ bias,
                                           int act, int y16, const f32x16 (&acc)[TM][TN], int lane, int wm, int wn, int n0,
                                           RowFn out_row) {
  const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      long long row;
      if (!out_row(acc_row(wm, TM, i, r, lh), row)) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n0 + acc_col(wn, TN, j, l31);
        if (n < N) {
          float v = acc[i][j][r];
          if (!raw) {
            if (bias) v += bias[n];
            if (act == S2I_ACT_LRELU) v = v > 0.f ? v : 0.2f * v;
            else if (act == S2I_ACT_TANH) v = tanhf(v);
            else if (act == S2I_ACT_RELU) v = fmaxf(v, 0.f);
          }
          if (!raw && y16) reinterpret_cast<unsigned short*>(out)[row * ldo + n] = f2bf(v);
          else out[row * ldo + n] = v;
        }
      }
    }
  }
}

// fp32 slab [rows][N] of a split-K convolution or of a weight gradient
template <int TM, int TN, class RowFn>
__device__ __forceinline__ void store_slab(float* __restrict__ slab, int N, const f32x16 (&acc)[TM][TN], int lane, int wm, int wn,
                                           int n0, RowFn out_row) {
  store_tile<TM, TN>(slab, N, N, true, nullptr, S2I_ACT_NONE, 0, acc, lane, wm, wn, n0, out_row);
}

// BatchNorm column sums and sums of squares of the accumulators over the block's rows (rows that do not exist gathered
// zeros and contribute nothing) -> part[0 | 1][gm][n].  red: LDS, [2][WAVES_M][BN] floats, free once every wave has
// reached the barrier below.  Summation order: over i, r in a lane, the other half-wave, then over WAVES_M.
template <int TM, int TN, int WAVES_M, int BN>
__device__ __forceinline__ void tile_col_stats(float* __restrict__ part, int nparts, int N, float* red,
                                               const f32x16 (&acc)[TM][TN], int tid, int lane, int wm, int wn, int n0, int gm) {
  const int l31 = lane & 31, lh = lane >> 5;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    float sv = 0.f, sq = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[i][j][r];
        sv += v;
        sq += v * v;
      }
    sv += __shfl_xor(sv, 32);
    sq += __shfl_xor(sq, 32);
    if (lh == 0) {
      const int col = acc_col(wn, TN, j, l31);
      red[(0 * WAVES_M + wm) * BN + col] = sv;
      red[(1 * WAVES_M + wm) * BN + col] = sq;
    }
  }
  __syncthreads();
  if (tid < BN) {
    const int n = n0 + tid;
    if (n < N) {
      float sv = 0.f, sq = 0.f;
#pragma unroll
      for (int q = 0; q < WAVES_M; ++q) {
        sv += red[(0 * WAVES_M + q) * BN + tid];
        sq += red[(1 * WAVES_M + q) * BN + tid];
      }
      part[((size_t)0 * nparts + gm) * N + n] = sv;
      part[((size_t)1 * nparts + gm) * N + n] = sq;
    }
  }
}
