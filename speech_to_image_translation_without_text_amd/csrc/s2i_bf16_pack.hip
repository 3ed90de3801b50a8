// bf16 activation path: the weight re-pack kernels and the split-K reduction with bf16 output (s2i_bf16.h says what the
// path is).
#include "s2i_bf16.h"

namespace {

// ---- weights: packed fp32 P[Tsrc][R][C] -> bf16 Wb[phase][chunk][tap][Npad][CK] -------------------------------------
//   transpose = 0 (forward): n = column of P (cout), k = row of P (cin)
//   transpose = 1 (input gradient): n = row of P (cin), k = column of P (cout)
// One thread per 16-byte output segment; for transpose = 0 the 8 values of a segment are a column walk of P, so a
// 32 x 32 tile goes through LDS (reads coalesced along the columns of P, writes along k).
__device__ __forceinline__ int src_tap(int kind, int flip, int T, int t, int phase) {
  if (kind == KB_TCONV) {
    const int py = phase >> 1, px = phase & 1, a = t >> 1, b = t & 1;
    const int k4y = py ? (a ? 0 : 2) : (a ? 3 : 1);
    const int k4x = px ? (b ? 0 : 2) : (b ? 3 : 1);
    return k4y * 4 + k4x;
  }
  return flip ? (T - 1 - t) : t;
}

constexpr int PACK16_KT = 4;   // 32 x 32 tiles per block of the batched re-pack (even)

__device__ __forceinline__ void pack_bf16_block(const float* __restrict__ P, unsigned short* __restrict__ out, int R, int C,
                                                int kind, int flip, int transpose, int T, int Nn, int Npad, int Kk,
                                                int CK, int bx, int by, int zt, float (&tile)[32][33]) {
  const int phase = zt / T, t = zt - phase * T;   // zt = phase * T + t
  const int ts = src_tap(kind, flip, T, t, phase);
  const float* sp = P + (size_t)ts * R * C;
  const int n0 = bx * 32, k0 = by * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  // tile[kl][nl]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v = 0.f;
    if (!transpose) {
      const int k = k0 + ty + 8 * q, n = n0 + tx;      // P[k][n], coalesced along n
      if (k < Kk && n < Nn) v = sp[(size_t)k * C + n];
      tile[ty + 8 * q][tx] = v;
    } else {
      const int n = n0 + ty + 8 * q, k = k0 + tx;      // P[n][k], coalesced along k
      if (k < Kk && n < Nn) v = sp[(size_t)n * C + k];
      tile[tx][ty + 8 * q] = v;
    }
  }
  __syncthreads();
  // 32 n x 4 segments of 8 k
  if (threadIdx.x < 128) {
    const int nl = threadIdx.x >> 2, sg = threadIdx.x & 3;
    const int n = n0 + nl, k = k0 + sg * 8;
    if (n < Npad && k < Kk) {
      const int nchunk = Kk / CK;
      const int cc = k / CK, kc = k - cc * CK;
      u32x4 v;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        f32x2 f = {tile[sg * 8 + 2 * h][nl], tile[sg * 8 + 2 * h + 1][nl]};
        v[h] = __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
      }
      const size_t o = ((((size_t)phase * nchunk + cc) * T + t) * Npad + n) * CK + kc;
      *reinterpret_cast<u32x4*>(out + o) = v;
    }
  }
}

// PACK16_KT tiles of 32 x 32 in one block, side by side along the SOURCE-contiguous dimension (n for the forward layout, k for
// the transposed one): all loads of the strip are issued before the one barrier (16 in flight per thread instead of 4), and a
// source row contributes 512 contiguous bytes to a block instead of 128 (round 3: D_NET256's re-pack 283 -> 237 us with the
// tiles walked one after another, -> see profiles/README.md for this form).
__device__ __forceinline__ void pack_bf16_strip(const s2i_pack16_item& it, int bx, int by, int zt,
                                                float (&tile)[PACK16_KT][33][33]) {   // 33 x 33: tile i starts one bank later
  const int T = it.T, C = it.C, Kk = it.Kk, Nn = it.Nn, Npad = it.Npad, CK = it.CK;
  const int phase = zt / T, t = zt - phase * T;
  const int ts = src_tap(it.kind, it.flip, T, t, phase);
  const float* sp = it.P + (size_t)ts * it.R * C;
  // 16-byte loads: a strip row is PACK16_KT * 32 floats = 32 lanes x 4; eight rows per pass, four passes
  static_assert(PACK16_KT == 4, "a strip row is covered by 32 lanes of four floats");
  const int c4 = threadIdx.x & 31, r8 = threadIdx.x >> 5;
  const int i = c4 >> 3, cl = (c4 & 7) * 4;          // tile of the strip, first of the lane's four columns inside it
  const bool vec_ok = (C & 3) == 0 && ((size_t)sp & 15) == 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int rl = r8 + 8 * q;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!it.transpose) {
      const int k = by * 32 + rl, n = (bx * PACK16_KT) * 32 + c4 * 4;      // P[k][n .. n + 3]
      if (k < Kk && n < Nn) {
        const float* src = sp + (size_t)k * C + n;
        if (vec_ok && n + 3 < C) v = *reinterpret_cast<const f32x4*>(src);
        else
#pragma unroll
          for (int j = 0; j < 4; ++j) if (n + j < C) v[j] = src[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (n + j >= Nn) v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[i][rl][cl + j] = v[j];
    } else {
      const int n = bx * 32 + rl, k = (by * PACK16_KT) * 32 + c4 * 4;      // P[n][k .. k + 3]
      if (n < Nn && k < Kk) {
        const float* src = sp + (size_t)n * C + k;
        if (vec_ok && k + 3 < C) v = *reinterpret_cast<const f32x4*>(src);
        else
#pragma unroll
          for (int j = 0; j < 4; ++j) if (k + j < C) v[j] = src[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (k + j >= Kk) v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[i][cl + j][rl] = v[j];
    }
  }
  __syncthreads();
  const int half = threadIdx.x >> 7, w = threadIdx.x & 127;
  const int nl = w >> 2, sg = w & 3;
  const int nchunk = Kk / CK;
#pragma unroll
  for (int j = 0; j < PACK16_KT / 2; ++j) {
    const int i = 2 * j + half;
    const int n0 = (it.transpose ? bx : bx * PACK16_KT + i) * 32, k0 = (it.transpose ? by * PACK16_KT + i : by) * 32;
    const int n = n0 + nl, k = k0 + sg * 8;
    if (n < Npad && k < Kk) {
      const int cc = k / CK, kc = k - cc * CK;
      u32x4 v;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        f32x2 f = {tile[i][sg * 8 + 2 * h][nl], tile[i][sg * 8 + 2 * h + 1][nl]};
        v[h] = __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
      }
      const size_t o = ((((size_t)phase * nchunk + cc) * T + t) * Npad + n) * CK + kc;
      *reinterpret_cast<u32x4*>(it.out + o) = v;
    }
  }
}

__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ P, unsigned short* __restrict__ out, int R,
                                                        int C, int kind, int flip, int transpose, int T, int nphase,
                                                        int Nn, int Npad, int Kk, int CK) {
  __shared__ float tile[32][33];
  pack_bf16_block(P, out, R, C, kind, flip, transpose, T, Nn, Npad, Kk, CK, blockIdx.x, blockIdx.y, blockIdx.z, tile);
}

// every bf16 weight copy of a network in ONE launch (after the fused Adam): item k owns the linear blocks
// [block0, block0 + gx * gy * nphase * T), block0 ascending
__global__ __launch_bounds__(256) void pack_bf16_batched_kernel(const s2i_pack16_item* __restrict__ items, int n) {
  __shared__ float tile[PACK16_KT][33][33];
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {                       // last item with block0 <= b
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].block0 <= b) lo = mid;
    else hi = mid - 1;
  }
  const s2i_pack16_item it = items[lo];
  const int r = b - it.block0;
  const int bx = r % it.gx, by = (r / it.gx) % it.gy, zt = r / (it.gx * it.gy);   // it.gx / it.gy count STRIPS
  pack_bf16_strip(it, bx, by, zt, tile);
}

// ---- split-K reduction with bf16 output (+ BatchNorm column statistics), as splitk_reduce_stats_kernel -----------------
__global__ __launch_bounds__(256) void splitk_reduce_bf16_kernel(const float* __restrict__ slab, int S, long long rows,
                                                                 int N, unsigned short* __restrict__ y, int ldy,
                                                                 float* __restrict__ part, int nparts, int cpb, int ppg,
                                                                 long long Rg) {
  __shared__ f32x4 sh[2][256];
  const int tid = threadIdx.x;
  const int rpb = 256 / cpb;
  const int ql = tid % cpb, rl = tid / cpb;
  const int quad = blockIdx.y * cpb + ql;
  const int Q = N / 4;
  const int grp = blockIdx.x / ppg, pp = blockIdx.x - grp * ppg;
  const long long chunk = (Rg + ppg - 1) / ppg;
  const long long r0 = grp * Rg + pp * chunk;
  const long long gend = (grp + 1) * Rg < rows ? (grp + 1) * Rg : rows;
  const long long r1 = r0 + chunk < gend ? r0 + chunk : gend;
  const size_t sstride = (size_t)rows * N;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  if (quad < Q) {
    for (long long row = r0 + rl; row < r1; row += rpb) {
      const float* sp = slab + row * N + quad * 4;
      f32x4 v = *reinterpret_cast<const f32x4*>(sp);
      for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(sp + s * sstride);
      u32x2 o = {pack2(v[0], v[1]), pack2(v[2], v[3])};
      *reinterpret_cast<u32x2*>(y + row * ldy + quad * 4) = o;
      s0 += v;
      s1 += v * v;
    }
  }
  if (!part) return;
  sh[0][tid] = s0;
  sh[1][tid] = s1;
  __syncthreads();
  if (rl == 0 && quad < Q) {
    for (int r = 1; r < rpb; ++r) {
      s0 += sh[0][r * cpb + ql];
      s1 += sh[1][r * cpb + ql];
    }
    *reinterpret_cast<f32x4*>(part + ((size_t)0 * nparts + blockIdx.x) * N + quad * 4) = s0;
    *reinterpret_cast<f32x4*>(part + ((size_t)1 * nparts + blockIdx.x) * N + quad * 4) = s1;
  }
}

// what both re-pack entry points ask of their source: P[Tsrc][R][C] holds the N x Cx (wmode != 0) / Cx x N matrix of every tap
int pack_source_ok(const s2i_conv_desc* d, bool pointers, int R, int C) {
  S2I_REQUIRE(pointers, "pack(bf16): null pointer");
  const int Kk = d->Cx, Nn = d->N;
  if (d->wmode != 0) S2I_REQUIRE(R >= Nn && C >= Kk, "pack(bf16): P is %d x %d, need rows >= %d cols >= %d", R, C, Nn, Kk);
  else S2I_REQUIRE(R >= Kk && C >= Nn, "pack(bf16): P is %d x %d, need rows >= %d cols >= %d", R, C, Kk, Nn);
  return 0;
}

}  // namespace

int launch_splitk_reduce_bf16(const s2i_conv_desc* d, const BPlan& pl, unsigned short* y, float* part, const float* ws,
                              hipStream_t st) {
  S2I_REQUIRE((d->N % 4) == 0, "conv(bf16): split-K needs N %% 4 == 0");
  const int Q = d->N / 4;
  int cpb = 1;
  while (cpb < Q && cpb < 256) cpb <<= 1;
  const int groups = d->groups < 1 ? 1 : d->groups;
  const int nparts = stat_parts(pl, groups);
  hipLaunchKernelGGL(splitk_reduce_bf16_kernel, dim3(nparts, (Q + cpb - 1) / cpb), dim3(256), 0, st, ws, pl.splitk, pl.Mrows,
                     d->N, y, d->ldy, d->stats ? part : nullptr, nparts, cpb, nparts / groups, pl.Mrows / groups);
  S2I_LAUNCH_CHECK("splitk_reduce_bf16");
  return 0;
}

extern "C" int s2i_pack_conv_weight_bf16(const s2i_conv_desc* d, const float* packed, int R, int C, unsigned short* out,
                                         void* stream) {
  BPlan pl;
  if (plan_bf16(d, &pl) || pack_source_ok(d, packed && out, R, C)) return 1;
  dim3 grid(pl.Npad / 32, d->Cx / 32, pl.nphases * pl.T);
  hipLaunchKernelGGL(pack_bf16_kernel, grid, dim3(256), 0, (hipStream_t)stream, packed, out, R, C, pl.kb, d->flip,
                     d->wmode != 0, pl.T, pl.nphases, d->N, pl.Npad, d->Cx, pl.CK);
  S2I_LAUNCH_CHECK("pack_bf16");
  return 0;
}

extern "C" int s2i_pack16_item_fill(const s2i_conv_desc* d, const float* packed, int R, int C, unsigned short* out,
                                    s2i_pack16_item* item) {
  BPlan pl;
  if (plan_bf16(d, &pl)) return -1;
  if (pack_source_ok(d, packed && out && item, R, C)) return 1;
  const int transpose = d->wmode != 0, Kk = d->Cx;
  item->P = packed; item->out = out; item->R = R; item->C = C; item->kind = pl.kb; item->flip = d->flip;
  item->transpose = transpose; item->T = pl.T; item->nphase = pl.nphases; item->Nn = d->N; item->Npad = pl.Npad;
  item->Kk = Kk; item->CK = pl.CK; item->block0 = 0;
  // strips of PACK16_KT tiles along the source-contiguous dimension (pack_bf16_strip)
  item->gx = transpose ? pl.Npad / 32 : (pl.Npad / 32 + PACK16_KT - 1) / PACK16_KT;
  item->gy = transpose ? (Kk / 32 + PACK16_KT - 1) / PACK16_KT : Kk / 32;
  return item->gx * item->gy * pl.nphases * pl.T;   // blocks of this item
}

extern "C" int s2i_pack_conv_weights_bf16_batched(const s2i_pack16_item* items_dev, int n, int total_blocks, void* stream) {
  S2I_REQUIRE(items_dev && n > 0 && total_blocks > 0, "pack(bf16, batched): empty table");
  hipLaunchKernelGGL(pack_bf16_batched_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, items_dev, n);
  S2I_LAUNCH_CHECK("pack_bf16_batched");
  return 0;
}
