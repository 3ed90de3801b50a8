// Pieces shared by the implicit-GEMM convolution units (internal, next to s2i_tile.h): the kernel parameter block and gather
// helpers of the StackGAN-v2 convolutions, the fp32 matrix loop, the bounds-checked loads, the bf16 split, the two plans
// and the host functions that cross a unit boundary.  Only what two or more units use lives here; a helper of one family
// stays in that family's file.  Kernels are never declared here: each __global__ template is defined in one unit, or in
// one private header where several units instantiate it (s2i_conv_fwd.h), every instantiation is compiled in exactly one
// unit, and the other units reach it through the launch_* host functions below.
//
// One gather formulation covers every convolution on the StackGAN-v2 path
// (reference StackGAN_v2/model.py:125-140, 144-169, 287-298, 358-398):
//   K1    : 1x1 / nn.Linear
//   K3S1  : conv3x3 pad 1 (and, with flipped taps + transposed weights, its input gradient)
//   K4S2  : Conv2d(k4,s2,p1) of the D towers; also the input gradient of an upBlock
//   TCONV : 4-phase transposed k4 s2 p1 conv = nearest-x2 upsample + conv3x3 collapsed to 2x2 taps
//           per output parity (2.25x fewer MACs than the literal upsample+conv); also the input
//           gradient of Conv2d(k4,s2,p1)
// Activations are NHWC so the K (channel) direction of the gather is contiguous in HBM; a per-image
// vector (c_code) can be concatenated in front of the stored channels without materialising the
// torch.cat of model.py:277/434.
#pragma once
#include "s2i_common.h"
#include "s2i_tile.h"

struct IgemmP {
  const float* __restrict__ x;
  const float* __restrict__ cvec;
  const float* __restrict__ w;
  const float* __restrict__ bias;
  const float* __restrict__ cls_bias;
  float* __restrict__ y;
  float* __restrict__ part;
  float* __restrict__ slab;
  int B, H, W, Cx, Cc, Ca;
  int Ho, Wo, lgWo, lgHoWo;
  int M, N, K, T;
  int kind, flip, act, stats, splitk, cps, nchunks;
  int ldw, wR, ldy, nparts;
  int g_kw, g_s, g_pad;  // geometry of S2I_CONV_1D (1 x kw taps along W, stride, padding)
  int wt;                // weights read transposed per tap (small_n_conv_kernel; the igemm takes it as a template flag)
  int x16, y16;          // x / y hold bf16 instead of fp32 (bf16 activation mode: the arithmetic here stays fp32)
  unsigned x_bytes, c_bytes, w_bytes;
  long long Mrows;
  // split-bf16 weights [plane][tap][n][k] (igemm_fwd_split_kernel)
  const unsigned short* __restrict__ wsp;
  int wsp_np, wsp_kp, wsp_plane;  // rows per tap, row length (bf16 elements), elements per plane
  unsigned wsp_bytes;
  // apply-on-load (INACT instantiations): x holds the RAW output of the producing convolution; the gather applies that
  // layer's BatchNorm (scale, shift from its (groups, 4, Cx) coefficient table) and LeakyReLU while it stages the operand
  const float* __restrict__ in_coef;
  int in_rows_per_group;   // output rows of THIS launch per BatchNorm group of the producer (rows beyond: next group)
};

// stride, padding and taps per kernel row of a kind; S2I_CONV_1D takes its own from the descriptor (IgemmP::g_*; the weight
// gradient has no 1-D form and passes the 1 x 1 values)
__device__ __forceinline__ void geom(int kind, int s1d, int pad1d, int kw1d, int& s, int& pad, int& kw) {
  if (kind == S2I_CONV_1D) { s = s1d; pad = pad1d; kw = kw1d; }
  else if (kind == S2I_CONV_K3S1) { s = 1; pad = 1; kw = 3; }
  else if (kind == S2I_CONV_K4S2) { s = 2; pad = 1; kw = 4; }
  else { s = 1; pad = 0; kw = 1; }
}

__device__ __forceinline__ void tap_delta(int kind, int kw, int t, int py, int px, int& dy, int& dx) {
  if (kind == S2I_TCONV_K4S2) {
    const int a = t >> 1, b = t & 1;
    dy = a ? (py ? 1 : -1) : 0;
    dx = b ? (px ? 1 : -1) : 0;
  } else if (kind == S2I_CONV_1D) {
    dy = 0;
    dx = t;
  } else {
    dy = t / kw;
    dx = t - dy * kw;
  }
}

// bit t set <=> tap t of the pixel whose base coordinate is (by,bx) falls inside the H x W tensor
__device__ __forceinline__ unsigned tap_mask(int kind, int kw, int by, int bx, int H, int W, int py, int px) {
  if (kind == S2I_TCONV_K4S2) {
    const int sy = py ? 1 : -1, sx = px ? 1 : -1;
    const bool y0 = by >= 0 && by < H, y1 = by + sy >= 0 && by + sy < H;
    const bool x0 = bx >= 0 && bx < W, x1 = bx + sx >= 0 && bx + sx < W;
    return (unsigned)(y0 && x0) | ((unsigned)(y0 && x1) << 1) | ((unsigned)(y1 && x0) << 2) |
           ((unsigned)(y1 && x1) << 3);
  }
  unsigned cols = 0, mask = 0;
  for (int kx = 0; kx < kw; ++kx) cols |= (unsigned)(bx + kx >= 0 && bx + kx < W) << kx;
  if (kind == S2I_CONV_1D) return (by >= 0 && by < H) ? cols : 0u;
  for (int ky = 0; ky < kw; ++ky)
    if (by + ky >= 0 && by + ky < H) mask |= cols << (ky * kw);
  return mask;
}

// which tap of the packed weight tensor the gather tap t multiplies
__device__ __forceinline__ int tap_weight(int kind, int flip, int T, int t, int py, int px) {
  if (kind == S2I_TCONV_K4S2) {
    const int a = t >> 1, b = t & 1;
    const int k4y = py ? (a ? 0 : 2) : (a ? 3 : 1);
    const int k4x = px ? (b ? 0 : 2) : (b ? 3 : 1);
    return k4y * 4 + k4x;
  }
  return flip ? (T - 1 - t) : t;
}

// output pixel of GEMM row m (the output extents are powers of two); P: IgemmP, or WgradP whose pixels are the reduction index
template <class P>
__device__ __forceinline__ void row_pixel(const P& p, int m, int& b, int& oy, int& ox) {
  b = m >> p.lgHoWo;
  const int r = m & ((1 << p.lgHoWo) - 1);
  oy = r >> p.lgWo;
  ox = r & (p.Wo - 1);
}

// One 32-deep K chunk: 16 k-pairs, each TM x TN v_mfma_f32_32x32x2_f32.  The fragments of pair kk+1 are read
// from LDS BEFORE the MFMAs of pair kk are issued (two register sets), so the LDS latency sits behind 4+ MFMAs
// of this wave instead of relying on the other waves of the SIMD to cover it.
template <int TM, int TN, int LDA, int LDB, int KK0 = 0, int KK1 = 16>
__device__ __forceinline__ void mma_chunk(const float* As, const float* Bs, int arow0, int bcol0,
                                          int lane, f32x16 (&acc)[TM][TN]) {
  static_assert((KK1 - KK0) % 2 == 0, "k-pairs are processed two at a time");
  const int l31 = lane & 31, lh = lane >> 5;
  const float* ap = As + lh * LDA + arow0 + l31;
  const float* bp = Bs + lh * LDB + bcol0 + l31;
  float a0[TM], b0[TN], a1[TM], b1[TN];  // two named fragment sets (a runtime-indexed pair would go to scratch)
#pragma unroll
  for (int i = 0; i < TM; ++i) a0[i] = ap[(2 * KK0) * LDA + i * 32];
#pragma unroll
  for (int j = 0; j < TN; ++j) b0[j] = bp[(2 * KK0) * LDB + j * 32];
#pragma unroll
  for (int kk = KK0; kk < KK1; kk += 2) {
#pragma unroll
    for (int i = 0; i < TM; ++i) a1[i] = ap[(2 * (kk + 1)) * LDA + i * 32];
#pragma unroll
    for (int j = 0; j < TN; ++j) b1[j] = bp[(2 * (kk + 1)) * LDB + j * 32];
    // pin the order (hipcc otherwise sinks the reads next to their use): next pair's LDS reads, THEN this pair's
    // MFMAs.  Only for the 2x2 wave tile: with fewer MFMAs per pair the pinned schedule makes hipcc spill.
    if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i], b0[j], acc[i][j], 0, 0, 0);
    if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
    if (kk + 2 < KK1) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a0[i] = ap[(2 * (kk + 2)) * LDA + i * 32];
#pragma unroll
      for (int j = 0; j < TN; ++j) b0[j] = bp[(2 * (kk + 2)) * LDB + j * 32];
    }
    if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i], b1[j], acc[i][j], 0, 0, 0);
    if constexpr (TM * TN >= 4) __builtin_amdgcn_sched_barrier(0);
  }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define S2I_OOB 0x7ffffff0  // byte offset past any tensor: the buffer bounds check returns zeros

__device__ __forceinline__ f32x4 bload4(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
// four consecutive elements at the byte offset an fp32 tensor would have; `is16`: the tensor holds bf16 (half the offset)
__device__ __forceinline__ f32x4 bload4_any(__amdgpu_buffer_rsrc_t r, int byte_off, int is16) {
  if (!is16) return bload4(r, byte_off);
  const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off == S2I_OOB ? S2I_OOB : (byte_off >> 1), 0, 0);
  return f32x4{__builtin_bit_cast(float, v[0] << 16), __builtin_bit_cast(float, v[0] & 0xffff0000u),
               __builtin_bit_cast(float, v[1] << 16), __builtin_bit_cast(float, v[1] & 0xffff0000u)};
}

// split-bf16 operands (igemm_fwd_split_kernel, igemm_wgrad_split_kernel): v = v1 + v2 + v3 with v1 = bf16(v), v2 = bf16(v - v1), ...
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int NP>
__device__ __forceinline__ void split4(const f32x4 v, u32x2 (&out)[NP]) {
  f32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) {
    const unsigned pa = __builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2));
    const unsigned pb = __builtin_bit_cast(unsigned, __builtin_convertvector(b, bf16x2));
    out[pl] = u32x2{pa, pb};
    if (pl + 1 < NP) {
      a[0] -= __builtin_bit_cast(float, pa << 16);
      a[1] -= __builtin_bit_cast(float, pa & 0xffff0000u);
      b[0] -= __builtin_bit_cast(float, pb << 16);
      b[1] -= __builtin_bit_cast(float, pb & 0xffff0000u);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------
// What the operands of a forward convolution are (derived once from the entry point's arguments by fwd_mode)
struct FwdMode {
  int x16, y16;         // x / y stored as bf16 (s2i_conv_forward_dt)
  int planes;           // bf16 planes of pre-split weights (s2i_conv_forward_split), 0 = fp32 weights
  bool bias, cls_bias;  // a bias / class-bias table is passed
  bool in_act;          // x is the producer's raw output, activated while it is staged (s2i_conv_forward_in)
};

// The kernel a planned forward convolution launches.  The matrix families list their tile shapes in one order (F32 and
// F32IN all four, SPLIT the first three), so a family's first value + the shape's index is the kernel; the WT / CA32 template
// flags of igemm_fwd_kernel and the plane count are plan fields.  fwd_kernels[] (s2i_conv_plan.hip) holds each one's rows and
// columns per block and its block size; s2i_conv_plan_query reports these values.
enum FwdKernel {
  FWD_F32_128x128, FWD_F32_128x64, FWD_F32_128x32, FWD_F32_96x128,           // igemm_fwd_kernel<BM, BN, ..., WT, CA32>
  FWD_F32IN_128x128, FWD_F32IN_128x64, FWD_F32IN_128x32, FWD_F32IN_96x128,   // ... <..., false, true, INACT>: apply-on-load
  FWD_SPLIT_128x128, FWD_SPLIT_128x64, FWD_SPLIT_128x32,                     // igemm_fwd_split_kernel<..., planes>
  FWD_SMALLN_4, FWD_SMALLN_8, FWD_SMALLN_16,                                 // small_n_conv_kernel<Ca / 4>
  FWD_TCONV_N4_64,                                                           // tconv_n4_tile_kernel<64>
  FWD_CONV3_N4_16, FWD_CONV3_N4_32,                                          // conv3_n4_tile_kernel<CCH>; Ca = 64: <32>, two chunks
  FWD_RGB_OUT_4, FWD_RGB_OUT_8, FWD_RGB_OUT_9, FWD_RGB_OUT_16, FWD_RGB_OUT_18, FWD_RGB_OUT_36,   // rgb_out_kernel<KSTEPS>
  FWD_RGB_IN_1x3, FWD_RGB_IN_2x3, FWD_RGB_IN_1x4, FWD_RGB_IN_2x4,            // rgb_in_kernel<MT, KH>
  FWD_THIN_OUT,                                                              // thin_out_kernel
  FWD_THIN_IN_16, FWD_THIN_IN_32,                                            // thin_in_kernel<NOUT>
  FWD_KERNEL_COUNT
};
struct FwdKernelInfo { int bm, bn, threads; };   // output rows (pixels of one phase) and columns per block, block size

// What follows the main launch where K is split
enum FwdReduce {
  FWD_REDUCE_NONE,       // K is not split, or the kernel does not split it
  FWD_REDUCE_PLAIN,      // splitk_reduce_kernel
  FWD_REDUCE_COLSTATS,   // splitk_reduce_kernel, then s2i_colstats over y (statistics where N or ldy is no multiple of 4)
  FWD_REDUCE_STATS       // splitk_reduce_stats_kernel
};

// Everything a forward launch needs, decided by plan_fwd; the launchers take it as const
struct FwdPlan {
  int T, K, Ca, Ho, Wo, M, nphases;
  long long Mrows;
  // the matrix tiling of the layer (plan_fwd_tiles): the statistics rows and the split eligibility follow from it alone.
  // A vector-unit kernel that takes the layer ignores the split but the workspace still holds its slabs, as it always has.
  int bm, gridM, gridN, nchunks, splitk, cps;
  FwdKernel kernel;
  bool wt, ca32;        // template flags of igemm_fwd_kernel
  int planes;           // bf16 planes of the SPLIT family (else 0)
  int threads, gx, gy, gz;
  int prep_elems;       // elements thin_table_kernel / rgb_afrag_kernel writes into the workspace before the main launch (0: none)
  FwdReduce reduce;
  size_t ws_bytes;      // the larger of the split-K slabs and the table / fragment buffer; the launch refuses less
};

// What the operands of a weight gradient are (derived once from the entry point's dtypes, planes and coefficient table)
enum WgMode {
  WG_MODE_F32,      // fp32 a and g
  WG_MODE_F32_IN,   // fp32, a is the producer's raw output activated while it is staged (s2i_conv_wgrad_in)
  WG_MODE_A16,      // a stored as bf16, g fp32
  WG_MODE_G16,      // g stored as bf16, a fp32
  WG_MODE_B16,      // both stored as bf16
  WG_MODE_SPLIT1, WG_MODE_SPLIT2, WG_MODE_SPLIT3   // fp32 operands split into 1 - 3 bf16 planes while they are staged
};

// The kernel a planned weight gradient launches: family and K x N tile.  The matrix families list their tile shapes in one
// order (F32 all eight, B16 the first six, SPLIT the first four), so a family's first value + the shape's index is the kernel.
// wg_kernels[] (s2i_wgrad_plan.hip) holds each one's tile and block size; s2i_wgrad_plan_query reports these values.
enum WgKernel {
  WG_F32_128x128, WG_F32_128x64, WG_F32_128x32, WG_F32_64x64, WG_F32_256x128, WG_F32_256x256, WG_F32_96x64, WG_F32_96x32,
  WG_F32IN_128x128,                                                       // igemm_wgrad_kernel<..., INACT>
  WG_B16_128x128, WG_B16_128x64, WG_B16_128x32, WG_B16_64x64, WG_B16_256x128, WG_B16_256x256,   // igemm_wgrad_b16_kernel
  WG_B16D1_64x64,                                                         // ... with the fp32 NHWC4 image of the first D conv
  WG_SPLIT_128x128, WG_SPLIT_128x64, WG_SPLIT_128x32, WG_SPLIT_64x64,     // igemm_wgrad_split_kernel<..., planes>
  WG_ROWS3_32x64, WG_ROWS3_32x32, WG_ROWS3_64x128, WG_ROWS3_64x64, WG_ROWS3_64x32,   // wgrad_k3_rows_kernel<Ca, BN>
  WG_SMALLN_16, WG_SMALLN_32, WG_SMALLN_64,                               // small_n_wgrad_kernel<Ca / 4>
  WG_KERNEL_COUNT
};
struct WgKernelInfo { int bm, bn, threads; };   // K rows and N columns of the result per block, block size

// Everything a weight-gradient launch needs, decided by plan_wgrad; the launcher takes it as const
struct WgPlan {
  int T, K, Cin, Ho, Wo, M;
  WgKernel kernel;
  int planes;           // bf16 planes of the SPLIT family (else 0)
  int threads, gx, gy, gz;
  int stage;            // pixels per stage of the kernel's reduction loop: 32, or 64 in the B16 families
  int nchunks, cps;     // stages in the pixel range and stages per split (WgradP::nchunks / cps)
  int slabs;            // K x N fp32 slabs the launch writes and the finish sums
  int ws_slabs;         // slabs the workspace holds: the split of the 32-pixel plan, >= slabs
};
// bytes of the workspace every s2i_wgrad_workspace_bytes* query reports and the launcher asks for
static inline size_t wg_workspace_bytes(const WgPlan& pl, int N) { return (size_t)pl.ws_slabs * pl.K * N * sizeof(float); }

// Unit interfaces.  An int launch_* function returns 0 after a launch, 1 with the error text set.  None of them is exported.
#pragma GCC visibility push(hidden)
// s2i_conv_plan.hip: both return 0, or 1 with the error text set.  fwd_mode names the operands of an entry point's
// arguments; plan_fwd decides the launch, or refuses a layer that no kernel takes in this mode.
int fwd_mode(int x16, int y16, int planes, bool bias, bool cls_bias, bool in_coef, FwdMode* mode);
int plan_fwd(const s2i_conv_desc* d, const FwdMode& mode, FwdPlan* pl);
// s2i_conv_fwd.hip: the matrix families (the byte windows of p come from conv_forward_impl), small_n_conv_kernel and the
// reduction of a split
int launch_igemm_fwd(const FwdPlan& pl, const IgemmP& p, hipStream_t st);
// s2i_conv_fwd_<BM>x<BN>.hip, s2i_conv_fwd_split.hip: the instantiations of one fp32 tile shape each, and of the split-bf16
// tiles.  Only launch_igemm_fwd calls them; they launch and return nothing, the launch check is its.
void launch_fwd_128x128(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st);
void launch_fwd_128x64(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st);
void launch_fwd_128x32(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st);
void launch_fwd_96x128(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st);
void launch_fwd_split(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st);
int launch_small_n_conv(const FwdPlan& pl, const IgemmP& p, hipStream_t st);
int launch_splitk_reduce(const s2i_conv_desc* d, const FwdPlan& pl, const float* bias, float* y, float* part, void* ws,
                         int y16, void* stream);
// s2i_conv_thin.hip: the thin-layer and RGB kernels (FWD_TCONV_N4_64 ... FWD_THIN_IN_32) after their table / fragment
// preparation in ws
int launch_thin(const s2i_conv_desc* d, const FwdPlan& pl, const IgemmP& p, void* ws, hipStream_t st);
// s2i_wgrad_plan.hip: both return 0, or 1 with the error text set.  wg_mode names the operands of an entry point's
// arguments; plan_wgrad decides the launch, or refuses a layer that no kernel takes in this mode.
int wg_mode(int a16, int g16, int planes, bool a_coef, WgMode* mode);
int plan_wgrad(const s2i_wgrad_desc* d, WgMode mode, WgPlan* pl);
#pragma GCC visibility pop
