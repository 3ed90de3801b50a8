// Pieces shared by the units of the bf16 activation path (internal, next to s2i_tile.h; BASELINE config 4): implicit-GEMM
// convolutions whose activations live in HBM as bf16 NHWC, weights as bf16 (fp32 masters stay in the trainer's flat buffers),
// products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, BatchNorm statistics taken from the fp32 accumulators.
//   s2i_bf16_conv.hip     the 128-pixel kernel        s2i_bf16_pack.hip   weight re-pack, split-K reduction with bf16 output
//   s2i_bf16_conv_v2.hip  the 256-pixel kernel        s2i_bf16_plan.hip   plan_bf16, its query, the entry point (no kernel)
// Only what two or more units use lives here.  Kernels are never declared here: each __global__ template is defined and
// instantiated in exactly one unit and reached from the others through the launch_* host functions below.
//
// What is different from the fp32 / split kernels of s2i_conv_fwd.h (which gather an im2col chunk per 32-deep K step
// from global memory, i.e. pull every input pixel through L2 once per tap):
//   * the block stages a 2-D input PATCH with its halo in LDS once per channel chunk -- the pixels of TB images x
//     (TH-1)*s+KH rows x (TW-1)*s+KW columns -- and every tap reads its MFMA A-fragments from that patch at a
//     wave-uniform offset.  Out-of-image halo pixels are zero-filled by the bounds-checked buffer load, so the
//     matrix loop has no masks at all;
//   * the K loop runs (channel chunk, tap group) instead of (tap, channel): one LDS stage carries all 9 taps of a
//     3x3 (8 of the 16 taps of a 4x4, the 4 taps of one transposed-conv phase) for CK channels, 32-36 MFMAs per wave
//     between two barriers instead of 8;
//   * weights are pre-arranged at pack time in exactly the order the stages consume them,
//     Wb[phase][chunk][tap][n][CK] (tap flip / transposition / parity tap selection of the input-gradient forms
//     already applied), so a stage's B tile is ONE contiguous run of global memory;
//   * LDS rows are CK*2 bytes (32 / 64 / 128) with the 16-byte segments XOR-swizzled by the row index, so a
//     ds_read_b128 fragment read is conflict-free without padding;
//   * bf16 results leave through an LDS transpose and 16-byte row-contiguous stores.
// Rows of the GEMM are output pixels; a block owns a tile of 128 (256) of them shaped TB x TH x TW (powers of two) chosen
// from the map size, e.g. 4 x 32 pixels of one image on wide maps, 8 whole 4x4 maps at the discriminators' tails.
#pragma once
#include "s2i_common.h"
#include "s2i_tile.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#define S2I_OOB 0x7ffffff0

enum { KB_K3S1 = 0, KB_K4S2 = 1, KB_TCONV = 2 };

struct ConvBP {
  const unsigned short* __restrict__ x;
  const unsigned short* __restrict__ w;
  const float* __restrict__ cls_bias;
  unsigned short* __restrict__ y;
  float* __restrict__ part;
  float* __restrict__ slab;
  int B, H, W, C;
  int Ho, Wo;              // output grid of one phase
  int N, Npad, ldy;
  int lgTW, lgTH, lgTB;
  int tilesX, tilesY;      // tiles per image along x / y (powers of two)
  int ntiles;              // tiles in all (tilesX * tilesY * image groups)
  int PH, PW, npix;
  int nchunk, splitk, cps;
  int stats, nparts;
  long long Mrows;         // rows of y (all phases)
  unsigned x_bytes, w_bytes;
  int dbg;                 // ablation switches of tools/conv16_bench.py (S2I_B16_DBG; 0 in production): 1 no patch loads after
                           // the first, 2 no weight loads after the first, 4 no LDS staging after the first, 8 no MFMA,
                           // 16 no output stores
};

__device__ __forceinline__ u32x4 bload16(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
}

// output pixel of row r of the TB x TH x TW pixel tile at (b0, oy0, ox0); false beyond the batch
__device__ __forceinline__ bool tile_pixel(const ConvBP& p, int b0, int oy0, int ox0, int r, int& b, int& oy, int& ox) {
  const int TW = 1 << p.lgTW, TH = 1 << p.lgTH;
  const int tx = r & (TW - 1), ty = (r >> p.lgTW) & (TH - 1), tb = r >> (p.lgTW + p.lgTH);
  b = b0 + tb;
  oy = oy0 + ty;
  ox = ox0 + tx;
  return b < p.B;
}

// global row (pixel of y) of that tile row; false beyond the batch.  A transposed-conv phase (py, px) interleaves its rows.
template <int KIND>
__device__ __forceinline__ bool tile_out_row(const ConvBP& p, int b0, int oy0, int ox0, int py, int px, int r, long long& row) {
  int b, oy, ox;
  if (!tile_pixel(p, b0, oy0, ox0, r, b, oy, ox)) return false;
  if (KIND == KB_TCONV) row = ((long long)b * (2 * p.Ho) + 2 * oy + py) * (2 * p.Wo) + 2 * ox + px;
  else row = ((long long)b * p.Ho + oy) * p.Wo + ox;
  return true;
}

__device__ __forceinline__ unsigned pack2(float a, float b) {
  f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// DBG & 32 (diagnostic build of tools/conv16_timeline.py only): wave 0 stamps s_memtime at the phase boundaries into a
// buffer of its own (p.slab, 64 stamps per block); no stamp executes in the production instantiation
template <int DBG>
__device__ __forceinline__ void bf16_stamp(const ConvBP& p, int tid, int i) {
  if constexpr ((DBG & 32) != 0) {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (tid == 0 && i < 64) {
      const size_t blk = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
      reinterpret_cast<unsigned long long*>(p.slab)[blk * 64 + i] = t;
    }
  }
}

// LDS bytes of the epilogue's transpose of a BM x BN bf16 tile: rows of BN * 2 bytes, 16 bytes apart
constexpr size_t bf16_epilogue_bytes(int bm, int bn) { return (size_t)bm * (bn * 2 + 16); }

// most patch pixels the 128-pixel / the 256-pixel kernel stages per channel chunk: the planner checks a patch against it, the
// kernel sizes its per-thread load plan by it
constexpr int bf16_max_pix(int kb, int ck) { return kb == KB_K4S2 ? (ck == 16 ? 800 : 672) : 320; }
constexpr int bf16_v2_max_pix(int kb) { return kb == KB_K4S2 ? 1280 : (kb == KB_K3S1 ? 416 : 336); }

// The accumulators of a block of BN channels become a bf16 tile in LDS, rows of BN * 2 bytes 16 bytes apart
// (bf16_epilogue_bytes; smem is free of the matrix loop's reads): lanes l and l^1 (columns c, c+1) exchange one register of
// each row pair so that every lane owns two adjacent columns of ONE row and writes them as a dword.  Ends at the barrier:
// the caller then stores the rows with 16-byte row-contiguous stores.
// Only conv_bf16_v2_kernel calls it.  conv_bf16_kernel keeps the same lines inline: with this function (in either form, to
// the barrier or with the stores) hipcc schedules the prologue of most of its instantiations differently.
template <int TM, int TN, int BN>
__device__ __forceinline__ void transpose_tile_bf16(unsigned char* smem, const f32x16 (&acc)[TM][TN], int lane, int wm, int wn,
                                                    int l31, int lh) {
  constexpr int ERS = BN * 2 + 16;
  const bool odd = lane & 1;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float mine0 = acc[i][j][2 * q], mine1 = acc[i][j][2 * q + 1];
        const float give = odd ? mine0 : mine1;
        const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, give), 0xB1, 0xF, 0xF, true));
        const int reg = 2 * q + (odd ? 1 : 0);
        const int rr = acc_row(wm, TM, i, reg, lh);
        const int col = acc_col(wn, TN, j, l31 & ~1);
        const unsigned v = odd ? pack2(got, mine1) : pack2(mine0, got);
        *reinterpret_cast<unsigned*>(smem + rr * ERS + col * 2) = v;
      }
  __syncthreads();
}

// ---- host side ---------------------------------------------------------------------------------
// Every instantiation of the two convolution kernels, each list in the order its unit instantiates them (that order is the
// layout of the unit's code object).  The B16Kernel values, the names, the planner's match and the two
// launch switches are generated from these lists and nothing else names an instantiation.
//   conv_bf16_kernel (128 pixels): kind, BN, CK, TG
#define S2I_BF16_TILES(X) \
  X(K3S1, 128, 16, 9) X(K3S1, 64, 32, 9) X(K3S1, 32, 64, 9) X(K3S1, 32, 32, 9) \
  X(K4S2, 128, 32, 4) X(K4S2, 128, 16, 8) X(K4S2, 64, 32, 8) X(K4S2, 32, 32, 8) \
  X(TCONV, 128, 32, 4) X(TCONV, 64, 64, 4) X(TCONV, 32, 64, 4) X(TCONV, 32, 32, 4)
//   conv_bf16_v2_kernel (256 pixels, BN = 128): id, kind, CK, TG, two patch buffers, padded patch width.  The two-buffer forms
//   first, the stride-2 forms last
#define S2I_BF16_V2_TILES(X) \
  X(V2_K3S1, K3S1, 32, 3, true, 0) X(V2_TCONV, TCONV, 64, 2, true, 0) X(V2_K4S2_PW66, K4S2, 32, 4, false, 66) \
  X(V2_K4S2, K4S2, 32, 4, false, 0)

enum B16Kernel {
  B16_NO_KERNEL = -1,   // planned, but conv_bf16_kernel is not instantiated for this (kind, BN, CK): the layer is not eligible
#define S2I_ID(K, bn, ck, tg) B16_##K##_##bn##x##ck,
  S2I_BF16_TILES(S2I_ID)
#undef S2I_ID
#define S2I_ID(id, K, ck, tg, pdb, pwc) B16_##id,
  S2I_BF16_V2_TILES(S2I_ID)
#undef S2I_ID
  B16_KERNEL_COUNT
};

// What a descriptor launches, all of it: plan_bf16 decides, s2i_conv_bf16_plan_query reports, the launch_* functions obey.
struct BPlan {
  int v2;   // conv_bf16_v2_kernel: 256-pixel tiles, 512 threads
  int kb, T, NG, TG, Ho, Wo, nphases, BN, CK, Npad;
  int lgTW, lgTH, lgTB, tilesX, tilesY, tilesB, PH, PW, npix;
  int nchunk, splitk, cps, gridM, gridN;
  long long Mrows;
  B16Kernel kernel;
  int threads, gx, smem;   // block size; grid x (gridM, or the block slots of the persistent form); dynamic LDS bytes
};

// more than 64 KB of dynamic LDS needs the attribute once per kernel: `raised` is the instantiation's own flag
inline int bf16_raise_lds(const void* kernel, int bytes, bool* raised) {
  if (*raised) return 0;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) S2I_FAIL("conv(bf16): hipFuncSetAttribute: %s", hipGetErrorString(e));
  *raised = true;
  return 0;
}

// Unit interfaces.  A launch_* function returns 0 after a launch, 1 with the error text set.  None of them is exported.
#pragma GCC visibility push(hidden)
// s2i_bf16_plan.hip: the one place that knows which kernel, grid and LDS size a descriptor launches; the kernels' names for
// error texts ("K3S1_128x16", "V2_K4S2_PW66"; _lib.B16_KERNELS holds the ones tools and tests read)
int plan_bf16(const s2i_conv_desc* d, BPlan* pl);
extern const char* const b16_kernel_names[B16_KERNEL_COUNT];
// s2i_bf16_conv.hip: the 128-pixel kernel (!pl.v2); s2i_bf16_conv_v2.hip: the 256-pixel kernel (pl.v2)
int launch_conv_bf16(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st);
int launch_conv_bf16_v2(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st);
// s2i_bf16_pack.hip: sums the pl.splitk slabs of ws into y (bf16) and, with part, the BatchNorm column statistics
int launch_splitk_reduce_bf16(const s2i_conv_desc* d, const BPlan& pl, unsigned short* y, float* part, const float* ws,
                              hipStream_t st);
#pragma GCC visibility pop
