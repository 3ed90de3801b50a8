// What two or more of the HBM-bound units share (internal; s2i_bn.hip, s2i_layout.hip, s2i_cvec.hip, s2i_losses.hip,
// s2i_rnn.hip, s2i_optim.hip, s2i_grid.hip): the sigmoid forms, the 16-byte and scalar loads / stores of fp32 and bf16 tensors, the
// thread layout of the per-channel reductions, the grid of a grid-stride launch, the stream and dtype-check macros.  A
// helper that one unit alone uses stays in that unit.  Kernels are never declared here: each __global__ kernel is defined
// and instantiated in exactly one unit.
#pragma once
#include "s2i_common.h"
#include <math.h>

namespace {
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }
// the gate of the GLU passes over bf16 tensors: v_rcp_f32 (1 ulp) instead of the IEEE division sequence (v_div_scale x2,
// v_rcp, four v_fma, v_div_fmas, v_div_fixup): those passes are VALU-bound (tools/elementwise_bench.py: GLU backward
// reduce 1.75 -> 2.64 TB/s), and the gate's relative error stays ~1e-7, far below the bf16 rounding of its operands.
// fp32 tensors, the logit heads and the LSTM keep the exact form (the fp32 parity tests sit on LeakyReLU decisions that a
// 1e-7 perturbation re-rolls).
struct bf16_t;
template <typename T> __device__ __forceinline__ float sigmoid_gate_(float v) {
  if constexpr (sizeof(T) == 2) return __builtin_amdgcn_rcpf(1.f + __expf(-v));
  else return 1.f / (1.f + __expf(-v));
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// activation tensors are fp32 or bf16 (bf16 activation mode, BASELINE config 4): T = float | bf16_t; the arithmetic of
// every kernel below stays fp32, only the HBM representation changes
struct bf16_t { unsigned short v; };
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2_ __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 ld4(const bf16_t* p) {
  const u32x2 h = *reinterpret_cast<const u32x2*>(p);
  return f32x4{__builtin_bit_cast(float, h[0] << 16), __builtin_bit_cast(float, h[0] & 0xffff0000u),
               __builtin_bit_cast(float, h[1] << 16), __builtin_bit_cast(float, h[1] & 0xffff0000u)};
}
__device__ __forceinline__ void st4(bf16_t* p, f32x4 v) {
  const f32x2_ a = {v[0], v[1]}, b = {v[2], v[3]};
  *reinterpret_cast<u32x2*>(p) = u32x2{__builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2_)),
                                       __builtin_bit_cast(unsigned, __builtin_convertvector(b, bf16x2_))};
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return __builtin_bit_cast(float, (unsigned)p->v << 16); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { p->v = __builtin_bit_cast(unsigned short, (__bf16)v); }

// thread layout for per-channel reductions over the rows of an [M][C] tensor:
// `cpb` threads across channel quads, 256/cpb row lanes.
struct RedGeom {
  int Q, cpb, rpb, gy;
};
static RedGeom red_geom(int C) {
  RedGeom g;
  g.Q = C / 4;
  int cpb = 1;
  while (cpb < g.Q && cpb < 256) cpb <<= 1;
  g.cpb = cpb;
  g.rpb = 256 / cpb;
  g.gy = (g.Q + cpb - 1) / cpb;
  return g;
}

// blocks of a grid-stride launch over `total` items, at most `cap`
inline int grid_for(long long total, int block = 256, int cap = 2048 * 4) {
  long long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
}  // namespace

// every entry point takes its stream as `void* stream`
#define ST ((hipStream_t)stream)
#define S2I_DT_CHECK(dt, name) S2I_REQUIRE((dt) == S2I_DT_F32 || (dt) == S2I_DT_BF16, name ": unknown dtype %d", (dt))
