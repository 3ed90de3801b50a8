// The per-step half of the image transform on resident uint8 images (StackGAN_v2/datasets.py:40-66 behind main.py:127-131):
// RandomCrop window, RandomHorizontalFlip, the two PIL-bilinear pyramid levels of that window, ToTensor + Normalize.
// Everything up to the final normalisation is integer arithmetic on tables the host computed the way PIL does, so the
// float planes are bit-identical to what the host path (PIL + to_normalized_tensor) produces for the same draws.
#include "s2i_common.h"

namespace {

constexpr int IP_BAND = 32;                      // level-0 rows per block: 16 rows of level 1, 8 rows of level 2
constexpr int IP_HALO = 2;                       // the scale-4 filter of output row y reads window rows 4y-2 .. 4y+5
constexpr int IP_ROWS = IP_BAND + 2 * IP_HALO;
constexpr int IP_SMAX = 256;                     // largest window the static LDS tiles hold
constexpr int IP_K1 = 4, IP_K2 = 8;              // taps per output position at scale 2 / scale 4
constexpr int IP_PRECISION_BITS = 32 - 8 - 2;    // PIL's 8-bit resample: 22-bit fixed-point coefficients

// ToTensor then Normalize(0.5, 0.5), the operations of u8_to_image_kernel in the same order
__device__ __forceinline__ float ip_norm(int u) {
  const float t = (float)u / 255.f;
  return (t - 0.5f) / 0.5f;
}

__device__ __forceinline__ int ip_clip8(unsigned acc) {
  const int v = (int)acc >> IP_PRECISION_BITS;
  return min(max(v, 0), 255);
}

// One tap sum of PIL's ImagingResampleHorizontal_8bpc / Vertical_8bpc.  p points at sample `first`, samples lie `step`
// bytes apart; the tap index is clamped to [first, last] so that no table content can take a read outside the tile (a
// clamped tap of a PIL table has coefficient 0).
template <int K>
__device__ __forceinline__ int ip_taps(const unsigned char* __restrict__ p, int step, const int* __restrict__ tab,
                                       int first, int last) {
  const int start = tab[0];
  unsigned acc = 1u << (IP_PRECISION_BITS - 1);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int i = min(max(start + k, first), last);
    acc += (unsigned)p[(i - first) * step] * (unsigned)tab[1 + k];
  }
  return ip_clip8(acc);
}

// horizontal pass of one level over every staged row: src [nl][S][3] -> dst [nl][Wo][3], uint8 as in PIL
template <int K>
__device__ __forceinline__ void ip_horizontal(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                              const int* __restrict__ tab, int nl, int S, int Wo, int tid) {
  const int rb = Wo * 3;
  for (int e = tid; e < nl * rb; e += 256) {
    const int r = e / rb, j = e - r * rb;
    const int x = j / 3, ch = j - x * 3;
    dst[e] = (unsigned char)ip_taps<K>(src + r * S * 3 + ch, 3, tab + x * (K + 1), 0, S - 1);
  }
}

// vertical pass of one level for the block's output rows [y0, y0 + ny), normalised, x fastest so the plane stores coalesce
template <int K>
__device__ __forceinline__ void ip_vertical(const unsigned char* __restrict__ hz, const int* __restrict__ tab, int lo,
                                            int hi, int y0, int ny, int Wo, float* __restrict__ out, int tid) {
  const int rb = Wo * 3;
  for (int e = tid; e < ny * rb; e += 256) {
    const int y = e / rb, rem = e - y * rb;
    const int ch = rem / Wo, x = rem - ch * Wo;
    const int v = ip_taps<K>(hz + x * 3 + ch, rb, tab + (y0 + y) * (K + 1), lo, hi - 1);  // hz rows are window rows lo..hi-1
    out[((size_t)ch * Wo + (y0 + y)) * Wo + x] = ip_norm(v);
  }
}

// grid (bands, images).  A block stages its band of the (mirrored) window plus the halo in LDS with coalesced byte
// loads, writes level 0 from there, filters every staged row horizontally for both smaller levels into LDS (uint8, as
// PIL's intermediate image), then runs the vertical pass from LDS.
template <int L>
__global__ __launch_bounds__(256) void image_batch_kernel(const unsigned char* __restrict__ pool, long long pool_bytes,
                                                          const long long* __restrict__ offsets,
                                                          const int* __restrict__ sizes, int npool,
                                                          const int* __restrict__ plan, int S,
                                                          const int* __restrict__ tab1, const int* __restrict__ tab2,
                                                          float* __restrict__ out0, float* __restrict__ out1,
                                                          float* __restrict__ out2) {
  __shared__ __attribute__((aligned(16))) unsigned char src[IP_ROWS * IP_SMAX * 3];
  __shared__ unsigned char hz1[L >= 2 ? IP_ROWS * (IP_SMAX / 2) * 3 : 4];
  __shared__ unsigned char hz2[L >= 3 ? IP_ROWS * (IP_SMAX / 4) * 3 : 4];
  const int tid = threadIdx.x, img = blockIdx.y;
  const int pi = plan[img * 4 + 0], top = plan[img * 4 + 1], left = plan[img * 4 + 2], flip = plan[img * 4 + 3];
  if (pi < 0 || pi >= npool) return;             // every exit below is block-uniform and ahead of the barriers
  const long long off = offsets[pi];
  const int h = sizes[pi * 2], w = sizes[pi * 2 + 1];
  // a plan row whose window does not lie inside its image, or an image that does not lie inside the pool, is skipped:
  // its planes keep what they held.  plan_batch cannot produce one.
  if (h < S || w < S || top < 0 || left < 0 || top > h - S || left > w - S) return;
  if (off < 0 || off + (long long)h * w * 3 > pool_bytes) return;

  const int r0 = blockIdx.x * IP_BAND;
  const int nrows = min(IP_BAND, S - r0);
  const int lo = L >= 2 ? max(r0 - IP_HALO, 0) : r0;
  const int hi = L >= 2 ? min(r0 + nrows + IP_HALO, S) : r0 + nrows;
  const int nl = hi - lo, rb = S * 3;

  const unsigned char* base = pool + off + ((long long)(top + lo) * w + left) * 3;
  for (int r = 0; r < nl; ++r) {
    const unsigned char* g = base + (long long)r * w * 3;
    for (int j = tid; j < rb; j += 256) {
      const int c = j / 3, ch = j - c * 3;
      src[r * rb + (flip ? (S - 1 - c) * 3 + ch : j)] = g[j];
    }
  }
  __syncthreads();

  // level 0: four pixels (12 bytes) per thread -> one float4 per colour plane
  const int quads = S / 4;
  float* o0 = out0 + (size_t)img * 3 * S * S;
  for (int e = tid; e < nrows * quads; e += 256) {
    const int r = e / quads, q = e - r * quads;
    const unsigned* sp = reinterpret_cast<const unsigned*>(src + (r0 - lo + r) * rb + q * 12);
    const unsigned wd[3] = {sp[0], sp[1], sp[2]};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = k * 3 + ch;
        v[k] = ip_norm((int)((wd[b >> 2] >> ((b & 3) * 8)) & 255u));
      }
      *reinterpret_cast<f32x4*>(o0 + ((size_t)ch * S + r0 + r) * S + q * 4) = v;
    }
  }
  if (L == 1) return;

  ip_horizontal<IP_K1>(src, hz1, tab1, nl, S, S / 2, tid);
  if (L >= 3) ip_horizontal<IP_K2>(src, hz2, tab2, nl, S, S / 4, tid);
  __syncthreads();
  ip_vertical<IP_K1>(hz1, tab1, lo, hi, r0 / 2, nrows / 2, S / 2, out1 + (size_t)img * 3 * (S / 2) * (S / 2), tid);
  if (L >= 3)
    ip_vertical<IP_K2>(hz2, tab2, lo, hi, r0 / 4, nrows / 4, S / 4, out2 + (size_t)img * 3 * (S / 4) * (S / 4), tid);
}

}  // namespace

extern "C" int s2i_image_batch(const unsigned char* pool, long long pool_bytes, const long long* offsets,
                               const int* sizes, int npool, const int* plan, int n, int S, int L, const int* tab1,
                               const int* tab2, float* out0, float* out1, float* out2, void* stream) {
  S2I_REQUIRE(pool && offsets && sizes && plan && out0 && pool_bytes > 0 && npool > 0, "image_batch: bad args");
  S2I_REQUIRE(n > 0 && n <= 65535, "image_batch: n = %d outside 1..65535", n);
  S2I_REQUIRE(L >= 1 && L <= 3, "image_batch: %d levels, expected 1..3", L);
  S2I_REQUIRE(S >= 4 && S <= IP_SMAX && S % 4 == 0, "image_batch: size %d is not a multiple of 4 in 4..%d", S, IP_SMAX);
  S2I_REQUIRE(L < 2 || (tab1 && out1), "image_batch: level 1 needs its table and its output");
  S2I_REQUIRE(L < 3 || (tab2 && out2), "image_batch: level 2 needs its table and its output");
  S2I_REQUIRE(((size_t)out0 & 15) == 0, "image_batch: out0 is not 16-byte aligned");
  const dim3 grid(s2i_cdiv(S, IP_BAND), n), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (L == 1)
    hipLaunchKernelGGL(image_batch_kernel<1>, grid, block, 0, st, pool, pool_bytes, offsets, sizes, npool, plan, S, tab1,
                       tab2, out0, out1, out2);
  else if (L == 2)
    hipLaunchKernelGGL(image_batch_kernel<2>, grid, block, 0, st, pool, pool_bytes, offsets, sizes, npool, plan, S, tab1,
                       tab2, out0, out1, out2);
  else
    hipLaunchKernelGGL(image_batch_kernel<3>, grid, block, 0, st, pool, pool_bytes, offsets, sizes, npool, plan, S, tab1,
                       tab2, out0, out1, out2);
  S2I_LAUNCH_CHECK("image_batch");
  return 0;
}
