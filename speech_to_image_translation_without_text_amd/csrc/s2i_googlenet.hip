// Memory-bound pieces of the BVLC GoogLeNet feature extractor (Audio_to_Image/prepare_image_feature.py:86-118, the
// deploy network up to pool5/7x7_s1): the 10-view input stage, the two LRN + max-pool pairs of the stem and the 3x3 max
// pools with Caffe's ceil rule.  The convolutions are s2i_conv2d_forward (s2i_conv2d.hip).  NHWC fp32 throughout.
#include "s2i_common.h"

namespace {

constexpr int kSrc = 227;    // Transformer input extent (prepare_image_feature.py:103)
constexpr int kView = 224;   // crop extent

constexpr int kMaxSide = 1 << 20;   // keeps (2 r + 1) n inside an int

// Source taps of resized coordinate r (0..226) on an axis of n pixels: src = (r + 0.5) n / 227 - 0.5, clamped to
// [0, n - 1].  The integer part is exact ((2r + 1) n - 227 over 454 in integers); the fraction is rounded once.
__device__ __forceinline__ void src_coord(int r, int n, int& i0, int& i1, float& l) {
  const int num = (2 * r + 1) * n - kSrc;
  if (num <= 0) {
    i0 = 0;
    l = 0.f;
  } else {
    i0 = num / (2 * kSrc);
    l = (float)(num - i0 * 2 * kSrc) * (1.f / (2 * kSrc));
  }
  if (i0 >= n - 1) {
    i0 = n - 1;
    l = 0.f;
  }
  i1 = min(i0 + 1, n - 1);
}

// one thread per output pixel of one view: grid (pixels / 256, 10 views, B images).  Bilinear resize of image b to
// 227 x 227 with half-pixel centres, sampled at the view's pixel, x255 is implicit (the source is 0..255), RGB -> BGR,
// minus the BGR mean, one 16-byte store (the 4th channel zero).
__global__ __launch_bounds__(256) void googlenet_prep_kernel(const unsigned char* __restrict__ img,
                                                             const long long* __restrict__ offsets,
                                                             const int* __restrict__ hs, const int* __restrict__ ws,
                                                             long long nbytes, float m0, float m1, float m2,
                                                             float* __restrict__ y) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= kView * kView) return;
  const int view = blockIdx.y, b = blockIdx.z;
  const int oy = pix / kView, ox = pix - oy * kView;
  const int k = view % 5;
  // crop origins (x0, y0): (0,0), (3,0), (1,1), (0,3), (3,3)
  const int cx = (k == 1 || k == 4) ? 3 : (k == 2 ? 1 : 0);
  const int cy = (k == 3 || k == 4) ? 3 : (k == 2 ? 1 : 0);
  int ry = cy + oy;
  if (view >= 5) ry = kSrc - 1 - ry;   // np.fliplr of a CHW array reverses the rows
  const int rx = cx + ox;
  f32x4 out;
  const long long off = offsets[b];
  const int H = hs[b], W = ws[b];
  if (off < 0 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || off + 3LL * H * W > nbytes) {
    out = f32x4{NAN, NAN, NAN, 0.f};   // an inconsistent descriptor shows up in the output, never as a stray read
  } else {
    int y0, y1, x0, x1;
    float ly, lx;
    src_coord(ry, H, y0, y1, ly);
    src_coord(rx, W, x0, x1, lx);
    const unsigned char* p = img + off;
    const unsigned char* p00 = p + ((size_t)y0 * W + x0) * 3;
    const unsigned char* p01 = p + ((size_t)y0 * W + x1) * 3;
    const unsigned char* p10 = p + ((size_t)y1 * W + x0) * 3;
    const unsigned char* p11 = p + ((size_t)y1 * W + x1) * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = (float)p00[c] + lx * ((float)p01[c] - (float)p00[c]);
      const float bot = (float)p10[c] + lx * ((float)p11[c] - (float)p10[c]);
      v[c] = top + ly * (bot - top);
    }
    out = f32x4{v[2] - m0, v[1] - m1, v[0] - m2, 0.f};
  }
  const size_t o = (((size_t)b * 10 + view) * (kView * kView) + pix) * 4;
  *reinterpret_cast<f32x4*>(y + o) = out;
}

enum { OP_POOL = 0, OP_POOL_LRN = 1, OP_LRN_POOL = 2 };

template <int V>
struct Vec;
template <>
struct Vec<4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  static __device__ __forceinline__ void store(float* p, const float* v) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  }
};
template <>
struct Vec<1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};

// The channel window of one pixel that the LRN of channels [c0, c0 + V) reads: channels [c0 - R, c0 + V + R), zero
// outside [0, C).  R = 4 covers local_size <= 9.  With V = 4 it is three 16-byte loads (C % 4 == 0 keeps a group whole).
constexpr int R = 4;
template <int V>
__device__ __forceinline__ void load_window(const float* px, int c0, int C, float* win) {
  if constexpr (V == 4) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int c = c0 - 4 + 4 * g;
      if (c >= 0 && c < C) {
        Vec<4>::load(px + c, win + 4 * g);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) win[4 * g + j] = 0.f;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V + 2 * R; ++j) {
      const int c = c0 - R + j;
      win[j] = (c >= 0 && c < C) ? px[c] : 0.f;
    }
  }
}

// y[j] = win[R + j] * (k + alpha / n * sum_{|d| <= n/2} win[R + j + d]^2) ^ -beta   (Caffe LRN ACROSS_CHANNELS)
template <int V>
__device__ __forceinline__ void lrn(const float* win, int half, float an, float beta, float kk, float* out) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float s = 0.f;
#pragma unroll
    for (int d = -R; d <= R; ++d) {
      const float t = win[R + j + d];
      if (d >= -half && d <= half) s = fmaf(t, t, s);
    }
    out[j] = win[R + j] * powf(fmaf(an, s, kk), -beta);
  }
}

// One thread per (output pixel, group of V channels).  Max over the 3 x 3 window at (oy*stride - pad, ox*stride - pad),
// taps outside the map skipped (Caffe's padded max pool; the ceil rule's last window is clipped the same way).
// OP_POOL_LRN: the LRN of the pooled pixel (the pooled window of every channel the LRN reads is recomputed in registers).
// OP_LRN_POOL: the max of the LRN of each tap (each tap's LRN recomputed for every window that reads it).
template <int V, int OP>
__global__ __launch_bounds__(256) void maxpool3_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                       int C, int ldx, int Ho, int Wo, int ldy, int coff, int stride,
                                                       int pad, int half, float an, float beta, float kk,
                                                       long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int G = C / V;
  const int g = (int)(idx % G);
  const long long pix = idx / G;
  const int ox = (int)(pix % Wo);
  const long long t = pix / Wo;
  const int oy = (int)(t % Ho);
  const int b = (int)(t / Ho);
  const int c0 = g * V;
  const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
  const float* xb = x + (size_t)b * H * W * ldx;
  float res[V];
  if constexpr (OP == OP_POOL_LRN) {
    constexpr int NW = V + 2 * R;
    float m[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) m[j] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = iy0 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ix0 + kx;
        if (ix < 0 || ix >= W) continue;
        float win[NW];
        load_window<V>(xb + ((size_t)iy * W + ix) * ldx, c0, C, win);
#pragma unroll
        for (int j = 0; j < NW; ++j) m[j] = fmaxf(m[j], win[j]);
      }
    }
    lrn<V>(m, half, an, beta, kk, res);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) res[j] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = iy0 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ix0 + kx;
        if (ix < 0 || ix >= W) continue;
        const float* px = xb + ((size_t)iy * W + ix) * ldx;
        float v[V];
        if constexpr (OP == OP_LRN_POOL) {
          float win[V + 2 * R];
          load_window<V>(px, c0, C, win);
          lrn<V>(win, half, an, beta, kk, v);
        } else {
          Vec<V>::load(px + c0, v);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) res[j] = fmaxf(res[j], v[j]);
      }
    }
  }
  Vec<V>::store(y + pix * ldy + coff + c0, res);
}

template <int OP>
void launch_maxpool3(bool vec, const float* x, float* y, int B, int H, int W, int C, int ldx, int Ho, int Wo, int ldy,
                     int coff, int stride, int pad, int half, float an, float beta, float kk, hipStream_t st) {
  const int V = vec ? 4 : 1;
  const long long total = (long long)B * Ho * Wo * (C / V);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec)
    hipLaunchKernelGGL((maxpool3_kernel<4, OP>), grid, dim3(256), 0, st, x, y, H, W, C, ldx, Ho, Wo, ldy, coff, stride,
                       pad, half, an, beta, kk, total);
  else
    hipLaunchKernelGGL((maxpool3_kernel<1, OP>), grid, dim3(256), 0, st, x, y, H, W, C, ldx, Ho, Wo, ldy, coff, stride,
                       pad, half, an, beta, kk, total);
}

// F.max_pool2d(kernel_size=3, stride, padding=pad, ceil_mode=True) output extent, with the rule that the last window
// starts inside the input or its left padding
int ceil_extent(int n, int stride, int pad) {
  int o = (n + 2 * pad - 3 + stride - 1) / stride + 1;
  if (pad > 0 && (o - 1) * stride >= n + pad) --o;
  return o;
}

int maxpool3_common(int op, const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy, int coff, int stride,
                    int pad, int size, float alpha, float beta, float k, void* stream, const char* what) {
  S2I_REQUIRE(x && y, "%s: null pointer", what);
  S2I_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && ldx >= C && coff >= 0 && ldy >= coff + C,
              "%s: bad shape (B %d, H %d, W %d, C %d, ldx %d, ldy %d, coff %d)", what, B, H, W, C, ldx, ldy, coff);
  S2I_REQUIRE((stride == 1 || stride == 2) && (pad == 0 || pad == 1), "%s: stride %d / pad %d outside {1, 2} / {0, 1}",
              what, stride, pad);
  S2I_REQUIRE(H + 2 * pad >= 3 && W + 2 * pad >= 3, "%s: a 3x3 window needs H, W >= %d", what, 3 - 2 * pad);
  if (op != OP_POOL) {
    S2I_REQUIRE(size >= 1 && size <= 2 * R + 1 && size % 2 == 1, "%s: local_size %d must be odd and <= %d", what, size,
                2 * R + 1);
    S2I_REQUIRE(beta >= 0.f && k > 0.f && alpha >= 0.f, "%s: LRN needs alpha >= 0, beta >= 0, k > 0", what);
  }
  const int Ho = ceil_extent(H, stride, pad), Wo = ceil_extent(W, stride, pad);
  S2I_REQUIRE((long long)B * Ho * Wo * C < (1LL << 40), "%s: output too large for one launch", what);
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && coff % 4 == 0 && ((uintptr_t)x & 15) == 0 &&
                   ((uintptr_t)y & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const int half = size / 2;
  const float an = size >= 1 ? alpha / (float)size : 0.f;
  if (op == OP_POOL)
    launch_maxpool3<OP_POOL>(vec, x, y, B, H, W, C, ldx, Ho, Wo, ldy, coff, stride, pad, 0, 0.f, 0.f, 1.f, st);
  else if (op == OP_POOL_LRN)
    launch_maxpool3<OP_POOL_LRN>(vec, x, y, B, H, W, C, ldx, Ho, Wo, ldy, coff, stride, pad, half, an, beta, k, st);
  else
    launch_maxpool3<OP_LRN_POOL>(vec, x, y, B, H, W, C, ldx, Ho, Wo, ldy, coff, stride, pad, half, an, beta, k, st);
  S2I_LAUNCH_CHECK(what);
  return 0;
}

}  // namespace

extern "C" int s2i_googlenet_prep(const unsigned char* img, long long nbytes, const long long* offsets, const int* hs,
                                  const int* ws, int B, float mean_b, float mean_g, float mean_r, float* y,
                                  void* stream) {
  S2I_REQUIRE(img && offsets && hs && ws && y, "googlenet_prep: null pointer");
  S2I_REQUIRE(B >= 1 && B <= 65535 && nbytes >= 3, "googlenet_prep: bad batch (B %d, %lld bytes)", B, nbytes);
  S2I_REQUIRE(((uintptr_t)y & 15) == 0, "googlenet_prep: the output must be 16-byte aligned");
  const dim3 grid(s2i_cdiv(kView * kView, 256), 10, B);
  hipLaunchKernelGGL(googlenet_prep_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, offsets, hs, ws, nbytes,
                     mean_b, mean_g, mean_r, y);
  S2I_LAUNCH_CHECK("googlenet_prep");
  return 0;
}

extern "C" int s2i_maxpool3(const float* x, int B, int H, int W, int C, int ldx, int stride, int pad, float* y, int ldy,
                            int coff, void* stream) {
  return maxpool3_common(OP_POOL, x, B, H, W, C, ldx, y, ldy, coff, stride, pad, 0, 0.f, 0.f, 1.f, stream, "maxpool3");
}

extern "C" int s2i_lrn_maxpool3(int order, const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy,
                                int coff, int size, float alpha, float beta, float k, void* stream) {
  S2I_REQUIRE(order == S2I_POOL_THEN_LRN || order == S2I_LRN_THEN_POOL, "lrn_maxpool3: unknown order %d", order);
  return maxpool3_common(order == S2I_POOL_THEN_LRN ? OP_POOL_LRN : OP_LRN_POOL, x, B, H, W, C, ldx, y, ldy, coff, 2, 0,
                         size, alpha, beta, k, stream, "lrn_maxpool3");
}
