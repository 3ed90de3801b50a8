// Training kernels of the speech encoder's conv stack (Audio_to_Image/speech_encoder.py:26-52 under autograd, as
// train_audio_encoder.py:168-216 drives it), fp32, NHWC [B][1][W][C]:
//   - input gradient of a (1 x kw) temporal convolution: implicit GEMM on v_mfma_f32_32x32x2_f32, one launch phase per
//     parity of the output position for stride 2, so the structurally zero half of K is never multiplied;
//   - its weight gradient: the row reduction over B * Wo is split into slabs that a second kernel sums in a fixed order
//     (in double) straight into the OIHW parameter layout: no atomics, bit-identical from run to run;
//   - train-mode BatchNorm + ReLU: apply, and the reduce / apply passes of the backward with the ReLU decision read from
//     the stored forward output;
//   - MaxPool2d((1,3),(1,2),(0,1)) backward as a gather with the maximum recomputed from the stored input;
//   - the two finalize steps of the leading BatchNorm2d(1), whose tensor the per-channel kernels see as [n/4][4].
// Nothing here allocates or synchronises; no kernel uses scratch.
#include "s2i_igemm.h"
#include "s2i_elementwise.h"

namespace {

// ---- temporal-conv input gradient -----------------------------------------------------------------------------------
// dx[b, i, c] = sum_t sum_o dy[b, (i + pad - t) / s, o] * w[o, c, t] over the taps with (i + pad - t) % s == 0.
// Phase ph = (i + pad) % s owns the taps t = ph + s u, u = 0 .. nt - 1, and the rows i = s q + r, r = (ph - pad) mod s:
// for them j = jb - u with jb = (i + pad - ph) / s, a stride-1 gather of dy.  K = nt * Cout, Cout a multiple of 32, so
// a 32-deep chunk lies inside one tap.  The weight is the packed forward tensor P[t][c][o] (s2i_pack_conv_weight), read
// with k = o contiguous: both operands are staged "row x 4 consecutive k" and written transposed into LDS.
struct DgradP {
  const float* __restrict__ dy;
  const float* __restrict__ w;
  float* __restrict__ dx;
  int B, W, Wo, Cin, Cout, wR, ldw, kw, s, pad;
  int Wq, lgWq, Mq;  // input positions per phase and image (W / s), its log2, rows per phase (B * Wq)
  unsigned dy_bytes, w_bytes;
};

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256, 2) void conv1d_dgrad_kernel(DgradP p) {
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int LDA = BM + 1, LDB = BN + 1;
  constexpr int ASLOTS = BM / 32, BSLOTS = BN / 32;
  __shared__ float As[32 * LDA];
  __shared__ float Bs[32 * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, ph = blockIdx.z;
  const int kq = tid & 7, mrow = tid >> 3;
  const int r = (((ph - p.pad) % p.s) + p.s) % p.s;
  const int nt = (p.kw - ph + p.s - 1) / p.s;
  const int cpt = p.Cout / 32;          // chunks per tap
  const int nchunks = nt * cpt;

  const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, p.dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);

  int abase[ASLOTS], ajb[ASLOTS], wconst[BSLOTS];
#pragma unroll
  for (int i = 0; i < ASLOTS; ++i) {
    const int m = m0 + mrow + 32 * i;
    abase[i] = 0;
    ajb[i] = -(1 << 24);
    if (m < p.Mq) {
      const int b = m >> p.lgWq, q = m & (p.Wq - 1);
      const int jb = (q * p.s + r + p.pad - ph) / p.s;
      ajb[i] = jb;
      abase[i] = ((b * p.Wo + jb) * p.Cout + kq * 4) * 4;
    }
  }
#pragma unroll
  for (int j = 0; j < BSLOTS; ++j) {
    const int n = n0 + mrow + 32 * j;
    wconst[j] = n < p.Cin ? (n * p.ldw + kq * 4) * 4 : S2I_OOB;
  }

  f32x4 ra[ASLOTS], rb[BSLOTS];
  auto fetch = [&](int kc) {
    const int u = kc / cpt;
    const int o0 = (kc - u * cpt) * 32;
    const int t = ph + p.s * u;
    const int aoff = (o0 - u * p.Cout) * 4;
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i) {
      const int j = ajb[i] - u;
      ra[i] = bload4(rdy, (j >= 0 && j < p.Wo) ? abase[i] + aoff : S2I_OOB);
    }
    const int wbase = (t * p.wR * p.ldw + o0) * 4;
#pragma unroll
    for (int j = 0; j < BSLOTS; ++j) rb[j] = bload4(rw, wconst[j] == S2I_OOB ? S2I_OOB : wbase + wconst[j]);
  };

  // Two-level sum: K reaches 3 072 (512 -> 1024, k5 s2), and one fp32 chain of that length collects more rounding error
  // than a blocked product does; `part` is folded into `acc` every eight chunks (256 terms).
  f32x16 acc[TM][TN], part[TM][TN];
  zero_acc(acc);
  zero_acc(part);
  if (nchunks > 0) fetch(0);
  for (int kc = 0; kc < nchunks; ++kc) {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) As[(kq * 4 + j) * LDA + mrow + 32 * i] = ra[i][j];
#pragma unroll
    for (int i = 0; i < BSLOTS; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) Bs[(kq * 4 + j) * LDB + mrow + 32 * i] = rb[i][j];
    __syncthreads();
    if (kc + 1 < nchunks) fetch(kc + 1);
    mma_chunk<TM, TN, LDA, LDB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, part);
    if ((kc & 7) == 7 || kc + 1 == nchunks) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] += part[i][j];
#pragma unroll
          for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
        }
    }
    __syncthreads();
  }
  store_tile<TM, TN>(p.dx, p.Cin, p.Cin, true, nullptr, S2I_ACT_NONE, 0, acc, lane, wm, wn, n0, [&](int ml, long long& row) {
    const int m = m0 + ml;
    if (m >= p.Mq) return false;
    const int b = m >> p.lgWq, q = m & (p.Wq - 1);
    row = (long long)b * p.W + q * p.s + r;
    return true;
  });
}

// ---- temporal-conv weight gradient ----------------------------------------------------------------------------------
// slab[split][o][t][c] = sum over the split's rows m = (b, ox) of dy[m][o] * x[b, ox s - pad + t, c].  A block owns one tap
// and a BM x BN tile of (o, c); both operands are contiguous along the tile axis, so a 32-row chunk is staged with
// 16-byte loads and stores.  wgrad_sum_kernel adds the slabs in split order.
struct WgradP1 {
  const float* __restrict__ x;
  const float* __restrict__ dy;
  float* __restrict__ slab;
  int B, W, Wo, lgWo, Cin, Cout, kw, s, pad, M;
  int nchunks, cps, splits;
  unsigned x_bytes, dy_bytes;
};

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256, 2) void conv1d_wgrad_kernel(WgradP1 p) {
  constexpr int TM = BM / (WAVES_M * 32), TN = BN / (WAVES_N * 32);
  constexpr int LDA = BM, LDB = BN;
  constexpr int ASLOTS = BM / 32, BSLOTS = BN / 32;
  constexpr int AROWS = 1024 / BM, BROWS = 1024 / BN;   // rows of a chunk one pass of the block stages
  __shared__ __attribute__((aligned(16))) float As[32 * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[32 * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int t = blockIdx.y % p.kw, cn = blockIdx.y / p.kw;
  const int o0 = blockIdx.x * BM, c0 = cn * BN, split = blockIdx.z;
  const int acol = (tid % (BM / 4)) * 4, arow = tid / (BM / 4);
  const int bcol = (tid % (BN / 4)) * 4, brow = tid / (BN / 4);
  const bool a_ok = o0 + acol < p.Cout, b_ok = c0 + bcol < p.Cin;

  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, p.dy_bytes, 0x00020000);

  f32x4 ra[ASLOTS], rb[BSLOTS];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i) {
      const int m = kc * 32 + arow + i * AROWS;
      ra[i] = bload4(rdy, (a_ok && m < p.M) ? (m * p.Cout + o0 + acol) * 4 : S2I_OOB);
    }
#pragma unroll
    for (int i = 0; i < BSLOTS; ++i) {
      const int m = kc * 32 + brow + i * BROWS;
      const int b = m >> p.lgWo, ox = m & (p.Wo - 1);
      const int pos = ox * p.s - p.pad + t;
      rb[i] = bload4(rx, (b_ok && m < p.M && pos >= 0 && pos < p.W) ? ((b * p.W + pos) * p.Cin + c0 + bcol) * 4 : S2I_OOB);
    }
  };

  f32x16 acc[TM][TN];
  zero_acc(acc);
  const int c_begin = split * p.cps;
  const int c_end = min(p.nchunks, c_begin + p.cps);
  if (c_begin < c_end) fetch(c_begin);
  for (int kc = c_begin; kc < c_end; ++kc) {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i) *reinterpret_cast<f32x4*>(As + (arow + i * AROWS) * LDA + acol) = ra[i];
#pragma unroll
    for (int i = 0; i < BSLOTS; ++i) *reinterpret_cast<f32x4*>(Bs + (brow + i * BROWS) * LDB + bcol) = rb[i];
    __syncthreads();
    if (kc + 1 < c_end) fetch(kc + 1);
    mma_chunk<TM, TN, LDA, LDB>(As, Bs, wm * TM * 32, wn * TN * 32, lane, acc);
    __syncthreads();
  }
  const int ldo = p.kw * p.Cin;
  float* out = p.slab + (size_t)split * p.Cout * ldo + (size_t)t * p.Cin;
  store_tile<TM, TN>(out, ldo, p.Cin, true, nullptr, S2I_ACT_NONE, 0, acc, lane, wm, wn, c0, [&](int ml, long long& row) {
    if (o0 + ml >= p.Cout) return false;
    row = o0 + ml;
    return true;
  });
}

// dw[o][c][0][t] = sum over the splits, in order, of slab[split][o][t][c]
__global__ void conv1d_wgrad_sum_kernel(const float* __restrict__ slab, int splits, int O, int C, int kw,
                                        float* __restrict__ dw) {
  const long long total = (long long)O * kw * C;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const long long ot = e / C;
    const int t = (int)(ot % kw);
    const long long o = ot / kw;
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)slab[(size_t)k * total + e];
    dw[(o * C + c) * kw + t] = (float)s;
  }
}

struct WgradPlan1 {
  int Wo, M, tile, gridM, gridN, nchunks, cps, splits;
};

int plan_wgrad1(int B, int W, int Cin, int Cout, int kw, int s, int pad, WgradPlan1* pl) {
  S2I_REQUIRE(B > 0 && W > 0 && s2i_is_pow2(W) && Cin > 0 && Cout > 0 && Cin % 4 == 0 && Cout % 4 == 0,
              "conv1d wgrad: bad extent (B=%d W=%d Cin=%d Cout=%d)", B, W, Cin, Cout);
  S2I_REQUIRE(kw >= 1 && kw <= 31 && s >= 1 && pad >= 0, "conv1d wgrad: bad kw/stride/pad");
  pl->Wo = (W + 2 * pad - kw) / s + 1;
  S2I_REQUIRE(pl->Wo >= 1 && s2i_is_pow2(pl->Wo), "conv1d wgrad: output width %d is not a power of two", pl->Wo);
  const long long M = (long long)B * pl->Wo;
  S2I_REQUIRE(M * Cout * 4 < 0x7ff00000ll && (long long)B * W * Cin * 4 < 0x7ff00000ll,
              "conv1d wgrad: tensor exceeds the 2 GiB buffer-addressing window");
  pl->M = (int)M;
  pl->tile = (Cout > 64 && Cin > 64) ? 0 : (Cout > 64 ? 1 : 2);   // 128 x 128, 128 x 64, 64 x 64
  const int BM = pl->tile == 2 ? 64 : 128, BN = pl->tile == 0 ? 128 : 64;
  pl->gridM = s2i_cdiv(Cout, BM);
  pl->gridN = s2i_cdiv(Cin, BN) * kw;
  pl->nchunks = s2i_cdiv(M, 32);
  // Split the rows where the result has too few tiles to fill the chip (768 block slots), keeping at least four chunks
  // per split; and never let one block accumulate more than 512 rows in fp32 (the slabs are added in double).
  const long long tiles = (long long)pl->gridM * pl->gridN;
  int splits = (int)(768 / tiles);
  if (splits > pl->nchunks / 4) splits = pl->nchunks / 4;
  if (splits < s2i_cdiv(pl->nchunks, 16)) splits = s2i_cdiv(pl->nchunks, 16);
  if (splits < 1) splits = 1;
  pl->cps = s2i_cdiv(pl->nchunks, splits);
  pl->splits = s2i_cdiv(pl->nchunks, pl->cps);
  return 0;
}

// ---- train-mode BatchNorm + ReLU --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(const float* __restrict__ y, long long M, int C,
                                                          const float* __restrict__ coef, float* __restrict__ out) {
  const int Q = C / 4;
  const long long total = M * Q;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(e % Q);
    const f32x4 yv = ld4(y + e * 4), sc = ld4(coef + 2 * C + q * 4), sh = ld4(coef + 3 * C + q * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaxf(sc[j] * yv[j] + sh[j], 0.f);
    st4(out + e * 4, o);
  }
}

// part[0 | 1][blockIdx.x][c] = sums over the block's row chunk of dz and dz * xhat, dz = dout where out > 0
__global__ __launch_bounds__(256) void bn_relu_bwd_reduce_kernel(const float* __restrict__ y, const float* __restrict__ out,
                                                                 const float* __restrict__ dout, long long M, int C,
                                                                 const float* __restrict__ coef, float* __restrict__ part,
                                                                 int nparts, int cpb) {
  __shared__ f32x4 sh[2][256];
  const int tid = threadIdx.x;
  const int rpb = 256 / cpb;
  const int ql = tid % cpb, rl = tid / cpb;
  const int quad = blockIdx.y * cpb + ql;
  const int Q = C / 4;
  const long long chunk = (M + nparts - 1) / nparts;
  const long long r0 = blockIdx.x * chunk;
  const long long r1 = r0 + chunk < M ? r0 + chunk : M;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  if (quad < Q) {
    const f32x4 mean = ld4(coef + quad * 4), invstd = ld4(coef + C + quad * 4);
    for (long long row = r0 + rl; row < r1; row += rpb) {
      const long long off = row * C + quad * 4;
      const f32x4 yv = ld4(y + off), ov = ld4(out + off), dv = ld4(dout + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dz = ov[j] > 0.f ? dv[j] : 0.f;
        s0[j] += dz;
        s1[j] += dz * ((yv[j] - mean[j]) * invstd[j]);
      }
    }
  }
  sh[0][tid] = s0;
  sh[1][tid] = s1;
  __syncthreads();
  if (rl == 0 && quad < Q) {
    for (int r = 1; r < rpb; ++r) {
      s0 += sh[0][r * cpb + ql];
      s1 += sh[1][r * cpb + ql];
    }
    st4(part + ((size_t)0 * nparts + blockIdx.x) * C + quad * 4, s0);
    st4(part + ((size_t)1 * nparts + blockIdx.x) * C + quad * 4, s1);
  }
}

// dy = scale * (dz - mean_dz - xhat * mean_dz_xhat)
__global__ __launch_bounds__(256) void bn_relu_bwd_apply_kernel(const float* __restrict__ y, const float* __restrict__ out,
                                                                const float* __restrict__ dout, long long M, int C,
                                                                const float* __restrict__ coef, const float* __restrict__ red2,
                                                                float* __restrict__ dy) {
  const int Q = C / 4;
  const long long total = M * Q;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(e % Q);
    const f32x4 yv = ld4(y + e * 4), ov = ld4(out + e * 4), dv = ld4(dout + e * 4);
    const f32x4 mean = ld4(coef + q * 4), invstd = ld4(coef + C + q * 4), sc = ld4(coef + 2 * C + q * 4);
    const f32x4 m1 = ld4(red2 + q * 4), m2 = ld4(red2 + C + q * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dz = ov[j] > 0.f ? dv[j] : 0.f;
      const float xhat = (yv[j] - mean[j]) * invstd[j];
      o[j] = sc[j] * (dz - m1[j] - xhat * m2[j]);
    }
    st4(dy + e * 4, o);
  }
}

// ---- max-pool backward ------------------------------------------------------------------------------------------------
// window j covers positions 2j - 1, 2j, 2j + 1; its gradient goes to the first position that holds its maximum
__device__ __forceinline__ int pool_argmax(const float* __restrict__ row, int C, int W, int j, int lanec) {
  const int x0 = 2 * j - 1;
  int best = x0 >= 0 ? x0 : x0 + 1;
  float m = row[(long long)best * C + lanec];
  for (int pos = best + 1; pos <= x0 + 2 && pos < W; ++pos) {
    const float v = row[(long long)pos * C + lanec];
    if (v > m) { m = v; best = pos; }
  }
  return best;
}

__global__ void maxpool_w3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, int W, int C,
                                        long long total, float* __restrict__ dx) {
  const int Wo = W / 2;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const long long r = e / C;        // (b*H + h) * W + i
    const int i = (int)(r % W);
    const long long bh = r / W;
    const float* row = x + bh * W * C;
    const float* drow = dy + bh * Wo * C;
    float g = 0.f;
    const int j0 = i >> 1;            // even i: its centre window; odd i: the window to its left
    if (pool_argmax(row, C, W, j0, c) == i) g += drow[(long long)j0 * C + c];
    if ((i & 1) && j0 + 1 < Wo && pool_argmax(row, C, W, j0 + 1, c) == i) g += drow[(long long)(j0 + 1) * C + c];
    dx[e] = g;
  }
}

// ---- the leading BatchNorm2d(1) -----------------------------------------------------------------------------------------
// The per-channel kernels see its n elements as [n / 4][4]; these two fold the four columns of their partial sums into the
// one channel and write coefficient tables replicated four times, so the C = 4 apply kernels read them unchanged.
template <int MODE>  // 0: statistics -> coef4 [4][4], running statistics;  1: backward sums -> dgamma, dbeta, red2 [2][4]
__global__ __launch_bounds__(256) void bn1_finalize_kernel(const float* __restrict__ part, int nparts, double count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ rmean, float* __restrict__ rvar,
                                                           long long* __restrict__ nbt, float momentum, float eps,
                                                           float* __restrict__ out, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  __shared__ double sh[2][256];
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int i = tid; i < nparts * 4; i += 256) {
    a0 += (double)part[i];
    a1 += (double)part[(size_t)nparts * 4 + i];
  }
  sh[0][tid] = a0;
  sh[1][tid] = a1;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 256; ++k) { a0 += sh[0][k]; a1 += sh[1][k]; }
  if (MODE == 0) {
    const double mean = a0 / count;
    double var = a1 / count - mean * mean;
    if (var < 0) var = 0;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[0] * invstd;
    const float shf = beta[0] - (float)mean * sc;
    for (int j = 0; j < 4; ++j) {
      out[j] = (float)mean;
      out[4 + j] = invstd;
      out[8 + j] = sc;
      out[12 + j] = shf;
    }
    if (rmean) {
      const double unb = count > 1 ? var * count / (count - 1) : var;
      rmean[0] = (1.f - momentum) * rmean[0] + momentum * (float)mean;
      rvar[0] = (1.f - momentum) * rvar[0] + momentum * (float)unb;
    }
    if (nbt) nbt[0] += 1;
  } else {
    for (int j = 0; j < 4; ++j) {
      out[j] = (float)(a0 / count);
      out[4 + j] = (float)(a1 / count);
    }
    if (dbeta) dbeta[0] = (float)a0;
    if (dgamma) dgamma[0] = (float)a1;
  }
}

// Statistics of the one channel: part[0 | 1][block][0 .. 1] = the sum of x and of x * x over the block's quads, each held as
// a (high, low) pair of floats (columns 2 .. 3 zero) that bn1_finalize_kernel, which adds all four columns in double, puts
// together again.  Every term and every sum is double: the input is log-mel in dB (mean about -40, mean^2 / var 3 .. 5), so
// var = E[x^2] - mean^2 magnifies the relative error of E[x^2] that many times, and fp32 squares in fp32 chains
// (s2i_colstats on the [n / 4][4] view) left the running variance of an 80-element input 2.5e-7 off, outside its bound.
__global__ __launch_bounds__(256) void bn1_stats_kernel(const float* __restrict__ x, long long Q, float* __restrict__ part,
                                                        int nparts) {
  __shared__ double sh[2][256];
  const int tid = threadIdx.x;
  const long long chunk = (Q + nparts - 1) / nparts;
  const long long q0 = blockIdx.x * chunk;
  const long long q1 = q0 + chunk < Q ? q0 + chunk : Q;
  double a0 = 0.0, a1 = 0.0;
  for (long long q = q0 + tid; q < q1; q += 256) {
    const f32x4 xv = ld4(x + q * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double v = (double)xv[j];
      a0 += v;
      a1 += v * v;
    }
  }
  sh[0][tid] = a0;
  sh[1][tid] = a1;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 256; ++k) { a0 += sh[0][k]; a1 += sh[1][k]; }
  const float h0 = (float)a0, h1 = (float)a1;
  st4(part + ((size_t)0 * nparts + blockIdx.x) * 4, f32x4{h0, (float)(a0 - (double)h0), 0.f, 0.f});
  st4(part + ((size_t)1 * nparts + blockIdx.x) * 4, f32x4{h1, (float)(a1 - (double)h1), 0.f, 0.f});
}

// Backward sums of the one channel: part[0 | 1][block][0] = sum of dout and of dout * xhat over the block's quads (columns
// 1 .. 3 zero, so bn1_finalize_kernel reads the layout of the C = 4 kernels).  A thread adds four products in fp32 and
// carries its sum in double; the block's 256 sums are added in double, in thread order.  (The C = 4 walk of
// s2i_bn_act_bwd_reduce adds a block's rows in one fp32 chain, which the scalar BatchNorm's d weight, a sum over every
// input element, does not tolerate.)
__global__ __launch_bounds__(256) void bn1_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                             long long Q, const float* __restrict__ coef,
                                                             float* __restrict__ part, int nparts) {
  __shared__ double sh[2][256];
  const int tid = threadIdx.x;
  const long long chunk = (Q + nparts - 1) / nparts;
  const long long q0 = blockIdx.x * chunk;
  const long long q1 = q0 + chunk < Q ? q0 + chunk : Q;
  const float mean = coef[0], invstd = coef[4];
  double a0 = 0.0, a1 = 0.0;
  for (long long q = q0 + tid; q < q1; q += 256) {
    const f32x4 xv = ld4(x + q * 4), dv = ld4(dout + q * 4);
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s0 += dv[j];
      s1 += dv[j] * ((xv[j] - mean) * invstd);
    }
    a0 += (double)s0;
    a1 += (double)s1;
  }
  sh[0][tid] = a0;
  sh[1][tid] = a1;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 256; ++k) { a0 += sh[0][k]; a1 += sh[1][k]; }
  st4(part + ((size_t)0 * nparts + blockIdx.x) * 4, f32x4{(float)a0, 0.f, 0.f, 0.f});
  st4(part + ((size_t)1 * nparts + blockIdx.x) * 4, f32x4{(float)a1, 0.f, 0.f, 0.f});
}

}  // namespace

extern "C" int s2i_conv1d_dgrad(const float* dy, const float* w_packed, float* dx, int B, int W, int Cin, int Cout, int wR,
                                int ldw, int kw, int stride, int pad, void* stream) {
  S2I_REQUIRE(dy && w_packed && dx, "conv1d dgrad: null pointer");
  S2I_REQUIRE(B > 0 && W > 0 && s2i_is_pow2(W) && Cin > 0 && Cin % 4 == 0 && Cout > 0 && Cout % 32 == 0,
              "conv1d dgrad: bad extent (B=%d W=%d Cin=%d Cout=%d; Cout must be a multiple of 32)", B, W, Cin, Cout);
  S2I_REQUIRE(kw >= 1 && kw <= 31 && (stride == 1 || stride == 2) && pad >= 0 && kw >= stride && W % stride == 0,
              "conv1d dgrad: bad kw/stride/pad (%d, %d, %d)", kw, stride, pad);
  S2I_REQUIRE(wR >= Cin && ldw >= Cout && ldw % 4 == 0, "conv1d dgrad: packed weight %d x %d too small for %d x %d", wR, ldw,
              Cin, Cout);
  const int Wo = (W + 2 * pad - kw) / stride + 1;
  S2I_REQUIRE(Wo >= 1 && s2i_is_pow2(Wo), "conv1d dgrad: output width %d is not a power of two", Wo);
  const long long dyb = (long long)B * Wo * Cout * 4, wb = (long long)kw * wR * ldw * 4;
  S2I_REQUIRE(dyb < 0x7ff00000ll && wb < 0x7ff00000ll && (long long)B * W * Cin * 4 < 0x7ff00000ll,
              "conv1d dgrad: tensor exceeds the 2 GiB buffer-addressing window");
  DgradP p;
  p.dy = dy; p.w = w_packed; p.dx = dx;
  p.B = B; p.W = W; p.Wo = Wo; p.Cin = Cin; p.Cout = Cout; p.wR = wR; p.ldw = ldw; p.kw = kw; p.s = stride; p.pad = pad;
  p.Wq = W / stride; p.lgWq = s2i_ilog2(p.Wq); p.Mq = B * p.Wq;
  p.dy_bytes = (unsigned)dyb; p.w_bytes = (unsigned)wb;
  hipStream_t st = (hipStream_t)stream;
  if (Cin > 64) {
    dim3 grid(s2i_cdiv(p.Mq, 128), s2i_cdiv(Cin, 128), stride);
    hipLaunchKernelGGL((conv1d_dgrad_kernel<128, 128, 2, 2>), grid, dim3(256), 0, st, p);
  } else {
    dim3 grid(s2i_cdiv(p.Mq, 128), s2i_cdiv(Cin, 64), stride);
    hipLaunchKernelGGL((conv1d_dgrad_kernel<128, 64, 4, 1>), grid, dim3(256), 0, st, p);
  }
  S2I_LAUNCH_CHECK("conv1d_dgrad");
  return 0;
}

extern "C" size_t s2i_conv1d_wgrad_workspace_bytes(int B, int W, int Cin, int Cout, int kw, int stride, int pad) {
  WgradPlan1 pl;
  if (plan_wgrad1(B, W, Cin, Cout, kw, stride, pad, &pl)) return 0;
  return (size_t)pl.splits * Cout * kw * Cin * sizeof(float);
}

extern "C" int s2i_conv1d_wgrad(const float* x, const float* dy, float* dw_oihw, int B, int W, int Cin, int Cout, int kw,
                                int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE(x && dy && dw_oihw, "conv1d wgrad: null pointer");
  WgradPlan1 pl;
  if (plan_wgrad1(B, W, Cin, Cout, kw, stride, pad, &pl)) return 1;
  const size_t need = (size_t)pl.splits * Cout * kw * Cin * sizeof(float);
  S2I_REQUIRE(ws && ws_bytes >= need, "conv1d wgrad: workspace too small (%zu < %zu)", ws_bytes, need);
  WgradP1 p;
  p.x = x; p.dy = dy; p.slab = (float*)ws;
  p.B = B; p.W = W; p.Wo = pl.Wo; p.lgWo = s2i_ilog2(pl.Wo); p.Cin = Cin; p.Cout = Cout; p.kw = kw; p.s = stride; p.pad = pad;
  p.M = pl.M; p.nchunks = pl.nchunks; p.cps = pl.cps; p.splits = pl.splits;
  p.x_bytes = (unsigned)((long long)B * W * Cin * 4); p.dy_bytes = (unsigned)((long long)pl.M * Cout * 4);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(pl.gridM, pl.gridN, pl.splits);
  if (pl.tile == 0) hipLaunchKernelGGL((conv1d_wgrad_kernel<128, 128, 2, 2>), grid, dim3(256), 0, st, p);
  else if (pl.tile == 1) hipLaunchKernelGGL((conv1d_wgrad_kernel<128, 64, 4, 1>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((conv1d_wgrad_kernel<64, 64, 2, 2>), grid, dim3(256), 0, st, p);
  S2I_LAUNCH_CHECK("conv1d_wgrad");
  const long long total = (long long)Cout * kw * Cin;
  hipLaunchKernelGGL(conv1d_wgrad_sum_kernel, dim3(grid_for(total)), dim3(256), 0, st, (const float*)ws, pl.splits, Cout, Cin,
                     kw, dw_oihw);
  S2I_LAUNCH_CHECK("conv1d_wgrad_sum");
  return 0;
}

extern "C" int s2i_bn_relu_forward(const float* y, long long M, int C, const float* coef4, float* out, void* stream) {
  S2I_REQUIRE(y && coef4 && out && M > 0 && C > 0 && C % 4 == 0, "bn_relu_forward: bad args");
  hipLaunchKernelGGL(bn_relu_fwd_kernel, dim3(grid_for(M * (C / 4))), dim3(256), 0, ST, y, M, C, coef4, out);
  S2I_LAUNCH_CHECK("bn_relu_forward");
  return 0;
}

extern "C" int s2i_bn_relu_bwd_reduce(const float* y, const float* out, const float* dout, long long M, int C,
                                      const float* coef4, float* part, int nparts, void* stream) {
  S2I_REQUIRE(y && out && dout && coef4 && part && M > 0 && C > 0 && C % 4 == 0 && nparts > 0 && nparts <= M,
              "bn_relu_bwd_reduce: bad args");
  RedGeom g = red_geom(C);
  hipLaunchKernelGGL(bn_relu_bwd_reduce_kernel, dim3(nparts, g.gy), dim3(256), 0, ST, y, out, dout, M, C, coef4, part,
                     nparts, g.cpb);
  S2I_LAUNCH_CHECK("bn_relu_bwd_reduce");
  return 0;
}

extern "C" int s2i_bn_relu_bwd_apply(const float* y, const float* out, const float* dout, long long M, int C,
                                     const float* coef4, const float* red2, float* dy, void* stream) {
  S2I_REQUIRE(y && out && dout && coef4 && red2 && dy && M > 0 && C > 0 && C % 4 == 0, "bn_relu_bwd_apply: bad args");
  hipLaunchKernelGGL(bn_relu_bwd_apply_kernel, dim3(grid_for(M * (C / 4))), dim3(256), 0, ST, y, out, dout, M, C, coef4,
                     red2, dy);
  S2I_LAUNCH_CHECK("bn_relu_bwd_apply");
  return 0;
}

extern "C" int s2i_maxpool_w3s2_backward(const float* x, const float* dy, int B, int H, int W, int C, float* dx,
                                         void* stream) {
  S2I_REQUIRE(x && dy && dx && B > 0 && H > 0 && W >= 2 && W % 2 == 0 && C > 0, "maxpool_w3s2_backward: bad args");
  const long long total = (long long)B * H * W * C;
  hipLaunchKernelGGL(maxpool_w3s2_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, ST, x, dy, W, C, total, dx);
  S2I_LAUNCH_CHECK("maxpool_w3s2_backward");
  return 0;
}

extern "C" int s2i_bn1_stats(const float* x, long long n, float* part, int nparts, void* stream) {
  S2I_REQUIRE(x && part && n > 0 && n % 4 == 0 && nparts > 0, "bn1_stats: bad args");
  hipLaunchKernelGGL(bn1_stats_kernel, dim3(nparts), dim3(256), 0, ST, x, n / 4, part, nparts);
  S2I_LAUNCH_CHECK("bn1_stats");
  return 0;
}

extern "C" int s2i_bn1_finalize(const float* part, int nparts, long long count, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                                float eps, float* coef4x4, void* stream) {
  S2I_REQUIRE(part && nparts > 0 && count > 0 && gamma && beta && coef4x4, "bn1_finalize: bad args");
  S2I_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn1_finalize: running stats must come in pairs");
  hipLaunchKernelGGL((bn1_finalize_kernel<0>), dim3(1), dim3(256), 0, ST, part, nparts, (double)count, gamma, beta,
                     running_mean, running_var, num_batches_tracked, momentum, eps, coef4x4, (float*)nullptr,
                     (float*)nullptr);
  S2I_LAUNCH_CHECK("bn1_finalize");
  return 0;
}

extern "C" int s2i_bn1_bwd_finalize(const float* part, int nparts, long long count, float* dgamma, float* dbeta,
                                    float* red2x4, void* stream) {
  S2I_REQUIRE(part && nparts > 0 && count > 0 && red2x4, "bn1_bwd_finalize: bad args");
  hipLaunchKernelGGL((bn1_finalize_kernel<1>), dim3(1), dim3(256), 0, ST, part, nparts, (double)count, (const float*)nullptr,
                     (const float*)nullptr, (float*)nullptr, (float*)nullptr, (long long*)nullptr, 0.f, 0.f, red2x4, dgamma,
                     dbeta);
  S2I_LAUNCH_CHECK("bn1_bwd_finalize");
  return 0;
}

extern "C" int s2i_bn1_bwd_reduce(const float* x, const float* dout, long long n, const float* coef4x4, float* part,
                                  int nparts, void* stream) {
  S2I_REQUIRE(x && dout && coef4x4 && part && n > 0 && n % 4 == 0 && nparts > 0, "bn1_bwd_reduce: bad args");
  hipLaunchKernelGGL(bn1_bwd_reduce_kernel, dim3(nparts), dim3(256), 0, ST, x, dout, n / 4, coef4x4, part, nparts);
  S2I_LAUNCH_CHECK("bn1_bwd_reduce");
  return 0;
}
