/*
 * s2i_hip.h — C-ABI of the MI355X (gfx950) kernels under the StackGAN-v2 G/D train step.
 *
 * The reference (smallflyingpig/speech-to-image-translation-without-text) has no FFI of its own:
 * its hot path is stock torch.nn modules (StackGAN_v2/model.py:112-551) driven by
 * StackGAN_v2/trainer.py:375-489.  Each entry point below replaces one group of torch ops on that
 * path; the reference site it stands in for is cited next to it.  The Python host
 * (speech_to_image_translation_without_text_amd/ops.py) binds these with ctypes.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer, borrowed for the stream-ordered duration of the call;
 *   - nothing here allocates, frees or synchronises; scratch comes in through (ws, ws_bytes);
 *   - every call returns 0 on success; on failure a non-zero code, and s2i_last_error() holds text;
 *   - `stream` is a hipStream_t passed as void*;
 *   - activations are NHWC fp32, channel counts multiples of 4, spatial extents powers of two;
 *   - conv weights are consumed in the packed layout P[tap][Cin][Coutp] (Coutp = Cout rounded up
 *     to 4) written by s2i_pack_conv_weight from the reference's OIHW parameter tensors.
 */
#ifndef S2I_HIP_H
#define S2I_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2I_ABI_VERSION 7

/* conv geometry kinds */
#define S2I_CONV_K1      0  /* 1x1 / nn.Linear (model.py:179, 217)                              */
#define S2I_CONV_K3S1    1  /* conv3x3 pad 1 (model.py:125-128)                                 */
#define S2I_CONV_K4S2    2  /* Conv2d(k4,s2,p1) (model.py:371, 383-394); also dgrad of upBlock  */
#define S2I_TCONV_K4S2   3  /* 4-phase transposed conv k4 s2 p1: nearest x2 + conv3x3 collapsed
                               (model.py:133-140) and dgrad of Conv2d(k4,s2,p1)                 */

#define S2I_CONV_1D      4  /* (1 x kw) conv along W with stride / padding from the descriptor: the temporal
                               convolutions of the speech encoder (Audio_to_Image/speech_encoder.py:26-37);
                               forward only here: the gradients are s2i_conv1d_dgrad / s2i_conv1d_wgrad */

/* activations */
#define S2I_ACT_NONE     0
#define S2I_ACT_GLU      1  /* model.py:112-122 */
#define S2I_ACT_LRELU    2  /* nn.LeakyReLU(0.2), model.py:363, 373 */
#define S2I_ACT_TANH     3  /* model.py:293 */
#define S2I_ACT_RELU     4  /* speech_encoder.py:12 */

/* element types of activation tensors (bf16 activation mode, BASELINE config 4) */
#define S2I_DT_F32       0
#define S2I_DT_BF16      1

/* weight pack modes */
#define S2I_PACK_PLAIN   0  /* P[t][i][o] = W[o][i][t]                                          */
#define S2I_PACK_UPFOLD  1  /* 3x3 -> effective 4x4 taps of nearest-x2 + conv3x3               */

const char* s2i_last_error(void);
int  s2i_version(void);
/* Integer tuning knobs of the launch planners (tools and tests; every knob has a measured default; a negative value
   restores it, and s2i_get_tuning reports -1 for a knob at its default).  Returns 0, or non-zero for an unknown key.  The library reads no environment variable on a launch path: the ONE variable
   S2I_TUNE="key=value,key=value" is parsed once, when the library is loaded. */
int  s2i_set_tuning(const char* key, int value);
int  s2i_get_tuning(const char* key, int* value);
/* 0 when the current device is gfx950, non-zero (and last_error set) otherwise */
int  s2i_check_device(void);

/* ---- implicit-GEMM convolution (fp32 MFMA v_mfma_f32_32x32x2_f32) ------------------------- */
typedef struct s2i_conv_desc {
  int kind;      /* S2I_CONV_* / S2I_TCONV_K4S2                                                  */
  int B, H, W;   /* batch and spatial extent of the GATHERED tensor x                           */
  int Cx;        /* channels stored in x                                                        */
  int Cc;        /* channels of a per-image vector broadcast over space and concatenated FIRST
                    (torch.cat((c_code, h_code), 1), model.py:277, 434); 0 = none               */
  int N;         /* output channels                                                             */
  int wmode;     /* 0: weights used as P[t][k][n];  1: transposed per tap, P[t][n][k] (dgrad)    */
  int flip;      /* 1: tap t reads P[T-1-t] (dgrad of a stride-1 3x3)                            */
  int wR;        /* rows per tap in P                                                           */
  int ldw;       /* row stride of P (= Coutp of the forward layer)                              */
  int act;       /* epilogue: S2I_ACT_NONE / LRELU / TANH                                        */
  int stats;     /* 1: also emit per-row-tile column sums and sums of squares (BatchNorm)       */
  int ldy;       /* row stride of y                                                             */
  int groups;    /* BatchNorm groups: the rows are `groups` equal, independent batches stacked along
                    the batch axis (real / wrong / fake passes of trainer.py:390-392 in one launch);
                    statistics are kept per group.  0 or 1 = one batch                           */
  int nosplit;   /* 1: never split K (required with a class bias, s2i_conv_forward_cls)           */
  int kw, stride, pad; /* S2I_CONV_1D geometry (ignored by the other kinds)                       */
  int tile_rows; /* output rows per block of the fp32 matrix kernel: 0 = the planner chooses (96 or 128, whichever
                    fills whole rounds of the chip's block slots); 96 or 128 forces it (96 only where N > 64)     */
  int in_act;    /* s2i_conv_forward_in only: activation of the PRODUCING block applied to x while it is gathered
                    (S2I_ACT_LRELU); 0 elsewhere                                                              */
  int in_groups; /* ... and the number of BatchNorm groups of its coefficient table (0 or 1 = one)               */
} s2i_conv_desc;

/* scratch bytes the s2i_conv_forward* entry points need for this descriptor, whatever dtypes, bias or weight planes the
   call passes (split-K slabs, or the weight table / fragment buffer of a thin-layer kernel; 0: none).  The kernel a launch
   takes follows from the descriptor and the operands alone, never from the workspace: a call that passes less than its
   plan needs (s2i_conv_plan_query says how much, never more than this) returns non-zero with the error text set and
   launches nothing. */
size_t s2i_conv_workspace_bytes(const s2i_conv_desc* d);
/* number of partial rows the stats epilogue writes: part is [2][nparts][N] floats */
int    s2i_conv_stat_parts(const s2i_conv_desc* d);
/*
 * y[row][n] = act( sum_{t,c} X(row,t,c) * Wt[t][c][n] + bias[n] )
 * X gathers x (and cvec) per `kind`; rows enumerate (b,oy,ox) of the output grid.
 * Replaces F.conv2d / F.linear forward and their input-gradient on the reference path.
 */
int s2i_conv_forward(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                     const float* bias, float* y, float* part, void* ws, size_t ws_bytes,
                     void* stream);

/* Same, plus `cls_bias` [B][9][N]: a per-image, per-border-class term added before the statistics
   (the pre-reduced contribution of the broadcast c_code channels, see s2i_cvec_bias_table). */
int s2i_conv_forward_cls(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                         const float* bias, const float* cls_bias, float* y, float* part, void* ws,
                         size_t ws_bytes, void* stream);

/* Apply-on-load ("BatchNorm + LeakyReLU fused into the consuming convolution", model.py:369-376 followed by :371 / :360
   of the next block): x_raw is the RAW output y of the producing convolution and in_coef its (in_groups, 4, Cx)
   coefficient table [mean, invstd, scale, shift] (s2i_bn_finalize); the gather computes
   LeakyReLU(scale * y + shift) while it stages the operand, padding taps staying zero, so the producer's activated tensor
   is never written or read.  fp32, forward weight layout (wmode 0), 32 | Cx, no broadcast vector, kinds K1 / K3S1 / K4S2;
   with in_groups > 1 the rows of one producer group must be whole row tiles (as for `groups`). */
int s2i_conv_forward_in(const s2i_conv_desc* d, const float* x_raw, const float* in_coef, const float* w, float* y,
                        float* part, void* ws, size_t ws_bytes, void* stream);
/* What a forward convolution of this descriptor launches (host only; tools and the plan tests).  The operands are those of
   the entry point that would run it: x_dtype / y_dtype as for s2i_conv_forward_dt, planes as for s2i_conv_forward_split
   (0 = fp32 weights), whether a bias / class-bias table is passed, and d->in_act != 0 for s2i_conv_forward_in.
   out = { kernel id (FwdKernel of csrc/s2i_igemm.h), output rows and columns per block, threads per block, grid x / y / z of
   the main launch, K splits, 32-deep K chunks per split, K chunks, elements a table / fragment preparation launch writes
   first (0 = none), reduction after a split (0 none, 1 sum, 2 sum then column statistics, 3 sum fused with the statistics),
   workspace bytes the launch asks for, M, K }.  Non-zero, with out zeroed, where the plan refuses the layer in this mode. */
int s2i_conv_plan_query(const s2i_conv_desc* d, int x_dtype, int y_dtype, int planes, int has_bias, int has_cls_bias,
                        int out[15]);

/* ---- spatially constant channels of a 3x3 conv (c_code broadcast, model.py:272-279) -----------
 * A channel that is constant over space contributes sum over the IN-BOUNDS taps of c*W: a bias that
 * depends only on the image and on which borders the pixel touches (9 classes).  Forward: table
 * [B][9][N] from c (B,Cc) and the packed weight rows [0,Cc).  Backward: border sums of dY give, per
 * tap, the sum of dY over the pixels where the tap is in bounds; from them dc and dW[:, :Cc]. */
int s2i_cvec_bias_table(const float* cvec, const float* packed, int B, int Cc, int Ip, int Op, int N,
                        float* table, void* ws /* >= B*9*N floats */, size_t ws_bytes, void* stream);
size_t s2i_border_sums_workspace_bytes(int B, int H, int W, int C);
/* tapsum[b][t][c] = sum of dy[b,y,x,c] over pixels where tap t (3x3, pad 1) is in bounds */
int s2i_tap_sums(const float* dy, int B, int H, int W, int C, float* tapsum, void* ws, size_t ws_bytes,
                 void* stream);
/* dc[b][cc] = sum_{t,co} P[t][cc][co]*tapsum[b][t][co];  dW[co][cc][t] (+)= sum_b c[b][cc]*tapsum[b][t][co]
   (dW is the OIHW gradient of a parameter with I_total input channels, channels [0,Cc) written) */
int s2i_cvec_grads(const float* cvec, const float* packed, const float* tapsum, int B, int Cc, int Ip,
                   int Op, int N, int O, int I_total, float* dc, float* dw_oihw, int accumulate,
                   void* stream);

/* ---- weight gradient ------------------------------------------------------------------------ */
typedef struct s2i_wgrad_desc {
  int kind;      /* geometry of the gather applied to `a`                                        */
  int B, H, W;   /* extent of the gathered tensor a                                             */
  int Ca;        /* channels stored in a                                                        */
  int Cc;        /* broadcast-vector channels concatenated first (0 = none)                     */
  int N;         /* channels of the plain (un-gathered) operand g                               */
  int ldg;       /* row stride of g                                                             */
  int swap;      /* 0: result rows (tap,cin) x cols cout;  1: rows (tap,cout) x cols cin        */
  int fold;      /* 1: fold effective 4x4 taps back onto the 3x3 parameter (S2I_PACK_UPFOLD)    */
  int O, I, KH, KW; /* shape of the OIHW gradient tensor written                                */
  int accumulate;   /* 1: grad += result, 0: grad = result                                      */
  int i_off;        /* the I input channels computed here are channels [i_off, i_off+I) of a       */
  int I_total;      /* parameter with I_total input channels (0 = I): the c_code / h_code split    */
  int a_act;        /* s2i_conv_wgrad_in only: activation of the block that produced `a` (S2I_ACT_LRELU)    */
  int a_groups;     /* ... and the BatchNorm groups of its coefficient table (0 or 1 = one; at most 3)      */
} s2i_wgrad_desc;

size_t s2i_wgrad_workspace_bytes(const s2i_wgrad_desc* d);
/*
 * grad_oihw (+)= sum_rows A(row,t,c) * g[row][n]   — the weight-gradient of F.conv2d / F.linear
 * (autograd of model.py:125-128, 179, 217, 371, 383-394), written straight into the reference's
 * OIHW parameter layout.
 */
int s2i_conv_wgrad(const s2i_wgrad_desc* d, const float* a, const float* cvec, const float* g,
                   float* grad_oihw, void* ws, size_t ws_bytes, void* stream);

/* The weight gradient of the same consumer: the gathered operand is the producer's RAW output a_raw with its coefficient
   table, activated while it is staged (s2i_conv_forward_in).  Only where s2i_conv_wgrad_in_eligible(d) says so (the
   generic fp32 128 x 128 plan: every layer of the discriminator towers); otherwise the caller materialises the operand. */
int s2i_conv_wgrad_in_eligible(const s2i_wgrad_desc* d);
int s2i_conv_wgrad_in(const s2i_wgrad_desc* d, const float* a_raw, const float* a_coef, const float* g,
                      float* grad_oihw, void* ws, size_t ws_bytes, void* stream);


/* ---- split-bf16 matrix products (1 / 2 / 3 bf16 planes; opt-in) ---------------------
 * Same convolution as s2i_conv_forward_cls, with every fp32 operand written as a sum of `planes` bf16 numbers and the
 * products taken by v_mfma_f32_32x32x16_bf16 with fp32 accumulation (planes = 2: 3 products, ~2^-16 relative;
 * planes = 3: 6 products, ~2^-23).  wsplit holds the weights pre-split as [plane][tap][np][kp] bf16, n = output column of the
 * GEMM, k = its reduction index (s2i_split_packed_weight: out_cr for the forward, out_rc for the input gradient that
 * the fp32 path expresses with wmode = 1).  Eligible when the gathered channel count (and Cc) are multiples of 32. */
int s2i_conv_split_eligible(const s2i_conv_desc* d);
int s2i_conv_forward_split(const s2i_conv_desc* d, const float* x, const float* cvec,
                           const unsigned short* wsplit, int planes, int np, int kp, const float* bias,
                           const float* cls_bias, float* y, float* part, void* ws, size_t ws_bytes,
                           void* stream);
/* weight gradient with split-bf16 products (both operands are split while they are staged) */
size_t s2i_wgrad_workspace_bytes_split(const s2i_wgrad_desc* d, int planes);
int s2i_conv_wgrad_split(const s2i_wgrad_desc* d, int planes, const float* a, const float* cvec,
                         const float* g, float* grad_oihw, void* ws, size_t ws_bytes, void* stream);
/* packed fp32 weights P[T][R][C] (s2i_pack_conv_weight) -> bf16 planes, both operand layouts from one read:
   out_rc [plane][T][R][C] (input gradient) and out_cr [plane][T][C][R] (forward); either may be NULL */
int s2i_split_packed_weight(const float* packed, int T, int R, int C, int planes, unsigned short* out_rc,
                            unsigned short* out_cr, void* stream);


/* ---- bf16 activation mode (BASELINE config 4: bf16 activations / weights in HBM, bf16 MFMA, fp32 accumulate) -------
 * Activations between the fused blocks are bf16 NHWC; BatchNorm statistics come from the fp32 accumulators; master
 * weights, gradients, Adam and EMA stay fp32 (trainer.py:236-252).  The same convolutions as above
 * (model.py:125-140, 358-398 and their gradients) for layers whose channel count is a multiple of 32:
 *   - the block stages a 2-D input patch with its halo in LDS once per channel chunk and all taps read from it;
 *   - weights arrive pre-arranged by s2i_pack_conv_weight_bf16 as Wb[phase][chunk][tap][Npad][CK] bf16, from the packed
 *     fp32 copy P[t][R][C]: d->wmode = 0 uses P[t][k][n] (forward), 1 uses P[t][n][k] (input gradient), d->flip /
 *     the transposed-conv parity select the source tap; P may point at a row offset inside a tap (channel split).
 * d->Cc must be 0 (a broadcast vector is concatenated by the caller), d->act NONE, N and ldy multiples of 8. */
/* What s2i_conv_forward_bf16 launches for this descriptor, and everything a caller sizes by it (host only; one planning pass).
   out = { kernel id (B16Kernel of csrc/s2i_bf16.h; -1: planned, but the kernel is not instantiated for this tile, i.e. the
   layer is not eligible and the caller takes s2i_conv_forward_dt), output pixels per tile (128 or 256), output channels per
   block BN, input channels per LDS stage CK, threads per block, grid x (the block slots of the persistent form where it is
   taken) / y / z, tile width / rows / images, tiles, K splits, channel chunks per split, channel chunks, partial rows of the
   statistics (part is [2][rows][N] floats), Npad, elements of the packed bf16 weights, dynamic LDS bytes, workspace bytes
   (split-K slabs; 0: none), rows of y }.  The arrangement of the packed weights is identified by CK | Npad << 8: the same
   layer at another batch or map size may be planned onto another kernel, so a cache of packed bf16 weights is keyed by it.
   Non-zero, with out zeroed and the error text set, where the plan refuses the descriptor. */
int s2i_conv_bf16_plan_query(const s2i_conv_desc* d, long long out[21]);
int s2i_pack_conv_weight_bf16(const s2i_conv_desc* d, const float* packed, int R, int C, unsigned short* out,
                              void* stream);
/* The bf16 copies of a whole network in one launch (after the fused Adam step).  s2i_pack16_item_fill (host only, no
 * launch) fills the item of one (descriptor, packed fp32 source, destination) exactly as s2i_pack_conv_weight_bf16 would
 * pack it and returns its block count (-1 on error); the caller assigns block0 = running sum of the counts and uploads the
 * array. */
typedef struct s2i_pack16_item {
  const float* P;        /* packed fp32 source (P[t][R][C], possibly offset to a row inside a tap) */
  unsigned short* out;   /* Wb[phase][chunk][tap][Npad][CK] */
  int R, C, kind, flip, transpose, T, nphase, Nn, Npad, Kk, CK, gx, gy, block0;
} s2i_pack16_item;
int s2i_pack16_item_fill(const s2i_conv_desc* d, const float* packed, int R, int C, unsigned short* out,
                         s2i_pack16_item* item);
int s2i_pack_conv_weights_bf16_batched(const s2i_pack16_item* items_dev, int n, int total_blocks, void* stream);
int s2i_conv_forward_bf16(const s2i_conv_desc* d, const unsigned short* x, const unsigned short* w,
                          const float* cls_bias, unsigned short* y, float* part, void* ws, size_t ws_bytes,
                          void* stream);
/* The fp32-MFMA convolution / weight gradient of s2i_conv_forward_cls / s2i_conv_wgrad with x / y (a / g) stored as
   S2I_DT_F32 or S2I_DT_BF16: the edges of the bf16 mode (image tensors, channel counts that are not multiples of 32).
   Two bf16 operands of a weight gradient run on the bf16 matrix cores. */
int s2i_conv_forward_dt(const s2i_conv_desc* d, const void* x, int x_dtype, const float* cvec, const float* w,
                        const float* bias, const float* cls_bias, void* y, int y_dtype, float* part, void* ws,
                        size_t ws_bytes, void* stream);
size_t s2i_wgrad_workspace_bytes_dt(const s2i_wgrad_desc* d, int a_dtype, int g_dtype);
/* What a weight gradient of this descriptor launches (host only; tools and the plan tests).  The operands are those of the
   entry point that would run it: a_dtype / g_dtype as for s2i_conv_wgrad_dt, planes as for s2i_conv_wgrad_split (0 = none),
   in_act != 0 for s2i_conv_wgrad_in.  out = { kernel id (WgKernel of csrc/s2i_igemm.h), K rows and N columns of the result per
   block, threads per block, grid x / y / z, pixels per stage of the reduction loop, slabs the launch writes, slabs the workspace
   holds (what the s2i_wgrad_workspace_bytes* queries size, never fewer), K, M }.  Non-zero, with out zeroed, where the plan
   refuses the layer in this mode. */
int s2i_wgrad_plan_query(const s2i_wgrad_desc* d, int a_dtype, int g_dtype, int planes, int in_act, int out[12]);
int s2i_conv_wgrad_dt(const s2i_wgrad_desc* d, const void* a, int a_dtype, const float* cvec, const void* g,
                      int g_dtype, float* grad_oihw, void* ws, size_t ws_bytes, void* stream);
/* `_dt` forms of the BatchNorm / activation / layout kernels below: every activation tensor of the call has `dtype`; they
   accept the same activations as the fp32 forms and refuse the others the same way */
int s2i_bn_act_forward_dt(int dtype, const void* y, long long M, int groups, int C, const float* coef4, int act,
                          const void* residual, void* out, void* stream);
int s2i_bn_act_bwd_reduce_dt(int dtype, const void* y, const void* dout, int lddout, long long M, int groups, int C,
                             const float* coef4, int act, float* part, int nparts, void* stream);
int s2i_bn_act_bwd_apply_dt(int dtype, const void* y, const void* dout, int lddout, long long M, int groups, int C,
                            const float* coef4, const float* red2, int act, void* dy, void* stream);
int s2i_act_backward_dt(int dtype, const void* out, const void* dout, int lddout, long long M, int C, int act,
                        void* dy, void* stream);
int s2i_nchw_to_nhwc_dt(int dtype, const float* src, void* dst, int B, int C, int H, int W, int Cp, void* stream);
int s2i_nhwc_to_nchw_dt(int dtype, const void* src, int lds, float* dst, int B, int C, int H, int W, void* stream);
int s2i_spatial_sum_dt(int dtype, const void* src, int ld, int B, int HW, int C, float* dst, void* ws,
                       size_t ws_bytes, void* stream);
int s2i_tap_sums_dt(int dtype, const void* dy, int B, int H, int W, int C, float* tapsum, void* ws, size_t ws_bytes,
                    void* stream);
/* dst[n] = (dst_dtype) src[n] for a contiguous tensor, n % 4 == 0 */
int s2i_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long long n, void* stream);

/* OIHW parameter -> packed P[t][Ip][Op] (Ip >= I, Op = O rounded up to 4; padding zero filled) */
int s2i_pack_conv_weight(const float* w_oihw, float* packed, int O, int I, int KH, int KW,
                         int Ip, int mode, void* stream);
/* The same for a whole network in one launch: `items` is a DEVICE array; item k owns the linear blocks
   [block0, block0 + gx * ceil(Ip / 8)) with gx = ceil(Op / 32), block0 ascending; total_blocks = their sum;
   max_taps = the largest KH*KW.  Used after the fused Adam step (trainer.py:236-252 equivalent). */
typedef struct s2i_pack_item {
  const float* w;   /* OIHW parameter */
  float* packed;    /* P[t][Ip][Op]   */
  int O, I, KH, KW, Ip, mode, gx, block0;
} s2i_pack_item;
int s2i_pack_conv_weights_batched(const s2i_pack_item* items_dev, int n, int total_blocks, int max_taps,
                                  void* stream);

/* ---- BatchNorm (training statistics) + activation ------------------------------------------ */
/*
 * Reduce the conv epilogue's partials to batch statistics (nn.BatchNorm2d/1d in training mode,
 * model.py:137, 147, 158, 161, 218, 361, 372): mean, biased var -> invstd, scale = gamma*invstd,
 * shift = beta - mean*scale; running_mean/var updated with momentum (unbiased var), as torch does.
 * out4 = [mean | invstd | scale | shift], each C floats, once per group (groups x 4 x C); `count` is
 * the number of rows of ONE group; the partial rows are split evenly over the groups, which are
 * processed in order (running statistics receive `groups` successive updates).
 */
int s2i_bn_finalize(const float* part, int nparts, int groups, int C, long long count, const float* gamma,
                    const float* beta, float* running_mean, float* running_var,
                    long long* num_batches_tracked /* int64, += groups (one per stacked batch); may be NULL */, float momentum,
                    float eps, float* out4, void* stream);
/* eval-mode BatchNorm: scale/shift from the running statistics (trainer.py:681-803 path) */
int s2i_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* out4, void* stream);
/*
 * out = act(scale*y + shift) (+ residual).  GLU halves the channel count (C -> C/2).
 * Replaces BatchNorm apply + GLU / LeakyReLU / ResBlock add (model.py:116-122, 165-169).
 * act is S2I_ACT_NONE, S2I_ACT_GLU or S2I_ACT_LRELU; any other value (TANH, RELU, out of range) is refused: non-zero
 * return, message in s2i_last_error(), nothing launched.  The same holds for the two backward passes below.
 */
int s2i_bn_act_forward(const float* y, long long M, int groups, int C, const float* coef4, int act,
                       const float* residual, float* out, void* stream);
/* column sums of the raw tensor when no conv epilogue produced them: part = [2][nparts][C] */
int s2i_colstats(const float* y, long long M, int C, int ldy, float* part, int nparts,
                 void* stream);
/*
 * Backward of bn_act_forward, pass 1: per-channel sums of dz and dz*xhat (dz = gradient w.r.t. the
 * BatchNorm output after un-doing the activation).  part = [2][nparts][C].
 */
int s2i_bn_act_bwd_reduce(const float* y, const float* dout, int lddout, long long M, int groups, int C,
                          const float* coef4, int act, float* part, int nparts, void* stream);
/* finalise pass 1: dgamma, dbeta (accumulated or assigned) and the two means for pass 2.
   red2 = [mean_dz | mean_dz_xhat], each C floats. */
int s2i_bn_bwd_finalize(const float* part, int nparts, int groups, int C, long long count, float* dgamma,
                        float* dbeta, int accumulate, float* red2, void* stream);
/* pass 2: dy = scale * (dz - mean_dz - xhat*mean_dz_xhat) */
int s2i_bn_act_bwd_apply(const float* y, const float* dout, int lddout, long long M, int groups, int C,
                         const float* coef4, const float* red2, int act, float* dy, void* stream);

/* ---- plain activations ---------------------------------------------------------------------- */
/* dy = dout * act'(out) for LRELU / TANH given the forward OUTPUT (sign- / value-recoverable); any other act is refused
   (non-zero return, message in s2i_last_error(), nothing launched) */
int s2i_act_backward(const float* out, const float* dout, int lddout, long long M, int C, int act,
                     float* dy, void* stream);
/* 2-D GLU without BatchNorm (CA_NET, model.py:183): out[M][C/2] */
int s2i_glu_forward(const float* x, long long M, int C, float* out, void* stream);
int s2i_glu_backward(const float* x, const float* dout, long long M, int C, float* dx,
                     void* stream);

/* ---- layout ---------------------------------------------------------------------------------- */
/* NCHW (C channels) -> NHWC with Cp >= C channels (extra channels zero), and back */
int s2i_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, int Cp,
                     void* stream);
int s2i_nhwc_to_nchw(const float* src, int lds, float* dst, int B, int C, int H, int W,
                     void* stream);
/* [-1,1] float image (NHWC, row stride lds, first 3 channels) -> HWC uint8 RGB, the reference's
   `img.add(1).div(2).mul(255).clamp(0, 255).byte()` (trainer.py:676) fused with its permute(1,2,0) */
int s2i_image_to_u8(const float* src, int lds, unsigned char* dst, long long npix, void* stream);
/* HWC uint8 RGB [B][H][W][3] -> normalised NCHW float [B][3][H][W]: the reference's per-sample
   `ToTensor()` (x / 255) followed by `Normalize((.5,.5,.5), (.5,.5,.5))` ((t - 0.5) / 0.5), datasets.py:440-442,
   applied on the device to the collated uint8 batch (same fp32 operations in the same order: bit-identical) */
int s2i_u8_to_image(const unsigned char* src, float* dst, int B, int H, int W, void* stream);
/* The per-step half of the training image transform on images that stay in device memory (StackGAN_v2/datasets.py:40-66
   behind the transform of main.py:127-131): for each of the n plan rows (pool index, top, left, flip) the S x S
   RandomCrop window of resident image `pool index`, mirrored when flip != 0 (RandomHorizontalFlip), normalised as
   s2i_u8_to_image does, into out0 [n][3][S][S]; with L >= 2 also PIL's 8-bit bilinear resize of that window (not of the
   previous level, datasets.py:57-64) to S/2 into out1 [n][3][S/2][S/2], and with L = 3 to S/4 into out2.
   pool holds the uint8 HWC images back to back; image i starts at byte offsets[i] and is sizes[2i] rows of sizes[2i+1]
   pixels.  tab1 [S/2][5] and tab2 [S/4][9] are PIL's resample coefficients of S -> S/2 and S -> S/4 computed on the
   host: per output position the first input index, then 4 (8) taps in 22-bit fixed point, zero where PIL has fewer; the
   same table serves both passes.  A tap sum is (1 << 21) + sum of pixel * tap, shifted right by 22 and clamped to
   0..255; the horizontal pass writes a uint8 intermediate, as PIL does, so every plane is bit-identical to the host path.
   S is a multiple of 4 up to 256; out0 is 16-byte aligned.  A plan row that does not fit its image is skipped. */
int s2i_image_batch(const unsigned char* pool, long long pool_bytes, const long long* offsets, const int* sizes,
                    int npool, const int* plan, int n, int S, int L, const int* tab1, const int* tab2, float* out0,
                    float* out1, float* out2, void* stream);
/* The snapshot grid of the training loop (StackGAN_v2/trainer.py:268-295: `vutils.save_image(img, path, normalize=True)`,
   i.e. torchvision's make_grid(normalize=True) with its defaults followed by save_image's quantisation), composed on the
   device.  src holds N three-channel fp32 images addressed by element strides (image, row, column, channel): an NCHW
   batch and the generator's NHWC4 output alike; a fourth NHWC channel is never read.  dst is ONE uint8 HWC image of
   ymaps (H + padding) + padding rows by xmaps (W + padding) + padding columns, xmaps = min(nrow, N), ymaps =
   ceil(N / xmaps); image k has its top-left corner at row (k / xmaps)(H + padding) + padding, column
   (k % xmaps)(W + padding) + padding; every other pixel, the cells of an incomplete last row included, is 0.
   fp32, in this order, every operation rounded on its own (no fused multiply-add, IEEE division): lo / hi = minimum /
   maximum over all N 3 H W values (one pair for the batch); d = max(hi - lo, 1e-5); v = (x - lo) / d; q = v * 255;
   q = q + 0.5; clamp to [0, 255]; truncate.  A batch that holds a NaN or an infinity is outside the contract.
   workspace: s2i_image_grid_workspace_bytes() bytes of the caller's (per-block minima and maxima: the reduction and the
   composition are two launches on `stream` with no host round trip between them). */
size_t s2i_image_grid_workspace_bytes(void);
int s2i_image_grid_u8(const float* src, int N, int H, int W, long long stride_n, long long stride_y, long long stride_x,
                      long long stride_c, int nrow, int padding, float* workspace, unsigned char* dst, void* stream);
/* sum over the H*W rows of each image of the first C columns of a [B*HW][ld] tensor -> [B][C] */
int s2i_spatial_sum(const float* src, int ld, int B, int HW, int C, float* dst, void* ws,
                    size_t ws_bytes, void* stream);
size_t s2i_spatial_sum_workspace_bytes(int B, int HW, int C);

/* ---- differentiable augmentation of discriminator inputs, fused into the image layout conversion (csrc/s2i_diffaug.hip) ----
   x: fp32 NCHW [N][3][H][W], H == W, H even; table: DEVICE fp32 [N][8] of uniforms in [0, 1), row n =
   (u_b, u_s, u_c, u_tx, u_ty, u_cx, u_cy, unused); policy: a mask of the bits below; y: fp32 NHWC4 [N][H][W][4], channel 3
   exactly 0.  The stages apply in the order colour, translation, cutout; a stage whose bit is clear is the identity, and
   policy 0 writes what s2i_nchw_to_nhwc(.., Cp = 4) writes, bit for bit.  All arithmetic is fp32.
   colour:      b = u_b - 0.5, s = 2 u_s, k = u_c + 0.5; m = mean of the image's 3 H W raw values, p = mean of the pixel's
                three raw channels;  y_c = ((x_c + b) - (p + b)) s + (p + b);  z_c = (y_c - (m + b)) k + (m + b)
   translation: S = int(H / 8 + 0.5), n_t = 2 S + 1; tx = min(int(u_tx * n_t), n_t - 1) - S (one fp32 multiply, truncated),
                ty likewise; out[r][q] = z[r + ty][q + tx] where that source lies inside the image, exactly 0 elsewhere
   cutout:      c = int(H / 2 + 0.5), n_c = H + 1 - c % 2; oy = min(int(u_cy * n_c), n_c - 1), ox likewise; rows
                [oy - c / 2, oy - c / 2 + c) x columns [ox - c / 2, ox - c / 2 + c) of the translated image become exactly 0
   s2i_diffaug_backward is the exact adjoint: dy is the gradient of y as NHWC rows of `dtype` with pixel stride ld >= 4
   (the convention of s2i_nhwc_to_nchw_dt), dx fp32 NCHW [N][3][H][W];  g_z[r][q] = dy[r - ty][q - tx] where that pixel
   exists and is not cut out, else 0;  g_y = k g_z + (1 - k) mean_image(g_z);  g_x_c = s g_y_c + (1 - s) mean_c(g_y).
   Each direction is one launch, or two with S2I_DIFFAUG_COLOR (a per-image reduction into the caller's workspace of
   s2i_diffaug_workspace_bytes(N, H, W) bytes, summed in a fixed order: the same inputs give the same bits; ws may be NULL
   without the colour bit).  x and y must be 16-byte aligned.  Bad arguments (a null pointer, N < 1, H != W, H odd, an
   unknown policy bit, ld < 4, a workspace too small) return non-zero before any launch. */
enum { S2I_DIFFAUG_COLOR = 1, S2I_DIFFAUG_TRANSLATION = 2, S2I_DIFFAUG_CUTOUT = 4, S2I_DIFFAUG_ALL = 7 };
size_t s2i_diffaug_workspace_bytes(int N, int H, int W);
int s2i_diffaug_forward(const float* x, const float* table, int policy, float* y, int N, int H, int W, void* ws,
                        size_t ws_bytes, void* stream);
int s2i_diffaug_backward(int dtype, const void* dy, int ld, const float* table, int policy, float* dx, int N, int H, int W,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- SpecAugment of a log-mel training batch: masks drawn and applied on the device (csrc/s2i_specaug.hip) -------------
   x, y: fp32 [B][T][40] (the S2I_LOGMEL_NHWC batch), 16-byte aligned; they may be the same buffer.  valid: DEVICE int32
   [B]; n = valid[b] (clamped to [0, T]) is the number of leading rows of utterance b the masks may touch; rows at or after
   n are copied unchanged.  freq_masks, time_masks in [0, 8]; freq_width in [0, 20]; time_width >= 0; time_ratio in (0, 1];
   T <= 419430 (40 T < 2^24: the fp32 conversions below are exact).
   draws:  utterance b has 2 (freq_masks + time_masks) uniforms u_0, u_1, ...; nothing is uploaded.  Group g of four is
           Philox4x32-10 on key (seed mod 2^32, seed div 2^32) and counter (step mod 2^32, step div 2^32, b, g): ten rounds
           (c0, c1, c2, c3) -> (hi(0xCD9E8D57 c2) ^ c1 ^ k0, lo(0xCD9E8D57 c2), hi(0xD2511F53 c0) ^ c3 ^ k1, lo(0xD2511F53 c0)),
           hi / lo the halves of the 64-bit product, with k0 += 0x9E3779B9, k1 += 0xBB67AE85 (mod 2^32) between rounds.
           Output word r_i of group g gives u_{4g+i} = (float)(r_i >> 8) * 2^-24, in [0, 1).  Mask k (frequency masks
           first, then time masks) takes u = u_{2k}, u' = u_{2k+1}.  The same (seed, step, b) gives the same masks on any
           grid and in any batch.
   masks:  int() truncates one fp32 product.
           frequency: f = min(int(u (float)(freq_width + 1)), freq_width); f0 = min(int(u' (float)(40 - f + 1)), 40 - f);
                      bins [f0, f0 + f) of rows [0, n)
           time:      W = min(time_width, int(time_ratio (float)n)); t = min(int(u (float)(W + 1)), W);
                      t0 = min(int(u' (float)(n - t + 1)), n - t); rows [t0, t0 + t), all bins; n == 0 or W == 0: nothing
   value:  every masked cell of utterance b becomes m_b = S_b / (float)(40 n), S_b the fp32 sum of its 40 n unmasked inputs
           in a fixed order (no atomics; the same inputs give the same bits): the 10 n sixteen-byte pieces of rows [0, n)
           are cut into segs = min(64, max(1, 10 T div 1024)) runs of chunk = ceil(10 n / segs) consecutive pieces; thread j
           of a run's 256 adds pieces j, j + 256, ... in that order into four lanes starting at 0; the lanes fold
           (a0 + a1) + (a2 + a3); a wave's 64 lanes by an xor butterfly (offsets 32 .. 1); the four waves ((w0 + w1) + w2)
           + w3; the segs run sums, zero-padded to 64, by the same butterfly.  A term passes through at most
           d(T) = ceil(ceil(10 T / segs) / 256) + 17 additions (22 at T = 128, 21 at T = 2048).
   At most two launches on `stream` with no host round trip: the run sums into the caller's workspace of
   s2i_specaug_workspace_bytes(B) bytes, then a copy-or-mask in 16-byte pieces, four per thread; with x == y only pieces
   that hold a masked cell are written.  freq_masks == time_masks == 0 writes y = x bit for bit (one launch, none with
   x == y; ws may be NULL).  Bad arguments (a null pointer, B < 1, T < 1, T too large, misalignment, a count, width or
   ratio outside its range, a workspace too small) return non-zero before any launch. */
size_t s2i_specaug_workspace_bytes(int B);
int s2i_specaug(const float* x, const int* valid, int B, int T, float* y, int freq_masks, int freq_width, int time_masks,
                int time_width, float time_ratio, unsigned long long seed, unsigned long long step, void* ws,
                size_t ws_bytes, void* stream);

/* ---- additive white noise and babble on a batch of waveforms, in place (csrc/s2i_waveaug.hip) ----------------------------
   x: the flat fp32 batch that s2i_pcm_resample wrote, 16-byte aligned; clip b is x[offsets[b] .. offsets[b] + n), offsets
   DEVICE int64 [B] in floats, n = lens[b] (DEVICE int32 [B], clamped to [0, max_len]).  max_len is the host's bound on the
   lens, in [1, 2^31 - 5]: a sample number i stays under 2^31 - 4.  pool: the fp32 samples an interferer is read from,
   16-byte aligned, never written and disjoint from x; NULL turns babble off for every clip.  table: DEVICE, 32 bytes per
   clip, 16-byte aligned:
     float g_white; float g_babble; long long src; int n_j; int start; unsigned uid; int pad;
   g_white = 10^(-snr / 10) and g_babble = 10^(-snr / 10) / Q_j (Q_j the interferer's mean square), computed in float64 by
   the host and rounded to fp32 once; 0 switches the term off.  The interferer is pool[src .. src + n_j), n_j >= 1, read
   cyclically from `start` in [0, n_j); uid is the clip's id in the noise counter.
   power:  P_b = S_b / (float)n (a correctly rounded division), S_b the fp32 sum of the n squares x_i x_i (each square
           rounded, then added) in a fixed order without atomics.  The clip is cut into runs of 8192 samples = 2048
           four-sample pieces, counted from its first sample; thread j of a run's 256 adds pieces j, j + 256, ..., j + 1792
           in that order, sample c of a piece into lane c of a four-lane accumulator that starts at 0 (a sample at or past
           n adds nothing); the lanes fold (a0 + a1) + (a2 + a3); a wave's 64 lanes by an xor butterfly (offsets 32 .. 1);
           the four waves ((w0 + w1) + w2) + w3.  The ceil(n / 8192) run sums are added by 64 lanes, lane l taking runs l,
           l + 64, ... in that order from 0, then the same butterfly.  The zero tail s2i_pcm_resample writes is part of the
           n samples.  The same clip gives the same bits in any batch, at any offset and for any max_len.
   white:  a_w = sqrtf(P_b g_white) (the product rounded, the root correctly rounded).  Sample i takes the Philox4x32-10
           block (the rounds of s2i_specaug) with key (seed mod 2^32, (seed div 2^32) ^ 0x57415645) and counter
           (step mod 2^32, step div 2^32, uid, 2 + i div 2): words (r0, r1) for an even i, (r2, r3) for an odd one.  h = the
           sum of the four 16-bit halves of the two words, in [0, 262140]; e_i = ((float)h - 131070.0f) c with
           c = 0x1.bb67aep-16f, 1 / sqrt((2^32 - 1) / 3) rounded to fp32: the sum of four uniform 16-bit integers, centred
           and scaled to unit variance (Irwin-Hall; |e_i| <= 3.4641).  The key differs from s2i_specaug's in word 1 for
           every seed, so the two never share a block; counters 0 and 1 of a uid are the host's draws.
   babble: a_b = sqrtf(P_b g_babble);  v_i = pool[src + (start + i) mod n_j].
   result: y_i = (x_i + a_w e_i) + a_b v_i, every product and every sum rounded to fp32 on its own, in that order (a term
           that is off is not added).  P_b == 0, or both gains 0, leaves the clip unwritten; samples outside the clips are
           never written.
   Two launches on `stream` with no host round trip: the run sums into the caller's workspace of
   s2i_wave_mix_workspace_bytes(B, max_len) = 4 B ceil(max_len / 8192) bytes, then the mix, four pieces per thread, in
   16-byte accesses where the clip starts on a 16-byte boundary and sample by sample elsewhere (the same sums either way).
   Bad arguments (a null x, offsets, lens, table or workspace, B < 1, max_len outside its range, a misaligned buffer, a
   workspace too small) return non-zero before any launch; s2i_wave_mix_workspace_bytes returns 0 for them. */
size_t s2i_wave_mix_workspace_bytes(int B, int max_len);
int s2i_wave_mix(float* x, const long long* offsets, const int* lens, int B, int max_len, const float* pool,
                 const void* table, unsigned long long seed, unsigned long long step, void* ws, size_t ws_bytes,
                 void* stream);

/* ---- room reverberation of a batch of waveforms (csrc/s2i_reverb.hip) -------------------------------------------------------
   Each clip is convolved with a room impulse response (RIR) of its own: a unit direct path and an exponentially decaying
   noise tail.  table: DEVICE, 16 bytes per clip, 16-byte aligned:
     float alpha; float slope; int taps; unsigned uid;
   taps == 0 switches the clip off; else taps is a multiple of 32 in [32, max_taps].  slope = -log2(1000) / (T60 16000), the
   log2 of the envelope per tap (the tail is 60 dB down after T60 seconds), and alpha = sqrt(10^(-DRR / 10) / E) with
   E = sum_{k = 1}^{taps - 1} 2^(2 k slope), both computed in float64 by the host and rounded to fp32 once; uid is the clip's
   id in the counter.

   s2i_reverb_rir writes h[B][max_taps] (fp32, 16-byte aligned), max_taps a multiple of 32 in [32, 16000].  Row b:
     h[0] = 1;   h[k] = (alpha e_k) env_k for 1 <= k < taps;   h[k] = 0 for taps <= k < max_taps
   (a row with taps == 0 is all zeros and never read).  env_k = exp2f((float)k slope): the product rounded to fp32, then
   exp2f.  e_k is s2i_wave_mix's unit-variance value ((float)s - 131070.0f) 0x1.bb67aep-16f, s the sum of the four 16-bit
   halves of two words of the Philox4x32-10 block with key (seed mod 2^32, (seed div 2^32) ^ 0x52455642) and counter
   (step mod 2^32, step div 2^32, uid, 1 + k div 2): words (r0, r1) for an even k, (r2, r3) for an odd one.  The key differs
   in word 1 from s2i_specaug's and from s2i_wave_mix's for every seed, so no block is shared with either; counter 0 of a
   uid is the host's draws.  The two products are rounded to fp32 one after the other, alpha e_k first (no fused
   multiply-add).  One launch, one thread per tap.

   s2i_reverb writes y, a second flat fp32 buffer laid out as x: clip b is x[offsets[b] .. offsets[b] + n) and
   y[offsets[b] .. offsets[b] + n), offsets DEVICE int64 [B] in floats, n = lens[b] (DEVICE int32 [B], clamped to
   [0, max_len]); max_len is the host's bound on the lens, in [1, 2^31 - 8225].  x, y and h are 16-byte aligned and y is
   disjoint from x and h.  For a clip with taps > 0
     y_i = sum_{k = 0}^{taps - 1} h[k] x_{i - k},   i in [0, n),   x_i = 0 for i < 0:
   the clip keeps its length and the tail past it is cut; nothing is renormalised (the log-mel front end is invariant to a
   clip's gain).  A clip with taps == 0 is copied bit for bit.  Floats outside the clips are never written.
   order:  the sum is a block-Toeplitz product on v_mfma_f32_32x32x2_f32, an exact fmaf chain.  Write i = 32 a + b with
           b in [0, 32).  Output i has ONE fp32 accumulator that starts at +0 and takes
             acc = fmaf(h[32 j + b - m], x[32 (a - j) + m], acc)     (h = 0 outside [0, taps), x = 0 outside [0, n))
           for j = 0, 1, ..., min(taps / 32, a) in that order and, inside a j, for m = 0, 1, ..., 31 in that order.  Blocks
           j > a multiply samples before the clip and are skipped.  The order depends on i, taps and n alone: the same clip
           with the same h gives the same bits alone or in any batch, at any offset and for any max_len, on every run.
   One launch over (clip, tile of 8192 outputs), no workspace, no atomics, no host round trip.
   Bad arguments (a null pointer, B < 1, max_len or max_taps outside its range, a misaligned buffer, y == x or y == h)
   return non-zero before any launch. */
int s2i_reverb_rir(const void* table, int B, int max_taps, float* h, unsigned long long seed, unsigned long long step,
                   void* stream);
int s2i_reverb(const float* x, const long long* offsets, const int* lens, int B, int max_len, const void* table,
               const float* h, int max_taps, float* y, void* stream);

/* ---- time stretch of a batch of waveforms: the short-time phase vocoder (csrc/s2i_stretch.hip) -----------------------------
   librosa.effects.time_stretch with n_fft 512, hop 128, a periodic Hann window and zero centre padding, the phase kept in
   turns; with the resampler behind it, it is also the pitch shift.  x: a flat fp32 batch, clip b is
   x[offsets[b] .. offsets[b] + n), offsets DEVICE int64 [B] in floats, n = lens[b] (DEVICE int32 [B], clamped to
   [0, max_len]); max_len is the host's bound on the lens, in [1, 2^29 - 1025].  y: a second flat fp32 buffer, disjoint from
   x; clip b is written to y[out_offsets[b] .. out_offsets[b] + out_len), out_offsets DEVICE int64 [B].  x, y, the basis
   and the workspace are 16-byte aligned.  table: DEVICE, 16 bytes per clip, 16-byte aligned:
     double rate; int out_len; int out_frames;
   rate == 1.0 exactly copies the first min(n, out_len) samples bit for bit.  Otherwise rate lies in [0.25, 4] and, with
   F = 1 + n div 128, out_len = floor(n / rate + 0.5) and out_frames = ceil(F / rate), both computed in float64 by the
   host; out_len is clamped to [0, max_out_len] (the host's bound on the out_len, at most 4 max_len) and out_frames to
   [0, 4 F].  A clip with n == 0 or a rate outside [0.25, 4] (NaN included) is left unwritten.  So is a stretched
   clip whose frames, counted behind those of every stretched clip before it in the table, reach beyond the totals given,
   and with it every stretched clip behind it; copied clips are written all the same.  Floats outside the clips are never written.
   basis: DEVICE fp32 [s2i_stretch_basis_elems() = 2 x 512 x 512 + 512], built in float64 and rounded once:
     forward [512 samples i][512 columns]: column tile 2 t + h (16 columns, c the column inside it) holds, for bin
       k = 16 t + c, w[i] cos(2 pi i k / 512) where h = 0 and -w[i] sin(2 pi i k / 512) where h = 1; bin 0 has no sine and
       its h = 1 column is bin 256's cosine, w[i] cos(pi i);
     inverse [512 rows][512 samples i]: row k <= 256 is c_k w[i] / 512 cos(2 pi i k / 512) and row 256 + k, k = 1..255, is
       -2 w[i] / 512 sin(2 pi i k / 512), c_0 = c_256 = 1 and c_k = 2 otherwise;
     both stored in fragment order: element (row r, column c of column tile nt) at
       ((r div 16 * 32 + nt) * 64 + (r mod 4) * 16 + c) * 4 + (r mod 16) div 4;
     then w[512], w[i] = 0.5 - 0.5 cos(2 pi i / 512).
   analysis:  the clip is zero-padded by 256 samples at both ends; X_t[k] = sum_i w[i] xpad[128 t + i] e^(-2 pi i k / 512)
           for t < F, k = 0..256 (frames F and F + 1 are zero); |X| = hypotf(re, im) and
           arg X / 2 pi = atan2f(im, re) 0x1.45f306p-3f are what is kept (arg(0) = 0).
   stretch:  for output frame t < out_frames: s = (double)t rate, j = floor(s), a = (float)(s - j);
             M_t[k] = (1 - a) |X_j[k]| + a |X_j+1[k]|, each product rounded, then the sum;
             Y_t[k] = M_t[k] (cos, sin)(2 pi theta_t[k]) through sincospif(2 theta);
             theta_0[k] = arg X_0[k] / 2 pi;  with phi_k = (k mod 4) / 4 and wrap(v) = v - rintf(v),
             d = wrap((arg X_j+1[k] / 2 pi - arg X_j[k] / 2 pi) - phi_k),  theta_t+1[k] = wrap((theta_t[k] + phi_k) + d).
   synthesis:  y_t[i] = sum over the 512 rows of the inverse basis of [Re Y_t[0..256] | Im Y_t[1..255]] times the row.
   overlap-add:  for m in [0, out_len), u = m + 256: the frames t < out_frames with 0 <= u - 128 t < 512, in ascending t,
           add y_t[u - 128 t] to a numerator and w[u - 128 t] w[u - 128 t] (rounded) to a denominator, both from 0;
           out[m] = numerator / denominator (a correctly rounded division) where the denominator exceeds 1e-10f, else the
           numerator; 0 where no frame covers u.
   order:  each output of a transform is summed in SIXTEEN runs of 32 consecutive samples (analysis) or basis rows
           (synthesis).  A run has an fp32 accumulator p_r of its own that starts at +0 and takes its 32 products on
           v_mfma_f32_16x16x4_f32 in ascending order, each product an fmaf; the output is
           (((0 + p_0) + p_1) + ...) + p_15.  A product with a zero of the padding adds +-0.  The phase recursion of a (clip, bin) is one
           thread's, in ascending t.  Every order depends on the clip alone: the same clip with the same rate gives the
           same bits alone or in any batch, at any offset and for any max_len, on every run.
   Five launches on `stream` (the clips' places in the workspace, analysis, recursion, synthesis, overlap-add), no atomics,
   no block waits on another, no host round trip.  The caller owns the workspace of
   s2i_time_stretch_workspace_bytes(B, in_frames_total, out_frames_total) bytes, the totals being at least the sums of F
   and of out_frames over the clips with rate != 1.  Bad arguments (a null pointer, B < 1, max_len or max_out_len outside its
   range, negative totals, a misaligned buffer, y == x, a workspace too small) return non-zero before any launch;
   s2i_time_stretch_workspace_bytes returns 0 for them. */
size_t s2i_stretch_basis_elems(void);
size_t s2i_time_stretch_workspace_bytes(int B, long long in_frames_total, long long out_frames_total);
int s2i_time_stretch(const float* x, const long long* offsets, const int* lens, int B, int max_len, const void* table,
                     const float* basis, float* y, const long long* out_offsets, int max_out_len,
                     long long in_frames_total, long long out_frames_total, void* ws, size_t ws_bytes, void* stream);

/* ---- CA_NET reparameterisation + KL (model.py:182-200, trainer.py:54-58) -------------------- */
/* h = GLU output [B][2E] = [mu | logvar];  c = eps*exp(0.5*logvar) + mu */
int s2i_reparam_forward(const float* h, const float* eps, int B, int E, float* c, void* stream);
/* dh[:, :E] = dc + dmu_extra ; dh[:, E:] = dc*eps*0.5*exp(0.5*logvar) + dlogvar_extra */
int s2i_reparam_backward(const float* h, const float* eps, const float* dc, const float* dmu,
                         const float* dlogvar, int B, int E, float* dh, void* stream);
/* kl = -0.5*mean(1 + logvar - mu^2 - exp(logvar));  also the gradient scaled by `gscale` */
int s2i_kl_forward(const float* mu, int ldmu, const float* logvar, int ldlv, int B, int E,
                   float* kl, void* stream);
int s2i_kl_backward(const float* mu, int ldmu, const float* logvar, int ldlv, int B, int E,
                    const float* gout, float* dmu, float* dlogvar, void* stream);

/* ---- logit heads: Conv2d(C,1,k=4,s=4)+Sigmoid on a 4x4 map (model.py:414-422) + BCE --------- */
/* x NHWC [B][16][C]; w OIHW [1][C][4][4]; prob[b] = sigmoid(<x_b,w> + bias) */
int s2i_logit_forward(const float* x, const float* w, const float* bias, int B, int C,
                      float* prob, void* stream);
/* dlogit[b] given dprob; dx (+)= dlogit*w ; dw (+)= sum_b dlogit*x ; dbias (+)= sum dlogit */
int s2i_logit_backward(const float* x, const float* w, const float* prob, const float* dprob,
                       int B, int C, float* dx, int acc_dx, float* dw, float* dbias, int acc_dw,
                       void* stream);
/* nn.BCELoss(mean) with torch's log clamp at -100 (trainer.py:394-409, 439-443):
   loss (+)= weight * mean(-(t*log p + (1-t)*log(1-p))) ; dprob = weight*gout * dL/dp */
int s2i_bce_forward(const float* prob, float target, int B, float weight, float* loss,
                    int accumulate, void* stream);
int s2i_bce_backward(const float* prob, float target, int B, float weight, const float* gout,
                     float* dprob, void* stream);

/* Sum of G*H BCE terms in one launch (the six terms of trainer.py:394-409): probs[h] is head h's
   probabilities for G stacked batches of B rows; term (g,h) uses target[g*H+h] and weight[g*H+h].
   loss = sum_{g,h} weight * mean_b BCE(probs[h][g*B+b], target);  backward writes dprobs[h] likewise. */
int s2i_bce_multi_forward(const float* const* probs_dev, const float* target, const float* weight, int G, int H,
                          int B, float* loss, void* stream);
int s2i_bce_multi_backward(const float* const* probs_dev, const float* target, const float* weight, int G, int H,
                           int B, const float* gout, float* const* dprobs_dev, void* stream);

/* ---- class-aware loss (trainer.py:298-311) ------------------------------------------------------ */
/* scores = X X^T [B][B] (from s2i_conv_forward, K1, wmode 1); labels int32 [B];
   loss = max(0, mean(S) - mean(S[same class, off-diagonal])) / D, 0 when no such pair.
   dscores = d loss / d S (so that dX = (dS + dS^T) X), both scaled by nothing: caller scales. */
int s2i_cal_loss(const float* scores, const int* labels, int B, int D, float* loss, int accumulate,
                 float* dscores_sym, void* stream);

/* ---- speech-encoder front-end (Audio_to_Image/speech_encoder.py:15-97), inference ---------------- */
/* nn.MaxPool2d((1,3), stride (1,2), padding (0,1)) on NHWC [B][H][W][C] -> [B][H][W/2][C] */
int s2i_maxpool_w3s2(const float* x, int B, int H, int W, int C, float* y, void* stream);
/*
 * One nn.LSTM step for every sequence of a packed batch, one direction.
 *   xproj [B][T][ldx] (this direction's 4*Hd gate pre-activations from the input, biases included, at
 *   column offset already applied), hproj [B][4*Hd] = h_prev W_hh^T, gates in torch order (i, f, g, o).
 *   Sequence b has lens[b] valid steps; at step `s` it processes t = s (forward) or lens[b]-1-s (reverse);
 *   finished sequences keep their state and write nothing (padded outputs stay zero).
 *   h, c [B][Hd] are updated in place; out [B][T][ldo] receives h at (b, t) at column offset applied.
 */
int s2i_lstm_cell(const float* xproj, int ldx, const float* hproj, const int* lens, int B, int T, int Hd,
                  int step, int reverse, float* h, float* c, float* out, int ldo, void* stream);
/* The same step for all D directions in one launch, with the recurrent projection fused in: gates = xproj[b][t] +
 * h_in[d][b] . whh_d^T (whh_* are the reference's weight_hh_l0 / weight_hh_l0_reverse, (4*Hd, Hd) row-major);
 * h_in / h_out [D][B][Hd] are distinct buffers (ping-pong), c [D][B][Hd] in place; direction 1 runs reversed. */
int s2i_lstm_step(const float* xproj, int ldx, const float* whh_fwd, const float* whh_rev, const int* lens,
                  int B, int T, int Hd, int D, int step, const float* h_in, float* h_out, float* c, float* out,
                  int ldo, void* stream);
/* y[b][c] = mean over the T rows of x[b][t][c] (sent_emb = output.mean(-2), speech_encoder.py:93) */
int s2i_time_mean(const float* x, int B, int T, int C, float* y, void* stream);

/* ---- speech-encoder head, training (Audio_to_Image/train_audio_encoder.py:168-216, 308-361, jel.py:17-43) -------- */
/*
 * s2i_lstm_step that also stores what the backward needs.  Same recurrence, same `out` bit for bit.  In addition, for every
 * valid (b, t, d): gates [B][T][D*4*Hd] (i, f, g, o AFTER their activations, in xproj's column layout), cst [B][T][D*Hd]
 * (c_t, in out's layout) and hprev [D][B][T][Hd] (the h the step started from).  ldx = D*4*Hd and ldo = D*Hd (dense rows).
 * The call with step = 0 also zeroes out and hprev at t >= lens[b], so neither needs clearing; gates and cst are not
 * written there.  B <= 32, Hd % 8 == 0, Hd <= 512.
 */
int s2i_lstm_train_step(const float* xproj, int ldx, const float* whh_fwd, const float* whh_rev, const int* lens, int B, int T,
                        int Hd, int D, int step, const float* h_in, float* h_out, float* c, float* out, int ldo,
                        float* gates, float* cst, float* hprev, void* stream);
/* s2i_lstm_cell with the same stores, one direction: xproj, out, gates (row stride ldx) and cst (row stride ldo) carry the
 * direction's column offset, hprev is the direction's [B][T][Hd].  Any B and Hd. */
int s2i_lstm_train_cell(const float* xproj, int ldx, const float* hproj, const int* lens, int B, int T, int Hd, int step,
                        int reverse, float* h, float* c, float* out, int ldo, float* gates, float* cst, float* hprev,
                        void* stream);
/*
 * One step of the LSTM's backward through time, every direction in one launch.  Called for step = max(lens)-1 .. 0, the
 * first call with first = 1.  With dh = d_out[b][t] + d_sent[b] / T + dG_{step+1}[b] . W_hh (d_out [B][T][D*Hd] and d_sent
 * [B][D*Hd] may each be null; d_sent is the gradient of the mean over all T steps) and dc = dc_rec + dh o (1 - tanh^2 c_t):
 *   dG[b][t] = (dc g i(1-i), dc c_{prev} f(1-f), dc i (1-g^2), dh tanh(c_t) o(1-o)),   dc_rec = dc f
 * dG [B][T][D*4*Hd] is written at every valid (b, t) and, by the first call, zeroed at t >= lens[b].  whht_* are the
 * TRANSPOSED recurrent weights, [Hd][4*Hd] row-major.  dc [D][B][Hd] is scratch carried between the calls (initialised by
 * the first).  A sequence with step >= lens[b] contributes nothing.  B <= 32, Hd % 8 == 0, Hd <= 512.
 */
int s2i_lstm_bwd_step(const float* d_out, const float* d_sent, const float* gates, const float* cst, const float* whht_fwd,
                      const float* whht_rev, const int* lens, int B, int T, int Hd, int D, int step, int first, float* dc,
                      float* dG, void* stream);
/* The same step for one direction with the recurrent product done by the caller: dhrec [B][Hd] = dgt . W_hh of the
 * previous call (ignored when first), dgt [B][4*Hd] receives this step's dG rows (zero for step >= lens[b]).  d_out, d_sent,
 * cst (row stride ldo) and gates, dG (row stride ldg) carry the direction's column offset; dc [B][Hd].  Any B and Hd. */
int s2i_lstm_bwd_cell(const float* d_out, const float* d_sent, int ldo, const float* gates, int ldg, const float* cst,
                      const float* dhrec, const int* lens, int B, int T, int Hd, int step, int reverse, int first, float* dc,
                      float* dG, float* dgt, void* stream);
/* db [N] = the column sums of dG [M][N] (bias_ih and bias_hh gradients: both equal the sum of dG over every (b, t)) */
int s2i_lstm_bias_grad(const float* dG, long long M, int N, float* db, void* stream);
/*
 * The encoder's loss and its gradient for the audio embedding; audio, image [B][C], label [B].
 *   flags bit 0: joint-embedding loss, score = image . audio^T, score_abs[i][j] = score[i][j] - score[j][j],
 *                (c_diff sum_{label_i != label_j} relu(score_abs + 1) + c_same sum_{label_i == label_j} relu(score_abs)) / B^2
 *                and accu = 100 / B #{i: argmax_j score[i][j] == i} (lowest index wins a tie)
 *         bit 1: mean |audio / |audio|_F - image / |image|_F| over B*C, times lambda_l1
 *         bit 2: sum softmax(image / T) (log softmax(image / T) - log_softmax(audio)) / (B*C), times lambda_distill
 * scal[5] = total, jel, l1, distill (unweighted parts), accu; grad [B][C] = d total / d audio.
 */
#define S2I_ENC_LOSS_JEL 1
#define S2I_ENC_LOSS_L1 2
#define S2I_ENC_LOSS_DISTILL 4
size_t s2i_encoder_loss_workspace_bytes(int B);
int s2i_encoder_loss(const float* audio, const float* image, const int* label, int B, int C, float c_diff, float c_same,
                     int flags, float lambda_l1, float lambda_distill, float distill_T, void* ws, size_t ws_bytes,
                     float* grad, float* scal, void* stream);

/* ---- speech-encoder conv stack, training (Audio_to_Image/speech_encoder.py:26-52 under autograd, as driven by
 * train_audio_encoder.py:168-216).  fp32, single GPU, activations NHWC [B][1][W][C], W and Wo powers of two. ------------- */
/*
 * Input gradient of a (1 x kw) temporal convolution, Wo = (W + 2 pad - kw) / stride + 1:
 *   dx[b][i][c] = sum_t sum_o dy[b][(i + pad - t) / stride][o] * w[o][c][t]   over the taps with (i + pad - t) % stride == 0
 * dy [B][Wo][Cout], dx [B][W][Cin] (every element written); w_packed is the forward's P[t][wR][ldw] (S2I_PACK_PLAIN).
 * stride 1 or 2, stride <= kw <= 31, 32 | Cout, 4 | Cin.  Implicit GEMM on v_mfma_f32_32x32x2_f32; with stride 2 each
 * parity of i + pad is a launch phase with its own taps, so no structurally zero product is computed.
 */
int s2i_conv1d_dgrad(const float* dy, const float* w_packed, float* dx, int B, int W, int Cin, int Cout, int wR, int ldw,
                     int kw, int stride, int pad, void* stream);
/*
 * Its weight gradient, written (not accumulated) in the parameter's OIHW (Cout, Cin, 1, kw) layout:
 *   dw[o][c][0][t] = sum_{b, ox} dy[b][ox][o] * x[b][ox stride - pad + t][c]     (positions outside [0, W) contribute nothing)
 * The B * Wo rows are split into slabs where the result has too few tiles to fill the chip, and never more than 512 rows
 * per slab; a second launch adds the slabs in a fixed order (in double).  No atomics: bit-identical from run to run.
 * The workspace holds the slabs; s2i_conv1d_wgrad_workspace_bytes returns 0 for a bad geometry.
 */
size_t s2i_conv1d_wgrad_workspace_bytes(int B, int W, int Cin, int Cout, int kw, int stride, int pad);
int s2i_conv1d_wgrad(const float* x, const float* dy, float* dw_oihw, int B, int W, int Cin, int Cout, int kw, int stride,
                     int pad, void* ws, size_t ws_bytes, void* stream);
/* Train-mode BatchNorm + ReLU on the raw convolution output y [M][C] with the coefficient table of s2i_bn_finalize (one
   group): out = max(scale * y + shift, 0). */
int s2i_bn_relu_forward(const float* y, long long M, int C, const float* coef4, float* out, void* stream);
/* Its backward in the reduce / finalize / apply scheme of s2i_bn_act_bwd_*: dz = dout where the stored forward output
   `out` is > 0, else 0 (ReLU'(0) = 0).  Pass 1: part = [2][nparts][C] sums of dz and dz * xhat over nparts row chunks
   (nparts <= M); s2i_bn_bwd_finalize turns them into dgamma, dbeta and red2; pass 2: dy = scale * (dz - mean_dz - xhat *
   mean_dz_xhat). */
int s2i_bn_relu_bwd_reduce(const float* y, const float* out, const float* dout, long long M, int C, const float* coef4,
                           float* part, int nparts, void* stream);
int s2i_bn_relu_bwd_apply(const float* y, const float* out, const float* dout, long long M, int C, const float* coef4,
                          const float* red2, float* dy, void* stream);
/* Backward of s2i_maxpool_w3s2 as a gather: dx[i] = sum of dy[j] over the (at most two) windows j that contain i and whose
   maximum, recomputed from the stored pool input x, is at i; a tie goes to the lowest position, as torch's max_pool2d.
   x, dx [B][H][W][C], dy [B][H][W/2][C]. */
int s2i_maxpool_w3s2_backward(const float* x, const float* dy, int B, int H, int W, int C, float* dx, void* stream);
/* The leading BatchNorm2d(1): one channel over all n = 4 q elements.  The per-channel apply kernels run on the [q][4] view
   (s2i_bn_act_forward / _bwd_apply with C = 4, S2I_ACT_NONE); the two finalize calls fold the four columns
   of the partial sums ([2][nparts][4]) into the one channel.  s2i_bn1_stats writes the sums of x and of x * x in that
   layout, formed in double and stored as (high, low) float pairs in columns 0 and 1: the input is un-normalised log-mel
   (mean^2 several times the variance), which fp32 sums of fp32 squares do not tolerate.  s2i_bn1_bwd_reduce writes the backward sums of dout and
   dout * xhat in that layout (column 0; a block's terms are added in double: d weight is a sum over every input element).  s2i_bn1_finalize writes the C = 4 coefficient table
   [mean x4 | invstd x4 | scale x4 | shift x4] and updates the running statistics as s2i_bn_finalize does (count = n);
   s2i_bn1_bwd_finalize writes dgamma[0], dbeta[0] (assigned; either may be NULL) and red2 = [mean_dz x4 | mean_dz_xhat x4]. */
int s2i_bn1_stats(const float* x, long long n, float* part, int nparts, void* stream);
int s2i_bn1_finalize(const float* part, int nparts, long long count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                     float* coef4x4, void* stream);
int s2i_bn1_bwd_reduce(const float* x, const float* dout, long long n, const float* coef4x4, float* part, int nparts,
                       void* stream);
int s2i_bn1_bwd_finalize(const float* part, int nparts, long long count, float* dgamma, float* dbeta, float* red2x4,
                         void* stream);

/* ---- optimiser (trainer.py:236-252, 571-572) -------------------------------------------------- */
/* torch.optim.Adam (no weight decay, no amsgrad) on a flat buffer, step = 1-based step count */
int s2i_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                  float beta2, float eps, int step, const int* step_dev, float gscale, void* stream);
/* torch.optim.Adam(weight_decay = wd) on a flat buffer, the speech encoder's optimiser (train_audio_encoder.py:462):
   the effective gradient is gscale * g + weight_decay * p (L2 decay, added before the moments), then the update of
   s2i_adam_step.  With weight_decay = 0 the results are those of s2i_adam_step bit for bit. */
int s2i_adam_l2_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, const int* step_dev, float gscale, void* stream);
/* *counter += 1 on the stream (device-resident Adam step count, so a captured hipGraph of the
   train step replays with the right bias correction) */
int s2i_increment(int* counter, void* stream);
/* Gradient-norm clipping and the non-finite guard of the fused optimiser: three launches, nothing read by the host.
   The layout is trainer.FlatNet's: tensor s holds sizes[s] >= 1 elements from element offsets[s] (a multiple of 4) of the flat
   buffer g of n elements, cut into chunks of S2I_GRAD_CHUNK elements from its first element on; chunk0[s] is the index of
   its first chunk among all chunks and chunk0[S] = nchunks.  offsets, sizes [S] and chunk0 [S + 1] are device arrays.
   s2i_grad_sumsq: partials[c] = sum of the squares of chunk c, every element converted to fp64 first (the square is then
   exact and no sum over fp32 data overflows or underflows), one block per chunk, 16-byte loads where the chunk's first
   element is 16-byte aligned, elements between tensors never read, no atomics; the order of the additions is a function of
   the layout alone (csrc/s2i_optim.hip states it), so equal inputs give equal bits.  A chunk that would leave [0, n) is
   not read and its partial is NaN.
   s2i_grad_clip_scale (one block): seg[s] = sum of tensor s's partials, total = sum of seg in ascending s,
   norm = sqrt(total) |gscale|, coef = min(1, max_norm / (norm + 1e-6)) if max_norm > 0 else 1 (torch.nn.utils.clip_grad_norm_),
   scale_dev[0] = (float)(gscale coef), apply_dev[0] = isfinite(total); if that holds and step_dev is given, step_dev[0] += 1
   (it stands in for s2i_increment).  stats, S2I_GRAD_STATS_HEAD + 2 S doubles, zeroed by the caller before the first call:
   [0] norm [1] coef [2] scale [3] apply of this call; since the caller last zeroed them [4] applied updates, [5] those with
   coef < 1, [6] skipped ones, [7] sum and [8] maximum of norm over the applied ones; [9] total; [HEAD + s] the norm of
   tensor s, sqrt(seg[s]) |gscale|; [HEAD + S + s] seg[s]. */
#define S2I_GRAD_CHUNK 4096
#define S2I_GRAD_STATS_HEAD 16
int s2i_grad_sumsq(const float* g, long long n, const long long* offsets, const long long* sizes, const long long* chunk0,
                   int S, long long nchunks, double* partials, void* stream);
int s2i_grad_clip_scale(const double* partials, const long long* chunk0, int S, double gscale, double max_norm, int* step_dev,
                        float* scale_dev, int* apply_dev, double* stats, void* stream);
/* s2i_adam_step / s2i_adam_l2_step with the step count, gscale and a flag read from the device: gscale_dev[0] takes
   gscale's place, and with apply_dev[0] == 0 nothing is stored: p, m and v stay as they are, weight decay included.  With
   gscale_dev[0] == gscale the results are those of the host-value entry points bit for bit. */
int s2i_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                      float eps, const int* step_dev, const float* gscale_dev, const int* apply_dev, void* stream);
int s2i_adam_l2_step_dev(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, const int* step_dev, const float* gscale_dev, const int* apply_dev,
                         void* stream);
/* avg = decay*avg + (1-decay)*p */
int s2i_ema_update(float* avg, const float* p, long long n, float decay, void* stream);
/* y = x * a_dev[0] (the scalar lives on the device: no host synchronisation) */
int s2i_scale_dev(float* y, const float* x, long long n, const float* a_dev, void* stream);
/* y = a*x (+ y) elementwise helpers used for gradient averaging and accumulation */
int s2i_axpby(float* y, const float* x, long long n, float a, float b, void* stream);

/* ---- launch-plan replay (host-side machinery of this build; the reference's loop body, trainer.py:536-572, is a
 * Python loop over torch ops) -----------------------------------------------------------------------------------------
 * One stream's piece of the train step is recorded ONCE by HIP stream capture (so launches that do not come from this
 * library are recorded too) and re-issued per step from one C call: s2i_plan_create walks the captured hipGraph_t in
 * dependency order and keeps every node's function, geometry and argument pointers; s2i_plan_replay issues them as plain
 * launches on the given stream.  The caller keeps the captured graph (the argument storage belongs to it) and the memory
 * pool the capture allocated from alive for as long as the plan is used.  Only kernel, 1-D memset and memcpy nodes
 * are accepted; anything else fails with a message (the caller then falls back to the eager step).
 * counts, if not NULL, receives [kernels, memsets, memcpys]. */
int s2i_plan_create(void* hip_graph, void** plan_out, int* counts);
int s2i_plan_replay(void* plan, void* stream);
int s2i_plan_destroy(void* plan);

/* ---- Inception-v3 scorer (StackGAN_v2/model.py:17-109, trainer.py:217-232, 563-565) ------------------------------------
 * Forward only, fp32, eval-mode BatchNorm folded into the convolutions (speech_to_image_translation_without_text_amd/
 * inception.py).  Unlike the kinds above, spatial extents, channel counts and kernel geometry are arbitrary. */
typedef struct s2i_conv2d_desc {
  int B, H, W;   /* batch and extent of the NHWC input x                                        */
  int C;         /* input channels                                                              */
  int ldx;       /* floats between consecutive pixels of x (>= C; 0 = C)                         */
  int N;         /* output channels                                                             */
  int kh, kw;    /* kernel extent                                                               */
  int sh, sw;    /* stride                                                                      */
  int ph, pw;    /* zero padding                                                                */
  int Ho, Wo;    /* output extent: (H + 2 ph - kh) / sh + 1 and (W + 2 pw - kw) / sw + 1          */
  int ldy;       /* floats between consecutive pixels of y (>= coff + N)                         */
  int coff;      /* first channel of y written: channels outside [coff, coff + N) stay untouched */
  int relu;      /* epilogue: y = relu(acc + bias) when 1, acc + bias when 0                      */
  int tile;      /* block tile: 0 = the planner chooses; 1 = 128 x 128, 2 = 128 x 64, 3 = 64 x 64 (rows x channels) */
} s2i_conv2d_desc;

/* the block tile the planner uses for d (1..3, see `tile`), or -1 with s2i_last_error() set for a bad descriptor */
int    s2i_conv2d_plan(const s2i_conv2d_desc* d);
/* floats of the packed weight the forward reads: P[(ky * kw + kx) * C + c][Np], Np = N rounded up to 4, the columns
   [N, Np) zero; 0 for a bad descriptor */
size_t s2i_conv2d_weight_elems(const s2i_conv2d_desc* d);
/* y[p][coff + n] = act( sum_{ky,kx,c} x[b, oy*sh - ph + ky, ox*sw - pw + kx, c] * P[(ky*kw + kx)*C + c][n] + bias[n] )
   (bias may be NULL).  Implicit GEMM on v_mfma_f32_32x32x2_f32; the output can be a channel slice of a wider tensor,
   which makes the torch.cat of an Inception block free.  Replaces BasicConv2d (conv + BatchNorm(eps 1e-3) + ReLU, eval)
   and the final fc of torchvision's Inception3. */
int s2i_conv2d_forward(const s2i_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y,
                       void* stream);

/* pools of Inception3 on NHWC fp32 (x pixel stride ldx, y pixel stride ldy, written at channel offset coff) */
#define S2I_POOL_MAX3S2  0  /* F.max_pool2d(kernel_size=3, stride=2): output (H - 3) / 2 + 1                  */
#define S2I_POOL_AVG3S1  1  /* F.avg_pool2d(kernel_size=3, stride=1, padding=1), count_include_pad: output H x W */
#define S2I_POOL_GLOBAL  2  /* mean over the whole H x W map (avg_pool2d(kernel_size=8) on 8 x 8): output 1 x 1  */
int s2i_pool2d(int mode, const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy, int coff,
               void* stream);

/* INCEPTION_V3.forward's input stage (model.py:93-104) in one pass: x*0.5 + 0.5, ImageNet mean / std per channel,
   bilinear resize (align_corners=False) to S x S, NHWC out with Cy = 3 or 4 channels (the 4th written as zero).
   img is a 3-channel image addressed by element strides (sb, sc, sh, sw): an NCHW tensor or an NCHW view of NHWC
   storage alike. */
int s2i_inception_prep(const float* img, int B, int Hin, int Win, long long sb, long long sc, long long sh,
                       long long sw, float* y, int S, int Cy, void* stream);

/* nn.Softmax(dim=1) of `rows` rows of `cols` logits (row strides ldx, ldy) */
int s2i_softmax_rows(const float* x, int rows, int cols, int ldx, float* y, int ldy, void* stream);

/* ---- BVLC GoogLeNet image features (Audio_to_Image/prepare_image_feature.py:86-118, deploy net up to pool5/7x7_s1) ---
 * Forward only, fp32, NHWC (speech_to_image_translation_without_text_amd/googlenet.py).  The convolutions are
 * s2i_conv2d_forward; the pieces below are what it cannot do. */
/* get_one_image_feature's input stage (prepare_image_feature.py:88-93 with load_net_transformer's Transformer,
   :100-116): image b is the uint8 RGB HWC array img[offsets[b] .. offsets[b] + 3 hs[b] ws[b]) (offsets, hs, ws are
   DEVICE arrays; nbytes is the size of img).  Bilinear resize to 227 x 227 with half-pixel centres (edge-clamped when
   a side grows), RGB -> BGR, minus the BGR mean, then the ten 224 x 224 views: crops at (x0, y0) = (0,0), (3,0),
   (1,1), (0,3), (3,3), then the same five of the up-down flipped image (np.fliplr of the CHW array reverses rows).
   y is [B * 10][224][224][4] fp32, view-major per image, the 4th channel zero. */
int s2i_googlenet_prep(const unsigned char* img, long long nbytes, const long long* offsets, const int* hs,
                       const int* ws, int B, float mean_b, float mean_g, float mean_r, float* y, void* stream);
/* Caffe MAX pooling, kernel 3, stride 1 or 2, pad 0 or 1, the ceil output rule (F.max_pool2d(..., ceil_mode=True)):
   GoogLeNet's pool3/3x3_s2, pool4/3x3_s2 (stride 2, pad 0) and every inception/pool (stride 1, pad 1).  NHWC, x pixel
   stride ldx, y pixel stride ldy, written at channel offset coff. */
int s2i_maxpool3(const float* x, int B, int H, int W, int C, int ldx, int stride, int pad, float* y, int ldy, int coff,
                 void* stream);
/* LRN (ACROSS_CHANNELS: y = x (k + alpha / size * sum of x^2 over channels c - size/2 .. c + size/2, zero padded)^-beta)
   fused with the adjacent 3x3 stride-2 ceil max pool, in one launch:
   S2I_POOL_THEN_LRN is pool1/3x3_s2 -> pool1/norm1, S2I_LRN_THEN_POOL is conv2/norm2 -> pool2/3x3_s2.  size odd, <= 9. */
#define S2I_POOL_THEN_LRN 0
#define S2I_LRN_THEN_POOL 1
int s2i_lrn_maxpool3(int order, const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy, int coff,
                     int size, float alpha, float beta, float k, void* stream);

/* ---- speech front end: WAV samples -> log-mel (Audio_to_Image/utils.py:292-340, load_one_audio_file) ---------------
 * sr 16 kHz, n_fft = win_length = 400, hop 160, symmetric Hamming window, center=True with reflect padding, 40 Slaney mel
 * bands from 20 Hz, power_to_db(ref=np.max, amin=1e-10, top_db=80), 0 dB fill (or truncation) to T frames.
 * A batch is a ragged flat fp32 sample buffer: utterance b is x[offsets[b] .. offsets[b] + lens[b]), lens[b] >= 1 (the
 * reference turns an empty file into 200 zeros; the caller does the same); it has n_frames = 1 + lens[b] / 160 frames.
 * The sequence is s2i_signal_mean, s2i_logmel_power, s2i_logmel_finish on one stream; the caller owns every buffer. */
#define S2I_LOGMEL_NFFT          400
#define S2I_LOGMEL_HOP           160
#define S2I_LOGMEL_NMEL          40
#define S2I_LOGMEL_TILE_FRAMES   64  /* frames per entry of the tile table                                        */
#define S2I_LOGMEL_BFT           0   /* logmel_finish layout: (B, 40, T), the reference's array                   */
#define S2I_LOGMEL_NHWC          1   /* logmel_finish layout: [B][1][T][40], the layout CNNRNN computes in          */

/* floats of the packed DFT basis (400 x 416, window folded in; 16-byte aligned).  Column pair q of 16-wide pair tile
   t = q / 16 has a cos column (N-tile 2t) and a sin column (N-tile 2t + 1): (w_n cos(2 pi n q / 400),
   -w_n sin(2 pi n q / 400)) for q = 1..199, (w_n, w_n cos(pi n)) for q = 0 (bins 0 and 200), zero for q = 200..207.
   Element (n, column c of N-tile nt) is stored at ((n / 16 * 26 + nt) * 64 + (n % 4) * 16 + c) * 4 + (n % 16) / 4. */
size_t s2i_logmel_basis_elems(void);
/* mean[b] = mean of utterance b (y - y.mean(), utils.py:318); also sets maxbits[b] = 0 for s2i_logmel_power */
int s2i_signal_mean(const float* x, const long long* offsets, const int* lens, int B, float* mean, unsigned* maxbits,
                    void* stream);
/* Mel power of every frame (utils.py:319-327: pre-emphasis, librosa.stft, |.|^2, mel_basis . spec).  tiles [ntiles][2]
   holds (b, first frame) for every 64-frame tile of every utterance; melbank [40][201] is the fp32 mel filter bank and
   mel_range [40][2] each filter's nonzero bin range [lo, hi).  melpow [B][T][40] receives frames < T; maxbits[b]
   receives the bits of the largest mel power over ALL frames of utterance b (power_to_db's ref). */
int s2i_logmel_power(const float* x, const long long* offsets, const int* lens, int B, const float* mean,
                     const float* basis, const float* melbank, const int* mel_range, const int* tiles, int ntiles,
                     int T, float* melpow, unsigned* maxbits, void* stream);
/* power_to_db(ref=max, top_db=80) and the 0 dB fill to T (utils.py:328-338) into `out` in S2I_LOGMEL_BFT or
   S2I_LOGMEL_NHWC layout */
int s2i_logmel_finish(const float* melpow, const unsigned* maxbits, const int* lens, int B, int T, int layout,
                      float* out, void* stream);
/* A batch out of kept log-mel rows: the padding / truncation to T of load_one_audio_file (utils.py:329-340) applied to
   rows s2i_logmel_finish made earlier.  pool [rows][40] fp32 holds the kept rows of every utterance of a split back to
   back; out is S2I_LOGMEL_NHWC [B][1][T][40].  out[b][0][t][:] = pool[row_offsets[b] + t][:] for t < frames[b] and 0.0f
   (0 dB, the fill of s2i_logmel_finish) for frames[b] <= t < T; frames[b] is in [0, T] (values outside are clamped),
   and a negative row offset (an utterance that is not stored) gives an all-fill utterance.  pool and out are 16-byte
   aligned; the rows move as 16-byte pieces addressed in 64 bits, so a pool may hold more than 2^31 floats.  One
   launch, no workspace. */
int s2i_logmel_gather(const float* pool, const long long* row_offsets, const int* frames, int B, int T, float* out,
                      void* stream);

/* ---- any WAV -> 16 kHz mono fp32 (Audio_to_Image/utils.py:313, librosa.load(path, 16000)) ---------------------------
 * Decode, mixdown and band-limited resampling (resampy's kaiser_best, which librosa.load of the reference's era calls) of
 * one group of clips that share (rate, sample format, channel count), in one launch, in front of the log-mel entries.
 * With g = gcd(16000, rate): L = 16000 / g, M = rate / g, scale = min(1, L / M), W = ceil(64 / scale), taps = 2 W + 2 and
 *   table[p][j] = scale h(scale (W - j + p / L)),  h(t) = r sinc(r t) I0(beta sqrt(1 - (t / 64)^2)) / I0(beta) on |t| <= 64,
 * r = 0.9475937167399596, beta = 14.769656459379492, built in float64 and rounded to fp32 once by the caller.  Output m of
 * a clip of n frames: q = (m M) div L, p = (m M) mod L (64-bit), y[m] = sum_j x[q - W + j] table[p][j] with x = 0 outside
 * [0, n); n_out = ceil(n L / M) outputs, those with m >= floor(n L / M) are 0.0f.  rate 16000 is L = M = 1, W = 0, table
 * [1, 0].  Decode (little-endian, interleaved): u8 (v - 128) / 128; s16 / s24 / s32 float(v) 2^-(bits - 1); f32 as is; f64
 * rounded to fp32.  Mono: channels added in channel order in fp32, then a correctly rounded division by float(channels).
 * Decode, then mono, then resample. */
#define S2I_PCM_U8   0
#define S2I_PCM_S16  1
#define S2I_PCM_S24  2
#define S2I_PCM_S32  3
#define S2I_PCM_F32  4
#define S2I_PCM_F64  5
#define S2I_RESAMPLE_TILE        1024   /* outputs per entry of the tile table                                        */
#define S2I_RESAMPLE_MAX_WINDOW  13826  /* 12 * 1024 + 2 * 768 + 2 floats of LDS: a tile's input window at 192 kHz     */
/* raw: the byte buffer (16-byte aligned); clip b's `data` bytes start at raw + byte_offsets[b], a multiple of 16, and
   hold in_frames[b] frames of `channels` samples of `format`.  table is the device table in the layout
   [L][tpad], tpad = taps rounded up to a multiple of 4, pad zero (each phase's row 16-byte aligned; the pad is not
   read).  tiles [ntiles][2] holds (clip, first output index) for every 1024 outputs of every clip with out_lens > 0.
   Clip b's out_lens[b] = ceil(in_frames[b] L / M) outputs go to out + out_offsets[b]; every one of them is written and
   nothing else is.  Refused before any launch: null pointers, B < 1, an unknown format, channels outside [1, 8], L / M
   that is not the reduced ratio of 16000 to a rate in [4000, 192000] (L in [1, 16000], L / 4 <= M <= 12 L, gcd 1), W
   outside [0, 768] or a table over 2^24 floats, a tile window over S2I_RESAMPLE_MAX_WINDOW, raw, table or out off a
   16-byte boundary.  W is otherwise the caller's (the section's value for a real rate; tests pass others with their own
   tables).  One launch, dynamic LDS only; no atomics, no workspace, no synchronisation. */
int s2i_pcm_resample(const void* raw, const long long* byte_offsets, const int* in_frames, int B, int format,
                     int channels, int L, int M, int W, const float* table, const int* tiles, int ntiles, float* out,
                     const long long* out_offsets, const int* out_lens, void* stream);

/* ---- streaming feature moments for the Frechet distance (StackGAN_v2/trainer.py:103-144) -----------------------------
 * compute_frethet_distance fits a Gaussian to each set of Inception pool3 rows with np.mean and np.cov.  Both follow
 * from the row count, the column sums and the Gram matrix X^T X, which add up exactly across chunks of rows, so the
 * rows can be scored chunk by chunk and dropped (speech_to_image_translation_without_text_amd/gan_metrics.py). */
/* colsum[D] += sum over r of x_r and gram[D][D] += X^T X for the fp32 rows x_r = x + r ldx (r < rows, ldx >= D), both
   fp64 on the device, in place.  Products are exact (fp32 -> fp64, v_mfma_f64_16x16x4_f64); the sums are fp64 in a
   fixed order, so a result is bit-identical from run to run.  Only the 64 x 64 tiles of gram on or above the diagonal
   are written (a diagonal tile in full): the entries below the diagonal tiles keep whatever they held, and a reader
   mirrors the upper triangle.  rows = 0 is a no-op.  No atomics, no workspace, no synchronisation. */
int s2i_moments_accumulate(const float* x, int rows, int D, long long ldx, double* colsum, double* gram, void* stream);

/* ---- nearest-row search: the k best of every score row, chunk by chunk --------------------------------------------
 * A gallery is scored a chunk of rows at a time with the fp32 1x1 matrix kernel; this folds each [Q, chunk] block of
 * scores into a running [Q][k] result, so the [Q, N] matrix of the whole gallery never exists
 * (speech_to_image_translation_without_text_amd/retrieval.py, Gallery). */
/* For every query row q: the k best of scores[q][0..N) (row stride lds floats), row id = base + j, merged with the k
 * entries already in best_score / best_row [Q][k] when merge != 0 (otherwise those are overwritten).
 * Order: score descending; equal scores by ascending row id; NaN ranks as -inf.  Output rows are sorted in that order;
 * slots beyond the number of candidates hold (-inf, -1).  1 <= k <= 64, N <= 2^30.  No arithmetic on the scores:
 * bit-exact.  One block per query; no atomics, no workspace, no synchronisation. */
int s2i_topk_rows(const float* scores, int Q, int N, int lds, int base, int k, float* best_score, int* best_row,
                  int merge, void* stream);

/* ---- the rank of one candidate among the candidates of other classes, chunk by chunk --------------------------------
 * The speech-image consistency score (R-precision and recall@k of generated images against the test utterances;
 * retrieval.Gallery.rank, gan_metrics.ConsistencyScorer) needs, for every query, how many gallery rows of OTHER classes
 * score above its own designated row.  That rank can be in the thousands, so a top k does not give it; like
 * s2i_topk_rows this folds one [Q, N] block of scores (row stride lds floats, column j = gallery row base + j) at a
 * time, and the [Q, rows] matrix never exists. */
#define S2I_RANK_GATHER 0
#define S2I_RANK_COUNT 1
/* mode S2I_RANK_GATHER: for every q with base <= own_row[q] < base + N, own_score[q] = scores[q][own_row[q] - base]
 *   (the bits, a NaN included); every other q, own_row[q] = -1 ("no own row") among them, is left untouched.  Reads
 *   scores and own_row, writes own_score; query_label, row_label, gt and eq are not touched and may be null.
 * mode S2I_RANK_COUNT: for every q, over the columns j whose row_label[base + j] != query_label[q]:
 *   gt[q] += #{j : scores[q][j] > own_score[q]},  eq[q] += #{j : scores[q][j] == own_score[q]}   (float comparisons).
 *   A NaN score counts in neither.  A NaN own_score[q] makes EVERY column of another class count in gt (a NaN one too),
 *   so that query ranks last.  Rows of the query's own class are never counted, its own row included.  own_row is not
 *   read.  gt and eq are int32 [Q], accumulated in place across chunks; the caller zeroes them.
 * row_label is int32 over the whole gallery (n_labels entries, indexed by global row: base + N <= n_labels);
 * query_label and own_row are int32 [Q].  N <= 2^30, base + N <= INT_MAX.  Any row stride lds >= N, base and pointer
 * are taken (16-byte loads where the addresses allow, single loads before and after).  No arithmetic on the scores,
 * integer counters: exact, and identical from run to run.  One block per query when counting; no atomics, no
 * workspace, no synchronisation. */
int s2i_rank_rows(const float* scores, int Q, int N, int lds, int base, const int* own_row, const int* query_label,
                  const int* row_label, int n_labels, float* own_score, int* gt, int* eq, int mode, void* stream);

/* ---- kernel inception distance and k-nearest-neighbour manifolds, chunk by chunk --------------------------------------
 * KID (the unbiased MMD^2 with the cubic polynomial kernel) and precision / recall / density / coverage compare every
 * row of one set of Inception pool3 rows with every row of another (gan_metrics.kid, gan_metrics.prdc).  Like
 * s2i_topk_rows and s2i_rank_rows the three folds below take one [Q, N] block of scores at a time, exactly as
 * ops.score_rows writes it (fp32, row stride lds >= N floats, column j = row base + j of the other set), so the
 * [rows, rows] matrix never exists.  Common to the three: Q >= 1, 1 <= N <= 2^30, base >= 0, base + N <= INT_MAX; any
 * row stride, base and pointer are taken (16-byte loads where the addresses allow, single loads before and after); one
 * block per query; no atomics, no workspace, no allocation, no synchronisation, no environment reads; bad arguments
 * return non-zero before any launch. */
/* sum[q] += sum over j of k(q, j),  k = t * t * t,  t = (double)scores[q][j] * inv_d + 1.0, every operation rounded on
 * its own in fp64 (no contraction).  When own_base >= 0 the column j with base + j == own_base + q is left out: the
 * off-diagonal sum of a set against itself (query q is row own_base + q of that set); own_base = -1 leaves nothing out.
 * The sum runs in a fixed order (lane accumulators, a wave butterfly, the waves in order through LDS), so the same
 * inputs and geometry give the same bits from run to run; against another order it differs by at most
 * N 2^-52 sum_j |k|.  sum is fp64 [Q], accumulated in place across chunks; the caller zeroes it. */
int s2i_polykernel_rows(const float* scores, int Q, int N, int lds, int base, int own_base, double inv_d, double* sum,
                        void* stream);
/* Rewrites the block in place to the negated squared distance,
 *   scores[q][j] = -fmaxf(0.f, (q_norm2[q] + row_norm2[base + j]) - 2.f * scores[q][j]),
 * in fp32, evaluated as written (2 s is exact, so contracting the subtraction into an FMA changes nothing: an fp32
 * restatement on the host reproduces the bits).  A NaN stays a NaN.  The own row (base + j == own_base + q, own_base >= 0;
 * -1: none) becomes -inf.  Negated, so that s2i_topk_rows, which takes the largest, finds the nearest rows as it is.
 * q_norm2 is fp32 [Q]; row_norm2 is fp32 over the whole other set (n_rows entries, indexed by global row:
 * base + N <= n_rows). */
int s2i_sqdist_rows(float* scores, int Q, int N, int lds, int base, int own_base, const float* q_norm2,
                    const float* row_norm2, int n_rows, void* stream);
/* Compare-only fold of a block s2i_sqdist_rows has rewritten (nd = negated squared distances):
 *   count[q] += #{j : nd[q][j] >= row_bound[base + j]}   (int32: the balls of the other set that hold query q),
 *   best[q] = max(best[q], max over j of nd[q][j])        (fp32: minus the squared distance to the nearest row).
 * row_bound[r] is -radius_r^2, column k - 1 of the top k of the other set against itself, used as it comes; it is fp32
 * over the whole other set (n_rows entries: base + N <= n_rows).  A NaN entry counts nowhere and never becomes best; a NaN
 * bound counts nothing.  The caller zeroes count and sets best to -inf; either of the two may be null, not both.
 * Integer counters and comparisons only: exact, whatever the division of a row among lanes, waves or chunks. */
int s2i_ball_rows(const float* nd, int Q, int N, int lds, int base, const float* row_bound, int n_rows, int* count,
                  float* best, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S2I_HIP_H */
