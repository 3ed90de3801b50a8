// Forward launch of the implicit-GEMM convolutions: conv_forward_impl fills the parameter block of the plan (plan_fwd,
// s2i_conv_plan.hip) and launches it; the s2i_conv_forward* entry points.  The kernels live in the s2i_conv_fwd*.hip
// units and s2i_conv_thin.hip and are reached through the launch_* functions of s2i_igemm.h.
#include "s2i_igemm.h"

static int conv_forward_impl(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                             const unsigned short* wsp, int planes, int np, int kp, const float* bias,
                             const float* cls_bias, float* y, float* part, void* ws, size_t ws_bytes, void* stream,
                             int x16 = 0, int y16 = 0, const float* in_coef = nullptr) {
  FwdMode mode;
  FwdPlan pl;
  if (fwd_mode(x16, y16, wsp ? planes : 0, bias != nullptr, cls_bias != nullptr, in_coef != nullptr, &mode) || plan_fwd(d, mode, &pl))
    return 1;
  S2I_REQUIRE(x != nullptr || d->Cx == 0, "conv: x is null");
  S2I_REQUIRE(d->Cc == 0 || cvec != nullptr, "conv: cvec is null but Cc > 0");
  S2I_REQUIRE((w || wsp) && y, "conv: null weight/output");
  S2I_REQUIRE(!d->stats || part, "conv: stats requested without a partial buffer");
  // the plan never looks at the workspace: a short one is refused, not answered with another kernel
  S2I_REQUIRE(ws_bytes >= pl.ws_bytes && (pl.ws_bytes == 0 || ws), "conv: workspace too small (%zu < %zu bytes; s2i_conv_workspace_bytes)",
              ws_bytes, pl.ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  IgemmP p;
  p.x = x; p.cvec = cvec; p.w = w; p.bias = bias; p.cls_bias = cls_bias; p.y = y; p.part = part; p.slab = (float*)ws;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cx = d->Cx; p.Cc = d->Cc; p.Ca = pl.Ca;
  p.Ho = pl.Ho; p.Wo = pl.Wo; p.lgWo = s2i_ilog2(pl.Wo); p.lgHoWo = s2i_ilog2(pl.Ho * pl.Wo);
  p.M = pl.M; p.N = d->N; p.K = pl.K; p.T = pl.T;
  p.kind = d->kind; p.flip = d->flip; p.act = d->act; p.stats = d->stats;
  p.splitk = pl.splitk; p.cps = pl.cps; p.nchunks = pl.nchunks;
  p.ldw = d->ldw; p.wR = d->wR; p.ldy = d->ldy; p.nparts = pl.gridM * pl.nphases;
  p.g_kw = d->kw; p.g_s = d->stride; p.g_pad = d->pad; p.wt = pl.wt;
  p.Mrows = pl.Mrows;
  p.x16 = x16; p.y16 = y16;
  p.wsp = wsp; p.wsp_np = np; p.wsp_kp = kp; p.wsp_plane = 0; p.wsp_bytes = 0;
  p.in_coef = in_coef; p.in_rows_per_group = in_coef ? pl.M / (d->in_groups < 1 ? 1 : d->in_groups) : pl.M;
  if (pl.kernel >= FWD_TCONV_N4_64) return launch_thin(d, pl, p, ws, st);
  if (pl.kernel >= FWD_SMALLN_4) return launch_small_n_conv(pl, p, st);
  // the matrix families address their tensors through buffer windows
  const int wtaps = d->kind == S2I_TCONV_K4S2 ? 16 : pl.T;
  const unsigned long long xb = (unsigned long long)d->B * d->H * d->W * d->Cx * (x16 ? 2ull : 4ull);
  const unsigned long long wb = (unsigned long long)wtaps * d->wR * d->ldw * 4ull;
  S2I_REQUIRE(xb < 0x7ff00000ull && wb < 0x7ff00000ull, "conv: tensor exceeds the 2 GiB buffer-addressing window");
  p.x_bytes = (unsigned)xb;
  p.c_bytes = (unsigned)((unsigned long long)d->B * d->Cc * 4ull);
  p.w_bytes = (unsigned)wb;
  if (pl.planes) {
    const unsigned long long pe = (unsigned long long)wtaps * np * kp;  // elements per plane
    S2I_REQUIRE(pe * planes * 2ull < 0x7ff00000ull, "conv(split): weight planes exceed the buffer window");
    S2I_REQUIRE(kp >= pl.Ca && np >= d->N, "conv(split): weight planes %d x %d too small for N=%d K=%d", np, kp, d->N, pl.Ca);
    p.wsp_plane = (int)pe;
    p.wsp_bytes = (unsigned)(pe * planes * 2ull);
  }
  if (launch_igemm_fwd(pl, p, st)) return 1;
  return pl.reduce != FWD_REDUCE_NONE ? launch_splitk_reduce(d, pl, bias, y, part, ws, y16, stream) : 0;
}

extern "C" int s2i_conv_forward(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                                const float* bias, float* y, float* part, void* ws, size_t ws_bytes,
                                void* stream) {
  return s2i_conv_forward_cls(d, x, cvec, w, bias, nullptr, y, part, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_forward_cls(const s2i_conv_desc* d, const float* x, const float* cvec, const float* w,
                                    const float* bias, const float* cls_bias, float* y, float* part, void* ws,
                                    size_t ws_bytes, void* stream) {
  S2I_REQUIRE(w != nullptr, "conv: null weight");
  return conv_forward_impl(d, x, cvec, w, nullptr, 0, 0, 0, bias, cls_bias, y, part, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_forward_in(const s2i_conv_desc* d, const float* x_raw, const float* in_coef, const float* w, float* y,
                                   float* part, void* ws, size_t ws_bytes, void* stream) {
  S2I_REQUIRE(w != nullptr && in_coef != nullptr, "conv(apply-on-load): null weight / coefficient table");
  return conv_forward_impl(d, x_raw, nullptr, w, nullptr, 0, 0, 0, nullptr, nullptr, y, part, ws, ws_bytes, stream, 0, 0, in_coef);
}

extern "C" int s2i_conv_forward_split(const s2i_conv_desc* d, const float* x, const float* cvec,
                                      const unsigned short* wsplit, int planes, int np, int kp, const float* bias,
                                      const float* cls_bias, float* y, float* part, void* ws, size_t ws_bytes,
                                      void* stream) {
  S2I_REQUIRE(wsplit != nullptr && planes >= 1 && planes <= 3, "conv(split): need 1 to 3 bf16 planes");
  S2I_REQUIRE(np > 0 && kp > 0 && (kp % 8) == 0, "conv(split): weight rows must be multiples of 8 bf16 (kp=%d)", kp);
  return conv_forward_impl(d, x, cvec, nullptr, wsplit, planes, np, kp, bias, cls_bias, y, part, ws, ws_bytes, stream);
}

extern "C" int s2i_conv_forward_dt(const s2i_conv_desc* d, const void* x, int x_dtype, const float* cvec, const float* w,
                                   const float* bias, const float* cls_bias, void* y, int y_dtype, float* part, void* ws,
                                   size_t ws_bytes, void* stream) {
  S2I_REQUIRE(w != nullptr, "conv: null weight");
  S2I_REQUIRE((x_dtype == S2I_DT_F32 || x_dtype == S2I_DT_BF16) && (y_dtype == S2I_DT_F32 || y_dtype == S2I_DT_BF16),
              "conv: unknown dtype");
  return conv_forward_impl(d, (const float*)x, cvec, w, nullptr, 0, 0, 0, bias, cls_bias, (float*)y, part, ws, ws_bytes,
                           stream, x_dtype == S2I_DT_BF16, y_dtype == S2I_DT_BF16);
}
