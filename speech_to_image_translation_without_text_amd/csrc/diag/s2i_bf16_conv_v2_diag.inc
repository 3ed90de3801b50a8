// Diagnostic launches of conv_bf16_v2_kernel (libs2i_hip_diag.so only, see s2i_bf16_diag.inc).
#include "s2i_bf16_diag.inc"

// returns true when it launched (or failed: *rc != 0), false to fall through to the production dispatch
static bool diag_launch_conv_bf16_v2(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st, int* rc) {
  if (p.dbg != 32 || pl.kb != KB_K4S2 || p.splitk != 1) return false;
  if (pl.kernel == B16_V2_K4S2_PW66)
    diag_launch(conv_bf16_v2_kernel<KB_K4S2, 32, 4, false, 32, 66>, 160 * 1024, pl.threads, pl.smem, p, grid, st, true, rc);
  else diag_launch(conv_bf16_v2_kernel<KB_K4S2, 32, 4, false, 32>, 160 * 1024, pl.threads, pl.smem, p, grid, st, true, rc);
  return true;
}
