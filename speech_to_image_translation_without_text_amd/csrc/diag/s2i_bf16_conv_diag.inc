// Diagnostic launches of conv_bf16_kernel (libs2i_hip_diag.so only, see s2i_bf16_diag.inc).
#include "s2i_bf16_diag.inc"

// returns true when it launched (or failed: *rc != 0), false to fall through to the production dispatch
static bool diag_launch_conv_bf16(const BPlan& pl, const ConvBP& p, dim3 grid, hipStream_t st, int* rc) {
  if (pl.kernel == B16_K4S2_128x16 && pl.TG == 8) {
#define S2I_DBG(v) if (p.dbg == v) { diag_launch(conv_bf16_kernel<KB_K4S2, 128, 16, 8, v>, 96 * 1024, pl.threads, pl.smem, p, grid, st, false, rc); return true; }
    S2I_DBG(1) S2I_DBG(2) S2I_DBG(4) S2I_DBG(7) S2I_DBG(8) S2I_DBG(15) S2I_DBG(16) S2I_DBG(31) S2I_DBG(24)
#undef S2I_DBG
  }
  if (p.dbg == 32 && pl.kernel == B16_K4S2_128x32 && pl.TG == 4 && p.splitk == 1) {
    diag_launch(conv_bf16_kernel<KB_K4S2, 128, 32, 4, 32>, 96 * 1024, pl.threads, pl.smem, p, grid, st, true, rc);
    return true;
  }
  return false;
}
