// The 96 x 128 tile of igemm_fwd_kernel (s2i_conv_fwd.h): its four WT / CA32 forms and the apply-on-load form, waves 1 x 4.
#include "s2i_conv_fwd.h"

void launch_fwd_96x128(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  launch_fwd<96, 128, 1, 4>(pl, p, grid, st);
}
