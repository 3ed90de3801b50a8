// The 128 x 64 tile of igemm_fwd_kernel (s2i_conv_fwd.h): its four WT / CA32 forms and the apply-on-load form, waves 2 x 2.
#include "s2i_conv_fwd.h"

void launch_fwd_128x64(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  launch_fwd<128, 64, 2, 2>(pl, p, grid, st);
}
