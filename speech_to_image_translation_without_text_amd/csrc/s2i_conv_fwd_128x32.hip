// The 128 x 32 tile of igemm_fwd_kernel (s2i_conv_fwd.h): its four WT / CA32 forms and the apply-on-load form, waves 4 x 1.
#include "s2i_conv_fwd.h"

void launch_fwd_128x32(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  launch_fwd<128, 32, 4, 1>(pl, p, grid, st);
}
