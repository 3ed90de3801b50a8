// The 128 x 128 tile of igemm_fwd_kernel (s2i_conv_fwd.h): its four WT / CA32 forms and the apply-on-load form, waves 2 x 2.
#include "s2i_conv_fwd.h"

void launch_fwd_128x128(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  launch_fwd<128, 128, 2, 2>(pl, p, grid, st);
}
