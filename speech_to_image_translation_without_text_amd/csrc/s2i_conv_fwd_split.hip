// The split-bf16 tiles of igemm_fwd_split_kernel (s2i_conv_fwd.h): 128 x 128, 128 x 64 and 128 x 32, each with 1 - 3 planes.
#include "s2i_conv_fwd.h"

void launch_fwd_split(const FwdPlan& pl, const IgemmP& p, dim3 grid, hipStream_t st) {
  switch (pl.kernel) {
    case FWD_SPLIT_128x128: launch_split<128, 128, 2, 2>(pl, p, grid, st); break;
    case FWD_SPLIT_128x64: launch_split<128, 64, 2, 2>(pl, p, grid, st); break;
    case FWD_SPLIT_128x32: launch_split<128, 32, 4, 1>(pl, p, grid, st); break;
    default: break;   // launch_igemm_fwd sends nothing else here
  }
}
