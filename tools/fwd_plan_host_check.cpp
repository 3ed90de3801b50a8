// Stand-alone host check of the forward planner: s2i_conv_plan_query and the three queries beside it over a few hundred
// descriptors, refused ones included, built with the host sanitizers.  It links the two host-side units the planner needs
// and never touches a device, so it runs anywhere the compiler does:
//
//   cd speech_to_image_translation_without_text_amd/csrc
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         ../../tools/fwd_plan_host_check.cpp s2i_conv_plan.hip s2i_runtime.hip -o /tmp/fwd_plan_host_check && /tmp/fwd_plan_host_check
//
// tests/test_fwd_plan_cpu.py builds and runs it the same way.  Besides what the sanitizers see, it checks that every reported
// kernel id indexes the kernel table (rows, columns and threads come back non-zero), that a refusal zeroes the output, and that
// no mode's plan asks for more workspace than s2i_conv_workspace_bytes reports.
#include <stdio.h>
#include <string.h>
#include "../include/s2i_hip.h"

static const int kKernels = 30;   // FWD_KERNEL_COUNT of csrc/s2i_igemm.h

int main() {
  static const int kinds[] = {S2I_CONV_K1, S2I_CONV_K3S1, S2I_CONV_K4S2, S2I_TCONV_K4S2, S2I_CONV_1D, 7};
  static const int batches[] = {0, 1, 9, 65, 144}, extents[] = {1, 6, 8, 64}, cxs[] = {0, 4, 6, 16, 32, 64, 136}, ns[] = {3, 4, 16, 32, 64, 136};
  long asked = 0, planned = 0, refused = 0;
  int seen[kKernels] = {0};
  for (int kind : kinds) for (int B : batches) for (int HW : extents) for (int Cx : cxs) for (int N : ns)
    for (int variant = 0; variant < 6; ++variant) {
      s2i_conv_desc d;
      memset(&d, 0, sizeof d);
      d.kind = kind; d.B = B; d.H = HW; d.W = variant == 5 ? 2 * HW : HW; d.Cx = Cx; d.N = N;
      d.Cc = variant == 1 ? 32 : 0;
      d.wmode = variant == 2;
      d.wR = d.wmode ? N : Cx + d.Cc; d.ldw = d.wmode ? Cx + d.Cc : (N + 3) & ~3;
      d.ldy = N == 3 ? 4 : N;
      d.stats = variant == 3; d.groups = variant == 3 ? 3 : 1;
      d.nosplit = variant == 4;
      d.in_act = variant == 4 ? S2I_ACT_LRELU : 0; d.in_groups = 1;
      d.kw = 5; d.stride = 1; d.pad = 2;
      d.tile_rows = variant == 2 ? 96 : 0;
      const size_t ws = s2i_conv_workspace_bytes(&d);
      const int parts = s2i_conv_stat_parts(&d), eligible = s2i_conv_split_eligible(&d);
      for (int mode = 0; mode < 24; ++mode) {
        const int x16 = mode & 1, y16 = (mode >> 1) & 1, bias = (mode >> 2) & 1, planes = mode >= 16 ? 3 : (mode >= 8 ? 1 : 0);
        int out[15];
        for (int& v : out) v = -1;
        const int rc = s2i_conv_plan_query(&d, x16, y16, planes, bias, mode == 7, out);
        ++asked;
        if (rc) {
          ++refused;
          for (int v : out)
            if (v != 0) { fprintf(stderr, "a refused query left %d in its output\n", v); return 1; }
          if (!s2i_last_error()[0]) { fprintf(stderr, "a refusal without an error text\n"); return 1; }
          continue;
        }
        ++planned;
        if (parts < 0 || (planes && !eligible)) { fprintf(stderr, "planned what the descriptor queries refuse (kind %d)\n", kind); return 1; }
        if (out[0] < 0 || out[0] >= kKernels || out[1] <= 0 || out[2] <= 0 || out[3] <= 0 || out[4] <= 0 || out[5] <= 0 || out[6] <= 0) {
          fprintf(stderr, "kernel %d: rows %d cols %d threads %d grid %d x %d x %d\n", out[0], out[1], out[2], out[3], out[4], out[5], out[6]);
          return 1;
        }
        if ((size_t)out[12] > ws) { fprintf(stderr, "kernel %d asks for %d bytes, the query reports %zu\n", out[0], out[12], ws); return 1; }
        seen[out[0]] = 1;
      }
    }
  int kinds_seen = 0;
  for (int v : seen) kinds_seen += v;
  printf("fwd_plan_host_check: %ld queries, %ld planned onto %d kernels, %ld refused\n", asked, planned, kinds_seen, refused);
  return planned > 1000 && refused > 1000 ? 0 : 1;
}
