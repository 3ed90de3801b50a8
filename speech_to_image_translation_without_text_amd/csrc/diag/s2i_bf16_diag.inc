// Diagnostic launches of the bf16 convolution kernels: compile-time ablations (DBG bits 1..16) and the in-kernel
// s_memtime timeline (DBG 32) of tools/conv16_bench.py / tools/conv16_timeline.py.  Compiled ONLY into
// libs2i_hip_diag.so (`make diag`, -DS2I_DIAG): this code allocates, synchronises and copies, which the product
// library (include/s2i_hip.h: "nothing here allocates, frees or synchronises") never does.
// Knobs (s2i_set_tuning): b16_dbg = DBG value; the timeline of a DBG-32 launch is written to the path in $S2I_B16_TIMELINE.
// This part is shared: s2i_bf16_conv_diag.inc and s2i_bf16_conv_v2_diag.inc hold the instantiations of their kernel.
#include <stdlib.h>
#include <vector>

// launches a DBG instantiation; timeline (DBG 32): its p.slab points at 64 stamps per block, which are then dumped
template <class Kernel>
static void diag_launch(Kernel kernel, int lds_max, int threads, size_t shb, ConvBP p, dim3 grid, hipStream_t st, bool timeline,
                        int* rc) {
  const size_t nblk = (size_t)grid.x * grid.y * grid.z, bytes = nblk * 64 * sizeof(unsigned long long);
  unsigned long long* dbuf = nullptr;
  if (timeline) {
    if (hipMalloc((void**)&dbuf, bytes) != hipSuccess) { s2i_set_error("conv(bf16): timeline buffer"); *rc = 1; return; }
    (void)hipMemsetAsync(dbuf, 0, bytes, st);
    p.slab = reinterpret_cast<float*>(dbuf);
  }
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  hipLaunchKernelGGL(kernel, grid, dim3(threads), shb, st, p);
  if (!timeline) return;
  (void)hipStreamSynchronize(st);
  const char* path = getenv("S2I_B16_TIMELINE");
  if (path) {
    std::vector<unsigned long long> h(nblk * 64);
    (void)hipMemcpy(h.data(), dbuf, bytes, hipMemcpyDeviceToHost);
    FILE* f = fopen(path, "wb");
    if (f) { fwrite(h.data(), 1, bytes, f); fclose(f); }
  }
  (void)hipFree(dbuf);
}
