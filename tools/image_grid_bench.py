"""Time of one ops.image_grid_uint8 call (reduction + composition launches) on a snapshot-sized batch (dev tool, GPU box
only).  usage: python tools/image_grid_bench.py [images] [size]"""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import ops

ops._lib_ready()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 24
S = int(sys.argv[2]) if len(sys.argv) > 2 else 256
dev = torch.device("cuda:0")
x = torch.tanh(torch.randn(N, S, S, 4, device=dev))          # the generator's NHWC4 image tensor


def timeit(fn, reps=200):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


t = [timeit(lambda: ops.image_grid_uint8(x, nrow=8, padding=2, layout="nhwc")) for _ in range(5)]
g = ops.image_grid_uint8(x, nrow=8, padding=2, layout="nhwc")
moved = 2 * x.numel() * 4 + g.numel()                         # the batch is read twice (all four channels' lines), the grid written once
print("image_grid_uint8 %d x %d x %d NHWC4 -> %s: median %.1f us per call (5 windows of 200 calls: %s), %.2f TB/s of %d bytes"
      % (N, S, S, tuple(g.shape), sorted(t)[2], " ".join("%.1f" % v for v in t), moved / sorted(t)[2] / 1e6, moved))
