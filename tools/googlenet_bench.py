"""GoogLeNet feature extractor timing (GPU box only): the full forward over 48 seeded 500 x 375 images (480 views); every
convolution of it alone, grouped by class (TFLOP/s against the 157.3 TFLOP/s fp32 matrix peak of the MI355X); the input
kernel and the two fused LRN + pool kernels (GB/s of compulsory traffic against 6.3 TB/s achievable HBM bandwidth); and
end-to-end images/s of extract_image_feature.extract_paths, PIL decoding of synthetic JPEGs included.  Seeded He-scaled
weights (the timing does not depend on them).  FLOPs come from the architecture table.

Usage:  python tools/googlenet_bench.py [--images 48] [--reps 10] [--files 480]
"""
import argparse
import collections
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from speech_to_image_translation_without_text_amd import _lib, extract_image_feature as X, googlenet as G  # noqa: E402
from googlenet_ref import random_weights  # noqa: E402

PEAK_TF = 157.3
HBM_GBS = 6300.0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def conv_class(name, k):
    return "7x7" if k == 7 else "%dx%d" % (k, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--files", type=int, default=480, help="synthetic JPEGs for the end-to-end rate")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.require_device()
    net = G.GoogLeNetFeatures(random_weights(0), dev)
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (375, 500, 3)).astype(np.uint8) for _ in range(args.images)]
    B, V = len(imgs), 10 * len(imgs)
    full_ms = timed(lambda: net(imgs), args.reps)

    # the input kernel
    x = torch.empty(V, G.VIEW, G.VIEW, 4, device=dev)
    keep = net.prep(imgs, x)
    prep_ms = timed(lambda: net.prep(imgs, x), args.reps)
    del keep
    prep_bytes = sum(im.size for im in imgs) + x.numel() * 4

    # the two LRN + pool pairs at their production shapes
    c1 = torch.relu(torch.randn(V, 112, 112, 64, device=dev) * 40)
    c2 = torch.relu(torch.randn(V, 56, 56, 192, device=dev) * 40)
    lp1_ms = timed(lambda: net.lrn_pool(_lib.POOL_THEN_LRN, c1, V, 112), args.reps)
    lp2_ms = timed(lambda: net.lrn_pool(_lib.LRN_THEN_POOL, c2, V, 56), args.reps)
    lp1_bytes = (c1.numel() + V * 56 * 56 * 64) * 4
    lp2_bytes = (c2.numel() + V * 28 * 28 * 192) * 4
    del c1, c2

    # every convolution alone, at its production shape (input of the right width, output of its own)
    groups = collections.OrderedDict()
    for name, (cin, cout, k, s, p) in G.architecture().items():
        H = G.VIEW if name == "conv1/7x7_s2" else (G.map_sizes()[1] if name.startswith("conv2") else
                                                   G.layer_extent(name))
        xin = torch.randn(V, H, H, 4 if name == "conv1/7x7_s2" else cin, device=dev)
        ms = timed(lambda: net.conv(name, xin, V, H, H), args.reps)
        Ho = G.layer_extent(name)
        flops = 2.0 * V * Ho * Ho * cout * cin * k * k
        g = groups.setdefault(conv_class(name, k), {"layers": 0, "ms": 0.0, "gflop": 0.0})
        g["layers"] += 1
        g["ms"] += ms
        g["gflop"] += flops / 1e9
        del xin
    for g in groups.values():
        g["tflops"] = round(g["gflop"] / g["ms"], 1)
        g["pct_peak"] = round(100 * g["tflops"] / PEAK_TF, 1)
        g["ms"] = round(g["ms"], 3)
        g["gflop"] = round(g["gflop"], 1)
    conv_ms = sum(g["ms"] for g in groups.values())
    total_flop = V * G.flops_per_view()

    # end to end over synthetic JPEGs
    from PIL import Image
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(args.files):
            p = os.path.join(d, "%d.jpg" % i)
            a = (np.add.outer(np.arange(375), np.arange(500))[:, :, None] * (i % 7 + 1) + rng.integers(0, 40, (375, 500, 3)))
            Image.fromarray((a % 256).astype(np.uint8)).save(p, quality=90)
            paths.append(p)
        X.extract_paths(net, paths[:G.MAX_BATCH])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X.extract_paths(net, paths)
        torch.cuda.synchronize()
        e2e = len(paths) / (time.perf_counter() - t0)

    res = {
        "images": B, "views": V,
        "forward_ms": round(full_ms, 3), "images_per_s_gpu": round(B / full_ms * 1e3, 1),
        "forward_tflops": round(total_flop / full_ms / 1e9, 1),
        "conv_ms_sum": round(conv_ms, 3), "conv_tflops": round(total_flop / conv_ms / 1e9, 1), "conv_classes": groups,
        "prep_ms": round(prep_ms, 3), "prep_gbs": round(prep_bytes / prep_ms / 1e6, 1),
        "pool_lrn_ms": round(lp1_ms, 3), "pool_lrn_gbs": round(lp1_bytes / lp1_ms / 1e6, 1),
        "lrn_pool_ms": round(lp2_ms, 3), "lrn_pool_gbs": round(lp2_bytes / lp2_ms / 1e6, 1),
        "hbm_gbs": HBM_GBS, "peak_tflops": PEAK_TF,
        "e2e_files": len(paths), "e2e_images_per_s": round(e2e, 1),
    }
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
