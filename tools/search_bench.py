"""Times retrieval.Gallery.search (chunked fp32 scores + s2i_topk_rows, the [Q, N] matrix never held) against the stock
path on the same device, torch.matmul + torch.topk over the whole [Q, N] matrix, with HIP events: median of --iters after
--warmup.  Rows of 1024 floats; N = 29 330 (every image view of the CUB test split) and 1 000 000; Q = 1, 64 and 29 330;
k = 10 and 50.  For each it also reports the peak device memory either path takes above what is resident before it runs
(gallery and queries).  The stock path is skipped, and said to be, where its score matrix alone passes --stock_cap_gb.

Prints one JSON line.  No thresholds: the stock figure is the comparison, and some shapes favour it.

    python tools/search_bench.py [--iters 20] [--warmup 5] [--rows 29330,1000000] [--queries 1,64,29330] [--ks 10,50]
                                 [--chunk_rows 2048,8192,32768]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_to_image_translation_without_text_amd import _lib, retrieval  # noqa: E402

C = 1024


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def peak_above(fn, dev):
    """Peak bytes allocated during fn() above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def host_rows(n, seed):
    """n x 1024 fp32 rows: one 65 536-row normal block repeated with a factor per repeat, so no two rows are equal."""
    block = np.random.default_rng(seed).standard_normal((min(n, 65536), C), dtype=np.float32)
    out = np.empty((n, C), dtype=np.float32)
    for t, s in enumerate(range(0, n, block.shape[0])):
        e = min(s + block.shape[0], n)
        np.multiply(block[:e - s], np.float32(1.0 + 1e-3 * t), out=out[s:e])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=str, default="29330,1000000")
    ap.add_argument("--queries", type=str, default="1,64,29330")
    ap.add_argument("--ks", type=str, default="10,50")
    ap.add_argument("--chunk_rows", type=str, default=str(retrieval.GALLERY_CHUNK_ROWS),
                    help="comma-separated chunk sizes to time Gallery.search at")
    ap.add_argument("--stock_cap_gb", type=float, default=16.0, help="largest [Q, N] fp32 matrix the stock path is run at")
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    ints = lambda text: [int(v) for v in text.split(",")]  # noqa: E731
    result = {"device": torch.cuda.get_device_name(dev), "iters": args.iters, "warmup": args.warmup, "C": C, "runs": []}
    for n in ints(args.rows):
        rows = host_rows(n, 1)
        plain = torch.from_numpy(rows).to(dev)                           # the stock path's gallery, [N, C]
        galleries = {cr: retrieval.Gallery(rows, dev, chunk_rows=cr) for cr in ints(args.chunk_rows)}
        del rows
        for nq in ints(args.queries):
            q = torch.randn(nq, C, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
            for k in ints(args.ks):
                run = {"N": n, "Q": nq, "k": k}
                for cr, gal in galleries.items():
                    gal._scores = None
                    peak = peak_above(lambda: gal.search(q, k), dev)
                    run["gallery_chunk%d" % cr] = {"ms": timed(lambda: gal.search(q, k), args.iters, args.warmup),
                                                   "peak_mb": peak / 2 ** 20, "gallery_mb": gal.nbytes / 2 ** 20}
                    gal._scores = None
                matrix_gb = nq * n * 4 / 2 ** 30
                if matrix_gb > args.stock_cap_gb:
                    run["stock"] = "not run: the [Q, N] fp32 matrix alone is %.1f GB" % matrix_gb
                else:
                    def stock():
                        return torch.topk(torch.matmul(q, plain.t()), k, dim=1)
                    peak = peak_above(stock, dev)
                    run["stock"] = {"ms": timed(stock, args.iters, args.warmup), "peak_mb": peak / 2 ** 20}
                    # the two paths must name the same rows where fp32 rounding cannot reorder them: report, not a gate
                    ours = next(iter(galleries.values())).search(q, k)[1]
                    run["rows_agree_with_stock"] = float((ours == stock()[1]).float().mean())
                    torch.cuda.empty_cache()
                result["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
        del plain, galleries
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
