"""WAV -> 16 kHz converter timing (GPU box only).

For B = 64 clips of 6 s, PCM16 mono, at 48 kHz and at 44.1 kHz: one s2i_pcm_resample launch over the uploaded group
(audio.launch_resample) timed with HIP events, the median of 20 launches after 5 warm-up launches; GB/s counts the clip
bytes read plus the fp32 samples written, GFLOP/s counts 2 * taps per output.  Beside it the three log-mel launches
(audio.launch) on the batch the converter produced, and, where scipy is installed, scipy.signal.resample_poly over the
same clips on 16 threads.  One JSON line goes to --out (default profiles/resample_bench.json) and to stdout.  The
kernel's name is stable (pcm_resample_kernel) for a separate rocprofv3 --kernel-trace --stats run.

Usage:  python tools/resample_bench.py [--out profiles/resample_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import _lib, audio  # noqa: E402

B, SECONDS, WARMUP, REPS, THREADS = 64, 6, 5, 20, 16


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def bench_rate(rate, dev):
    rng = np.random.default_rng(rate)
    n = SECONDS * rate
    pcm = [np.clip(rng.standard_normal(n) * 3000, -32768, 32767).astype("<i2") for _ in range(B)]
    raws = [p.view(np.uint8) for p in pcm]
    L, M, W, taps = audio.resample_plan(rate)
    out_lens = np.array([audio.resampled_length(n, rate)] * B, dtype=np.int64)
    out_offsets = np.cumsum(out_lens) - out_lens
    image, where, ntiles = audio.pack_group(raws, [n] * B, out_offsets, out_lens)
    image_d = torch.from_numpy(image).to(dev)
    table = audio.device_resample_table(dev, rate)
    flat = torch.empty(int(out_lens.sum()), dtype=torch.float32, device=dev)

    def convert():
        audio.launch_resample(image_d, where, ntiles, B, _lib.PCM_S16, 1, L, M, W, table, flat)
    ms = median_ms(convert)
    sigs = [flat[int(o):int(o + k)] for o, k in zip(out_offsets, out_lens)]
    batch = audio.prepare_batch(sigs, audio.TARGET_LENGTH, dev)
    mel = torch.empty((B, 1, audio.TARGET_LENGTH, audio.N_MELS), dtype=torch.float32, device=dev)
    mel_ms = median_ms(lambda: audio.launch(batch, mel, "nhwc"))
    outputs = int(out_lens.sum())
    row = {"rate": rate, "L": L, "M": M, "W": W, "taps": taps, "tiles": ntiles, "outputs": outputs,
           "resample_ms": round(ms, 4), "gb_per_s": round((2 * n * B + 4 * outputs) / ms / 1e6, 1),
           "gflop_per_s": round(2.0 * taps * outputs / ms / 1e6, 1), "logmel_ms": round(mel_ms, 4)}
    try:
        from scipy.signal import resample_poly
    except ImportError:
        return row
    xs = [p.astype(np.float32) / np.float32(32768) for p in pcm]
    with ThreadPoolExecutor(max_workers=THREADS) as ex:
        list(ex.map(lambda x: resample_poly(x, L, M), xs[:THREADS]))           # warm-up
        t0 = time.perf_counter()
        list(ex.map(lambda x: resample_poly(x, L, M), xs))
        row["scipy_resample_poly_16_threads_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    args = p.parse_args()
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda:0")
    result = {"bench": "resample", "clips": B, "seconds": SECONDS, "format": "s16 mono", "warmup": WARMUP, "reps": REPS,
              "cases": [bench_rate(rate, dev) for rate in (48000, 44100)]}
    line = json.dumps(result)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
