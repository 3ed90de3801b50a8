"""Speech front end timing (GPU box only).

  fused     s2i_signal_mean + logmel_power + logmel_finish (audio.launch) on device events after warm-up;
  composed  the same math from existing pieces: torch reflect pad + unfold builds the frames [1, 1, F, 400] in HBM,
            the 400 x 402 window-folded DFT runs through conv_raw(CONV_K1), torch does the power, the mel matmul and
            the dB step;
for 240 utterances x 2048 frames and for 240 lengths drawn from 3-12 s.  TFLOP/s use the algorithmic count
frames x (2*400*400 + 2*201*40) against the 157.3 TFLOP/s fp32 matrix peak.  Then end-to-end extraction (WAV files on
disk -> pickles, seeded random encoder) in utterances/s.  Kernel names are stable (signal_mean_kernel,
logmel_power_kernel, logmel_finish_kernel) for a separate rocprofv3 --kernel-trace --stats run.

Usage:  python tools/logmel_bench.py [--reps 20] [--skip-e2e]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import _lib, audio, ops  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import CONV_K1, PACK_PLAIN  # noqa: E402

PEAK_TF = 157.3


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def composed_setup(dev):
    basis = torch.from_numpy(np.concatenate([
        audio.dft_basis64()[:, [32 * (q // 16) + (q % 16) for q in range(200)]],           # cos 0..199
        (audio.hamming_window() * np.cos(np.pi * np.arange(400)))[:, None],               # cos 200
        audio.dft_basis64()[:, [32 * (q // 16) + 16 + (q % 16) for q in range(1, 200)]],  # sin 1..199
        np.zeros((400, 2))], axis=1).astype(np.float32))                                  # 402 -> 404 columns
    packed = ops.pack_weight(basis.t().contiguous().to(dev), PACK_PLAIN)
    bank = torch.from_numpy(audio.mel_filterbank()).to(dev)
    return packed, bank


def composed(sigs, T, packed, bank):
    frames = []
    for s in sigs:
        y = s - s.mean()
        y = torch.cat([y[:1], y[1:] - 0.97 * y[:-1]])
        yp = torch.nn.functional.pad(y.view(1, 1, -1), (200, 200), mode="reflect").view(-1)
        frames.append(yp.unfold(0, 400, 160))
    fr = torch.cat(frames)
    F = fr.shape[0]
    fr = torch.nn.functional.pad(fr, (0, 0, 0, -F % 64)).view(-1, 1, 64, 400)   # the K1 kind needs power-of-two W
    spec, _, _ = ops.conv_raw(CONV_K1, fr, None, packed, 404, wR=packed.shape[1], ldw=packed.shape[2])
    spec = spec.view(-1, 404)[:F]
    re, im = spec[:, :201], torch.nn.functional.pad(spec[:, 201:400], (1, 1))
    mel = (re * re + im * im) @ bank.t()
    out, start = [], 0
    for f in frames:
        m = mel[start:start + f.shape[0]]
        start += f.shape[0]
        db = 10 * torch.log10(m.clamp_min(1e-10)) - 10 * torch.log10(m.max().clamp_min(1e-10))
        db = db.clamp_min(-80.0)[:T]
        out.append(torch.nn.functional.pad(db, (0, 0, 0, T - db.shape[0])))
    return torch.stack(out)


def bench_case(name, lens, reps, dev, packed, bank):
    g = torch.Generator().manual_seed(1)
    sigs = [(0.3 * torch.randn(int(n), generator=g)).to(dev) for n in lens]
    batch = audio.prepare_batch(sigs, 2048, dev)
    out = torch.empty((len(sigs), 1, 2048, 40), dtype=torch.float32, device=dev)
    frames = int((1 + np.asarray(lens) // 160).sum())
    t_fused = timed(lambda: audio.launch(batch, out, "nhwc"), reps)
    ref = composed(sigs, 2048, packed, bank)
    err = float((ref - out.view(len(sigs), 2048, 40)).abs().max())
    t_comp = timed(lambda: composed(sigs, 2048, packed, bank), max(3, reps // 4))
    fl = audio.flops(frames)
    return {"case": name, "utterances": len(sigs), "frames": frames, "fused_ms": round(t_fused, 4),
            "fused_tflops": round(fl / t_fused / 1e9, 2), "fused_pct_peak": round(100 * fl / t_fused / 1e9 / PEAK_TF, 1),
            "composed_ms": round(t_comp, 4), "composed_tflops": round(fl / t_comp / 1e9, 2),
            "speedup": round(t_comp / t_fused, 2), "max_abs_db_diff_vs_composed": round(err, 5)}


def bench_e2e(dev, n=240):
    from speech_to_image_translation_without_text_amd import extract_audio_feature as E
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        names = []
        for i in range(n):
            y = np.clip(rng.standard_normal(int(rng.integers(3 * 16000, 12 * 16000))) * 3000, -32768, 32767)
            with wave.open(os.path.join(d, "%d.wav" % i), "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(16000)
                f.writeframes(y.astype("<i2").tobytes())
            names.append("%d.wav" % i)
        with open(os.path.join(d, "test.json"), "w") as f:
            json.dump({"audio_base_path": d, "data": [{"audio": names[i:i + 10]} for i in range(0, n, 10)]}, f)
        torch.manual_seed(0)
        model = CNNRNN(40, embedding_dim=1024, nhidden=1024, nsent=1024, bidirectional=True).eval().to(dev)
        E.extract_split(model, d, "test", "birds", "0", batch_size=n)        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.extract_split(model, d, "test", "birds", "0", batch_size=n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"case": "extract_e2e", "utterances": n, "seconds": round(dt, 3), "utterances_per_s": round(n / dt, 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--skip-e2e", action="store_true")
    args = p.parse_args()
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda:0")
    packed, bank = composed_setup(dev)
    rng = np.random.default_rng(0)
    rows = [bench_case("240x2048", [2047 * 160] * 240, args.reps, dev, packed, bank),
            bench_case("240x3-12s", rng.integers(3 * 16000, 12 * 16000, 240), args.reps, dev, packed, bank)]
    if not args.skip_e2e:
        rows.append(bench_e2e(dev))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
