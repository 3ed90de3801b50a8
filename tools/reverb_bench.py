"""Room reverberation of the encoder's training audio (GPU box only).

  kernels   s2i_reverb_rir + s2i_reverb alone (tables uploaded once, no host checks inside the timed window) at
            B = --batch clips of 5 s and of 20 s, T60 of 0.2 / 0.6 / 1.0 s (3200 / 9600 / 16000 taps), every clip
            reverberated: median device time of the two launches over --iters, the FLOP/s on 2 n taps per clip (what the
            convolution needs; the zero products of the two end blocks and of the clip's first taps are not counted), and
            that rate over the 157.3 TFLOP/s of the fp32 matrix cores (a compute bound: the kernel reads and writes each
            sample once per 1024 taps);
  feeder    wall ms per batch of wave_loader.ResidentWaveSet, synchronised per batch, under --base and under --base plus
            --reverb, over the synthetic CUB-shaped tree of tools/speech_loader_bench.py;
  step      EncoderTrainer fed under --base (what the step was before reverb= existed) and under --base plus --reverb, in
            alternating blocks of --block steps, the fastest block of each; and the step alone on one batch held on the
            device, which is what a batch has to be made faster than.

Prints one JSON line and writes it to --out.

    python tools/reverb_bench.py [--items 640] [--batch 64] [--out profiles/reverb_bench.json]
"""
import argparse
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from speech_loader_bench import batch_walls, write_tree  # noqa: E402
from waveaug_bench import _Fed, block_ms, forever  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib, ops, wave_loader  # noqa: E402
from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer  # noqa: E402
from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN  # noqa: E402
from speech_to_image_translation_without_text_amd.train_encoder_head import SplitData  # noqa: E402

F32_MATRIX_TFLOPS = 157.3
RATE = 16000


def note(msg):
    print("[reverb_bench] " + msg, file=sys.stderr, flush=True)


def kernel_case(dev, B, seconds, t60, iters, warmup):
    """the two launches on B clips of `seconds`, all reverberated at T60 = t60"""
    lib = _lib.load()
    n = int(seconds * RATE)
    plan = ops.waveaug_plan(ops.waveaug_policy("reverb=1@%s:%s@5:5" % (t60, t60)), 0, 0, np.arange(B), np.full(B, n))
    table = ops.reverb_table(plan)
    taps = int(table["taps"].max())
    offsets = np.arange(B, dtype=np.int64) * n
    x = 0.1 * torch.randn(B * n, device=dev)
    y = torch.empty_like(x)
    h = torch.empty(B * taps, dtype=torch.float32, device=dev)
    table_d = torch.from_numpy(table.view(np.uint8).copy()).to(dev)
    off_d = torch.from_numpy(offsets).to(dev)
    lens_d = torch.full((B,), n, dtype=torch.int32, device=dev)

    def rir():
        _lib.check(lib.s2i_reverb_rir(_lib.ptr(table_d), B, taps, _lib.ptr(h), 1, 2, _lib.stream()), "s2i_reverb_rir")

    def conv():
        _lib.check(lib.s2i_reverb(_lib.ptr(x), _lib.ptr(off_d), _lib.ptr(lens_d), B, n, _lib.ptr(table_d), _lib.ptr(h), taps,
                                  _lib.ptr(y), _lib.stream()), "s2i_reverb")
    both, rir_only = [], []
    for k in range(warmup + iters):
        a, m, b = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        rir()
        m.record()
        conv()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            both.append(a.elapsed_time(b))
            rir_only.append(a.elapsed_time(m))
    ms = sorted(both)[len(both) // 2]
    flop = 2.0 * B * n * taps
    tflops = flop / ms / 1e9
    return {"seconds": seconds, "t60": t60, "taps": taps, "samples": B * n, "launches_ms": round(ms, 4),
            "min_ms": round(min(both), 4), "max_ms": round(max(both), 4), "rir_ms": round(sorted(rir_only)[len(rir_only) // 2], 4),
            "gflop": round(flop / 1e9, 2), "tflops": round(tflops, 2),
            "fraction_of_157_3_tflops": round(tflops / F32_MATRIX_TFLOPS, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block", type=int, default=60, help="steps per alternating block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--base", type=str, default="speed=0.9/1.0/1.1,white=0.3@5:25,babble=0.2@0:15")
    ap.add_argument("--reverb", type=str, default="reverb=0.3@0.2:0.6@0:15")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "reverb_bench.json"))
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.batch
    out = {"tool": "reverb_bench", "device": torch.cuda.get_device_name(dev), "batch": B, "items": args.items,
           "base": args.base, "reverb": args.reverb, "kernels": []}
    torch.manual_seed(0)
    for seconds in (5, 20):
        for t60 in (0.2, 0.6, 1.0):
            out["kernels"].append(kernel_case(dev, B, seconds, t60, args.iters, args.warmup))
            note("kernels: %r" % out["kernels"][-1])
    with tempfile.TemporaryDirectory() as root:
        out["audio_seconds"] = round(write_tree(root, args.items), 1)
        split = SplitData(root, "train", "birds")
        ws = wave_loader.ResidentWaveSet(split, dev, workers=16)
        torch.cuda.synchronize()
        specs = {"base": args.base, "base_reverb": args.base + "," + args.reverb}
        augs = {k: wave_loader.WaveAug(s, 0) for k, s in specs.items()}
        count = [0]

        def step():
            count[0] += 1
            return count[0]
        random.seed(0)
        out["feeder"] = {k: batch_walls(_Fed(ws, aug=a, step=step), B, dev, 2) for k, a in augs.items()}
        note("feeder: %r" % out["feeder"])
        torch.manual_seed(0)
        model = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).to(dev)
        trainer = EncoderTrainer(model, jel=True)
        feeds = {k: forever(lambda a=a: ws.batches(B, dev, True, aug=a, step=lambda: trainer.steps)) for k, a in augs.items()}
        for it in feeds.values():
            block_ms(trainer, it, 5)                     # warm-up
        blocks = {k: [] for k in feeds}
        for _ in range(args.blocks):
            for k, it in feeds.items():
                blocks[k].append(round(block_ms(trainer, it, args.block), 3))
        held = next(feeds["base_reverb"])
        alone = [round(block_ms(trainer, forever(lambda: [held]), args.block), 3) for _ in range(args.blocks)]
        out["step"] = {"blocks_ms": blocks, "fastest_ms": {k: min(v) for k, v in blocks.items()},
                       "added_ms": round(min(blocks["base_reverb"]) - min(blocks["base"]), 3),
                       "step_alone_blocks_ms": alone, "step_alone_ms": min(alone)}
        made = out["feeder"]["base_reverb"]["median_ms"]
        out["batch_made_ms"] = made
        out["batch_made_faster_than_consumed"] = bool(made < min(alone))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
