"""Pitch and tempo augmentation of the encoder's training audio (GPU box only).

  kernels   s2i_time_stretch alone (tables uploaded and the workspace allocated once, no host checks inside the timed
            window) at B = --batch clips of 5 s and of 20 s, every clip stretched, at rho = 0.5 / 0.9 / 1.1 / 2.0: median
            device time of the five launches over --iters after --warmup (HIP events), the FLOP of the two transforms
            (2 x 512 x 512 per analysed frame and as much per output frame), their rate over the whole time, and that rate
            over the 157.3 TFLOP/s of the fp32 matrix cores;
  feeder    wall ms per batch of wave_loader.ResidentWaveSet, synchronised per batch, under --base and under --base plus
            --voice, over the synthetic CUB-shaped tree of tools/speech_loader_bench.py;
  step      EncoderTrainer fed under --base and under --base plus --voice, in alternating blocks of --block steps, the
            fastest block of each; and the step alone on one batch held on the device, which is what a batch has to be
            made faster than.

Prints one JSON line and writes it to --out.

    python tools/stretch_bench.py [--items 640] [--batch 64] [--out profiles/stretch_bench.json]
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
    print("[stretch_bench] " + msg, file=sys.stderr, flush=True)


def kernel_case(dev, B, seconds, rho, iters, warmup):
    """the five launches on B clips of `seconds`, all stretched by rho"""
    lib = _lib.load()
    n = int(seconds * RATE)
    table = np.zeros(B, dtype=ops.STRETCH_ENTRY)
    table["rate"], table["out_len"] = rho, int(np.floor(n / rho + 0.5))
    x = 0.1 * torch.randn(B * n, device=dev)
    args = ops.time_stretch_prepare(x, np.arange(B, dtype=np.int64) * n, np.full(B, n), table)
    need = lib.s2i_time_stretch_workspace_bytes(B, args["in_frames"], args["out_frames"])
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    basis = ops.device_stretch_basis(dev)

    def launch():
        _lib.check(lib.s2i_time_stretch(_lib.ptr(x), args["offsets"], args["lens"], B, args["max_len"], args["table"],
                                        _lib.ptr(basis), _lib.ptr(args["out"]), args["out_offsets"], args["max_out_len"],
                                        args["in_frames"], args["out_frames"], _lib.ptr(ws), need, _lib.stream()),
                   "s2i_time_stretch")
    times = []
    for k in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    ms = sorted(times)[len(times) // 2]
    flop = 2.0 * 512 * 512 * (args["in_frames"] + args["out_frames"])
    tflops = flop / ms / 1e9
    return {"seconds": seconds, "rho": rho, "in_frames": args["in_frames"], "out_frames": args["out_frames"],
            "workspace_mb": round(need / 2 ** 20, 1), "launches_ms": round(ms, 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4), "gflop": round(flop / 1e9, 2), "tflops": round(tflops, 2),
            "fraction_of_157_3_tflops": round(tflops / F32_MATRIX_TFLOPS, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=60, help="steps per alternating block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--base", type=str, default="speed=0.9/1.0/1.1,white=0.3@5:25,babble=0.2@0:15")
    ap.add_argument("--voice", type=str, default="pitch=-2/0/2,tempo=0.9/1.0/1.1")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "stretch_bench.json"))
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.batch
    out = {"tool": "stretch_bench", "device": torch.cuda.get_device_name(dev), "batch": B, "items": args.items,
           "base": args.base, "voice": args.voice, "kernels": []}
    torch.manual_seed(0)
    for seconds in (5, 20):
        for rho in (0.5, 0.9, 1.1, 2.0):
            out["kernels"].append(kernel_case(dev, B, seconds, rho, args.iters, args.warmup))
            note("kernels: %r" % out["kernels"][-1])
            torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as root:
        out["audio_seconds"] = round(write_tree(root, args.items), 1)
        split = SplitData(root, "train", "birds")
        ws = wave_loader.ResidentWaveSet(split, dev, workers=16)
        torch.cuda.synchronize()
        specs = {"base": args.base, "base_voice": args.base + "," + args.voice}
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
        held = next(feeds["base_voice"])
        alone = [round(block_ms(trainer, forever(lambda: [held]), args.block), 3) for _ in range(args.blocks)]
        out["step"] = {"blocks_ms": blocks, "fastest_ms": {k: min(v) for k, v in blocks.items()},
                       "added_ms": round(min(blocks["base_voice"]) - min(blocks["base"]), 3),
                       "step_alone_blocks_ms": alone, "step_alone_ms": min(alone)}
        made = out["feeder"]["base_voice"]["median_ms"]
        out["batch_made_ms"] = made
        out["batch_made_faster_than_consumed"] = bool(made < min(alone))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
