"""What the trainers' `specaug` option costs (GPU box only): ops.specaug at B = 64, T = 2048 beside ops.logmel_gather of
the same batch (the launch that makes a resident feeder's batch; both read and write the same 21 MB), and one
EncoderTrainer.step with and without the policy.

  specaug      us per call on HIP events, out of place (what the trainers call: the reduction over the valid rows, then a
               copy-or-mask of every piece, with the output's allocation) and in place (only masked pieces are written);
  gather       us per call of ops.logmel_gather producing the same [64, 1, 2048, 40] batch from a pool of 64 x 2048 rows;
  step         ms per EncoderTrainer.step (CNNRNN 40 -> 1024, bidirectional, B = 64, jel) of two trainers from one
               initialisation, one with the policy, in alternating blocks inside one process.

The three launches are timed in interleaved rounds (median and minimum over all rounds); the step blocks alternate off / on
and the fastest block of each is reported beside all of them.  Prints one JSON line and writes it to --out.

    python tools/specaug_bench.py [--batch 64] [--policy freq=2x8,time=2x40,ratio=0.2] [--out profiles/specaug_bench.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import _lib, ops  # noqa: E402
from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer  # noqa: E402
from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN  # noqa: E402

T = 2048


def one_call_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def summary(times):
    times = sorted(times)
    return {"median_us": round(times[len(times) // 2], 2), "min_us": round(times[0], 2)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--policy", type=str, default="freq=2x8,time=2x40,ratio=0.2")
    ap.add_argument("--iters", type=int, default=50, help="interleaved rounds of the three launches")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="alternating off / on blocks of steps")
    ap.add_argument("--skip-step", action="store_true", help="leave out the EncoderTrainer steps")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "specaug_bench.json"))
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.batch
    policy = ops.specaug_policy(args.policy)
    rng = np.random.RandomState(0)
    cap_lens = sorted(rng.randint(4, T // 64 + 1, B).tolist(), reverse=True)      # 256 .. 2048 frames an utterance
    valid = torch.tensor([64 * n for n in cap_lens], dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.empty((B * T, 40), dtype=torch.float32, device=dev).uniform_(-80.0, 0.0, generator=g)
    offsets = torch.arange(B, dtype=torch.int64, device=dev) * T
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    mel = ops.logmel_gather(pool, offsets, frames, T)
    scratch = mel.clone()
    step = [0]

    def aug():
        step[0] += 1
        return ops.specaug(mel, valid, policy, 1234, step[0])

    def aug_in_place():
        step[0] += 1
        return ops.specaug(scratch, valid, policy, 1234, step[0], out=scratch)

    calls = {"specaug": aug, "specaug_in_place": aug_in_place, "gather": lambda: ops.logmel_gather(pool, offsets, frames, T)}
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.iters):
        for k, fn in calls.items():
            times[k].append(one_call_us(fn))
    batch_bytes = B * T * 160
    valid_bytes = int(valid.sum()) * 160
    out = {"tool": "specaug_bench", "device": torch.cuda.get_device_name(dev), "batch": B, "T": T, "policy": args.policy,
           "valid_rows_mean": round(float(valid.float().mean()), 1), "batch_bytes": batch_bytes, "rounds": args.iters,
           "specaug": dict(summary(times["specaug"]), bytes_read=valid_bytes + batch_bytes, bytes_written=batch_bytes),
           "specaug_in_place": dict(summary(times["specaug_in_place"]), bytes_read_at_least=valid_bytes),
           "gather": dict(summary(times["gather"]), bytes_read=batch_bytes, bytes_written=batch_bytes),
           "note": "each call between two events, with the host's enqueue and the output's allocation; the in-place call "
                   "masks a batch that earlier calls have masked already"}
    out["specaug_over_gather"] = round(out["specaug"]["median_us"] / out["gather"]["median_us"], 2)

    if not args.skip_step:
        torch.manual_seed(1234)
        net = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).eval()
        trainers = {"off": EncoderTrainer(copy.deepcopy(net).to(dev), jel=True),
                    "on": EncoderTrainer(copy.deepcopy(net).to(dev), jel=True, specaug=args.policy, specaug_seed=1234)}
        image = torch.randn(B, 1024, generator=torch.Generator().manual_seed(1))
        label = torch.arange(B, dtype=torch.int64) % 40

        def block(tr, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = tr.step(mel, cap_lens, image, label)
            torch.cuda.synchronize()
            if not bool(torch.isfinite(loss["loss"])):
                raise RuntimeError("non-finite loss")
            return (time.perf_counter() - t0) / steps * 1e3
        for tr in trainers.values():
            block(tr, 3)
        blocks = {"off": [], "on": []}
        for _ in range(args.rounds):
            for k, tr in trainers.items():
                blocks[k].append(block(tr, args.steps))
        out["step"] = {"steps_per_block": args.steps,
                       "ms_per_step": {k: round(min(v), 3) for k, v in blocks.items()},
                       "ms_per_step_blocks": {k: [round(x, 3) for x in v] for k, v in blocks.items()},
                       "on_minus_off_ms": round(min(blocks["on"]) - min(blocks["off"]), 3),
                       "note": "the fastest block of each setting; blocks alternate off / on; every step uploads image "
                               "features and labels as the CLI's loop does"}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
