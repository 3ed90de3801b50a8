"""Waveform augmentation of the encoder's training audio (GPU box only): wave_loader.ResidentWaveSet with and without
--waveaug against speech_loader.ResidentSpeechSet, over the synthetic CUB-shaped tree of tools/speech_loader_bench.py.

  construct   seconds and bytes of the waveform pool; CUB's 88 550 training utterances extrapolated from bytes per
              utterance (marked as extrapolated: nothing that size was built);
  feeder      wall ms per batch, synchronised per batch: the log-mel pool (one gather launch), the waveform pool with
              augmentation off (bypass + log-mel) and on (--spec);
  launches    one augmented batch split on HIP events (median of --iters): the resample launches (one per speed), the mix
              through ops.wave_mix (host checks and the table upload included) and its two kernel launches alone, the
              three log-mel launches as the feeder runs them; the two mix kernels' bytes read + written over their time
              next to the 6.3 TB/s a streaming copy reaches, labelled launch- or bandwidth-bound by the sibling benches' rule;
  step        EncoderTrainer fed by the log-mel pool (what `train_encoder --resident` runs) and by the augmented waveform
              pool, in alternating blocks of --block steps, the fastest block of each, next to DESIGN.md 8b3's 8.16 ms.

Prints one JSON line and writes it to --out.

    python tools/waveaug_bench.py [--items 960] [--batch 64] [--out profiles/waveaug_bench.json]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_loader_bench import STEP_MS, STREAM_CEILING_GBS, batch_walls, write_tree  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib, ops, speech_loader, wave_loader  # noqa: E402
from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer  # noqa: E402
from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN  # noqa: E402
from speech_to_image_translation_without_text_amd.train_encoder_head import SplitData  # noqa: E402

CUB_TRAIN_UTTERANCES = 88550


def note(msg):
    print("[waveaug_bench] " + msg, file=sys.stderr, flush=True)


class _Fed:
    """a feeder with its keywords bound, for batch_walls"""

    def __init__(self, feeder, **kw):
        self.feeder, self.kw = feeder, kw

    def batches(self, batch, dev, shuffle):
        return self.feeder.batches(batch, dev, shuffle, **self.kw)


def event_ms(fn, iters, warmup):
    times = []
    for k in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def launches(ws, aug, B, iters, warmup):
    """one augmented batch of the first B stored utterances, stage by stage"""
    from speech_to_image_translation_without_text_amd import audio
    pairs = []
    for i in range(len(ws)):
        pairs += [(i, u) for u in range(len(ws.frames[i])) if ws.frames[i][u] >= 64][:1]
        if len(pairs) == B:
            break
    flat_ids = np.array([ws.first[i] + u for i, u in pairs])
    lens = ws.samples[flat_ids]
    plan = ops.waveaug_plan(aug.policy, aug.seed, 0, np.arange(B), lens, ws.stored_lens, ws.stored_q, ws.T)
    table = ops.wave_mix_table(plan, ws.stored_offsets, ws.stored_lens)
    state = {}

    def resample():
        state["flat"], state["off"] = wave_loader.render(ws.pool, ws.offsets[flat_ids], lens, plan["rate"], plan["out_len"])

    # both mix timings work in place on the one rendered batch, so the clips' power grows from one iteration to the
    # next; the launches and the bytes they move are the same every time, which is all that is timed
    def mix():
        ops.wave_mix(state["flat"], state["off"], plan["out_len"], table, aug.seed, 0, pool=ws.pool)

    def mix_kernels():
        ops.wave_mix_launch(state["args"], aug.seed, 0)

    def mel():          # what ResidentWaveSet.mel runs: no concatenation copy
        out = torch.empty((B, 1, ws.T, audio.N_MELS), dtype=torch.float32, device=ws.device)
        audio.launch(audio.prepare_flat(state["flat"], state["off"], plan["out_len"], ws.T, ws.device), out, "nhwc")
    out = {"speeds": len(set(plan["rate"].tolist())), "resample_ms": round(event_ms(resample, iters, warmup), 4)}
    mix_ms = event_ms(mix, iters, warmup)
    state["args"] = ops.wave_mix_prepare(state["flat"], state["off"], plan["out_len"], table, pool=ws.pool)
    kernels_ms = event_ms(mix_kernels, iters, warmup)
    samples = int(plan["out_len"].sum())
    # the power pass reads every clip; the mix reads and writes the clips with a term on and reads their interferers
    on = (plan["g_white"] != 0) | (plan["g_babble"] != 0)
    moved = 4 * samples + 8 * int(plan["out_len"][on].sum()) + 4 * int(plan["out_len"][plan["g_babble"] != 0].sum())
    gbs = moved / kernels_ms / 1e6
    out.update(mix_ms=round(mix_ms, 4), mix_kernels_ms=round(kernels_ms, 4), mix_bytes=moved, mix_gbytes_per_s=round(gbs, 1),
               mix_fraction_of_6300_gbs=round(gbs / STREAM_CEILING_GBS, 4),
               mix_ms_at_6300_gbs=round(moved / STREAM_CEILING_GBS / 1e6, 5),
               bound="launch" if gbs < 0.5 * STREAM_CEILING_GBS else "bandwidth",
               white_clips=int((plan["g_white"] != 0).sum()), babble_clips=int((plan["g_babble"] != 0).sum()),
               logmel_ms=round(event_ms(mel, iters, warmup), 4), samples=samples)
    return out


def block_ms(trainer, it, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(*next(it))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def forever(make):
    while True:
        yield from make()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=960)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=30, help="steps per alternating block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--spec", type=str, default="speed=0.9/1.0/1.1,white=0.3@5:25,babble=0.2@0:15")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "waveaug_bench.json"))
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.batch
    out = {"tool": "waveaug_bench", "device": torch.cuda.get_device_name(dev), "items": args.items,
           "utterances": args.items * 10, "batch": B, "T": 2048, "spec": args.spec}
    with tempfile.TemporaryDirectory() as root:
        out["audio_seconds"] = round(write_tree(root, args.items), 1)
        split = SplitData(root, "train", "birds")
        t0 = time.perf_counter()
        ws = wave_loader.ResidentWaveSet(split, dev, workers=16)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        per = ws.nbytes / len(ws.stored)
        out["construct"] = {"seconds": round(dt, 3), "utterances_per_s": round(len(ws.stored) / dt, 1), "nbytes": ws.nbytes,
                            "bytes_per_utterance": round(per), "message": ws.message,
                            "cub_train_extrapolated": {"utterances": CUB_TRAIN_UTTERANCES,
                                                       "gbytes": round(per * CUB_TRAIN_UTTERANCES / 1e9, 1),
                                                       "seconds": round(dt * CUB_TRAIN_UTTERANCES / len(ws.stored), 1),
                                                       "measured": False}}
        note("pool: %r" % out["construct"])
        rs = speech_loader.ResidentSpeechSet(split, dev, workers=16)
        aug = wave_loader.WaveAug(args.spec, 0)
        count = [0]

        def step():
            count[0] += 1
            return count[0]
        random.seed(0)
        out["feeder"] = {"logmel_pool": batch_walls(rs, B, dev, 2), "wave_pool_off": batch_walls(ws, B, dev, 2),
                         "wave_pool_on": batch_walls(_Fed(ws, aug=aug, step=step), B, dev, 2)}
        note("feeder: %r" % out["feeder"])
        out["launches"] = launches(ws, aug, B, args.iters, args.warmup)
        note("launches: %r" % out["launches"])
        torch.manual_seed(0)
        model = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).to(dev)
        trainer = EncoderTrainer(model, jel=True)
        feeds = {"logmel_pool": forever(lambda: rs.batches(B, dev, True)),
                 "wave_pool_on": forever(lambda: ws.batches(B, dev, True, aug=aug, step=lambda: trainer.steps))}
        for it in feeds.values():
            block_ms(trainer, it, 5)                     # warm-up
        blocks = {k: [] for k in feeds}
        for _ in range(args.blocks):
            for k, it in feeds.items():
                blocks[k].append(round(block_ms(trainer, it, args.block), 3))
        ref = STEP_MS.get(B)
        out["step"] = {"blocks_ms": blocks, "fastest_ms": {k: min(v) for k, v in blocks.items()}, "step_ms_8b3": ref,
                       "added_ms": round(min(blocks["wave_pool_on"]) - min(blocks["logmel_pool"]), 3)}
        made = out["feeder"]["wave_pool_on"]["median_ms"]
        out["batch_made_faster_than_consumed"] = bool(ref is not None and made < ref)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
