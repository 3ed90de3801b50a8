"""Speech input pipeline (GPU box only): train_encoder_head.SplitData.batches against speech_loader.ResidentSpeechSet.

Writes a synthetic CUB-shaped tree (--items x 10 utterances of 3-9 s of PCM16 at 16 kHz, 10 x 1024 image features per item;
seeded, nothing is downloaded) and reports, at batch size --batch,

  host        ms per batch of SplitData.batches (read 64 WAVs, upload, three log-mel kernels), synchronised per batch, the
              files in the page cache (they were just written: the state this tool can reach);
  resident    wall ms per batch of ResidentSpeechSet.batches (draws, two index uploads, one launch), synchronised per batch;
  construct   seconds and utterances per second of building the pool, and its bytes;
  gather      the launch alone on HIP events (median of --iters after --warmup), its bytes read + written over that time
              and that as a fraction of the 6.3 TB/s a streaming copy reaches on this part;
  epoch       EncoderTrainer over one epoch of the tree, fed by either feeder;

next to the measured step times of DESIGN.md section 8b3 (8.16 ms at B = 64, 5.13 ms at B = 32): "a batch is made faster
than it is consumed" is resident median < step time.  Prints one JSON line and writes it to --out.

    python tools/speech_loader_bench.py [--items 960] [--batch 64] [--out profiles/speech_loader_bench.json]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
import wave
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import _lib, datasets, ops, speech_loader  # noqa: E402
from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer  # noqa: E402
from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN  # noqa: E402
from speech_to_image_translation_without_text_amd.train_encoder_head import SplitData  # noqa: E402

STREAM_CEILING_GBS = 6300.0
STEP_MS = {64: 8.16, 32: 5.13}      # EncoderTrainer.step, DESIGN.md section 8b3


def write_tree(root, items, utterances=10, classes=40):
    """`items` x `utterances` clips of 3-9 s: a tone in a slice of one shared noise buffer, so that writing is cheap."""
    rng = np.random.RandomState(0)
    noise = (0.05 * rng.randn(16000 * 19)).astype(np.float32)
    seconds = rng.uniform(3.0, 9.0, (items, utterances))
    starts = rng.randint(0, 16000 * 10, (items, utterances))

    def one(job):
        i, u = job
        n = int(16000 * seconds[i, u])
        sig = 0.3 * np.sin(2 * np.pi * (150 + 3 * ((7 * i + u) % 200)) * np.arange(n, dtype=np.float32) / 16000.0)
        sig += noise[starts[i, u]:starts[i, u] + n]
        path = os.path.join(root, "audio", "train", "item%d" % i, "utt%d.wav" % u)
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())

    for i in range(items):
        os.makedirs(os.path.join(root, "audio", "train", "item%d" % i))
    with ThreadPoolExecutor(max_workers=16) as ex:
        list(ex.map(one, [(i, u) for i in range(items) for u in range(utterances)]))
    data = [{"audio": ["train/item%d/utt%d.wav" % (i, u) for u in range(utterances)],
             "class": "%03d.Species_%d" % (i % classes + 1, i % classes)} for i in range(items)]
    feat = os.path.join(root, "train", "image_features.pickle")
    os.makedirs(os.path.dirname(feat))
    datasets.save_embedding_pickle(rng.randn(items, 10, 1024).astype(np.float32), feat)
    with open(os.path.join(root, "train.json"), "w") as f:
        json.dump({"audio_base_path": os.path.join(root, "audio"), "image_feature_path": feat, "data": data}, f)
    return float(seconds.sum())


def batch_walls(feeder, batch, dev, epochs):
    """wall ms of every batch of `epochs` shuffled epochs, each batch synchronised; the first batch is a warm-up"""
    walls = []
    for _ in range(epochs):
        it = feeder.batches(batch, dev, True)
        while True:
            t0 = time.perf_counter()
            b = next(it, None)
            if b is None:
                break
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
    walls = sorted(walls[1:])
    return {"batches": len(walls), "median_ms": round(walls[len(walls) // 2], 3), "p90_ms": round(walls[len(walls) * 9 // 10], 3),
            "max_ms": round(walls[-1], 3)}


def epoch_seconds(trainer, feeder, batch, dev):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for mel, cap_lens, image, label in feeder.batches(batch, dev, True):
        trainer.step(mel, cap_lens, image, label)
    torch.cuda.synchronize()
    return round(time.perf_counter() - t0, 3)


def note(msg):
    print("[speech_loader_bench] " + msg, file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=960)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--resident-epochs", type=int, default=5)
    ap.add_argument("--skip-epoch", action="store_true", help="leave out the EncoderTrainer epochs")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "speech_loader_bench.json"))
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = args.batch
    out = {"tool": "speech_loader_bench", "device": torch.cuda.get_device_name(dev), "items": args.items,
           "utterances": args.items * 10, "batch": B, "T": 2048}
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        out["audio_seconds"] = round(write_tree(root, args.items), 1)
        note("tree written in %.1f s" % (time.perf_counter() - t0))
        split = SplitData(root, "train", "birds")
        random.seed(0)
        out["host"] = dict(batch_walls(split, B, dev, 1), page_cache="warm: the files were written by this process")
        note("host feeder: %r" % out["host"])
        t0 = time.perf_counter()
        rs = speech_loader.ResidentSpeechSet(split, dev, workers=16)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["construct"] = {"seconds": round(dt, 3), "utterances_per_s": round(args.items * 10 / dt, 1),
                            "rows": rs.pool.shape[0], "nbytes": rs.nbytes, "bytes_per_utterance": round(rs.nbytes / (args.items * 10))}
        note("pool: %r" % out["construct"])
        random.seed(0)
        out["resident"] = batch_walls(rs, B, dev, args.resident_epochs)
        note("resident feeder: %r" % out["resident"])

        # the launch alone, on the utterances of one drawn batch
        random.seed(1)
        drawn = [(i, rs.draw(i)[1]) for i in range(B)]
        frames = np.array([rs.frames[i][u] for i, u in drawn], dtype=np.int64)
        off_d = torch.from_numpy(rs.row_offsets[[rs.first[i] + u for i, u in drawn]]).to(dev)
        frm_d = torch.from_numpy(frames.astype(np.int32)).to(dev)
        for _ in range(args.warmup):
            ops.logmel_gather(rs.pool, off_d, frm_d, rs.T)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.logmel_gather(rs.pool, off_d, frm_d, rs.T)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        k_ms = times[len(times) // 2]
        moved = int(frames.sum()) * 160 + B * rs.T * 160
        gbs = moved / (k_ms * 1e-3) / 1e9
        out["gather"] = {"ms": round(k_ms, 5), "min_ms": round(times[0], 5), "bytes_read_plus_written": moved,
                         "gbytes_per_s": round(gbs, 1), "fraction_of_6300_gbs": round(gbs / STREAM_CEILING_GBS, 4),
                         "ms_at_6300_gbs": round(moved / STREAM_CEILING_GBS / 1e6, 5),
                         "bound": "launch" if gbs < 0.5 * STREAM_CEILING_GBS else "bandwidth",
                         "note": "one launch with its output allocation between two events; 'launch' = under half the "
                                 "streaming ceiling, the time is the launch's fixed cost, not the bytes"}
        out["step_ms_8b3"] = {"B64": STEP_MS[64], "B32": STEP_MS[32]}
        if B in STEP_MS:
            out["batch_made_faster_than_consumed"] = bool(out["resident"]["median_ms"] < STEP_MS[B])
            out["host_batch_made_faster_than_consumed"] = bool(out["host"]["median_ms"] < STEP_MS[B])
        out["resident_faster_than_host"] = bool(out["resident"]["median_ms"] < out["host"]["median_ms"])

        if not args.skip_epoch:
            torch.manual_seed(1234)
            trainer = EncoderTrainer(CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).eval().to(dev), jel=True)
            random.seed(2)
            warm = epoch_seconds(trainer, rs, B, dev)
            random.seed(3)
            host_s = epoch_seconds(trainer, split, B, dev)
            random.seed(3)
            res_s = epoch_seconds(trainer, rs, B, dev)
            steps = -(-args.items // B)
            out["epoch"] = {"steps": steps, "warmup_epoch_s": warm, "host_s": host_s, "resident_s": res_s,
                            "host_ms_per_step": round(host_s / steps * 1e3, 2),
                            "resident_ms_per_step": round(res_s / steps * 1e3, 2)}
            note("epoch: %r" % out["epoch"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
