"""Input pipeline throughput (GPU box only): the host DataLoader against the resident image pool.

Writes a synthetic CUB-shaped tree of JPEGs (sizes from a fixed list around 500 x 375, bounding boxes, ten 1024-d
embeddings per image; seeded, nothing is downloaded) and reports samples per second -- one sample is a real and a wrong
image, each as a 64 / 128 / 256 pyramid, as float tensors on the device -- for

  host_w0    make_dataloader(workers=0) + the trainer's prepare_data step (uint8 batches, normalised on the device);
  host_w16   the same with 16 worker processes over 320 batches, with and without the workers' start;
  resident   device_loader.ResidentTrainSet(...).loader(...): the random draws on the host, one small plan copy, one launch;

then, for a 48 + 48 batch of the resident path: the kernel's time on device events, its bytes moved (the windows read,
the three float planes written) over that time as a fraction of 8 TB/s, the wall time of one whole batch (draws, copy,
launch, synchronise) with nothing else running, the pool's size and its construction time.  With --step-ms (the
ms_per_step of `bench.py --math bf16 --batch 48` from the same session) it says whether a batch is made in less time than
the step takes to consume it.

Usage:  python tools/loader_bench.py [--images 960] [--batch 48] [--reps 200] [--step-ms 16.0] [--skip-host]
"""
import argparse
import json
import os
import pickle
import random
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import _lib, datasets as D, device_loader as DL, ops  # noqa: E402

PEAK_HBM_GBS = 8000.0
SIZES = [(500, 375), (500, 333), (375, 500), (500, 400), (480, 360), (500, 357), (333, 500), (500, 500), (446, 500),
         (500, 281)]     # (width, height), the spread of CUB-200-2011's files


def write_tree(root, n, classes=40, dim=1024):
    rng = np.random.RandomState(0)
    img_root = os.path.join(root, "CUB_200_2011", "images")
    items, boxes, names = [], [], []
    for i in range(n):
        cls = "%03d.Species_%d" % (i % classes + 1, i % classes)
        rel = "%s/img_%05d.jpg" % (cls, i)
        os.makedirs(os.path.join(img_root, cls), exist_ok=True)
        w, h = SIZES[i % len(SIZES)]
        # smooth content with some texture, so that the JPEGs have a photograph's size and decode cost
        low = rng.randint(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(low).resize((w, h), Image.BILINEAR)).astype(np.int16)
        img = np.clip(img + rng.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(img_root, rel), quality=90)
        bw, bh = int(w * (0.45 + 0.4 * rng.rand())), int(h * (0.45 + 0.4 * rng.rand()))
        boxes.append((i + 1, float(rng.randint(0, w - bw)), float(rng.randint(0, h - bh)), float(bw), float(bh)))
        names.append((i + 1, rel))
        items.append({"image": rel, "class": cls, "audio": [], "text": []})
    with open(os.path.join(root, "train.json"), "w") as fp:
        json.dump({"image_base_path": img_root, "audio_base_path": "", "data": items}, fp)
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    with open(os.path.join(root, "train", "audio_features_image.pickle"), "wb") as fp:
        pickle.dump(rng.randn(n, 10, dim).astype(np.float32), fp)
    with open(os.path.join(root, "CUB_200_2011", "bounding_boxes.txt"), "w") as fp:
        for b in boxes:
            fp.write("%d %.1f %.1f %.1f %.1f\n" % b)
    with open(os.path.join(root, "CUB_200_2011", "images.txt"), "w") as fp:
        for nm in names:
            fp.write("%d %s\n" % nm)


def to_device(batch, dev):
    """condGANTrainer.prepare_data's work on a train tuple."""
    real, wrong, emb = batch[0], batch[1], batch[2]

    def move(t):
        t = t.to(dev, non_blocking=True)
        return ops.images_from_uint8_hwc(t.contiguous()) if t.dtype == torch.uint8 else t
    return [move(t) for t in real], [move(t) for t in wrong], emb.float().to(dev, non_blocking=True)


def host_rate(ds, batch, workers, dev, batches):
    """`batches` batches over the tree (repeated as often as that takes).  Worker processes prefetch two batches each,
    so a short run would time the queue, not the workers: the 16-worker run is long, and both the rate after the first
    batch (which leaves the workers' start out but counts the prefetched batches) and the rate of the whole run (which
    counts the start) are reported; the truth lies between them."""
    reps = -(-batches * batch // len(ds))
    loader = D.make_dataloader(torch.utils.data.Subset(ds, list(range(len(ds))) * reps), batch, workers=workers,
                               shuffle=True)
    start = time.perf_counter()
    it = iter(loader)
    first = next(it)
    to_device(first, dev)
    torch.cuda.synchronize()
    t0, samples = time.perf_counter(), 0
    for k, b in enumerate(it):
        if k >= batches:
            break
        to_device(b, dev)
        samples += b[2].shape[0]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    del it
    whole = (samples + first[2].shape[0]) / (t1 - start)
    return {"samples": samples, "seconds": round(t1 - t0, 3), "first_batch_s": round(t0 - start, 3),
            "samples_per_s": round(samples / (t1 - t0), 1), "samples_per_s_with_start": round(whole, 1),
            "images_per_s": round(2 * samples / (t1 - t0), 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=960)
    p.add_argument("--batch", type=int, default=48)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--step-ms", type=float, default=None)
    p.add_argument("--skip-host", action="store_true")
    args = p.parse_args()
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda:0")
    random.seed(0)
    B, S = args.batch, 256
    out = {"tool": "loader_bench", "images": args.images, "batch": B, "size": S}
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, args.images)
        ds = D.BirdsDataset(root, train=True, base_size=64, transform=D.default_image_transform(S),
                            device_normalize=True)
        if not args.skip_host:
            out["host_w0"] = host_rate(ds, B, 0, dev, 4)
            out["host_w16"] = host_rate(ds, B, 16, dev, 320)
        t0 = time.perf_counter()
        rs = DL.ResidentTrainSet(ds, dev, workers=16)
        torch.cuda.synchronize()
        out["construct_s"] = round(time.perf_counter() - t0, 3)
        out["construct_images_per_s"] = round(args.images / (time.perf_counter() - t0), 1)
    out["pool_bytes"] = rs.pool_bytes
    out["pool_bytes_per_image"] = round(rs.pool_bytes / args.images)

    # whole epochs, pipelined: nothing synchronises inside an iteration
    loader = rs.loader(B, shuffle=True)
    for _ in loader:
        pass
    torch.cuda.synchronize()
    epochs = max(1, args.reps * B // args.images)
    t0, samples = time.perf_counter(), 0
    for e in range(epochs):
        loader.set_epoch(e + 1)
        for b in loader:
            samples += b[2].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["resident"] = {"samples": samples, "seconds": round(dt, 4), "samples_per_s": round(samples / dt, 1),
                       "images_per_s": round(2 * samples / dt, 1)}

    # one 48 + 48 batch alone: wall time with a synchronise after every batch (draws + plan copy + launch + kernel)
    idx = list(range(B))
    for _ in range(5):
        rs.batch(idx)
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        rs.batch(idx)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    walls.sort()
    out["batch_wall_ms"] = {"median": round(walls[len(walls) // 2], 4), "p90": round(walls[len(walls) * 9 // 10], 4),
                            "max": round(walls[-1], 4)}
    t0 = time.perf_counter()
    for _ in range(args.reps):
        DL.plan_batch(ds, idx)
    out["plan_ms"] = round((time.perf_counter() - t0) / args.reps * 1e3, 4)

    # the kernel alone, on device events
    plan = torch.from_numpy(DL.plan_batch(ds, idx)[0]).to(dev)

    def launch():
        return ops.image_batch(rs.pool, rs.offsets, rs.sizes, plan, S, 3, rs.tab1, rs.tab2)
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        launch()
    b.record()
    torch.cuda.synchronize()
    k_ms = a.elapsed_time(b) / args.reps
    n = 2 * B
    moved = n * S * S * 3 + n * 3 * 4 * (S * S + S * S // 4 + S * S // 16)
    out["kernel"] = {"name": "image_batch_kernel<3>", "images": n, "ms": round(k_ms, 5), "bytes_moved": moved,
                     "gbytes_per_s": round(moved / (k_ms * 1e-3) / 1e9, 1),
                     "hbm_frac_of_8TBs": round(moved / (k_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                     "note": "back-to-back launches with their output allocation, device events; bytes = the windows read "
                             "+ the three float planes written"}
    if args.step_ms is not None:
        out["step_ms_bf16_b48"] = args.step_ms
        out["batch_made_faster_than_consumed"] = bool(out["batch_wall_ms"]["median"] < args.step_ms)
        for k in ("host_w0", "host_w16"):
            if k in out:
                out[k]["ms_per_batch"] = round(B / out[k]["samples_per_s"] * 1e3, 2)
                out[k]["ms_per_batch_with_start"] = round(B / out[k]["samples_per_s_with_start"] * 1e3, 2)
                out[k]["meets_step_bound"] = bool(out[k]["ms_per_batch_with_start"] < args.step_ms)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
