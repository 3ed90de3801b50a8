"""Speech-image consistency timing (GPU box only): gan_metrics.score_generator with a ConsistencyScorer end to end on a
synthetic test split (seeded G at cfg/birds_3stages.yml widths, seeded Inception-v3 and GoogLeNet weights, random
1024-wide embeddings; --items items of ten sentences each, batch 24), with the time of its parts measured alone on the
same shapes: G, GoogLeNet on the fake and the real images (quantisation included), and the rank passes.  The rank passes
are also timed at the size of the CUB test split (29 330 queries against 29 330 rows), and s2i_rank_rows alone on one
[QUERY_BLOCK, chunk] block of scores, as bytes of scores read per second against the achievable HBM bandwidth.  Seeded
weights: the timing does not depend on them, and the scores they give mean nothing.  Prints one JSON line.

Usage:  python tools/consistency_bench.py [--items 96] [--reps 20] [--split_items 2933] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from googlenet_ref import random_weights  # noqa: E402
from inception_bench import seeded_state_dict, timed  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib, gan_metrics as GM, googlenet as G, model, ops  # noqa: E402
from speech_to_image_translation_without_text_amd import retrieval, trainer as T  # noqa: E402
from speech_to_image_translation_without_text_amd.miscc.config import cfg, cfg_from_file  # noqa: E402

HBM_GBS = 6300.0        # achievable, MI355X
S = 10


def rank_kernel_alone(dev, Q, N, reps):
    """s2i_rank_rows in count mode on a [Q, N] block of random scores, 200 labels: ms and GB/s of scores read."""
    g = torch.Generator(device=dev).manual_seed(3)
    sc = torch.randn(Q, N, device=dev, generator=g)
    rlab = torch.randint(0, 200, (N,), device=dev, generator=g, dtype=torch.int32)
    qlab = torch.randint(0, 200, (Q,), device=dev, generator=g, dtype=torch.int32)
    own = torch.randn(Q, device=dev, generator=g)
    gt = torch.zeros(Q, dtype=torch.int32, device=dev)
    eq = torch.zeros(Q, dtype=torch.int32, device=dev)
    ms = timed(lambda: ops.rank_rows(sc, None, qlab, rlab, 0, own, gt, eq, "count"), reps)
    row = torch.randint(0, N, (Q,), device=dev, generator=g, dtype=torch.int32)
    gather_ms = timed(lambda: ops.rank_rows(sc, row, None, None, 0, own, None, None, "gather"), reps)
    gbs = Q * N * 4 / (ms * 1e-3) / 1e9
    return dict(Q=Q, N=N, count_ms=round(ms, 4), count_gb_per_s=round(gbs, 1), count_share_of_hbm=round(gbs / HBM_GBS, 3),
                gather_ms=round(gather_ms, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=96)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--split_items", type=int, default=2933, help="items of the full-split rank timing (CUB test: 2933)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda:0")
    cfg_from_file(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "cfg", "birds_3stages.yml"))
    g = torch.Generator().manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(dev), "items": args.items, "sentences": S, "batch": args.batch}

    # the rank kernel alone, on the blocks Gallery.rank gives it
    rec["rank_kernel"] = [rank_kernel_alone(dev, retrieval.QUERY_BLOCK, n, args.reps)
                          for n in (S * args.split_items, retrieval.GALLERY_CHUNK_ROWS)]

    # the rank passes at the size of a whole split: scores, gather, scores again, count
    n_split = args.split_items
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((n_split, S, G.FEATURES), dtype=np.float32)
    labels = rng.integers(0, 200, n_split)
    gal = retrieval.Gallery(emb, dev, views="all")
    q = torch.randn(n_split * S, G.FEATURES, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    own = np.arange(n_split * S)
    qlab, rlab = np.repeat(labels, S), np.repeat(labels, S)
    reps = max(2, args.reps // 4)
    rank_ms = timed(lambda: gal.rank(q, own, qlab, rlab), reps)
    search_ms = timed(lambda: gal.search(q, 50), reps)
    rec["rank_split"] = dict(queries=n_split * S, rows=n_split * S, rank_ms=round(rank_ms, 2),
                             search_top50_ms=round(search_ms, 2))
    del gal, q, emb
    torch.cuda.empty_cache()

    # end to end
    torch.manual_seed(0)
    netG = T.G_NET()
    netG.apply(T.weights_init)
    netG = netG.to(dev).eval()
    incep = model.INCEPTION_V3(weights=seeded_state_dict(1))
    gnet = G.GoogLeNetFeatures(random_weights(0), dev)
    B = args.batch
    batches = max(1, args.items // B)
    items = batches * B
    emb = torch.randn(items, S, cfg.TEXT.DIMENSION, generator=g)
    labels = np.arange(items) % 50
    loader = []
    for k in range(batches):
        imgs = [torch.rand(B, 3, 64 * 2 ** i, 64 * 2 ** i, generator=g) * 2 - 1 for i in range(cfg.TREE.BRANCH_NUM)]
        loader.append((imgs, emb[k * B:(k + 1) * B], ["b/%d" % i for i in range(B)]))

    def run(with_consistency):
        sc = GM.GeneratorScorer(incep, items * S, dev)
        cons = GM.ConsistencyScorer(gnet, emb.numpy(), labels, dev) if with_consistency else None
        GM.score_generator(netG, loader, sc, seed=0, consistency=cons)
        res = cons.result() if cons is not None else None
        torch.cuda.synchronize()
        return res

    e2e = {}
    for name, flag in (("with", True), ("without", False)):
        run(flag)                            # warm-up: code objects, allocator, weight packing
        t0 = time.perf_counter()
        res = run(flag)
        e2e[name] = time.perf_counter() - t0
        if flag:
            rec["scores_of_seeded_weights"] = res

    # the parts alone, on the shapes score_generator gives them
    per = max(1, GM.G_STACK_IMAGES // B)
    groups = [min(per, S - s0) for s0 in range(0, S, per)]
    z = torch.randn(per * B, cfg.GAN.Z_DIM, generator=g).to(dev)
    eps = torch.randn(per * B, cfg.GAN.EMBEDDING_DIM, generator=g).to(dev)
    c = torch.cat([emb[:B, s] for s in range(per)]).contiguous().to(dev)
    with torch.no_grad():
        fake = netG(z, c, eps, True)[0][-1]
    real = loader[0][0][-1].to(dev)

    def g_pass():
        with torch.no_grad():
            for k in groups:
                netG(z[:k * B], c[:k * B], eps[:k * B], True)

    def googlenet_pass():
        gnet.rows(ops.images_to_uint8_hwc(real.permute(0, 2, 3, 1).contiguous()))
        for k in groups:
            gnet.rows(ops.images_to_uint8_hwc(fake[:k * B]))

    cons = GM.ConsistencyScorer(None, emb.numpy(), labels, dev)
    rows = torch.randn(items * S, G.FEATURES, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    cons.add_rows(rows, np.repeat(np.arange(items), S), np.tile(np.arange(S), items))
    cons.add_rows(rows[:items], np.arange(items), real=True)
    reps = max(2, args.reps // 4)
    tg = timed(g_pass, reps) * batches
    tn = timed(googlenet_pass, reps) * batches
    tr = timed(cons.result, reps)
    n_fake = items * S
    rec.update(fake_images=n_fake, real_images=items, e2e_ms=round(e2e["with"] * 1e3, 1),
               e2e_images_per_s=round(n_fake / e2e["with"], 1), e2e_without_consistency_ms=round(e2e["without"] * 1e3, 1),
               g_ms=round(tg, 1), googlenet_ms=round(tn, 1), rank_ms=round(tr, 2),
               rank_share_of_googlenet=round(tr / tn, 4))
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
