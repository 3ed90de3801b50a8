"""KID and precision / recall / density / coverage timing (GPU box only): gan_metrics.kid and gan_metrics.prdc on seeded
rows at the size of the CUB test split (29 330 fake rows against 2 933 real ones, 2 048 wide), every pass of each timed
alone (the three kernel sums of KID; the norms, the two radius passes and the two ball passes of prdc), and the pieces of
one [QUERY_BLOCK, rows] block alone: the fp32 matrix launch that writes the scores and each fold of csrc/s2i_manifold.hip
(with s2i_topk_rows at nearest_k) as bytes of scores moved per second against the achievable HBM bandwidth.  Also the
deviation of kid from the float64 reference on the GPU suite's D = 2048 case (tests/manifold_ref.py, WIDE_SHAPES), which
the suite's bound is set from.  Times are device events around repeated calls after a warm-up; seeded rows: the timing
does not depend on them, and the metric values they give mean nothing.  Prints one JSON line.

Usage:  python tools/manifold_bench.py [--fake 29330] [--real 2933] [--reps 20] [--nearest_k 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import manifold_ref as M  # noqa: E402
from inception_bench import timed  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib, gan_metrics as GM, ops, retrieval  # noqa: E402

HBM_GBS = 6300.0        # achievable, MI355X
D = GM.POOL3


def block_alone(dev, q_rows, rows, chunks, k, reps):
    """One [Q, N] block: the matrix launch and every fold on it, ms each; the folds also as GB/s of scores moved."""
    Q, N = q_rows.shape[0], rows.shape[0]
    scratch = torch.empty(Q * N, dtype=torch.float32, device=dev)
    _, n, packed = chunks[0]
    assert n == N
    out = dict(Q=Q, N=N)
    ms = timed(lambda: ops.score_rows(q_rows, packed, N, scratch), reps)
    out.update(scores_ms=round(ms, 4), scores_tflops=round(2.0 * Q * N * D / (ms * 1e-3) / 1e12, 1))
    sc = ops.score_rows(q_rows, packed, N, scratch)
    sums = torch.zeros(Q, dtype=torch.float64, device=dev)
    qn, rn = GM._norm2(q_rows, Q), GM._norm2(rows, 4096)
    bound = -0.5 * (qn.mean() + rn)             # radii of the order of the distances: the comparison goes both ways
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    best = torch.full((Q,), float("-inf"), device=dev)
    pair = (torch.empty((Q, k), device=dev), torch.empty((Q, k), dtype=torch.int32, device=dev))
    # ball and topk on distances as the passes give them; sqdist last: repeated in place it drives the block to -inf
    folds = (("polykernel", 1, lambda: ops.polykernel_rows(sc, 1.0 / D, sums, own_base=0)),
             ("ball", 1, lambda: ops.ball_rows(sc, bound, count=count, best=best)),
             ("topk", 1, lambda: ops.topk_rows(sc, k, out=pair)),
             ("sqdist", 2, lambda: ops.sqdist_rows(sc, qn, rn, own_base=0)))          # read and written back
    for name, passes, fn in folds:
        if name == "ball":
            ops.sqdist_rows(sc, qn, rn, own_base=0)
        ms = timed(fn, reps)
        gbs = passes * Q * N * 4 / (ms * 1e-3) / 1e9
        out.update({name + "_ms": round(ms, 4), name + "_gb_per_s": round(gbs, 1),
                    name + "_share_of_hbm": round(gbs / HBM_GBS, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fake", type=int, default=29330)
    ap.add_argument("--real", type=int, default=2933)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nearest_k", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda:0")
    k, reps = args.nearest_k, args.reps
    chunk, block = retrieval.GALLERY_CHUNK_ROWS, retrieval.QUERY_BLOCK
    g = torch.Generator(device=dev).manual_seed(0)
    real = torch.randn(args.real, D, device=dev, generator=g)
    fake = 0.9 * torch.randn(args.fake, D, device=dev, generator=g)
    fake[:, 0] += 0.3
    rec = {"device": torch.cuda.get_device_name(dev), "fake_rows": args.fake, "real_rows": args.real, "dim": D,
           "nearest_k": k, "chunk_rows": chunk, "query_block": block, "reps": reps}

    pack_ms = timed(lambda: (retrieval.pack_device_rows(real, chunk), retrieval.pack_device_rows(fake, chunk)), reps)
    (rq, rc), (fq, fc) = retrieval.pack_device_rows(real, chunk), retrieval.pack_device_rows(fake, chunk)
    scratch = GM._pair_scratch(real, fake, chunk, block)
    rec["pack_both_sets_ms"] = round(pack_ms, 3)
    rec["block"] = block_alone(dev, fq[:block], fake, fc, k, reps * 10)

    inv_d = 1.0 / D
    kid_passes = {}
    for name, q, c, own in (("fake_fake", fq, fc, True), ("real_real", rq, rc, True), ("fake_real", fq, rc, False)):
        kid_passes[name + "_ms"] = round(timed(lambda: GM._kernel_sums(q, c, own, inv_d, block, scratch), reps), 3)
    rec["kid_passes"] = kid_passes
    rec["kid_ms"] = round(timed(lambda: GM.kid(fake, real), reps), 3)           # packing and the D2H of the sums included

    norms_ms = timed(lambda: (GM._norm2(real, block), GM._norm2(fake, block)), reps)
    rn, fn = GM._norm2(real, block), GM._norm2(fake, block)
    p = {"norms_ms": round(norms_ms, 3)}
    p["real_radii_ms"] = round(timed(lambda: GM._radii(rq, rc, rn, k, block, scratch), reps), 3)
    p["fake_radii_ms"] = round(timed(lambda: GM._radii(fq, fc, fn, k, block, scratch), reps), 3)
    rb, fb = GM._radii(rq, rc, rn, k, block, scratch), GM._radii(fq, fc, fn, k, block, scratch)
    p["fake_in_real_balls_ms"] = round(timed(lambda: GM._balls(fq, fn, rc, rn, rb, block, scratch), reps), 3)
    p["real_in_fake_balls_ms"] = round(timed(lambda: GM._balls(rq, rn, fc, fn, fb, block, scratch), reps), 3)
    rec["prdc_passes"] = p
    rec["prdc_ms"] = round(timed(lambda: GM.prdc(real, fake, k), reps), 3)
    res = GM.prdc(real, fake, k)
    rec["values_of_seeded_rows"] = dict(kid=GM.kid(fake, real), **{key: res[key] for key in GM.PRDC_KEYS})
    del rq, rc, fq, fc, scratch, res, real, fake
    torch.cuda.empty_cache()

    # what the GPU suite's full-width KID bound is set from
    s = M.WIDE_SHAPES
    wr, wf = M.real_valued_rows(s["seed"], s["D"], s["real"], s["fake"])
    want = M.kid_ref(wf, wr)
    got = GM.kid(torch.from_numpy(wf).to(dev), torch.from_numpy(wr).to(dev), chunk_rows=s["chunk_rows"],
                 query_block=s["query_block"])
    rec["kid_wide"] = dict(real=s["real"], fake=s["fake"], dim=s["D"], seed=s["seed"], kid=got, kid_ref=float(want),
                           kid_wide_deviation=abs(got - float(want)), worst_case_bound=M.kid_fp32_bound(wf, wr))
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
