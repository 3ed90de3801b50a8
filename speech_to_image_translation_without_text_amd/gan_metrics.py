"""Score a trained generator on the test split: Inception score, NLPP and FID, the paper's metrics (StackGAN_v2/
trainer.py:88-159, whose evaluate() computes them only in dead code after its early return, :803-825).

    python -m speech_to_image_translation_without_text_amd.gan_metrics --cfg cfg/birds_3stages.yml \\
        --netG output/Model/netG_600.pth --inception inception_v3_google-1a9a5a14.pth --data_dir data/birds \\
        [--real_stats stats.npz] [--save_images] [--seed S] [--max_items K] [--out metrics.json]
        [--googlenet bvlc_googlenet.caffemodel [--consistency_cosine]] [--kid] [--prdc] [--nearest_k K]

G runs in .eval() over every embedding column of every test item, its last-stage images go through the native
Inception-v3 (inception.py), and the pool3 rows of each pass are folded into fp64 moments on the device
(s2i_moments_accumulate: column sums and X^T X), so no pool3 row is kept and the Gaussian of each set costs one D2H copy
of D (D + 1) doubles.  The softmax rows, which the split-wise IS and NLPP need in order, are kept on the device.
The values are those of torchvision's Inception-v3 weights: the paper used TF Inception models, so they are not
comparable to its numbers.

With --googlenet the record also says whether the pictures show what was said (`ConsistencyScorer`): every fake image,
quantised as its PNG would be, goes through BVLC GoogLeNet on the device (googlenet.GoogLeNetFeatures.rows), and its
ten-view pool5 row is ranked against the speech embeddings of the whole split (retrieval.Gallery.rank, s2i_rank_rows):
recall@1/5/10, the median rank and the closed-form R-precision under `fake_*` keys, with the same scores of the real
images under `real_*` keys as the ceiling the speech encoder allows.

With --kid, --prdc or --nearest_k the pool3 rows are kept on the device after all (`FeatureRows`) and the record gains
`kid` (the unbiased cubic-kernel MMD^2 over the full samples) and `precision`, `recall`, `density`, `coverage` (k-nearest-
neighbour manifolds): `kid` and `prdc` below fold the chunked scores of the fp32 matrix kernel with s2i_polykernel_rows,
s2i_sqdist_rows + s2i_topk_rows and s2i_ball_rows, so no rows x rows matrix exists.  The real
set has one row per item and the fake set one per sentence.
"""
import argparse
import json
import math
import os
import queue
import random
import threading

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream
from .trainer import (_frechet_from_moments, compute_inception_score, negative_log_posterior_probability,
                      save_singleimages)

POOL3, CLASSES = 2048, 1000
GOOGLENET_FEATURES = 1024      # googlenet.FEATURES: pool5/7x7_s1
# Sentences of one batch are stacked into one G launch up to this many images.  The largest G tensor at
# cfg/birds_3stages.yml widths is the stage-3 joint input, 128 x 128 x 160 fp32 = 10.5 MB per image, so 96 images stay
# at 1.0 GB, half of the 2 GiB that the kernels' 32-bit byte offsets reach.
G_STACK_IMAGES = 96


class FeatureMoments:
    """Count, column sums and Gram matrix of a stream of D-wide fp32 rows, accumulated in fp64 on `device`."""

    def __init__(self, D, device):
        self.D = int(D)
        self.device = torch.device(device)
        self._buf = torch.zeros(self.D + 1, self.D, dtype=torch.float64, device=self.device)   # [colsum; gram]
        self.colsum, self.gram = self._buf[0], self._buf[1:]
        self.n = 0

    def update(self, rows):
        """Fold (N, D) fp32 device rows (row stride >= D) into the moments: one launch on the current stream, no sync."""
        if (rows.dim() != 2 or rows.shape[1] != self.D or rows.dtype != torch.float32 or rows.stride(1) != 1
                or rows.device != self.device):
            raise ValueError("rows must be (N, %d) fp32 with unit column stride on %s, got %s %s on %s"
                             % (self.D, self.device, tuple(rows.shape), rows.dtype, rows.device))
        if rows.shape[0] == 0:
            return
        check(_lib.load().s2i_moments_accumulate(ptr(rows), rows.shape[0], self.D, rows.stride(0), ptr(self.colsum),
                                                 ptr(self.gram), stream()), "s2i_moments_accumulate")
        self.n += rows.shape[0]

    def mean_cov(self):
        """float64 (mu, sigma, n): sigma normalised by n - 1, as np.cov(rowvar=False)."""
        if self.n < 2:
            raise ValueError("a covariance needs at least 2 rows, have %d" % self.n)
        buf = self._buf.cpu().numpy()
        g = np.triu(buf[1:])           # the kernel maintains the tiles on and above the diagonal
        g = g + np.triu(g, 1).T
        s, n = buf[0], self.n
        return s / n, (g - np.outer(s, s) / n) / (n - 1), n

    def save(self, path):
        mu, sigma, n = self.mean_cov()
        save_stats(path, mu, sigma, n)

    @staticmethod
    def load(path, D=None):
        return load_stats(path, D)


def save_stats(path, mu, sigma, n):
    np.savez(path, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64), n=np.int64(n))


def load_stats(path, D=None):
    """(mu, sigma, n) of a .npz written by save_stats; ValueError unless mu is (D,), sigma (D, D) and n >= 2."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("mu", "sigma", "n") if k not in z.files]
        if missing:
            raise ValueError("%s lacks %s" % (path, missing))
        mu, sigma, n = z["mu"].astype(np.float64), z["sigma"].astype(np.float64), int(z["n"])
    d = mu.shape[0] if mu.ndim == 1 else -1
    if d < 1 or sigma.shape != (d, d):
        raise ValueError("%s: mu %s and sigma %s are not (D,) and (D, D)" % (path, mu.shape, sigma.shape))
    if D is not None and d != D:
        raise ValueError("%s holds %d-d statistics, expected %d" % (path, d, D))
    if n < 2:
        raise ValueError("%s: statistics of %d rows (need >= 2)" % (path, n))
    return mu, sigma, n


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """The Frechet distance of compute_frethet_distance from two fitted Gaussians."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape or sigma1.shape != mu1.shape * 2:
        raise ValueError("mismatched statistics: mu %s / %s, sigma %s / %s"
                         % (mu1.shape, mu2.shape, sigma1.shape, sigma2.shape))
    return float(_frechet_from_moments(mu1, sigma1, mu2, sigma2, eps))


def nhwc4_as_nchw(img):
    """G's nhwc=True output (B, H, W, 4) as the (B, 3, H, W) view Inception's input stage reads (any strides)."""
    return img[..., :3].permute(0, 3, 1, 2)


class FeatureRows:
    """The D-wide fp32 rows of a stream themselves, on `device` in arrival order: what KID and the nearest-neighbour
    manifolds need and FeatureMoments drops.  The buffer holds `capacity` rows and doubles when more arrive (one device
    copy per doubling).  n rows so far; rows() is the [n, D] view of them."""

    def __init__(self, D, device, capacity=1024):
        self.D = int(D)
        self.device = torch.device(device)
        self._buf = torch.empty(max(1, int(capacity)), self.D, dtype=torch.float32, device=self.device)
        self.n = 0

    def __len__(self):
        return self.n

    def append(self, rows):
        """Copy (N, D) fp32 device rows (any row stride) behind the kept ones: device to device, no sync."""
        if rows.dim() != 2 or rows.shape[1] != self.D or rows.dtype != torch.float32 or rows.device != self.device:
            raise ValueError("rows must be (N, %d) fp32 on %s, got %s %s on %s"
                             % (self.D, self.device, tuple(rows.shape), rows.dtype, rows.device))
        n = rows.shape[0]
        if self.n + n > self._buf.shape[0]:
            grown = torch.empty(max(2 * self._buf.shape[0], self.n + n), self.D, dtype=torch.float32, device=self.device)
            grown[:self.n].copy_(self._buf[:self.n])
            self._buf = grown
        self._buf[self.n:self.n + n].copy_(rows)
        self.n += n

    def rows(self):
        return self._buf[:self.n]


def _device_rows(name, rows):
    """A FeatureRows or an fp32 [n, D] device tensor as that tensor."""
    rows = rows.rows() if isinstance(rows, FeatureRows) else rows
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.dtype != torch.float32:
        raise ValueError("%s: rows must be a FeatureRows or an fp32 [n, D] tensor" % name)
    if not rows.is_cuda:
        raise _lib.S2IError("%s runs on the MI355X kernels: there is no CPU fallback (rows on %s)" % (name, rows.device))
    return rows.detach()


def _pair_blocks(queries, chunks, query_block, scratch):
    """(q0, q1, start, scores [q1 - q0, n]) for every (query block, chunk) pair: one launch of the fp32 matrix kernel each,
    all into the one scratch block."""
    for q0 in range(0, queries.shape[0], query_block):
        q1 = min(queries.shape[0], q0 + query_block)
        for start, n, packed in chunks:
            yield q0, q1, start, ops.score_rows(queries[q0:q1], packed, n, scratch)


def _pair_args(name, a, b, chunk_rows, query_block):
    from . import retrieval
    a, b = _device_rows(name, a), _device_rows(name, b)
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError("%s: the two sets must share width and device, got %s on %s and %s on %s"
                         % (name, tuple(a.shape), a.device, tuple(b.shape), b.device))
    chunk_rows = int(chunk_rows or retrieval.GALLERY_CHUNK_ROWS)
    query_block = int(query_block or retrieval.QUERY_BLOCK)
    if chunk_rows < 1 or query_block < 1:
        raise ValueError("%s: chunk_rows and query_block must be >= 1" % name)
    return a, b, chunk_rows, query_block


def _pair_scratch(a, b, chunk_rows, query_block):
    need = min(max(a.shape[0], b.shape[0]), query_block) * min(max(a.shape[0], b.shape[0]), chunk_rows)
    return torch.empty(need, dtype=torch.float32, device=a.device)


def _kernel_sums(queries, chunks, own, inv_d, query_block, scratch):
    """fp64 [Q] on the device: for every query row the sum of the cubic kernel against every row of `chunks`; own=True:
    the chunks hold the queries themselves, and a row's kernel with itself is left out."""
    sums = torch.zeros(queries.shape[0], dtype=torch.float64, device=queries.device)
    for q0, q1, start, sc in _pair_blocks(queries, chunks, query_block, scratch):
        ops.polykernel_rows(sc, inv_d, sums[q0:q1], base=start, own_base=q0 if own else None)
    return sums


def _norm2(rows, block):
    """fp32 [n]: the squared norm of every row, formed in fp64 on the device, `block` rows at a time."""
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    for s in range(0, rows.shape[0], block):
        out[s:s + block] = rows[s:s + block].double().square_().sum(dim=1)
    return out


def _radii(queries, chunks, norms, k, query_block, scratch):
    """fp32 [n]: -r^2 of every row of a set, the k-th largest negated squared distance to another row of it (the chunks
    hold the queries themselves)."""
    Q, dev = queries.shape[0], queries.device
    best = (torch.empty((Q, k), dtype=torch.float32, device=dev), torch.empty((Q, k), dtype=torch.int32, device=dev))
    for q0, q1, start, sc in _pair_blocks(queries, chunks, query_block, scratch):
        ops.sqdist_rows(sc, norms[q0:q1], norms, base=start, own_base=q0)
        pair = (best[0][q0:q1], best[1][q0:q1])
        if start == 0:
            ops.topk_rows(sc, k, base=start, out=pair)
        else:
            ops.topk_rows(sc, k, base=start, best=pair)
    return best[0][:, k - 1].contiguous()


def _balls(queries, q_norms, chunks, norms, bound, query_block, scratch):
    """(count int32 [Q], best fp32 [Q]): how many balls of the other set (-r^2 in `bound`) hold each query, and minus its
    squared distance to the nearest row of that set."""
    Q, dev = queries.shape[0], queries.device
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    best = torch.full((Q,), float("-inf"), dtype=torch.float32, device=dev)
    for q0, q1, start, sc in _pair_blocks(queries, chunks, query_block, scratch):
        ops.sqdist_rows(sc, q_norms[q0:q1], norms, base=start)
        ops.ball_rows(sc, bound, base=start, count=count[q0:q1], best=best[q0:q1])
    return count, best


def kid(x_rows, y_rows, chunk_rows=None, query_block=None):
    """The kernel inception distance (Binkowski et al. 2018) of two sets of feature rows as a float64: the unbiased
    estimator of MMD^2 with the kernel k(a, b) = (a . b / D + 1)^3,

        Sxx / (m (m - 1)) + Syy / (n (n - 1)) - 2 Sxy / (m n),

    Sxx and Syy the sums of k over the ordered pairs of DIFFERENT rows of one set, Sxy over all pairs across the sets.
    x_rows [m, D] and y_rows [n, D]: FeatureRows or fp32 device tensors, m, n >= 2.

    This is the estimator over the full samples: no subsets are drawn, so there is no seed.  It has the same expectation
    as the usual protocol that averages the estimator over random subsets, with lower variance (every pair is used);
    that protocol's standard deviation over subsets is not produced.

    Every (query_block, chunk_rows) block of scores comes from one launch of the fp32 matrix kernel and is folded by
    s2i_polykernel_rows into per-query fp64 sums, which are copied to the host (m or n doubles per pass) and added there
    in float64; no [m, n] matrix exists.  There is no CPU fallback."""
    from . import retrieval
    x, y, chunk_rows, query_block = _pair_args("kid", x_rows, y_rows, chunk_rows, query_block)
    m, n, D = x.shape[0], y.shape[0], x.shape[1]
    if m < 2 or n < 2:
        raise ValueError("kid: each set needs at least 2 rows, have %d and %d" % (m, n))
    inv_d = 1.0 / D
    with torch.cuda.device(x.device):
        xq, xc = retrieval.pack_device_rows(x, chunk_rows)
        yq, yc = retrieval.pack_device_rows(y, chunk_rows)
        scratch = _pair_scratch(x, y, chunk_rows, query_block)
        sxx, syy, sxy = (math.fsum(_kernel_sums(q, c, own, inv_d, query_block, scratch).cpu().tolist())
                         for q, c, own in ((xq, xc, True), (yq, yc, True), (xq, yc, False)))
    return sxx / (m * (m - 1.0)) + syy / (n * (n - 1.0)) - 2.0 * sxy / (float(m) * n)     # Python floats: float64


def prdc(real_rows, fake_rows, nearest_k=5, chunk_rows=None, query_block=None):
    """Precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) of fake feature rows
    against real ones, from k-nearest-neighbour balls: r_i is the distance from row i to its nearest_k-th nearest OTHER
    row of its own set.  With N real and M fake rows,

        precision  the share of fake rows that lie in the ball of at least one real row,
        density    the number of real balls that hold a fake row, summed over the fake rows, over nearest_k M,
        recall     the share of real rows that lie in the ball of at least one fake row,
        coverage   the share of real rows whose nearest fake row lies inside their own ball,

    a row on the surface of a ball counting as inside.  One nearest_k serves all four, as in the `prdc` reference
    implementation (default 5; 3 is Kynkaanniemi's setting); 1 <= nearest_k <= 64 and each set holds more rows than that.
    real_rows [N, D] and fake_rows [M, D]: FeatureRows or fp32 device tensors.

    Four passes over (query_block, chunk_rows) blocks of scores from the fp32 matrix kernel, each block rewritten in
    place to negated squared distances (s2i_sqdist_rows, |a|^2 + |b|^2 - 2 a.b in fp32, the squared norms formed in fp64
    on the device and stored as fp32): real against real and fake against fake are folded by s2i_topk_rows into the k
    nearest other rows (the radii), fake against real and real against fake by s2i_ball_rows into counts and the nearest
    distance.  Nothing of size N x M exists beyond one block.

    Returns the four values as floats with `nearest_k`, and the per-query device tensors they come from:
    real_bound [N], fake_bound [M] fp32 (-r_i^2), fake_count [M] int32 and fake_best [M] fp32 (the real balls that hold
    each fake row; minus its squared distance to the nearest real row), real_count [N] and real_best [N] (the same for
    each real row among the fake ones).  There is no CPU fallback."""
    from . import retrieval
    real, fake, chunk_rows, query_block = _pair_args("prdc", real_rows, fake_rows, chunk_rows, query_block)
    k = int(nearest_k)
    if not 1 <= k <= _lib.TOPK_MAX:
        raise ValueError("prdc: nearest_k must lie in 1..%d, got %d" % (_lib.TOPK_MAX, k))
    N, M = real.shape[0], fake.shape[0]
    if N <= k or M <= k:
        raise ValueError("prdc: each set must hold more than nearest_k = %d rows, have %d real and %d fake" % (k, N, M))
    dev = real.device
    with torch.cuda.device(dev):
        rq, rc = retrieval.pack_device_rows(real, chunk_rows)
        fq, fc = retrieval.pack_device_rows(fake, chunk_rows)
        scratch = _pair_scratch(real, fake, chunk_rows, query_block)

        rn, fn = _norm2(real, query_block), _norm2(fake, query_block)
        real_bound = _radii(rq, rc, rn, k, query_block, scratch)
        fake_bound = _radii(fq, fc, fn, k, query_block, scratch)
        fake_count, fake_best = _balls(fq, fn, rc, rn, real_bound, query_block, scratch)
        real_count, real_best = _balls(rq, rn, fc, fn, fake_bound, query_block, scratch)
        hit_f = int((fake_count > 0).sum().item())
        tot_f = int(fake_count.sum(dtype=torch.int64).item())
        hit_r = int((real_count > 0).sum().item())
        cov_r = int((real_best >= real_bound).sum().item())
    return dict(precision=hit_f / float(M), recall=hit_r / float(N), density=tot_f / (float(k) * M), coverage=cov_r / float(N),
                nearest_k=k, real_bound=real_bound, fake_bound=fake_bound, fake_count=fake_count, fake_best=fake_best,
                real_count=real_count, real_best=real_best)


_kid, _prdc = kid, prdc      # GeneratorScorer.result has flags of these names
PRDC_KEYS = ("precision", "recall", "density", "coverage", "nearest_k")


class GeneratorScorer:
    """IS / NLPP over the fake softmax rows (kept on the device in arrival order, in a buffer preallocated for n_fake_max
    rows that grows if more arrive) and FID between the streamed fake and real pool3 moments.  `inception` is a
    model.INCEPTION_V3 with weights or an inception.InceptionNet.  keep_rows=True also keeps every pool3 row on the
    device (two FeatureRows, 8 KB a row), which `result(kid=True)` and `result(prdc=True)` need; it changes nothing
    else."""

    def __init__(self, inception, n_fake_max, device=None, keep_rows=False):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.net = inception.net(self.device) if hasattr(inception, "net") else inception
        self.soft = torch.empty(max(1, int(n_fake_max)), CLASSES, device=self.device)
        self.n_fake = 0
        self.fake = FeatureMoments(POOL3, self.device)
        self.real = FeatureMoments(POOL3, self.device)
        self._pool3 = self._soft_real = None
        self.fake_rows = FeatureRows(POOL3, self.device, n_fake_max) if keep_rows else None
        self.real_rows = FeatureRows(POOL3, self.device) if keep_rows else None

    def _scratch(self, n):
        if self._pool3 is None or self._pool3.shape[0] < n:
            self._pool3 = torch.empty(n, POOL3, device=self.device)
            self._soft_real = torch.empty(n, CLASSES, device=self.device)
        return self._pool3[:n]

    def _images(self, images):
        imgs = [images] if torch.is_tensor(images) else list(images)
        return imgs, sum(t.shape[0] for t in imgs)

    def add_fake(self, images):
        """One Inception pass over (B, 3, H, W) fp32 images in [-1, 1] (or a list of them, scored as their concatenation):
        softmax rows appended to the kept rows, pool3 rows folded into the fake moments."""
        imgs, n = self._images(images)
        if self.n_fake + n > self.soft.shape[0]:      # more than announced: grow (one device copy per doubling)
            grown = torch.empty(max(2 * self.soft.shape[0], self.n_fake + n), CLASSES, device=self.device)
            grown[:self.n_fake].copy_(self.soft[:self.n_fake])
            self.soft = grown
        pool3 = self._scratch(n)
        self.net.run(imgs, self.soft[self.n_fake:self.n_fake + n], pool3)
        self.fake.update(pool3)
        if self.fake_rows is not None:
            self.fake_rows.append(pool3)
        self.n_fake += n

    def add_real(self, images):
        imgs, n = self._images(images)
        pool3 = self._scratch(n)
        self.net.run(imgs, self._soft_real[:n], pool3)
        self.real.update(pool3)
        if self.real_rows is not None:
            self.real_rows.append(pool3)

    def fake_predictions(self):
        return self.soft[:self.n_fake].cpu().double().numpy()

    def result(self, num_splits=10, real_stats=None, kid=False, prdc=False, nearest_k=5):
        """{is_mean, is_std, nlpp_mean, nlpp_std, fid, n_fake, n_real} plus the fitted 'fake_stats' / 'real_stats'
        (mu, sigma, n).  real_stats, if given, replaces the streamed real moments.  kid=True adds `kid` (the module's
        kid of the kept fake rows against the kept real rows), prdc=True adds `precision`, `recall`, `density`,
        `coverage` and `nearest_k`; both need keep_rows=True and real rows that were scored here.  The real set has one
        row per item and the fake set one per sentence: recall and coverage see that many fakes per real image."""
        if kid or prdc:
            if self.fake_rows is None:
                raise ValueError("GeneratorScorer: kid and prdc need the pool3 rows: construct with keep_rows=True")
            if len(self.real_rows) == 0:
                raise ValueError("GeneratorScorer: kid and prdc need the real rows, and no real image was scored "
                                 "(precomputed real_stats hold moments, not rows)")
        pred = self.fake_predictions()
        is_mean, is_std = compute_inception_score(pred, num_splits)
        nlpp_mean, nlpp_std = negative_log_posterior_probability(pred, num_splits)
        fake = self.fake.mean_cov()
        real = real_stats if real_stats is not None else self.real.mean_cov()
        fid = frechet_distance(fake[0], fake[1], real[0], real[1])
        out = dict(is_mean=float(is_mean), is_std=float(is_std), nlpp_mean=float(nlpp_mean), nlpp_std=float(nlpp_std),
                   fid=fid, n_fake=int(fake[2]), n_real=int(real[2]), fake_stats=fake, real_stats=real)
        if kid:
            out["kid"] = _kid(self.fake_rows, self.real_rows)
        if prdc:
            res = _prdc(self.real_rows, self.fake_rows, nearest_k)
            out.update((key, res[key]) for key in PRDC_KEYS)
        return out


class ConsistencyScorer:
    """Speech-image consistency of generated images: image query, utterance candidates.

    The gallery holds every utterance embedding of the split (embeddings [N, S, C], row i * S + s, Gallery(views="all")),
    C = 1024: the space the speech encoder is trained to share with GoogLeNet's pool5.  The image generated from
    utterance s of item i is a query whose own candidate is row i * S + s; it is ranked against the rows of OTHER
    classes (labels [N]; another description of the same species is not a wrong answer, and a tie counts against the
    query): retrieval.Gallery.rank and retrieval.rank_metrics have the definitions.  The real image of each item, queried
    once per sentence, gives the `real_*` scores: the ceiling the encoder allows, without which the fake scores cannot be
    read.  `googlenet` is a googlenet.GoogLeNetFeatures on `device` (None where only add_rows is used).  The fp32 rows are
    kept on the device (4 KB each).  There is no CPU fallback."""

    def __init__(self, googlenet, embeddings, labels, device=None, cosine=False, chunk_rows=None):
        from . import retrieval
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        emb = np.asarray(embeddings if isinstance(embeddings, np.ndarray) else [np.asarray(e) for e in embeddings],
                         dtype=np.float32)
        if emb.ndim != 3:
            raise ValueError("ConsistencyScorer: embeddings must be [N, S, C], got %s" % (emb.shape,))
        labels = np.asarray(labels).reshape(-1)
        if labels.shape[0] != emb.shape[0]:
            raise ValueError("ConsistencyScorer: %d labels for %d items" % (labels.shape[0], emb.shape[0]))
        self.gallery = retrieval.Gallery(emb, self.device, views="all", cosine=cosine,
                                         chunk_rows=chunk_rows or retrieval.GALLERY_CHUNK_ROWS)
        self.net = googlenet
        self.items, self.sentences, self.dim = emb.shape
        if googlenet is not None and self.dim != GOOGLENET_FEATURES:
            raise ValueError("ConsistencyScorer: the embeddings are %d wide, GoogLeNet's pool5 rows %d"
                             % (self.dim, GOOGLENET_FEATURES))
        self.labels = np.unique(labels, return_inverse=True)[1].reshape(-1).astype(np.int32)
        self.row_labels = np.repeat(self.labels, self.sentences)
        self._fake, self._real = [], []

    def _index(self, name, values, n, limit):
        v = np.asarray(values.cpu() if torch.is_tensor(values) else values).reshape(-1).astype(np.int64)
        if v.shape[0] != n or (n and (v.min() < 0 or v.max() >= limit)):
            raise ValueError("ConsistencyScorer: %d rows need %d %s in 0..%d" % (n, n, name, limit - 1))
        return v

    def add_rows(self, rows, items, sentences=None, real=False):
        """Precomputed feature rows [n, C] (kept as fp32 on the device): fake rows of (items[j], sentences[j]), or with
        real=True the real rows of items[j] (`sentences` is not used)."""
        rows = torch.as_tensor(rows)
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError("ConsistencyScorer: rows must be [n, %d], got %s" % (self.dim, tuple(rows.shape)))
        n = rows.shape[0]
        it = self._index("items", items, n, self.items)
        rows = rows.detach().to(device=self.device, dtype=torch.float32)
        if real:
            self._real.append((rows, it))
        else:
            self._fake.append((rows, it, self._index("sentences", sentences, n, self.sentences)))

    def _features(self, u8):
        if self.net is None:
            raise ValueError("ConsistencyScorer: built without a GoogLeNet: only add_rows is available")
        return self.net.rows(u8)

    def add_fake(self, img_nhwc, items, sentences):
        """G's last-stage NHWC images in [-1, 1] (B, H, W, C >= 3), generated from (items[j], sentences[j]): quantised as
        the PNG writer quantises them (ops.images_to_uint8_hwc), then GoogLeNet's ten-view mean rows."""
        self.add_rows(self._features(ops.images_to_uint8_hwc(img_nhwc)), items, sentences)

    def add_real(self, images, items):
        """The real image of every items[j]: uint8 (B, H, W, 3) RGB, or fp32 (B, 3, H, W) in [-1, 1] (quantised as the
        fake ones are)."""
        images = images.to(self.device)
        if images.dtype != torch.uint8:
            images = ops.images_to_uint8_hwc(images.float().permute(0, 2, 3, 1).contiguous())
        self.add_rows(self._features(images.contiguous()), items, real=True)

    def _rank(self, rows, items, sentences):
        from . import retrieval
        qlab = self.labels[items]
        gt, eq = self.gallery.rank(rows, items * self.sentences + sentences, qlab, self.row_labels)
        return retrieval.rank_metrics(gt, eq, retrieval.other_class_counts(qlab, self.row_labels))

    def result(self):
        """{fake_recall@1, fake_recall@5, fake_recall@10, fake_median_rank, fake_r_precision, fake_n_queries,
        fake_n_skipped} over the fake rows in arrival order, and the same under real_* with each real row queried once per
        sentence of its item.  A side that received no rows is left out."""
        out = {}
        if self._fake:
            rows = torch.cat([f[0] for f in self._fake])
            res = self._rank(rows, np.concatenate([f[1] for f in self._fake]), np.concatenate([f[2] for f in self._fake]))
            out.update(("fake_" + k, v) for k, v in res.items())
        if self._real:
            rows = torch.cat([r[0] for r in self._real])
            items = np.concatenate([r[1] for r in self._real])
            S = self.sentences
            res = self._rank(rows.repeat_interleave(S, dim=0), np.repeat(items, S), np.tile(np.arange(S), items.shape[0]))
            out.update(("real_" + k, v) for k, v in res.items())
        return out


class _PngWriter:
    """Writes save_singleimages PNGs on a host thread once the device copy of a batch has landed."""

    def __init__(self, save_dir, split_dir="valid"):
        self.save_dir, self.split_dir = save_dir, split_dir
        self.q = queue.Queue(maxsize=4)
        self.err = None
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def put(self, img_nhwc, filenames, sentence_ids):
        u8 = ops.images_to_uint8_hwc(img_nhwc)
        host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(u8, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.q.put((ev, host, list(filenames), list(sentence_ids)))

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            if self.err is not None:
                continue
            ev, host, names, sids = job
            try:
                ev.synchronize()
                a = host.numpy()
                B = len(names)
                for k, s in enumerate(sids):
                    save_singleimages(a[k * B:(k + 1) * B], names, self.save_dir, self.split_dir, s, a.shape[1], 0)
            except Exception as e:   # reported by close()
                self.err = e

    def close(self):
        self.q.put(None)
        self.t.join()
        if self.err is not None:
            raise self.err


@torch.no_grad()
def score_generator(netG, loader, scorer, seed, sentences=None, max_items=None, save_images=None,
                    stack_images=G_STACK_IMAGES, consistency=None):
    """Drive G (.eval()) over the test loader's (images per branch, embeddings (B, S, D), filenames) batches and feed
    `scorer`: each batch's last-branch real images once, then its fake images sentence by sentence, items in order within
    a sentence (the reference's row order).  z (B, Z_DIM) then eps (B, EMBEDDING_DIM) are drawn per sentence from one
    CPU generator seeded with `seed`, so stacking sentences into one G launch (up to stack_images images) draws the same
    noise.  `save_images`: a directory that receives the reference-named PNGs (single_samples/valid/...).
    `consistency`: a ConsistencyScorer over the loader's items in loader order (item index = position in the split, its
    sentences = the embedding columns); it is fed the same real and fake tensors and changes nothing else: the same noise,
    the same PNGs, the same `scorer` input.
    Returns the number of test items scored."""
    from .miscc.config import cfg
    dev = scorer.device
    netG.eval()
    g = torch.Generator().manual_seed(int(seed))
    writer = _PngWriter(save_images) if save_images else None
    items = 0
    try:
        for imgs, emb, names in loader:
            if max_items is not None and items >= max_items:
                break
            B = emb.shape[0] if max_items is None else min(emb.shape[0], max_items - items)
            emb = emb[:B].float().to(dev)
            names = list(names)[:B]
            real = imgs[-1][:B].to(dev, non_blocking=True)
            scorer.add_real(ops.images_from_uint8_hwc(real.contiguous()) if real.dtype == torch.uint8 else real.float())
            if consistency is not None:
                consistency.add_real(real, np.arange(items, items + B))
            sent = list(range(emb.shape[1])) if sentences is None else list(sentences)
            per = max(1, int(stack_images) // B)
            for s0 in range(0, len(sent), per):
                ss = sent[s0:s0 + per]
                zs, es = [], []
                for _ in ss:
                    zs.append(torch.randn(B, cfg.GAN.Z_DIM, generator=g))
                    es.append(torch.randn(B, cfg.GAN.EMBEDDING_DIM, generator=g))
                c = torch.cat([emb[:, s] for s in ss]).contiguous()
                fake, _, _ = netG(torch.cat(zs).to(dev), c, torch.cat(es).to(dev), True)
                scorer.add_fake(nhwc4_as_nchw(fake[-1]))
                if consistency is not None:
                    consistency.add_fake(fake[-1], np.tile(np.arange(items, items + B), len(ss)), np.repeat(ss, B))
                if writer is not None:
                    writer.put(fake[-1], names, ss)
            items += B
    finally:
        if writer is not None:
            writer.close()
    return items


# ---- command line ----------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="IS, NLPP and FID of a trained generator on the test split")
    p.add_argument("--cfg", default=None, help="YAML of the generator (widths, branches, batch size)")
    p.add_argument("--netG", required=True, help="generator state_dict (netG_<N>.pth)")
    p.add_argument("--inception", required=True, help="torchvision-layout Inception-v3 state_dict (local file)")
    p.add_argument("--data_dir", required=True, help="dataset root holding test.json and test/audio_features_*.pickle")
    p.add_argument("--feature_switch", default="image", help="test/audio_features_<switch>.pickle")
    p.add_argument("--real_stats", default=None,
                   help=".npz of the real images' mu / sigma / n: read if it exists (real images are not scored), "
                        "else written")
    p.add_argument("--save_images", action="store_true", default=False,
                   help="write the PNGs under <netG dir>/iteration<N>/single_samples/valid/")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--max_items", type=int, default=None, help="score only the first K test items")
    p.add_argument("--batch_size", type=int, default=None, help="default: TRAIN.BATCH_SIZE")
    p.add_argument("--workers", type=int, default=None, help="default: WORKERS")
    p.add_argument("--out", default="metrics.json", help="JSON record; fid_stats_fake/real.npz go next to it")
    p.add_argument("--googlenet", default=None,
                   help="bvlc_googlenet.caffemodel (local file): adds the speech-image consistency scores (fake_* and "
                        "real_* recall@k, median rank, R-precision) to the record; the embeddings must be 1024 wide")
    p.add_argument("--consistency_cosine", action="store_true", default=False,
                   help="rank by cosine similarity instead of the dot product")
    p.add_argument("--kid", action="store_true", default=False,
                   help="add `kid`: the unbiased cubic-kernel MMD^2 of the fake against the real pool3 rows (full samples)")
    p.add_argument("--prdc", action="store_true", default=False,
                   help="add `precision`, `recall`, `density`, `coverage`: k-nearest-neighbour manifolds of the pool3 rows")
    p.add_argument("--nearest_k", type=int, default=None, metavar="K",
                   help="the k of --prdc, 1..64 (default 5; 3 is Kynkaanniemi's setting); implies --prdc")
    args = p.parse_args(argv)
    if args.max_items is not None and args.max_items < 1:
        p.error("--max_items must be >= 1")
    args.real_stats_mode = None if not args.real_stats else ("read" if os.path.isfile(args.real_stats) else "write")
    if args.nearest_k is not None:
        if not 1 <= args.nearest_k <= _lib.TOPK_MAX:
            p.error("--nearest_k must lie in 1..%d" % _lib.TOPK_MAX)
        args.prdc = True
    else:
        args.nearest_k = 5
    args.keep_rows = args.kid or args.prdc
    if args.keep_rows and args.real_stats_mode == "read":
        p.error("--kid, --prdc and --nearest_k compare pool3 rows, and with --real_stats %s, which exists, the real "
                "images are not scored, so there are no real rows: drop --real_stats or name a file to be written"
                % args.real_stats)
    return args


def _image_dir(netG_path):
    """<netG dir>/iteration<N>, as the reference's evaluate names it (trainer.py:714-718)."""
    iteration = int(netG_path[netG_path.rfind('_') + 1:netG_path.rfind('.')])
    return '%s/iteration%d' % (os.path.dirname(os.path.abspath(netG_path)), iteration)


def main(argv=None):
    args = parse_args(argv)
    from .datasets import BirdsDataset, default_image_transform, make_dataloader
    from .miscc.config import cfg, cfg_from_file
    from .model import INCEPTION_V3
    from .speech_to_image import load_generator
    if args.cfg:
        cfg_from_file(args.cfg)
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    real_stats = load_stats(args.real_stats, POOL3) if args.real_stats_mode == "read" else None
    random.seed(args.seed)          # the test transform's random crop and flip (main.py:127-131)
    torch.manual_seed(args.seed)
    imsize = cfg.TREE.BASE_SIZE * (2 ** (cfg.TREE.BRANCH_NUM - 1))
    dataset = BirdsDataset(args.data_dir, train=False, base_size=cfg.TREE.BASE_SIZE,
                           transform=default_image_transform(imsize), feature_switch=args.feature_switch)
    bs = args.batch_size or cfg.TRAIN.BATCH_SIZE
    loader = make_dataloader(dataset, bs, shuffle=False,
                             workers=cfg.WORKERS if args.workers is None else args.workers)
    n_items = len(dataset) if args.max_items is None else min(len(dataset), args.max_items)
    n_sent = dataset.embedding.shape[1]
    scorer = GeneratorScorer(INCEPTION_V3(args.inception), n_items * n_sent, dev, keep_rows=args.keep_rows)
    netG = load_generator(args.netG, dev)
    consistency = None
    if args.googlenet:
        from .googlenet import GoogLeNetFeatures
        from .retrieval import labels_from_json
        labels = labels_from_json(os.path.join(args.data_dir, "test.json"))
        consistency = ConsistencyScorer(GoogLeNetFeatures(args.googlenet, dev), np.asarray(dataset.embedding)[:n_items],
                                        labels[:n_items], dev, cosine=args.consistency_cosine)
    score_generator(netG, loader, scorer, args.seed, max_items=args.max_items,
                    save_images=_image_dir(args.netG) if args.save_images else None, consistency=consistency)
    res = scorer.result(10, real_stats, kid=args.kid, prdc=args.prdc, nearest_k=args.nearest_k)
    if consistency is not None:
        res.update(consistency.result(), consistency_score="cosine" if args.consistency_cosine else "dot")
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    fake_stats, rstats = res.pop("fake_stats"), res.pop("real_stats")
    save_stats(os.path.join(out_dir, "fid_stats_fake.npz"), *fake_stats)
    save_stats(os.path.join(out_dir, "fid_stats_real.npz"), *rstats)
    if args.real_stats_mode == "write":
        save_stats(args.real_stats, *rstats)
    rec = dict(res, netG=os.path.abspath(args.netG), seed=args.seed, items=n_items, sentences=n_sent,
               real_stats=os.path.abspath(args.real_stats) if args.real_stats else None)
    with open(args.out, "w") as f:
        json.dump(rec, f)
        f.write("\n")
    line = ("IS %.4f +- %.4f, NLPP %.4f +- %.4f, FID %.4f (%d fake, %d real)"
            % (res["is_mean"], res["is_std"], res["nlpp_mean"], res["nlpp_std"], res["fid"], res["n_fake"], res["n_real"]))
    if args.kid:
        line += ", KID %.6f" % res["kid"]
    if args.prdc:
        line += (", precision %.4f, recall %.4f, density %.4f, coverage %.4f (k %d)"
                 % (res["precision"], res["recall"], res["density"], res["coverage"], res["nearest_k"]))
    print(line)
    return rec


if __name__ == "__main__":
    main()
