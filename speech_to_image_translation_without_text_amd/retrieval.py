"""Speech-to-image retrieval score of a speech encoder: the class-centre accuracy and AP@50 of the reference's
EvalClass.eval_class and eval_audio_feature (Audio_to_Image/train_audio_encoder.py:219-244, 364-382), on the host in
float64 (the sizes are a few thousand rows of 1024).

    python -m speech_to_image_translation_without_text_amd.retrieval --audio data/birds/test/audio_features_0.pickle \\
        --image data/birds/test/image_features_googlenet_caffe.pickle --data_dir data/birds --split test [--seed 0]

prints and writes (``--out``, default ``<audio pickle dir>/retrieval_<split>.json``) one JSON line with ``accu`` and
``ap50`` in percent.  With ``--recall`` the line also carries ``recall@1``, ``recall@5``, ``recall@10`` and ``recall@50``:
the instance-level score, every one of the ten utterances of every item against the mean-of-views image rows, ranked on the
GPU (`Gallery`, `recall_at_k`).

`Gallery` keeps image-feature rows in HBM and answers "which rows does this embedding score highest against": the scores
of one chunk of rows at a time come from the fp32 1x1 matrix kernel and are folded into a running top k by s2i_topk_rows,
so the [queries, rows] matrix never exists.  `eval_class` stays on the host as it was.

`Gallery.rank` answers the other question a retrieval score asks, "where does THIS row stand for this query": the same
chunked scores are folded by s2i_rank_rows into the number of rows of other classes that score above (or exactly as) a
designated own row, and `rank_metrics` turns those counters into recall@k, the median rank and the closed-form
R-precision (gan_metrics.ConsistencyScorer).
"""
import argparse
import json
import os
import pickle
import random

import numpy as np

from . import datasets

TOPK = 50
RECALL_KS = (1, 5, 10, 50)
# Gallery rows scored per matrix launch, and queries per launch (DESIGN.md section 8b7 has the measurements behind them)
GALLERY_CHUNK_ROWS = 65536
QUERY_BLOCK = 4096


def eval_class(query, target, labels, topk=TOPK):
    """(accuracy %, AP@topk %): the class centres are the means of the query rows of each class; target row i scores
    target_i . centre_c; accuracy is that of the argmax class; for each class the top-k targets by its score are drawn
    and those of that class counted, over all drawn (train_audio_encoder.py:219-244)."""
    query = np.asarray(query, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    lab = lab.reshape(-1)
    if query.ndim != 2 or target.shape != query.shape or lab.shape[0] != query.shape[0]:
        raise ValueError("query %s, target %s and %d labels must agree" % (query.shape, target.shape, lab.shape[0]))
    ncls = int(lab.max()) + 1
    centres = np.stack([query[lab == c].mean(axis=0) for c in range(ncls)])
    scores = target @ centres.T
    accu = float((scores.argmax(axis=1) == lab).mean())
    k = min(topk, scores.shape[0])
    hits = 0
    for c in range(ncls):
        top = np.argsort(scores[:, c])[-k:]
        hits += int((lab[top] == c).sum())
    return accu * 100.0, hits / float(ncls * k) * 100.0


def labels_from_json(path):
    """The class of every item of a split JSON: the integer before the first '.' of its `class`."""
    with open(path) as f:
        meta = json.load(f)
    return [int(str(item["class"]).split(".")[0]) for item in meta["data"]]


def labels_from_filenames(path):
    """The reference's label source: a pickled list of `filenames` such as '001.Black_footed_Albatross/...'."""
    with open(path, "rb") as f:
        names = pickle.load(f)
    return [int(str(n).split(".")[0]) for n in names]


def draw_views(audio, image, seed):
    """One of the 10 rows per item, as eval_audio_feature draws them after random.seed(seed): every audio draw first,
    then every image draw."""
    rng = random.Random(seed)
    n = len(audio)
    a_idx = [rng.randint(0, 9) for _ in range(n)]
    i_idx = [rng.randint(0, 9) for _ in range(n)]
    a = np.stack([np.asarray(audio[i])[j] for i, j in enumerate(a_idx)])
    b = np.stack([np.asarray(image[i])[j] for i, j in enumerate(i_idx)])
    return a, b


def eval_features(audio, image, labels, seed=0, topk=TOPK):
    if not len(audio) == len(image) == len(labels):
        raise ValueError("%d audio items, %d image items and %d labels" % (len(audio), len(image), len(labels)))
    a, b = draw_views(audio, image, seed)
    return eval_class(a, b, labels, topk)


def eval_feature_files(audio_pickle, image_pickle, labels, seed=0, topk=TOPK):
    """eval_audio_feature (train_audio_encoder.py:364-382) on the two pickles (read with the restricted unpickler)."""
    return eval_features(datasets.load_embedding_pickle(audio_pickle), datasets.load_embedding_pickle(image_pickle),
                         labels, seed, topk)


class Gallery:
    """Feature rows resident on `device`, searched by dot product (the score of the embedding loss and of eval_class) or,
    with cosine=True, by cosine similarity.

    features   [N, V, C] (a list of N arrays [V, C], the image-feature pickles) or [N, C]
    views      "mean": one row per item, the mean of its V views, formed in float64 on the host and stored as fp32;
               "all": N * V rows, row i * V + v.  [N, C] features are one row per item either way.
    cosine     rows (float64, on the host, before the fp32 store) and queries (fp32, on the device) are divided by their
               L2 norms; an all-zero row stays zero.
    chunk_rows rows per matrix launch.  Every chunk is packed once here (ops.pack_weight, PACK_PLAIN) and stays in HBM:
               4 * C bytes per row, C rounded up to a multiple of 4.

    rows, items, nviews (V where views="all", else None), dim, nbytes.  There is no CPU fallback."""

    def __init__(self, features, device, views="mean", cosine=False, chunk_rows=GALLERY_CHUNK_ROWS):
        import torch
        from . import _lib, ops
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.S2IError("the gallery is packed for and searched by the MI355X kernels: there is no CPU fallback "
                                "(device %s)" % self.device)
        if views not in ("mean", "all"):
            raise ValueError("Gallery: views must be 'mean' or 'all', got %r" % (views,))
        self.chunk_rows = int(chunk_rows)
        if self.chunk_rows < 1:
            raise ValueError("Gallery: chunk_rows must be >= 1")
        rows, self.items, self.nviews = gallery_rows(features, views, cosine)
        self.cosine = bool(cosine)
        self.rows, self.dim = rows.shape
        self.cpad = (self.dim + 3) & ~3
        if self.chunk_rows * self.cpad * 4 >= 0x7ff00000:
            raise ValueError("Gallery: a chunk of %d rows of %d floats exceeds the matrix kernel's 2 GiB operand window"
                             % (self.chunk_rows, self.cpad))
        self.chunks = []
        with torch.cuda.device(self.device):
            for s in range(0, self.rows, self.chunk_rows):
                part = np.zeros((min(self.chunk_rows, self.rows - s), self.cpad), dtype=np.float32)
                part[:, :self.dim] = rows[s:s + self.chunk_rows]
                self.chunks.append((s, part.shape[0], ops.pack_weight(torch.from_numpy(part).to(self.device), ops.PACK_PLAIN)))
        self.nbytes = sum(c[2].numel() * 4 for c in self.chunks)
        self._scores = None

    def _check_queries(self, queries, what):
        import torch
        q = torch.as_tensor(queries)
        if q.dim() != 2 or q.shape[1] != self.dim or q.shape[0] < 1:
            raise ValueError("Gallery.%s: queries must be [Q >= 1, %d], got %s" % (what, self.dim, tuple(q.shape)))
        return q

    def _prepare(self, q):
        """The queries as the matrix kernel takes them (fp32 on the device, normalised where cosine, padded to cpad,
        contiguous), and the score scratch of one (QUERY_BLOCK, chunk) launch.  Called on self.device."""
        import torch
        q = q.detach().to(device=self.device, dtype=torch.float32)
        if self.cosine:
            norm = torch.linalg.vector_norm(q, dim=1, keepdim=True)
            q = q / torch.where(norm > 0, norm, torch.ones_like(norm))
        if self.cpad != self.dim:
            q = torch.nn.functional.pad(q, (0, self.cpad - self.dim))
        q = q.contiguous()
        need = min(q.shape[0], QUERY_BLOCK) * min(self.chunk_rows, self.rows)
        if self._scores is None or self._scores.numel() < need:
            self._scores = torch.empty(need, dtype=torch.float32, device=self.device)
        return q

    def search(self, queries, k):
        """(scores [Q, k] fp32, items [Q, k] int64, views [Q, k] int64 or None) on the device: for each query row its k
        best gallery rows, best first; equal scores by ascending row.  k is clipped to the number of rows (64 at the most
        after that: the kernel's limit)."""
        import torch
        from . import ops
        q = self._check_queries(queries, "search")
        k = min(int(k), self.rows)
        if not 1 <= k <= 64:
            raise ValueError("Gallery.search: k must lie in 1..64 after clipping to the %d rows, got %d" % (self.rows, k))
        with torch.cuda.device(self.device):
            q = self._prepare(q)
            Q = q.shape[0]
            best = (torch.empty((Q, k), dtype=torch.float32, device=self.device),
                    torch.empty((Q, k), dtype=torch.int32, device=self.device))
            for q0 in range(0, Q, QUERY_BLOCK):
                qb = q[q0:q0 + QUERY_BLOCK]
                pair = (best[0][q0:q0 + QUERY_BLOCK], best[1][q0:q0 + QUERY_BLOCK])
                for i, (start, n, packed) in enumerate(self.chunks):
                    sc = ops.score_rows(qb, packed, n, self._scores)
                    if i == 0:
                        ops.topk_rows(sc, k, base=start, out=pair)
                    else:
                        ops.topk_rows(sc, k, base=start, best=pair)
            row = best[1].to(torch.int64)
        if self.nviews is None:
            return best[0], row, None
        return best[0], torch.div(row, self.nviews, rounding_mode="floor"), row % self.nviews

    def rank(self, queries, own_rows, query_labels, row_labels):
        """(gt, eq) int32 [Q] on the device.  Query q designates gallery row own_rows[q] (-1: none) and has class
        query_labels[q]; row_labels gives the class of every gallery row.  Among the rows of OTHER classes, gt[q] score
        strictly above the own row and eq[q] exactly as it does (float comparison; s2i_rank_rows has the NaN rules).  Rows
        of the query's class are never counted, the own row included.  A query without an own row is compared with a
        score of 0.

        Two passes over the (QUERY_BLOCK, chunk) launches `search` makes: the first gathers each own score out of the
        chunk that holds it (chunks without an own row of the block are skipped), the second counts.  The own score so
        comes from the same kind of launch, on the same operands, that scores its neighbours, and nothing of size
        Q x rows exists."""
        import torch
        from . import ops
        q = self._check_queries(queries, "rank")
        Q = q.shape[0]
        own = np.asarray(own_rows.cpu() if torch.is_tensor(own_rows) else own_rows).reshape(-1).astype(np.int64)
        qlab = np.asarray(query_labels.cpu() if torch.is_tensor(query_labels) else query_labels).reshape(-1)
        rlab = np.asarray(row_labels.cpu() if torch.is_tensor(row_labels) else row_labels).reshape(-1)
        if own.shape[0] != Q or qlab.shape[0] != Q or rlab.shape[0] != self.rows:
            raise ValueError("Gallery.rank: %d own rows and %d query labels for %d queries, %d row labels for %d rows"
                             % (own.shape[0], qlab.shape[0], Q, rlab.shape[0], self.rows))
        if own.min() < -1 or own.max() >= self.rows:
            raise ValueError("Gallery.rank: own rows must lie in -1..%d" % (self.rows - 1))
        for lab in (qlab, rlab):
            if lab.dtype.kind not in "iu" or lab.min() < -2 ** 31 or lab.max() > 2 ** 31 - 1:
                raise ValueError("Gallery.rank: labels must be integers that fit int32")
        with torch.cuda.device(self.device):
            q = self._prepare(q)
            own_d = torch.from_numpy(own.astype(np.int32)).to(self.device)
            qlab_d = torch.from_numpy(qlab.astype(np.int32)).to(self.device)
            rlab_d = torch.from_numpy(rlab.astype(np.int32)).to(self.device)
            own_score = torch.zeros(Q, dtype=torch.float32, device=self.device)
            gt = torch.zeros(Q, dtype=torch.int32, device=self.device)
            eq = torch.zeros(Q, dtype=torch.int32, device=self.device)
            for q0 in range(0, Q, QUERY_BLOCK):
                q1 = min(Q, q0 + QUERY_BLOCK)
                qb, ob = q[q0:q1], own[q0:q1]
                for start, n, packed in self.chunks:
                    if ((ob >= start) & (ob < start + n)).any():
                        sc = ops.score_rows(qb, packed, n, self._scores)
                        ops.rank_rows(sc, own_d[q0:q1], None, None, start, own_score[q0:q1], None, None, "gather")
                for start, n, packed in self.chunks:
                    sc = ops.score_rows(qb, packed, n, self._scores)
                    ops.rank_rows(sc, None, qlab_d[q0:q1], rlab_d, start, own_score[q0:q1], gt[q0:q1], eq[q0:q1], "count")
        return gt, eq


def pack_device_rows(rows, chunk_rows=GALLERY_CHUNK_ROWS):
    """(padded, chunks): fp32 rows [R, C] that are ALREADY on the device, as the matrix kernel takes them on either side.
    `padded` is the rows as queries ([R, cpad] contiguous, C rounded up to a multiple of 4 with zeros; `rows` itself where
    nothing had to change), `chunks` the list of (start, n, packed) that Gallery keeps, every chunk packed on the device
    (ops.pack_weight, PACK_PLAIN).  No host round trip.  There is no CPU fallback."""
    import torch
    from . import _lib, ops
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.dtype != torch.float32 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("pack_device_rows: rows must be an fp32 [R >= 1, C >= 1] tensor")
    if not rows.is_cuda:
        raise _lib.S2IError("rows are packed for and scored by the MI355X kernels: there is no CPU fallback (rows on %s)"
                            % rows.device)
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("pack_device_rows: chunk_rows must be >= 1")
    R, C = rows.shape
    cpad = (C + 3) & ~3
    if chunk_rows * cpad * 4 >= 0x7ff00000:
        raise ValueError("pack_device_rows: a chunk of %d rows of %d floats exceeds the matrix kernel's 2 GiB operand window"
                         % (chunk_rows, cpad))
    with torch.cuda.device(rows.device):
        padded = rows.detach()
        if cpad != C:
            padded = torch.nn.functional.pad(padded, (0, cpad - C))
        padded = padded.contiguous()
        chunks = [(s, min(chunk_rows, R - s), ops.pack_weight(padded[s:s + chunk_rows], ops.PACK_PLAIN))
                  for s in range(0, R, chunk_rows)]
    return padded, chunks


def rank_metrics(gt, eq, n_candidates, m=99, ks=(1, 5, 10)):
    """The retrieval scores of Gallery.rank's counters, on the host in float64.

    For query i, c = gt[i] + eq[i] wrong candidates stand at or ahead of its own one (a tie counts against the query) among
    the n = n_candidates[i] gallery rows of other classes.

    recall@k      percent of queries with c < k: the own candidate among the first k of itself and the n others.
    median_rank   the median of 1 + c.
    r_precision   100 x the mean of  prod_{t < m'} (n - c - t) / (n - t),  m' = min(m, n), 0 where n - c < m': the exact
                  probability that the own candidate comes first among itself and m mismatched candidates drawn without
                  replacement from the n (all m' drawn ones must be among the n - c that score below it), i.e. the
                  expectation of the sampled R-precision protocol.  Nothing is sampled: no seed.
    n_queries     queries scored;  n_skipped  queries with n == 0 (nothing to be ranked against), left out of all means.
    With no query left the scores are NaN."""
    gt = np.asarray(gt.cpu() if hasattr(gt, "cpu") else gt).reshape(-1).astype(np.int64)
    eq = np.asarray(eq.cpu() if hasattr(eq, "cpu") else eq).reshape(-1).astype(np.int64)
    n = np.asarray(n_candidates).reshape(-1).astype(np.int64)
    m, ks = int(m), [int(k) for k in ks]
    if not gt.shape == eq.shape == n.shape:
        raise ValueError("rank_metrics: %d gt, %d eq and %d candidate counts" % (gt.shape[0], eq.shape[0], n.shape[0]))
    if m < 1 or not ks or min(ks) < 1:
        raise ValueError("rank_metrics: m and every k must be >= 1, got m %d, ks %s" % (m, ks))
    c = gt + eq
    if gt.size and (min(gt.min(), eq.min(), n.min()) < 0 or (c > n).any()):
        raise ValueError("rank_metrics: counters must satisfy 0 <= gt + eq <= n_candidates")
    keep = n > 0
    c, n = c[keep], n[keep]
    out = {"n_queries": int(keep.sum()), "n_skipped": int((~keep).sum())}
    if c.size == 0:
        out.update(("recall@%d" % k, float("nan")) for k in ks)
        out.update(median_rank=float("nan"), r_precision=float("nan"))
        return out
    for k in ks:
        out["recall@%d" % k] = float((c < k).mean() * 100.0)
    out["median_rank"] = float(np.median(1.0 + c))
    mm = np.minimum(m, n)
    p = np.ones(c.shape[0], dtype=np.float64)
    nf, cf = n.astype(np.float64), c.astype(np.float64)
    for t in range(int(mm.max())):
        live = t < mm
        p = np.where(live, p * np.maximum(nf - cf - t, 0.0) / np.where(live, nf - t, 1.0), p)
    out["r_precision"] = float(p.mean() * 100.0)
    return out


def other_class_counts(query_labels, row_labels):
    """For every query the number of gallery rows whose label differs from its own: rank_metrics' n_candidates."""
    qlab, rlab = np.asarray(query_labels).reshape(-1), np.asarray(row_labels).reshape(-1)
    vals, cnt = np.unique(rlab, return_counts=True)
    pos = np.searchsorted(vals, qlab)
    pos = np.minimum(pos, len(vals) - 1)
    same = np.where(vals[pos] == qlab, cnt[pos], 0)
    return rlab.shape[0] - same


def gallery_rows(features, views="mean", cosine=False):
    """(rows [R, C] fp32, items N, V or None): the host side of Gallery -- the rows it stores, in its order."""
    feats = np.asarray(features if isinstance(features, np.ndarray) else [np.asarray(f) for f in features])
    if feats.ndim not in (2, 3) or feats.shape[0] < 1 or feats.shape[-1] < 1 or (feats.ndim == 3 and feats.shape[1] < 1):
        raise ValueError("Gallery: features must be [N, V, C] or [N, C], got %s" % (feats.shape,))
    items, nviews = feats.shape[0], None
    if feats.ndim == 3:
        if views == "mean":
            feats = feats.astype(np.float64).mean(axis=1)
        else:
            nviews = feats.shape[1]
            feats = feats.reshape(items * nviews, feats.shape[2])
    if cosine:
        feats = feats.astype(np.float64)
        norm = np.sqrt((feats * feats).sum(axis=1, keepdims=True))
        feats = feats / np.where(norm > 0, norm, 1.0)
    return feats.astype(np.float32), items, nviews


def recall_at_k(audio, gallery, ks=RECALL_KS):
    """{k: percent} instance-level recall: every utterance audio[i][u] of every item i is a query, and it is a hit at k
    when any of its k best gallery rows belongs to item i.  One Gallery.search at max(ks)."""
    a = np.asarray(audio if isinstance(audio, np.ndarray) else [np.asarray(f) for f in audio], dtype=np.float32)
    if a.ndim != 3 or a.shape[0] != gallery.items:
        raise ValueError("recall_at_k: audio %s does not give [N, U, C] utterances for the gallery's %d items"
                         % (a.shape, gallery.items))
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1:
        raise ValueError("recall_at_k: ks must be positive, got %s" % (ks,))
    n, u, c = a.shape
    _, items, _ = gallery.search(a.reshape(n * u, c), max(ks))
    hit = items.cpu().numpy() == np.repeat(np.arange(n), u)[:, None]
    return {k: float(hit[:, :k].any(axis=1).mean() * 100.0) for k in ks}


def get_parser():
    p = argparse.ArgumentParser(description="speech-to-image retrieval accuracy and AP@50")
    p.add_argument("--audio", required=True, help="audio_features_<switch>.pickle (N, 10, D)")
    p.add_argument("--image", required=True, help="image feature pickle (N x (10, D))")
    p.add_argument("--data_dir", default=None, help="directory with <split>.json (labels from each item's class)")
    p.add_argument("--split", default="test")
    p.add_argument("--filenames", default=None, help="filenames.pickle to take the labels from instead")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--topk", type=int, default=TOPK)
    p.add_argument("--out", default=None, help="JSON output (default <audio dir>/retrieval_<split>.json)")
    p.add_argument("--recall", action="store_true", default=False,
                   help="add recall@1/5/10/50: all ten utterances of each item against the mean-of-views image rows, "
                        "ranked on the GPU")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.filenames:
        labels = labels_from_filenames(args.filenames)
    elif args.data_dir:
        labels = labels_from_json(os.path.join(args.data_dir, "%s.json" % args.split))
    else:
        raise SystemExit("give --data_dir (split JSON) or --filenames for the labels")
    accu, ap = eval_feature_files(args.audio, args.image, labels, args.seed, args.topk)
    result = {"split": args.split, "items": len(labels), "seed": args.seed, "accu": accu, "ap50": ap}
    if args.recall:
        import torch
        gallery = Gallery(datasets.load_embedding_pickle(args.image), torch.device("cuda", torch.cuda.current_device()))
        recall = recall_at_k(datasets.load_embedding_pickle(args.audio), gallery)
        result.update(("recall@%d" % k, v) for k, v in recall.items())
    line = json.dumps(result)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(args.audio)), "retrieval_%s.json" % args.split)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
    return accu, ap


if __name__ == "__main__":
    main()
