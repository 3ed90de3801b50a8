"""Plain-numpy restatement of the rank fold (s2i_rank_rows, retrieval.Gallery.rank) and of rank_metrics' closed forms,
with the mutants the GPU suite's inputs must tell apart, and the exact-in-fp32 inputs that suite uses."""
import itertools
import math

import numpy as np

MUTANTS = ("tie_wins", "same_class_counted", "own_row_counted", "base_ignored")


def gather(scores, own_row, base, own_score):
    """own_score[q] = scores[q][own_row[q] - base] where the own row lies in [base, base + N); the rest untouched."""
    out = np.array(own_score, copy=True)
    N = scores.shape[1]
    for q, r in enumerate(own_row):
        if base <= r < base + N:
            out[q] = scores[q, r - base]
    return out


def count(scores, qlabel, rlabel, base, own_score, gt=None, eq=None, mutant=None, own_row=None):
    """(gt, eq) after one chunk: columns of other classes above / exactly at own_score; a NaN score in neither; a NaN own
    score puts every column of another class into gt.  `mutant` is one of MUTANTS: a wrong rule."""
    Q, N = scores.shape
    gt = np.zeros(Q, np.int64) if gt is None else np.array(gt, dtype=np.int64)
    eq = np.zeros(Q, np.int64) if eq is None else np.array(eq, dtype=np.int64)
    lab = np.asarray(rlabel)[(0 if mutant == "base_ignored" else base) + np.arange(N)]
    for q in range(Q):
        other = lab != qlabel[q]
        if mutant == "same_class_counted":
            other = np.ones(N, bool)
            if own_row is not None and base <= own_row[q] < base + N:
                other[own_row[q] - base] = False
        elif mutant == "own_row_counted" and own_row is not None and base <= own_row[q] < base + N:
            other = other.copy()
            other[own_row[q] - base] = True
        s, own = scores[q], own_score[q]
        if np.isnan(own):
            gt[q] += int(other.sum())
            continue
        with np.errstate(invalid="ignore"):
            above, level = (s > own) & other, (s == own) & other
        if mutant == "tie_wins":
            level = np.zeros(N, bool)
        gt[q] += int(above.sum())
        eq[q] += int(level.sum())
    return gt, eq


def rank_counts(scores, own_row, qlabel, rlabel, base=0, chunks=None, mutant=None):
    """(gt, eq, own_score) of a whole [Q, R] score matrix whose column j is row base + j: the gather pass, then the count
    pass, over `chunks` (column counts, default one chunk).  Queries without an own row are compared with 0."""
    scores = np.asarray(scores)
    Q, R = scores.shape
    cuts = np.concatenate([[0], np.cumsum(chunks if chunks is not None else [R])])
    assert cuts[-1] == R
    own = np.zeros(Q, scores.dtype)
    for a, b in zip(cuts[:-1], cuts[1:]):
        own = gather(scores[:, a:b], own_row, base + a, own)
    gt = eq = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        gt, eq = count(scores[:, a:b], qlabel, rlabel, base + a, own, gt, eq, mutant, own_row)
    return gt, eq, own


# ---- the closed forms --------------------------------------------------------------------------------------------------
def r_precision_closed(n, c, m):
    """P(the own candidate is first among itself and m' = min(m, n) of the n others drawn without replacement), c of the
    n standing at or ahead of it: C(n - c, m') / C(n, m'), exact in integers."""
    mm = min(m, n)
    return math.comb(n - c, mm) / math.comb(n, mm) if n - c >= mm else 0.0


def r_precision_enumerated(n, c, m):
    """The same by brute force: every draw of m' of the n others (the first c are the ones ahead); the own one wins when
    none of those is drawn."""
    mm = min(m, n)
    draws = list(itertools.combinations(range(n), mm))
    return sum(1 for d in draws if all(j >= c for j in d)) / len(draws)


def metrics(gt, eq, n, m=99, ks=(1, 5, 10)):
    c = np.asarray(gt, np.int64) + np.asarray(eq, np.int64)
    n = np.asarray(n, np.int64)
    keep = n > 0
    c, n = c[keep], n[keep]
    out = {"n_queries": int(keep.sum()), "n_skipped": int((~keep).sum())}
    for k in ks:
        out["recall@%d" % k] = 100.0 * float(np.mean(c < k))
    out["median_rank"] = float(np.median(1 + c))
    out["r_precision"] = 100.0 * float(np.mean([r_precision_closed(int(a), int(b), m) for a, b in zip(n, c)]))
    return out


# ---- inputs whose scores are exact in fp32 -----------------------------------------------------------------------------
C = 64


def integer_features(seed, rows, dim=C):
    """Integers in [-8, 8]: a dot product of 64 of them is an integer below 2^24, so fp32 and fp64 agree on every score
    whatever the order of the sums, and ties occur naturally."""
    return np.random.RandomState(seed).randint(-8, 9, size=(rows, dim)).astype(np.float32)


def case(seed, Q, R, classes=7, dup=True):
    """(queries [Q, C], gallery [R, C], own_row [Q], qlabel [Q], rlabel [R]).  Query q's own row is drawn among the rows
    of its class (about one in eight gets -1); with `dup` some row of ANOTHER class is made a copy of the own row, which
    forces a tie on top of the natural ones."""
    rng = np.random.RandomState(seed + 1000)
    gal = integer_features(seed, R)
    qs = integer_features(seed + 1, Q)
    rlabel = rng.randint(0, classes, size=R).astype(np.int32)
    own = np.full(Q, -1, np.int32)
    qlabel = rng.randint(0, classes, size=Q).astype(np.int32)
    for q in range(Q):
        if rng.randint(8) == 0 and Q > 1:
            continue
        r = rng.randint(R)
        own[q] = r
        qlabel[q] = rlabel[r]
    if dup and R >= 2:
        for q in range(0, Q, 3):
            if own[q] < 0:
                continue
            others = np.flatnonzero(rlabel != qlabel[q])
            if others.size:
                gal[others[rng.randint(others.size)]] = gal[own[q]]
    return qs, gal, own, qlabel, rlabel


def scores64(qs, gal):
    return qs.astype(np.float64) @ gal.astype(np.float64).T
