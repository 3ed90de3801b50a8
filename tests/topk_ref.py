"""numpy restatement of the nearest-row search (csrc/s2i_topk.hip, ops.topk_rows, retrieval.Gallery / recall_at_k): the
selection rule, the chunked merge, the Gallery's row rules in float64, the case lists of the two test files, the mutants
the comparison must refuse, and the fp32 yardsticks of the end-to-end bound.

The rule: higher score first; equal scores by ascending row id; NaN ranks as -inf (and -0 equals +0); slots beyond the
candidates hold (-inf, -1), which rank behind every real row.  Scores are carried, never computed: bit for bit.
"""
import numpy as np

NEG_INF = np.float32(-np.inf)

# ---- selection ----------------------------------------------------------------------------------------------------------


def _rank_value(score, nan_first=False):
    s = np.asarray(score, dtype=np.float64).copy()
    s[np.isnan(s)] = np.inf if nan_first else -np.inf
    return s


def select(score, row, k, tie_high=False, nan_first=False):
    """The k best of the entries (score [Q, E] fp32, row [Q, E] int) of each query, padded with (-inf, -1).  Row ids rank
    as unsigned 32-bit words, so the empty slot's -1 comes last among equals."""
    score = np.asarray(score, dtype=np.float32)
    row = np.asarray(row, dtype=np.int64)
    Q, E = score.shape
    out_s = np.full((Q, k), NEG_INF, dtype=np.float32)
    out_r = np.full((Q, k), -1, dtype=np.int32)
    for q in range(Q):
        urow = row[q] & 0xffffffff
        order = np.lexsort((-urow if tie_high else urow, -_rank_value(score[q], nan_first)))[:k]
        out_s[q, :len(order)] = score[q, order]
        out_r[q, :len(order)] = row[q, order]
    return out_s, out_r


def topk(scores, k, base=0, **rule):
    """One-shot selection over scores [Q, N]: row id = base + column."""
    scores = np.asarray(scores, dtype=np.float32)
    Q, N = scores.shape
    return select(scores, np.broadcast_to(base + np.arange(N, dtype=np.int64), (Q, N)), k, **rule)


def merge(best, scores, k, base, **rule):
    """Fold a chunk into a running pair: the selection over the pair's k entries and the chunk's rows."""
    s, r = topk(scores, k, base, **rule)
    if best is None:
        return s, r
    return select(np.concatenate([best[0], s], axis=1), np.concatenate([best[1], r], axis=1), k, **rule)


def chunk_starts(N, sizes):
    """Column ranges of a chunk plan: the listed sizes in turn, then the rest in one piece."""
    out, s = [], 0
    for n in sizes:
        if s >= N:
            break
        out.append((s, min(s + n, N)))
        s = min(s + n, N)
    if s < N:
        out.append((s, N))
    return out


def chunked(scores, k, sizes, base=0, **rule):
    best = None
    for s, e in chunk_starts(scores.shape[1], sizes):
        best = merge(best, scores[:, s:e], k, base + s, **rule)
    return best


# ---- mutants: each takes (scores, k, sizes, base) like `chunked` and is wrong in one way -----------------------------------
def mutant_tie_high(scores, k, sizes, base=0):
    return chunked(scores, k, sizes, base, tie_high=True)


def mutant_boundary_drops_one(scores, k, sizes, base=0):
    """Only k - 1 entries survive a chunk boundary."""
    best = None
    for s, e in chunk_starts(scores.shape[1], sizes):
        if best is not None:
            best[0][:, k - 1], best[1][:, k - 1] = NEG_INF, -1
        best = merge(best, scores[:, s:e], k, base + s)
    return best


def mutant_merge_drops_base(scores, k, sizes, base=0):
    """Chunks after the first number their rows from the chunk's own start."""
    best = None
    for i, (s, e) in enumerate(chunk_starts(scores.shape[1], sizes)):
        best = merge(best, scores[:, s:e], k, base + s if i == 0 else 0)
    return best


def mutant_nan_first(scores, k, sizes, base=0):
    return chunked(scores, k, sizes, base, nan_first=True)


MUTANTS = {"tie_high": mutant_tie_high, "boundary_drops_one": mutant_boundary_drops_one,
           "merge_drops_base": mutant_merge_drops_base, "nan_first": mutant_nan_first}

# ---- selection cases --------------------------------------------------------------------------------------------------
# (Q, N, k, lds, base): lds 0 = N.  (2, 5, 8) has more slots than rows; (4, 12289, 10) runs with padded rows; one case runs
# at a large base.  4097 and 12289 are one past a multiple of the 4096 elements sixteen waves take per step.
SELECT_CASES = [(1, 1, 1, 0, 0), (3, 70, 5, 0, 0), (2, 64, 64, 0, 0), (2, 5, 8, 0, 0), (33, 257, 50, 0, 1 << 20),
                (1, 4097, 64, 0, 0), (4, 12289, 10, 12292, 0)]
PATTERNS = ("normal", "equal", "two_valued", "ascending", "descending", "specials")
MERGE_CASES = [(1, 4097, 64), (4, 12289, 10)]
MERGE_SIZES = (1, 7, 64, 4096)


def case_id(case):
    return "Q%d_N%d_k%d" % tuple(case[:3])


def make_scores(Q, N, k, pattern, seed=0):
    rng = np.random.RandomState(1000 * seed + 7 * Q + N + k)
    if pattern == "normal":
        return rng.randn(Q, N).astype(np.float32)
    if pattern == "equal":
        return np.full((Q, N), 0.5, dtype=np.float32)
    if pattern == "two_valued":
        # fewer high values than k, so the k-th place falls among the equal low ones and is decided by the row id
        x = np.ones((Q, N), dtype=np.float32)
        for q in range(Q):
            x[q, rng.permutation(N)[:min(k // 2, N - 1)]] = 2.0
        return x
    if pattern == "ascending":
        return (np.arange(N, dtype=np.float32)[None, :] + np.arange(Q, dtype=np.float32)[:, None]) * np.float32(0.25)
    if pattern == "descending":
        return -(np.arange(N, dtype=np.float32)[None, :] + np.arange(Q, dtype=np.float32)[:, None]) * np.float32(0.25)
    if pattern == "specials":
        # query 0: a third NaN, a third -inf, some +inf, zeros of both signs; the other queries a sprinkling of each.
        # Where k comes near N the NaN and -inf rows reach the top k
        x = rng.randn(Q, N).astype(np.float32)
        for q in range(Q):
            perm = rng.permutation(N)
            n = max(1, N // 3) if q == 0 else max(1, N // 50)
            x[q, perm[:n]] = np.nan
            x[q, perm[n:2 * n]] = -np.inf
            x[q, perm[2 * n:2 * n + max(1, n // 4)]] = np.inf
            if q == 0 and N >= 8:
                # zeros of both signs: they tie, so the row id orders them, and each keeps its sign bit
                rest = perm[2 * n + max(1, n // 4):]
                x[q, rest[:len(rest) // 2]] = np.float32(-0.0)
                x[q, rest[len(rest) // 2:len(rest) // 2 + 2]] = np.float32(0.0)
        return x
    raise ValueError(pattern)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


# ---- Gallery, float64 -----------------------------------------------------------------------------------------------------
def gallery_rows64(features, views="mean", cosine=False):
    """(rows [R, C] float64 holding the fp32 values the Gallery stores, V or None): the mean over views and the cosine
    division in float64, then the fp32 store."""
    f = np.asarray(features, dtype=np.float64)
    nviews = None
    if f.ndim == 3:
        if views == "mean":
            f = f.mean(axis=1)
        else:
            nviews = f.shape[1]
            f = f.reshape(-1, f.shape[2])
    if cosine:
        norm = np.sqrt((f * f).sum(axis=1, keepdims=True))
        f = f / np.where(norm > 0, norm, 1.0)
    return f.astype(np.float32).astype(np.float64), nviews


def scores64(features, queries, views="mean", cosine=False):
    rows, nviews = gallery_rows64(features, views, cosine)
    q = np.asarray(queries, dtype=np.float32).astype(np.float64)
    if cosine:
        norm = np.sqrt((q * q).sum(axis=1, keepdims=True))
        q = q / np.where(norm > 0, norm, 1.0)
    return q @ rows.T, nviews


def scores32(features, queries, views="mean", cosine=False):
    """The same in fp32 on the CPU: queries normalised in fp32, one running fp32 sum per score over the columns in
    order (elementwise IEEE operations, the same on every CPU)."""
    rows = gallery_rows64(features, views, cosine)[0].astype(np.float32)
    q = np.asarray(queries, dtype=np.float32)
    if cosine:
        norm = np.sqrt((q * q).sum(axis=1, keepdims=True, dtype=np.float32))
        q = q / np.where(norm > 0, norm, np.float32(1.0))
    acc = np.zeros((q.shape[0], rows.shape[0]), dtype=np.float32)
    for c in range(q.shape[1]):
        acc += q[:, c:c + 1] * rows[:, c][None, :]
    return acc


def search64(features, queries, k, views="mean", cosine=False):
    """(scores [Q, k] float64, items, views or None) of the float64 ranking."""
    s, nviews = scores64(features, queries, views, cosine)
    k = min(k, s.shape[1])
    order = np.stack([np.lexsort((np.arange(s.shape[1]), -s[q]))[:k] for q in range(s.shape[0])])
    top = np.take_along_axis(s, order, axis=1)
    if nviews is None:
        return top, order, None
    return top, order // nviews, order % nviews


def recall64(audio, features, ks, views="mean", cosine=False):
    a = np.asarray(audio, dtype=np.float32)
    n, u, c = a.shape
    _, items, _ = search64(features, a.reshape(n * u, c), max(ks), views, cosine)
    own = np.repeat(np.arange(n), u)[:, None]
    return {k: float((items[:, :k] == own).any(axis=1).mean() * 100.0) for k in ks}


# ---- end-to-end cases ---------------------------------------------------------------------------------------------------
# (Q, N, C, V, views, (seed of the dot-product run, seed of the cosine run)); every case with k = E2E_K, chunk_rows 128 and
# the default.  The seeds are chosen so that the fp64 scores are separated as E2E_MARGIN asks.
E2E_K = 10
E2E_CASES = [(3, 70, 40, 1, "mean", (0, 0)), (5, 300, 1024, 10, "mean", (0, 0)), (33, 1000, 1024, 2, "all", (47, 248))]
# max|fp32 - fp64| / max|fp64| over the top-k scores of the fp64 ranking (measure_yardsticks; test_speech_search_cpu.py
# measures them again); the GPU bound is twice this
E2E_YARDSTICK = {("Q3_N70_C40_V1_mean", False): 1.274e-7, ("Q3_N70_C40_V1_mean", True): 1.891e-7,
                 ("Q5_N300_C1024_V10_mean", False): 8.625e-7, ("Q5_N300_C1024_V10_mean", True): 1.012e-6,
                 ("Q33_N1000_C1024_V2_all", False): 9.278e-7, ("Q33_N1000_C1024_V2_all", True): 1.217e-6}
E2E_BOUNDS = {key: 2 * y for key, y in E2E_YARDSTICK.items()}
# the ranking is only asked for where fp64 separates consecutive scores of the top k + 1 by more than this multiple of
# yardstick x max|score|: far outside what fp32 rounding can reorder
E2E_MARGIN = 100.0


def e2e_id(case):
    return "Q%d_N%d_C%d_V%d_%s" % tuple(case[:5])


def e2e_data(case, cosine):
    Q, N, C, V, views, seeds = case
    rng = np.random.RandomState(4000 + seeds[int(bool(cosine))])
    feats = rng.randn(N, V, C).astype(np.float32)
    queries = rng.randn(Q, C).astype(np.float32)
    return feats, queries


def top_scores_err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def e2e_separation(case, cosine):
    """(smallest gap between consecutive fp64 scores among each query's top k + 1, max|score| over the top k)."""
    feats, queries = e2e_data(case, cosine)
    top, _, _ = search64(feats, queries, E2E_K + 1, case[4], cosine)
    return float(np.min(top[:, :-1] - top[:, 1:])), float(np.abs(top[:, :E2E_K]).max())


def measure_yardsticks():
    out = {}
    for case in E2E_CASES:
        for cosine in (False, True):
            feats, queries = e2e_data(case, cosine)
            top, items, views = search64(feats, queries, E2E_K, case[4], cosine)
            rows = items if views is None else items * case[3] + views
            s32 = scores32(feats, queries, case[4], cosine)
            out[(e2e_id(case), cosine)] = top_scores_err(np.take_along_axis(s32, rows, axis=1), top)
    return out


if __name__ == "__main__":
    for key, y in measure_yardsticks().items():
        print(key, "%.3e" % y)
    for case in E2E_CASES:
        for cosine in (False, True):
            print(e2e_id(case), cosine, "gap %.3e max %.3e" % e2e_separation(case, cosine))
