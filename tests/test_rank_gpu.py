"""GPU suite of the rank fold: s2i_rank_rows (ops.rank_rows) against tests/rank_ref.py with exact equality on scores that
are exact in fp32, at every size where the kernel takes another path (one column, a row shorter than a 16-byte load, one
wave and several, a second trip through the loop, row strides, bases and pointers that move the 16-byte boundary), with
sentinels around everything it writes; and retrieval.Gallery.rank against counts made in numpy from the scores of the
gallery's own launches."""
import numpy as np
import pytest
import torch

import rank_ref as R

pytestmark = pytest.mark.gpu

QS = (1, 5, 37)
NS = (1, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1030, 4100)       # 4100: four waves and a second trip through the loop
BASES = (0, 5, 2 ** 20)
GUARD = 8
SENT_I, SENT_F = -77777, -12345.5


def guarded(values, dtype, dev):
    """A device vector with GUARD sentinels on either side; returns (whole, the middle view)."""
    values = np.asarray(values)
    sent = SENT_F if dtype == torch.float32 else SENT_I
    whole = torch.full((values.shape[0] + 2 * GUARD,), sent, dtype=dtype)
    whole[GUARD:GUARD + values.shape[0]] = torch.from_numpy(values).to(dtype)
    whole = whole.to(dev)
    return whole, whole[GUARD:GUARD + values.shape[0]]


def guards_intact(whole):
    h = whole.cpu()
    sent = SENT_F if h.dtype == torch.float32 else SENT_I
    return bool((h[:GUARD] == sent).all() and (h[-GUARD:] == sent).all())


def strided_scores(scores, lds, off, dev):
    """The [Q, N] scores as a device view with row stride lds whose first element sits `off` floats past an allocation
    (which is 256-byte aligned); the gaps hold +inf, which would count if read."""
    Q, N = scores.shape
    buf = torch.full((off + Q * lds + 4,), float("inf"), dtype=torch.float32)
    view = buf[off:off + Q * lds].view(Q, lds)[:, :N]
    view.copy_(torch.from_numpy(np.asarray(scores, np.float32)))
    dbuf = buf.to(dev)
    return dbuf[off:off + Q * lds].view(Q, lds)[:, :N]


def labels_around(rlabel, base, seed):
    """Row labels of a whole gallery whose rows base .. base + N are `rlabel`; the rows around them carry other labels,
    so a kernel that ignored `base` or ran past N would count differently."""
    rng = np.random.RandomState(seed)
    full = rng.randint(0, 7, size=base + rlabel.shape[0] + 9).astype(np.int32)
    full[base:base + rlabel.shape[0]] = rlabel
    return full


def run_fold(dev, scores_d, own_row, qlabel, full_label, base, own0, gt0, eq0):
    from speech_to_image_translation_without_text_amd import ops
    own_w, own_s = guarded(own0, torch.float32, dev)
    gt_w, gt = guarded(gt0, torch.int32, dev)
    eq_w, eq = guarded(eq0, torch.int32, dev)
    row_d = torch.from_numpy(np.asarray(own_row, np.int32)).to(dev)
    ql_d = torch.from_numpy(np.asarray(qlabel, np.int32)).to(dev)
    rl_d = torch.from_numpy(full_label).to(dev)
    ops.rank_rows(scores_d, row_d, None, None, base, own_s, None, None, "gather")
    after_gather = own_s.cpu().numpy().copy()
    assert guards_intact(gt_w) and guards_intact(eq_w) and np.array_equal(gt.cpu().numpy(), gt0)   # gather writes no counter
    ops.rank_rows(scores_d, None, ql_d, rl_d, base, own_s, gt, eq, "count")
    torch.cuda.synchronize()
    assert guards_intact(own_w) and guards_intact(gt_w) and guards_intact(eq_w)
    assert np.array_equal(own_s.cpu().numpy(), after_gather, equal_nan=True)                       # count writes no score
    return after_gather, gt.cpu().numpy().astype(np.int64), eq.cpu().numpy().astype(np.int64)


def chunk_case(seed, Q, N, base):
    """One chunk of N rows at global rows base ..: own rows inside it, -1, and just outside it on either side."""
    qs, gal, own, ql, rl = R.case(seed, Q, N)
    sc = R.scores64(qs, gal)
    assert np.array_equal(sc.astype(np.float32).astype(np.float64), sc)
    own_row = np.where(own >= 0, own + base, -1).astype(np.int64)
    if Q >= 5:
        own_row[1] = base + N                      # the first row of the next chunk
        own_row[3] = base - 1 if base else base + N + 3
    rng = np.random.RandomState(seed + 5)
    own0 = rng.randint(-40, 40, size=Q).astype(np.float32)         # what an earlier chunk gathered
    gt0, eq0 = rng.randint(0, 1000, size=Q), rng.randint(0, 50, size=Q)
    return sc, own_row, ql, rl, own0, gt0, eq0


@pytest.mark.parametrize("N", NS)
def test_kernel_equals_the_reference_exactly(gpu, N):
    ties = 0
    for Q in QS:
        for base in BASES:
            sc, own_row, ql, rl, own0, gt0, eq0 = chunk_case(N * 7 + Q, Q, N, base)
            full = labels_around(rl, base, N + Q)
            want_own = R.gather(sc.astype(np.float32), own_row, base, own0)
            want_gt, want_eq = R.count(sc, ql, full, base, want_own.astype(np.float64), gt0, eq0)
            ties += int((want_eq - eq0).sum())
            for lds, off in ((N, 0), (N + 3, 0), (N, 1), (N + 3, 2)):
                got = run_fold(gpu, strided_scores(sc, lds, off, gpu), own_row, ql, full, base, own0, gt0, eq0)
                what = "Q %d N %d base %d lds %d off %d" % (Q, N, base, lds, off)
                assert np.array_equal(got[0], want_own), what
                assert np.array_equal(got[1], want_gt) and np.array_equal(got[2], want_eq), what
    print("N %d: %d ties counted" % (N, ties))
    if N >= 63:
        assert ties > 0


def test_chunks_of_a_gallery_equal_one_launch_and_a_rerun_is_identical(gpu):
    from speech_to_image_translation_without_text_amd import ops
    Q, rows = 37, 301
    qs, gal, own, ql, rl = R.case(3, Q, rows)
    sc = R.scores64(qs, gal)
    assert np.abs(sc).max() < 2 ** 24
    want_gt, want_eq, want_own = R.rank_counts(sc, own, ql, rl)
    print("301 rows: max |s| %d, %d ties" % (np.abs(sc).max(), want_eq.sum()))
    assert want_eq.sum() > 12
    own_d, ql_d, rl_d = (torch.from_numpy(np.asarray(a, np.int32)).to(gpu) for a in (own, ql, rl))
    results = []
    for chunks in ([rows], [64, 1, 100, 136], [64, 1, 100, 136]):
        cuts = np.concatenate([[0], np.cumsum(chunks)])
        own_s = torch.zeros(Q, device=gpu)
        gt = torch.zeros(Q, dtype=torch.int32, device=gpu)
        eq = torch.zeros(Q, dtype=torch.int32, device=gpu)
        parts = [torch.from_numpy(sc[:, a:b].astype(np.float32)).contiguous().to(gpu) for a, b in zip(cuts[:-1], cuts[1:])]
        for part, a in zip(parts, cuts[:-1]):
            ops.rank_rows(part, own_d, None, None, int(a), own_s, None, None, "gather")
        for part, a in zip(parts, cuts[:-1]):
            ops.rank_rows(part, None, ql_d, rl_d, int(a), own_s, gt, eq, "count")
        results.append((own_s.cpu().numpy(), gt.cpu().numpy(), eq.cpu().numpy()))
    for got in results:
        assert np.array_equal(got[0], want_own.astype(np.float32))
        assert np.array_equal(got[1], want_gt) and np.array_equal(got[2], want_eq)
    # every wrong rule is told apart by these inputs (at a base other than 0 for the rule that ignores it)
    big = labels_around(rl, 5, 1)
    got = run_fold(gpu, strided_scores(sc, rows, 0, gpu), own + 5 * (own >= 0), ql, big, 5, np.zeros(Q, np.float32),
                   np.zeros(Q, np.int64), np.zeros(Q, np.int64))
    assert np.array_equal(got[1], want_gt) and np.array_equal(got[2], want_eq)
    for mutant in R.MUTANTS:
        bad = R.rank_counts(sc, own + 5 * (own >= 0), ql, big, base=5, mutant=mutant)
        assert not (np.array_equal(bad[0], got[1]) and np.array_equal(bad[1], got[2])), mutant


def test_one_class_nan_and_infinite_scores(gpu):
    Q, N = 5, 257
    sc, own_row, ql, rl, own0, gt0, eq0 = chunk_case(11, Q, N, 0)
    # every row of the queries' class: nothing is counted, whatever the scores
    one = np.zeros(N, np.int32)
    got = run_fold(gpu, strided_scores(sc, N, 0, gpu), own_row, np.zeros(Q, np.int32), one, 0, own0, gt0, eq0)
    assert np.array_equal(got[1], gt0) and np.array_equal(got[2], eq0)
    # NaN and infinite candidates, infinite and NaN own scores
    s = sc.astype(np.float32)
    rng = np.random.RandomState(2)
    s[:, rng.choice(N, 40, replace=False)] = np.nan
    s[:, rng.choice(N, 30, replace=False)] = np.inf
    s[:, rng.choice(N, 30, replace=False)] = -np.inf
    own_row = np.array([7, 8, 9, 10, -1])
    s[0, 7], s[1, 8], s[2, 9], s[3, 10] = np.nan, np.inf, -np.inf, 5.0
    ql = rl[[7, 8, 9, 10, 0]]
    want_own = R.gather(s, own_row, 0, own0)
    assert np.isnan(want_own[0]) and want_own[1] == np.inf and want_own[2] == -np.inf
    want_gt, want_eq = R.count(s.astype(np.float64), ql, rl, 0, want_own.astype(np.float64), gt0, eq0)
    assert want_gt[0] - gt0[0] == int((rl != ql[0]).sum())          # a NaN own score ranks last
    assert want_eq[1] > eq0[1] and want_eq[2] > eq0[2]              # +inf ties +inf, -inf ties -inf
    for lds, off in ((N, 0), (N + 3, 1)):
        got = run_fold(gpu, strided_scores(s, lds, off, gpu), own_row, ql, rl, 0, own0, gt0, eq0)
        assert np.array_equal(got[0], want_own, equal_nan=True)
        assert np.array_equal(got[1], want_gt) and np.array_equal(got[2], want_eq)


@pytest.mark.parametrize("cosine", [False, True], ids=["dot", "cosine"])
def test_gallery_rank_equals_counts_from_its_own_scores(gpu, cosine, monkeypatch):
    from speech_to_image_translation_without_text_amd import ops, retrieval
    monkeypatch.setattr(retrieval, "QUERY_BLOCK", 5)
    N, S, C, Q = 23, 3, 50, 13                                       # C = 50: padded to 52
    rng = np.random.RandomState(4)
    feats = rng.randn(N, S, C).astype(np.float32)
    feats[4, 1] = feats[17, 2]                                       # equal rows in different classes: exact ties
    labels = (np.arange(N) % 6).astype(np.int32)
    rlabel = np.repeat(labels, S)
    item = rng.randint(0, N, size=Q)
    sent = rng.randint(0, S, size=Q)
    item[0], sent[0] = 17, 2
    own = item * S + sent
    own[4] = -1
    queries = (feats[item, sent] + 0.5 * rng.randn(Q, C)).astype(np.float32)
    queries[0] = feats[17, 2]
    rows = N * S
    results = []
    for chunk_rows in (7, 64, rows):
        g = retrieval.Gallery(feats, gpu, views="all", cosine=cosine, chunk_rows=chunk_rows)
        assert g.rows == rows
        gt, eq = g.rank(queries, own, labels[item], rlabel)
        assert gt.dtype == torch.int32 and eq.dtype == torch.int32 and gt.device.type == "cuda"
        assert g._scores.numel() <= 5 * min(chunk_rows, rows)        # nothing of size Q x rows
        # the scores of the gallery's own launches, block by block and chunk by chunk, on the host
        q = g._prepare(torch.from_numpy(queries))
        host = np.zeros((Q, rows), np.float32)
        scratch = torch.empty(5 * min(chunk_rows, rows), device=gpu)
        for q0 in range(0, Q, 5):
            for start, n, packed in g.chunks:
                host[q0:q0 + 5, start:start + n] = ops.score_rows(q[q0:q0 + 5], packed, n, scratch).cpu().numpy()
        want_gt, want_eq, _ = R.rank_counts(host.astype(np.float64), own, labels[item], rlabel)
        assert np.array_equal(gt.cpu().numpy(), want_gt) and np.array_equal(eq.cpu().numpy(), want_eq), chunk_rows
        results.append((gt.cpu().numpy(), eq.cpu().numpy()))
        again = g.rank(queries, own, labels[item], rlabel)
        assert torch.equal(again[0], gt) and torch.equal(again[1], eq)
    print("cosine %s: gt %s eq %s" % (cosine, results[0][0].tolist(), results[0][1].tolist()))
    assert results[0][1][0] >= 1                                     # the duplicated row of another class ties query 0
    m = retrieval.rank_metrics(*results[0], retrieval.other_class_counts(labels[item], rlabel))
    assert m["n_queries"] == Q and 0.0 <= m["r_precision"] <= 100.0
    with pytest.raises(ValueError):
        g.rank(queries, own[:-1], labels[item], rlabel)
    with pytest.raises(ValueError):
        g.rank(queries, np.full(Q, rows), labels[item], rlabel)
