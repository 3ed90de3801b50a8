"""Host side of the speech-image consistency score (no GPU here): the closed-form R-precision against brute-force
enumeration, rank_metrics on hand-made counters, the numpy restatement of the rank fold (tests/rank_ref.py) with its
chunking and the mutants it must tell apart, the s2i_rank_rows symbol and its refusals, and the refusal of a CPU device."""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_form_equals_enumeration_over_all_draws():
    from speech_to_image_translation_without_text_amd import retrieval
    for n in range(1, 8):
        for c in range(0, n + 1):
            for m in range(1, 5):
                want = R.r_precision_enumerated(n, c, m)
                assert R.r_precision_closed(n, c, m) == pytest.approx(want, abs=1e-15), (n, c, m)
                got = retrieval.rank_metrics([c], [0], [n], m=m)["r_precision"]
                assert got == pytest.approx(100.0 * want, abs=1e-12), (n, c, m, got, want)
                # a tie counts exactly as a loss does
                if c:
                    assert retrieval.rank_metrics([c - 1], [1], [n], m=m)["r_precision"] == got


def test_rank_metrics_on_hand_made_counters():
    from speech_to_image_translation_without_text_amd import retrieval
    gt = np.array([0, 0, 3, 9, 150])
    eq = np.array([0, 1, 1, 0, 0])
    n = np.array([200, 200, 200, 200, 200])
    got = retrieval.rank_metrics(gt, eq, n)                       # c = 0, 1, 4, 9, 150
    assert got["n_queries"] == 5 and got["n_skipped"] == 0
    assert got["recall@1"] == 20.0 and got["recall@5"] == 60.0 and got["recall@10"] == 80.0
    assert got["median_rank"] == 5.0
    # m = 99 of n = 200: c = 1 -> (200 - 99) / 200; c = 150 -> 0 (fewer than 99 stand below it)
    want = [1.0, 101 / 200.0, R.r_precision_closed(200, 4, 99), R.r_precision_closed(200, 9, 99), 0.0]
    assert got["r_precision"] == pytest.approx(100.0 * np.mean(want), rel=1e-13)
    ref = R.metrics(gt, eq, n)
    assert set(ref) == set(got)
    for k in ref:
        assert got[k] == pytest.approx(ref[k], rel=1e-13), k
    other = retrieval.rank_metrics(gt, eq, n, m=3, ks=(2, 50))
    assert other["recall@2"] == 40.0 and other["recall@50"] == 80.0 and "recall@1" not in other
    # torch tensors, as Gallery.rank returns them, are taken too
    import torch
    assert retrieval.rank_metrics(torch.from_numpy(gt.astype(np.int32)), torch.from_numpy(eq.astype(np.int32)), n) == got


def test_queries_without_candidates_are_skipped_and_m_is_clipped():
    from speech_to_image_translation_without_text_amd import retrieval
    got = retrieval.rank_metrics([0, 0, 2], [0, 0, 0], [0, 5, 5], m=99)
    assert got["n_queries"] == 2 and got["n_skipped"] == 1
    # m' = min(99, 5) = 5: c = 0 -> 1, c = 2 -> 0 (only 3 stand below it)
    assert got["r_precision"] == 50.0 and got["recall@1"] == 50.0 and got["median_rank"] == 2.0
    assert retrieval.rank_metrics([1], [0], [5], m=7)["r_precision"] == retrieval.rank_metrics([1], [0], [5], m=5)["r_precision"]
    assert retrieval.rank_metrics([1], [0], [5], m=4)["r_precision"] == pytest.approx(100.0 * 1 / 5)   # C(4,4) / C(5,4)
    empty = retrieval.rank_metrics([0], [0], [0])
    assert empty["n_queries"] == 0 and empty["n_skipped"] == 1 and np.isnan(empty["r_precision"])
    for bad in (([1], [0], [0]), ([3], [3], [5]), ([-1], [0], [5]), ([1, 2], [0], [5])):
        with pytest.raises(ValueError):
            retrieval.rank_metrics(*bad)
    with pytest.raises(ValueError):
        retrieval.rank_metrics([0], [0], [5], m=0)
    assert retrieval.other_class_counts([0, 1, 9], [0, 0, 1, 2, 2, 2]).tolist() == [4, 5, 6]


def test_reference_fold_by_hand_and_in_chunks():
    nan, inf = np.nan, np.inf
    #                 row  10    11    12   13    14    15   16    17
    s = np.array([[1.0, 3.0, nan, 3.0, -inf, inf, 2.0, 3.0]])
    rlabel = np.zeros(18, np.int32)
    rlabel[10:18] = [1, 2, 2, 1, 2, 2, 1, 2]
    gt, eq, own = R.rank_counts(s, [13], [1], rlabel, base=10)
    assert own.tolist() == [3.0]
    # other-class rows: 11 (3.0, tie), 12 (NaN, neither), 14 (-inf), 15 (+inf, above), 17 (3.0, tie); 10, 13, 16 are class 1
    assert (gt.tolist(), eq.tolist()) == ([1], [2])
    gt, eq, _ = R.rank_counts(s, [12], [2], rlabel, base=10)      # a NaN own score: all three class-1 rows count
    assert (gt.tolist(), eq.tolist()) == ([3], [0])
    gt, eq, own = R.rank_counts(s, [-1], [1], rlabel, base=10)    # no own row: compared with 0
    assert own.tolist() == [0.0] and (gt.tolist(), eq.tolist()) == ([3], [0])
    # chunking does not change a count, and every mutant is told apart on the exact-integer case
    qs, gal, own_row, ql, rl = R.case(3, 37, 301)
    sc = R.scores64(qs, gal)
    assert np.abs(sc).max() < 2 ** 24 and np.array_equal(sc, (qs @ gal.T).astype(np.float64))
    big = np.zeros(5 + 301, np.int32)
    big[5:] = rl
    big[:5] = 99
    one = R.rank_counts(sc, own_row + 5 * (own_row >= 0), ql, big, base=5)
    split = R.rank_counts(sc, own_row + 5 * (own_row >= 0), ql, big, base=5, chunks=[64, 1, 100, 136])
    for a, b in zip(one, split):
        assert np.array_equal(a, b)
    assert one[1].sum() > 12                                      # ties, natural and forced
    for mutant in R.MUTANTS:
        bad = R.rank_counts(sc, own_row + 5 * (own_row >= 0), ql, big, base=5, mutant=mutant)
        assert not (np.array_equal(bad[0], one[0]) and np.array_equal(bad[1], one[1])), mutant


def test_symbol_is_declared_exported_and_bound():
    from speech_to_image_translation_without_text_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    assert re.search(r"\bint s2i_rank_rows\(const float\* scores, int Q, int N, int lds, int base, const int\* own_row, "
                     r"const int\* query_label,\s+const int\* row_label, int n_labels, float\* own_score, int\* gt, "
                     r"int\* eq, int mode, void\* stream\);", header)
    assert "#define S2I_RANK_GATHER 0" in header and "#define S2I_RANK_COUNT 1" in header
    lib = _lib.load()
    assert hasattr(lib, "s2i_rank_rows") and "s2i_rank_rows" in _lib.EXPORTED_SYMBOLS
    assert (_lib.RANK_GATHER, _lib.RANK_COUNT) == (0, 1)
    makefile = open(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc", "Makefile")).read()
    assert "s2i_rank.hip" in makefile


def test_bad_arguments_are_refused_before_any_device_is_touched():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    f = (ctypes.c_float * 8)()
    i = (ctypes.c_int * 8)()
    fa, ia = ctypes.addressof(f), ctypes.addressof(i)               # host memory: never dereferenced

    def refused(word, scores=fa, Q=1, N=4, lds=4, base=0, own_row=ia, qlabel=ia, rlabel=ia, n_labels=8, own_score=fa,
                gt=ia, eq=ia, mode=_lib.RANK_COUNT):
        assert lib.s2i_rank_rows(scores, Q, N, lds, base, own_row, qlabel, rlabel, n_labels, own_score, gt, eq, mode,
                                 None) != 0
        msg = lib.s2i_last_error().decode()
        assert msg.startswith("rank_rows:") and word in msg, msg

    refused("null", scores=None)
    refused("null", own_score=None)
    refused("null", gt=None)
    refused("null", rlabel=None)
    refused("null", own_row=None, mode=_lib.RANK_GATHER)
    refused("mode", mode=2)
    refused("positive", Q=0)
    refused("positive", N=0)
    refused("stride", lds=3)
    refused("leave int", base=-1)
    refused("leave int", base=2 ** 31 - 3)
    refused("row labels", base=5)                                    # 5 + 4 > 8 labels
    refused("aligned", scores=fa + 2)


def test_wrapper_validates_and_there_is_no_cpu_fallback():
    import torch
    from speech_to_image_translation_without_text_amd import _lib, gan_metrics, ops, retrieval
    x = torch.zeros(2, 8)
    i32 = torch.zeros(2, dtype=torch.int32)
    f32 = torch.zeros(2)
    lab = torch.zeros(8, dtype=torch.int32)
    good = dict(scores=x, own_row=i32, query_label=i32, row_label=lab, base=0, own_score=f32, gt=i32.clone(),
                eq=i32.clone(), mode="count")
    for change in (dict(scores=torch.zeros(8)), dict(scores=x.double()), dict(scores=x.t()), dict(base=-1),
                   dict(base=2 ** 31 - 8), dict(mode="both")):
        with pytest.raises(ValueError):
            ops.rank_rows(**dict(good, **change))
    with pytest.raises(_lib.S2IError):
        ops.rank_rows(**good)                                        # CPU tensors
    with pytest.raises(_lib.S2IError):
        retrieval.Gallery(np.zeros((3, 2, 8), np.float32), "cpu", views="all")
    assert callable(retrieval.Gallery.rank)
    with pytest.raises(_lib.S2IError):
        gan_metrics.ConsistencyScorer(None, np.zeros((3, 2, 8), np.float32), [0, 1, 2], "cpu")


def test_command_line_flags_default_off():
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    base = ["--netG", "netG_1.pth", "--inception", "i.pth", "--data_dir", "d"]
    a = GM.parse_args(base)
    assert a.googlenet is None and a.consistency_cosine is False
    a = GM.parse_args(base + ["--googlenet", "g.caffemodel", "--consistency_cosine"])
    assert a.googlenet == "g.caffemodel" and a.consistency_cosine is True
