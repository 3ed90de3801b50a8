"""Host side of the search by speech (no GPU here): the s2i_topk_rows symbol and its refusals, the numpy restatement of
the selection and its chunked merge (tests/topk_ref.py) with the mutants it must tell apart, recall_at_k's counting, the
parsers, the unchanged retrieval JSON line, and the seeds and yardsticks of the end-to-end GPU cases."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    from speech_to_image_translation_without_text_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    assert re.search(r"\bint s2i_topk_rows\(const float\* scores, int Q, int N, int lds, int base, int k, "
                     r"float\* best_score, int\* best_row,\s+int merge, void\* stream\);", header)
    assert "#define S2I_ABI_VERSION 7" in header
    lib = _lib.load()
    assert hasattr(lib, "s2i_topk_rows") and "s2i_topk_rows" in _lib.EXPORTED_SYMBOLS
    assert lib.s2i_version() == _lib.ABI_VERSION == 7
    assert _lib.TOPK_MAX == 64
    makefile = open(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc", "Makefile")).read()
    assert "s2i_topk.hip" in makefile


def test_bad_arguments_are_refused_before_any_device_is_touched():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int * 64)()
    s, bs, br = ctypes.addressof(f), ctypes.addressof(f), ctypes.addressof(i)   # host memory: never dereferenced

    def refused(word, scores=s, Q=1, N=4, lds=4, base=0, k=2, best_score=bs, best_row=br):
        assert lib.s2i_topk_rows(scores, Q, N, lds, base, k, best_score, best_row, 0, None) != 0
        msg = lib.s2i_last_error().decode()
        assert msg.startswith("topk_rows:") and word in msg, msg

    refused("null", scores=None)
    refused("null", best_score=None)
    refused("null", best_row=None)
    refused("k 0", k=0)
    refused("k 65", k=65)
    refused("Q 0", Q=0)
    refused("N 0", N=0)
    refused("stride", lds=3)
    refused("row ids", base=-1)
    refused("row ids", base=2 ** 31 - 4)          # base + N = 2^31: one past int
    refused("row ids", base=2 ** 31 - 1, N=1, lds=1)


def test_ops_wrapper_checks_its_arguments_and_has_no_cpu_fallback():
    import torch
    from speech_to_image_translation_without_text_amd import _lib, ops
    x = torch.zeros(2, 8)
    for bad, kw in ((torch.zeros(8), {}), (x.double(), {}), (x.t(), {}), (x, {"k": 0}), (x, {"k": 65}), (x, {"base": -1}),
                    (x, {"base": 2 ** 31 - 8})):
        with pytest.raises(ValueError):
            ops.topk_rows(bad, kw.pop("k", 2), **kw)
    with pytest.raises(ValueError):
        ops.topk_rows(x, 2, best=(torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.int32)),
                      out=(torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.int32)))
    with pytest.raises(_lib.S2IError):
        ops.topk_rows(x, 2)                        # a CPU tensor
    from speech_to_image_translation_without_text_amd import retrieval
    with pytest.raises(_lib.S2IError):
        retrieval.Gallery(np.zeros((3, 2, 8), np.float32), "cpu")


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _plans(N):
    """Chunk plans that cut N differently: the GPU test's, single rows, a ragged fixed size."""
    plans = [R.MERGE_SIZES, (1,) * min(N, 3), (max(1, N // 3),) * 3]
    return [p for p in plans if len(R.chunk_starts(N, p)) > 1] or [R.MERGE_SIZES]


def _truth(case, pattern):
    Q, N, k, _, base = case
    x = R.make_scores(Q, N, k, pattern)
    return x, R.topk(x, k, base)


def test_one_shot_selection_follows_the_rule_on_hand_made_rows():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([[1.0, 3.0, nan, 3.0, -inf, inf, -0.0, 0.0]], dtype=np.float32)
    s, r = R.topk(x, 8, base=10)
    assert r.tolist() == [[15, 11, 13, 10, 16, 17, 12, 14]]          # 3.0 ties and +-0 by row; NaN with -inf by row
    assert R.same_bits(s, x[:, [5, 1, 3, 0, 6, 7, 2, 4]])             # the NaN and the -0 come back as they went in
    s, r = R.topk(x[:, :3], 5)
    assert r.tolist() == [[1, 0, 2, -1, -1]] and np.isneginf(s[0, 3:]).all() and np.isnan(s[0, 2])
    # an empty slot ranks behind a real -inf row when a pair is merged
    s2, r2 = R.merge((s, r), np.array([[-inf, 2.0]], dtype=np.float32), 5, base=3)
    assert r2.tolist() == [[1, 4, 0, 2, 3]]


@pytest.mark.parametrize("case", R.SELECT_CASES, ids=R.case_id)
def test_chunked_merge_equals_one_shot_selection(case):
    Q, N, k, _, base = case
    for pattern in R.PATTERNS:
        x, (s, r) = _truth(case, pattern)
        assert s.shape == (Q, k) and r.dtype == np.int32
        assert ((r == -1).sum(axis=1) == max(0, k - N)).all()
        for plan in _plans(N):
            cs, cr = R.chunked(x, k, plan, base)
            assert R.same_bits(cs, s) and (cr == r).all(), (pattern, plan)


@pytest.mark.parametrize("name", sorted(R.MUTANTS))
def test_each_mutant_differs_from_the_truth_on_a_listed_case(name):
    caught = []
    for case in R.SELECT_CASES:
        Q, N, k, _, base = case
        for pattern in R.PATTERNS:
            x, (s, r) = _truth(case, pattern)
            cs, cr = R.MUTANTS[name](x, k, R.MERGE_SIZES, base)
            if not (R.same_bits(cs, s) and (cr == r).all()):
                caught.append((R.case_id(case), pattern))
    print(name, caught)
    assert caught, name
    merge_ids = {R.case_id(c) for c in R.MERGE_CASES}
    if name in ("boundary_drops_one", "merge_drops_base"):       # the GPU merge test runs exactly these cases
        assert any(cid in merge_ids for cid, _ in caught), caught


# ---- recall_at_k, the parsers, the unchanged JSON line ---------------------------------------------------------------------
class _FakeGallery:
    """search() answers from the float64 restatement: recall_at_k's counting needs no device."""

    def __init__(self, feats, views="mean"):
        self.feats, self.views, self.items = feats, views, len(feats)

    def search(self, queries, k):
        import torch
        s, items, views = R.search64(self.feats, queries, k, self.views)
        return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(items), None


def test_recall_at_k_on_a_hand_made_case():
    from speech_to_image_translation_without_text_amd import retrieval
    feats = np.eye(4, dtype=np.float32)[:, None, :]                                # item i is axis i
    audio = np.zeros((4, 2, 4), dtype=np.float32)
    for i in range(4):
        audio[i, 0] = [4 - abs(i - j) for j in range(4)]                           # own item first
    audio[0, 1] = [1, 9, 0, 0]                                                      # own item second
    audio[1, 1] = [3, 1, 9, 5]                                                      # own item fourth
    audio[2, 1] = [0, 0, 9, 1]                                                      # first
    audio[3, 1] = [9, 5, 3, 1]                                                      # fourth
    got = retrieval.recall_at_k(audio, _FakeGallery(feats), ks=(1, 2, 3, 4))
    assert got == {1: 62.5, 2: 75.0, 3: 75.0, 4: 100.0}
    assert got == R.recall64(audio, feats, (1, 2, 3, 4))
    with pytest.raises(ValueError):
        retrieval.recall_at_k(audio[:3], _FakeGallery(feats))
    with pytest.raises(ValueError):
        retrieval.recall_at_k(audio, _FakeGallery(feats), ks=(0,))


def test_gallery_rows_follow_the_float64_rules():
    from speech_to_image_translation_without_text_amd import retrieval
    rng = np.random.RandomState(3)
    feats = rng.randn(6, 3, 8).astype(np.float32)
    feats[2] = 0                                                                    # an all-zero item stays zero
    for views in ("mean", "all"):
        for cosine in (False, True):
            rows, items, nviews = retrieval.gallery_rows(list(feats), views, cosine)
            ref, ref_views = R.gallery_rows64(feats, views, cosine)
            assert rows.dtype == np.float32 and items == 6 and nviews == ref_views
            assert np.array_equal(rows.astype(np.float64), ref)
    rows, items, nviews = retrieval.gallery_rows(feats[:, 0], "all", False)
    assert rows.shape == (6, 8) and nviews is None
    with pytest.raises(ValueError):
        retrieval.gallery_rows(np.zeros((0, 3, 8)), "mean")


def test_parsers():
    from speech_to_image_translation_without_text_amd import retrieval, speech_search
    a = retrieval.get_parser().parse_args(["--audio", "a.pickle", "--image", "i.pickle"])
    assert a.recall is False
    assert retrieval.get_parser().parse_args(["--audio", "a", "--image", "i", "--recall"]).recall is True
    p = speech_search.get_parser()
    a = p.parse_args(["--model", "m.pt", "--image", "i.pickle", "--data_dir", "d", "x.wav", "y.wav"])
    assert (a.topk, a.views, a.cosine, a.resample, a.out, a.split, a.dataset, a.bidirectional, a.wavs) == \
        (10, "mean", False, False, None, "test", "birds", False, ["x.wav", "y.wav"])
    assert a.chunk_rows == retrieval.GALLERY_CHUNK_ROWS
    a = p.parse_args(["--model", "m.pt", "--bidirectional", "--image", "i.pickle", "--dataset", "flowers", "--data_dir", "d",
                      "--split", "train", "--topk", "50", "--views", "all", "--cosine", "--resample", "--out", "h.jsonl",
                      "x.wav"])
    assert (a.topk, a.views, a.cosine, a.resample, a.out, a.split, a.dataset, a.bidirectional) == \
        (50, "all", True, True, "h.jsonl", "train", "flowers", True)
    for bad in (["--image", "i", "--data_dir", "d", "x.wav"], ["--model", "m", "--image", "i", "--data_dir", "d"],
                ["--model", "m", "--image", "i", "--data_dir", "d", "--views", "max", "x.wav"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_a_gallery_that_disagrees_with_the_split_json_is_refused(tmp_path):
    from speech_to_image_translation_without_text_amd import datasets, speech_search
    with open(tmp_path / "test.json", "w") as f:
        json.dump({"image_base_path": "/img", "data": [{"image": "a.jpg"}, {"image": "b.jpg"}, {"image": "c.jpg"}]}, f)
    pickle_path = str(tmp_path / "feat.pickle")
    datasets.save_embedding_pickle(np.zeros((2, 10, 8), np.float32), pickle_path)
    with pytest.raises(ValueError, match=r"holds 2 items .* lists 3 images"):
        speech_search.load_gallery(pickle_path, str(tmp_path), "test", "birds", "cpu")


def test_retrieval_json_line_without_recall_is_unchanged(tmp_path, capsys):
    from speech_to_image_translation_without_text_amd import datasets, retrieval
    rng = np.random.RandomState(0)
    audio, image = rng.randn(6, 10, 8).astype(np.float32), rng.randn(6, 10, 8).astype(np.float32)
    datasets.save_embedding_pickle(audio, str(tmp_path / "audio.pickle"))
    datasets.save_embedding_pickle(image, str(tmp_path / "image.pickle"))
    with open(tmp_path / "test.json", "w") as f:
        json.dump({"data": [{"class": "%03d.x" % (1 + i % 3)} for i in range(6)]}, f)
    accu, ap = retrieval.main(["--audio", str(tmp_path / "audio.pickle"), "--image", str(tmp_path / "image.pickle"),
                               "--data_dir", str(tmp_path), "--seed", "2"])
    labels = [1 + i % 3 for i in range(6)]
    assert (accu, ap) == retrieval.eval_features(audio, image, labels, 2, 50)
    expect = json.dumps({"split": "test", "items": 6, "seed": 2, "accu": accu, "ap50": ap}) + "\n"
    assert capsys.readouterr().out == expect
    assert open(tmp_path / "retrieval_test.json").read() == expect
    assert list(json.loads(expect)) == ["split", "items", "seed", "accu", "ap50"]


# ---- the end-to-end cases of the GPU test ---------------------------------------------------------------------------------
def test_end_to_end_seeds_separate_the_scores_and_the_yardsticks_are_as_recorded():
    """For the reference alone: in float64 the consecutive scores of each query's top k + 1 lie more than
    E2E_MARGIN x yardstick x max|score| apart, so an fp32 ranking must agree with it row for row; and the recorded
    yardsticks are what the fp32 restatement gives (one running sum per score, elementwise IEEE operations)."""
    got = R.measure_yardsticks()
    assert set(got) == set(R.E2E_YARDSTICK) == {(R.e2e_id(c), cos) for c in R.E2E_CASES for cos in (False, True)}
    for case in R.E2E_CASES:
        for cosine in (False, True):
            key = (R.e2e_id(case), cosine)
            y = R.E2E_YARDSTICK[key]
            gap, top = R.e2e_separation(case, cosine)
            print(key, "yardstick %.3e (recorded %.3e) gap %.3e margin %.3e" % (got[key], y, gap, R.E2E_MARGIN * y * top))
            assert got[key] == pytest.approx(y, rel=0.01)
            assert R.E2E_BOUNDS[key] == 2 * y
            assert gap > R.E2E_MARGIN * y * top, key
    assert [c[:4] for c in R.E2E_CASES] == [(3, 70, 40, 1), (5, 300, 1024, 10), (33, 1000, 1024, 2)]
    assert [c[4] for c in R.E2E_CASES] == ["mean", "mean", "all"]
