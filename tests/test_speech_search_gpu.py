"""Search by speech on the MI355X: s2i_topk_rows bit for bit against the numpy restatement (tests/topk_ref.py) on every
listed case and pattern, between guard bands; the chunked merge against the one-shot selection; retrieval.Gallery.search
and recall_at_k against the float64 restatement (row ids exactly, scores within twice the fp32 yardstick); and the
speech_search CLI on two generated WAVs and a 12-item gallery."""
import json
import os
import wave

import numpy as np
import pytest
import torch

import topk_ref as R

pytestmark = pytest.mark.gpu

GUARD = 128
ROW_SENTINEL = -77777777


def _guarded(Q, k, dev):
    """((score view, row view), check): a [Q, k] pair in the middle of buffers whose bands must come back untouched."""
    fs = torch.full((Q * k + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    fr = torch.full((Q * k + 2 * GUARD,), ROW_SENTINEL, dtype=torch.int32, device=dev)
    pair = (fs[GUARD:GUARD + Q * k].view(Q, k), fr[GUARD:GUARD + Q * k].view(Q, k))

    def check(what):
        for band in (fs[:GUARD], fs[GUARD + Q * k:]):
            assert bool(torch.isnan(band).all()), "%s: score guard band written" % (what,)
        for band in (fr[:GUARD], fr[GUARD + Q * k:]):
            assert bool((band == ROW_SENTINEL).all()), "%s: row guard band written" % (what,)
    return pair, check


def _device_scores(x, lds, dev):
    """x [Q, N] on the device with row stride lds; the padding columns hold +inf, which would win if they were read."""
    Q, N = x.shape
    if not lds:
        return torch.from_numpy(x).to(dev)
    full = torch.full((Q, lds), float("inf"), dtype=torch.float32, device=dev)
    full[:, :N] = torch.from_numpy(x).to(dev)
    return full[:, :N]


def _assert_same(got, ref, what):
    gs, gr = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (gr == ref[1]).all(), "%s: rows differ at %s" % (what, np.argwhere(gr != ref[1])[:5].tolist())
    assert R.same_bits(gs, ref[0]), "%s: score bits differ" % (what,)


@pytest.mark.parametrize("case", R.SELECT_CASES, ids=R.case_id)
def test_selection_is_bit_exact_between_guard_bands(gpu, case):
    from speech_to_image_translation_without_text_amd import ops
    Q, N, k, lds, base = case
    for pattern in R.PATTERNS:
        x = R.make_scores(Q, N, k, pattern)
        ref = R.topk(x, k, base)
        pair, check = _guarded(Q, k, gpu)
        got = ops.topk_rows(_device_scores(x, lds, gpu), k, base=base, out=pair)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == pair[0].data_ptr() and got[1].data_ptr() == pair[1].data_ptr()
        _assert_same(got, ref, (R.case_id(case), pattern))
        check((R.case_id(case), pattern))
    # fresh tensors when no pair is given
    s, r = ops.topk_rows(_device_scores(x, lds, gpu), k, base=base)
    assert s.shape == (Q, k) and s.dtype == torch.float32 and r.dtype == torch.int32
    _assert_same((s, r), ref, "fresh")


@pytest.mark.parametrize("case", R.MERGE_CASES, ids=R.case_id)
def test_chunked_merge_equals_the_one_shot_selection(gpu, case):
    from speech_to_image_translation_without_text_amd import ops
    Q, N, k = case
    base = 3
    for pattern in R.PATTERNS:
        x = R.make_scores(Q, N, k, pattern)
        ref = R.topk(x, k, base)
        xd = torch.from_numpy(x).to(gpu)
        one = ops.topk_rows(xd, k, base=base)
        pair, check = _guarded(Q, k, gpu)
        chunks = R.chunk_starts(N, R.MERGE_SIZES)
        # 1, 7, 64 and 4096 rows, then the rest (at N = 4097 the fourth chunk is cut short and nothing is left)
        assert [e - s for s, e in chunks[:3]] == [1, 7, 64] and chunks[3][1] == min(N, 4168) and chunks[-1][1] == N
        for i, (s, e) in enumerate(chunks):
            if i == 0:
                ops.topk_rows(xd[:, s:e], k, base=base + s, out=pair)
            else:
                got = ops.topk_rows(xd[:, s:e], k, base=base + s, best=pair)
                assert got[0].data_ptr() == pair[0].data_ptr()
        torch.cuda.synchronize()
        _assert_same(pair, ref, (R.case_id(case), pattern, "chunked"))
        _assert_same(one, ref, (R.case_id(case), pattern, "one shot"))
        check((R.case_id(case), pattern))


def test_mutants_are_told_apart_by_what_the_gpu_returns(gpu):
    """The comparison above has teeth: each mutant of the restatement disagrees with the kernel's chunked result."""
    from speech_to_image_translation_without_text_amd import ops
    Q, N, k = R.MERGE_CASES[1]
    for name, patterns in (("tie_high", ("equal",)), ("boundary_drops_one", ("descending",)),
                           ("merge_drops_base", ("normal",)), ("nan_first", ("specials",))):
        for pattern in patterns:
            x = R.make_scores(Q, N, k, pattern)
            xd = torch.from_numpy(x).to(gpu)
            pair = None
            for i, (s, e) in enumerate(R.chunk_starts(N, R.MERGE_SIZES)):
                pair = ops.topk_rows(xd[:, s:e], k, base=s, best=pair)
            ms, mr = R.MUTANTS[name](x, k, R.MERGE_SIZES, 0)
            assert not ((pair[1].cpu().numpy() == mr).all() and R.same_bits(pair[0].cpu().numpy(), ms)), name


# ---- Gallery ----------------------------------------------------------------------------------------------------------------
_E2E_REF = {}


def _e2e_ref(case, cosine):
    key = (R.e2e_id(case), cosine)
    if key not in _E2E_REF:
        feats, queries = R.e2e_data(case, cosine)
        _E2E_REF[key] = (feats, queries, R.search64(feats, queries, R.E2E_K, case[4], cosine))
    return _E2E_REF[key]


@pytest.mark.parametrize("cosine", [False, True], ids=["dot", "cosine"])
@pytest.mark.parametrize("chunk_rows", [128, None], ids=["chunk128", "default"])
@pytest.mark.parametrize("case", R.E2E_CASES, ids=R.e2e_id)
def test_gallery_search_against_float64(gpu, case, chunk_rows, cosine):
    from speech_to_image_translation_without_text_amd import retrieval
    Q, N, C, V, views, _ = case
    feats, queries, (ref_s, ref_items, ref_views) = _e2e_ref(case, cosine)
    kw = {} if chunk_rows is None else {"chunk_rows": chunk_rows}
    gal = retrieval.Gallery(list(feats), gpu, views=views, cosine=cosine, **kw)
    assert gal.rows == (N * V if views == "all" else N) and gal.items == N and gal.dim == C
    assert len(gal.chunks) == -(-gal.rows // gal.chunk_rows) and gal.nbytes >= gal.rows * C * 4
    s, items, vw = gal.search(torch.from_numpy(queries).to(gpu), R.E2E_K)
    torch.cuda.synchronize()
    assert s.shape == (Q, R.E2E_K) and s.dtype == torch.float32 and s.device.type == "cuda"
    assert items.dtype == torch.int64 and items.device.type == "cuda"
    assert (items.cpu().numpy() == ref_items).all(), "items differ for queries %s" % (
        np.unique(np.argwhere(items.cpu().numpy() != ref_items)[:, 0]).tolist(),)
    if views == "all":
        assert vw.dtype == torch.int64 and (vw.cpu().numpy() == ref_views).all()
    else:
        assert vw is None and ref_views is None
    err = R.top_scores_err(s.cpu().numpy(), ref_s)
    key = (R.e2e_id(case), cosine)
    print("%s chunk_rows %s: score error %.3e (yardstick %.3e, bound %.3e)"
          % (key, gal.chunk_rows, err, R.E2E_YARDSTICK[key], R.E2E_BOUNDS[key]))
    assert err <= R.E2E_BOUNDS[key]
    # host arrays are taken too, and a query's answer does not depend on its neighbours
    s2, items2, _ = gal.search(queries[:2], R.E2E_K)
    assert torch.equal(items2, items[:2]) and torch.equal(s2, s[:2])


def test_search_refusals(gpu):
    from speech_to_image_translation_without_text_amd import retrieval
    gal = retrieval.Gallery(np.random.RandomState(0).randn(100, 8).astype(np.float32), gpu)
    assert gal.nviews is None and gal.rows == 100
    with pytest.raises(ValueError):
        gal.search(np.zeros((2, 9), np.float32), 5)
    with pytest.raises(ValueError):
        gal.search(np.zeros((2, 8), np.float32), 65)
    with pytest.raises(ValueError):
        gal.search(np.zeros((2, 8), np.float32), 0)
    with pytest.raises(ValueError):
        retrieval.Gallery(np.zeros((4, 8), np.float32), gpu, views="max")
    # k is clipped to the rows; a ragged feature width is padded for the matrix kernel and changes nothing
    feats = np.random.RandomState(1).randn(12, 3, 10).astype(np.float32)
    queries = np.random.RandomState(2).randn(4, 10).astype(np.float32)
    s, items, views = retrieval.Gallery(feats, gpu, views="all", chunk_rows=5).search(queries, 50)
    ref_s, ref_items, ref_views = R.search64(feats, queries, 50, "all")
    assert s.shape == (4, 36) and (items.cpu().numpy() == ref_items).all() and (views.cpu().numpy() == ref_views).all()
    assert R.top_scores_err(s.cpu().numpy(), ref_s) < 1e-6


@pytest.mark.parametrize("views", ["mean", "all"])
def test_recall_at_k_against_the_restatement(gpu, views):
    from speech_to_image_translation_without_text_amd import retrieval
    rng = np.random.RandomState(11)
    N, U, V, C = 40, 3, 2, 64
    feats = rng.randn(N, V, C).astype(np.float32)
    audio = (0.35 * feats.mean(axis=1)[:, None, :] + rng.randn(N, U, C)).astype(np.float32)
    ks = (1, 5, 10, 50)
    gal = retrieval.Gallery(feats, gpu, views=views, chunk_rows=32)
    got = retrieval.recall_at_k(audio, gal, ks)
    ref = R.recall64(audio, feats, tuple(min(k, gal.rows) for k in ks), views)
    print(views, got)
    assert list(got) == list(ks)
    assert [got[k] for k in ks] == [ref[min(k, gal.rows)] for k in ks]
    assert 0.0 < got[1] < got[10] <= got[50] <= 100.0          # neither trivial nor saturated at the top


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def _write_wav(path, seconds, seed):
    rng = np.random.RandomState(seed)
    n = int(16000 * seconds)
    t = np.arange(n) / 16000.0
    sig = 0.3 * np.sin(2 * np.pi * (200 + 70 * seed) * t) + 0.05 * rng.randn(n)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def test_cli_ranks_as_float64_ranks_the_embeddings(gpu, tmp_path, capsys):
    from encoder_ref import build_encoder
    from speech_to_image_translation_without_text_amd import datasets, encoder_train, speech_search, speech_to_image
    from speech_to_image_translation_without_text_amd.extract_audio_feature import load_encoder, read_wavs
    root = str(tmp_path)
    model = os.path.join(root, "encoder.pt")
    encoder_train.HeadTrainer(build_encoder()).save(model, 1)
    wavs = [os.path.join(root, "a.wav"), os.path.join(root, "b.wav")]
    for i, w in enumerate(wavs):
        _write_wav(w, 1.0, i + 1)
    feats = np.random.RandomState(5).randn(12, 10, 1024).astype(np.float32)
    pickle_path = os.path.join(root, "test", "image_features.pickle")
    datasets.save_embedding_pickle(feats, pickle_path)
    with open(os.path.join(root, "test.json"), "w") as f:
        json.dump({"image_base_path": "/birds", "data": [{"image": "cls%d/img%02d.jpg" % (i % 3, i)} for i in range(12)]}, f)
    common = ["--model", model, "--bidirectional", "--image", pickle_path, "--dataset", "birds", "--data_dir", root]

    with torch.no_grad():
        emb = speech_to_image.embed(load_encoder(model, True, 1, gpu), read_wavs(wavs)).cpu().numpy()
    ref_s, ref_items, _ = R.search64(feats, emb, 12, "mean")
    assert np.min(ref_s[:, :-1] - ref_s[:, 1:]) > 1e-3 * np.abs(ref_s).max()      # nothing fp32 could reorder

    capsys.readouterr()
    speech_search.main(common + ["--topk", "5"] + wavs)
    lines = [json.loads(t) for t in capsys.readouterr().out.strip().split("\n")]
    assert [ln["wav"] for ln in lines] == wavs
    for q, ln in enumerate(lines):
        assert [h["rank"] for h in ln["hits"]] == [1, 2, 3, 4, 5]
        assert [h["image"] for h in ln["hits"]] == [
            os.path.join("/birds", "images", "cls%d/img%02d.jpg" % (i % 3, i)) for i in ref_items[q, :5]]
        assert all(h["view"] is None for h in ln["hits"])
        assert np.allclose([h["score"] for h in ln["hits"]], ref_s[q, :5], rtol=0, atol=1e-5 * np.abs(ref_s).max())

    out = os.path.join(root, "hits.jsonl")
    got = speech_search.main(common + ["--topk", "50", "--views", "all", "--cosine", "--out", out] + wavs)
    printed = capsys.readouterr().out
    assert open(out).read() == printed and [json.loads(t) for t in printed.strip().split("\n")] == got
    cos_s, cos_items, cos_views = R.search64(feats, emb, 50, "all", True)
    for q, ln in enumerate(got):
        assert len(ln["hits"]) == 50 and [h["view"] for h in ln["hits"]][:3] == cos_views[q, :3].tolist()
        assert ln["hits"][0]["image"].endswith("img%02d.jpg" % cos_items[q, 0])
    mean_all = speech_search.main(common + ["--topk", "50"] + wavs)
    assert [len(ln["hits"]) for ln in mean_all] == [12, 12]                         # clipped to the gallery
    assert [[h["image"] for h in ln["hits"][:5]] for ln in mean_all] == [[h["image"] for h in ln["hits"]] for ln in lines]

    # the refusals of the stages it is built from
    short = os.path.join(root, "short.wav")
    _write_wav(short, 0.3, 9)
    with pytest.raises(ValueError, match="shorter than 64 frames"):
        speech_search.main(common + [short])
    with open(os.path.join(root, "test.json"), "w") as f:
        json.dump({"image_base_path": "/birds", "data": [{"image": "x.jpg"}] * 11}, f)
    with pytest.raises(ValueError, match="holds 12 items .* lists 11 images"):
        speech_search.main(common + wavs)
