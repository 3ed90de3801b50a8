"""GPU suite of the speech-image consistency score: GoogLeNetFeatures.rows (device images in, device rows out) against
the host-upload path bit for bit and its ten-view mean against float64; gan_metrics.ConsistencyScorer against
tests/rank_ref.py on the rows it kept; score_generator with and without a consistency scorer; the command line end to
end.  Seeded GoogLeNet, Inception and generator weights at the small widths of tests/test_gan_metrics_gpu.py: no value
of the metric itself means anything here."""
import json
import pickle

import numpy as np
import pytest
import torch

import googlenet_ref as GR
import rank_ref as R
from helpers import CASES, build_nets, configure, make_cub_tree, random_state_dict

pytestmark = pytest.mark.gpu

CASE = dict(CASES['small3'], t=1024)        # the speech embedding is as wide as pool5: the two share one space
SENTENCES = 2


@pytest.fixture(scope="module")
def googlenet(gpu):
    from speech_to_image_translation_without_text_amd import googlenet as G
    w = GR.random_weights(0)
    return G.GoogLeNetFeatures(w, gpu), w


def inception_weights():
    sd = random_state_dict(seed=5)
    sd["fc.weight"] = sd["fc.weight"] * 0.01       # no posterior underflows to 0 (log(0) makes IS nan)
    return sd


def synthetic_loader(case, sizes=(3, 2), sentences=SENTENCES, seed=11):
    g = torch.Generator().manual_seed(seed)
    out, k = [], 0
    for B in sizes:
        imgs = [torch.rand(B, 3, 64 * 2 ** i, 64 * 2 ** i, generator=g) * 2 - 1 for i in range(3)]
        emb = torch.randn(B, sentences, case['t'], generator=g)
        out.append((imgs, emb, ["bird%d/img%d" % (j % 2, j) for j in range(k, k + B)]))
        k += B
    return out


@pytest.fixture(scope="module")
def generator(gpu):
    netG, _ = build_nets(CASE)
    gsd = torch.Generator().manual_seed(3)
    for k, v in netG.state_dict().items():         # non-trivial running statistics
        if k.endswith('running_mean'):
            v.copy_(0.1 * torch.randn(v.shape, generator=gsd))
        elif k.endswith('running_var'):
            v.copy_(0.5 + torch.rand(v.shape, generator=gsd))
    yield netG.to(gpu)
    configure(CASES['small3'])


# ---- GoogLeNetFeatures.rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 49])          # 49 = MAX_BATCH + 1: a second chunk of one image
def test_rows_equal_the_host_upload_path_and_the_mean_is_within_its_bound(gpu, googlenet, B):
    from speech_to_image_translation_without_text_amd import _lib, googlenet as G
    assert G.MAX_BATCH + 1 == 49
    net, _ = googlenet
    u8 = np.random.default_rng(B).integers(0, 256, (B, 40, 56, 3)).astype(np.uint8)
    want = net(list(u8))                                             # host arrays, uploaded by prep
    dev = torch.from_numpy(u8).to(gpu)
    views = net.rows(dev, per_view=True)
    assert views.shape == (B, 10, 1024) and views.dtype == torch.float32 and views.device.type == "cuda"
    assert torch.equal(views.cpu(), want)
    mean = net.rows(dev)
    assert mean.shape == (B, 1024) and mean.device.type == "cuda"
    v64 = want.double().numpy()
    # s2i_time_mean adds the ten views in order in fp32 and divides once: ten roundings (the first addition, to 0, is
    # exact), so |error| <= 10 u mean|views| to first order, u = 2^-24; 11 covers the higher-order terms
    bound = 11 * 2.0 ** -24 * np.abs(v64).mean(axis=1)
    err = np.abs(mean.cpu().double().numpy() - v64.mean(axis=1))
    print("B %d: worst error / bound %.3g, %.1f%% of the features non-zero" % (
        B, float((err / np.maximum(bound, 1e-300)).max()), 100.0 * float((v64 != 0).mean())))
    assert (v64 != 0).mean() > 0.2
    assert (err <= bound).all()
    assert torch.equal(net.rows(dev), mean)                          # a rerun is bit-identical
    for bad in (dev.float(), dev[..., :2], dev[:, :, ::2], dev.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            net.rows(bad)
    with pytest.raises(_lib.S2IError):
        net.rows(torch.from_numpy(u8))                               # host pixels go through net(images)


# ---- the scorer ----------------------------------------------------------------------------------------------------------
def expected(scorer, gpu):
    """The scorer's result from tests/rank_ref.py: the rows it kept, scored by the gallery's own launches (one query
    block: these cases are far below QUERY_BLOCK) copied to the host, counted and summarised in numpy."""
    from speech_to_image_translation_without_text_amd import ops, retrieval
    g, S = scorer.gallery, scorer.sentences
    rlabel = np.repeat(scorer.labels, S)

    def side(rows, items, sents):
        assert rows.shape[0] <= retrieval.QUERY_BLOCK
        q = g._prepare(rows)
        host = np.zeros((rows.shape[0], g.rows), np.float32)
        scratch = torch.empty(rows.shape[0] * min(g.chunk_rows, g.rows), device=gpu)
        for start, n, packed in g.chunks:
            host[:, start:start + n] = ops.score_rows(q, packed, n, scratch).cpu().numpy()
        qlab = scorer.labels[items]
        gt, eq, _ = R.rank_counts(host.astype(np.float64), items * S + sents, qlab, rlabel)
        n_other = np.array([(rlabel != l).sum() for l in qlab])
        return R.metrics(gt, eq, n_other)

    out = {}
    if scorer._fake:
        res = side(torch.cat([f[0] for f in scorer._fake]), np.concatenate([f[1] for f in scorer._fake]),
                   np.concatenate([f[2] for f in scorer._fake]))
        out.update(("fake_" + k, v) for k, v in res.items())
    if scorer._real:
        rows = torch.cat([r[0] for r in scorer._real])
        items = np.concatenate([r[1] for r in scorer._real])
        res = side(rows.repeat_interleave(S, dim=0), np.repeat(items, S), np.tile(np.arange(S), items.shape[0]))
        out.update(("real_" + k, v) for k, v in res.items())
    return out


def assert_same_metrics(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-12), (k, got[k], want[k])   # float64 either side


@pytest.mark.parametrize("cosine", [False, True], ids=["dot", "cosine"])
def test_scorer_on_precomputed_rows_equals_the_reference(gpu, cosine):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    N, S, C = 6, 2, 1024
    rng = np.random.default_rng(8)
    emb = rng.standard_normal((N, S, C)).astype(np.float32)
    labels = np.array([3, 3, 9, 9, 4, 1])                           # two pairs of items share a species
    scorer = GM.ConsistencyScorer(None, emb, labels, gpu, cosine=cosine, chunk_rows=5)
    assert scorer.gallery.rows == N * S and len(scorer.gallery.chunks) == 3
    items, sents = np.repeat(np.arange(N), S), np.tile(np.arange(S), N)
    fake = (0.03 * emb[items, sents] + rng.standard_normal((N * S, C))).astype(np.float32)   # weakly aligned: ranks spread
    scorer.add_rows(fake[:5], items[:5], sents[:5])
    scorer.add_rows(torch.from_numpy(fake[5:]).to(gpu), items[5:], sents[5:])
    scorer.add_rows(emb.mean(axis=1) + 0.5 * rng.standard_normal((N, C)).astype(np.float32), np.arange(N), real=True)
    got = scorer.result()
    print(json.dumps(got))
    assert got["fake_n_queries"] == got["real_n_queries"] == N * S and got["fake_n_skipped"] == 0
    assert 0.0 < got["fake_recall@1"] < 100.0                        # not a degenerate case: some queries win, some lose
    assert_same_metrics(got, expected(scorer, gpu))
    with pytest.raises(ValueError):
        scorer.add_rows(fake[:2], [0, N], [0, 0])
    with pytest.raises(ValueError):
        scorer.add_rows(fake[:2, :100], [0, 1], [0, 0])
    with pytest.raises(ValueError):
        scorer.add_fake(torch.zeros(1, 8, 8, 4, device=gpu), [0], [0])   # no GoogLeNet given


def test_embeddings_equal_to_the_fake_rows_give_full_recall(gpu):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    N, S, C = 5, 2, 1024
    emb = np.random.default_rng(1).standard_normal((N, S, C)).astype(np.float32)
    scorer = GM.ConsistencyScorer(None, emb, np.arange(N), gpu)
    scorer.add_rows(emb.reshape(N * S, C), np.repeat(np.arange(N), S), np.tile(np.arange(S), N))
    got = scorer.result()
    assert got["fake_recall@1"] == 100.0 and got["fake_median_rank"] == 1.0 and got["fake_r_precision"] == 100.0
    assert got["fake_n_queries"] == N * S and "real_recall@1" not in got
    # all items of one species: nothing to be ranked against, every query skipped
    one = GM.ConsistencyScorer(None, emb, np.zeros(N, int), gpu)
    one.add_rows(emb.reshape(N * S, C), np.repeat(np.arange(N), S), np.tile(np.arange(S), N))
    got = one.result()
    assert got["fake_n_queries"] == 0 and got["fake_n_skipped"] == N * S


def test_score_generator_with_and_without_the_consistency_scorer(gpu, googlenet, generator, tmp_path):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM, model, ops
    net, _ = googlenet
    loader = synthetic_loader(CASE)
    incep = model.INCEPTION_V3(weights=inception_weights())
    emb = np.concatenate([b[1].numpy() for b in loader])
    labels = np.array([0, 1, 0, 2, 1])
    runs = {}
    for name in ("off", "on"):
        scorer = GM.GeneratorScorer(incep, 10, gpu)
        cons = GM.ConsistencyScorer(net, emb, labels, gpu) if name == "on" else None
        n = GM.score_generator(generator, loader, scorer, seed=4, save_images=str(tmp_path / name), consistency=cons)
        assert n == 5
        res = scorer.result(10)
        pngs = sorted((tmp_path / name).rglob("*.png"))
        runs[name] = (res, {str(p.relative_to(tmp_path / name)): p.read_bytes() for p in pngs}, cons)
    off, on = runs["off"], runs["on"]
    assert len(off[1]) == 5 * SENTENCES and off[1] == on[1]                      # the same noise, byte-identical PNGs
    for k in ("is_mean", "is_std", "nlpp_mean", "nlpp_std", "fid", "n_fake", "n_real"):
        assert off[0][k] == on[0][k], k                                           # bit-identical
    cons = on[2]
    got = cons.result()
    print(json.dumps(got))
    assert got["fake_n_queries"] == got["real_n_queries"] == 5 * SENTENCES
    assert_same_metrics(got, expected(cons, gpu))
    # the rows it kept are GoogLeNet's rows of the quantised images, in score_generator's order: batch by batch,
    # sentence-major inside a batch
    items = np.concatenate([f[1] for f in cons._fake])
    sents = np.concatenate([f[2] for f in cons._fake])
    assert items.tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 3, 4] and sents.tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 1, 1]
    real = loader[1][0][-1].to(gpu)
    u8 = ops.images_to_uint8_hwc(real.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(cons._real[1][0], net.rows(u8)) and cons._real[1][1].tolist() == [3, 4]
    for k, v in got.items():
        if "recall" in k or "precision" in k:
            assert 0.0 <= v <= 100.0, (k, v)


def test_command_line_end_to_end(gpu, googlenet, tmp_path):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    _, w = googlenet
    netG, _ = build_nets(CASE)
    root = tmp_path / "birds"
    make_cub_tree(str(root), n=6, dim=CASE['t'])
    emb = np.random.RandomState(3).randn(6, SENTENCES, CASE['t']).astype(np.float32)
    with open(root / "test" / "audio_features_image.pickle", "wb") as fp:       # two sentences per item
        pickle.dump(emb, fp)
    (tmp_path / "Model").mkdir()
    torch.save(netG.state_dict(), str(tmp_path / "Model" / "netG_5.pth"))
    torch.save(inception_weights(), str(tmp_path / "inception.pth"))
    (tmp_path / "g.caffemodel").write_bytes(GR.encode_caffemodel({n: list(v) for n, v in w.items()}))
    (tmp_path / "g.yml").write_text(
        "TREE:\n  BRANCH_NUM: 3\nTRAIN:\n  BATCH_SIZE: 3\nGAN:\n  GF_DIM: %d\n  EMBEDDING_DIM: %d\n  Z_DIM: %d\n"
        "  R_NUM: 2\n  B_CONDITION: True\nTEXT:\n  DIMENSION: %d\n" % (CASE['gf'], CASE['ef'], CASE['z'], CASE['t']))
    recs = {}
    try:
        for name, extra in (("plain", []), ("dot", ["--googlenet", str(tmp_path / "g.caffemodel")]),
                            ("cosine", ["--googlenet", str(tmp_path / "g.caffemodel"), "--consistency_cosine"])):
            out = tmp_path / name / "metrics.json"
            GM.main(["--cfg", str(tmp_path / "g.yml"), "--netG", str(tmp_path / "Model" / "netG_5.pth"), "--inception",
                     str(tmp_path / "inception.pth"), "--data_dir", str(root), "--seed", "2", "--out", str(out),
                     "--workers", "0", "--max_items", "5"] + extra)      # 10 fakes: one per IS split
            recs[name] = json.loads(out.read_text())
    finally:
        configure(CASES['small3'])
    plain = recs["plain"]
    assert not any(k.startswith(("fake_", "real_r", "real_n", "real_m")) for k in plain)      # real_stats is the FID's
    assert "consistency_score" not in plain
    for name in ("dot", "cosine"):
        rec = recs[name]
        print(name, json.dumps({k: v for k, v in rec.items() if k.startswith(("fake_", "real_")) and k != "real_stats"}))
        assert rec["consistency_score"] == name
        for side in ("fake_", "real_"):
            assert rec[side + "n_queries"] == 5 * SENTENCES and rec[side + "n_skipped"] == 0
            assert rec[side + "median_rank"] >= 1.0
            for k in ("recall@1", "recall@5", "recall@10", "r_precision"):
                assert 0.0 <= rec[side + k] <= 100.0, (side + k, rec[side + k])
        for k in ("is_mean", "is_std", "nlpp_mean", "nlpp_std", "fid", "n_fake", "n_real"):
            assert np.isfinite(plain[k]) and rec[k] == plain[k], (name, k)       # the other scores do not move
