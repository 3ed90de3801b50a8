"""GPU suite of the GoogLeNet feature extractor: the ten-view input kernel, the fused LRN + max-pool kernels and the 3x3
max pools against float64 torch, the whole network with seeded weights against the float64 restatement in
googlenet_ref.py, chunking, and the extraction CLI end to end through the retrieval score."""
import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import googlenet_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5


def ragged_images():
    """A non-square image, one smaller than 227 on one side, a grayscale and an RGBA one, through PIL's convert("RGB")."""
    from PIL import Image
    rng = np.random.default_rng(7)
    yy, xx = np.meshgrid(np.arange(300), np.arange(451), indexing="ij")
    smooth = np.stack([(yy * 0.8) % 256, (xx * 0.5) % 256, (yy + xx) % 256], 2).astype(np.uint8)
    small = rng.integers(0, 256, (150, 260, 3)).astype(np.uint8)
    gray = Image.fromarray(rng.integers(0, 256, (240, 233)).astype(np.uint8), "L").convert("RGB")
    rgba = Image.fromarray(rng.integers(0, 256, (229, 400, 4)).astype(np.uint8), "RGBA").convert("RGB")
    return [smooth, small, np.asarray(gray), np.asarray(rgba)]




def test_prep_kernel_against_float64(gpu):
    from speech_to_image_translation_without_text_amd import googlenet as G
    net = G.GoogLeNetFeatures.__new__(G.GoogLeNetFeatures)
    net.device, net.mean_bgr = gpu, G.MEAN_BGR
    imgs = ragged_images()
    y = torch.full((10 * len(imgs), 224, 224, 4), SENTINEL, device=gpu)
    keep = net.prep(imgs, y)
    torch.cuda.synchronize()
    del keep
    got = y.cpu().double()
    assert torch.all(got[..., 3] == 0)
    worst = 0.0
    for i, im in enumerate(imgs):
        ref = torch.from_numpy(R.views(im)).permute(0, 2, 3, 1)
        err = float((got[10 * i:10 * i + 10, ..., :3] - ref).abs().max())
        worst = max(worst, err)
    print("prep worst abs error %.3g" % worst)
    assert worst <= R.PREP_BOUND


def launch_pool(gpu, kind, x, C, coff=0, extra=0, stride=2, pad=0):
    from speech_to_image_translation_without_text_amd import _lib
    B, H, W, ldx = x.shape
    Ho = (H + 2 * pad - 3 + stride - 1) // stride + 1
    Wo = (W + 2 * pad - 3 + stride - 1) // stride + 1
    if pad and (Ho - 1) * stride >= H + pad:
        Ho -= 1
    if pad and (Wo - 1) * stride >= W + pad:
        Wo -= 1
    ldy = coff + C + extra
    y = torch.full((B, Ho, Wo, ldy), SENTINEL, device=gpu)
    lib = _lib.load()
    xd = x.to(gpu)
    if kind == "pool":
        rc = lib.s2i_maxpool3(_lib.ptr(xd), B, H, W, C, ldx, stride, pad, _lib.ptr(y), ldy, coff, _lib.stream())
    else:
        order = _lib.POOL_THEN_LRN if kind == "pool_lrn" else _lib.LRN_THEN_POOL
        rc = lib.s2i_lrn_maxpool3(order, _lib.ptr(xd), B, H, W, C, ldx, _lib.ptr(y), ldy, coff, 5, 1e-4, 0.75, 1.0,
                                  _lib.stream())
    _lib.check(rc, kind)
    got = y.cpu()
    assert torch.all(got[..., :coff] == SENTINEL) and torch.all(got[..., coff + C:] == SENTINEL)
    return got[..., coff:coff + C].double()


def ref_pool(kind, x, C, stride=2, pad=0):
    t = x[..., :C].permute(0, 3, 1, 2).double()
    if kind == "pool":
        r = F.max_pool2d(t, 3, stride, pad, ceil_mode=True)
    elif kind == "pool_lrn":
        r = R.lrn(R.pool_s2(t))
    else:
        r = R.pool_s2(R.lrn(t))
    return r.permute(0, 2, 3, 1)


# (kind, B, H, W, C, ldx extra, coff, y extra): GoogLeNet's two stem pairs and pools, then odd maps, sliced channels and
# the scalar path (C % 4 != 0)
POOL_CASES = [
    ("pool_lrn", 2, 112, 112, 64, 0, 0, 0),
    ("lrn_pool", 2, 56, 56, 192, 0, 0, 0),
    ("pool_lrn", 3, 13, 9, 12, 4, 4, 8),
    ("lrn_pool", 3, 9, 14, 20, 0, 8, 4),
    ("pool_lrn", 2, 7, 11, 7, 1, 1, 2),
    ("lrn_pool", 2, 10, 5, 3, 0, 2, 1),
    ("pool", 2, 28, 28, 480, 0, 0, 0),
    ("pool", 2, 14, 14, 832, 0, 0, 0),
    ("pool", 2, 15, 8, 12, 4, 4, 4),
    ("pool", 2, 6, 9, 5, 2, 3, 1),
]


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "%s-%dx%dx%d-c%d" % (c[0], c[2], c[3], c[4], c[6]))
def test_lrn_pool_kernels_against_float64(gpu, case):
    kind, B, H, W, C, xe, coff, ye = case
    g = torch.Generator().manual_seed(H * 131 + C)
    x = torch.relu(torch.randn(B, H, W, C + xe, generator=g) * 40.0)   # post-ReLU magnitudes where the LRN matters
    got = launch_pool(gpu, kind, x, C, coff, ye)
    ref = ref_pool(kind, x, C)
    assert got.shape == ref.shape
    err = float(((got - ref).abs() / (1.0 + ref.abs())).max())
    assert err < 2e-6, err


@pytest.mark.parametrize("shape", [(2, 28, 28, 192), (2, 14, 14, 528), (2, 7, 7, 832), (2, 9, 6, 12), (2, 5, 8, 7)])
def test_stride1_pool_against_float64(gpu, shape):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, H, W, C, generator=g)
    got = launch_pool(gpu, "pool", x, C, 4 if C % 4 == 0 else 1, 4, stride=1, pad=1)
    ref = ref_pool("pool", x, C, 1, 1)
    assert got.shape == ref.shape and torch.equal(got, ref)


def test_pool_rejects_bad_arguments(gpu):
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    x = torch.zeros(1, 8, 8, 8, device=gpu)
    assert lib.s2i_maxpool3(_lib.ptr(x), 1, 8, 8, 8, 8, 3, 0, _lib.ptr(x), 8, 0, _lib.stream()) == 1
    assert b"stride" in lib.s2i_last_error()
    assert lib.s2i_lrn_maxpool3(0, _lib.ptr(x), 1, 8, 8, 8, 8, _lib.ptr(x), 8, 0, 4, 1e-4, 0.75, 1.0,
                                _lib.stream()) == 1
    assert b"local_size" in lib.s2i_last_error()
    assert lib.s2i_lrn_maxpool3(7, _lib.ptr(x), 1, 8, 8, 8, 8, _lib.ptr(x), 8, 0, 5, 1e-4, 0.75, 1.0,
                                _lib.stream()) == 1


# max |GPU - float64| / max |feature| over 30 views measured on an MI355X: 5.74e-7; the bound is 2x that
NET_BOUND = 1.2e-6


@pytest.fixture(scope="module")
def net_and_weights(gpu):
    from speech_to_image_translation_without_text_amd import googlenet as G
    w = R.random_weights(0)
    return G.GoogLeNetFeatures(w, gpu), w


def test_network_against_float64(net_and_weights):
    net, w = net_and_weights
    imgs = ragged_images()[:3]
    got = net(imgs).double()
    assert got.shape == (3, 10, 1024)
    with torch.no_grad():
        ref = R.forward(w, np.concatenate([R.views(im) for im in imgs])).reshape(3, 10, 1024)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    print("network max error / max |feature| = %.3g (max |feature| %.3g)" % (err, scale))
    assert scale > 0 and float((ref > 0).double().mean()) > 0.2
    assert err < NET_BOUND


def test_chunking_does_not_change_results(net_and_weights):
    net, _ = net_and_weights
    imgs = ragged_images()
    one = net(imgs)
    assert torch.equal(net(imgs, batch_size=1), one)
    assert torch.equal(net(imgs, batch_size=3), one)
    with pytest.raises(ValueError):
        net(imgs, batch_size=49)


def test_cli_end_to_end(gpu, tmp_path, net_and_weights):
    from PIL import Image
    from speech_to_image_translation_without_text_amd import (datasets, extract_image_feature as X, googlenet as G,
                                                              retrieval)
    net, w = net_and_weights
    paths = R.make_data_dir(tmp_path, "birds", n=(5, 4))
    rng = np.random.default_rng(3)
    for split, ps in paths.items():
        for i, p in enumerate(ps):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            a = rng.integers(0, 256, (180 + 17 * i, 240 - 9 * i, 3)).astype(np.uint8)
            Image.fromarray(a).save(p, quality=90) if p.endswith(".jpg") else Image.fromarray(a).save(p)
    model = tmp_path / "g.caffemodel"
    model.write_bytes(R.encode_caffemodel({n: list(v) for n, v in w.items()}))
    X.main(["--weights", str(model), "--dataset", "birds", "--data_dir", str(tmp_path), "--batch_size", "2"])
    for split, ps in paths.items():
        out = tmp_path / split / "image_features_googlenet_caffe.pickle"
        feats = datasets.load_embedding_pickle(str(out))
        assert feats.shape == (len(ps), 10, 1024) and feats.dtype == np.float32
        want = net([G.read_image(p) for p in ps])
        assert np.array_equal(feats, want.numpy())
    # retrieval on the image pickle and an extract_audio_feature-format audio pickle
    n = len(paths["test"])
    audio = rng.standard_normal((n, 10, 1024)).astype(np.float32)
    apath = tmp_path / "test" / "audio_features_0.pickle"
    datasets.save_embedding_pickle(audio, str(apath))
    ipath = tmp_path / "test" / "image_features_googlenet_caffe.pickle"
    accu, ap = retrieval.main(["--audio", str(apath), "--image", str(ipath), "--data_dir", str(tmp_path), "--split",
                               "test", "--seed", "4"])
    line = json.loads((tmp_path / "test" / "retrieval_test.json").read_text())
    assert line["accu"] == accu and line["ap50"] == ap and line["items"] == n
    labels = retrieval.labels_from_json(str(tmp_path / "test.json"))
    with open(ipath, "rb") as f:
        image = pickle.load(f)
    assert (accu, ap) == retrieval.eval_features(audio, image, labels, 4)
    assert 0.0 <= accu <= 100.0 and 0.0 <= ap <= 100.0
