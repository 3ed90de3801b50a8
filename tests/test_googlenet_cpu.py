"""CPU suite of the GoogLeNet feature extractor: the caffemodel reader against a test-local protobuf encoder (V2 `layer`
and V1 `layers`, packed and unpacked data, `shape` and legacy dims), error reports, the architecture table, the ten-view
table through the float64 restatement, and the CLI's split / path logic and pickle format."""
import os
import pickle

import numpy as np
import pytest

from googlenet_ref import (CROPS, _len_field, encode_blob, encode_caffemodel, make_data_dir, preprocess, random_weights,
                           views)


def small_layers(seed=0, shapes=None):
    rng = np.random.default_rng(seed)
    shapes = shapes or {"conv1/7x7_s2": ((4, 3, 7, 7), (4,)), "inception_3a/1x1": ((2, 5, 1, 1), (2,))}
    return {n: [rng.standard_normal(ws).astype(np.float32), rng.standard_normal(bs).astype(np.float32)]
            for n, (ws, bs) in shapes.items()}


@pytest.mark.parametrize("v1", [False, True])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("legacy", [False, True])
def test_caffemodel_round_trip(v1, packed, legacy):
    from speech_to_image_translation_without_text_amd import googlenet as G
    layers = small_layers()
    got = G.parse_caffemodel(encode_caffemodel(layers, v1, packed, legacy))
    assert list(got) == list(layers)            # blob-less layers and heads skipped, order kept
    for n, blobs in layers.items():
        assert len(got[n]) == 2
        w, b = got[n]
        assert w.dtype == np.float32 and np.array_equal(w, blobs[0])
        if legacy:
            assert b.shape == (1, 1, 1) + blobs[1].shape
        assert np.array_equal(b.reshape(-1), blobs[1])


def test_caffemodel_full_network_from_file(tmp_path):
    from speech_to_image_translation_without_text_amd import googlenet as G
    w = random_weights(3)
    path = tmp_path / "g.caffemodel"
    path.write_bytes(encode_caffemodel({n: list(v) for n, v in w.items()}, v1=True, legacy=True))
    got = G.check_weights(G.load_caffemodel(str(path)))
    assert list(got) == list(G.architecture())
    for n, (wt, bt) in w.items():
        assert np.array_equal(got[n][0], wt) and np.array_equal(got[n][1], bt)


def test_caffemodel_truncated_and_corrupt():
    from speech_to_image_translation_without_text_amd import googlenet as G
    data = encode_caffemodel(small_layers())
    for cut in (len(data) - 1, len(data) // 2, 7):
        with pytest.raises(G.CaffemodelError, match="truncated"):
            G.parse_caffemodel(data[:cut])
    with pytest.raises(G.CaffemodelError, match="wire type"):
        G.parse_caffemodel(bytes([0x0F]) + data)          # field 1, wire type 7
    bad = {"conv1/7x7_s2": [np.zeros((4, 3, 7, 7), np.float32)]}
    blob = bytearray(encode_blob(bad["conv1/7x7_s2"][0]))
    blob[2 + 1 + 1] = 5                                   # first dim 4 -> 5: the shape no longer matches the data
    msg = _len_field(1, b"conv1/7x7_s2") + _len_field(7, bytes(blob))
    with pytest.raises(G.CaffemodelError, match="holds"):
        G.parse_caffemodel(_len_field(100, msg))


def test_check_weights_names_missing_and_wrong_layers():
    from speech_to_image_translation_without_text_amd import googlenet as G
    w = random_weights(0)
    del w["inception_4c/5x5"]
    del w["conv2/3x3"]
    w["inception_5b/pool_proj"] = (np.zeros((128, 833, 1, 1), np.float32), np.zeros(128, np.float32))
    w["inception_3a/1x1"] = (w["inception_3a/1x1"][0], np.zeros(63, np.float32))
    w["fc8"] = (np.zeros((2, 2, 1, 1), np.float32), np.zeros(2, np.float32))
    w["loss1/conv"] = (np.zeros((2, 2, 1, 1), np.float32), np.zeros(2, np.float32))   # heads are ignored
    with pytest.raises(ValueError) as e:
        G.check_weights(w)
    msg = str(e.value)
    for part in ("inception_4c/5x5", "conv2/3x3", "inception_5b/pool_proj weight: (128, 833, 1, 1)",
                 "inception_3a/1x1 bias: (63,)", "unexpected layers: fc8"):
        assert part in msg, msg
    assert "loss1/conv" not in msg
    # in-memory dicts of (w, b) tuples, legacy (1, 1, 1, O) biases and torch tensors are accepted
    import torch
    w = random_weights(0)
    w["conv1/7x7_s2"] = (torch.from_numpy(w["conv1/7x7_s2"][0]), w["conv1/7x7_s2"][1].reshape(1, 1, 1, -1))
    got = G.check_weights(w)
    assert got["conv1/7x7_s2"][1].shape == (64,)


def test_architecture_table():
    from speech_to_image_translation_without_text_amd import googlenet as G
    assert [G.block_width(b) for b in G.BLOCKS] == [256, 480, 512, 512, 512, 528, 832, 832, 1024]
    assert G.map_sizes() == [112, 56, 28, 14, 7, 1]
    arch = G.architecture()
    assert len(arch) == 3 + 6 * 9
    # the channel chain: every block reads the previous block's width
    cin = 192
    for b in G.BLOCKS:
        for br in ("1x1", "3x3_reduce", "5x5_reduce", "pool_proj"):
            assert arch[b[0] + "/" + br][0] == cin
        cin = G.block_width(b)
    # parameters from the table, written out independently
    n = 64 * 3 * 49 + 64 + 64 * 64 + 64 + 192 * 64 * 9 + 192
    cin = 192
    for _, n1, r3, n3, r5, n5, npp in G.BLOCKS:
        n += (cin * n1 + n1) + (cin * r3 + r3) + (r3 * 9 * n3 + n3) + (cin * r5 + r5) + (r5 * 25 * n5 + n5)
        n += cin * npp + npp
        cin = n1 + n3 + n5 + npp
    assert G.parameter_count() == n == 5973552
    assert abs(G.flops_per_view() / 2 - 1.58e9) < 0.01e9
    # the largest tensor of a chunk fits s2i_conv2d_forward's 32-bit offsets
    assert G.MAX_BATCH * 10 * 112 * 112 * 64 * 4 < G.CONV2D_BYTE_LIMIT
    assert (G.MAX_BATCH + 19) * 10 * 112 * 112 * 64 * 4 > G.CONV2D_BYTE_LIMIT


def test_view_table_on_an_asymmetric_image():
    """Crop origins and order, and the up-down (not left-right) flip, on a 227 x 227 image whose pixel encodes (y, x)."""
    yy, xx = np.meshgrid(np.arange(227), np.arange(227), indexing="ij")
    img = np.stack([yy, xx, (yy * 7 + xx) % 256], axis=2).astype(np.uint8)
    v = views(img, mean_bgr=(0.0, 0.0, 0.0))        # (10, 3, 224, 224), BGR: channel 2 is R = y, 1 is G = x
    assert v.shape == (10, 3, 224, 224)
    for k, (x0, y0) in enumerate(CROPS):
        assert v[k, 2, 0, 0] == y0 and v[k, 1, 0, 0] == x0
        assert v[k, 2, 223, 223] == y0 + 223 and v[k, 1, 223, 223] == x0 + 223
        # flipped: view 5 + k at (oy, ox) is the resized pixel (226 - (y0 + oy), x0 + ox)
        assert v[5 + k, 2, 0, 0] == 226 - y0 and v[5 + k, 1, 0, 0] == x0
        assert v[5 + k, 2, 223, 5] == 226 - (y0 + 223) and v[5 + k, 1, 223, 5] == x0 + 5
        assert v[5 + k, 0, 10, 20] == ((226 - (y0 + 10)) * 7 + x0 + 20) % 256
    # mean subtraction in BGR order
    m = views(np.zeros((227, 227, 3), np.uint8))
    assert np.allclose(m[0, :, 5, 5], [-104.00698793, -116.66876762, -122.67891434])


def test_resize_restatement():
    """Half-pixel bilinear: a 2x downscale averages 2 x 2 blocks; upscaling clamps to the edge; a constant stays one."""
    from googlenet_ref import resize_bilinear
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (454, 454, 3)).astype(np.float64)
    r = resize_bilinear(a)
    blocks = a.reshape(227, 2, 227, 2, 3).mean(axis=(1, 3))
    assert np.allclose(r, blocks)
    small = rng.integers(0, 256, (5, 7, 3))
    r = resize_bilinear(small)
    assert np.array_equal(r[0, 0], small[0, 0]) and np.array_equal(r[-1, -1], small[-1, -1])
    assert np.allclose(resize_bilinear(np.full((31, 400, 3), 9)), 9)
    assert preprocess(np.zeros((3, 3, 3), np.uint8)).shape == (3, 227, 227)


def test_as_rgb_matches_pil_convert():
    from PIL import Image
    from speech_to_image_translation_without_text_amd import googlenet as G
    rng = np.random.default_rng(1)
    gray = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    rgba = rng.integers(0, 256, (9, 11, 4)).astype(np.uint8)
    assert np.array_equal(G.as_rgb(gray), np.asarray(Image.fromarray(gray, "L").convert("RGB")))
    assert np.array_equal(G.as_rgb(rgba), np.asarray(Image.fromarray(rgba, "RGBA").convert("RGB")))
    with pytest.raises(ValueError):
        G.as_rgb(np.zeros((4, 4, 3), np.float32))


def test_mean_file(tmp_path):
    from speech_to_image_translation_without_text_amd import googlenet as G
    m = np.stack([np.full((256, 256), v) for v in (100.0, 110.0, 120.0)])
    m[0, 0, 0] += 256 * 256
    np.save(tmp_path / "m.npy", m)
    assert np.allclose(G.mean_from_file(str(tmp_path / "m.npy")), (101.0, 110.0, 120.0))
    np.save(tmp_path / "bad.npy", m[:, 0])
    with pytest.raises(ValueError):
        G.mean_from_file(str(tmp_path / "bad.npy"))


def test_cli_split_paths(tmp_path):
    from speech_to_image_translation_without_text_amd import extract_image_feature as X
    want = make_data_dir(tmp_path, "birds", feature_path="custom/train_feats.pickle")
    paths, out = X.split_items(str(tmp_path), "train", "birds")
    assert paths == want["train"] and "/images/" in paths[0]
    assert out == str(tmp_path / "custom/train_feats.pickle")
    paths, out = X.split_items(str(tmp_path), "test", "birds")
    assert paths == want["test"]
    assert out == os.path.join(str(tmp_path), "test", "image_features_googlenet_caffe.pickle")
    fl = tmp_path / "flowers"
    fl.mkdir()
    want = make_data_dir(fl, "flowers")
    paths, out = X.split_items(str(fl), "test", "flowers")
    assert paths == want["test"] and "/images/" not in paths[0]
    assert out == os.path.join(str(fl), "test_image_feature_caffe.pickle")
    with pytest.raises(ValueError):
        X.split_items(str(fl), "test", "places")


def test_feature_pickle_format(tmp_path):
    from speech_to_image_translation_without_text_amd import datasets, extract_image_feature as X
    feats = np.random.default_rng(0).standard_normal((4, 10, 1024)).astype(np.float32)
    p = str(tmp_path / "sub" / "f.pickle")
    X.write_feature_pickle(feats, p)
    with open(p, "rb") as f:
        raw = pickle.load(f)
    assert isinstance(raw, list) and len(raw) == 4 and raw[0].shape == (10, 1024) and raw[0].dtype == np.float32
    back = datasets.load_embedding_pickle(p)
    assert back.shape == (4, 10, 1024) and np.array_equal(back, feats)
