"""The host half of the resident image pipeline (device_loader.py): PIL's bilinear resample restated on integer
tables, and a batch plan that makes the host dataset's random draws.  Everything here is an equality."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import imagepipe_ref as R
from helpers import CASES, configure

from speech_to_image_translation_without_text_amd import datasets as D
from speech_to_image_translation_without_text_amd import device_loader as DL

PLAN_SEED = 5


def _patterns(h, w):
    rng = np.random.RandomState(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    stripes = (((xx // 3 + yy // 2) & 1) * 255).astype(np.uint8)
    return {"random": rng.randint(0, 256, (h, w, 3), dtype=np.uint8),
            "checker": np.repeat(checker[:, :, None], 3, 2),
            "stripes": np.stack([stripes, 255 - stripes, checker], 2)}


# (in_w, in_h) -> (out_w, out_h): the pyramid's own ratios, then non-square sizes at non-integer ratios, down and up
RESIZES = [((256, 256), (128, 128)), ((256, 256), (64, 64)), ((64, 64), (32, 32)), ((64, 64), (16, 16)),
           ((333, 500), (304, 456)), ((500, 375), (405, 304)), ((211, 157), (100, 74)), ((72, 74), (304, 312)),
           ((97, 61), (13, 40))]


@pytest.mark.parametrize("src,dst", RESIZES)
def test_restated_resample_equals_pil(src, dst):
    for name, img in _patterns(src[1], src[0]).items():
        ref = np.asarray(Image.fromarray(img).resize(dst, Image.BILINEAR))
        got = R.resize_bilinear(img, dst[0], dst[1])
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, src, dst, int((got != ref).sum()))


def test_coefficients_of_the_pyramid_scales():
    one = 1 << DL.PRECISION_BITS
    starts, taps = DL.pil_bilinear_coeffs(256, 128)
    assert taps.shape == (128, 4) and taps.dtype == np.int32 and starts.dtype == np.int32
    assert taps[5].tolist() == [one // 8, 3 * one // 8, 3 * one // 8, one // 8] and starts[5] == 9
    assert starts[0] == 0 and taps[0, 3] == 0 and taps[0, :3].sum() in (one - 1, one, one + 1)   # edge: renormalised
    starts, taps = DL.pil_bilinear_coeffs(256, 64)
    assert taps.shape == (64, 8) and starts[3] == 10 and taps[3].tolist() == [one * k // 32 for k in (1, 3, 5, 7, 7, 5, 3, 1)]
    beyond = starts[:, None] + np.arange(8)[None, :] >= 256
    assert beyond.any() and not taps[beyond].any()          # a window cut by the image's edge is padded with zero taps
    tab = DL.coeff_table(64, 16, 8)
    assert tab.shape == (16, 9) and np.array_equal(tab[:, 0], DL.pil_bilinear_coeffs(64, 16)[0])
    with pytest.raises(ValueError):
        DL.coeff_table(64, 8, 8)                             # scale 8 needs 16 taps


def _host_apply(ds, item, top, left, flip):
    """The plan's choices for one image, carried out with PIL alone."""
    rel = ds._get_img(ds.json_data[item])
    img = Image.open(os.path.join(ds.image_folder, rel)).convert('RGB')
    bbox = ds._get_bbox(rel)
    if bbox is not None:
        img = img.crop(D.crop_box(bbox, *img.size))
    S = ds.imsize[-1]
    img = D.Resize(int(S * 76 / 64))(img)
    img = img.crop((left, top, left + S, top + S))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return [D.to_normalized_tensor(D.Resize(s)(img) if s != S else img) for s in ds.imsize]


@pytest.mark.parametrize("size", [256, 64])
@pytest.mark.parametrize("birds", [True, False])
def test_plan_makes_the_host_datasets_draws(tmp_path, birds, size):
    configure(CASES['full3_fwd'])
    R.make_tree(str(tmp_path), birds=birds)
    ds = R.make_dataset(str(tmp_path), birds, size)
    emb = D.load_embedding_pickle(str(tmp_path / "train" / "audio_features_image.pickle"))
    n = len(ds)
    random.seed(PLAN_SEED)
    host = [ds[i] for i in range(n)]
    after_host = random.random()
    random.seed(PLAN_SEED)
    plan, captions, paths, labels = DL.plan_batch(ds, list(range(n)))
    assert random.random() == after_host                     # the same number of draws was consumed
    assert plan.shape == (2 * n, 4) and plan.dtype == np.int32
    assert plan[:n, 0].tolist() == list(range(n))
    for i in range(n):
        real, wrong, e, path, label = host[i]
        assert path == paths[i] and label == labels[i]
        assert np.array_equal(e, emb[i][captions[i]])
        assert labels[int(plan[n + i, 0])] != label          # the wrong image is of another class
        for got, row in ((real, plan[i]), (wrong, plan[n + i])):
            ref = _host_apply(ds, *[int(v) for v in row])
            assert len(got) == len(ref) == 3
            for a, b in zip(got, ref):
                assert a.shape == b.shape and torch.equal(a, b), (i, row.tolist())
    # the seed is chosen so that the plan exercises both flip values, and the tree so that windows really move
    assert set(plan[:, 3].tolist()) == {0, 1}
    hw = DL.host_index(ds).hw
    assert (hw[:, 0] != hw[:, 1]).any() and int(hw.min()) == int(size * 76 / 64)
    assert plan[:, 1].max() > 0 and plan[:, 2].max() > 0


def test_plan_skips_the_crop_draws_for_an_image_of_the_crop_size(tmp_path):
    """RandomCrop draws nothing when the image is t x t already; the flip draw still happens."""
    configure(CASES['full3_fwd'])
    R.make_tree(str(tmp_path), birds=False)
    ds = R.make_dataset(str(tmp_path), False, 64)
    idx = DL.host_index(ds)
    idx.hw[:] = 64                                             # pretend every resident image is the crop size

    class Counting:                                            # a recorder in front of a private generator
        def __init__(self, seed):
            self.inner, self.calls = random.Random(seed), []

        def randint(self, a, b):
            self.calls.append(("randint", a, b))
            return self.inner.randint(a, b)

        def random(self):
            self.calls.append(("random",))
            return self.inner.random()

    rng = Counting(1)
    plan, _, _, _ = DL.plan_batch(ds, [0], rng)
    kinds = [c for c in rng.calls if c[0] == "random" or c[2] != 11]   # drop the rejection loop's randint(0, 11)
    assert kinds == [("randint", 0, 9), ("random",), ("random",)]
    assert plan[:, 1:3].tolist() == [[0, 0], [0, 0]]


def test_constructor_refusals(tmp_path):
    configure(CASES['full3_fwd'])
    R.make_tree(str(tmp_path), birds=True)
    root = str(tmp_path)
    with pytest.raises(ValueError, match="train"):
        DL.ResidentTrainSet(R.make_dataset(root, True, 256, train=False), "cpu")
    odd = [D.Compose([D.Resize(304), D.RandomCrop(256)]),
           D.Compose([D.Resize(300), D.RandomCrop(256), D.RandomHorizontalFlip()]),
           D.Compose([D.Resize(304), D.RandomCrop(256), D.RandomHorizontalFlip(0.3)]),
           D.Compose([D.RandomCrop(256), D.Resize(304), D.RandomHorizontalFlip()]),
           None]
    for tr in odd:
        with pytest.raises(ValueError, match="transform"):
            DL.ResidentTrainSet(D.BirdsDataset(root, train=True, base_size=64, transform=tr), "cpu")
    with pytest.raises(ValueError, match="branch sizes"):
        DL.ResidentTrainSet(D.BirdsDataset(root, train=True, base_size=32, transform=D.default_image_transform(256)),
                            "cpu")
    assert DL._threads(64) == 16 and DL._threads(3) == 3 and DL._threads(0) == 1


@pytest.mark.parametrize("birds", [True, False])
def test_resident_pool_holds_the_resized_images(tmp_path, birds):
    """The pool (here in host memory: no kernel runs) holds, back to back, what get_imgs has before its first draw."""
    configure(CASES['full3_fwd'])
    R.make_tree(str(tmp_path), birds=birds)
    ds = R.make_dataset(str(tmp_path), birds, 64)
    rs = DL.ResidentTrainSet(ds, "cpu", workers=4)
    assert len(rs) == 12 and rs.size == 64 and rs.levels == 3
    assert rs.offsets.dtype == torch.int64 and rs.sizes.dtype == torch.int32 and rs.pool.dtype == torch.uint8
    total = 0
    for i in range(len(rs)):
        rel = ds._get_img(ds.json_data[i])
        img = Image.open(os.path.join(ds.image_folder, rel)).convert('RGB')
        if birds:
            img = img.crop(D.crop_box(ds.bbox[rel[:-4]], *img.size))
        ref = np.asarray(D.Resize(76)(img))
        assert int(rs.offsets[i]) == total and rs.sizes[i].tolist() == list(ref.shape[:2])
        assert np.array_equal(rs.image(i).numpy(), ref)
        total += ref.size
    assert rs.pool_bytes == total == rs.pool.numel()
    from speech_to_image_translation_without_text_amd import _lib
    with pytest.raises(_lib.S2IError):                        # no fallback: a pool in host memory cannot serve batches
        rs.batch([0, 1])


def test_loader_order_and_sharding_without_a_device(tmp_path):
    configure(CASES['full3_fwd'])
    R.make_tree(str(tmp_path), birds=False)
    rs = DL.ResidentTrainSet(R.make_dataset(str(tmp_path), False, 64), "cpu")
    assert rs.loader(5, shuffle=False).indices() == list(range(12)) and len(rs.loader(5, shuffle=False)) == 3
    ld = rs.loader(4, shuffle=True, seed=3)
    e0 = ld.indices()
    ld.set_epoch(1)
    assert sorted(e0) == list(range(12)) and ld.indices() != e0 and sorted(ld.indices()) == list(range(12))
    with pytest.raises(ValueError):
        rs.loader(4, rank=0)


def test_entry_point_reports_bad_arguments():
    """s2i_image_batch checks its arguments on the host before any launch: the usual error path, no GPU needed."""
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    p = 4096    # never dereferenced: every call below is refused before the launch

    def call(n=2, S=256, L=3, tab1=p, tab2=p, out1=p, out2=p, out0=p):
        return lib.s2i_image_batch(p, 1 << 20, p, p, 4, p, n, S, L, tab1, tab2, out0, out1, out2, None)
    assert call(S=250) != 0 and b"multiple of 4" in lib.s2i_last_error()
    assert call(S=512) != 0 and b"multiple of 4" in lib.s2i_last_error()
    assert call(L=4) != 0 and b"levels" in lib.s2i_last_error()
    assert call(L=0) != 0 and b"levels" in lib.s2i_last_error()
    assert call(n=0) != 0 and call(n=70000) != 0
    assert call(tab2=None) != 0 and b"level 2" in lib.s2i_last_error()
    assert call(L=2, out1=None) != 0 and b"level 1" in lib.s2i_last_error()
    assert call(out0=p + 4) != 0 and b"aligned" in lib.s2i_last_error()
