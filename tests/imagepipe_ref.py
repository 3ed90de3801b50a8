"""Integer reference of the resident image pipeline (speech_to_image_translation_without_text_amd/device_loader.py,
csrc/s2i_imagepipe.hip): PIL's two-pass 8-bit bilinear resample restated in numpy on `pil_bilinear_coeffs`, the window /
mirror step, and the small dataset trees the image-pipeline tests share.  No floating point before the final
normalisation, so the GPU test compares with equality."""
import json
import os
import pickle

import numpy as np
import torch
from PIL import Image

from speech_to_image_translation_without_text_amd import datasets as D
from speech_to_image_translation_without_text_amd.device_loader import PRECISION_BITS, pil_bilinear_coeffs


def resample_axis(a, out_size, axis):
    """One pass of PIL's 8-bit resample along `axis` of a uint8 array: uint8 out.  Each tap sum starts at 1 << 21, adds
    pixel * coefficient, is shifted right by 22 and clamped to 0..255."""
    a = np.moveaxis(np.asarray(a, dtype=np.uint8), axis, 0).astype(np.int64)
    starts, taps = pil_bilinear_coeffs(a.shape[0], out_size)
    acc = np.full((out_size,) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for k in range(taps.shape[1]):
        src = np.minimum(starts.astype(np.int64) + k, a.shape[0] - 1)     # a tap past the window has coefficient 0
        acc += a[src] * taps[:, k].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(img, out_w, out_h):
    """`Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR)` for a uint8 (H, W, C) array: the horizontal pass
    writes a uint8 intermediate, then the vertical pass; a pass whose size does not change is not run."""
    img = np.asarray(img, dtype=np.uint8)
    if img.shape[1] != out_w:
        img = resample_axis(img, out_w, 1)
    if img.shape[0] != out_h:
        img = resample_axis(img, out_h, 0)
    return img


def window(img, top, left, size, flip):
    """RandomCrop's window of a uint8 (H, W, 3) image, then RandomHorizontalFlip's mirror."""
    win = np.asarray(img)[top:top + size, left:left + size]
    assert win.shape[:2] == (size, size)
    return np.ascontiguousarray(win[:, ::-1] if flip else win)


def normalize(u8_hwc):
    """The host normalisation: ToTensor + Normalize(0.5, 0.5) -> float32 CHW tensor."""
    return D.to_normalized_tensor(Image.fromarray(np.ascontiguousarray(u8_hwc)))


def pyramid(img, top, left, flip, size, levels):
    """What the kernel owes for one plan row: `levels` float CHW tensors, largest first; every smaller level is a
    resize of the window itself (not of the previous level)."""
    win = window(img, top, left, size, flip)
    return [normalize(win if i == 0 else resize_bilinear(win, size >> i, size >> i)) for i in range(levels)]


def make_tree(root, n=12, birds=True, dim=32):
    """The synthetic tree of tests/test_datasets.py: n PNGs of differing, non-square sizes in three classes, the json
    splits, the (n, 10, dim) embedding pickles and, for birds, the CUB bounding-box files."""
    rng = np.random.RandomState(0)
    img_root = os.path.join(root, "images")
    items, boxes, names = [], [], []
    for i in range(n):
        cls = "%03d.Bird_%d" % (i % 3 + 1, i % 3) if birds else str(i % 3)
        rel = "%s/img_%d.png" % (cls, i)
        os.makedirs(os.path.join(img_root, os.path.dirname(rel)), exist_ok=True)
        w, h = 90 + 7 * i, 120 - 3 * i
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(img_root, rel))
        key = "image" if birds else "img"
        items.append({key: rel, "class": cls, "audio": ["a_%d_%d.wav" % (i, k) for k in range(10)], "text": ["t"] * 10})
        boxes.append((i + 1, 10.0 + i, 20.0, 50.0 + i, 40.0))
        names.append((i + 1, rel))
    for split in ("train", "test"):
        with open(os.path.join(root, split + ".json"), "w") as fp:
            json.dump({"image_base_path": img_root, "audio_base_path": os.path.join(root, "audio"), "data": items}, fp)
        emb = rng.randn(n, 10, dim).astype(np.float32)
        os.makedirs(os.path.join(root, split), exist_ok=True)
        with open(os.path.join(root, split, "audio_features_image.pickle"), "wb") as fp:
            pickle.dump(emb, fp)
    os.makedirs(os.path.join(root, "CUB_200_2011"), exist_ok=True)
    with open(os.path.join(root, "CUB_200_2011", "bounding_boxes.txt"), "w") as fp:
        for b in boxes:
            fp.write("%d %.1f %.1f %.1f %.1f\n" % b)
    with open(os.path.join(root, "CUB_200_2011", "images.txt"), "w") as fp:
        for nm in names:
            fp.write("%d %s\n" % nm)


def make_dataset(root, birds, size, train=True, **kw):
    """A dataset over `make_tree(root)` with the standard transform at crop size `size` and three branches."""
    cls = D.BirdsDataset if birds else D.FlowersDataset
    return cls(root, train=train, base_size=size // 4, transform=D.default_image_transform(size), **kw)


def assert_batches_equal(a, b, what=""):
    """Two train tuples (real_imgs, wrong_imgs, embedding, paths, labels): every element equal."""
    for k in (0, 1):
        assert len(a[k]) == len(b[k])
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            x, y = x.cpu(), y.cpu()
            assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape, (what, k, i, x.shape, y.shape)
            assert torch.equal(x, y), "%s: %s branch %d differs in %d elements" % (
                what, ("real", "wrong")[k], i, int((x != y).sum()))
    assert a[2].dtype == b[2].dtype and torch.equal(a[2].cpu(), b[2].cpu()), what + ": embedding"
    assert list(a[3]) == list(b[3]), what + ": paths"
    assert a[4].dtype == b[4].dtype and torch.equal(a[4].cpu(), b[4].cpu()), what + ": labels"
