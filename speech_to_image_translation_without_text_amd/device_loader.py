"""Training images resident in device memory; the per-step transform on the GPU.

The host path (datasets.py) repeats for every sample, twice (real and wrong image): decode, bounding-box crop,
`Resize(int(S * 76 / 64))`, random crop, random flip, two further PIL bilinear resizes, normalisation
(StackGAN_v2/datasets.py:40-66 behind main.py:127-131).  Everything up to the first random draw depends on the image
alone, so `ResidentTrainSet` does it once and keeps the uint8 result on the device; what changes per step -- an S x S
window, a mirror, the pyramid of that window, the normalisation -- is one launch of `s2i_image_batch` driven by a small
integer plan.  `plan_batch` makes the random draws with the calls and in the order of the host path, so with the same
seed of Python's `random` both paths choose the same captions, wrong images, windows and flips, and every tensor of a
batch is bit-identical to the host DataLoader's (tests/test_imagepipe_cpu.py, tests/test_imagepipe_gpu.py).

The host path stays the default; nothing here changes it.
"""
import math
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from . import datasets as D

MAX_DECODE_THREADS = 16
PRECISION_BITS = 32 - 8 - 2        # PIL's 8-bit resample keeps 22-bit fixed-point coefficients
_CHUNK_BYTES = 64 << 20            # host staging buffer of the pool upload


# ---- PIL's bilinear resample, restated -------------------------------------------------------------------------------
def pil_bilinear_coeffs(in_size, out_size):
    """The integer coefficients of PIL's `resize(..., BILINEAR)` along one axis of an 8-bit image: `(starts, taps)`,
    int32 arrays of shape (out_size,) and (out_size, ksize).  Output position x is
    `clip8(((1 << 21) + sum_k pixel[starts[x] + k] * taps[x, k]) >> 22)`; taps past a position's window are 0.
    Computed in double with PIL's own sequence of operations (precompute_coeffs + normalize_coeffs_8bpc)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("pil_bilinear_coeffs: sizes must be positive")
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    rows, starts = [], np.zeros(out_size, np.int32)
    for x in range(out_size):
        center = (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = []
        for i in range(xmin, xmax):
            a = abs((i - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        starts[x] = xmin
        rows.append([int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w])
    taps = np.zeros((out_size, max(len(r) for r in rows)), np.int32)
    for x, r in enumerate(rows):
        taps[x, :len(r)] = r
    return starts, taps


def coeff_table(in_size, out_size, ktaps):
    """`pil_bilinear_coeffs` in the layout `s2i_image_batch` reads: int32 (out_size, 1 + ktaps), the start index then
    the taps."""
    starts, taps = pil_bilinear_coeffs(in_size, out_size)
    if taps.shape[1] > ktaps:
        raise ValueError("%d -> %d needs %d taps, the kernel takes %d" % (in_size, out_size, taps.shape[1], ktaps))
    tab = np.zeros((out_size, 1 + ktaps), np.int32)
    tab[:, 0] = starts
    tab[:, 1:1 + taps.shape[1]] = taps
    return tab


# ---- what the standard transform does before and after its first random draw ------------------------------------------
def _standard_transform(dataset):
    """(S, resize) of a dataset built with `default_image_transform(S)`; anything else is refused."""
    tr = getattr(dataset, "transform", None)
    steps = getattr(tr, "transforms", None)
    if (not isinstance(tr, D.Compose) or len(steps) != 3 or type(steps[0]) is not D.Resize
            or type(steps[1]) is not D.RandomCrop or type(steps[2]) is not D.RandomHorizontalFlip):
        raise ValueError("ResidentTrainSet needs a dataset built with datasets.default_image_transform(S) "
                         "(Resize, RandomCrop, RandomHorizontalFlip); got %r" % (tr,))
    S = steps[1].size
    if steps[0].size != int(S * 76 / 64) or steps[2].p != 0.5:
        raise ValueError("ResidentTrainSet: transform is not default_image_transform(%d): Resize(%d), flip p = %r"
                         % (S, steps[0].size, steps[2].p))
    L = len(dataset.imsize)
    if not 1 <= L <= 3 or list(dataset.imsize) != [S >> (L - 1 - i) for i in range(L)] or S % (1 << (L - 1)):
        raise ValueError("ResidentTrainSet: branch sizes %r do not halve down from the crop size %d" % (dataset.imsize, S))
    return S, steps[0]


def _require_train(dataset):
    if getattr(getattr(dataset, "iterator", None), "__name__", "") != "prepare_train_pairs":
        raise ValueError("ResidentTrainSet holds the train split: the dataset was built with train=False")


def _path_of(dataset, index):
    rel = dataset._get_img(dataset.json_data[index])
    return rel, os.path.join(dataset.image_folder, rel)


def _resident_size(dataset, resize, index):
    """(h, w) of item `index` after the bounding-box crop and the Resize, from the file header alone."""
    rel, full = _path_of(dataset, index)
    with Image.open(full) as img:
        w, h = img.size
    bbox = dataset._get_bbox(rel)
    if bbox is not None:
        x1, y1, x2, y2 = D.crop_box(bbox, w, h)
        w, h = x2 - x1, y2 - y1
    w, h = resize.output_size(w, h)
    return h, w


def _resident_image(dataset, resize, index):
    """get_imgs up to the first random draw (datasets.py:40-56): open, RGB, crop_box, Resize -> uint8 HWC."""
    rel, full = _path_of(dataset, index)
    img = Image.open(full).convert('RGB')
    bbox = dataset._get_bbox(rel)
    if bbox is not None:
        img = img.crop(D.crop_box(bbox, *img.size))
    return np.asarray(resize(img), dtype=np.uint8)


class _HostIndex:
    """What `plan_batch` needs of a dataset, read once: per-item class label, path and resident (h, w)."""

    def __init__(self, dataset, workers=MAX_DECODE_THREADS):
        _require_train(dataset)
        self.size, resize = _standard_transform(dataset)
        n = len(dataset)
        self.paths = [dataset._get_img(it) for it in dataset.json_data]
        self.labels = [dataset._get_class(it) for it in dataset.json_data]
        with ThreadPoolExecutor(max_workers=_threads(workers)) as ex:
            self.hw = np.array(list(ex.map(lambda i: _resident_size(dataset, resize, i), range(n))),
                               dtype=np.int32).reshape(n, 2)
        if n and int(self.hw.min()) < self.size:
            raise ValueError("ResidentTrainSet: an image is smaller than the crop after Resize")


def _threads(workers):
    return max(1, min(int(workers), MAX_DECODE_THREADS))


def host_index(dataset, workers=MAX_DECODE_THREADS):
    idx = dataset.__dict__.get("_resident_index")
    if idx is None:
        idx = dataset.__dict__["_resident_index"] = _HostIndex(dataset, workers)
    return idx


def plan_batch(dataset, indices, rng=random):
    """The random draws of one batch, with the calls and in the order `dataset[i]` makes them for i in `indices`
    (BaseDataset.prepare_train_pairs): per item the caption (`get_rand`), the rejection loop of `find_wrong_image`,
    then for the real and for the wrong image RandomCrop's two `randint`s (none when the image is the crop size already)
    and RandomHorizontalFlip's `random()`.

    Returns (plan, captions, paths, labels): plan int32 (2B, 4) of (pool index, top, left, flip), the B real rows
    first, then the B wrong rows; the caption index, image path and class label of every item."""
    hi = host_index(dataset)
    t, n_items = hi.size, len(hi.labels)
    B = len(indices)
    plan = np.zeros((2 * B, 4), np.int32)
    captions, paths, labels = [], [], []
    for b, index in enumerate(indices):
        index = int(index)
        label = hi.labels[index]
        captions.append(rng.randint(0, len(dataset.embedding[index]) - 1))
        while True:
            wrong = rng.randint(0, n_items - 1)
            if hi.labels[wrong] != label:
                break
        for row, item in ((b, index), (B + b, wrong)):
            h, w = int(hi.hw[item, 0]), int(hi.hw[item, 1])
            top = left = 0
            if not (w == t and h == t):
                top = rng.randint(0, h - t)
                left = rng.randint(0, w - t)
            plan[row] = (item, top, left, 1 if rng.random() < 0.5 else 0)
        paths.append(hi.paths[index])
        labels.append(label)
    return plan, captions, paths, labels


# ---- the resident pool ---------------------------------------------------------------------------------------------
class ResidentTrainSet:
    """Every train image of `dataset` (a train-mode BirdsDataset, FlowersDataset or other BaseDataset built with
    `default_image_transform(S)`) after its bounding-box crop and `Resize(int(S * 76 / 64))`, as uint8 HWC in one
    contiguous buffer on `device`, with device tables of each image's byte offset (int64) and (h, w) (int32).  Class
    labels, paths and the (N, 10, D) embedding array stay on the host.  CUB at S = 256 is about 3 GB."""

    def __init__(self, dataset, device, workers=16):
        self.dataset = dataset
        self.device = torch.device(device)
        self.index = host_index(dataset, workers)
        self.size = self.index.size
        self.levels = len(dataset.imsize)
        _, resize = _standard_transform(dataset)
        hw = self.index.hw
        nbytes = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64) * 3
        offsets = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)
        self.pool_bytes = int(offsets[-1])
        self.pool = torch.empty(self.pool_bytes, dtype=torch.uint8, device=self.device)
        self._upload(dataset, resize, offsets, _threads(workers))
        self.offsets = torch.from_numpy(offsets[:-1].copy()).to(self.device)
        self.sizes = torch.from_numpy(np.ascontiguousarray(hw)).to(self.device)
        self.host_offsets = offsets
        S = self.size
        self.tab1 = torch.from_numpy(coeff_table(S, S // 2, 4)).to(self.device) if self.levels >= 2 else None
        self.tab2 = torch.from_numpy(coeff_table(S, S // 4, 8)).to(self.device) if self.levels >= 3 else None
        self.embedding = np.asarray(dataset.embedding)

    def _upload(self, dataset, resize, offsets, threads):
        """Decode with a bounded thread pool, in chunks of about 64 MB that go to the device as one copy each."""
        n = len(dataset)
        with ThreadPoolExecutor(max_workers=threads) as ex:
            first = 0
            while first < n:
                last = first + 1
                while last < n and offsets[last + 1] - offsets[first] <= _CHUNK_BYTES:
                    last += 1
                stage = np.empty(int(offsets[last] - offsets[first]), np.uint8)
                for i, a in zip(range(first, last), ex.map(lambda i: _resident_image(dataset, resize, i),
                                                           range(first, last))):
                    if a.shape != (int(self.index.hw[i, 0]), int(self.index.hw[i, 1]), 3):
                        raise ValueError("%s decodes to %r, its header promised %r"
                                         % (self.index.paths[i], a.shape, tuple(self.index.hw[i])))
                    o = int(offsets[i] - offsets[first])
                    stage[o:o + a.size] = a.reshape(-1)
                self.pool[int(offsets[first]):int(offsets[last])].copy_(torch.from_numpy(stage))
                first = last

    def __len__(self):
        return len(self.dataset)

    def image(self, index):
        """Resident image `index` as a uint8 (h, w, 3) tensor on the pool's device (a view of the pool)."""
        h, w = (int(v) for v in self.index.hw[index])
        o = int(self.host_offsets[index])
        return self.pool[o:o + h * w * 3].view(h, w, 3)

    def batch(self, indices, rng=random):
        """One train tuple `(real_imgs, wrong_imgs, embedding, paths, labels)` in the layout the host DataLoader's
        default collation yields: image lists smallest branch first, float32 NCHW on the device; embedding (B, D)
        float32, paths a list of strings, labels an int64 tensor."""
        from . import _lib, ops
        if self.device.type != "cuda":
            raise _lib.S2IError("the image pool is on %s: batches are made by the MI355X kernel, there is no CPU "
                                "fallback" % self.device)
        plan, captions, paths, labels = plan_batch(self.dataset, indices, rng)
        B = len(paths)
        # one small pinned copy; the caching host allocator keeps the block until the copy has run
        plan_dev = torch.from_numpy(plan).pin_memory().to(self.device, non_blocking=True)
        outs = ops.image_batch(self.pool, self.offsets, self.sizes, plan_dev, self.size, self.levels, self.tab1,
                               self.tab2)
        real = [o[:B] for o in reversed(outs)]
        wrong = [o[B:] for o in reversed(outs)]
        emb = torch.from_numpy(np.stack([self.embedding[i][c] for i, c in zip(indices, captions)]))
        return real, wrong, emb, paths, torch.tensor(labels, dtype=torch.int64)

    def loader(self, batch_size, shuffle=True, rank=None, world_size=None, seed=0):
        return ResidentLoader(self, batch_size, shuffle, rank, world_size, seed)


class ResidentLoader:
    """Iterates a ResidentTrainSet like `make_dataloader`'s DataLoader: `len`, `iter`, a ragged last batch.  Without
    shuffling the order is 0..N-1; with it, each epoch has its own permutation seeded by `seed + epoch` (`set_epoch`).
    With `rank` and `world_size` that permutation is dealt round-robin to the ranks: the shards are disjoint and cover
    the split when world_size divides N, and are otherwise padded from the permutation's head, as DistributedSampler
    pads, so that every rank runs the same number of steps."""

    def __init__(self, resident, batch_size, shuffle=True, rank=None, world_size=None, seed=0):
        if (rank is None) != (world_size is None):
            raise ValueError("ResidentLoader: rank and world_size go together")
        if rank is not None and not 0 <= rank < world_size:
            raise ValueError("ResidentLoader: rank %r outside 0..%d" % (rank, world_size - 1))
        self.dataset = resident
        self.batch_size = int(batch_size)
        self.shuffle, self.rank, self.world_size, self.seed = bool(shuffle), rank, world_size, int(seed)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        if self.rank is not None:
            total = math.ceil(n / self.world_size) * self.world_size
            order = (order + order[:total - n])[self.rank:total:self.world_size]
        return order

    def _count(self):
        n = len(self.dataset)
        return n if self.rank is None else math.ceil(n / self.world_size)

    def __len__(self):
        return math.ceil(self._count() / self.batch_size)

    def __iter__(self):
        order = self.indices()
        for first in range(0, len(order), self.batch_size):
            yield self.dataset.batch(order[first:first + self.batch_size])
