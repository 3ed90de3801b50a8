"""The resident image pipeline on the MI355X (csrc/s2i_imagepipe.hip, device_loader.py): the kernel against the integer
reference of tests/imagepipe_ref.py, whole batches against the host DataLoader under the same seed, and the batches
through the train step and the trainer's loop.  Every comparison is an equality over every element."""
import random

import numpy as np
import pytest
import torch

import imagepipe_ref as R
from helpers import CASES, build_nets, configure

from speech_to_image_translation_without_text_amd import datasets as D
from speech_to_image_translation_without_text_amd import device_loader as DL
from speech_to_image_translation_without_text_amd.miscc.config import cfg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size,shapes", [(256, [(300, 341), (256, 256), (311, 257)]), (64, [(76, 95), (64, 64), (90, 65)])])
def test_kernel_corner_cases_against_the_integer_reference(gpu, size, shapes):
    """A hand-made plan on non-square resident images: windows at both ends of both axes, both flip values, an image
    that is exactly the window, a second and third image behind the first (offset table), L = 1, 2 and 3."""
    from speech_to_image_translation_without_text_amd import ops
    rng = np.random.RandomState(size)
    imgs = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    imgs[2][::2, ::2] = 0
    imgs[2][1::2, 1::2] = 255                                 # hard edges: the clamp and the rounding both matter
    offs = np.concatenate([[0], np.cumsum([a.size for a in imgs])]).astype(np.int64)
    pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(gpu)
    offsets = torch.from_numpy(offs[:-1].copy()).to(gpu)
    sizes = torch.tensor(shapes, dtype=torch.int32, device=gpu)
    rows = []
    for item, (h, w) in enumerate(shapes):
        for top in sorted({0, h - size, (h - size) // 2}):
            for left in sorted({0, w - size, (w - size) // 3}):
                for flip in (0, 1):
                    rows.append((item, top, left, flip))
    plan = np.array(rows, dtype=np.int32)
    assert {(r[1], r[2]) for r in rows if r[0] == 0} >= {(0, 0), (shapes[0][0] - size, shapes[0][1] - size)}
    tab1 = torch.from_numpy(DL.coeff_table(size, size // 2, 4)).to(gpu)
    tab2 = torch.from_numpy(DL.coeff_table(size, size // 4, 8)).to(gpu)
    plan_dev = torch.from_numpy(plan).to(gpu)
    for levels in (1, 2, 3):
        outs = ops.image_batch(pool, offsets, sizes, plan_dev, size, levels, tab1 if levels >= 2 else None,
                               tab2 if levels >= 3 else None)
        assert [tuple(o.shape) for o in outs] == [(len(rows), 3, size >> i, size >> i) for i in range(levels)]
        outs = [o.cpu() for o in outs]
        for k, (item, top, left, flip) in enumerate(rows):
            ref = R.pyramid(imgs[item], top, left, flip, size, levels)
            for i in range(levels):
                assert outs[i].dtype == torch.float32 and torch.equal(outs[i][k], ref[i]), (
                    "L=%d row %r level %d: %d elements differ" % (levels, rows[k], i, int((outs[i][k] != ref[i]).sum())))


def test_kernel_skips_a_row_that_does_not_fit(gpu):
    """A plan row outside its image or outside the pool reads nothing and writes nothing; its neighbours are served."""
    from speech_to_image_translation_without_text_amd import ops
    img = np.random.RandomState(0).randint(0, 256, (80, 70, 3), dtype=np.uint8)
    pool = torch.from_numpy(img.reshape(-1)).to(gpu)
    offsets = torch.zeros(1, dtype=torch.int64, device=gpu)
    sizes = torch.tensor([[80, 70]], dtype=torch.int32, device=gpu)
    plan = torch.tensor([[0, 16, 6, 0], [0, 17, 0, 0], [0, 0, 7, 1], [1, 0, 0, 0], [-1, 0, 0, 0], [0, -1, 0, 0],
                         [0, 3, 2, 1]], dtype=torch.int32, device=gpu)
    tab1 = torch.from_numpy(DL.coeff_table(64, 32, 4)).to(gpu)
    out0, out1 = ops.image_batch(pool, offsets, sizes, plan, 64, 2, tab1)
    out0, out1 = out0.cpu(), out1.cpu()
    for k, (top, left, flip) in ((0, (16, 6, 0)), (6, (3, 2, 1))):
        ref = R.pyramid(img, top, left, flip, 64, 2)
        assert torch.equal(out0[k], ref[0]) and torch.equal(out1[k], ref[1])
    # the skipped rows were written by nobody: fill the outputs, run again into the same tensors, look at them
    from speech_to_image_translation_without_text_amd import _lib
    a = torch.full((7, 3, 64, 64), 7.0, device=gpu)
    b = torch.full((7, 3, 32, 32), 7.0, device=gpu)
    _lib.check(_lib.load().s2i_image_batch(_lib.ptr(pool), pool.numel(), _lib.ptr(offsets), _lib.ptr(sizes), 1,
                                           _lib.ptr(plan), 7, 64, 2, _lib.ptr(tab1), None, _lib.ptr(a), _lib.ptr(b), None,
                                           _lib.stream()), "s2i_image_batch")
    a, b = a.cpu(), b.cpu()
    for k in (1, 2, 3, 4, 5):
        assert bool((a[k] == 7.0).all()) and bool((b[k] == 7.0).all()), k
    assert torch.equal(a[0], out0[0]) and torch.equal(b[6], out1[6])


@pytest.mark.parametrize("size", [256, 64])       # 256 is the full size and also the small3 case's (its nets are narrow,
@pytest.mark.parametrize("birds", [True, False])  # not its images); 64 runs the pyramid 64 / 32 / 16
def test_epoch_equals_the_host_dataloader(gpu, tmp_path, birds, size):
    configure(CASES['small3'])
    R.make_tree(str(tmp_path), birds=birds, dim=CASES['small3']['t'])
    ds = R.make_dataset(str(tmp_path), birds, size)
    rs = DL.ResidentTrainSet(ds, gpu)
    assert rs.pool.device.type == "cuda" and rs.offsets.device.type == "cuda" and rs.sizes.device.type == "cuda"
    B = 5                                                     # 12 items: 5, 5 and a ragged 2
    random.seed(21)
    host = list(D.make_dataloader(ds, B, shuffle=False))
    random.seed(21)
    loader = rs.loader(B, shuffle=False)
    res = list(loader)
    assert len(loader) == len(host) == len(res) == 3 and res[-1][2].shape[0] == 2
    for k, (h, r) in enumerate(zip(host, res)):
        assert all(t.device.type == "cuda" and t.is_contiguous() for t in r[0] + r[1])
        assert [tuple(t.shape[1:]) for t in r[0]] == [(3, size >> 2, size >> 2), (3, size >> 1, size >> 1), (3, size, size)]
        assert isinstance(r[3], list) and r[4].dtype == torch.int64
        R.assert_batches_equal(h, r, "batch %d" % k)
    # a dataset that leaves normalisation to the device hands over uint8: the resident batch equals its normalised form
    from speech_to_image_translation_without_text_amd import ops
    du = R.make_dataset(str(tmp_path), birds, size, device_normalize=True)
    random.seed(21)
    first = next(iter(D.make_dataloader(du, B, shuffle=False)))
    for k in (0, 1):
        for i in range(3):
            assert torch.equal(ops.images_from_uint8_hwc(first[k][i].to(gpu).contiguous()), res[0][k][i])


def test_train_step_from_resident_batch_equals_host_batch(gpu, tmp_path):
    """Bit-identical inputs into a bitwise reproducible step: the losses are equal, not close."""
    from speech_to_image_translation_without_text_amd import trainer as T
    case = CASES['small3']
    configure(case)
    R.make_tree(str(tmp_path), birds=True, dim=case['t'])
    size = cfg.TREE.BASE_SIZE * 4
    losses = []
    for resident in (False, True):
        random.seed(11)
        netG, netsD = build_nets(case)
        netG.to(gpu)
        [d.to(gpu) for d in netsD]
        tr = T.condGANTrainer(None, None, size, False)
        tr.build(netG, netsD)
        ds = D.BirdsDataset(str(tmp_path), train=True, base_size=cfg.TREE.BASE_SIZE,
                            transform=D.default_image_transform(size))
        if resident:
            batch = next(iter(DL.ResidentTrainSet(ds, gpu).loader(8, shuffle=False)))
        else:
            batch = next(iter(D.make_dataloader(ds, 8, shuffle=False)))
        _, real, wrong, e, labels = tr.prepare_data(batch)
        if resident:
            assert all(a is b for a, b in zip(real, batch[0]))    # prepare_data passes float device tensors through
        g = torch.Generator(device=gpu).manual_seed(2)
        noise = torch.randn(8, cfg.GAN.Z_DIM, device=gpu, generator=g)
        eps = torch.randn(8, cfg.GAN.EMBEDDING_DIM, device=gpu, generator=g)
        errD, errG, kl = tr.train_step(real, wrong, e, labels, noise, eps)
        losses.append((float(errD), float(errG), float(kl)))
        assert all(np.isfinite(v) for v in losses[-1])
    print("host %r resident %r" % (losses[0], losses[1]))
    assert losses[0] == losses[1]


def test_trainer_loop_runs_from_the_resident_loader(gpu, tmp_path):
    """condGANTrainer.train() takes the loader as it takes a DataLoader: two steps of one epoch, then the checkpoints."""
    from speech_to_image_translation_without_text_amd import trainer as T
    case = dict(CASES['small3'], B=6)
    configure(case)
    try:
        cfg.TRAIN.MAX_EPOCH = 1
        cfg.TRAIN.SNAPSHOT_INTERVAL = 1000
        R.make_tree(str(tmp_path / "data"), birds=True, dim=case['t'])
        ds = D.BirdsDataset(str(tmp_path / "data"), train=True, base_size=cfg.TREE.BASE_SIZE,
                            transform=D.default_image_transform(256))
        loader = DL.ResidentTrainSet(ds, gpu).loader(6, shuffle=True, seed=1)
        assert len(loader) == 2
        torch.manual_seed(0)
        random.seed(0)
        tr = T.condGANTrainer(str(tmp_path / "run"), loader, 256, False)
        assert tr.num_batches == 2
        tr.train()
        model_dir = tmp_path / "run" / "Model"
        assert (model_dir / "netG_2.pth").exists() and all((model_dir / ("netD%d.pth" % i)).exists() for i in range(3))
        sdG = torch.load(str(model_dir / "netG_2.pth"), weights_only=True, map_location="cpu")
        assert all(torch.isfinite(v.float()).all() for v in sdG.values())
        assert int(sdG['module.h_net1.fc.1.num_batches_tracked']) == 2
    finally:
        cfg.TRAIN.MAX_EPOCH = 600
        cfg.TRAIN.SNAPSHOT_INTERVAL = 2000


def test_rank_shards_are_disjoint_and_cover_the_split(gpu, tmp_path):
    configure(CASES['small3'])
    R.make_tree(str(tmp_path), birds=False, dim=CASES['small3']['t'])
    rs = DL.ResidentTrainSet(R.make_dataset(str(tmp_path), False, 64), gpu)
    loaders = [rs.loader(3, shuffle=True, rank=r, world_size=2, seed=4) for r in range(2)]
    shards = [ld.indices() for ld in loaders]
    assert [len(s) for s in shards] == [6, 6] and [len(ld) for ld in loaders] == [2, 2]
    assert not set(shards[0]) & set(shards[1]) and sorted(shards[0] + shards[1]) == list(range(12))
    for ld in loaders:
        ld.set_epoch(1)
    again = [ld.indices() for ld in loaders]
    assert again != shards and sorted(again[0] + again[1]) == list(range(12)) and not set(again[0]) & set(again[1])
    # the batches a rank yields are its shard, in order
    random.seed(0)
    got = [p for batch in loaders[1] for p in batch[3]]
    assert got == [rs.index.paths[i] for i in again[1]]
