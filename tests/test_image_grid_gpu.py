"""The snapshot image grid on the MI355X: s2i_image_grid_u8 (ops.image_grid_uint8) against the float32 restatement
(grid_ref.py), bit for bit; the grids condGANTrainer.train() writes at every snapshot and what they leave of the training
state (nothing); the interpolation strip of speech_to_image --interpolate.

Bit-identical means torch.equal on the uint8 grid: the arithmetic is fully specified (include/s2i_hip.h) and numpy float32
reproduces it operation by operation, so there is no tolerance anywhere in this file."""
import os
import wave

import numpy as np
import pytest
import torch
from PIL import Image

import grid_ref as G
from helpers import CASES, configure

pytestmark = pytest.mark.gpu


# ---- the kernel --------------------------------------------------------------------------------------------------------
def _batch(seed, N, H, W, layout):
    """randn * 1.5 (values well outside [-1, 1]); NHWC batches are NHWC4 with NaN in the channel nothing may read."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, 3, H, W)) * 1.5).astype(np.float32)
    if layout == "nchw":
        return x
    y = np.full((N, H, W, 4), np.nan, np.float32)
    y[..., :3] = x.transpose(0, 2, 3, 1)
    return y


def _check(gpu, x, nrow, padding, layout):
    from speech_to_image_translation_without_text_amd import ops
    got = ops.image_grid_uint8(torch.from_numpy(x).to(gpu), nrow=nrow, padding=padding, layout=layout)
    want = torch.from_numpy(G.image_grid_u8(x, nrow, padding, layout))
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%d of %d bytes differ, first at %s: got %d, want %d" % (
            len(bad), want.numel(), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))
    return got


@pytest.mark.parametrize("N,H,W,nrow,padding,layout", [
    (1, 4, 4, 8, 2, "nchw"),          # one image: xmaps = N
    (5, 6, 10, 8, 2, "nchw"),         # one partial row; H != W catches swapped strides
    (11, 64, 64, 8, 2, "nhwc"),       # two rows, the last one partial; NaN in the fourth channel
    (23, 16, 16, 10, 2, "nchw"),      # nrow != 8, three rows
    (5, 6, 10, 8, 0, "nchw"),         # no padding
    (7, 5, 3, 2, 3, "nhwc"),          # padding wider than an image is tall, odd sizes
])
def test_grid_matches_float32_restatement(gpu, N, H, W, nrow, padding, layout):
    _check(gpu, _batch(N * 100 + H, N, H, W, layout), nrow, padding, layout)


def test_extrema_in_the_last_image_of_a_many_block_reduction(gpu):
    """8 x 256 x 256 NHWC4: 2048 blocks' worth of pixels on the capped reduction grid; the global minimum and maximum sit
    in the last image, the maximum in its very last pixel."""
    x = _batch(8, 8, 256, 256, "nhwc")
    x[7, 255, 255, 2] = 9.0
    x[7, 200, 13, 0] = -9.5
    got = _check(gpu, x, 8, 2, "nhwc")
    assert got[2 + 255, 7 * 258 + 2 + 255].tolist()[2] == 255 and got[2 + 200, 7 * 258 + 2 + 13].tolist()[0] == 0


def test_constant_batch_and_views(gpu):
    from speech_to_image_translation_without_text_amd import ops
    x = np.full((3, 3, 8, 8), -0.25, np.float32)
    assert not _check(gpu, x, 8, 2, "nchw").any()
    # a batch slice and a channel slice are taken by their strides, a bf16 batch is converted first
    big = torch.from_numpy(_batch(3, 9, 8, 12, "nchw")).to(gpu)
    part = ops.image_grid_uint8(big[:5], nrow=8, padding=2)
    assert torch.equal(part.cpu(), torch.from_numpy(G.image_grid_u8(big[:5].cpu().numpy())))
    wide = torch.randn(4, 6, 8, 12, device=gpu)
    assert torch.equal(ops.image_grid_uint8(wide[:, 2:5]).cpu(),
                       torch.from_numpy(G.image_grid_u8(wide[:, 2:5].cpu().numpy())))
    half = big[:5].to(torch.bfloat16)
    assert torch.equal(ops.image_grid_uint8(half).cpu(), torch.from_numpy(G.image_grid_u8(half.float().cpu().numpy())))


def test_bad_arguments_launch_nothing(gpu):
    from speech_to_image_translation_without_text_amd import _lib, ops
    lib = _lib.load()
    src = torch.randn(2, 3, 4, 4, device=gpu)
    ws = torch.zeros(lib.s2i_image_grid_workspace_bytes() // 4, device=gpu)
    dst = torch.full((8, 14, 3), 7, dtype=torch.uint8, device=gpu)
    good = dict(src=src.data_ptr(), N=2, H=4, W=4, nrow=8, padding=2, ws=ws.data_ptr(), dst=dst.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.s2i_image_grid_u8(a['src'], a['N'], a['H'], a['W'], 48, 4, 1, 16, a['nrow'], a['padding'], a['ws'],
                                     a['dst'], _lib.stream())
    for bad in (dict(N=0), dict(N=-3), dict(H=0), dict(W=-1), dict(nrow=0), dict(padding=-1), dict(src=None),
                dict(ws=None), dict(dst=None), dict(H=2 ** 31 - 1, padding=2 ** 31 - 1)):
        with pytest.raises(_lib.S2IError, match="image_grid_u8"):
            _lib.check(call(**bad), "s2i_image_grid_u8")
    torch.cuda.synchronize()
    assert bool((dst == 7).all()) and not bool(ws.any())
    with pytest.raises(_lib.S2IError):
        ops.image_grid_uint8(src, nrow=0)
    with pytest.raises(ValueError):
        ops.image_grid_uint8(src, layout="chwn")
    _lib.check(call(), "s2i_image_grid_u8")
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), torch.from_numpy(G.image_grid_u8(src.cpu().numpy())))


# ---- the trainer's snapshots -------------------------------------------------------------------------------------------
def _train(out_dir, vis_count):
    """The seeded two-epoch run of test_model_gpu.test_training_loop_checkpoint_and_resume (small3 widths, B = 8, two
    batches per epoch) with a snapshot every second iteration; returns the trainer and what each snapshot handed back."""
    from speech_to_image_translation_without_text_amd import trainer as T
    from speech_to_image_translation_without_text_amd.miscc.config import cfg, cfg_reset
    case = dict(CASES['small3'], B=8)
    seen = []

    class Recording(T.condGANTrainer):
        def snapshot_images(self, count, real_imgs, txt_embedding):
            grids = super().snapshot_images(count, real_imgs, txt_embedding)
            seen.append(dict(count=count, grids=[g.cpu().numpy() for g in grids], real=real_imgs[-1].cpu().numpy(),
                             fake=[f.cpu().numpy() for f in self.fake_imgs]))
            return grids
    try:
        configure(case)
        cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.SNAPSHOT_INTERVAL, cfg.TRAIN.VIS_COUNT = 2, 2, vis_count
        g = torch.Generator().manual_seed(2)

        def sample():
            imgs = [torch.rand(8, 3, 64 << i, 64 << i, generator=g) * 2 - 1 for i in range(3)]
            wrong = [torch.rand(8, 3, 64 << i, 64 << i, generator=g) * 2 - 1 for i in range(3)]
            return imgs, wrong, torch.randn(8, case['t'], generator=g), ['k'] * 8, torch.arange(8) % 3
        loader = [sample(), sample()]
        torch.manual_seed(0)
        tr = Recording(str(out_dir), loader, 256, False)
        tr.train()
        torch.cuda.synchronize()
    finally:
        cfg_reset()
    return tr, seen


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("snapshots")
    return d, _train(d / "on", 5), _train(d / "off", 0)


def test_train_writes_the_reference_grids(runs):
    d, (tr, seen), _ = runs
    image_dir = d / "on" / "Image"
    assert [s['count'] for s in seen] == [2, 4]
    want_files = {"real_samples.png"} | {"count_%09d_fake_samples%d.png" % (c, i) for c in (2, 4) for i in range(3)}
    assert set(os.listdir(image_dir)) == want_files
    for s in seen:
        assert len(s['grids']) == 4
        sizes = [256] + [64 << i for i in range(3)]
        for grid, size in zip(s['grids'], sizes):
            assert grid.dtype == np.uint8 and grid.shape == (size + 4, 5 * (size + 2) + 2, 3)
        for i in range(3):
            png = np.asarray(Image.open(image_dir / ("count_%09d_fake_samples%d.png" % (s['count'], i))))
            np.testing.assert_array_equal(png, s['grids'][1 + i])
            assert s['fake'][i].shape == (8, 64 << i, 64 << i, 4)
            np.testing.assert_array_equal(s['grids'][1 + i], G.image_grid_u8(s['fake'][i][:5], 8, 2, "nhwc"))
            assert s['grids'][1 + i].max() == 255          # a generator's tanh output spans more than a point
        np.testing.assert_array_equal(s['grids'][0], G.image_grid_u8(s['real'][:5], 8, 2, "nchw"))
    # real_samples.png is overwritten: it shows the last snapshot's batch; the trainer keeps the last snapshot's images
    np.testing.assert_array_equal(np.asarray(Image.open(image_dir / "real_samples.png")), seen[-1]['grids'][0])
    assert not np.array_equal(seen[0]['grids'][3], seen[1]['grids'][3])     # the EMA generator moved in between
    for i in range(3):
        np.testing.assert_array_equal(seen[-1]['grids'][1 + i],
                                      G.image_grid_u8(tr.fake_imgs[i][:5].cpu().numpy(), 8, 2, "nhwc"))
    # one noise for the run, from a private generator
    assert tuple(tr.fixed_noise.shape) == (8, CASES['small3']['z'])
    assert tuple(tr.fixed_eps.shape) == (8, CASES['small3']['ef'])


def test_snapshots_leave_the_training_state_alone(runs):
    """The same seeded run with VIS_COUNT = 0 and VIS_COUNT = 5: every tensor of every checkpoint is bit-identical, the
    BatchNorm step counters included, and without VIS_COUNT no picture is written."""
    d, _, (tr_off, seen_off) = runs
    assert seen_off == [] and os.listdir(d / "off" / "Image") == []
    for name in ["netG_2.pth", "netG_4.pth"] + ["netD%d.pth" % i for i in range(3)]:
        on = torch.load(str(d / "on" / "Model" / name), weights_only=True, map_location="cpu")
        off = torch.load(str(d / "off" / "Model" / name), weights_only=True, map_location="cpu")
        assert list(on) == list(off) and len(on) > 0
        for k in on:
            assert torch.equal(on[k], off[k]), (name, k)
    sdG = torch.load(str(d / "on" / "Model" / "netG_4.pth"), weights_only=True, map_location="cpu")
    tracked = [k for k in sdG if k.endswith("num_batches_tracked")]
    assert tracked and all(int(sdG[k]) == 4 for k in tracked)


# ---- the interpolation strip -------------------------------------------------------------------------------------------
def _write_wav(path, y):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.clip(np.round(y * 32768), -32768, 32767).astype("<i2").tobytes())


def test_speech_to_image_interpolation(gpu, tmp_path, capsys):
    from speech_to_image_translation_without_text_amd import extract_audio_feature as E
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd import speech_to_image as S
    from speech_to_image_translation_without_text_amd.miscc.config import cfg_from_file, cfg_reset
    from speech_to_image_translation_without_text_amd.model import G_NET
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    from speech_to_image_translation_without_text_amd.trainer import weights_init
    rng = np.random.default_rng(7)
    wavs = []
    for j, n in enumerate((16000, 21000)):
        t = np.arange(n) / 16000.0
        y = 0.3 * np.sin(2 * np.pi * (150 + 90 * j) * t * (1 + 0.2 * t)) + 0.02 * rng.standard_normal(n)
        wavs.append(str(tmp_path / ("u%d.wav" % j)))
        _write_wav(wavs[-1], y)
    torch.manual_seed(0)
    enc = CNNRNN(40, embedding_dim=1024, nhidden=1024, nsent=1024, bidirectional=True, rnn_layers=1)
    g = torch.Generator().manual_seed(5)
    for k, v in enc.state_dict().items():
        if k.endswith('running_mean'):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith('running_var'):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
    torch.save({"meta": {}, "state_dict": enc.state_dict()}, tmp_path / "enc.pt")
    yml = tmp_path / "g.yml"
    yml.write_text("GAN:\n  GF_DIM: 16\n  Z_DIM: 100\n  EMBEDDING_DIM: 128\n  R_NUM: 2\n  B_CONDITION: True\n"
                   "TREE:\n  BRANCH_NUM: 2\n  BASE_SIZE: 64\nTEXT:\n  DIMENSION: 1024\n")
    cfg_reset()
    cfg_from_file(str(yml))
    try:
        torch.manual_seed(3)
        netG = G_NET()
        netG.apply(weights_init)
        torch.save({"module." + k: v for k, v in netG.state_dict().items()}, tmp_path / "netG_7.pth")
        common = ["--model", str(tmp_path / "enc.pt"), "--netG", str(tmp_path / "netG_7.pth"), "--out_dir",
                  str(tmp_path / "png"), "--cfg", str(yml), "--bidirectional", "--seed", "5", "--interpolate", "3"]
        with pytest.raises(SystemExit):
            S.main(common + wavs[:1])                       # exactly two utterances
        capsys.readouterr()
        S.main(common + wavs)
        printed = capsys.readouterr().out.split()
        model = E.load_encoder(str(tmp_path / "enc.pt"), bidirectional=True, device=gpu)
        emb = S.embed(model, E.read_wavs(wavs))
        imgs = S.interpolate(netG.to(gpu).eval(), emb[0], emb[1], 3, 5)
        want_singles = ops.images_to_uint8_hwc(imgs).cpu().numpy()
        imgs = imgs.cpu().numpy()
    finally:
        cfg_reset()
    names = ["interp_%d.png" % i for i in range(4)] + ["interp_grid.png"]
    assert sorted(os.listdir(tmp_path / "png")) == sorted(names)
    assert printed == [str(tmp_path / "png" / n) for n in names]
    assert imgs.shape == (4, 128, 128, 4)
    strip = np.asarray(Image.open(tmp_path / "png" / "interp_grid.png"))
    assert strip.shape == (128 + 4, 4 * 130 + 2, 3)
    np.testing.assert_array_equal(strip, G.image_grid_u8(imgs, nrow=4, padding=2, layout="nhwc"))
    singles = [np.asarray(Image.open(tmp_path / "png" / n)) for n in names[:4]]
    assert all(s.shape == (128, 128, 3) for s in singles)
    np.testing.assert_array_equal(np.stack(singles), want_singles)
    assert not np.array_equal(singles[0], singles[-1])
