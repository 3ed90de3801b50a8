"""CPU suite of the Inception-v3 scorer: the reference's metric functions reproduced from a fixture the reference itself
generated (tests/golden/make_golden_inception_metrics.py), the torchvision-layout weights loader and BatchNorm folding,
and the general convolution's descriptor validation (host code, no GPU)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, random_state_dict

_spec = importlib.util.spec_from_file_location("make_golden_inception_metrics",
                                               os.path.join(GOLDEN, "make_golden_inception_metrics.py"))
mgm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgm)


def test_metrics_match_the_reference_fixture():
    from speech_to_image_translation_without_text_amd import trainer as T
    gold = np.load(os.path.join(GOLDEN, "inception_metrics.npz"))
    for seed, rows, classes, splits in mgm.SOFTMAX_CASES:
        p = mgm.softmax_rows(seed, rows, classes)
        np.testing.assert_allclose(T.compute_inception_score(p, splits), gold["is_%d" % seed], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(T.negative_log_posterior_probability(p, splits), gold["nlpp_%d" % seed], rtol=1e-10,
                                   atol=1e-12)
    for seed, rg, rr, dim in mgm.FID_CASES:
        g, r = mgm.features(seed, rg, rr, dim)
        fid, data = T.compute_frethet_distance(g, r)
        np.testing.assert_allclose(fid, gold["fid_%d" % seed], rtol=1e-6)
        assert data[0]["sigma"].shape == (dim, dim)


def test_state_dict_layout_and_parameter_count():
    from speech_to_image_translation_without_text_amd import inception as I
    assert I.parameter_count() == 27161264            # torchvision's published figure (aux_logits=True)
    assert len(I.architecture(aux_logits=False)) == 94
    shapes = I.state_dict_shapes()
    assert shapes["Mixed_6b.branch7x7dbl_3.conv.weight"] == (128, 128, 1, 7)
    assert shapes["Mixed_7b.branch3x3_2a.bn.running_var"] == (384,)
    assert shapes["Mixed_7c.branch3x3dbl_1.conv.weight"] == (448, 2048, 1, 1)
    assert shapes["Conv2d_1a_3x3.conv.weight"] == (32, 3, 3, 3)
    assert shapes["fc.weight"] == (1000, 2048)


@pytest.mark.parametrize("nbt", [True, False], ids=["with_num_batches_tracked", "without"])
def test_loader_accepts_torchvision_files(tmp_path, nbt):
    from speech_to_image_translation_without_text_amd import model
    path = tmp_path / "inception.pth"
    torch.save(random_state_dict(num_batches_tracked=nbt), str(path))
    m = model.INCEPTION_V3(weights=str(path))
    assert not any(k.startswith("AuxLogits.") for k in m.state)
    assert "Mixed_7c.branch_pool.conv.weight" in m.state
    with pytest.raises(RuntimeError):           # no fall-back on the CPU
        m(torch.zeros(1, 3, 64, 64))


def test_loader_rejects_missing_misshaped_and_unknown_keys():
    from speech_to_image_translation_without_text_amd import model
    sd = random_state_dict(aux_logits=False)
    del sd["Mixed_6e.branch7x7_2.bn.running_mean"]
    with pytest.raises(ValueError, match="lack"):
        model.INCEPTION_V3(weights=sd)
    sd = random_state_dict(aux_logits=False)
    sd["Mixed_5b.branch5x5_2.conv.weight"] = torch.zeros(64, 48, 3, 3)
    with pytest.raises(ValueError, match="shape"):
        model.INCEPTION_V3(weights=sd)
    sd = random_state_dict(aux_logits=False)
    sd["Mixed_8a.conv.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unexpected"):
        model.INCEPTION_V3(weights=sd)


def test_no_weights_keeps_raising():
    from speech_to_image_translation_without_text_amd import model
    with pytest.raises(RuntimeError):
        model.INCEPTION_V3()(torch.zeros(1, 3, 64, 64))


def test_batchnorm_folding_in_float64():
    """conv + BatchNorm(eps=1e-3, eval) + ReLU == relu(conv(x, w') + b') with the folded pair, for a 1x7 and a 3x3 s2."""
    from speech_to_image_translation_without_text_amd import inception as I
    sd = random_state_dict(1, aux_logits=False)
    folded = I.fold(sd)
    g = torch.Generator().manual_seed(3)
    for name in ("Mixed_6c.branch7x7_2", "Mixed_6a.branch3x3"):
        cin, cout, kh, kw, sh, sw, ph, pw = I.architecture()[name]
        x = torch.randn(2, cin, 11, 13, generator=g, dtype=torch.float64)
        ref = F.conv2d(x, sd[name + ".conv.weight"].double(), None, (sh, sw), (ph, pw))
        ref = F.relu(F.batch_norm(ref, sd[name + ".bn.running_mean"].double(), sd[name + ".bn.running_var"].double(),
                                  sd[name + ".bn.weight"].double(), sd[name + ".bn.bias"].double(), False, 0.0, 1e-3))
        w, b = folded[name]
        got = F.relu(F.conv2d(x, w, b, (sh, sw), (ph, pw)))
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_weight_packing_layout():
    from speech_to_image_translation_without_text_amd import inception as I
    w = torch.randn(6, 3, 2, 5)
    P = I.pack_weight(w, cin_pad=4)
    assert P.shape == (2 * 5 * 4, 8)
    for ky, kx, c, o in ((1, 4, 2, 5), (0, 0, 0, 0), (1, 2, 1, 3)):
        assert P[(ky * 5 + kx) * 4 + c, o] == w[o, c, ky, kx]
    assert torch.all(P[:, 6:] == 0) and torch.all(P.reshape(2, 5, 4, 8)[:, :, 3] == 0)


def test_conv2d_descriptor_validation_without_a_gpu():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()

    def desc(**kw):
        f = dict(B=2, H=35, W=35, C=48, ldx=0, N=64, kh=5, kw=5, sh=1, sw=1, ph=2, pw=2, Ho=35, Wo=35, ldy=288,
                 coff=64, relu=1, tile=0)
        f.update(kw)
        return _lib.Conv2dDesc(*[f[n] for n, _ in _lib.Conv2dDesc._fields_])

    ok = desc()
    assert lib.s2i_conv2d_plan(ctypes.byref(ok)) in (1, 2, 3)
    assert lib.s2i_conv2d_weight_elems(ctypes.byref(ok)) == 25 * 48 * 64
    assert lib.s2i_conv2d_weight_elems(ctypes.byref(desc(N=80))) == 25 * 48 * 80
    assert lib.s2i_conv2d_weight_elems(ctypes.byref(desc(N=30, coff=0))) == 25 * 48 * 32
    for bad, word in ((desc(Ho=34), b"output"), (desc(ldy=100), b"fit"), (desc(ph=5), b"padding"),
                      (desc(sh=0), b"stride"), (desc(C=0), b"positive"), (desc(ldx=40), b"ldx"), (desc(tile=4), b"tile"),
                      (desc(B=48, H=2000, W=2000, C=64, N=64, kh=1, kw=1, ph=0, pw=0, Ho=2000, Wo=2000, ldy=64, coff=0),
                       b"2 GB")):
        assert lib.s2i_conv2d_plan(ctypes.byref(bad)) == -1
        assert word in lib.s2i_last_error()
        assert lib.s2i_conv2d_weight_elems(ctypes.byref(bad)) == 0
    assert lib.s2i_conv2d_forward(None, None, None, None, None, None) != 0
    for t in (1, 2, 3):
        assert lib.s2i_conv2d_plan(ctypes.byref(desc(tile=t))) == t
    # few rows, many channels: the planner prefers more, narrower blocks in one round over wide blocks
    small = desc(B=2, H=8, W=8, C=1280, N=384, kh=1, kw=1, ph=0, pw=0, Ho=8, Wo=8, ldy=384, coff=0)
    assert lib.s2i_conv2d_plan(ctypes.byref(small)) == 3


def test_pool_and_prep_argument_errors_without_a_gpu():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    assert lib.s2i_pool2d(7, 1, 2, 8, 8, 16, 16, 1, 16, 0, None) != 0 and b"mode" in lib.s2i_last_error()
    assert lib.s2i_pool2d(0, 1, 2, 8, 8, 16, 16, 1, 8, 0, None) != 0 and b"shape" in lib.s2i_last_error()
    assert lib.s2i_inception_prep(1, 2, 64, 64, 1, 1, 1, 1, 1, 299, 5, None) != 0
    assert lib.s2i_softmax_rows(1, 4, 1000, 999, 1, 1000, None) != 0


def test_inception_is_off_by_default():
    from speech_to_image_translation_without_text_amd import trainer as T
    from speech_to_image_translation_without_text_amd.miscc.config import cfg, cfg_reset
    cfg_reset()
    assert cfg.TRAIN.INCEPTION_WEIGHTS == ""
    tr = T.condGANTrainer(None, None, 256, False)
    assert tr.inception_model is None and tr.score_inception(10) is None
