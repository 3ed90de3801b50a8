"""GPU suite of the Inception-v3 scorer: every distinct convolution of torchvision's Inception3 (s2i_conv2d_forward), the
pools, the input stage and the softmax against float64 CPU torch; the whole network with seeded torchvision-layout
weights against a float64 CPU restatement written here; and the trainer's opt-in scoring after eager and recorded steps."""
import ctypes
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import CASES, build_nets, make_batch, random_state_dict

pytestmark = pytest.mark.gpu


def conv_shapes():
    """(name, cin, cout, kh, kw, sh, sw, ph, pw, H): one entry per distinct shape of the eval network, plus the fc."""
    from speech_to_image_translation_without_text_amd import inception as I
    size = {"Conv2d_1a_3x3": 299, "Conv2d_2a_3x3": 149, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73,
            "Conv2d_4a_3x3": 73, "Mixed_5": 35, "Mixed_6a": 35, "Mixed_6": 17, "Mixed_7a": 17, "Mixed_7": 8}
    seen, out = set(), []
    for name, g in I.architecture(aux_logits=False).items():
        blk = name.split(".")[0]
        H = size.get(blk, size.get(blk[:7]))
        key = g + (H,)
        if key not in seen:
            seen.add(key)
            out.append((name,) + key)
    out.append(("fc", 2048, 1000, 1, 1, 1, 1, 0, 0, 1))
    return out


SHAPES = conv_shapes()


def run_conv(gpu, B, cin, cout, kh, kw, sh, sw, ph, pw, H, W=None, coff=0, extra=0, ldx_extra=0, relu=1, tile=0, seed=0,
             check_rows=None):
    from speech_to_image_translation_without_text_amd import _lib, inception as I
    W = W or H
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin + ldx_extra, generator=g)
    w = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    ldy = coff + cout + extra
    y = torch.full((B, Ho, Wo, ldy), 1234.5, device=gpu)
    d = _lib.Conv2dDesc(B, H, W, cin, cin + ldx_extra, cout, kh, kw, sh, sw, ph, pw, Ho, Wo, ldy, coff, relu, tile)
    xd, wd, bd = x.to(gpu), I.pack_weight(w.to(gpu)), b.to(gpu)
    assert wd.numel() == _lib.load().s2i_conv2d_weight_elems(ctypes.byref(d))
    _lib.check(_lib.load().s2i_conv2d_forward(ctypes.byref(d), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y),
                                              _lib.stream()), "s2i_conv2d_forward")
    got = y.cpu()
    rows = list(range(B)) if check_rows is None else check_rows
    xs = x[rows, :, :, :cin].permute(0, 3, 1, 2).double()
    ref = F.conv2d(xs, w.double(), b.double(), (sh, sw), (ph, pw))
    if relu:
        ref = F.relu(ref)
    ref = ref.permute(0, 2, 3, 1)
    sl = got[rows][..., coff:coff + cout].double()
    assert torch.all(got[..., :coff] == 1234.5) and torch.all(got[..., coff + cout:] == 1234.5), "wrote outside the slice"
    err = (sl - ref).abs().max().item()
    scale = ref.abs().max().item()
    return err, scale


@pytest.mark.parametrize("B", [2, 48])
@pytest.mark.parametrize("shape", SHAPES, ids=["%s_%dx%d_s%d_%d" % (s[0], s[3], s[4], s[5], s[9]) for s in SHAPES])
def test_conv2d_every_inception_shape(gpu, shape, B):
    name, cin, cout, kh, kw, sh, sw, ph, pw, H = shape
    rows = None if B <= 4 else [0, 23, 47]        # the float64 check of a 48-image launch looks at three of its images
    # write into a channel slice of a wider tensor with sentinels on both sides (coff 5 / 3 extra channels)
    err, scale = run_conv(gpu, B, cin, cout, kh, kw, sh, sw, ph, pw, H, coff=5, extra=3, relu=int(name != "fc"),
                          check_rows=rows, seed=SHAPES.index(shape))
    assert err <= 2e-5 * max(scale, 1.0), "%s: max |err| %.3g (scale %.3g)" % (name, err, scale)


@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("geom", [(3, 32, 3, 3, 2, 2, 0, 0, 37, 0), (4, 32, 3, 3, 2, 2, 0, 0, 37, 0),
                                  (160, 160, 1, 7, 1, 1, 0, 3, 17, 4), (96, 80, 5, 5, 1, 1, 2, 2, 13, 8),
                                  (448, 384, 3, 3, 1, 1, 1, 1, 8, 0), (36, 100, 7, 1, 1, 1, 3, 0, 11, 0)],
                         ids=["c3", "c4", "1x7_ldx", "5x5_ldx", "3x3_448", "7x1_c36"])
def test_conv2d_every_tile(gpu, geom, tile):
    """Each block tile on odd geometries: 3 channels (4-byte gather), an input pixel stride wider than C, N = 100."""
    cin, cout, kh, kw, sh, sw, ph, pw, H, ldx_extra = geom
    err, scale = run_conv(gpu, 3, cin, cout, kh, kw, sh, sw, ph, pw, H, W=H + 2, coff=7, extra=1, ldx_extra=ldx_extra,
                          tile=tile)
    assert err <= 2e-5 * max(scale, 1.0)


@pytest.mark.parametrize("mode", ["max", "avg", "global"])
def test_pools(gpu, mode):
    from speech_to_image_translation_without_text_amd import _lib
    g = torch.Generator().manual_seed(4)
    for B, H, C in ((2, 147, 64), (5, 35, 288), (3, 17, 768), (2, 8, 2048)):
        x = torch.randn(B, H, H, C + 4, generator=g)
        xn = x[..., :C].permute(0, 3, 1, 2).double()
        if mode == "max":
            ref, m = F.max_pool2d(xn, 3, 2), _lib.POOL_MAX3S2
        elif mode == "avg":
            ref, m = F.avg_pool2d(xn, 3, 1, 1, count_include_pad=True), _lib.POOL_AVG3S1
        else:
            ref, m = xn.mean((2, 3), keepdim=True), _lib.POOL_GLOBAL
        ref = ref.permute(0, 2, 3, 1)
        y = torch.full(ref.shape[:3] + (C + 10,), -7.0, device=gpu)
        _lib.check(_lib.load().s2i_pool2d(m, _lib.ptr(x.to(gpu)), B, H, H, C, C + 4, _lib.ptr(y), C + 10, 6, _lib.stream()),
                   "s2i_pool2d")
        got = y.cpu()
        assert torch.all(got[..., :6] == -7.0) and torch.all(got[..., 6 + C:] == -7.0)
        assert (got[..., 6:6 + C].double() - ref).abs().max().item() <= 2e-6


def reference_prep(img):
    """INCEPTION_V3.forward's input stage (model.py:93-104) in float64."""
    x = img.double() * 0.5 + 0.5
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64)[None, :, None, None]
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)[None, :, None, None]
    x = (x - mean) / std
    return F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)


@pytest.mark.parametrize("size", [64, 128, 256])
@pytest.mark.parametrize("layout", ["nchw", "nhwc4_view"])
def test_input_prep(gpu, size, layout):
    from speech_to_image_translation_without_text_amd import _lib
    g = torch.Generator().manual_seed(size)
    img = torch.rand(3, 3, size, size, generator=g) * 2 - 1
    if layout == "nchw":
        dev = img.to(gpu)
    else:    # what GET_IMAGE_G hands out: an NCHW view of NHWC4 storage
        store = torch.zeros(3, size, size, 4)
        store[..., :3] = img.permute(0, 2, 3, 1)
        dev = store.to(gpu).permute(0, 3, 1, 2)[:, :3]
    y = torch.full((3, 299, 299, 4), 5.0, device=gpu)
    sb, sc, sh, sw = dev.stride()
    _lib.check(_lib.load().s2i_inception_prep(_lib.ptr(dev), 3, size, size, sb, sc, sh, sw, _lib.ptr(y), 299, 4,
                                              _lib.stream()), "s2i_inception_prep")
    got = y.cpu()
    assert torch.all(got[..., 3] == 0)
    ref = reference_prep(img).permute(0, 2, 3, 1)
    # the source coordinate is a float32 product (as in torch's own float32 upsample): its rounding grows with the input
    # extent (measured 1.3e-5 / 3.0e-5 / 6.1e-5 at 64 / 128 / 256 px)
    assert (got[..., :3].double() - ref).abs().max().item() <= 2.5e-5 * size / 64
    # against the reference's own float32 computation (model.py:93-104) the difference is rounding only
    x32 = (img * 0.5 + 0.5 - torch.tensor([0.485, 0.456, 0.406])[None, :, None, None]) / \
        torch.tensor([0.229, 0.224, 0.225])[None, :, None, None]
    ref32 = F.interpolate(x32, size=(299, 299), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert (got[..., :3] - ref32).abs().max().item() <= 2e-6


def test_softmax_rows(gpu):
    from speech_to_image_translation_without_text_amd import _lib
    x = torch.randn(37, 1000, generator=torch.Generator().manual_seed(2)) * 6
    y = torch.empty(37, 1000, device=gpu)
    _lib.check(_lib.load().s2i_softmax_rows(_lib.ptr(x.to(gpu)), 37, 1000, 1000, _lib.ptr(y), 1000, _lib.stream()),
               "s2i_softmax_rows")
    ref = torch.softmax(x.double(), 1)
    assert (y.cpu().double() - ref).abs().max().item() <= 1e-6


# ---- the whole network against a float64 restatement of torchvision's Inception3 (eval) --------------------------------
def _bc(sd, name, x, stride=1, padding=0):
    x = F.conv2d(x, sd[name + ".conv.weight"], None, stride, padding)
    x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"],
                     sd[name + ".bn.bias"], False, 0.0, 0.001)
    return F.relu(x)


def reference_inception(sd, img):
    """INCEPTION_V3.forward (model.py:91-109) with MY_Inception3.forward (model.py:19-77), eval, float64."""
    sd = {k: v.double() for k, v in sd.items()}
    x = reference_prep(img)
    x = _bc(sd, "Conv2d_1a_3x3", x, 2)
    x = _bc(sd, "Conv2d_2a_3x3", x)
    x = _bc(sd, "Conv2d_2b_3x3", x, 1, 1)
    x = F.max_pool2d(x, 3, 2)
    x = _bc(sd, "Conv2d_3b_1x1", x)
    x = _bc(sd, "Conv2d_4a_3x3", x)
    x = F.max_pool2d(x, 3, 2)
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        b1 = _bc(sd, n + ".branch1x1", x)
        b5 = _bc(sd, n + ".branch5x5_2", _bc(sd, n + ".branch5x5_1", x), 1, 2)
        b3 = _bc(sd, n + ".branch3x3dbl_1", x)
        b3 = _bc(sd, n + ".branch3x3dbl_3", _bc(sd, n + ".branch3x3dbl_2", b3, 1, 1), 1, 1)
        bp = _bc(sd, n + ".branch_pool", F.avg_pool2d(x, 3, 1, 1))
        x = torch.cat([b1, b5, b3, bp], 1)
    n = "Mixed_6a"
    b3 = _bc(sd, n + ".branch3x3", x, 2)
    bd = _bc(sd, n + ".branch3x3dbl_3", _bc(sd, n + ".branch3x3dbl_2", _bc(sd, n + ".branch3x3dbl_1", x), 1, 1), 2)
    x = torch.cat([b3, bd, F.max_pool2d(x, 3, 2)], 1)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        b1 = _bc(sd, n + ".branch1x1", x)
        b7 = _bc(sd, n + ".branch7x7_1", x)
        b7 = _bc(sd, n + ".branch7x7_3", _bc(sd, n + ".branch7x7_2", b7, 1, (0, 3)), 1, (3, 0))
        bd = _bc(sd, n + ".branch7x7dbl_1", x)
        for i, p in ((2, (3, 0)), (3, (0, 3)), (4, (3, 0)), (5, (0, 3))):
            bd = _bc(sd, n + ".branch7x7dbl_%d" % i, bd, 1, p)
        bp = _bc(sd, n + ".branch_pool", F.avg_pool2d(x, 3, 1, 1))
        x = torch.cat([b1, b7, bd, bp], 1)
    n = "Mixed_7a"
    b3 = _bc(sd, n + ".branch3x3_2", _bc(sd, n + ".branch3x3_1", x), 2)
    b7 = _bc(sd, n + ".branch7x7x3_1", x)
    b7 = _bc(sd, n + ".branch7x7x3_3", _bc(sd, n + ".branch7x7x3_2", b7, 1, (0, 3)), 1, (3, 0))
    b7 = _bc(sd, n + ".branch7x7x3_4", b7, 2)
    x = torch.cat([b3, b7, F.max_pool2d(x, 3, 2)], 1)
    for n in ("Mixed_7b", "Mixed_7c"):
        b1 = _bc(sd, n + ".branch1x1", x)
        b3 = _bc(sd, n + ".branch3x3_1", x)
        b3 = torch.cat([_bc(sd, n + ".branch3x3_2a", b3, 1, (0, 1)), _bc(sd, n + ".branch3x3_2b", b3, 1, (1, 0))], 1)
        bd = _bc(sd, n + ".branch3x3dbl_2", _bc(sd, n + ".branch3x3dbl_1", x), 1, 1)
        bd = torch.cat([_bc(sd, n + ".branch3x3dbl_3a", bd, 1, (0, 1)), _bc(sd, n + ".branch3x3dbl_3b", bd, 1, (1, 0))], 1)
        bp = _bc(sd, n + ".branch_pool", F.avg_pool2d(x, 3, 1, 1))
        x = torch.cat([b1, b3, bd, bp], 1)
    pool3 = F.avg_pool2d(x, 8).reshape(x.shape[0], -1)
    logits = F.linear(pool3, sd["fc.weight"], sd["fc.bias"])
    return torch.softmax(logits, 1), pool3


def seeded_weights():
    sd = random_state_dict(seed=5)
    sd["fc.weight"] = sd["fc.weight"] * 3.0      # peakier class posteriors than a He-scaled fc gives
    return sd


def test_whole_network_against_float64(gpu):
    from speech_to_image_translation_without_text_amd import model
    sd = seeded_weights()
    img = torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(8)) * 2 - 1
    ref_soft, ref_pool = reference_inception(sd, img)
    net = model.INCEPTION_V3(weights=sd)
    soft, pool3 = net(img.to(gpu))
    soft, pool3 = soft.cpu().double(), pool3.cpu().double()
    e_soft = (soft - ref_soft).abs().max().item()
    e_pool = ((pool3 - ref_pool).abs().max() / ref_pool.abs().max()).item()
    print("softmax max |err| %.3g (max p %.3g), pool3 max rel err %.3g" % (e_soft, ref_soft.max().item(), e_pool))
    assert e_soft <= 8e-8 and e_pool <= 1.4e-6        # 2x the measured 4.1e-8 / 7.0e-7
    # two image tensors scored as one stacked batch give the same rows
    s2, p2 = net(img[:1].to(gpu), img[1:].to(gpu))
    assert torch.equal(s2.cpu().double(), soft) and torch.equal(p2.cpu().double(), pool3)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "replay"])
def test_training_collects_rows_and_scores_a_snapshot(gpu, tmp_path, graphed):
    from speech_to_image_translation_without_text_amd import model, trainer as T
    case = dict(CASES["small3"], B=4)
    netG, netsD = build_nets(case)
    netG.to(gpu)
    for d in netsD:
        d.to(gpu)
    batch = make_batch(case)
    tr = T.condGANTrainer(str(tmp_path), None, 256, False)
    tr.build(netG, netsD)
    sd = random_state_dict(seed=6)
    sd["fc.weight"] = sd["fc.weight"] * 0.01         # no posterior underflows to 0 (log(0) makes the score nan)
    incep = model.INCEPTION_V3(weights=sd)
    tr.enable_inception(incep)
    tr.inception_min_batches = 3
    if graphed:
        tr.enable_graph(warmup=1)
    gen = torch.Generator(device=gpu).manual_seed(3)
    for it in range(3):
        noise = torch.randn(case['B'], case['z'], device=gpu, generator=gen)
        eps = torch.randn(case['B'], case['ef'], device=gpu, generator=gen)
        real = [torch.rand(case['B'], 3, 64 << i, 64 << i, device=gpu, generator=gen) * 2 - 1 for i in range(3)]
        wrong = [t.to(gpu) for t in batch['wrong']]
        emb = batch['emb'].to(gpu)
        tr.train_step(real, wrong, emb, batch['labels'], noise, eps)
        b, soft, pool3 = tr._inception_rows[-1]
        s_ref, p_ref = incep(tr.fake_imgs[-1], real[-1])
        assert b == case['B'] and torch.equal(soft, s_ref) and torch.equal(pool3, p_ref), "step %d" % it
    pg, pr, ag, ar = tr.inception_arrays()
    assert pg.shape == (12, 1000) and ar.shape == (12, 2048)
    rec = tr.score_inception(3)
    assert tr._inception_rows == []
    logged = [json.loads(line) for line in open(tmp_path / "Log" / "metrics.jsonl")]
    assert logged == [rec] and all(np.isfinite(v) for v in rec.values())
    np.testing.assert_allclose([rec["inception_mean"], rec["inception_std"]], T.compute_inception_score(pg, 10),
                               rtol=1e-12)
    np.testing.assert_allclose([rec["nlpp_mean"], rec["nlpp_std"]], T.negative_log_posterior_probability(pg, 10),
                               rtol=1e-12)
    np.testing.assert_allclose(rec["fid"], T.compute_frethet_distance(ag, ar)[0], rtol=1e-12)
    assert rec["images"] == 12 and rec["batches"] == 3
