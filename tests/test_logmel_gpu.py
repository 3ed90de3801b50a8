"""Speech front end on the MI355X: audio.log_mel (s2i_signal_mean / s2i_logmel_power / s2i_logmel_finish) against the
float64 restatement (logmel_ref.py), then WAV files -> extractor pickles -> speech-to-image PNGs end to end.

Mel power is checked element by element as |P - P64| <= GAMMA * A with A = (sum_n |w_n yhat_n|)^2 * sum_k M[m, k], the
magnitude bound of the frame's fp32 DFT and projection.  GAMMA is about twice the worst ratio measured over every case
here; each case must also FAIL that check against a reference that is wrong in one way (periodic window, zero padding,
pre-emphasis after padding, HTK mel scale, max over the kept frames only)."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import logmel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 8e-7      # worst measured: 3.6e-7 (chirp)
SR = 16000


def _cases():
    rng = np.random.default_rng(2024)
    t = np.arange(3 * SR) / SR
    noise = (rng.standard_normal(3 * SR) * np.exp(-((t - 1.2) / 0.5) ** 2) * 0.4).astype(np.float32)
    chirp = (0.5 * np.sin(2 * np.pi * (100 * t + 0.5 * 2500 * t ** 2))).astype(np.float32)
    tone = (0.7 * np.cos(2 * np.pi * 40 * np.arange(2 * SR) / 400.0)).astype(np.float32)   # exactly on bin 40
    long = (0.01 * rng.standard_normal(2100 * 160 + 77)).astype(np.float32)                  # 2101 frames
    long[2060 * 160:2070 * 160] += (0.9 * np.sin(2 * np.pi * 1000 * np.arange(1600) / SR)).astype(np.float32)
    return {
        "noise": noise, "chirp": chirp, "tone": tone, "zeros": np.zeros(SR, np.float32),
        "empty": np.zeros(0, np.float32), "one": np.array([0.3], np.float32),
        "n150": (0.2 * rng.standard_normal(150)).astype(np.float32),
        "n399": (0.2 * rng.standard_normal(399)).astype(np.float32), "long": long,
    }


VARIANTS = ["periodic_window", "zero_pad", "preemph_after_pad", "htk"]


def _check_power(name, y, P, ref_got, T=2048):
    """returns the worst |P - P64| / A over the kept frames and the max"""
    P64, A = R.mel_power(y)
    keep = min(P64.shape[0], T)
    err = np.abs(P[:keep] - P64[:keep])
    ratio = float((err / np.maximum(A[:keep], 1e-300)).max()) if A.max() > 0 else float(err.max())
    assert np.all(err <= GAMMA * A[:keep]), "%s: mel power off by %.3g x A" % (name, ratio)
    ref64 = P64.max()
    assert abs(ref_got - ref64) <= GAMMA * A.max(), "%s: max %.9g vs %.9g" % (name, ref_got, ref64)
    return ratio, P64, A, keep


@pytest.fixture(scope="module")
def batch(gpu):
    from speech_to_image_translation_without_text_amd import audio
    cases = _cases()
    names = list(cases)
    out, nf, P, ref = audio.log_mel([cases[n] for n in names], return_power=True)
    nhwc, nf2 = audio.log_mel([cases[n] for n in names], layout="nhwc")
    torch.cuda.synchronize()
    return cases, names, out.cpu().numpy(), nf, P.cpu().numpy(), ref.cpu().numpy(), nhwc.cpu().numpy(), nf2


@pytest.mark.gpu
def test_logmel_power_matches_float64(batch):
    cases, names, out, nf, P, ref, _, _ = batch
    worst = {}
    for i, n in enumerate(names):
        worst[n], P64, A, keep = _check_power(n, cases[n], P[i], ref[i])
        if not P64.any():
            continue                                   # all-zero signals: every variant is zero too
        for v in VARIANTS:
            Pv, _ = R.mel_power(cases[n], variant=v)
            assert np.any(np.abs(P[i][:keep] - Pv[:keep]) > GAMMA * A[:keep]), "%s passes against %s" % (n, v)
    print("worst |P - P64| / A per case:", {k: "%.3g" % v for k, v in worst.items()})


@pytest.mark.gpu
def test_logmel_db_and_fill(batch):
    from speech_to_image_translation_without_text_amd import audio
    cases, names, out, nf, P, ref, nhwc, nf2 = batch
    assert (nf == nf2).all()
    for i, n in enumerate(names):
        y = cases[n]
        want, keep, ref64 = R.log_mel(y)
        assert nf[i] == keep == audio.n_frames(len(y))
        np.testing.assert_array_equal(nhwc[i, 0], out[i].T)
        assert not out[i][:, keep:].any(), "%s: frames past n_frames must be 0 dB" % n
        P64, A = R.mel_power(y)
        if not P64.any():
            assert not out[i].any(), "%s: silence must be 0 dB everywhere" % n
            continue
        # dB error from the power bound: 10/ln10 * (dP/P + dref/ref), used where P64 is well above its bound
        p, a = P64[:keep].T, A[:keep].T
        amax = A.max()
        ok = p >= 100 * GAMMA * a
        bound = 4.343 * 1.02 * (GAMMA * a / np.maximum(p, 1e-300) + GAMMA * amax / ref64) + 2e-4
        got = out[i][:, :keep]
        assert np.all(np.abs(got - want[:, :keep])[ok] <= bound[ok]), n
        assert (got >= -80.0).all() and got.max() <= 1e-3
    # the long clip's loudest burst is after frame 2048: a max over the kept frames only is a different array
    i = names.index("long")
    wrong, _, _ = R.log_mel(cases["long"], variant="max_kept_frames")
    assert np.abs(out[i] - wrong).max() > 1.0


@pytest.mark.gpu
def test_logmel_ragged_batch_of_240(gpu):
    from speech_to_image_translation_without_text_amd import audio
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 4 * SR, 240)
    lens[:3] = [1, 160, 64 * 160 - 1]
    clips = [(0.3 * rng.standard_normal(n) * np.sin(np.linspace(0, 7, n)) ** 2).astype(np.float32) for n in lens]
    _, nf, P, ref = audio.log_mel(clips, return_power=True)
    P, ref = P.cpu().numpy(), ref.cpu().numpy()
    worst = 0.0
    for i in range(0, 240, 7):
        r, _, _, _ = _check_power("item %d" % i, clips[i], P[i], ref[i])
        worst = max(worst, r)
    print("ragged worst ratio %.3g" % worst)


# ---- end to end -----------------------------------------------------------------------------------------------------
def _write_wav(path, y):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(SR)
        f.writeframes(np.clip(np.round(y * 32768), -32768, 32767).astype("<i2").tobytes())


def _encoder_net():
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    torch.manual_seed(0)
    net = CNNRNN(40, embedding_dim=1024, nhidden=1024, nsent=1024, bidirectional=True, rnn_layers=1)
    g = torch.Generator().manual_seed(5)
    for k, v in net.state_dict().items():
        if k.endswith('running_mean'):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith('running_var'):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
    return net.eval()


@pytest.fixture(scope="module")
def corpus(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("speech")
    wav = d / "wavs"
    wav.mkdir()
    rng = np.random.default_rng(7)
    items = []
    for k in range(2):
        names = []
        for j in range(10):
            n = int(rng.integers(1 * SR, 5 * SR)) if (k, j) != (1, 4) else 40 * 160      # one item under 64 frames
            t = np.arange(n) / SR
            y = 0.3 * np.sin(2 * np.pi * (150 + 60 * j) * t * (1 + 0.2 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * t))
            y = y + 0.02 * rng.standard_normal(n)
            name = "s%d_%d.wav" % (k, j)
            _write_wav(wav / name, y)
            names.append(name)
        items.append({"audio": names})
    (d / "test.json").write_text(json.dumps({"audio_base_path": str(wav), "data": items}))
    net = _encoder_net()
    torch.save({"meta": {}, "state_dict": {"module." + k: v for k, v in net.state_dict().items()}}, d / "enc.pt")
    r = subprocess.run([sys.executable, "-m", "speech_to_image_translation_without_text_amd.extract_audio_feature",
                        "--model", str(d / "enc.pt"), "--audio_switch", "3", "--dataset", "birds", "--bidirectional",
                        "--data_dir", str(d), "--splits", "test", "--batch_size", "240"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = [str(wav / n) for it in items for n in it["audio"]]
    return d, files, net


@pytest.mark.gpu
def test_extractor_matches_cpu_chain(corpus):
    from oracle import speech_encoder_oracle as orc
    from speech_to_image_translation_without_text_amd import audio, datasets
    d, files, net = corpus
    feats = datasets.load_embedding_pickle(str(d / "test" / "audio_features_3.pickle"))
    lens = datasets.load_embedding_pickle(str(d / "test" / "audio_features_lens_3.pickle"))
    assert feats.shape == (2, 10, 1024) and feats.dtype == np.float32 and lens.shape == (2, 10)
    p = {k: v.clone() for k, v in net.state_dict().items()}
    want = []
    for s in range(0, 20, 10):
        specs, nfs = [], []
        for f in files[s:s + 10]:
            spec, nf, _ = R.log_mel(audio.read_wav(f))
            specs.append(spec.astype(np.float32))
            nfs.append(nf)
        order = sorted(range(10), key=lambda i: -nfs[i])
        if nfs[order[-1]] < 64:
            specs[order[-1]], nfs[order[-1]] = specs[order[-2]], nfs[order[-2]]
        order = sorted(range(10), key=lambda i: -nfs[i])
        x = torch.from_numpy(np.stack([specs[i] for i in order]))
        with torch.no_grad():
            _, sent = orc.forward(p, x, torch.tensor([nfs[i] // 64 for i in order]), 512, True)
        chunk = np.empty((10, 1024), np.float32)
        chunk[order] = sent.numpy()
        want.append(chunk)
        np.testing.assert_array_equal(lens[s // 10], [audio.n_frames(len(audio.read_wav(f))) for f in files[s:s + 10]])
    want = np.stack(want)
    err = np.abs(feats - want)
    print("extractor vs CPU chain: max |diff| %.3g (max |emb| %.3g)" % (err.max(), np.abs(want).max()))
    np.testing.assert_allclose(feats, want, rtol=2e-3, atol=2e-4)


@pytest.mark.gpu
def test_extractor_batch_sizes_agree(corpus):
    from speech_to_image_translation_without_text_amd import datasets, extract_audio_feature as E
    d, files, net = corpus
    model = E.load_encoder(str(d / "enc.pt"), bidirectional=True, device=torch.device("cuda:0"))
    feats10, _ = E.encode_waveforms(model, E.read_wavs(files), batch_size=10)
    feats240 = datasets.load_embedding_pickle(str(d / "test" / "audio_features_3.pickle")).reshape(20, 1024)
    np.testing.assert_allclose(feats10, feats240, rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_speech_to_image_entry_point(corpus, tmp_path):
    from PIL import Image

    from speech_to_image_translation_without_text_amd import extract_audio_feature as E
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd import speech_to_image as S
    from speech_to_image_translation_without_text_amd.model import G_NET
    from speech_to_image_translation_without_text_amd.trainer import weights_init
    from speech_to_image_translation_without_text_amd.miscc.config import cfg_from_file, cfg_reset
    d, files, _ = corpus
    # G's widths come from the config: the child gets them through --cfg, this process from the same file
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
        wavs = [files[0], files[13]]
        r = subprocess.run([sys.executable, "-m", "speech_to_image_translation_without_text_amd.speech_to_image",
                            "--model", str(d / "enc.pt"), "--netG", str(tmp_path / "netG_7.pth"), "--out_dir",
                            str(tmp_path / "png"), "--cfg", str(yml), "--bidirectional", "--seed", "5"] + wavs,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        dev = torch.device("cuda:0")
        model = E.load_encoder(str(d / "enc.pt"), bidirectional=True, device=dev)
        emb = S.embed(model, E.read_wavs(wavs))
        netG = netG.to(dev).eval()
        z, eps = S.draw_noise(2, 5)
        with torch.no_grad():
            imgs, _, _ = netG(z.to(dev), emb, eps.to(dev), True)
        want = ops.images_to_uint8_hwc(imgs[-1]).cpu().numpy()
    finally:
        cfg_reset()
    assert want.shape == (2, 128, 128, 3)
    for w, img in zip(wavs, want):
        got = np.asarray(Image.open(tmp_path / "png" / (os.path.splitext(os.path.basename(w))[0] + ".png")))
        assert got.shape == img.shape
        assert np.abs(got.astype(int) - img.astype(int)).max() <= 1
