"""Speech front end on the CPU: the float64 restatement (logmel_ref.py) against torch.stft and hand-derived mel anchors,
the package's fp32 constants, read_wav, the extraction bookkeeping and the C-ABI's argument checks."""
import os
import pickle
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import logmel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clip(n, seed):
    return np.random.default_rng(seed).standard_normal(n) * np.hanning(n) * 0.3 if n else np.zeros(0)


@pytest.mark.parametrize("n", [201, 399, 400, 1000, 16000 + 37])
def test_restatement_matches_torch_stft(n):
    y = torch.from_numpy(_clip(n, n))
    yc = y - y.mean()
    yp = torch.cat([yc[:1], yc[1:] - 0.97 * yc[:-1]])
    st = torch.stft(yp, 400, hop_length=160, win_length=400, window=torch.hamming_window(400, periodic=False,
                                                                                         dtype=torch.float64),
                    center=True, pad_mode="reflect", return_complex=True)
    ref, _ = R.stft_power(y.numpy())
    got = (st.abs() ** 2).numpy().T
    assert got.shape == ref.shape == (1 + n // 160, 201)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * ref.max())


@pytest.mark.parametrize("n", [1, 2, 3, 150, 200])
def test_restatement_short_clips_use_repeated_reflection(n):
    y = _clip(n, 7) + 0.1
    yc = y - y.mean()
    yp = R.preemphasis(yc)
    padded = np.pad(yp, 200, "reflect")
    nf = 1 + n // 160
    fr = np.stack([padded[f * 160:f * 160 + 400] for f in range(nf)])
    want = np.abs(np.fft.rfft(fr * R.window()[None, :], axis=1)) ** 2
    got, _ = R.stft_power(y)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)


def test_mel_scale_anchors():
    assert R.hz_to_mel(1000.0) == pytest.approx(15.0, abs=1e-12)
    assert R.hz_to_mel(20.0) == pytest.approx(0.3, abs=1e-12)
    assert R.mel_to_hz(R.hz_to_mel(3456.0)) == pytest.approx(3456.0, rel=1e-12)
    f = R.mel_edges()
    assert len(f) == 42
    assert f[0] == pytest.approx(20.0, rel=1e-12) and f[-1] == pytest.approx(8000.0, rel=1e-12)
    M = R.mel_bank()
    fft_f = np.linspace(0, 8000, 201)
    # first triangle starts above 20 Hz (bin 1 = 40 Hz), the last reaches the Nyquist bin's neighbourhood
    assert np.nonzero(M[0])[0][0] == 1
    assert np.nonzero(M[-1])[0][-1] == 199
    assert (M.sum(axis=1) > 0).all(), "empty filter"
    for i in range(40):
        nz = np.nonzero(M[i])[0]
        assert (np.diff(nz) == 1).all(), "filter %d is not one contiguous bin range" % i
        # analytically at its centre f[i+1] a filter is 1 before normalisation: 2 / (f[i+2] - f[i]) after
        tri = lambda x: max(0.0, min((x - f[i]) / (f[i + 1] - f[i]), (f[i + 2] - x) / (f[i + 2] - f[i + 1])))
        assert tri(f[i + 1]) * 2.0 / (f[i + 2] - f[i]) == pytest.approx(2.0 / (f[i + 2] - f[i]), rel=1e-15)
        # and the stored row is that triangle (fp32) at the bin frequencies
        want = np.array([tri(x) for x in fft_f]) * 2.0 / (f[i + 2] - f[i])
        np.testing.assert_allclose(M[i], want, rtol=2e-7, atol=1e-12)


def test_package_constants_equal_restatement_in_fp32():
    from speech_to_image_translation_without_text_amd import audio as A
    np.testing.assert_array_equal(A.mel_filterbank(), R.mel_bank().astype(np.float32))
    rng = A.mel_ranges(A.mel_filterbank())
    for i, (lo, hi) in enumerate(rng):
        nz = np.nonzero(R.mel_bank()[i])[0]
        assert (lo, hi) == (nz[0], nz[-1] + 1)
    ref = R.dft_basis().astype(np.float32)                      # [400][201 cos | 201 sin]
    flat = A.pack_basis(A.dft_basis64().astype(np.float32))
    B = A.unpack_basis(flat)
    for q in range(200):
        t, c = divmod(q, 16)
        np.testing.assert_array_equal(B[:, 32 * t + c], ref[:, q])
        np.testing.assert_array_equal(B[:, 32 * t + 16 + c], ref[:, 200] if q == 0 else ref[:, 201 + q])
    for q in range(200, 208):
        t, c = divmod(q, 16)
        assert not B[:, 32 * t + c].any() and not B[:, 32 * t + 16 + c].any()
    # the header's element formula
    n, nt, c = 123, 17, 9
    assert flat[((n // 16 * 26 + nt) * 64 + (n % 4) * 16 + c) * 4 + (n % 16) // 4] == B[n, 16 * nt + c]


def _write_wav(path, data, rate=16000, width=2, channels=1):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(np.asarray(data).astype("<i%d" % width).tobytes())


def test_read_wav_pcm16(tmp_path):
    from speech_to_image_translation_without_text_amd.audio import read_wav
    d = np.array([-32768, -1, 0, 1, 32767, 1234], dtype=np.int16)
    _write_wav(tmp_path / "m.wav", d)
    y = read_wav(tmp_path / "m.wav")
    assert y.dtype == np.float32
    np.testing.assert_array_equal(y, d.astype(np.float32) / 32768.0)
    assert y[0] == -1.0
    st = np.array([[-32768, 32767], [100, -300], [5, 6]], dtype=np.int16)
    _write_wav(tmp_path / "s.wav", st.reshape(-1), channels=2)
    np.testing.assert_array_equal(read_wav(tmp_path / "s.wav"),
                                  (st.astype(np.float32) / 32768.0).mean(axis=1, dtype=np.float32))
    _write_wav(tmp_path / "e.wav", np.zeros(0, np.int16))
    assert read_wav(tmp_path / "e.wav").size == 0


def test_read_wav_refuses_other_formats(tmp_path):
    from speech_to_image_translation_without_text_amd.audio import read_wav
    _write_wav(tmp_path / "r.wav", np.zeros(10, np.int16), rate=22050)
    with pytest.raises(ValueError, match="22050"):
        read_wav(tmp_path / "r.wav")
    _write_wav(tmp_path / "w.wav", np.zeros(10, np.int32), width=4)
    with pytest.raises(ValueError, match="32-bit"):
        read_wav(tmp_path / "w.wav")
    with wave.open(str(tmp_path / "b.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(1)
        f.setframerate(16000)
        f.writeframes(bytes(10))
    with pytest.raises(ValueError, match="8-bit"):
        read_wav(tmp_path / "b.wav")


def test_n_frames_rule():
    from speech_to_image_translation_without_text_amd.audio import n_frames
    assert n_frames(0) == 2 and n_frames(1) == 1 and n_frames(159) == 1 and n_frames(160) == 2
    assert n_frames(16000 * 30) == 2048 and n_frames(160 * 2047) == 2048


# ---- extraction bookkeeping -----------------------------------------------------------------------------------------
class _StubEncoder(torch.nn.Module):
    """records forward_nhwc inputs; the embedding of an item is (its log-mel marker, its cap_len) broadcast"""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward_nhwc(self, x, cap_lens):
        self.calls.append((x.clone(), list(cap_lens)))
        assert list(cap_lens) == sorted(cap_lens, reverse=True)
        marker = x[:, 0, 0, 0]
        sent = torch.stack([marker, torch.tensor(cap_lens, dtype=torch.float32)], 1).repeat(1, 4)
        return None, sent


def _fake_log_mel(waves, layout="nhwc", device=None, **_):
    from speech_to_image_translation_without_text_amd.audio import n_frames
    nf = np.array([n_frames(len(w)) for w in waves], dtype=np.int64)
    x = torch.zeros(len(waves), 1, 4, 40)
    for i, w in enumerate(waves):
        x[i, 0, 0, 0] = float(w[0]) if len(w) else -1.0   # a test clip carries its id in its first sample
    return x, nf


def _reference_chunks(frames, ids):
    """extract_one_feature (extract_audio_feature.py:25-54) per chunk of 10, written out"""
    feats = []
    for s in range(0, len(frames), 10):
        fr = torch.tensor(frames[s:s + 10])
        sl, si = torch.sort(fr, stable=True, dim=0, descending=True)
        data = torch.tensor(ids[s:s + 10], dtype=torch.float32)[si]
        sl = sl.clone()
        if sl[-1] < 64:
            sl[-1] = sl[-2]
            data[-1] = data[-2]
        cap = sl // 64
        rec = torch.empty_like(si)
        rec[si] = torch.arange(len(si))
        feats.append(torch.stack([data, cap.float()], 1).repeat(1, 4)[rec])
    return torch.cat(feats).numpy()


@pytest.mark.parametrize("batch_size", [1, 7, 10, 25, 240])
def test_encode_waveforms_matches_chunk_of_ten_rule(monkeypatch, batch_size):
    from speech_to_image_translation_without_text_amd import audio, extract_audio_feature as E
    rng = np.random.default_rng(3)
    lengths = rng.integers(64 * 160, 600 * 160, 40)
    lengths[[3, 17, 18, 29]] = [5 * 160, 63 * 160, 10, 0]      # too short: alone, and two in one chunk; one empty
    ids = np.arange(1, 41, dtype=np.float32)
    waves = [np.full(int(n), i, dtype=np.float32) for n, i in zip(lengths, ids)]
    ids[29] = -1.0
    monkeypatch.setattr(audio, "log_mel", _fake_log_mel)
    enc = _StubEncoder()
    frames = np.array([audio.n_frames(n) for n in lengths])
    feats, got_frames = E.encode_waveforms(enc, waves, batch_size=batch_size)
    np.testing.assert_array_equal(got_frames, frames)
    np.testing.assert_array_equal(feats, _reference_chunks(frames, ids))
    assert sum(len(c[1]) for c in enc.calls) == 40


def test_chunk_sources_single_short_item_is_refused():
    from speech_to_image_translation_without_text_amd.extract_audio_feature import chunk_sources
    assert chunk_sources([100, 80, 30]).tolist() == [0, 1, 1]
    with pytest.raises(ValueError):
        chunk_sources([100] * 10 + [5])


def test_extract_split_writes_loadable_pickles(monkeypatch, tmp_path):
    import json
    from speech_to_image_translation_without_text_amd import datasets, extract_audio_feature as E
    wav_dir = tmp_path / "wavs"
    wav_dir.mkdir()
    items = []
    for k in range(2):
        names = []
        for j in range(10):
            name = "c%d_%d.wav" % (k, j)
            _write_wav(wav_dir / name, np.full(160 * (70 + 10 * j + k), 10 * k + j + 1, np.int16))
            names.append(name)
        items.append({"audio": names})
    (tmp_path / "test.json").write_text(json.dumps({"audio_base_path": str(wav_dir), "data": items}))
    monkeypatch.setattr(E.audio, "log_mel", lambda ws, **kw: (_fake_log_mel(ws)[0] * 32768.0, _fake_log_mel(ws)[1]))
    E.extract_split(_StubEncoder(), str(tmp_path), "test", "birds", "7", batch_size=6)
    f = datasets.load_embedding_pickle(str(tmp_path / "test" / "audio_features_7.pickle"))
    lens = datasets.load_embedding_pickle(str(tmp_path / "test" / "audio_features_lens_7.pickle"))
    assert f.shape == (2, 10, 8) and f.dtype == np.float32
    assert lens.shape == (2, 10) and lens.dtype == np.int64
    assert lens[1, 3] == 1 + 160 * (70 + 30 + 1) // 160
    np.testing.assert_array_equal(np.rint(f[:, :, 0]), np.arange(1, 21).reshape(2, 10))
    with open(tmp_path / "test" / "audio_features_7.pickle", "rb") as fp:
        assert isinstance(pickle.load(fp), np.ndarray)


def _save_encoder(tmp_path, wrap, prefix):
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    torch.manual_seed(0)
    net = CNNRNN(40, embedding_dim=1024, nhidden=1024, nsent=1024, bidirectional=True)
    sd = {(prefix + k): v for k, v in net.state_dict().items()}
    path = tmp_path / ("enc_%s_%s.pt" % (wrap, bool(prefix)))
    torch.save({"meta": {"epoch": 3}, "state_dict": sd} if wrap else sd, path)
    return net, path


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("prefix", ["", "module."])
def test_load_encoder_checkpoint_forms(tmp_path, wrap, prefix):
    from speech_to_image_translation_without_text_amd.extract_audio_feature import load_encoder
    net, path = _save_encoder(tmp_path, wrap, prefix)
    got = load_encoder(str(path), bidirectional=True)
    assert not got.training
    for k, v in net.state_dict().items():
        assert torch.equal(got.state_dict()[k], v)


def test_load_encoder_refuses_foreign_checkpoint(tmp_path):
    from speech_to_image_translation_without_text_amd.extract_audio_feature import load_encoder
    torch.save({"epoch": 3, "optimizer": "x"}, tmp_path / "bad.pt")
    with pytest.raises(Exception):
        load_encoder(str(tmp_path / "bad.pt"))


def test_entry_points_return_errors_without_a_device():
    """bad arguments come back as an error code and text before anything touches a device (run in a child so no HIP
    context is needed)"""
    code = r'''
import ctypes, sys
sys.path.insert(0, %r)
from speech_to_image_translation_without_text_amd import _lib
lib = _lib.load()
P = 4096
assert lib.s2i_logmel_basis_elems() == 400 * 416
assert lib.s2i_signal_mean(None, P, P, 1, P, P, None) != 0 and b"null" in lib.s2i_last_error()
assert lib.s2i_signal_mean(P, P, P, 0, P, P, None) != 0 and b"count" in lib.s2i_last_error()
args = [P, P, P, 2, P, P, P, P, P, 3, 2048, P, P, None]   # only ever passed with one argument broken
bad = list(args); bad[5] = 4100
assert lib.s2i_logmel_power(*bad) != 0 and b"aligned" in lib.s2i_last_error()
bad = list(args); bad[9] = 0
assert lib.s2i_logmel_power(*bad) != 0 and b"tile" in lib.s2i_last_error()
bad = list(args); bad[10] = 0
assert lib.s2i_logmel_power(*bad) != 0 and b"target" in lib.s2i_last_error()
bad = list(args); bad[0] = None
assert lib.s2i_logmel_power(*bad) != 0 and b"null" in lib.s2i_last_error()
assert lib.s2i_logmel_finish(P, P, P, 2, 2048, 5, P, None) != 0 and b"layout" in lib.s2i_last_error()
assert lib.s2i_logmel_finish(P, P, P, 0, 2048, 0, P, None) != 0 and b"shape" in lib.s2i_last_error()
assert lib.s2i_logmel_finish(None, P, P, 2, 2048, 0, P, None) != 0
print("ok")
''' % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
