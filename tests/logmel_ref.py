"""Float64 numpy restatement of the reference's log-mel (Audio_to_Image/utils.py:292-340 with librosa < 0.10) --
TEST INFRASTRUCTURE ONLY, like launch_ref.py.  librosa is not available, so each step is written out:

  1. y (float mono; an empty clip becomes 200 zeros)   2. y - mean, pre-emphasis 0.97 (utils.py:282-289)
  3. np.pad(y', 200, 'reflect'), frames of 400 every 160, symmetric Hamming window, rfft     4. |.|^2, Slaney mel bank
  5. power_to_db(ref=max over ALL frames, amin=1e-10, top_db=80)                            6. 0 dB fill / cut to T

The keyword `variant` switches on one deliberate deviation, so tests can show their tolerance rejects it:
"periodic_window", "zero_pad", "preemph_after_pad", "htk", "max_kept_frames".
"""
import numpy as np

SR, N_FFT, HOP, N_MELS, FMIN, TARGET = 16000, 400, 160, 40, 20.0, 2048
N_BINS = N_FFT // 2 + 1


def hz_to_mel(f, htk=False):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    mels = f / f_sp
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, mels)


def mel_to_hz(m, htk=False):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_edges(htk=False):
    """the 42 edge frequencies f[0..41] (Hz)"""
    return mel_to_hz(np.linspace(hz_to_mel(FMIN, htk), hz_to_mel(SR / 2.0, htk), N_MELS + 2), htk)


def mel_bank(htk=False):
    """librosa.filters.mel(16000, 400, n_mels=40, fmin=20) as stored (float32 triangles, then the in-place area
    normalisation), returned as float64 values of those float32 numbers."""
    fft_f = np.linspace(0.0, SR / 2.0, N_BINS)
    f = mel_edges(htk)
    fdiff = np.diff(f)
    ramps = np.subtract.outer(f, fft_f)
    w = np.zeros((N_MELS, N_BINS), dtype=np.float32)
    for i in range(N_MELS):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (f[2:N_MELS + 2] - f[:N_MELS]))[:, None]
    return w.astype(np.float64)


def window(periodic=False):
    n = np.arange(N_FFT, dtype=np.float64)
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * n / (N_FFT if periodic else N_FFT - 1))


def dft_basis(periodic=False):
    """[400 samples][201 cos + 201 sin] float64: w_n cos(2 pi n k / 400), -w_n sin(2 pi n k / 400)."""
    n = np.arange(N_FFT)[:, None]
    k = np.arange(N_BINS)[None, :]
    ang = 2.0 * np.pi * ((n * k) % N_FFT) / N_FFT
    w = window(periodic)[:, None]
    return np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1)


def preemphasis(y, coeff=0.97):
    return np.append(y[0], y[1:] - coeff * y[:-1])


def frames_of(y, variant=None):
    """the [n_frames][400] windowed-frame input of librosa.stft(center=True) for the pre-emphasised y (or, for
    preemph_after_pad, the mean-removed y)"""
    n_frames = 1 + len(y) // HOP
    if variant == "zero_pad":
        yp = np.pad(y, N_FFT // 2, mode="constant")
    else:
        yp = np.pad(y, N_FFT // 2, mode="reflect")
    if variant == "preemph_after_pad":
        yp = preemphasis(yp)
    idx = np.arange(n_frames)[:, None] * HOP + np.arange(N_FFT)[None, :]
    return yp[idx]


def stft_power(y, variant=None):
    """(n_frames, 201) |STFT|^2 of the raw clip y, float64, plus the magnitude bound row sum_n |w_n yhat_n| per frame"""
    y = np.asarray(y, dtype=np.float64)
    if y.size == 0:
        y = np.zeros(200)
    y = y - y.mean()
    if variant != "preemph_after_pad":
        y = preemphasis(y)
    fr = frames_of(y, variant)
    w = window(variant == "periodic_window")
    spec = np.fft.rfft(fr * w[None, :], axis=1)
    return np.abs(spec) ** 2, (np.abs(fr) * np.abs(w)[None, :]).sum(axis=1)


def mel_power(y, variant=None):
    """(n_frames, 40) mel power (all frames) and the (n_frames, 40) magnitude bound A = (sum |w yhat|)^2 sum_k M[m,k]"""
    p, mag = stft_power(y, variant)
    M = mel_bank(htk=(variant == "htk"))
    return p @ M.T, (mag ** 2)[:, None] * M.sum(axis=1)[None, :]


def log_mel(y, target_length=TARGET, variant=None):
    """(logspec (40, T) float64, n_frames, ref): load_one_audio_file for one clip"""
    mel, _ = mel_power(y, variant)
    nf = mel.shape[0]
    keep = min(nf, target_length)
    if variant == "max_kept_frames":
        mel = mel[:keep]
    ref = mel.max()
    db = 10.0 * np.log10(np.maximum(1e-10, mel)) - 10.0 * np.log10(max(1e-10, ref))
    db = np.maximum(db, db.max() - 80.0)
    out = np.zeros((N_MELS, target_length))
    out[:, :keep] = db[:keep].T
    return out, keep, ref
