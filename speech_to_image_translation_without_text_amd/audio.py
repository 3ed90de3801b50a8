"""Speech front end: 16 kHz PCM16 WAV files -> the reference's log-mel arrays, on the MI355X kernels.

The reference builds the encoder's input with librosa, one file at a time on the CPU (Audio_to_Image/utils.py:292-340,
`load_one_audio_file`): load at 16 kHz, subtract the mean, pre-emphasis 0.97, librosa.stft (n_fft = win_length = 400,
hop 160, symmetric scipy Hamming window, center=True with reflect padding), |.|^2, a 40-band Slaney mel bank from 20 Hz
(librosa.filters.mel(16000, 400, n_mels=40, fmin=20)), power_to_db(ref=np.max, top_db=80), and 0 dB padding or
truncation to 2048 frames.  Here a whole ragged batch runs as three kernels (csrc/s2i_audio.hip): a per-utterance mean,
`logmel_power` (the STFT as one fp32 MFMA GEMM against a window-folded DFT basis, power, mel projection and the
per-utterance max over every frame), and `logmel_finish` (dB, floor, fill).  The basis and the mel bank are built in
float64 here, rounded to fp32 once and cached per device.

read_wav uses the stdlib `wave` module: PCM16 at 16 kHz, mono or stereo (averaged).  Other rates and sample formats are
refused (there is no resampler).
"""
import wave

import numpy as np
import torch

from . import _lib
from ._lib import LOGMEL_BFT, LOGMEL_NHWC, LOGMEL_TILE_FRAMES, check, ptr, stream

SAMPLE_RATE = 16000
N_FFT = 400
HOP = 160
N_MELS = 40
FMIN = 20.0
TARGET_LENGTH = 2048
N_BINS = N_FFT // 2 + 1
_PAIR_TILES = 13          # 16-wide tiles of (cos, sin) column pairs; 13 * 16 = 208 >= 200 pairs
_NCOLS = 2 * 16 * _PAIR_TILES
_LAYOUTS = {"bft": LOGMEL_BFT, "nhwc": LOGMEL_NHWC}


# ---- constants (float64 on the host) -------------------------------------------------------------------------------
def hz_to_mel(f):
    """Slaney mel scale (librosa htk=False): linear below 1 kHz at 200/3 Hz per mel, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def hamming_window():
    """scipy.signal.hamming(400): the symmetric window 0.54 - 0.46 cos(2 pi n / 399), float64."""
    n = np.arange(N_FFT, dtype=np.float64)
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * n / (N_FFT - 1))


def mel_filterbank():
    """librosa.filters.mel(16000, 400, n_mels=40, fmin=20) (norm=1, htk=False) as librosa stores it: the triangles are
    computed in float64 and stored into a float32 array, then scaled in place by 2 / (f[i+2] - f[i])."""
    fft_f = np.linspace(0.0, SAMPLE_RATE / 2.0, N_BINS)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(FMIN), hz_to_mel(SAMPLE_RATE / 2.0), N_MELS + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fft_f)
    weights = np.zeros((N_MELS, N_BINS), dtype=np.float32)
    for i in range(N_MELS):
        weights[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    weights *= (2.0 / (mel_f[2:N_MELS + 2] - mel_f[:N_MELS]))[:, None]
    return weights


def mel_ranges(bank):
    """[40][2] int32: each filter's nonzero bin range [lo, hi) (a triangle covers a contiguous range)."""
    out = np.zeros((bank.shape[0], 2), dtype=np.int32)
    for i, row in enumerate(bank):
        nz = np.nonzero(row)[0]
        out[i] = (nz[0], nz[-1] + 1) if len(nz) else (0, 0)
    return out


def dft_basis64():
    """[400 samples][416 columns] float64, the window folded in, in the kernel's column order: column pair q of pair
    tile t = q // 16 is (cos, sin) of bin q at columns 32 t + q % 16 and 32 t + 16 + q % 16, for q = 1..199; q = 0 pairs
    bin 0's cos with bin 200's cos (neither has a sine part); q = 200..207 are zero."""
    n = np.arange(N_FFT)
    w = hamming_window()
    out = np.zeros((N_FFT, _NCOLS), dtype=np.float64)
    for q in range(200):
        t, c = divmod(q, 16)
        ang = 2.0 * np.pi * ((n * q) % N_FFT) / N_FFT
        out[:, 32 * t + c] = w * np.cos(ang)
        if q == 0:
            out[:, 32 * t + 16 + c] = w * np.cos(2.0 * np.pi * ((n * 200) % N_FFT) / N_FFT)
        else:
            out[:, 32 * t + 16 + c] = -w * np.sin(ang)
    return out


def pack_basis(basis):
    """[400][416] -> the flat fragment order of s2i_logmel_basis_elems (include/s2i_hip.h): element (n, c of N-tile nt)
    at ((n // 16 * 26 + nt) * 64 + (n % 4) * 16 + c) * 4 + (n % 16) // 4."""
    b = np.asarray(basis).reshape(N_FFT // 16, 4, 4, 2 * _PAIR_TILES, 16)     # [kg][u][g][nt][c], n = 16 kg + 4 u + g
    return np.ascontiguousarray(b.transpose(0, 3, 2, 4, 1)).reshape(-1)      # [kg][nt][g][c][u]


def unpack_basis(flat):
    b = np.asarray(flat).reshape(N_FFT // 16, 2 * _PAIR_TILES, 4, 16, 4)     # [kg][nt][g][c][u]
    return np.ascontiguousarray(b.transpose(0, 4, 2, 1, 3)).reshape(N_FFT, _NCOLS)


_CONSTS = {}


def device_constants(device):
    """(packed fp32 basis, fp32 mel bank [40][201], int32 ranges [40][2]) on `device`, built once per device."""
    key = str(device)
    if key not in _CONSTS:
        lib = _lib.load()
        packed = pack_basis(dft_basis64().astype(np.float32))
        if packed.size != lib.s2i_logmel_basis_elems():
            raise _lib.S2IError("logmel basis has %d floats, the library expects %d" % (packed.size,
                                                                                       lib.s2i_logmel_basis_elems()))
        bank = mel_filterbank()
        _CONSTS[key] = (torch.from_numpy(packed).to(device), torch.from_numpy(bank).to(device),
                        torch.from_numpy(mel_ranges(bank)).to(device))
    return _CONSTS[key]


# ---- WAV input -----------------------------------------------------------------------------------------------------
def read_wav(path):
    """16 kHz PCM16 WAV -> float32 mono in [-1, 1) (int16 / 32768; stereo channels averaged), as librosa.load(path,
    16000) returns it for the reference's files.  Any other rate or sample format raises ValueError."""
    with wave.open(str(path), "rb") as f:
        rate, width, ch, n = f.getframerate(), f.getsampwidth(), f.getnchannels(), f.getnframes()
        if f.getcomptype() != "NONE":
            raise ValueError("%s: compressed WAV (%s) is not supported; need PCM16" % (path, f.getcomptype()))
        if width != 2:
            raise ValueError("%s: %d-bit samples; need 16-bit PCM" % (path, 8 * width))
        if rate != SAMPLE_RATE:
            raise ValueError("%s: sample rate %d Hz; need %d Hz (no resampling)" % (path, rate, SAMPLE_RATE))
        if ch not in (1, 2):
            raise ValueError("%s: %d channels; need mono or stereo" % (path, ch))
        raw = f.readframes(n)
    y = np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)
    if ch == 2:
        y = y.reshape(-1, 2).mean(axis=1, dtype=np.float32)
    return y


def n_frames(num_samples, target_length=TARGET_LENGTH):
    """Frames the reference reports for a clip of `num_samples` (an empty clip counts as 200 zeros)."""
    return min(1 + (int(num_samples) or 200) // HOP, target_length)


# ---- the batch path ------------------------------------------------------------------------------------------------
def log_mel(waveforms, target_length=TARGET_LENGTH, layout="bft", device=None, return_power=False):
    """`load_one_audio_file` for a list of 1-D float arrays or tensors (16 kHz samples), in one batch on the GPU.

    Returns (logspec, n_frames): logspec is (B, 40, T) for layout "bft" or [B, 1, T, 40] for "nhwc" (the layout
    CNNRNN.forward_nhwc takes), float32 on the device; n_frames is an int64 ndarray, capped at T.  With
    return_power=True also returns the mel power [B, T, 40] of the kept frames and each utterance's max mel power over
    all its frames (power_to_db's ref)."""
    if layout not in _LAYOUTS:
        raise ValueError("layout must be one of %s" % sorted(_LAYOUTS))
    if int(target_length) < 1:
        raise ValueError("target_length must be >= 1")
    T = int(target_length)
    _lib.load()
    _lib.require_device()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if len(waveforms) == 0:
        raise ValueError("log_mel: no waveforms")
    sigs = []
    for w in waveforms:
        t = torch.as_tensor(w).detach().reshape(-1).to(device=dev, dtype=torch.float32)
        sigs.append(t if t.numel() else torch.zeros(200, dtype=torch.float32, device=dev))
    batch = prepare_batch(sigs, T, dev)
    out = torch.empty((len(sigs), N_MELS, T) if layout == "bft" else (len(sigs), 1, T, N_MELS), dtype=torch.float32,
                      device=dev)
    launch(batch, out, layout)
    nf = 1 + batch["lens"] // HOP
    frames = np.minimum(nf, T).astype(np.int64)
    if return_power:
        return out, frames, batch["melpow"], batch["maxbits"].view(torch.float32)
    return out, frames


def prepare_batch(sigs, T, dev):
    """device buffers of one ragged batch of non-empty fp32 device signals: the flat samples, int64 offsets, int32
    lengths, the tile table (one (b, first frame) entry per 64 frames) and the kernels' workspace"""
    lens = np.array([s.numel() for s in sigs], dtype=np.int64)
    if lens.max() >= 2 ** 31 - 2 * N_FFT:
        raise ValueError("log_mel: a clip of %d samples is too long" % lens.max())
    B = len(sigs)
    nf = 1 + lens // HOP
    ntile = (nf + LOGMEL_TILE_FRAMES - 1) // LOGMEL_TILE_FRAMES
    tiles = np.empty((int(ntile.sum()), 2), dtype=np.int32)
    tiles[:, 0] = np.repeat(np.arange(B), ntile)
    tiles[:, 1] = (np.arange(len(tiles)) - np.repeat(np.cumsum(ntile) - ntile, ntile)) * LOGMEL_TILE_FRAMES
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return dict(x=torch.cat(sigs), lens=lens, T=T, ntiles=len(tiles), offsets_d=torch.from_numpy(offsets).to(dev),
                lens_d=torch.from_numpy(lens.astype(np.int32)).to(dev), tiles_d=torch.from_numpy(tiles).to(dev),
                mean=torch.empty(B, dtype=torch.float32, device=dev),
                maxbits=torch.empty(B, dtype=torch.int32, device=dev),
                melpow=torch.empty((B, T, N_MELS), dtype=torch.float32, device=dev))


def launch(batch, out, layout):
    """the three kernels on the current stream: mean, mel power + max, dB + fill into `out`"""
    lib = _lib.load()
    basis, bank, ranges = device_constants(out.device)
    B, T, st = len(batch["lens"]), batch["T"], stream()
    x, off, lens, mean, maxbits, melpow = (ptr(batch[k]) for k in ("x", "offsets_d", "lens_d", "mean", "maxbits",
                                                                   "melpow"))
    check(lib.s2i_signal_mean(x, off, lens, B, mean, maxbits, st), "s2i_signal_mean")
    check(lib.s2i_logmel_power(x, off, lens, B, mean, ptr(basis), ptr(bank), ptr(ranges), ptr(batch["tiles_d"]),
                               batch["ntiles"], T, melpow, maxbits, st), "s2i_logmel_power")
    check(lib.s2i_logmel_finish(melpow, maxbits, lens, B, T, _LAYOUTS[layout], ptr(out), st), "s2i_logmel_finish")


def flops(num_frames):
    """Algorithmic FLOP count of the power + mel stage: a 400 x 400 real DFT and a 201 -> 40 projection per frame."""
    return float(num_frames) * (2 * N_FFT * N_FFT + 2 * N_BINS * N_MELS)

