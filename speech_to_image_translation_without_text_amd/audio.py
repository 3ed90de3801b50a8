"""Speech front end: 16 kHz PCM16 WAV files -> the reference's log-mel arrays, on the MI355X kernels.

The reference builds the encoder's input with librosa, one file at a time on the CPU (Audio_to_Image/utils.py:292-340,
`load_one_audio_file`): load at 16 kHz, subtract the mean, pre-emphasis 0.97, librosa.stft (n_fft = win_length = 400,
hop 160, symmetric scipy Hamming window, center=True with reflect padding), |.|^2, a 40-band Slaney mel bank from 20 Hz
(librosa.filters.mel(16000, 400, n_mels=40, fmin=20)), power_to_db(ref=np.max, top_db=80), and 0 dB padding or
truncation to 2048 frames.  Here a whole ragged batch runs as three kernels (csrc/s2i_audio.hip): a per-utterance mean,
`logmel_power` (the STFT as one fp32 MFMA GEMM against a window-folded DFT basis, power, mel projection and the
per-utterance max over every frame), and `logmel_finish` (dB, floor, fill).  The basis and the mel bank are built in
float64 here, rounded to fp32 once and cached per device.

read_wav uses the stdlib `wave` module: PCM16 at 16 kHz, mono or stereo (averaged), and refuses other rates and sample
formats.  Those go through the opt-in path below it: `read_audio` (a RIFF reader for PCM at 8, 16, 24 and 32 bits and
IEEE float at 32 and 64 bits, 1 to 8 channels, 4 to 192 kHz) and `to_16k`, which decodes, mixes down and resamples a
batch to 16 kHz on the GPU in one launch per (rate, format, channels) group (csrc/s2i_resample.hip), as
librosa.load(path, 16000) does on the CPU.

The resampler is band-limited interpolation with resampy's `kaiser_best` constants.  With g = gcd(16000, rate),
L = 16000 / g, M = rate / g, scale = min(1, L / M), W = ceil(64 / scale) and taps = 2 W + 2, the polyphase table is
table[p][j] = scale h(scale (W - j + p / L)) for the prototype h(t) = r sinc(r t) I0(beta sqrt(1 - (t / 64)^2)) / I0(beta)
on |t| <= 64 (0 outside), r = 0.9475937167399596, beta = 14.769656459379492, built in float64 and rounded to fp32 once.
Output m, in integers: q = (m M) div L, p = (m M) mod L, y[m] = sum_j x[q - W + j] table[p][j] with x = 0 outside the clip.
n frames give ceil(n L / M) outputs, and those from floor(n L / M) on are 0.0 (librosa's fix_length).  16 kHz is the bypass
L = M = 1, W = 0, table [1, 0] through the same kernel.  Decode: u8 (v - 128) / 128; s16, s24, s32 v 2^-(bits - 1); f32 as
is; f64 rounded to fp32; channels added in order in fp32 and divided by float(C).  Decode, then mono, then resample.
resampy itself linearly interpolates a 512-point-per-zero-crossing table, which a CPU restatement puts 1.2e-6 of max|y|
from the exact table used here (fp32 rounding level; not verified against librosa, which is not installed where this
was written); newer librosa releases default to another resampler (soxr).
"""
import collections
import math
import struct
import wave

import numpy as np
import torch

from . import _lib
from ._lib import (LOGMEL_BFT, LOGMEL_NHWC, LOGMEL_TILE_FRAMES, PCM_F32, PCM_F64, PCM_S16, PCM_S24, PCM_S32, PCM_U8,
                   RESAMPLE_MAX_WINDOW, RESAMPLE_TILE, check, ptr, stream)

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


# ---- any WAV -> 16 kHz mono (opt-in: --resample) ---------------------------------------------------------------------
MIN_RATE, MAX_RATE = 4000, 192000
MAX_CHANNELS = 8
MAX_TABLE_FLOATS = 1 << 24
KAISER_ZEROS = 64
KAISER_ROLLOFF = 0.9475937167399596
KAISER_BETA = 14.769656459379492
SAMPLE_BYTES = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4, PCM_F64: 8}
_PCM_BITS = {8: PCM_U8, 16: PCM_S16, 24: PCM_S24, 32: PCM_S32}
_FLOAT_BITS = {32: PCM_F32, 64: PCM_F64}

AudioInfo = collections.namedtuple("AudioInfo", "path rate channels format frames data_start data_bytes")


def resample_plan(rate):
    """(L, M, W, taps) of a file rate: the reduced ratio 16000 / rate, the half width ceil(64 / min(1, L / M)) in input
    samples and 2 W + 2 taps; (1, 1, 0, 2) at 16 kHz.  Rates outside [4000, 192000] or whose table would hold more than
    2^24 floats raise ValueError."""
    if isinstance(rate, bool) or int(rate) != rate:
        raise ValueError("sample rate %r is not an integer" % (rate,))
    rate = int(rate)
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError("sample rate %d Hz is outside [%d, %d]" % (rate, MIN_RATE, MAX_RATE))
    if rate == SAMPLE_RATE:
        return 1, 1, 0, 2
    g = math.gcd(SAMPLE_RATE, rate)
    L, M = SAMPLE_RATE // g, rate // g
    W = KAISER_ZEROS if M <= L else -(-KAISER_ZEROS * M // L)
    taps = 2 * W + 2
    if L * taps > MAX_TABLE_FLOATS:
        raise ValueError("sample rate %d Hz needs a resampling table of %d x %d floats, over %d"
                         % (rate, L, taps, MAX_TABLE_FLOATS))
    return L, M, W, taps


def kaiser_prototype(t):
    """h(t) of the module docstring, float64"""
    t = np.asarray(t, dtype=np.float64)
    u = np.clip(1.0 - (t / KAISER_ZEROS) ** 2, 0.0, None)
    h = KAISER_ROLLOFF * np.sinc(KAISER_ROLLOFF * t) * np.i0(KAISER_BETA * np.sqrt(u)) / np.i0(KAISER_BETA)
    return np.where(np.abs(t) <= KAISER_ZEROS, h, 0.0)


def resample_table(rate):
    """[L][taps] float64: table[p][j] = scale h(scale (W - j + p / L)); [[1, 0]] at 16 kHz"""
    L, M, W, taps = resample_plan(rate)
    if int(rate) == SAMPLE_RATE:
        return np.array([[1.0, 0.0]])
    scale = min(1.0, L / M)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(taps, dtype=np.float64)[None, :]
    return scale * kaiser_prototype(scale * (W - j + p / L))


def resampled_length(n, rate):
    """ceil(n L / M), librosa's n_samples, in integers"""
    L, M, _, _ = resample_plan(rate)
    return -(-int(n) * L // M)


def pack_resample_table(table):
    """[L][taps] -> the flat device layout of s2i_pcm_resample (include/s2i_hip.h): [L][tpad] with tpad = taps rounded up
    to a multiple of 4 and a zero pad, so that every phase's row is 16-byte aligned."""
    t = np.asarray(table)
    L, taps = t.shape
    out = np.zeros((L, (taps + 3) // 4 * 4), dtype=t.dtype)
    out[:, :taps] = t
    return out.reshape(-1)


def unpack_resample_table(flat, L, taps):
    return np.ascontiguousarray(np.asarray(flat).reshape(L, (taps + 3) // 4 * 4)[:, :taps])


_TABLES = {}


def device_resample_table(device, rate):
    """the packed fp32 table of `rate` on `device`, built once per (device, rate)"""
    key = (str(device), int(rate))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(pack_resample_table(resample_table(rate).astype(np.float32))).to(device)
    return _TABLES[key]


def _refuse(path, what):
    raise ValueError("%s: %s" % (path, what))


def probe_audio(path):
    """The header of a RIFF/WAVE file -> AudioInfo(path, rate, channels, format, frames, data_start, data_bytes); format
    is one of _lib.PCM_*.  Accepted: tag 1 (PCM at 8, 16, 24 or 32 bits), tag 3 (IEEE float at 32 or 64 bits) and tag
    0xFFFE (extensible: the sub-format is the GUID's first two bytes), 1 to 8 channels, rates resample_plan accepts.
    Unknown chunks (a LIST in front of `data` too) and the pad byte of odd-size chunks are skipped; a `data` size past
    the end of the file is cut to whole frames.  Everything else raises a ValueError that names the file."""
    path = str(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[8:12] != b"WAVE" or head[:4] not in (b"RIFF", b"RF64"):
            _refuse(path, "not a RIFF/WAVE file")
        if head[:4] == b"RF64":
            _refuse(path, "RF64 files are not supported")
        f.seek(0, 2)
        size = f.tell()
        pos, fmt = 12, None
        while True:
            f.seek(pos)
            ck = f.read(8)
            if len(ck) < 8:
                _refuse(path, "no `data` chunk" if fmt else "no `fmt ` chunk")
            cid, csize = ck[:4], struct.unpack("<I", ck[4:])[0]
            if cid == b"fmt ":
                body = f.read(min(csize, 40))
                if len(body) < 16:
                    _refuse(path, "`fmt ` chunk of %d bytes" % len(body))
                tag, ch, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == 0xFFFE:
                    if len(body) < 26:
                        _refuse(path, "extensible `fmt ` chunk of %d bytes" % len(body))
                    tag = struct.unpack("<H", body[24:26])[0]
                fmt = (tag, ch, rate, align, bits)
            elif cid == b"data":
                if fmt is None:
                    _refuse(path, "`data` chunk in front of `fmt `")
                break
            pos += 8 + csize + (csize & 1)
        start = pos + 8
    tag, ch, rate, align, bits = fmt
    if tag == 1:
        if bits not in _PCM_BITS:
            _refuse(path, "%d-bit PCM; need 8, 16, 24 or 32 bits" % bits)
        code = _PCM_BITS[bits]
    elif tag == 3:
        if bits not in _FLOAT_BITS:
            _refuse(path, "%d-bit float samples; need 32 or 64 bits" % bits)
        code = _FLOAT_BITS[bits]
    else:
        _refuse(path, "format tag 0x%04x (compressed?) is not supported; need PCM (1) or IEEE float (3)" % tag)
    if not 1 <= ch <= MAX_CHANNELS:
        _refuse(path, "%d channels; need 1 to %d" % (ch, MAX_CHANNELS))
    if align != SAMPLE_BYTES[code] * ch:
        _refuse(path, "block align %d contradicts %d bits x %d channels" % (align, bits, ch))
    try:
        resample_plan(rate)
    except ValueError as e:
        _refuse(path, str(e))
    frames = min(csize, max(size - start, 0)) // align
    return AudioInfo(path, rate, ch, code, frames, start, frames * align)


def read_audio(path):
    """(AudioInfo, the `data` chunk's whole frames as a uint8 array)"""
    info = probe_audio(path)
    with open(info.path, "rb") as f:
        f.seek(info.data_start)
        raw = np.frombuffer(f.read(info.data_bytes), dtype=np.uint8)
    if raw.size != info.data_bytes:
        _refuse(info.path, "read %d of %d data bytes" % (raw.size, info.data_bytes))
    return info, raw


def _pad16(n):
    return (int(n) + 15) // 16 * 16


def resample_tiles(out_lens):
    """[ntiles][2] int32 (clip, first output index): one entry per RESAMPLE_TILE outputs, as prepare_batch's table"""
    out_lens = np.asarray(out_lens, dtype=np.int64)
    ntile = (out_lens + RESAMPLE_TILE - 1) // RESAMPLE_TILE
    tiles = np.empty((int(ntile.sum()), 2), dtype=np.int32)
    tiles[:, 0] = np.repeat(np.arange(len(out_lens)), ntile)
    tiles[:, 1] = (np.arange(len(tiles)) - np.repeat(np.cumsum(ntile) - ntile, ntile)) * RESAMPLE_TILE
    return tiles


def pack_group(raws, frames, out_offsets, out_lens):
    """One host byte image of a group: int64 byte offsets [B] | int64 out offsets [B] | int32 frames [B] | int32 out
    lens [B] | int32 tiles [ntiles][2] | the clips' bytes, every part and every clip starting on a 16-byte boundary (byte
    offsets count from the first clip's part).  Returns (image, {part: byte position}, ntiles)."""
    B = len(raws)
    tiles = resample_tiles(out_lens)
    starts = np.zeros(B, dtype=np.int64)
    pos = 0
    for b, r in enumerate(raws):
        starts[b] = pos
        pos += _pad16(len(r))
    parts = [("boff", starts), ("ooff", np.asarray(out_offsets, dtype=np.int64)),
             ("frames", np.asarray(frames, dtype=np.int32)), ("olen", np.asarray(out_lens, dtype=np.int32)),
             ("tiles", tiles.reshape(-1))]
    where, at = {}, 0
    for name, a in parts:
        where[name] = at
        at += _pad16(a.nbytes)
    where["raw"] = at
    image = np.zeros(at + max(pos, 16), dtype=np.uint8)
    for name, a in parts:
        image[where[name]:where[name] + a.nbytes] = np.ascontiguousarray(a).view(np.uint8)
    for b, r in enumerate(raws):
        image[at + starts[b]:at + starts[b] + len(r)] = r
    return image, where, len(tiles)


def launch_resample(image_d, where, ntiles, B, fmt, channels, L, M, W, table_d, out):
    """s2i_pcm_resample over one uploaded group image (pack_group) on the current stream"""
    base = image_d.data_ptr()
    check(_lib.load().s2i_pcm_resample(base + where["raw"], base + where["boff"], base + where["frames"], B, fmt,
                                       channels, L, M, W, ptr(table_d), base + where["tiles"], ntiles, ptr(out),
                                       base + where["ooff"], base + where["olen"], stream()), "s2i_pcm_resample")


def to_16k(clips, device=None):
    """`librosa.load(path, 16000)` for a list of `read_audio` results, on the GPU: a list of 1-D fp32 device tensors of
    16 kHz mono samples, in input order, all views of one flat buffer.  The clips that share (rate, format, channels)
    form a group: one upload and one launch each.  `log_mel` takes the result unchanged."""
    _lib.load()
    _lib.require_device()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _lib.S2IError("to_16k runs on the MI355X kernels: there is no CPU fallback (device %s)" % dev)
    infos = [c[0] for c in clips]
    for info, raw in clips:
        if len(raw) != info.frames * info.channels * SAMPLE_BYTES[info.format]:
            raise ValueError("%s: %d data bytes, the header promised %d frames" % (info.path, len(raw), info.frames))
        if info.frames >= 2 ** 31 - 1:
            raise ValueError("%s: a clip of %d frames is too long" % (info.path, info.frames))
    out_lens = np.array([resampled_length(i.frames, i.rate) for i in infos], dtype=np.int64)
    out_offsets = np.cumsum(out_lens) - out_lens
    total = int(out_lens.sum())
    flat = torch.empty(total, dtype=torch.float32, device=dev)
    groups = {}
    for k, i in enumerate(infos):
        if out_lens[k] > 0:
            groups.setdefault((i.rate, i.format, i.channels), []).append(k)
    with torch.cuda.device(dev):
        for (rate, fmt, ch), ids in groups.items():
            L, M, W, _ = resample_plan(rate)
            image, where, ntiles = pack_group([clips[k][1] for k in ids], [infos[k].frames for k in ids],
                                              out_offsets[ids], out_lens[ids])
            image_d = torch.from_numpy(image).to(dev)
            launch_resample(image_d, where, ntiles, len(ids), fmt, ch, L, M, W, device_resample_table(dev, rate), flat)
    return [flat[int(o):int(o + n)] for o, n in zip(out_offsets, out_lens)]


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
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return prepare_flat(torch.cat(sigs), offsets, lens, T, dev)


def prepare_flat(flat, offsets, lens, T, dev):
    """prepare_batch's buffers over clips that already lie in one flat fp32 device tensor: clip b is
    flat[offsets[b] : offsets[b] + lens[b]], lens[b] >= 1 (host arrays; the clips need not be back to back)"""
    lens = np.asarray(lens, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    if lens.max() >= 2 ** 31 - 2 * N_FFT:
        raise ValueError("log_mel: a clip of %d samples is too long" % lens.max())
    if len(offsets) != len(lens) or lens.min() < 1 or offsets.min() < 0 or int((offsets + lens).max()) > flat.numel():
        raise ValueError("log_mel: a clip is empty or lies outside the flat buffer of %d samples" % flat.numel())
    B = len(lens)
    nf = 1 + lens // HOP
    ntile = (nf + LOGMEL_TILE_FRAMES - 1) // LOGMEL_TILE_FRAMES
    tiles = np.empty((int(ntile.sum()), 2), dtype=np.int32)
    tiles[:, 0] = np.repeat(np.arange(B), ntile)
    tiles[:, 1] = (np.arange(len(tiles)) - np.repeat(np.cumsum(ntile) - ntile, ntile)) * LOGMEL_TILE_FRAMES
    return dict(x=flat, lens=lens, T=T, ntiles=len(tiles), offsets_d=torch.from_numpy(offsets).to(dev),
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

