"""fp64 restatement of the WAV -> 16 kHz mono path (audio.to_16k, csrc/s2i_resample.hip), independent of the package.

Definition.  Band-limited interpolation with resampy's `kaiser_best` constants, the method librosa.load(path, 16000) of
the reference's era uses (Audio_to_Image/utils.py:313).  `rate` is the file's rate, g = gcd(16000, rate), L = 16000 / g,
M = rate / g, scale = min(1, L / M), W = ceil(64 / scale), taps = 2 W + 2.  Prototype
h(t) = r sinc(r t) I0(beta sqrt(1 - (t / 64)^2)) / I0(beta) for |t| <= 64 and 0 outside, r = 0.9475937167399596,
beta = 14.769656459379492, sinc(x) = sin(pi x) / (pi x).  table[p][j] = scale h(scale (W - j + p / L)), p in [0, L),
j in [0, taps), in float64, rounded to fp32 once.  Output m, in integers: q = (m M) div L, p = (m M) mod L,
y[m] = sum_j x[q - W + j] table[p][j] with x = 0 outside [0, n).  n_out = ceil(n L / M); outputs m >= floor(n L / M) are
0.0 (librosa's fix_length pads there); n = 0 gives an empty clip.  16 kHz is the bypass L = M = 1, W = 0, table [1, 0].
Decode (little-endian, interleaved): u8 (v - 128) / 128; s16, s24, s32 float(v) 2^-(bits - 1); f32 as is; f64 rounded to
fp32.  Mono: channels added in channel order in fp32, divided by float(C) in fp32.  Decode, then mono, then resample.

Known distance to librosa (not verified: neither librosa nor resampy is installed here): resampy linearly interpolates a
table of 512 points per zero crossing; a CPU restatement of that differs from the exact table by 1.2e-6 of max|y| at
44.1 and 48 kHz.  Newer librosa releases default to soxr.

`resample` takes the table as an argument, so it runs with any table (a random one makes every tap count), and `mutant`
names one of five wrong versions a test must be able to tell from it.  `resample_f32` is the same sum with the fp32
table and fp32 products and accumulation in tap order: the yardstick of the fp32 kernel's tolerance."""
import math
import struct

import numpy as np

OUT_RATE = 16000
ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
U8, S16, S24, S32, F32, F64 = range(6)
WIDTH = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
MUTANTS = ("q_plus_one", "phases_reversed", "last_tap_dropped", "tail_computed", "previous_clip_leaks")


def plan(rate):
    """(L, M, W, taps)"""
    if rate == OUT_RATE:
        return 1, 1, 0, 2
    g = math.gcd(OUT_RATE, rate)
    L, M = OUT_RATE // g, rate // g
    W = ZEROS if M <= L else (ZEROS * M + L - 1) // L
    return L, M, W, 2 * W + 2


def prototype(t):
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) <= ZEROS
    u = np.where(inside, 1.0 - (t / ZEROS) ** 2, 0.0)
    x = np.pi * ROLLOFF * t
    sinc = np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x))
    return np.where(inside, ROLLOFF * sinc * np.i0(BETA * np.sqrt(u)) / np.i0(BETA), 0.0)


def table(rate):
    """[L][taps] float64"""
    L, M, W, taps = plan(rate)
    if rate == OUT_RATE:
        return np.array([[1.0, 0.0]])
    scale = min(1.0, L / M)
    out = np.empty((L, taps))
    for p in range(L):
        out[p] = scale * prototype(scale * (W - np.arange(taps) + p / L))
    return out


def out_length(n, L, M):
    return -(-n * L // M)


def decode(raw, fmt, channels):
    """bytes -> [frames][channels] float32"""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    if fmt == U8:
        v = (raw.astype(np.float64) - 128.0) / 128.0
    elif fmt == S16:
        v = raw.view("<i2").astype(np.float64) / 2.0 ** 15
    elif fmt == S24:
        b = raw.reshape(-1, 3).astype(np.int64)
        i = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
        v = np.where(i >= 1 << 23, i - (1 << 24), i).astype(np.float64) / 2.0 ** 23
    elif fmt == S32:
        v = raw.view("<i4").astype(np.float64) / 2.0 ** 31
    elif fmt == F32:
        v = raw.view("<f4")
    else:
        v = raw.view("<f8")
    with np.errstate(over="ignore"):
        return v.astype(np.float32).reshape(-1, channels)


def mono(x):
    """[frames][C] float32 -> [frames] float32: channel order, fp32 sums, one fp32 division"""
    x = np.asarray(x, dtype=np.float32)
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = s + x[:, c]
    return s / np.float32(x.shape[1])


def _gather(x, L, M, W, taps, lo, hi, before, dq):
    """(operands [hi - lo][taps] float64, phases [hi - lo]): x[q - W + j] with zeros (or `before`) outside the clip"""
    n = len(x)
    m = np.arange(lo, hi, dtype=np.int64)
    q, p = (m * M) // L + dq, (m * M) % L
    idx = q[:, None] - W + np.arange(taps, dtype=np.int64)[None, :]
    xs = np.concatenate([np.asarray(x, dtype=np.float64), [0.0]])
    ops = xs[np.where((idx >= 0) & (idx < n), idx, n)]
    if before is not None:                   # the wrong clip start: indices under 0 read the previous clip's end
        b = np.asarray(before, dtype=np.float64)
        neg = idx < 0
        ops[neg] = b[np.maximum(len(b) + idx[neg], 0)]
    return ops, p


def resample(x, L, M, W, tab, lo=0, hi=None, mutant=None, before=None, acc=np.float64):
    """y[lo:hi] of the clip `x` (mono) under table `tab` [L][2 W + 2], float64 (or `acc`); the whole clip by default.
    Work is done in blocks of outputs, so a 13.5 M-sample clip's tail costs what the tail costs."""
    n, taps = len(x), 2 * W + 2
    tab = np.asarray(tab)
    assert tab.shape == (L, taps), (tab.shape, L, taps)
    nout, nfull = out_length(n, L, M), n * L // M
    hi = nout if hi is None else hi
    out = np.zeros(hi - lo, dtype=acc)
    for s in range(lo, hi, 4096):
        e = min(s + 4096, hi)
        ops, p = _gather(x, L, M, W, taps, s, e, before if mutant == "previous_clip_leaks" else None,
                         1 if mutant == "q_plus_one" else 0)
        rows = tab[(L - 1 - p) if mutant == "phases_reversed" else p]
        if mutant == "last_tap_dropped":
            rows = rows.copy()
            rows[:, -1] = 0
        if acc is np.float64:
            y = (ops * rows).sum(axis=1)
        else:                                 # fp32 products, fp32 accumulation in tap order
            o32, r32 = ops.astype(np.float32), rows.astype(np.float32)
            y = np.zeros(e - s, dtype=np.float32)
            for j in range(taps):
                y = y + o32[:, j] * r32[:, j]
        if mutant != "tail_computed":
            y[np.arange(s, e) >= nfull] = 0
        out[s - lo:e - lo] = y
    return out


def resample_f32(x, L, M, W, tab, lo=0, hi=None):
    return resample(x, L, M, W, np.asarray(tab, dtype=np.float32), lo, hi, acc=np.float32)


def load(raw, fmt, channels, rate, tab=None):
    """decode, mono, resample with the fp32-rounded table of `rate` (or `tab`) -> float64"""
    L, M, W, _ = plan(rate)
    tab = table(rate).astype(np.float32) if tab is None else tab
    return resample(mono(decode(raw, fmt, channels)), L, M, W, np.asarray(tab, dtype=np.float64))


def rel_err(got, ref):
    """max|got - ref| / max|ref|, the project's convention"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- test inputs ----------------------------------------------------------------------------------------------------
def encode(x, fmt):
    """[frames][C] float64 in [-1, 1) -> little-endian interleaved bytes of `fmt` (rounded to the format's grid)"""
    x = np.asarray(x, dtype=np.float64)
    if fmt == U8:
        return np.clip(np.round(x * 128 + 128), 0, 255).astype(np.uint8).tobytes()
    if fmt == S16:
        return np.clip(np.round(x * 2 ** 15), -2 ** 15, 2 ** 15 - 1).astype("<i2").tobytes()
    if fmt == S24:
        i = np.clip(np.round(x * 2 ** 23), -2 ** 23, 2 ** 23 - 1).astype(np.int64).reshape(-1) & 0xFFFFFF
        return np.stack([i & 255, i >> 8 & 255, i >> 16], axis=1).astype(np.uint8).tobytes()
    if fmt == S32:
        return np.clip(np.round(x * 2 ** 31), -2 ** 31, 2 ** 31 - 1).astype("<i4").tobytes()
    return x.astype("<f4" if fmt == F32 else "<f8").tobytes()


def write_wav(path, data, fmt, channels, rate, extensible=False, chunks_before=(), data_size=None):
    """A RIFF/WAVE file around `data` bytes.  `chunks_before` is a list of (id, body) put in front of `data` (an odd
    body gets its pad byte); `data_size` overrides the size the `data` header states."""
    width = WIDTH[fmt]
    tag = 3 if fmt in (F32, F64) else 1
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * width * channels,
                       width * channels, 8 * width)
    if extensible:
        body += struct.pack("<HHI", 22, 8 * width, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    out = b"WAVE" + b"fmt " + struct.pack("<I", len(body)) + body
    for cid, cbody in chunks_before:
        out += cid + struct.pack("<I", len(cbody)) + cbody + (b"\x00" if len(cbody) & 1 else b"")
    out += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + bytes(data)
    if len(data) & 1:
        out += b"\x00"
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(out)) + out)
