"""numpy restatement of the phase-vocoder time stretch (csrc/s2i_stretch.hip) and of the tempo= / pitch= fields of
ops.waveaug_plan, as include/s2i_hip.h and the plan's docstring word them.

`time_stretch(x, rho, dtype)` has two modes: dtype=np.float64 is the reference; dtype=np.float32 is the yardstick, the same
arithmetic with every array in float32 (the two DFTs as float32 matrix products against the bases rounded once, the same
wrapped recursion).  What the kernel may deviate from float64 is bounded by twice what the yardstick deviates
(DESIGN.md 8b4d); `measure_yardsticks()` prints the table."""
import math

import numpy as np

import resample_ref
import waveaug_ref

N_FFT = 512
HOP = 128
N_BINS = N_FFT // 2 + 1
KEY_XOR = 0x53545243
RATE = 16000
MIN_FRAMES = 64
RATE_GRID = 50


def window():
    """periodic Hann, float64"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def _angles(k):
    i = np.arange(N_FFT)[:, None]
    return 2.0 * np.pi * ((i * np.asarray(k)[None, :]) % N_FFT) / N_FFT       # [sample i][bin]


def forward_basis():
    """[512 samples][512 columns] float64, the window folded in: column k <= 256 is w cos(2 pi i k / 512), column
    256 + k for k = 1..255 is -w sin(2 pi i k / 512) (bins 0 and 256 have no imaginary part)."""
    w = window()[:, None]
    return np.concatenate([w * np.cos(_angles(np.arange(N_BINS))), -w * np.sin(_angles(np.arange(1, N_BINS - 1)))], axis=1)


def inverse_basis():
    """[512 rows][512 samples] float64: row k <= 256 is c_k w[i] / 512 cos(2 pi i k / 512), row 256 + k for k = 1..255 is
    -2 w[i] / 512 sin(2 pi i k / 512); c_0 = c_256 = 1, c_k = 2 otherwise."""
    w = window()[None, :] / N_FFT
    c = np.full(N_BINS, 2.0)
    c[0] = c[-1] = 1.0
    return np.concatenate([c[:, None] * w * np.cos(_angles(np.arange(N_BINS))).T,
                           -2.0 * w * np.sin(_angles(np.arange(1, N_BINS - 1))).T], axis=0)


def n_frames(n):
    return 1 + int(n) // HOP


def out_frames(n, rho):
    return int(math.ceil(n_frames(n) / float(rho)))


def out_length(n, rho):
    return int(math.floor(int(n) / float(rho) + 0.5))


def analysis(x, dtype=np.float64):
    """(re, im) [F][257] of the clip's F = 1 + n div 128 frames"""
    x = np.asarray(x, dtype=dtype)
    F = n_frames(len(x))
    pad = np.zeros(len(x) + N_FFT + HOP, dtype=dtype)
    pad[N_FFT // 2:N_FFT // 2 + len(x)] = x
    frames = np.stack([pad[HOP * t:HOP * t + N_FFT] for t in range(F)])
    X = frames @ forward_basis().astype(dtype)
    im = np.zeros((F, N_BINS), dtype=dtype)
    im[:, 1:N_BINS - 1] = X[:, N_BINS:]
    return X[:, :N_BINS], im


def polar(re, im):
    """(|X|, arg X / 2 pi) in the arrays' type"""
    dtype = re.dtype
    return np.hypot(re, im), np.arctan2(im, re) * dtype.type(1.0 / (2.0 * np.pi))


def _wrap(v):
    return v - np.rint(v)


def vocoder(mag, turns, rho, frames_out=None):
    """(re, im) [out_frames][257] of the stretched spectrum.  s = t rho in float64 whatever the arrays' type."""
    dtype = mag.dtype
    F = len(mag)
    frames_out = int(math.ceil(F / float(rho))) if frames_out is None else frames_out
    zero = np.zeros((2, N_BINS), dtype=dtype)
    mag, turns = np.concatenate([mag, zero]), np.concatenate([turns, zero])
    phi = ((np.arange(N_BINS) % 4) / 4.0).astype(dtype)
    two_pi = dtype.type(2.0 * np.pi)
    theta = turns[0].copy()
    re, im = np.zeros((frames_out, N_BINS), dtype=dtype), np.zeros((frames_out, N_BINS), dtype=dtype)
    for t in range(frames_out):
        s = float(t) * float(rho)
        j = int(math.floor(s))
        a = dtype.type(s - j)
        j = min(j, F)                                 # t rho < F up to its rounding: frames F and F + 1 are the zeros
        m = (dtype.type(1.0) - a) * mag[j] + a * mag[j + 1]
        re[t], im[t] = m * np.cos(two_pi * theta), m * np.sin(two_pi * theta)
        d = _wrap((turns[j + 1] - turns[j]) - phi)
        theta = _wrap((theta + phi) + d)
    return re, im


def synthesis(re, im):
    """[frames][512]: the windowed inverse transform of every frame; the imaginary parts of bins 0 and 256 are not read"""
    dtype = re.dtype
    return np.concatenate([re, im[:, 1:N_BINS - 1]], axis=1) @ inverse_basis().astype(dtype)


def overlap_add(frames, out_len):
    """out[m], m < out_len: the frames that cover u = m + 256 summed in ascending t, over the same sum of w^2 where that
    exceeds 1e-10"""
    dtype = frames.dtype
    T = len(frames)
    w = window().astype(dtype)
    w2 = w * w
    total = max(HOP * (T - 1) + N_FFT, out_len + N_FFT // 2) if T else out_len + N_FFT // 2
    num, den = np.zeros(total, dtype=dtype), np.zeros(total, dtype=dtype)
    for t in range(T):
        num[HOP * t:HOP * t + N_FFT] += frames[t]
        den[HOP * t:HOP * t + N_FFT] += w2
    num, den = num[N_FFT // 2:N_FFT // 2 + out_len], den[N_FFT // 2:N_FFT // 2 + out_len]
    return np.where(den > 1e-10, num / np.where(den > 1e-10, den, 1), num).astype(dtype)


def time_stretch(x, rho, dtype=np.float64):
    """The clip stretched by rho (duration / rho): librosa.effects.time_stretch with n_fft 512, hop 128, a periodic Hann
    window and zero centre padding, the phase kept in turns.  rho == 1 returns the clip."""
    x = np.asarray(x, dtype=dtype)
    if float(rho) == 1.0:
        return x.copy()
    re, im = vocoder(*polar(*analysis(x, dtype)), rho)
    return overlap_add(synthesis(re, im), out_length(len(x), rho))


def rel_err(got, ref):
    """max|got - ref| / max|ref| (the absolute deviation where the reference is all zeros)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.max(np.abs(ref)) if ref.size else 0.0
    d = np.max(np.abs(got - ref)) if ref.size else 0.0
    return float(d / scale) if scale > 0 else float(d)


# ---- the plan (ops.waveaug_plan's tempo= / pitch= fields) ---------------------------------------------------------------
def indices(seed, step, uid, n_tempo, n_pitch):
    """(tempo index, pitch index) of one uid: words 0 and 1 of the block at counter (step lo, step hi, uid, 0) on the key
    (seed lo, seed hi ^ KEY_XOR), each min(int(u (float)n), n - 1) with u = (r >> 8) 2^-24"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    r = waveaug_ref.philox4x32_10(step & 0xFFFFFFFF, step >> 32, int(uid), 0, seed & 0xFFFFFFFF, (seed >> 32) ^ KEY_XOR)
    u = [np.float32(int(w) >> 8) * np.float32(2.0 ** -24) for w in r]
    return waveaug_ref.draw(u[0], n_tempo), waveaug_ref.draw(u[1], n_pitch)


def read_rate(speed_rate, semitones):
    """R: the speed's rate where S == 0, else Rs 2^(S / 12) on the 50 Hz grid"""
    if semitones == 0:
        return int(speed_rate)
    return RATE_GRID * int(round(speed_rate * 2.0 ** (semitones / 12.0) / RATE_GRID))


def plan_one(policy, seed, step, uid, n, T=2048):
    """dict(rate, out_len, tempo, semitones, stretch_rate, stretch_len) of one clip of n samples under a policy with
    tempo= and / or pitch= (and speed=)."""
    speed_rate = RATE
    if policy["rates"] is not None:
        speed_rate = policy["rates"][waveaug_ref.draw(waveaug_ref.uniforms(seed, step, uid, 0)[0], len(policy["rates"]))]
    tempos, pitches = policy.get("tempo") or (1.0,), policy.get("pitch") or (0.0,)
    it, ip = indices(seed, step, uid, len(tempos), len(pitches))
    tempo, semis = float(tempos[it]), float(pitches[ip])
    R = read_rate(speed_rate, semis)
    rho = tempo * speed_rate / R
    stretch_len = out_length(n, rho) if rho != 1.0 else int(n)
    L, M, _, _ = resample_ref.plan(R)
    out_len = resample_ref.out_length(stretch_len, L, M)
    if (R != RATE or rho != 1.0) and waveaug_ref.n_frames(out_len, T) < MIN_FRAMES:
        return dict(rate=RATE, out_len=int(n), tempo=1.0, semitones=0.0, stretch_rate=1.0, stretch_len=int(n))
    return dict(rate=R, out_len=out_len, tempo=tempo, semitones=semis, stretch_rate=rho, stretch_len=stretch_len)


# ---- the cases ----------------------------------------------------------------------------------------------------------
CASE_LENS = (1, 127, 128, 129, 511, 512, 513, 640, 5000)
CASE_RATES = (0.25, 0.5, 0.84, 1.1, 2.0, 4.0)
LONG_CASE = (70000, 0.5)
FLOOR = 1e-3            # min |X_t[k]| over the clip's frames and bins, as a fraction of the maximum
# the seed of each length's input: the first one whose clip meets FLOOR (find_seed); test_stretch_cpu.py asserts it does
CASE_SEEDS = {1: 0, 127: 0, 128: 0, 129: 0, 511: 0, 512: 0, 513: 0, 640: 0, 5000: 0, 70000: 76}


def case_input(n, seed):
    """n samples of seeded uniform noise plus two weak tones, float32"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    x = rng.uniform(-0.5, 0.5, n) + 0.01 * np.sin(2.0 * np.pi * 0.0371 * i + 0.3) + 0.01 * np.sin(2.0 * np.pi * 0.211 * i + 1.1)
    return x.astype(np.float32)


def floor_ratio(x):
    """min |X| / max |X| over every frame and bin of the float64 analysis"""
    mag = np.hypot(*analysis(x))
    return float(mag.min() / mag.max())


def find_seed(n, limit=4000):
    for seed in range(limit):
        if floor_ratio(case_input(n, seed)) >= FLOOR:
            return seed
    raise ValueError("no seed under %d gives a clip of %d samples with every bin above %g of the maximum" % (limit, n, FLOOR))


def case_clip(n):
    return case_input(n, CASE_SEEDS[n])


def cases():
    """[(n, rho)]: every boundary length at every rate, then the long clip"""
    return [(n, r) for n in CASE_LENS for r in CASE_RATES] + [LONG_CASE]


# per case, the float32 mode's deviation from float64 (measure_yardsticks on the CPU)
YARDSTICK = {
    (1, 0.25): 4.26e-07, (1, 0.5): 4.26e-07, (1, 0.84): 4.26e-07, (1, 1.1): 0.0, (1, 2.0): 0.0, (1, 4.0): 0.0,
    (127, 0.25): 3.71e-07, (127, 0.5): 3.68e-07, (127, 0.84): 3.74e-07, (127, 1.1): 3.01e-07, (127, 2.0): 3.01e-07, (127, 4.0): 3.01e-07,
    (128, 0.25): 5.15e-07, (128, 0.5): 2.85e-07, (128, 0.84): 6.51e-07, (128, 1.1): 4.9e-07, (128, 2.0): 2.41e-07, (128, 4.0): 2.41e-07,
    (129, 0.25): 6.06e-07, (129, 0.5): 3.77e-07, (129, 0.84): 6.25e-07, (129, 1.1): 5.03e-07, (129, 2.0): 2.11e-07, (129, 4.0): 2.11e-07,
    (511, 0.25): 1.29e-06, (511, 0.5): 7.6e-07, (511, 0.84): 4.59e-07, (511, 1.1): 7.45e-07, (511, 2.0): 8e-07, (511, 4.0): 4.22e-07,
    (512, 0.25): 1.23e-06, (512, 0.5): 6.54e-07, (512, 0.84): 4.49e-07, (512, 1.1): 4.67e-07, (512, 2.0): 6.16e-07, (512, 4.0): 5.2e-07,
    (513, 0.25): 1.26e-06, (513, 0.5): 6.63e-07, (513, 0.84): 4.69e-07, (513, 1.1): 6.2e-07, (513, 2.0): 5.84e-07, (513, 4.0): 3.97e-07,
    (640, 0.25): 1.22e-06, (640, 0.5): 6.44e-07, (640, 0.84): 4.75e-07, (640, 1.1): 6.05e-07, (640, 2.0): 5.72e-07, (640, 4.0): 6.41e-07,
    (5000, 0.25): 2.97e-06, (5000, 0.5): 1.26e-06, (5000, 0.84): 1.59e-06, (5000, 1.1): 1.18e-06, (5000, 2.0): 2.56e-06, (5000, 4.0): 2.05e-06,
    (70000, 0.5): 4.91e-06,
}
# A yardstick under one unit roundoff says nothing: at n = 1 and rho >= 1.1 the single output is x_0 w[256]^2 / w[256]^2
# and the float32 mode happens to return it exactly.  A result that is rounded to fp32 once is off by up to 2^-24 of itself,
# so that is the least yardstick a case is held to (bound 2^-23, one ulp of max|ref|).
YARDSTICK_FLOOR = 2.0 ** -24


def bound(n, rho):
    """what the kernel may deviate from float64 in case (n, rho): twice the case's yardstick, at least twice the floor"""
    return 2.0 * max(YARDSTICK[(n, rho)], YARDSTICK_FLOOR)


def measure_yardsticks():
    """{(n, rho): rel_err of the float32 mode against float64}"""
    out = {}
    for n, rho in cases():
        x = case_clip(n)
        out[(n, rho)] = rel_err(time_stretch(x, rho, np.float32), time_stretch(x, rho, np.float64))
    return out


if __name__ == "__main__":
    for key, v in measure_yardsticks().items():
        print(key, "%.3g" % v)
