"""numpy restatement of the waveform augmentation (ops.waveaug_plan, csrc/s2i_waveaug.hip) as include/s2i_hip.h and
ops.waveaug_plan's docstring word it, independent of the package: Philox4x32-10 in uint64 arithmetic, the draws with their
one fp32 product, the speed stage through resample_ref, and the mix twice -- `mix` in float64 (the definition) and
`mix_f32` in fp32 with the kernel's documented order for the power sum (the yardstick of the GPU suite's bound).
Mutants of `mix` say what the GPU suite's bound must be able to see."""
import numpy as np

import resample_ref

KEY_XOR = 0x57415645
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
HOP, MIN_FRAMES, RATE = 160, 64, 16000
RUN = 8192
NOISE_C = np.float32(1.0 / np.sqrt((2.0 ** 32 - 1.0) / 3.0))       # rounded to fp32 once
MUTANTS = ("snr_sign", "q_dropped", "wrap_off_by_one", "odd_takes_r0r1", "power_without_tail", "white_scaled_after_babble")


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint64 arrays [4][...] of the output words (each < 2^32) for arrays of counters and one key"""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for r in range(10):
        p0 = np.uint64(M0) * c[0]          # < 2^64: no wrap
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        if r < 9:
            k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c)


def key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & MASK32, (seed >> 32) ^ KEY_XOR


def counter(step, uid, g):
    step = int(step) & (2 ** 64 - 1)
    return step & MASK32, step >> 32, uid, g


def uniforms(seed, step, uid, g):
    """the four u = (r >> 8) 2^-24 of block g of one uid, np.float32"""
    r = philox4x32_10(*counter(step, int(uid), g), *key(seed))
    return [np.float32(int(w) >> 8) * np.float32(2.0 ** -24) for w in r]


def draw(u, n):
    """min(int(u (float)n), n - 1): one fp32 product, truncated"""
    return min(int(np.float32(u) * np.float32(n)), int(n) - 1)


def n_frames(n, T):
    return min(1 + (int(n) or 200) // HOP, T)


def plan_one(policy, seed, step, uid, n, pool_lens=None, pool_q=None, T=2048):
    """The draws of one utterance of n samples: dict(rate, out_len, white_snr, babble_snr (None = off), g_white, g_babble
    (float64, before the one rounding to fp32), src, start)."""
    u0, u1 = uniforms(seed, step, uid, 0), uniforms(seed, step, uid, 1)
    rate = RATE
    if policy["rates"] is not None:
        rate = policy["rates"][draw(u0[0], len(policy["rates"]))]
    L, M, _, _ = resample_ref.plan(rate)
    out_len = resample_ref.out_length(int(n), L, M)
    if rate != RATE and n_frames(out_len, T) < MIN_FRAMES:
        rate, out_len = RATE, int(n)
    p = dict(rate=rate, out_len=out_len, white_snr=None, babble_snr=None, g_white=0.0, g_babble=0.0, src=0, start=0)
    if policy["white"] is not None:
        prob, lo, hi = policy["white"]
        if float(u0[1]) < prob:
            p["white_snr"] = lo + float(u0[2]) * (hi - lo)
            p["g_white"] = 10.0 ** (-p["white_snr"] / 10.0)
    if policy["babble"] is not None:
        prob, lo, hi = policy["babble"]
        j = draw(u1[1], len(pool_lens))
        p["src"], p["start"] = j, draw(u1[2], pool_lens[j])
        if float(u0[3]) < prob:
            p["babble_snr"] = lo + float(u1[0]) * (hi - lo)
            if pool_q[j] > 0.0:
                p["g_babble"] = 10.0 ** (-p["babble_snr"] / 10.0) / float(pool_q[j])
    return p


def speed(x, rate):
    """the clip read at `rate` and converted to 16 kHz, float64, with the fp32-rounded table the kernel gets"""
    if rate == RATE:
        return np.asarray(x, dtype=np.float64).copy()
    L, M, W, _ = resample_ref.plan(rate)
    tab = resample_ref.table(rate).astype(np.float32).astype(np.float64)
    return resample_ref.resample(np.asarray(x, dtype=np.float32), L, M, W, tab)


def noise_int(seed, step, uid, n, mutant=None):
    """h_i - 131070 for i < n, exact integers in float64"""
    i = np.arange(n, dtype=np.uint64)
    r = philox4x32_10(*counter(step, np.uint64(uid), np.uint64(2) + i // np.uint64(2)), *key(seed))
    odd = (i % np.uint64(2)) == 1
    if mutant == "odd_takes_r0r1":
        odd = np.zeros(n, dtype=bool)
    a, b = np.where(odd, r[2], r[0]), np.where(odd, r[3], r[1])
    h = (a & np.uint64(0xFFFF)) + (a >> np.uint64(16)) + (b & np.uint64(0xFFFF)) + (b >> np.uint64(16))
    return h.astype(np.float64) - 131070.0


def noise(seed, step, uid, n, mutant=None):
    """e_i as float64: one product with the fp32 constant (its rounding to fp32 is the kernel's)"""
    return noise_int(seed, step, uid, n, mutant) * float(NOISE_C)


def interferer(v, start, n, mutant=None):
    v = np.asarray(v)
    i = np.arange(n, dtype=np.int64)
    if mutant == "wrap_off_by_one":
        return v[(start + i) % max(len(v) - 1, 1)]
    return v[(start + i) % len(v)]


def mix(x, g_white, g_babble, v, start, seed, step, uid, mutant=None, tail=0):
    """float64 y of the definition for one clip.  g_white / g_babble: the fp32-rounded gains (0 = off); v: the interferer
    (None = off).  `tail`: the trailing samples the resampler zeroed (the power_without_tail mutant leaves them out of
    the mean).  Mutants snr_sign and q_dropped need the SNR and Q: pass them through `mutant=(name, snr_w, snr_b, Q)`."""
    name = mutant[0] if isinstance(mutant, tuple) else mutant
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    gw, gb = float(np.float32(g_white)), float(np.float32(g_babble))
    if name == "snr_sign":
        _, snr_w, snr_b, Q = mutant
        gw = float(np.float32(10.0 ** (snr_w / 10.0))) if gw else 0.0
        gb = float(np.float32(10.0 ** (snr_b / 10.0) / Q)) if gb else 0.0
    if name == "q_dropped":
        gb = float(np.float32(10.0 ** (-mutant[2] / 10.0))) if gb else 0.0
    m = n - tail if name == "power_without_tail" else n
    P = float(np.sum(x * x) / m)
    if P == 0.0:
        return x.copy()
    bab = np.sqrt(P * gb) * interferer(v, start, n, name).astype(np.float64) if gb else 0.0
    if name == "white_scaled_after_babble":
        # the babble goes in first and the white noise is scaled to the power of the sum: two additions in the other
        # order differ by a rounding only, which no bound sees; this is the form of the mistake that shows
        x = x + bab
        return x + (np.sqrt(float(np.sum(x * x) / m) * gw) * noise(seed, step, uid, n, name) if gw else 0.0)
    white = np.sqrt(P * gw) * noise(seed, step, uid, n, name) if gw else 0.0
    return (x + white) + bab


def _butterfly(v):
    """the xor butterfly over 64 fp32 lanes (offsets 32 .. 1): every lane ends with the same sum; lane 0's is returned"""
    v = np.asarray(v, dtype=np.float32).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    return v[0]


def power_sum_f32(x):
    """S_b in the kernel's documented order, np.float32"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    nruns = -(-n // RUN)
    sq = np.zeros(nruns * RUN, dtype=np.float32)
    sq[:n] = x * x
    sq = sq.reshape(nruns, 8, 256, 4)                      # run, step k, thread j, lane c
    acc = np.zeros((nruns, 256, 4), dtype=np.float32)
    for k in range(8):
        acc = acc + sq[:, k]
    t = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])      # [nruns][256]
    runs = np.zeros(-(-nruns // 64) * 64, dtype=np.float32)
    for r in range(nruns):
        w = [_butterfly(t[r, 64 * k:64 * k + 64]) for k in range(4)]
        runs[r] = ((w[0] + w[1]) + w[2]) + w[3]
    lanes = np.zeros(64, dtype=np.float32)
    for k in range(len(runs) // 64):
        lanes = lanes + runs[64 * k:64 * k + 64]
    return _butterfly(lanes)


def mix_f32(x, g_white, g_babble, v, start, seed, step, uid, power=None):
    """fp32 y as the kernel computes it: every product and sum rounded on its own; `power` overrides P_b"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    gw, gb = np.float32(g_white), np.float32(g_babble)
    P = np.float32(power) if power is not None else power_sum_f32(x) / np.float32(n)
    if P == 0:
        return x.copy()
    y = x.copy()
    if gw != 0:
        e = noise_int(seed, step, uid, n).astype(np.float32) * NOISE_C
        y = y + np.sqrt(P * gw) * e
    if gb != 0:
        y = y + np.sqrt(P * gb) * interferer(v, start, n).astype(np.float32)
    assert y.dtype == np.float32
    return y


def rel_err(got, ref):
    return resample_ref.rel_err(got, ref)


# ---- the kernel cases of the GPU suite (tests/test_waveaug_gpu.py); tests/test_waveaug_cpu.py runs the mutants on them -----
CASE_LENS = (1, 255, 1024, 1025, 3 * 1024 + 5)
CASE_SEED, CASE_STEP = 0x123456789ABCDEF, 2 ** 32 + 3
CASE_SNR_WHITE, CASE_SNR_BABBLE = 10.0, 5.0
POOL_LENS = (700, 3, 2048, 1, 1500)
ZERO_CLIP = 2          # all zeros: must come back untouched
TAIL = 16              # trailing zeros of the last clip, as the resampler's zero tail


def case_pool():
    """(pool float32, offsets int64 in floats (each a multiple of 4), lens, Q float64)"""
    rng = np.random.RandomState(4321)
    clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in POOL_LENS]
    offs, at = [], 0
    for c in clips:
        offs.append(at)
        at += (len(c) + 3) // 4 * 4
    pool = np.zeros(at, dtype=np.float32)
    for o, c in zip(offs, clips):
        pool[o:o + len(c)] = c
    q = np.array([np.mean(c.astype(np.float64) ** 2) for c in clips])
    return pool, np.array(offs, dtype=np.int64), np.array(POOL_LENS, dtype=np.int64), q


def case_batch():
    """The ragged batch: dict(clips (list of float32), offsets (floats inside a buffer of `size`, guard bands of 64 around
    and between), src / start per clip, uid).  Clip 1 starts 4 floats off a 64-byte boundary and clip 3 one float off a
    16-byte boundary; clip 2 is all zeros; clip 4's interferer (3 samples) wraps a thousand times and its tail is zero;
    clip 3 starts at its interferer's last sample."""
    rng = np.random.RandomState(99)
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in CASE_LENS]
    clips[ZERO_CLIP][:] = 0
    clips[4][-TAIL:] = 0
    src = [0, 2, 4, 2, 1]
    start = [699, 5, 0, POOL_LENS[2] - 1, 2]
    offsets, at = [], 64
    for b, c in enumerate(clips):
        at = (at + 15) // 16 * 16 + (4 if b == 1 else 1 if b == 3 else 0)
        offsets.append(at)
        at += len(c) + 64
    return dict(clips=clips, offsets=np.array(offsets, dtype=np.int64), size=at, src=src, start=start,
                uid=[7, 0, 2 ** 32 - 1, 3, 11])


def case_gains(q):
    """(g_white, g_babble per clip) float32 at the case's SNRs"""
    b = case_batch()
    gw = np.float32(10.0 ** (-CASE_SNR_WHITE / 10.0))
    return gw, [np.float32(10.0 ** (-CASE_SNR_BABBLE / 10.0) / q[j]) for j in b["src"]]
