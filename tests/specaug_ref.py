"""numpy restatement of s2i_specaug as include/s2i_hip.h words it: Philox4x32-10 in uint32 / uint64 arithmetic, the mask
geometry in integers with the one fp32 multiply done in np.float32, the masked value in float64.  Written from the
header's text, not from the kernel."""
import numpy as np

BINS = 40
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# Random123's known-answer vectors for philox4x32 with 10 rounds (counter, key, output), as torch's own
# at::philox_engine (ATen/core/PhiloxRNGEngine.h) reproduces them
PHILOX_KAT = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    c = [np.uint64(int(v) & MASK32) for v in counter]
    k = [int(key[0]) & MASK32, int(key[1]) & MASK32]
    for r in range(10):
        p0 = np.uint64(M0) * c[0]          # < 2^64: no wrap
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
        if r < 9:
            k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
    return tuple(int(v) for v in c)


def uniforms(seed, step, b, count):
    """u_0 .. u_{count-1} of utterance b as np.float32."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    out = []
    for g in range((count + 3) // 4):
        words = philox4x32_10((step & MASK32, step >> 32, b, g), (seed & MASK32, seed >> 32))
        out += [np.float32(w >> 8) * np.float32(2.0 ** -24) for w in words]
    return out[:count]


def _draw(u, n):
    return min(int(np.float32(u) * np.float32(n)), n - 1)


def masks(policy, seed, step, b, n):
    """([(f0, f1)] bins, [(t0, t1)] rows), half-open, of utterance b with n rows the masks may touch."""
    fm, fw, tm, tw, ratio = policy
    u = uniforms(seed, step, b, 2 * (fm + tm))
    freq, time = [], []
    for k in range(fm):
        f = _draw(u[2 * k], fw + 1)
        f0 = _draw(u[2 * k + 1], BINS - f + 1)
        freq.append((f0, f0 + f))
    for k in range(fm, fm + tm):
        W = min(tw, int(np.float32(ratio) * np.float32(n)))
        t = _draw(u[2 * k], W + 1)
        t0 = _draw(u[2 * k + 1], n - t + 1)
        time.append((t0, t0 + t))
    return freq, time


def mask_array(policy, seed, step, b, n, T):
    """bool [T, 40]: the cells of utterance b that take the mean."""
    freq, time = masks(policy, seed, step, b, n)
    m = np.zeros((T, BINS), dtype=bool)
    for f0, f1 in freq:
        m[:n, f0:f1] = True
    for t0, t1 in time:
        m[t0:t1, :] = True
    assert not m[n:].any()
    return m


def specaug(x, valid, policy, seed, step):
    """x [B, T, 40] -> (y float64 [B, T, 40], mask bool [B, T, 40], mean float64 [B])."""
    x = np.asarray(x)
    B, T, _ = x.shape
    y = x.astype(np.float64).copy()
    mask = np.zeros(x.shape, dtype=bool)
    mean = np.zeros(B)
    for b in range(B):
        n = int(valid[b])
        mask[b] = mask_array(policy, seed, step, b, n, T)
        if n > 0:
            mean[b] = x[b, :n].astype(np.float64).mean()
        y[b][mask[b]] = mean[b]
    return y, mask, mean


def segments(T):
    return min(64, max(1, 10 * T // 1024))


def depth(T):
    """d(T) of the header: the most additions a term of the utterance sum passes through."""
    chunk = -(-10 * T // segments(T))
    return -(-chunk // 256) + 17


def mean_bound(T, mean_abs):
    """|m_b - float64 mean| <= (d + 2) 2^-24 mean|x_b|: d additions of a same-sign sum, the division, and one unit for the
    higher-order terms."""
    return (depth(T) + 2) * 2.0 ** -24 * mean_abs


# The inputs of the GPU suite's kernel cases (tests/test_specaug_gpu.py); tests/test_specaug_cpu.py asserts that each
# yields a frequency mask and a time mask of width >= 1 in every utterance with valid >= 64 (case D: a frequency mask).
POLICY_A = (2, 8, 2, 20, 0.2)
CASES = {
    "A": dict(B=3, T=128, valid=[128, 64, 64], policy=POLICY_A, seed=11, step=0),
    "B": dict(B=5, T=128, valid=[128, 0, 64, 128, 64], policy=POLICY_A, seed=12, step=3),
    "C": dict(B=2, T=2048, valid=[2048, 1984], policy=(2, 8, 2, 40, 0.2), seed=13, step=2 ** 32 + 5),
    "D": dict(B=2, T=128, valid=[64, 64], policy=(2, 8, 2, 20, 0.01), seed=14, step=1),
    "E": dict(B=2, T=128, valid=[128, 64], policy=(8, 20, 8, 128, 1.0), seed=15, step=7),
}
TRAINER = dict(spec="freq=2x8,time=2x20,ratio=0.2", seed=21, steps=4)
TRAINER_ORDER = [2, 0, 3, 1]


def trainer_batch():
    """(mel fp32 [4, 1, 128, 40], cap_lens, image, label) of the trainer tests: encoder_conv_train_ref.trainer_case() with
    its utterances taken out of length order, so that the trainer's sort moves them and `b` is seen to be the caller's."""
    import encoder_conv_train_ref
    import torch
    mel, lens, image, label = encoder_conv_train_ref.trainer_case()
    order = torch.tensor(TRAINER_ORDER)
    return mel.float()[order].contiguous(), [lens[i] for i in TRAINER_ORDER], image.float()[order], label[order]


def case_input(name):
    """The case's batch, uniform in [-80, 0], fp32 [B, T, 40]."""
    c = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)) + 1000)
    return rng.uniform(-80.0, 0.0, size=(c["B"], c["T"], BINS)).astype(np.float32)
