"""Host side of the waveform augmentation: the policy grammar, the package's Philox against Random123's vectors and the
SpecAugment reference, every bucket boundary of the integer draws, the speed fallback, the feeder's `random` calls, the
reference's own SNR definition, and the mutants the GPU suite's bound must be able to see.  No GPU."""
import os
import random
import re

import numpy as np
import pytest
import torch

import specaug_ref
import waveaug_ref as ref
from speech_loader_ref import make_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = "speed=0.9/1.0/1.1,white=0.3@5:25,babble=0.2@0:15"


def _ops():
    from speech_to_image_translation_without_text_amd import ops
    return ops


# ---- policy grammar -------------------------------------------------------------------------------------------------------
def test_policy_accepts():
    ops = _ops()
    assert ops.waveaug_policy("") is None and ops.waveaug_policy(" , ") is None
    assert ops.waveaug_policy(SPEC) == {"rates": (14400, 16000, 17600), "white": (0.3, 5.0, 25.0), "babble": (0.2, 0.0, 15.0)}
    assert ops.waveaug_policy("babble=1@5:5 , speed=1.0") == {"rates": (16000,), "white": None, "babble": (1.0, 5.0, 5.0)}
    assert ops.waveaug_policy("white=1@-5:0")["white"] == (1.0, -5.0, 0.0)
    assert ops.waveaug_policy("speed=0.5/2.0")["rates"] == (8000, 32000)
    assert len(ops.waveaug_policy("speed=" + "/".join(["1.0"] * 8))["rates"]) == 8


@pytest.mark.parametrize("spec,word", [
    ("gain=2", "gain=2"), ("speed", "speed"), ("white=0.3@5:25,white=0.1@0:1", "white=0.1@0:1"),
    ("speed=", "speed="), ("speed=0.4", "speed=0.4"), ("speed=2.5", "speed=2.5"), ("speed=fast", "fast"),
    ("speed=0.90001", "speed=0.90001"), ("speed=" + "/".join(["1.0"] * 9), "1 to 8"),
    ("white=0@5:25", "white=0@5:25"), ("white=1.5@5:25", "white=1.5@5:25"), ("white=0.5@25:5", "white=0.5@25:5"),
    ("white=0.5", "white=0.5"), ("white=0.5@5", "white=0.5@5"), ("babble=nan@0:1", "babble=nan@0:1"),
    ("babble=0.5@0:inf", "babble=0.5@0:inf"), ("white=x@1:2", "white=x@1:2"),
])
def test_policy_refuses_with_the_offending_token(spec, word):
    with pytest.raises(ValueError) as e:
        _ops().waveaug_policy(spec)
    assert word in str(e.value)


def test_the_docstring_says_why_there_is_no_gain_key():
    doc = _ops().waveaug_policy.__doc__
    assert "no gain key" in doc and "invariant" in doc


# ---- Philox -------------------------------------------------------------------------------------------------------------------
def test_philox_known_answer_vectors():
    ops = _ops()
    for counter, key, out in specaug_ref.PHILOX_KAT:
        assert tuple(int(v) for v in ops.philox4x32_10(*counter, *key)) == out
        assert tuple(int(v) for v in ref.philox4x32_10(*counter, *key)) == out
        assert specaug_ref.philox4x32_10(counter, key) == out
    # arrays of counters: each column is the scalar result
    c2 = np.array([0, 1, 2 ** 32 - 1, 77])
    got = ops.philox4x32_10(5, 6, c2, 9, 0xDEADBEEF, 0x12345678)
    for n, uid in enumerate(c2):
        assert tuple(int(v) for v in got[:, n]) == specaug_ref.philox4x32_10((5, 6, int(uid), 9), (0xDEADBEEF, 0x12345678))


@pytest.mark.parametrize("seed", [0, 11, 2 ** 32 + 5, 2 ** 64 - 1, ref.KEY_XOR << 32])
def test_no_block_is_shared_with_specaugment(seed):
    """Same (seed, step, b): SpecAugment's key is (seed lo, seed hi), this one's (seed lo, seed hi ^ KEY_XOR); a Philox block
    is a bijection of the counter under one key, and the keys differ in word 1 for every seed."""
    ops = _ops()
    assert ops.WAVEAUG_KEY_XOR == ref.KEY_XOR != 0
    step, b = 2 ** 32 + 3, 4
    k = ref.key(seed)
    assert k != (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF) and k[0] == seed & 0xFFFFFFFF
    for g in range(4):
        sa = specaug_ref.philox4x32_10((step & 0xFFFFFFFF, step >> 32, b, g), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        wa = tuple(int(v) for v in ref.philox4x32_10(*ref.counter(step, b, g), *k))
        assert sa != wa and not set(sa) & set(wa)
        # and the package draws its uniforms from this module's blocks
        u = ops.waveaug_uniforms(seed, step, [b], g)[:, 0]
        assert [float(v) for v in u] == [float(v) for v in ref.uniforms(seed, step, b, g)]
        assert [float(v) for v in u] != [float(v) for v in specaug_ref.uniforms(seed, step, b, 4 * g + 4)[4 * g:]]


# ---- integer draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 7, 1, 1023, 1024, 1025])
def test_integer_draws_on_both_sides_of_every_bucket_boundary(n):
    """K = 3 speeds, a pool of 7 utterances, n_j in {1, 1023, 1024, 1025}: for every boundary k / n the largest u whose
    bucket is k - 1 and the smallest whose bucket is k, found on the 2^-24 grid from the fp32 product itself."""
    ops = _ops()
    grid = np.float32(2.0 ** -24)
    for k in range(1, n):
        m = int(np.ceil(k * 2.0 ** 24 / n))
        lo = next(j for j in range(m - 3, m + 4) if int(np.float32(j) * grid * np.float32(n)) >= k)   # first u in bucket k
        for j, want in ((lo - 1, k - 1), (lo, k)):
            u = np.float32(j) * grid
            assert ref.draw(u, n) == want
            assert int(ops._waveaug_index(np.array([u]), np.array([n]))[0]) == want
    top = np.float32(2 ** 24 - 1) * grid
    assert ref.draw(top, n) == n - 1 == int(ops._waveaug_index(np.array([top]), np.array([n]))[0])
    assert ref.draw(np.float32(0), n) == 0


def test_plan_equals_the_reference_plan():
    ops = _ops()
    policy = ops.waveaug_policy(SPEC)
    pool_lens = np.array([1, 1023, 1024, 1025, 20000, 12000, 16000])
    pool_q = np.array([0.01, 0.02, 0.0, 0.04, 0.05, 0.06, 0.07])
    lens = np.array([10240, 11263, 30000, 16000, 12345, 10240, 48000, 20000] * 8)
    uids = np.arange(len(lens))
    seen = set()
    for seed, step in ((1, 0), (2 ** 40 + 7, 2 ** 33 + 1)):
        plan = ops.waveaug_plan(policy, seed, step, uids, lens, pool_lens, pool_q, 2048)
        for b in range(len(lens)):
            one = ref.plan_one(policy, seed, step, b, lens[b], pool_lens, pool_q, 2048)
            assert plan["rate"][b] == one["rate"] and plan["out_len"][b] == one["out_len"]
            assert plan["g_white"][b] == np.float32(one["g_white"]) and plan["g_babble"][b] == np.float32(one["g_babble"])
            if one["g_babble"]:
                assert plan["src"][b] == one["src"] and plan["start"][b] == one["start"] < pool_lens[one["src"]]
            for name in ("white_snr", "babble_snr"):
                assert (one[name] is None and np.isnan(plan[name][b])) or plan[name][b] == one[name]
            seen.add((one["rate"], one["white_snr"] is not None, one["babble_snr"] is not None))
        assert np.all(plan["g_babble"][pool_q[plan["src"]] == 0] == 0)
    assert {r for r, _, _ in seen} == {14400, 16000, 17600} and len(seen) >= 8


def test_plan_leaves_random_and_torch_alone():
    ops = _ops()
    random.seed(5)
    torch.manual_seed(5)
    np.random.seed(5)
    states = random.getstate(), torch.get_rng_state(), np.random.get_state()[1].copy()
    ops.waveaug_plan(ops.waveaug_policy(SPEC), 3, 9, [0, 1], [16000, 20000], [16000], [0.1], 2048)
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    assert np.array_equal(np.random.get_state()[1], states[2])


# ---- speed fallback -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,speed,rate,out_len", [
    (10240, "1.1", 16000, 10240),      # 64 hops; at 1.1 it has 9310 samples, 59 frames: runs at 1.0
    (11263, "1.1", 17600, 10240),      # 70 hops; at 1.1 it has 10240 samples, 65 frames: stays at 1.1
    (11086, "1.1", 16000, 11086),      # the last length that falls back: 10079 samples, 63 frames
    (11087, "1.1", 17600, 10080),      # the first that does not: 10080 samples, 64 frames
    (10240, "0.9", 14400, 11378),      # slower is longer: no fallback
])
def test_speed_fallback(n, speed, rate, out_len):
    from speech_to_image_translation_without_text_amd import audio
    ops = _ops()
    policy = ops.waveaug_policy("speed=" + speed)          # 1.0 is not in the list
    plan = ops.waveaug_plan(policy, 1, 2, [0], [n])
    assert (int(plan["rate"][0]), int(plan["out_len"][0])) == (rate, out_len)
    one = ref.plan_one(policy, 1, 2, 0, n)
    assert (one["rate"], one["out_len"]) == (rate, out_len)
    assert audio.n_frames(out_len) >= 64
    assert (rate == 16000) == (audio.n_frames(audio.resampled_length(n, round(16000 * float(speed)))) < 64)


# ---- host draws ---------------------------------------------------------------------------------------------------------------
ITEM = [1.0, 0.3, 1.2, 0.7, 0.3, 1.5, 0.9, 0.3, 1.1, 0.8]


@pytest.fixture(scope="module")
def fake_set(tmp_path_factory):
    """a ResidentWaveSet without its pool: the draws need the split and the frame counts alone"""
    from speech_to_image_translation_without_text_amd import speech_loader, train_encoder_head, wave_loader
    root = str(tmp_path_factory.mktemp("wave_tree"))
    make_tree(root, "train", [ITEM[k:] + ITEM[:k] for k in range(6)], seed=3)
    split = train_encoder_head.SplitData(root, "train", "birds")
    ws = wave_loader.ResidentWaveSet.__new__(wave_loader.ResidentWaveSet)
    ws.split, ws.frames = split, speech_loader.scan_frames(split, workers=4)
    return split, ws


@pytest.mark.parametrize("shuffle", [False, True])
def test_draws_equal_split_datas_and_augmentation_leaves_random_alone(fake_set, shuffle):
    from speech_to_image_translation_without_text_amd import audio
    split, ws = fake_set
    ops = _ops()
    policy = ops.waveaug_policy(SPEC)
    for seed in range(4):
        random.seed(seed)
        order = list(range(len(split)))
        if shuffle:
            random.shuffle(order)
        host = []
        for i in order:
            image, wave, label = split.draw(i)
            host.append((image.tobytes(), len(wave), label))
        host_state = random.getstate()

        for augmented in (False, True):
            random.seed(seed)
            mine = []
            for items, drawn in ws.plan_batches(4, shuffle):
                for i, (image, u, label) in zip(items, drawn):
                    assert ws.frames[i][u] >= 64
                    mine.append((i, image.tobytes(), int(ws.frames[i][u]), label))
                if augmented:
                    ops.waveaug_plan(policy, seed, len(mine), np.arange(len(items)), [16000] * len(items), [16000, 9], [.1, .2])
            assert [i for i, _, _, _ in mine] == order
            assert [(v, f, c) for _, v, f, c in mine] == [(v, audio.n_frames(n), c) for v, n, c in host]
            assert random.getstate() == host_state


# ---- the reference's SNR definition ----------------------------------------------------------------------------------------
def test_babble_snr_is_the_drawn_one():
    rng = np.random.RandomState(1)
    x = rng.standard_normal(5000) * 0.2
    v = (rng.standard_normal(777) * 0.05).astype(np.float32)
    P, Q = np.mean(x * x), np.mean(v.astype(np.float64) ** 2)
    for snr in (-3.0, 0.0, 7.25, 15.0):
        g = 10.0 ** (-snr / 10.0) / Q
        a_b = np.sqrt(P * g)
        assert abs(10 * np.log10(P / (a_b ** 2 * Q)) - snr) < 1e-12
    one = ref.plan_one(_ops().waveaug_policy("babble=1@0:15"), 4, 5, 6, 5000, [777], [Q])
    a_b = np.sqrt(P * one["g_babble"])
    assert 0.0 <= one["babble_snr"] <= 15.0 and abs(10 * np.log10(P / (a_b ** 2 * Q)) - one["babble_snr"]) < 1e-12


def test_white_snr_over_65536_samples_within_the_irwin_hall_bound():
    """e is a sum of four uniform 16-bit integers, centred and scaled: variance 1 up to the rounding of c (1e-8), fourth
    moment 3 - (6 / 5) / 4 = 2.7 (a uniform's excess kurtosis, a quarter of it for the sum of four; the 16-bit grid
    moves it by 1e-9).  The mean of n squares has variance (mu4 - 1) / n, so
    the realised noise power sits within 6 standard deviations, 6 sqrt(1.7 / n), of its nominal value -- a fixed seed, so
    this checks arithmetic -- and the SNR within 10 log10 of that."""
    n = 2 ** 16
    e = ref.noise(0xABCDEF, 12, 34, n)
    assert abs(e).max() <= 3.4642 and abs(e.mean()) < 6 / np.sqrt(n)
    mu4 = 3.0 - 6.0 / 5.0 / 4.0            # excess kurtosis of a uniform is -6/5, of the sum of four a quarter of it
    bound = 6.0 * np.sqrt((mu4 - 1.0) / n)
    assert abs(np.mean(e * e) - 1.0) < bound
    assert abs(np.mean(e ** 4) - mu4) < 0.1
    rng = np.random.RandomState(2)
    x = 0.1 * rng.standard_normal(n)
    for snr in (5.0, 20.0):
        g = np.float32(10.0 ** (-snr / 10.0))
        y = ref.mix(x, g, 0.0, None, 0, 0xABCDEF, 12, 34)
        got = 10 * np.log10(np.mean(x * x) / np.mean((y - x) ** 2))
        assert abs(got - snr) < -10 * np.log10(1.0 - bound) + 1e-6, (got, snr)


# ---- the cases of the GPU suite and their mutants -------------------------------------------------------------------------------
def case_outputs(mutant=None):
    """(float64 reference, fp32 restatement) of the GPU suite's batch, all clips concatenated, white + babble"""
    pool, offs, lens, q = ref.case_pool()
    b = ref.case_batch()
    gw, gb = ref.case_gains(q)
    out64, out32 = [], []
    for c, (x, j, s, uid) in enumerate(zip(b["clips"], b["src"], b["start"], b["uid"])):
        v = pool[offs[j]:offs[j] + lens[j]]
        m = (mutant, ref.CASE_SNR_WHITE, ref.CASE_SNR_BABBLE, q[j]) if mutant in ("snr_sign", "q_dropped") else mutant
        out64.append(ref.mix(x, gw, gb[c], v, s, ref.CASE_SEED, ref.CASE_STEP, uid, mutant=m,
                             tail=ref.TAIL if c == 4 else 0))
        out32.append(ref.mix_f32(x, gw, gb[c], v, s, ref.CASE_SEED, ref.CASE_STEP, uid))
    return np.concatenate(out64), np.concatenate(out32)


def test_the_cases_are_what_the_gpu_suite_says():
    pool, offs, lens, q = ref.case_pool()
    b = ref.case_batch()
    assert [len(c) for c in b["clips"]] == [1, 255, 1024, 1025, 3 * 1024 + 5]
    assert b["offsets"][1] % 16 == 4 and b["offsets"][3] % 4 == 1 and b["offsets"][0] % 4 == 0
    assert not b["clips"][ref.ZERO_CLIP].any()
    assert lens[b["src"][4]] == 3 and len(b["clips"][4]) > 1000 * 3            # wraps several times
    assert b["start"][3] == lens[b["src"][3]] - 1                                 # the interferer's last sample
    assert np.all(offs % 4 == 0) and np.all(q > 0)
    ends = b["offsets"] + [len(c) for c in b["clips"]]
    assert np.all(b["offsets"][1:] - ends[:-1] >= 64) and b["offsets"][0] >= 64 and b["size"] - ends[-1] >= 64


def test_fp32_restatement_is_at_rounding_level_and_every_mutant_is_far_outside_the_bound():
    want, f32 = case_outputs()
    yardstick = ref.rel_err(f32, want)
    assert 0 < yardstick < 4 * 2.0 ** -24
    bound = 2 * yardstick
    for name in ref.MUTANTS:
        moved = ref.rel_err(case_outputs(name)[0], want)
        print("%s moves the reference by %.3g = %.0f bounds" % (name, moved, moved / bound))
        assert moved >= 100 * bound, name
    assert len(ref.MUTANTS) >= 6


def test_zero_clip_and_zero_power():
    x = np.zeros(100, dtype=np.float32)
    assert np.array_equal(ref.mix(x, 0.1, 0.1, np.ones(3, np.float32), 0, 1, 2, 3), x)
    assert np.array_equal(ref.mix_f32(x, 0.1, 0.1, np.ones(3, np.float32), 0, 1, 2, 3), x)


def test_power_sum_order_is_a_sum():
    rng = np.random.RandomState(3)
    for n in (1, 255, 8192, 8193, 70000):
        x = rng.standard_normal(n).astype(np.float32)
        exact = np.sum(x.astype(np.float64) ** 2)
        assert abs(float(ref.power_sum_f32(x)) - exact) <= 32 * 2.0 ** -24 * exact


# ---- the entry points -----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_refuse_bad_arguments_without_a_gpu():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    for name in ("s2i_wave_mix", "s2i_wave_mix_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    makefile = open(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc", "Makefile")).read()
    assert "s2i_waveaug.hip" in makefile
    assert lib.s2i_version() == _lib.ABI_VERSION == 7
    assert lib.s2i_wave_mix_workspace_bytes(5, 8192) == 20 and lib.s2i_wave_mix_workspace_bytes(5, 8193) == 40
    assert lib.s2i_wave_mix_workspace_bytes(0, 100) == 0 and lib.s2i_wave_mix_workspace_bytes(1, 2 ** 31 - 4) == 0
    ok = dict(x=4096, off=8192, lens=12288, B=2, max_len=100, pool=16384, table=20480, ws=24576, ws_bytes=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.s2i_wave_mix(a["x"], a["off"], a["lens"], a["B"], a["max_len"], a["pool"], a["table"], 1, 2, a["ws"],
                                a["ws_bytes"], None)
    for bad, word in ((dict(x=None), b"null"), (dict(off=None), b"null"), (dict(lens=None), b"null"),
                      (dict(table=None), b"null"), (dict(B=0), b"clip count"), (dict(max_len=0), b"max_len"),
                      (dict(max_len=2 ** 31 - 4), b"2^31 - 4"), (dict(x=4100), b"aligned"), (dict(pool=16388), b"aligned"),
                      (dict(table=20488), b"aligned"), (dict(ws=None), b"workspace"), (dict(ws_bytes=4), b"workspace")):
        assert call(**bad) != 0, bad
        assert word in lib.s2i_last_error(), (bad, lib.s2i_last_error())


def test_wave_mix_refuses_cpu_tensors_and_bad_tables():
    from speech_to_image_translation_without_text_amd import _lib
    ops = _ops()
    table = np.zeros(1, dtype=ops.WAVE_MIX_ENTRY)
    assert table.itemsize == 32
    with pytest.raises(_lib.S2IError):
        ops.wave_mix(torch.zeros(8), [0], [8], table, 1, 2)
