"""SpecAugment of the speech-encoder batches, CPU side: the policy parser, the numpy restatement's invariants and its
generator's known answers, the header / binding / argument checks of s2i_specaug (callable without a device), the CLI
plumbing, and the non-vacuity of the inputs the GPU suite uses."""
import argparse
import ctypes
import os
import random
import re

import numpy as np
import pytest

import specaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ops.specaug_policy --------------------------------------------------------------------------------------------------
def test_policy_three_keys_subsets_and_off():
    from speech_to_image_translation_without_text_amd import ops
    assert ops.specaug_policy("freq=2x8,time=2x40,ratio=0.2") == (2, 8, 2, 40, 0.2)
    assert ops.specaug_policy(" time=3x100 , freq=1x20 ") == (1, 20, 3, 100, 1.0)      # any order, ratio defaults to 1
    assert ops.specaug_policy("freq=2x8") == (2, 8, 0, 0, 1.0)
    assert ops.specaug_policy("time=8x0,ratio=1") == (0, 0, 8, 0, 1.0)
    assert ops.specaug_policy("ratio=0.5") == (0, 0, 0, 0, 0.5)
    assert ops.specaug_policy("") is None and ops.specaug_policy(" , ") is None


@pytest.mark.parametrize("spec,token", [
    ("freq=2x8,pitch=1x2", "pitch=1x2"),            # unknown key
    ("freq", "freq"),                               # no value
    ("freq=2", "freq=2"),                           # no width
    ("freq=2x", "freq=2x"),
    ("freq=axb", "freq=axb"),
    ("time=2.5x4", "time=2.5x4"),                   # not integers
    ("freq=9x8", "freq=9x8"),                       # more than 8 masks
    ("time=-1x8", "time=-1x8"),
    ("freq=2x21", "freq=2x21"),                     # wider than 20 bins
    ("time=2x-3", "time=2x-3"),
    ("ratio=0", "ratio=0"),
    ("ratio=1.5", "ratio=1.5"),
    ("ratio=nan", "ratio=nan"),
    ("ratio=big", "ratio=big"),
    ("freq=1x2,freq=2x2", "freq=2x2"),              # twice
])
def test_policy_names_the_malformed_token(spec, token):
    from speech_to_image_translation_without_text_amd import ops
    with pytest.raises(ValueError) as e:
        ops.specaug_policy(spec)
    assert repr(token) in str(e.value)


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, out in R.PHILOX_KAT:
        assert R.philox4x32_10(counter, key) == out


def test_uniforms_are_24_bit_fractions_of_the_counter_block():
    u = R.uniforms(seed=(0x299f31d0 << 32) | 0xa4093822, step=(0x85a308d3 << 32) | 0x243f6a88, b=0x13198a2e, count=3)
    # the header's layout: key (seed lo, seed hi), counter (step lo, step hi, b, group)
    words = R.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    assert [float(v) for v in u] == [(w >> 8) / 2.0 ** 24 for w in words[:3]]
    assert all(v.dtype == np.float32 and 0.0 <= v < 1.0 for v in u)
    five = R.uniforms(1, 2, 3, 5)
    assert float(five[4]) == (R.philox4x32_10((2, 0, 3, 1), (1, 0))[0] >> 8) / 2.0 ** 24      # group 1 starts u_4


def test_reference_invariants_over_200_triples():
    rng = random.Random(20260101)
    policy = (2, 8, 2, 40, 0.2)
    T = 2048
    changed = 0
    for i in range(200):
        seed, step, b = rng.getrandbits(64), rng.getrandbits(rng.choice([3, 20, 40])), rng.randrange(64)
        for n in (0, 64, 128, 2048):
            freq, time = R.masks(policy, seed, step, b, n)
            assert len(freq) == 2 and len(time) == 2
            for f0, f1 in freq:
                assert 0 <= f0 <= f1 <= 40 and f1 - f0 <= 8
            limit = min(40, int(np.floor(np.float32(0.2) * np.float32(n))))
            for t0, t1 in time:
                assert 0 <= t0 <= t1 <= n and t1 - t0 <= limit
            assert (freq, time) == R.masks(policy, seed, step, b, n)                  # the same triple, the same masks
            m = R.mask_array(policy, seed, step, b, n, T)
            assert not m[n:].any()                                                    # nothing at or after `valid`
            if n == 0:
                assert not m.any()
        changed += R.masks(policy, seed, step, b, 2048) != R.masks(policy, seed, step + 1, b, 2048)
    # two steps give different masks: all eight draws of the 2048-row utterance would have to coincide
    assert changed == 200


def test_reference_leaves_unmasked_cells_and_writes_the_mean():
    x = R.case_input("A")
    c = R.CASES["A"]
    y, mask, mean = R.specaug(x, c["valid"], c["policy"], c["seed"], c["step"])
    assert np.array_equal(y[~mask], x[~mask].astype(np.float64))
    for b, n in enumerate(c["valid"]):
        assert np.all(y[b][mask[b]] == mean[b]) and mean[b] == x[b, :n].astype(np.float64).mean()
    assert R.depth(128) == 22 and R.depth(2048) == 21 and R.segments(2048) == 20 and R.segments(128) == 1


def test_gpu_suite_inputs_are_not_vacuous():
    """For the exact (seed, step, shapes, policy) the GPU tests use, every utterance with valid >= 64 gets a frequency
    mask and (where the policy admits one: not case D, whose W is 0) a time mask at least one wide."""
    for name, c in R.CASES.items():
        for b, n in enumerate(c["valid"]):
            freq, time = R.masks(c["policy"], c["seed"], c["step"], b, n)
            if n >= 64:
                assert max(f1 - f0 for f0, f1 in freq) >= 1, (name, b)
                if name == "D":
                    assert all(t1 == t0 for t0, t1 in time), (name, b)
                else:
                    assert max(t1 - t0 for t0, t1 in time) >= 1, (name, b)
            else:
                assert not R.mask_array(c["policy"], c["seed"], c["step"], b, n, c["T"]).any()
    # case A's ragged rows: floor(0.2 * 64) = 12 binds, not 20
    for b in (1, 2):
        assert all(t1 - t0 <= 12 for t0, t1 in R.masks(R.POLICY_A, R.CASES["A"]["seed"], R.CASES["A"]["step"], b, 64)[1])
    t = R.TRAINER
    from speech_to_image_translation_without_text_amd import ops
    policy = ops.specaug_policy(t["spec"])
    mel, cap_lens, _, _ = R.trainer_batch()
    assert tuple(mel.shape) == (4, 1, 128, 40) and cap_lens != sorted(cap_lens, reverse=True) and min(cap_lens) >= 1
    for step in range(t["steps"]):
        for b, n in enumerate(cap_lens):
            freq, time = R.masks(policy, t["seed"], step, b, 64 * n)
            assert max(f1 - f0 for f0, f1 in freq) >= 1 and max(t1 - t0 for t0, t1 in time) >= 1, (step, b)


# ---- header, binding, argument checks ------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    from speech_to_image_translation_without_text_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    assert re.search(r"size_t s2i_specaug_workspace_bytes\(int B\);", header)
    decl = re.search(r"int s2i_specaug\(([^)]*)\)", header)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == [
        "const float* x", "const int* valid", "int B", "int T", "float* y", "int freq_masks", "int freq_width",
        "int time_masks", "int time_width", "float time_ratio", "unsigned long long seed", "unsigned long long step",
        "void* ws", "size_t ws_bytes", "void* stream"]
    assert "s2i_specaug" in _lib.EXPORTED_SYMBOLS and "s2i_specaug_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    assert "s2i_specaug.hip" in open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    lib = _lib.load()
    assert lib.s2i_version() == 7
    assert lib.s2i_specaug_workspace_bytes(0) == 0 and lib.s2i_specaug_workspace_bytes(3) >= 3 * 4


def test_bad_arguments_return_non_zero_before_any_launch():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    # host memory stands in for the device buffers: every call here is refused before a launch could read them
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    x = base + (-base) % 16
    valid = (ctypes.c_int * 1)(1)
    v = ctypes.addressof(valid)
    ws_bytes = lib.s2i_specaug_workspace_bytes(1)

    def call(x=x, valid=v, B=1, T=1, y=x, fm=1, fw=8, tm=1, tw=8, ratio=1.0, ws=x, ws_bytes=ws_bytes):
        rc = lib.s2i_specaug(x, valid, B, T, y, fm, fw, tm, tw, ratio, 1, 2, ws, ws_bytes, None)
        return rc, lib.s2i_last_error()

    for kw, word in [(dict(x=None), b"null"), (dict(valid=None), b"null"), (dict(y=None), b"null"),
                     (dict(B=0), b"bad shape"), (dict(T=0), b"bad shape"), (dict(T=2 ** 24), b"too large"),
                     (dict(x=x + 4), b"aligned"), (dict(y=x + 8), b"aligned"),
                     (dict(fm=9), b"mask counts"), (dict(fm=-1), b"mask counts"), (dict(tm=9), b"mask counts"),
                     (dict(fw=21), b"freq_width"), (dict(fw=-1), b"freq_width"), (dict(tw=-1), b"time_width"),
                     (dict(ratio=0.0), b"time_ratio"), (dict(ratio=1.5), b"time_ratio"), (dict(ratio=float("nan")), b"time_ratio"),
                     (dict(ws=None), b"workspace"), (dict(ws_bytes=ws_bytes - 1), b"workspace")]:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith(b"specaug:") and word in msg, (kw, rc, msg)
    # no masks and x == y: nothing to do, and no workspace needed
    assert lib.s2i_specaug(x, v, 1, 1, x, 0, 0, 0, 0, 1.0, 0, 0, None, 0, None) == 0


# ---- CLI plumbing --------------------------------------------------------------------------------------------------------
def test_parsers_accept_specaug_and_check_args_rejects_a_bad_spec():
    from speech_to_image_translation_without_text_amd import train_encoder, train_encoder_head
    for mod, argv in ((train_encoder_head, ["--model", "m.pt"]), (train_encoder, [])):
        args = mod.get_parser().parse_args(argv)
        assert args.specaug == ""
        train_encoder_head.check_args(args)
        assert train_encoder_head.trainer_kwargs(args)["specaug"] == ""
        args = mod.get_parser().parse_args(argv + ["--specaug", "freq=2x8,time=2x40,ratio=0.2", "--seed", "7"])
        train_encoder_head.check_args(args)
        kw = train_encoder_head.trainer_kwargs(args)
        assert kw["specaug"] == "freq=2x8,time=2x40,ratio=0.2" and kw["specaug_seed"] == 7
        with pytest.raises(SystemExit) as e:
            train_encoder_head.check_args(mod.get_parser().parse_args(argv + ["--specaug", "freq=2x80"]))
        assert "freq=2x80" in str(e.value)
    assert train_encoder.check_args is train_encoder_head.check_args


def test_trainer_kwargs_works_without_the_field():
    from speech_to_image_translation_without_text_amd import train_encoder_head
    args = train_encoder_head.get_parser().parse_args(["--model", "m.pt"])
    old = argparse.Namespace(**{k: v for k, v in vars(args).items() if k != "specaug"})
    assert not hasattr(old, "specaug")
    train_encoder_head.check_args(old)
    kw = train_encoder_head.trainer_kwargs(old)
    assert kw["specaug"] == "" and kw["specaug_seed"] == 0          # the head CLI's --seed defaults to None


def test_trainer_signature_defaults_to_off():
    import inspect
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer, HeadTrainer
    sig = inspect.signature(HeadTrainer.__init__).parameters
    assert sig["specaug"].default == "" and sig["specaug_seed"].default == 0
    assert EncoderTrainer.__init__ is HeadTrainer.__init__
