"""CPU checks of the WAV -> 16 kHz path: the plan, table and length rules of audio.py against the fp64 restatement
(tests/resample_ref.py), the restatement's own sanity (tones, tap sums, mutants), the RIFF reader, decode and mixdown,
the table's device layout, the C-ABI's argument checks and the four CLIs' --resample flag."""
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 12345, 16000, 22050, 24000, 32000, 44100, 48000, 96000)


# ---- plans, tables, lengths -----------------------------------------------------------------------------------------
def test_resample_plan_at_the_listed_rates():
    from speech_to_image_translation_without_text_amd import audio
    for rate in RATES:
        L, M, W, taps = audio.resample_plan(rate)
        assert (L, M, W, taps) == R.plan(rate), rate
        if rate != 16000:
            assert L * rate == M * 16000 and np.gcd(L, M) == 1
            assert W == int(np.ceil(64 / min(1.0, L / M) - 1e-9)) and taps == 2 * W + 2
    assert audio.resample_plan(44100) == (160, 441, 177, 356)
    assert audio.resample_plan(48000) == (1, 3, 192, 386)
    assert audio.resample_plan(8000) == (2, 1, 64, 130)
    assert audio.resample_plan(16000) == (1, 1, 0, 2)
    np.testing.assert_array_equal(audio.resample_table(16000), [[1.0, 0.0]])


def test_resample_plan_refusals():
    from speech_to_image_translation_without_text_amd import audio
    for rate in (3999, 0, -16000, 192001, 10 ** 6):
        with pytest.raises(ValueError, match=str(rate)):
            audio.resample_plan(rate)
    assert audio.resample_plan(4000)[:2] == (4, 1) and audio.resample_plan(192000) == (1, 12, 768, 1538)
    with pytest.raises(ValueError, match="191999"):     # L = 16000, taps = 1538: 24.6 M floats
        audio.resample_plan(191999)
    with pytest.raises(ValueError):
        audio.resample_plan(44100.5)


@pytest.mark.parametrize("rate", RATES)
def test_table_is_the_formula_and_sums_to_one(rate):
    from speech_to_image_translation_without_text_amd import audio
    got = audio.resample_table(rate)
    want = R.table(rate)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    assert np.abs(got.sum(axis=1) - 1.0).max() <= 1e-7
    if rate != 16000:
        # independent of both: one entry by the formula written out, with numpy.i0
        L, M, W, taps = R.plan(rate)
        scale = min(1.0, L / M)
        p, j = L // 2, W + 3
        t = scale * (W - j + p / L)
        h = 0.9475937167399596 * np.sinc(0.9475937167399596 * t) * np.i0(14.769656459379492 * np.sqrt(1 - (t / 64) ** 2)) \
            / np.i0(14.769656459379492)
        assert abs(got[p, j] - scale * h) <= 1e-15


def test_resampled_length_is_the_integer_rule():
    from speech_to_image_translation_without_text_amd import audio
    assert [audio.resampled_length(n, 44100) for n in (0, 1, 441, 442)] == [0, 1, 160, 161]
    assert [audio.resampled_length(n, 48000) for n in (0, 1, 2, 3, 4)] == [0, 1, 1, 1, 2]
    assert [audio.resampled_length(n, 8000) for n in (0, 1, 7)] == [0, 2, 14]
    assert audio.resampled_length(12345, 16000) == 12345
    n = 13_500_000
    assert audio.resampled_length(n, 44100) == -(-n * 160 // 441)
    assert audio.n_frames(audio.resampled_length(0, 44100)) == 2     # an empty clip still counts as 200 zeros


def test_zero_tail_where_ceil_differs_from_floor():
    rng = np.random.default_rng(0)
    for rate, n in ((44100, 442), (44100, 441), (48000, 10), (48000, 9), (22050, 1000), (8000, 33)):
        L, M, W, taps = R.plan(rate)
        tab = rng.standard_normal((L, taps))
        x = rng.standard_normal(n)
        y = R.resample(x, L, M, W, tab)
        nout, nfull = -(-n * L // M), n * L // M
        assert len(y) == nout
        assert (y[nfull:] == 0).all() and (y[:nfull] != 0).all()
        assert nout - nfull == (1 if (n * L) % M else 0)
    assert len(R.resample(np.zeros(0), 160, 441, 177, np.zeros((160, 356)))) == 0


# ---- sanity of the definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (48000, 44100, 22050, 8000))
def test_tones_come_out_as_the_16k_tone(rate):
    L, M, W, taps = R.plan(rate)
    tab = R.table(rate)
    n = int(rate * 0.25)
    edge = int(2 * W * min(1.0, L / M) + 2) + 1
    for f in (440.0, 3000.0, 7000.0, 9000.0, 12000.0):
        if f >= rate / 2:
            continue
        x = np.sin(2 * np.pi * f * np.arange(n) / rate + 0.3)
        y = R.resample(x, L, M, W, tab)
        mid = slice(edge, len(y) - edge - 1)
        if f <= 7000.0:
            want = np.sin(2 * np.pi * f * np.arange(len(y)) / 16000.0 + 0.3)
            err = np.abs(y - want)[mid].max()
            assert err <= 1e-6, (rate, f, err)
        else:
            left = np.abs(y)[mid].max()
            assert left <= 1e-7, (rate, f, left)


def test_mutants_of_the_restatement_show():
    """with a random table every tap counts (the Kaiser table's edge taps are ~1e-8 and would hide an off-by-one); each
    wrong version must be more than 10 x the loosest GPU bound away: the bound is 2 x the fp32 yardstick"""
    rng = np.random.default_rng(1)
    for L, M, W in ((1, 3, 2), (2, 1, 1), (3, 2, 4), (160, 441, 177)):
        taps = 2 * W + 2
        tab = rng.standard_normal((L, taps)).astype(np.float32)
        n = 1000 * M // L + 1                     # ceil differs from floor
        assert (n * L) % M or M == 1                # M = 1 has no tail
        x = rng.standard_normal(n).astype(np.float32)
        before = rng.standard_normal(2 * W + 8).astype(np.float32)
        truth = R.resample(x, L, M, W, tab)
        yard = R.rel_err(R.resample_f32(x, L, M, W, tab), truth)
        assert 0 < yard < 1e-5
        for mutant in R.MUTANTS:
            if (mutant == "phases_reversed" and L == 1) or (mutant == "tail_computed" and M == 1):
                continue                              # one phase has no order; no tail to compute
            d = R.rel_err(R.resample(x, L, M, W, tab, mutant=mutant, before=before), truth)
            assert d > 10 * 2 * yard and d > 1e-3, (L, M, W, mutant, d)


# ---- RIFF reader ----------------------------------------------------------------------------------------------------
FORMATS = (R.U8, R.S16, R.S24, R.S32, R.F32, R.F64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_probe_every_accepted_tag_and_width(fmt, tmp_path):
    from speech_to_image_translation_without_text_amd import audio
    x = np.random.default_rng(fmt).uniform(-0.9, 0.9, (37, 3))
    data = R.encode(x, fmt)
    for ext in (False, True):
        p = tmp_path / ("a%d.wav" % ext)
        R.write_wav(p, data, fmt, 3, 22050, extensible=ext)
        info = audio.probe_audio(p)
        assert (info.rate, info.channels, info.format, info.frames) == (22050, 3, fmt, 37)
        assert info.data_bytes == len(data) and info.path == str(p)
        got, raw = audio.read_audio(p)
        assert got == info and raw.dtype == np.uint8 and raw.tobytes() == data


def test_probe_skips_chunks_and_cuts_overlong_data(tmp_path):
    from speech_to_image_translation_without_text_amd import audio
    data = R.encode(np.linspace(-0.5, 0.5, 22).reshape(11, 2), R.S24)        # 66 bytes
    p = tmp_path / "l.wav"
    R.write_wav(p, data, R.S24, 2, 48000, chunks_before=[(b"LIST", b"INFOabc"), (b"junk", b"12345")])   # both odd
    info, raw = audio.read_audio(p)
    assert info.frames == 11 and raw.tobytes() == data
    R.write_wav(p, data + b"\x01\x02", R.S24, 2, 48000, data_size=10 ** 6)   # claims more than the file holds
    info, raw = audio.read_audio(p)
    assert info.frames == 11 and raw.tobytes() == data                       # cut to whole frames
    R.write_wav(p, b"", R.S16, 1, 16000)
    info, raw = audio.read_audio(p)
    assert info.frames == 0 and raw.size == 0
    # the stdlib writer's files read the same
    with wave.open(str(p), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.arange(20, dtype="<i2").tobytes())
    info, raw = audio.read_audio(p)
    assert (info.rate, info.channels, info.format, info.frames) == (16000, 2, R.S16, 10)
    assert raw.tobytes() == np.arange(20, dtype="<i2").tobytes()


def test_probe_refusals_name_the_file(tmp_path):
    from speech_to_image_translation_without_text_amd import audio
    p = tmp_path / "bad.wav"

    def refused(match):
        with pytest.raises(ValueError, match=match) as e:
            audio.probe_audio(p)
        assert "bad.wav" in str(e.value)

    def fmt_file(tag, ch, rate, align, bits, magic=b"RIFF"):
        body = struct.pack("<HHIIHH", tag, ch, rate, rate * align, align, bits)
        rest = b"WAVE" + b"fmt " + struct.pack("<I", 16) + body + b"data" + struct.pack("<I", 4) + bytes(4)
        p.write_bytes(magic + struct.pack("<I", len(rest)) + rest)

    fmt_file(2, 1, 16000, 1, 4)               # ADPCM
    refused("tag 0x0002")
    fmt_file(0x55, 2, 44100, 1, 0)            # MP3
    refused("tag 0x0055")
    fmt_file(1, 1, 16000, 2, 16, magic=b"RF64")
    refused("RF64")
    fmt_file(1, 0, 16000, 0, 16)
    refused("0 channels")
    fmt_file(1, 9, 16000, 18, 16)
    refused("9 channels")
    fmt_file(1, 2, 16000, 2, 16)
    refused("block align 2")
    fmt_file(1, 1, 3000, 2, 16)
    refused("3000")
    fmt_file(1, 1, 200000, 2, 16)
    refused("200000")
    fmt_file(1, 1, 191999, 2, 16)
    refused("191999")
    fmt_file(1, 1, 16000, 5, 40)
    refused("40-bit")
    fmt_file(3, 1, 16000, 2, 16)
    refused("16-bit float")
    p.write_bytes(b"not a wav file at all")
    refused("RIFF")
    p.write_bytes(b"RIFF" + struct.pack("<I", 4) + b"WAVE")
    refused("fmt")


def test_read_wav_keeps_its_refusals(tmp_path):
    from speech_to_image_translation_without_text_amd import audio
    with wave.open(str(tmp_path / "r.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(22050)
        f.writeframes(bytes(20))
    with pytest.raises(ValueError, match="22050 Hz; need 16000 Hz"):
        audio.read_wav(tmp_path / "r.wav")
    assert audio.probe_audio(tmp_path / "r.wav").rate == 22050


# ---- decode and mono ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", (1, 2, 3, 6))
@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_and_mono_against_numpy(fmt, channels):
    rng = np.random.default_rng(10 * fmt + channels)
    n = 50
    x = rng.uniform(-1, 1, (n, channels))
    x[0], x[1] = -1.0, 1.0                   # the formats' end points (clipped by encode)
    raw = R.encode(x, fmt)
    if fmt == R.U8:
        want = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128) / 128
    elif fmt == R.S16:
        want = np.frombuffer(raw, "<i2").astype(np.float32) / 32768
    elif fmt == R.S24:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3)
        want = np.array([int.from_bytes(bytes(t), "little", signed=True) for t in b], dtype=np.float64) / 8388608
        want = want.astype(np.float32)
    elif fmt == R.S32:
        want = (np.frombuffer(raw, "<i4").astype(np.float64) / 2147483648).astype(np.float32)
    elif fmt == R.F32:
        want = np.frombuffer(raw, "<f4")
    else:
        want = np.frombuffer(raw, "<f8").astype(np.float32)
    want = want.reshape(n, channels)
    got = R.decode(raw, fmt, channels)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    m = want[:, 0]
    for c in range(1, channels):
        m = (m + want[:, c]).astype(np.float32)
    np.testing.assert_array_equal(R.mono(got), (m / np.float32(channels)).astype(np.float32))
    # through the bypass table the whole restatement is the mono signal
    np.testing.assert_array_equal(R.load(raw, fmt, channels, 16000).astype(np.float32), R.mono(got))


def test_s16_mono_and_stereo_are_read_wav(tmp_path):
    from speech_to_image_translation_without_text_amd import audio
    rng = np.random.default_rng(3)
    for ch in (1, 2):
        v = rng.integers(-32768, 32768, (400, ch)).astype("<i2")
        with wave.open(str(tmp_path / "x.wav"), "wb") as f:
            f.setnchannels(ch)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(v.tobytes())
        np.testing.assert_array_equal(R.mono(R.decode(v.tobytes(), R.S16, ch)), audio.read_wav(tmp_path / "x.wav"))


# ---- device layout --------------------------------------------------------------------------------------------------
def test_pack_resample_table_round_trip():
    from speech_to_image_translation_without_text_amd import audio
    rng = np.random.default_rng(5)
    for L, taps in ((1, 2), (1, 386), (160, 356), (2, 130), (3, 10)):
        t = rng.standard_normal((L, taps)).astype(np.float32)
        flat = audio.pack_resample_table(t)
        tpad = (taps + 3) // 4 * 4
        assert flat.dtype == np.float32 and flat.shape == (L * tpad,)
        for p in (0, L - 1):
            np.testing.assert_array_equal(flat[p * tpad:p * tpad + taps], t[p])
            assert (flat[p * tpad + taps:(p + 1) * tpad] == 0).all()
        np.testing.assert_array_equal(audio.unpack_resample_table(flat, L, taps), t)


def test_tiles_and_group_image():
    from speech_to_image_translation_without_text_amd import audio
    tiles = audio.resample_tiles([1, 0, 1024, 1025, 3077])
    assert tiles.dtype == np.int32
    assert tiles.tolist() == [[0, 0], [2, 0], [3, 0], [3, 1024], [4, 0], [4, 1024], [4, 2048], [4, 3072]]
    raws = [np.arange(5, dtype=np.uint8), np.arange(40, dtype=np.uint8)]
    image, where, ntiles = audio.pack_group(raws, [5, 40], [0, 5], [5, 40])
    assert ntiles == 2 and all(v % 16 == 0 for v in where.values())
    boff = image[where["boff"]:where["boff"] + 16].view(np.int64)
    assert boff.tolist() == [0, 16]
    for b, r in zip(boff, raws):
        np.testing.assert_array_equal(image[where["raw"] + b:where["raw"] + b + len(r)], r)
    assert image[where["frames"]:where["frames"] + 8].view(np.int32).tolist() == [5, 40]
    assert image[where["olen"]:where["olen"] + 8].view(np.int32).tolist() == [5, 40]
    assert image[where["ooff"]:where["ooff"] + 16].view(np.int64).tolist() == [0, 5]
    assert image[where["tiles"]:where["tiles"] + 16].view(np.int32).tolist() == [0, 0, 1, 0]


# ---- interface ------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_device():
    code = r'''
import sys
sys.path.insert(0, %r)
from speech_to_image_translation_without_text_amd import _lib
lib = _lib.load()
assert lib.s2i_version() == 7
P = 4096
args = [P, P, P, 2, _lib.PCM_S16, 2, 160, 441, 177, P, P, 3, P, P, P, None]   # only ever passed with one argument broken
def refused(i, v, word):
    bad = list(args); bad[i] = v
    assert lib.s2i_pcm_resample(*bad) != 0, (i, v)
    assert word in lib.s2i_last_error(), (i, v, lib.s2i_last_error())
for i in (0, 1, 2, 9, 10, 12, 13, 14):
    refused(i, None, b"null")
refused(3, 0, b"count")
refused(4, 6, b"format"); refused(4, -1, b"format")
refused(5, 0, b"channels"); refused(5, 9, b"channels")
refused(6, 0, b"ratio"); refused(6, 16001, b"ratio"); refused(6, 147, b"ratio")      # gcd(147, 441) = 147
refused(7, 0, b"ratio"); refused(7, 160 * 12 + 1, b"ratio"); refused(7, 39, b"ratio")  # under 4 kHz
refused(8, -1, b"width"); refused(8, 769, b"width")
refused(9, P + 4, b"aligned"); refused(12, P + 8, b"aligned"); refused(0, P + 2, b"aligned")
refused(11, 0, b"tile")
bad = list(args); bad[6], bad[7], bad[8] = 16000, 16001, 768                           # 16000 x 1538 floats
assert lib.s2i_pcm_resample(*bad) != 0 and b"2^24" in lib.s2i_last_error()
bad = list(args); bad[6], bad[7], bad[8] = 1, 12, 768
bad[0] = None
assert lib.s2i_pcm_resample(*bad) != 0
print("ok")
''' % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_resample_flag_of_the_four_clis():
    from speech_to_image_translation_without_text_amd import (extract_audio_feature, speech_to_image, train_encoder,
                                                              train_encoder_head)
    assert extract_audio_feature.get_parser().parse_args([]).resample is False
    assert extract_audio_feature.get_parser().parse_args(["--resample"]).resample is True
    base = ["--model", "m.pt", "--netG", "g.pth", "--out_dir", "o", "a.wav"]
    assert speech_to_image.get_parser().parse_args(base).resample is False
    assert speech_to_image.get_parser().parse_args(base + ["--resample"]).resample is True
    assert train_encoder.get_parser().parse_args([]).resample is False
    assert train_encoder.get_parser().parse_args(["--resample", "--resident"]).resample is True
    assert train_encoder_head.get_parser().parse_args(["--model", "m.pt"]).resample is False
    assert train_encoder_head.get_parser().parse_args(["--model", "m.pt", "--resample"]).resample is True


def test_scan_frames_resample_uses_the_integer_rule(tmp_path):
    """the pool is sized from headers alone: n_frames(resampled_length(header frames, rate))"""
    import speech_loader_ref as SR
    from speech_to_image_translation_without_text_amd import audio, speech_loader
    from speech_to_image_translation_without_text_amd.train_encoder_head import SplitData
    paths = SR.make_tree(str(tmp_path), "train", [[0.1, 0.2], [0.3]])
    specs = [(R.F32, 1, 48000, 48001), (R.S24, 2, 44100, 442), (R.U8, 1, 8000, 0)]
    flat = [p for item in paths for p in item]
    for p, (fmt, ch, rate, n) in zip(flat, specs):
        R.write_wav(p, R.encode(np.zeros((n, ch)), fmt), fmt, ch, rate)
    split = SplitData(str(tmp_path), "train", "birds", resample=True)
    assert split.resample is True and SplitData(str(tmp_path), "train", "birds").resample is False
    frames = speech_loader.scan_frames(split, workers=2, resample=True)
    want = [audio.n_frames(-(-n * 16000 // rate)) for _, _, rate, n in specs]
    assert [f.tolist() for f in frames] == [want[:2], want[2:]]
    assert want == [1 + 16001 // 160, 1 + 161 // 160, 2]
