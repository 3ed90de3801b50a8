"""The room reverberation on the GPU: s2i_reverb_rir and s2i_reverb against tests/reverb_ref.py -- the impulse response tap
by tap, the convolution exactly on impulses and within the dot-product bound on noise, its determinism, the wrapper's
refusals -- and its place in the feeder: composition with the speed and noise stages, exact resume, extraction."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import reverb_ref as ref
from speech_loader_ref import make_tree
from test_waveaug_gpu import _epoch, _pickles, tree  # noqa: F401  (tree: the module-scoped fixture of the waveform feeder)

pytestmark = pytest.mark.gpu

SEED, STEP = 2 ** 37 + 21, 2 ** 32 + 3
TILE = 8192                     # outputs per workgroup of s2i_reverb
U = 2.0 ** -24                  # unit roundoff of fp32
MASK64 = 2 ** 64 - 1


def _ops():
    from speech_to_image_translation_without_text_amd import ops
    return ops


def entry(taps, uid, drr=6.0):
    """a table row as ops.waveaug_plan would make it for T60 = taps / 16000 (taps 32 and 64 lie under the policy's T60 range:
    the kernels take them all the same)"""
    if taps == 0:
        return (0.0, 0.0, 0, uid)
    slope = np.float32(-np.log2(1000.0) / taps)
    energy = np.exp2(2.0 * np.arange(1, taps, dtype=np.float64) * float(slope)).sum()
    return (np.float32(np.sqrt(10.0 ** (-drr / 10.0) / energy)), slope, taps, uid)


def make_table(rows):
    t = np.zeros(len(rows), dtype=_ops().REVERB_ENTRY)
    for b, r in enumerate(rows):
        t[b] = r
    return t


def device_rir(gpu, table, seed=SEED, step=STEP):
    """s2i_reverb_rir alone into a NaN-filled buffer: numpy [B][max_taps]"""
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    B, max_taps = len(table), max(int(table["taps"].max()), 32)
    with torch.cuda.device(gpu):
        t = torch.from_numpy(table.view(np.uint8).copy()).to(gpu)
        h = torch.full((B, max_taps), float("nan"), dtype=torch.float32, device=gpu)
        _lib.check(lib.s2i_reverb_rir(_lib.ptr(t), B, max_taps, _lib.ptr(h), seed & MASK64, step & MASK64, _lib.stream()),
                   "s2i_reverb_rir")
        torch.cuda.synchronize()
    return h.cpu().numpy()


def layout(lens, odd=()):
    """offsets of clips laid out with a guard band between them, on 16-byte boundaries but for the clips in `odd`"""
    offsets, at = [], 8
    for b, n in enumerate(lens):
        at = (at + 3) // 4 * 4 + (3 if b in odd else 0)
        offsets.append(at)
        at += n + 5
    return np.array(offsets, dtype=np.int64), at + 8


def run(gpu, clips, table, odd=(), seed=SEED, step=STEP):
    """the clips inside NaN guard bands through ops.reverb into a NaN-filled `out` -> (out as numpy, offsets, x buffer)"""
    ops = _ops()
    lens = [len(c) for c in clips]
    offsets, size = layout(lens, odd)
    buf = np.full(size, np.nan, dtype=np.float32)
    inside = np.zeros(size, dtype=bool)
    for o, c in zip(offsets, clips):
        buf[o:o + len(c)] = c
        inside[o:o + len(c)] = True
    x = torch.from_numpy(buf).to(gpu)
    out = torch.full_like(x, float("nan"))
    got = ops.reverb(x, offsets, lens, table, seed, step, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.uint32), buf.view(np.uint32)), "x was written"
    y = out.cpu().numpy()
    assert np.isnan(y[~inside]).all(), "a float outside the clips was written"
    assert not np.isnan(y[inside]).any(), "a sample was left unwritten"
    return y, offsets


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the impulse response ----------------------------------------------------------------------------------------------------
def test_rir_matches_the_reference(gpu):
    """Taps 32, 64, 800 and 16000 with distinct uids in one launch, into a NaN-filled buffer.

    The bound 16 x 2^-24 relative, per tap, is derived.  The reference is alpha e_k 2^(k slope) in float64 from the same fp32
    alpha, slope and e_k (e_k = fl(((float)s - 131070) c) is an integer times one constant, so its correctly rounded product
    is the same number on both sides).  The kernel computes fl(fl(alpha e_k) exp2f(fl((float)k slope))):
      - fl(k slope): relative 2^-24 of a magnitude of at most log2(1000) (taps - 1) / taps < 9.97 here (slope =
        -log2(1000) / taps), an absolute 9.97 x 2^-24 in the exponent, which exp2 turns into ln 2 x 9.97 x 2^-24 =
        6.9 x 2^-24 relative;
      - exp2f: 1 ulp in HIP's table of single-precision functions, at most 2 x 2^-24 relative;
      - the two rounded products: 2^-24 each.
    Sum: 10.9 x 2^-24, under 16 x 2^-24 with room for second-order terms."""
    taps = [32, 64, 800, 16000]
    table = make_table([entry(t, uid, drr) for t, uid, drr in zip(taps, (5, 2 ** 32 - 1, 0, 123456), (0.0, 6.0, -20.0, 30.0))])
    h = device_rir(gpu, table)
    assert h.shape == (4, 16000)
    worst = 0.0
    for b, t in enumerate(taps):
        want = ref.rir(table["alpha"][b], table["slope"][b], t, int(table["uid"][b]), SEED, STEP, 16000)
        assert not np.isnan(h[b]).any(), "a tap was left unwritten"
        assert h[b, 0] == np.float32(1.0)
        assert not h[b, t:].any(), "taps past the response must be zero"
        err = np.abs(h[b, 1:t].astype(np.float64) - want[1:t])
        assert np.all(err <= 16 * U * np.abs(want[1:t])), (t, float((err / np.abs(want[1:t]).clip(1e-300)).max() / U))
        worst = max(worst, float((err / np.abs(want[1:t]).clip(1e-300)).max() / U))
        assert np.count_nonzero(h[b, 1:t]) >= t - 2
    print("rir: worst tap error %.2f x 2^-24 relative, bound 16" % worst)
    # another step, another seed word, another uid: another tail
    assert not np.array_equal(device_rir(gpu, table, step=STEP + 1)[3], h[3])
    assert not np.array_equal(device_rir(gpu, table, seed=SEED + 2 ** 32)[3], h[3])
    # an off row is zeros
    assert not device_rir(gpu, make_table([entry(0, 1), entry(32, 2)]))[0].any()


# ---- 2. impulses ------------------------------------------------------------------------------------------------------------------
IMPULSE_LENS = (1, 31, 32, 33, 100, 2 * TILE + 17)


def impulse_cases():
    return [(n, p) for n in IMPULSE_LENS for p in sorted({0, 1, 31, 32, 33, n - 1}) if p < n]


@pytest.mark.parametrize("taps", [32, 1088, 16000])
def test_impulses_are_exact(gpu, taps):
    """x = one 1.0 at p: y_i = h[i - p] bit for bit (one product with 1.0 and zeros), for every i, at every clip length and
    impulse position that sits on or beside a block or tile edge; 1088 taps cross one chunk of the tap loop, 16000 fifteen.
    Then 0.5 at p1 and 2.0 at p2 >= p1 + taps: the two responses do not overlap, and scaling by a power of two is exact."""
    cases = impulse_cases()
    clips = []
    for n, p in cases:
        x = np.zeros(n, dtype=np.float32)
        x[p] = 1.0
        clips.append(x)
    n2, p1 = 2 * TILE + 17, 1
    p2 = max(p1 + taps, TILE + 33)
    assert p2 < n2
    two = np.zeros(n2, dtype=np.float32)
    two[p1], two[p2] = 0.5, 2.0
    clips.append(two)
    table = make_table([entry(taps, 10 + b) for b in range(len(clips))])
    h = device_rir(gpu, table)
    y, offsets = run(gpu, clips, table, odd=(3, 7, len(clips) - 2))
    for b, (n, p) in enumerate(cases):
        want = np.zeros(n, dtype=np.float32)
        m = min(n - p, taps)
        want[p:p + m] = h[b, :m]
        got = y[offsets[b]:offsets[b] + n]
        assert np.array_equal(bits(got), bits(want)), "n %d, impulse at %d: first wrong sample %d" % (
            n, p, int(np.flatnonzero(bits(got) != bits(want))[0]))
    want = np.zeros(n2, dtype=np.float32)
    m1, m2 = min(n2 - p1, taps), min(n2 - p2, taps)
    want[p1:p1 + m1] = np.float32(0.5) * h[-1, :m1]
    want[p2:p2 + m2] = np.float32(2.0) * h[-1, :m2]
    got = y[offsets[-1]:offsets[-1] + n2]
    assert np.array_equal(bits(got), bits(want)), "two impulses: first wrong sample %d" % int(
        np.flatnonzero(bits(got) != bits(want))[0])


# ---- 3. noise against float64 ---------------------------------------------------------------------------------------------------
RANDOM_LENS = (1, 31, 32, 1000, 8192, 20011)


@pytest.fixture(scope="module")
def random_clips():
    rng = np.random.RandomState(17)
    return [rng.standard_normal(n).astype(np.float32) for n in RANDOM_LENS] + [rng.standard_normal(777).astype(np.float32)]


@pytest.mark.parametrize("taps", [32, 96, 3200, 16000])
def test_random_input_against_float64(gpu, random_clips, taps):
    """Every sample of every clip: |y - y_ref| <= ((taps + 32) + 16) 2^-24 (|h| * |x|)_i, with y_ref and |h| * |x| from
    the float64 reference: (taps + 32) 2^-24 is the bound of an fp32 dot product of that many terms (the taps and the zeros
    of the two end blocks) in any order, 16 x 2^-24 the tap error of test_rir_matches_the_reference.  taps exceeds the
    clip's length in most of the cases.  The last clip is off and must come back as it went in."""
    clips = random_clips
    table = make_table([entry(taps, 100 + b) for b in range(len(RANDOM_LENS))] + [entry(0, 9)])
    y, offsets = run(gpu, clips, table, odd=(3,))
    worst = 0.0
    for b, x in enumerate(clips[:-1]):
        h = ref.rir(table["alpha"][b], table["slope"][b], taps, 100 + b, SEED, STEP)
        want = ref.convolve(x, h)
        scale = ref.convolve(np.abs(x), np.abs(h))
        err = np.abs(y[offsets[b]:offsets[b] + len(x)].astype(np.float64) - want)
        bound = ((taps + 32) + 16) * U * scale
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), "clip of %d samples, %d taps: %.3g of the bound at sample %d" % (
            len(x), taps, float((err / bound).max()), int(np.argmax(err / bound)))
    print("reverb, %d taps: worst error %.3g of the bound" % (taps, worst))
    off = y[offsets[-1]:offsets[-1] + 777]
    assert np.array_equal(bits(off), bits(clips[-1]))


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------
def test_reverb_is_deterministic_and_independent_of_the_batch(gpu):
    rng = np.random.RandomState(4)
    clip = rng.standard_normal(9000).astype(np.float32)
    others = [rng.standard_normal(n).astype(np.float32) for n in (40000, 300, 12000)]
    row = entry(3200, 77)
    alone, o = run(gpu, [clip], make_table([row]))
    want = bits(alone[o[0]:o[0] + 9000])
    again, o = run(gpu, [clip], make_table([row]))
    assert np.array_equal(bits(again[o[0]:o[0] + 9000]), want)
    # on an odd float
    moved, o = run(gpu, [clip], make_table([row]), odd=(0,))
    assert o[0] % 4 == 3 and np.array_equal(bits(moved[o[0]:o[0] + 9000]), want)
    # third among other clips, other taps and another max_len (five tiles instead of two)
    batch = [others[0], others[1], clip, others[2]]
    table = make_table([entry(16000, 1), entry(0, 2), row, entry(800, 3)])
    a, o = run(gpu, batch, table)
    b, _ = run(gpu, batch, table)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(bits(a[o[2]:o[2] + 9000]), want)


# ---- 5. the wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_the_kernels_trust(gpu):
    from speech_to_image_translation_without_text_amd import _lib
    ops = _ops()
    x = torch.ones(128, device=gpu)
    out = torch.full_like(x, float("nan"))
    t = make_table([entry(32, 0)])
    ok = dict(offsets=[0], lens=[64], table=t)
    for bad in (dict(lens=[129]), dict(offsets=[-1]), dict(offsets=[100]), dict(lens=[-1]),
                dict(offsets=[0, 32], lens=[40, 32], table=np.repeat(t, 2)),          # overlapping
                dict(table=np.repeat(t, 2)), dict(lens=[64, 8]), dict(offsets=[])):   # mismatched lengths
        a = dict(ok, **bad)
        with pytest.raises(ValueError):
            ops.reverb(x, a["offsets"], a["lens"], a["table"], 1, 2, out=out)
    for field, value in (("taps", 48), ("taps", 16032), ("taps", -32), ("alpha", float("nan")), ("slope", float("inf"))):
        t2 = t.copy()
        t2[field] = value
        with pytest.raises(ValueError):
            ops.reverb(x, [0], [64], t2, 1, 2, out=out)
    with pytest.raises(ValueError):
        ops.reverb(x.double(), [0], [64], t, 1, 2)
    with pytest.raises(ValueError):
        ops.reverb(x.reshape(2, 64), [0], [64], t, 1, 2)
    with pytest.raises(ValueError):
        ops.reverb(x[::2], [0], [64], t, 1, 2)
    with pytest.raises(ValueError):
        ops.reverb(x, [0], [64], t, 1, 2, out=x)
    with pytest.raises(ValueError):
        ops.reverb(x, [0], [64], t, 1, 2, out=out[:64])
    with pytest.raises(_lib.S2IError):
        ops.reverb(x.cpu(), [0], [64], t, 1, 2)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((x == 1).all()), "something was launched"
    y = ops.reverb(x, [0], [64], t, 1, 2)
    assert y.shape == x.shape and y.dtype == x.dtype and y.device == x.device and y.data_ptr() != x.data_ptr()


# ---- 6. the feeder ----------------------------------------------------------------------------------------------------------------
SPEED = "speed=0.9/1.0/1.1"
ROOM = "reverb=1@0.2:0.4@0:10"
PAIRS = [(0, 0), (1, 1), (3, 0), (4, 1), (5, 0)]


def _clips(flat, offsets, lens):
    flat = flat.cpu().numpy()
    return [bits(flat[o:o + n]) for o, n in zip(offsets, lens)]


def test_feeder_composes_speed_reverb_and_noise(gpu, tree, monkeypatch):  # noqa: F811
    from speech_to_image_translation_without_text_amd import wave_loader
    ops = _ops()
    ws = wave_loader.ResidentWaveSet(tree, gpu, target_length=128)
    seed, step = 2 ** 33 + 5, 7
    dry, off, lens, plan_dry = ws.waves(PAIRS, wave_loader.WaveAug(SPEED, seed), step)
    assert "taps" not in plan_dry
    wet, off_w, lens_w, plan = ws.waves(PAIRS, wave_loader.WaveAug(SPEED + "," + ROOM, seed), step)
    assert np.array_equal(off, off_w) and np.array_equal(lens, lens_w) and np.all(plan["taps"] >= 3200)
    want = ops.reverb(dry, off, lens, ops.reverb_table(plan), seed, step)
    for a, b, c in zip(_clips(wet, off, lens), _clips(want, off, lens), _clips(dry, off, lens)):
        assert np.array_equal(a, b) and not np.array_equal(a, c)
    # the noise is mixed into the reverberated clip, at its power
    noisy, off_n, lens_n, plan_n = ws.waves(PAIRS, wave_loader.WaveAug(SPEED + "," + ROOM + ",white=1@10:10", seed), step)
    assert np.array_equal(off, off_n) and np.array_equal(plan_n["taps"], plan["taps"])
    mixed = ops.wave_mix(want.clone(), off, lens, ops.wave_mix_table(plan_n), seed, step)
    for a, b, c in zip(_clips(noisy, off, lens), _clips(mixed, off, lens), _clips(want, off, lens)):
        assert np.array_equal(a, b) and not np.array_equal(a, c)
    # perturb (extraction) is the same composition without a pool
    waves = [np.asarray(ws.pool[int(ws.offsets[ws.first[i] + u]):][:int(ws.samples[ws.first[i] + u])].cpu()) for i, u in PAIRS]
    views = wave_loader.perturb(waves, wave_loader.WaveAug(SPEED + "," + ROOM + ",white=1@10:10", seed), gpu, step)
    for v, b in zip(views, _clips(noisy, off, lens)):
        assert np.array_equal(bits(v.cpu().numpy()), b)
    # without reverb= nothing of it runs
    monkeypatch.setattr(ops, "reverb", lambda *a, **k: pytest.fail("ops.reverb was called without reverb="))
    monkeypatch.setattr(ops, "reverb_table", lambda *a, **k: pytest.fail("a reverb table was made without reverb="))
    again, _, _, _ = ws.waves(PAIRS, wave_loader.WaveAug(SPEED, seed), step)
    assert all(np.array_equal(a, b) for a, b in zip(_clips(again, off, lens), _clips(dry, off, lens)))
    ws.waves(PAIRS)


# ---- 7. resume --------------------------------------------------------------------------------------------------------------------
TRAIN_SPEC = "speed=0.9/1.0/1.1,reverb=0.7@0.2:0.6@0:15,white=0.7@5:25,babble=0.6@0:15"


@pytest.mark.parametrize("kind", ["head", "encoder"])
def test_trainer_resumes_bit_for_bit_under_reverb(gpu, tree, kind):  # noqa: F811
    import encoder_conv_train_ref as R
    from test_encoder_resume_gpu import first_difference, trainers
    from speech_to_image_translation_without_text_amd import wave_loader
    ws = wave_loader.ResidentWaveSet(tree, gpu, target_length=128)
    aug = wave_loader.WaveAug(TRAIN_SPEC, seed=9)
    net = R.stack_net(bidirectional=True, nhidden=1024)

    def make():
        return trainers()[kind](copy.deepcopy(net).to(gpu), step_size=1, **R.TRAINER_LOSS)
    random.seed(41)
    straight = make()
    seen = _epoch(straight, ws, gpu, aug) + _epoch(straight, ws, gpu, aug)
    assert straight.steps == 4 and not torch.equal(seen[0], seen[2])
    random.seed(41)
    stopped = make()
    _epoch(stopped, ws, gpu, aug)
    state, draws = copy.deepcopy(stopped.state_dict()), random.getstate()
    random.seed(0)                                  # whatever happens between the runs
    resumed = make()
    resumed.load_state_dict(state)
    random.setstate(draws)
    assert resumed.steps == 2
    again = _epoch(resumed, ws, gpu, aug)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, seen[2:]))
    diff = first_difference(straight.state_dict(), resumed.state_dict())
    assert diff is None, "the resumed trainer differs first at %s" % diff
    # the control: the same draws without the room are other batches
    first = []
    for spec in (TRAIN_SPEC, TRAIN_SPEC.replace("reverb=0.7@0.2:0.6@0:15,", "")):
        random.seed(41)
        first.append(next(ws.batches(3, gpu, True, aug=wave_loader.WaveAug(spec, seed=9), step=lambda: 0))[0].clone())
    assert torch.equal(first[0][0, 0, :8], seen[0]) and not torch.equal(first[0], first[1])


def test_cli_resumes_bit_for_bit_under_reverb(gpu, tmp_path, capsys):
    from test_encoder_resume_gpu import COMMON, checkpoints_equal, cli_tree, result_lines
    from speech_to_image_translation_without_text_amd import train_encoder
    root = str(tmp_path)
    cli_tree(root)
    assert COMMON[-2:] == ["--state_every", "1"]
    out_s, out_r, out_p = (os.path.join(root, d) for d in ("straight", "stopped", "dry"))
    common = COMMON + ["--data_dir", root, "--waveaug", TRAIN_SPEC]
    train_encoder.main(common + ["--output_dir", out_s, "--epoch", "2"])
    straight = capsys.readouterr().out
    assert "resident train waveforms:" in straight
    train_encoder.main(common + ["--output_dir", out_r, "--epoch", "1"])
    capsys.readouterr()
    train_encoder.main(common + ["--output_dir", out_r, "--epoch", "2", "--resume", os.path.join(out_r, "state.pth")])
    leg2 = capsys.readouterr().out
    assert result_lines(leg2) == result_lines(straight, first=2) and len(result_lines(leg2)) == 2
    checkpoints_equal(os.path.join(out_s, "epoch_2.pth"), os.path.join(out_r, "epoch_2.pth"))
    # the control: without the room the run ends elsewhere
    train_encoder.main(COMMON + ["--data_dir", root, "--waveaug", TRAIN_SPEC.replace("reverb=0.7@0.2:0.6@0:15,", ""),
                                 "--output_dir", out_p, "--epoch", "2"])
    assert result_lines(capsys.readouterr().out) != result_lines(straight)
    with pytest.raises(SystemExit, match="reverb=2@"):
        train_encoder.main(COMMON + ["--data_dir", root, "--waveaug", "reverb=2@0.2:0.6@0:15", "--output_dir", out_p])


# ---- 8. extraction ----------------------------------------------------------------------------------------------------------------
def test_extraction_under_reverb(gpu, tmp_path):
    from encoder_ref import build_encoder
    from speech_to_image_translation_without_text_amd import extract_audio_feature as E
    root = str(tmp_path)
    make_tree(root, "train", [[0.7, 0.9, 0.3, 1.0, 0.8], [1.1, 0.66, 0.75, 0.72, 0.95]], seed=6)
    model_path = os.path.join(root, "encoder.pt")
    torch.save({"state_dict": build_encoder().state_dict()}, model_path)
    common = ["--model", model_path, "--bidirectional", "--data_dir", root, "--splits", "train", "--batch_size", "4"]
    room = "reverb=1@0.3:0.3@5:5"
    E.main(common + ["--audio_switch", "clean"])
    E.main(common + ["--audio_switch", "a", "--waveaug", room, "--waveaug_seed", "4"])
    E.main(common + ["--audio_switch", "b", "--waveaug", room, "--waveaug_seed", "4"])
    E.main(common + ["--audio_switch", "c", "--waveaug", room, "--waveaug_seed", "5"])
    clean, a, b, c = (_pickles(root, s) for s in ("clean", "a", "b", "c"))
    assert a == b and a[0] != clean[0] and c[0] != a[0] and a[1] == clean[1]      # a room keeps the lengths
    with pytest.raises(SystemExit, match="reverb=1@0.3"):
        E.main(common + ["--waveaug", "reverb=1@0.3:0.3"])
