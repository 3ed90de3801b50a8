"""The phase-vocoder time stretch on the GPU: s2i_time_stretch against tests/stretch_ref.py in float64 over the case table
(bound: twice the float32 mode's own deviation, stretch_ref.YARDSTICK), the rate-1 copy, the guard bands, batch
independence, the wrapper's refusals -- and its place in the feeder: composition with the speed, reverb and noise stages,
exact resume, extraction.

Measured on an MI355X: every one of the 55 cases lies within 0.55 of its own bound (1.10 x its own yardstick, at
n = 5000, rho = 0.25: 3.26e-6 against 2.97e-6); DESIGN.md 8b4d has the table case by case and what other summation
orders gave."""
import copy
import os
import random

import numpy as np
import pytest
import torch

import logmel_ref
import resample_ref
import reverb_ref
import stretch_ref as ref
import waveaug_ref
from speech_loader_ref import make_tree
from test_waveaug_gpu import _epoch, _pickles, tree  # noqa: F401  (tree: the module-scoped fixture of the waveform feeder)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of fp32
GAMMA = 8e-7        # tests/test_logmel_gpu.py's bound on the mel power, in units of the magnitude bound A


def _ops():
    from speech_to_image_translation_without_text_amd import ops
    return ops


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_table(lens, rates):
    t = np.zeros(len(lens), dtype=_ops().STRETCH_ENTRY)
    t["rate"] = rates
    t["out_len"] = [n if r == 1.0 else ref.out_length(n, r) for n, r in zip(lens, rates)]
    return t


def layout(lens, shift=0):
    """offsets of clips with a guard band between them, every clip on a 16-byte boundary; `shift` (a multiple of 4) moves
    them all"""
    offsets, at = [], 8 + shift
    for n in lens:
        at = (at + 3) // 4 * 4
        offsets.append(at)
        at += n + 5
    return np.array(offsets, dtype=np.int64), at + 8


def run(gpu, clips, rates, shift=0):
    """the clips inside NaN guard bands through ops.time_stretch into a NaN-filled `out` that is longer than needed ->
    the list of stretched clips (numpy).  Asserts that x is unchanged, that every float of `out` outside the clips stayed
    NaN and that every sample inside was written."""
    ops = _ops()
    lens = [len(c) for c in clips]
    offsets, size = layout(lens, shift)
    buf = np.full(size, np.nan, dtype=np.float32)
    for o, c in zip(offsets, clips):
        buf[o:o + len(c)] = c
    table = make_table(lens, rates)
    x = torch.from_numpy(buf).to(gpu)
    total = int(((table["out_len"].astype(np.int64) + 3) // 4 * 4).sum())
    out = torch.full((total + 64,), float("nan"), dtype=torch.float32, device=gpu)
    got, out_offsets, out_lens = ops.time_stretch(x, offsets, lens, table, out=out)
    assert got is out and np.array_equal(out_lens, table["out_len"])
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.uint32), buf.view(np.uint32)), "x was written"
    y = out.cpu().numpy()
    inside = np.zeros(len(y), dtype=bool)
    for o, n in zip(out_offsets, out_lens):
        assert o % 4 == 0
        inside[o:o + n] = True
    assert np.isnan(y[~inside]).all(), "a float outside the clips was written"
    assert not np.isnan(y[inside]).any(), "a sample was left unwritten"
    return [y[o:o + n].copy() for o, n in zip(out_offsets, out_lens)]


@pytest.fixture(scope="module")
def references():
    """{(n, rho): the float64 stretch of the case clip}, computed once"""
    return {(n, r): ref.time_stretch(ref.case_clip(n), r, np.float64) for n, r in ref.cases()}


# ---- 1. against float64 -----------------------------------------------------------------------------------------------------------
def test_case_table_against_float64_in_one_mixed_batch(gpu, references):
    """Every boundary length at every rate and the long clip, with three rate-1 clips among them, in one launch.  Per clip
    max|got - ref| / max|ref| <= 2 x the float32 mode's deviation in the same case (n, rho) (stretch_ref.YARDSTICK,
    measured on the CPU by measure_yardsticks; test_stretch_cpu.py holds the constants to a fresh measurement), and at
    least 2 x 2^-24 where that yardstick is smaller (stretch_ref.YARDSTICK_FLOOR has the reason).  The rate-1 clips must
    come back bit for bit."""
    cases = ref.cases()
    clips = [ref.case_clip(n) for n, _ in cases]
    rates = [r for _, r in cases]
    copies = {5: ref.case_clip(513), 23: ref.case_clip(1), 40: ref.case_clip(5000)}
    for at in sorted(copies):
        clips.insert(at, copies[at])
        rates.insert(at, 1.0)
    got = run(gpu, clips, rates)
    worst, failed = 0.0, []
    for y, x, r in zip(got, clips, rates):
        if r == 1.0:
            assert np.array_equal(bits(y), bits(x)), "a rate-1 clip of %d samples was not copied bit for bit" % len(x)
            continue
        n = len(x)
        want = references[(n, r)]
        assert len(y) == len(want) == ref.out_length(n, r)
        err = ref.rel_err(y, want)
        worst = max(worst, err / ref.bound(n, r))
        print("n %6d rho %.2f: %.3g (yardstick %.3g, %.2f of the bound)" % (n, r, err, ref.YARDSTICK[(n, r)], err / ref.bound(n, r)))
        if not err <= ref.bound(n, r):
            failed.append((n, r, err, ref.YARDSTICK[(n, r)]))
    print("stretch: worst case at %.2f of its bound" % worst)
    assert not failed, "over twice the case's yardstick (n, rho, deviation, yardstick): %s" % failed


def test_rate_one_is_a_copy(gpu):
    rng = np.random.RandomState(3)
    clips = [rng.standard_normal(n).astype(np.float32) for n in (1, 3, 4, 129, 2049, 30001)]
    for y, x in zip(run(gpu, clips, [1.0] * len(clips)), clips):
        assert np.array_equal(bits(y), bits(x))


def test_totals_too_small_leave_the_stretched_clips_alone_and_copy_the_rest(gpu):
    """include/s2i_hip.h: a stretched clip whose frames reach beyond the totals given is left unwritten, with every
    stretched clip behind it; clips before it and copied clips anywhere are written.  The wrapper never passes such totals,
    so this goes to the library: room for the first clip's frames only."""
    from speech_to_image_translation_without_text_amd import _lib
    ops = _ops()
    lib = _lib.load()
    rng = np.random.RandomState(5)
    clips = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in (300, 700, 40, 500)]
    rates = [2.0, 0.5, 1.0, 2.0]
    whole = run(gpu, clips, rates)
    lens = np.array([len(c) for c in clips])
    args = ops.time_stretch_prepare(torch.from_numpy(np.concatenate([np.pad(c, (0, -len(c) % 4)) for c in clips])).to(gpu),
                                    np.cumsum((lens + 3) // 4 * 4) - (lens + 3) // 4 * 4, lens, make_table(lens, rates))
    fin, fout = 1 + 300 // 128, ref.out_frames(300, 2.0)
    assert args["in_frames"] > fin and args["out_frames"] > fout
    args["out"].fill_(float("nan"))
    need = lib.s2i_time_stretch_workspace_bytes(4, fin, fout)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=gpu)
    _lib.check(lib.s2i_time_stretch(_lib.ptr(args["x"]), args["offsets"], args["lens"], 4, args["max_len"], args["table"],
                                    _lib.ptr(ops.device_stretch_basis(torch.device(gpu))), _lib.ptr(args["out"]),
                                    args["out_offsets"], args["max_out_len"], fin, fout, _lib.ptr(ws), need, _lib.stream()),
               "s2i_time_stretch")
    torch.cuda.synchronize()
    y = args["out"].cpu().numpy()
    got = [y[o:o + n] for o, n in zip(args["host_out_offsets"], args["host_out_lens"])]
    assert np.array_equal(bits(got[0]), bits(whole[0])) and np.array_equal(bits(got[2]), bits(clips[2]))
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------
def test_stretch_is_deterministic_and_independent_of_the_batch(gpu):
    """The same clip alone, alone at another offset, and third in a batch with longer clips (another max_len, other tiles,
    another place in the workspace): identical bits."""
    clip = ref.case_clip(5000)
    rng = np.random.RandomState(8)
    others = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in (20000, 300, 9001)]
    for rho in (0.84, 2.0):
        alone = bits(run(gpu, [clip], [rho])[0])
        assert np.array_equal(bits(run(gpu, [clip], [rho])[0]), alone)
        assert np.array_equal(bits(run(gpu, [clip], [rho], shift=1000)[0]), alone)
        batch = run(gpu, [others[0], others[1], clip, others[2]], [0.5, 1.0, rho, 4.0])
        assert np.array_equal(bits(batch[2]), alone)
        assert np.array_equal(bits(batch[1]), bits(others[1]))


# ---- 3. the wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_the_kernel_trusts(gpu):
    from speech_to_image_translation_without_text_amd import _lib
    ops = _ops()
    x = torch.ones(256, device=gpu)
    out = torch.full((1024,), float("nan"), device=gpu)
    t = make_table([64], [0.5])
    ok = dict(offsets=[0], lens=[64], table=t)
    for bad in (dict(lens=[257]), dict(offsets=[-4]), dict(offsets=[200]), dict(lens=[-1]), dict(offsets=[2]),
                dict(table=np.repeat(t, 2)), dict(lens=[64, 8]), dict(offsets=[])):
        a = dict(ok, **bad)
        with pytest.raises(ValueError):
            ops.time_stretch(x, a["offsets"], a["lens"], a["table"], out=out)
    for field, value in (("rate", 0.2), ("rate", 4.5), ("rate", float("nan")), ("rate", -1.0), ("out_len", 127), ("out_len", 64)):
        t2 = t.copy()
        t2[field] = value
        with pytest.raises(ValueError):
            ops.time_stretch(x, [0], [64], t2, out=out)
    with pytest.raises(ValueError):
        ops.time_stretch(x.double(), [0], [64], t)
    with pytest.raises(ValueError):
        ops.time_stretch(x.reshape(2, 128), [0], [64], t)
    with pytest.raises(ValueError):
        ops.time_stretch(x[::2], [0], [64], t)
    with pytest.raises(ValueError):
        ops.time_stretch(x[1:], [0], [64], t)                # misaligned
    with pytest.raises(ValueError):
        ops.time_stretch(x, [0], [64], t, out=x)
    with pytest.raises(ValueError):
        ops.time_stretch(x, [0], [64], t, out=out[:64])      # too small for 128 samples
    with pytest.raises(ValueError):
        ops.time_stretch(x, [0], [64], t, out=out.double())
    with pytest.raises(_lib.S2IError):
        ops.time_stretch(x.cpu(), [0], [64], t)
    with pytest.raises(ValueError, match="without tempo"):
        ops.stretch_table(ops.waveaug_plan(ops.waveaug_policy("speed=1.0"), 1, 2, [0], [20000]))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((x == 1).all()), "something was launched"
    y, off, lens = ops.time_stretch(x, [0], [64], t)
    assert y.dtype == x.dtype and y.device == x.device and y.data_ptr() != x.data_ptr() and lens.tolist() == [128] and off[0] == 0


# ---- 4. the feeder ----------------------------------------------------------------------------------------------------------------
VOICE = "pitch=-2/0/2,tempo=0.9/1.0/1.1"
SPEED = "speed=0.9/1.0/1.1"
ROOM = "reverb=1@0.2:0.4@0:10"
PAIRS = [(0, 0), (1, 1), (3, 0), (4, 1), (5, 0)]


def _clips(flat, offsets, lens):
    flat = flat.cpu().numpy()
    return [flat[o:o + n] for o, n in zip(offsets, lens)]


def test_feeder_composes_stretch_speed_reverb_and_noise(gpu, tree, monkeypatch):  # noqa: F811
    """The reference chain stretch_ref -> resample_ref -> reverb_ref -> waveaug_ref -> logmel_ref, stage by stage.  (a) the
    stretched and resampled waveform against the float64 chain stretch_ref -> resample_ref, within twice what the same
    chain in float32 (stretch_ref's float32 mode, then resample_ref.resample_f32) deviates; (b) the reverb, the noise and
    the log-mel are the launches of their own suites over that buffer, bit for bit, and each is held to its numpy
    reference over the stage before it as the device made it, within the bound its own suite derives (an error bound
    carried through a 3200-tap room and a noise whose gain follows the clip's power would be looser than these); (c)
    perturb is the same chain; (d) without the keys nothing of the stretch runs."""
    from speech_to_image_translation_without_text_amd import audio, wave_loader
    ops = _ops()
    T = 128
    ws = wave_loader.ResidentWaveSet(tree, gpu, target_length=T)
    seed = 2 ** 33 + 5
    waves = [audio.read_wav(ws.paths[ws.first[i] + u]) for i, u in PAIRS]
    stretched, pitched = 0, 0
    for step in (7, 8):
        aug = wave_loader.WaveAug(SPEED + "," + VOICE, seed)
        dry, off, lens, plan = ws.waves(PAIRS, aug, step)
        for b, (x, y) in enumerate(zip(waves, _clips(dry, off, lens))):
            one = ref.plan_one(aug.policy, seed, step, b, len(x), T)
            for key in ("rate", "out_len", "stretch_len"):
                assert one[key] == plan[key][b], (key, b)
            assert one["stretch_rate"] == plan["stretch_rate"][b] and one["tempo"] == plan["tempo"][b]
            assert len(y) == one["out_len"]
            stretched += one["stretch_rate"] != 1.0
            pitched += one["semitones"] != 0.0
            L, M, W, _ = resample_ref.plan(one["rate"])
            tab = resample_ref.table(one["rate"]).astype(np.float32)
            chain = {}
            for dtype in (np.float64, np.float32):
                s = ref.time_stretch(x, one["stretch_rate"], dtype)
                assert len(s) == one["stretch_len"]
                if one["rate"] == 16000:
                    chain[dtype] = s
                elif dtype is np.float64:
                    chain[dtype] = resample_ref.resample(s, L, M, W, tab.astype(np.float64))
                else:
                    chain[dtype] = resample_ref.resample_f32(s, L, M, W, tab)
            yard = ref.rel_err(chain[np.float32], chain[np.float64])
            err = ref.rel_err(y, chain[np.float64])
            print("step %d clip %d: rate %d rho %.4f: %.3g (yardstick %.3g)" % (step, b, one["rate"], one["stretch_rate"], err, yard))
            if one["stretch_rate"] == 1.0 and one["rate"] == 16000:
                assert np.array_equal(bits(y), bits(x))
            else:
                assert err <= 2 * yard, (step, b, err, yard)
        # (b) reverb and noise over the stretched buffer, then the log-mel
        full = wave_loader.WaveAug(SPEED + "," + VOICE + "," + ROOM + ",white=1@10:10", seed)
        wet, off_w, lens_w, plan_w = ws.waves(PAIRS, full, step)
        assert np.array_equal(off, off_w) and np.array_equal(lens, lens_w)
        assert np.array_equal(plan_w["stretch_rate"], plan["stretch_rate"]) and np.array_equal(plan_w["rate"], plan["rate"])
        rev = ops.reverb(dry, off, lens, ops.reverb_table(plan_w), seed, step)
        want = ops.wave_mix(rev.clone(), off, lens, ops.wave_mix_table(plan_w), seed, step)
        for a, b2, c in zip(_clips(wet, off, lens), _clips(want, off, lens), _clips(dry, off, lens)):
            assert np.array_equal(bits(a), bits(b2)) and not np.array_equal(bits(a), bits(c))
        mel, frames = ws.mel(PAIRS, full, step)
        direct = torch.empty_like(mel)
        audio.launch(audio.prepare_flat(want, off, lens, T, torch.device(gpu)), direct, "nhwc")
        assert torch.equal(mel, direct) and frames.tolist() == np.minimum(1 + lens // 160, T).tolist()
        # the rest of the reference chain, each stage's numpy reference over the stage before it as the device made it,
        # within that stage's own bound: reverb_ref (the dot-product bound of tests/test_reverb_gpu.py), waveaug_ref
        # (twice its fp32 restatement, tests/test_waveaug_gpu.py) and logmel_ref (GAMMA, tests/test_logmel_gpu.py)
        got_mel = mel.cpu().numpy()
        for b, (d, r, w) in enumerate(zip(_clips(dry, off, lens), _clips(rev, off, lens), _clips(wet, off, lens))):
            taps = int(plan_w["taps"][b])
            assert taps >= 3200
            h = reverb_ref.rir(plan_w["alpha"][b], plan_w["slope"][b], taps, b, seed, step)
            err = np.abs(r.astype(np.float64) - reverb_ref.convolve(d, h))
            assert np.all(err <= ((taps + 32) + 16) * U * reverb_ref.convolve(np.abs(d), np.abs(h))), (step, b, "reverb")
            args = (r, plan_w["g_white"][b], 0.0, None, 0, seed, step, b)
            noisy = waveaug_ref.mix(*args)
            assert plan_w["g_white"][b] > 0 and ref.rel_err(w, noisy) <= 2 * ref.rel_err(waveaug_ref.mix_f32(*args), noisy), (step, b, "noise")
            db, keep, ref64 = logmel_ref.log_mel(w.astype(np.float64), target_length=T)
            P64, A = logmel_ref.mel_power(w.astype(np.float64))
            p, a = P64[:keep].T, A[:keep].T
            ok = p >= 100 * GAMMA * a
            limit = 4.343 * 1.02 * (GAMMA * a / np.maximum(p, 1e-300) + GAMMA * A.max() / ref64) + 2e-4
            assert keep == frames[b] and np.all(np.abs(got_mel[b, 0, :keep].T - db[:, :keep])[ok] <= limit[ok]), (step, b, "log-mel")
        # (c) perturb (extraction) is the same composition without a pool
        views = wave_loader.perturb(waves, full, gpu, step)
        for v, b2 in zip(views, _clips(wet, off, lens)):
            assert np.array_equal(bits(v.cpu().numpy()), bits(b2))
    assert stretched >= 3 and pitched >= 2
    # (d) without the keys nothing of it runs
    for name in ("time_stretch", "stretch_table", "device_stretch_basis"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the stretch ran without tempo= or pitch="))
    ws.waves(PAIRS, wave_loader.WaveAug(SPEED + "," + ROOM, seed), 7)
    ws.waves(PAIRS)
    # and with them, where every clip draws rate 1
    still, off_s, lens_s, plan_s = ws.waves(PAIRS, wave_loader.WaveAug("tempo=1.0,pitch=0", seed), 7)
    assert np.all(plan_s["stretch_rate"] == 1.0)
    plain, off_p, lens_p, _ = ws.waves(PAIRS)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(_clips(still, off_s, lens_s), _clips(plain, off_p, lens_p)))


# ---- 5. resume --------------------------------------------------------------------------------------------------------------------
TRAIN_SPEC = VOICE + ",speed=0.9/1.0/1.1,white=0.7@5:25"


@pytest.mark.parametrize("kind", ["head", "encoder"])
def test_trainer_resumes_bit_for_bit_under_pitch_and_tempo(gpu, tree, kind):  # noqa: F811
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
    # the control: the same draws without the two keys are other batches
    first = []
    for spec in (TRAIN_SPEC, TRAIN_SPEC.replace(VOICE + ",", "")):
        random.seed(41)
        first.append(next(ws.batches(3, gpu, True, aug=wave_loader.WaveAug(spec, seed=9), step=lambda: 0))[0].clone())
    assert torch.equal(first[0][0, 0, :8], seen[0]) and not torch.equal(first[0], first[1])


def test_cli_resumes_bit_for_bit_under_pitch_and_tempo(gpu, tmp_path, capsys):
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
    # the control: without the two keys the run ends elsewhere
    train_encoder.main(COMMON + ["--data_dir", root, "--waveaug", TRAIN_SPEC.replace(VOICE + ",", ""), "--output_dir", out_p,
                                 "--epoch", "2"])
    assert result_lines(capsys.readouterr().out) != result_lines(straight)
    with pytest.raises(SystemExit, match="pitch=13"):
        train_encoder.main(COMMON + ["--data_dir", root, "--waveaug", "pitch=13", "--output_dir", out_p])


# ---- 6. extraction ----------------------------------------------------------------------------------------------------------------
def test_extraction_under_pitch_and_tempo(gpu, tmp_path):
    from encoder_ref import build_encoder
    from speech_to_image_translation_without_text_amd import extract_audio_feature as E
    root = str(tmp_path)
    make_tree(root, "train", [[0.7, 0.9, 0.3, 1.0, 0.8], [1.1, 0.66, 0.75, 0.72, 0.95]], seed=6)
    model_path = os.path.join(root, "encoder.pt")
    torch.save({"state_dict": build_encoder().state_dict()}, model_path)
    common = ["--model", model_path, "--bidirectional", "--data_dir", root, "--splits", "train", "--batch_size", "4"]
    E.main(common + ["--audio_switch", "clean"])
    E.main(common + ["--audio_switch", "a", "--waveaug", "pitch=3", "--waveaug_seed", "4"])
    E.main(common + ["--audio_switch", "b", "--waveaug", "pitch=3", "--waveaug_seed", "4"])
    E.main(common + ["--audio_switch", "c", "--waveaug", "tempo=1.25", "--waveaug_seed", "4"])
    clean, a, b, c = (_pickles(root, s) for s in ("clean", "a", "b", "c"))
    assert a == b and a[0] != clean[0] and c[0] != clean[0] and c[0] != a[0]
    assert c[1] != clean[1]                                                            # a tempo changes the lengths
    with pytest.raises(SystemExit, match="tempo=3"):
        E.main(common + ["--waveaug", "tempo=3"])
