"""Host side of the encoder's fused optimiser and data-parallel feeding: the fp64 restatement of Adam with L2 weight decay
against torch.optim.Adam, the mutants it must tell itself from, `shard_order` against torch's DistributedSampler, the
feeders' `order` argument, and the new symbol's declaration and binding.  No GPU."""
import os
import random
import re

import numpy as np
import pytest
import torch
from torch.utils.data.distributed import DistributedSampler

import encoder_dp_ref as D
from speech_loader_ref import make_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,gscale", [(D.TEST_WD, 1.0), (0.0, 1.0), (1e-5, 1.0), (D.TEST_WD, 0.5)])
def test_restatement_is_torch_adam_with_weight_decay(wd, gscale):
    """Three steps in fp64; with gscale = 0.5 torch.optim.Adam is given the halved gradients."""
    p0, grads = D.kernel_case(1025)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=D.ADAM["lr"], betas=(D.ADAM["b1"], D.ADAM["b2"]), eps=D.ADAM["eps"], weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for k, g in enumerate(grads):
        q.grad = (g * gscale).clone()
        opt.step()
        p, m, v = D.adam_l2_ref(p, g, m, v, wd=wd, step=k + 1, gscale=gscale, **D.ADAM)
        st = opt.state[q]
        assert D.rel_err(p, q) < 1e-12 and D.rel_err(m, st["exp_avg"]) < 1e-12 and D.rel_err(v, st["exp_avg_sq"]) < 1e-12


@pytest.mark.parametrize("n", D.KERNEL_SIZES)
def test_mutants_clear_ten_times_the_kernel_bound(n):
    """On the GPU test's own inputs and weight decay every mutant moves the PARAMETERS by more than 10 x their bound."""
    ref = D.kernel_ref(n, torch.float64, D.TEST_WD, D.TEST_GSCALE)
    for mutant in D.KERNEL_MUTANTS:
        e = D.rel_err(D.kernel_ref(n, torch.float64, D.TEST_WD, D.TEST_GSCALE, mutant)[0], ref[0])
        print("n=%d %s: p differs by %.3e (10 x bound %.2e)" % (n, mutant, e, 10 * D.KERNEL_BOUNDS["p"]))
        assert e > 10 * D.KERNEL_BOUNDS["p"], mutant


def test_the_reference_weight_decay_would_not_show_a_dropped_gscale():
    """Why the tests do not run at the trainers' 1e-5: Adam is nearly invariant to the scale of its gradient, so with a
    decay term that small a forgotten gscale stays inside 10 x the bound."""
    for n in D.KERNEL_SIZES:
        ref = D.kernel_ref(n, torch.float64, 1e-5, D.TEST_GSCALE)
        e = D.rel_err(D.kernel_ref(n, torch.float64, 1e-5, D.TEST_GSCALE, "no_gscale")[0], ref[0])
        assert e < 10 * D.KERNEL_BOUNDS["p"], (n, e)


def test_kernel_bounds_are_twice_the_fp32_yardstick():
    """The recorded yardsticks are what the restatement gives over ALL sizes of the GPU test, the second-trip size included:
    elementwise IEEE arithmetic, the same on any CPU, so the figures must agree from both sides."""
    got = D.kernel_yardstick()
    print(got)
    for k, y in D.KERNEL_YARDSTICK.items():
        assert got[k] == pytest.approx(y, rel=0.01), (k, got[k], y)
        assert D.KERNEL_BOUNDS[k] == 2 * y
    assert D.SECOND_TRIP > 4 * 256 * 8192                     # lane 0 takes a second trip (s2i_elementwise.h grid_for)
    header = open(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc", "s2i_elementwise.h")).read()
    assert "int cap = 2048 * 4" in header and "int block = 256" in header


def test_trajectory_bounds_are_twice_the_fp32_yardstick():
    """measure_yardsticks again (about 15 s).  These figures come from sign flips of elements whose gradient lies in the fp32
    backward's rounding noise, so another CPU's summation order may move them; the window is a factor of 1.5 either way,
    which still refuses a recorded yardstick inflated to loosen a bound."""
    got = D.measure_yardsticks()
    for k, y in D.TRAJ_YARDSTICK.items():
        print("%s: %.3e (recorded %.3e)" % (k, got[k], y))
        assert y / 1.5 <= got[k] <= y * 1.5, (k, got[k], y)
        assert D.TRAJ_BOUNDS[k] == 2 * y
    for k, y in D.KERNEL_YARDSTICK.items():
        assert got["adam_" + k] == pytest.approx(y, rel=0.01)
    assert got["_dp_mutant_no_allreduce"] > 0.5 and got["_dp_mutant_no_scale"] > 0.2


def test_update_err_ignores_a_few_flips_and_sees_a_wrong_step():
    g = torch.Generator().manual_seed(1)
    start = {"w": torch.randn(100000, generator=g, dtype=torch.float64)}
    ref = {"w": start["w"] - 1e-3 * torch.sign(torch.randn(100000, generator=g, dtype=torch.float64))}
    flipped = {"w": ref["w"].clone()}
    flipped["w"][:5] = 2 * start["w"][:5] - ref["w"][:5]
    assert D.update_err(ref, ref, start) == 0.0
    assert D.update_err(flipped, ref, start) < 2e-2 and D.rel_err(flipped["w"], ref["w"]) > 4e-4
    assert D.update_err(start, ref, start) == pytest.approx(1.0)


def test_data_parallel_restatement_is_the_trajectory_and_rejects_its_mutants():
    """dp_steps with one rank is encoder_conv_train_ref.trajectory (stock torch.optim.Adam; the hyperparameters differ by
    their rounding to fp32 only), and with two ranks a missing all-reduce or a missing 1 / world lies far outside the GPU
    test's bound."""
    import encoder_conv_train_ref as R
    net = R.stack_net(bidirectional=True, nhidden=512)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    case = R.trainer_case()
    _, traj = R.trajectory(net, *case, 2, torch.float64, **R.TRAINER_LOSS)
    _, one, running = D.dp_steps(net, [case], 2, torch.float64, wd=1e-5, **R.TRAINER_LOSS)
    e = D.update_err(one, traj, start)
    print("one rank against the trajectory: %.3e" % e)
    assert e < 1e-6 and all(D.rel_err(running[n], traj[n]) < 1e-6 for n in running)
    cases = [D.dp_case(r) for r in range(D.DP_WORLD)]
    losses, ref, _ = D.dp_steps(net, cases, D.DP_STEPS, torch.float64, **R.TRAINER_LOSS)
    assert all(abs(float(row[0]["loss"]) - float(row[1]["loss"])) > 1e-2 for row in losses)      # the ranks' data differ
    for mutant in ("no_allreduce", "no_scale"):
        _, wrong, _ = D.dp_steps(net, cases, D.DP_STEPS, torch.float64, mutant=mutant, **R.TRAINER_LOSS)
        e = D.update_err(wrong, ref, start)
        print("%s: %.3e (bound %.2e)" % (mutant, e, D.TRAJ_BOUNDS["dp_update"]))
        assert e > 100 * D.TRAJ_BOUNDS["dp_update"], mutant


# ---- sharding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("N", [1, 2, 7, 8, 9])
def test_shard_order_is_distributed_samplers_rule(N, world):
    from speech_to_image_translation_without_text_amd.train_encoder_head import shard_order
    order = list(range(N))
    random.Random(5 + N).shuffle(order)
    before = list(order)
    shares = [shard_order(order, r, world) for r in range(world)]
    assert order == before
    for r in range(world):
        sampler = DistributedSampler(range(N), num_replicas=world, rank=r, shuffle=False)
        assert shares[r] == [order[i] for i in sampler], (N, world, r)
    assert {len(s) for s in shares} == {-(-N // world)}
    assert set().union(*shares) == set(range(N))
    with pytest.raises(ValueError):
        shard_order(order, world, world)


# ---- the feeders' order argument ------------------------------------------------------------------------------------------------
SPEC = [[1.0, 0.3, 1.2], [0.3, 0.9], [0.7, 1.1], [0.8], [0.3, 1.3, 1.0]]


@pytest.fixture
def split(tmp_path, monkeypatch):
    """A SplitData whose log_mel is a stand-in (no GPU here): the "mel" of a batch holds each waveform's length and first
    sample, which name the utterance."""
    from speech_to_image_translation_without_text_amd import audio, train_encoder_head
    root = str(tmp_path)
    make_tree(root, "train", SPEC, seed=8)

    def fake_log_mel(waves, layout="nhwc", device=None, **kw):
        mel = torch.tensor([[len(w), float(w[0])] for w in waves], dtype=torch.float64)
        return mel, np.array([audio.n_frames(len(w)) for w in waves], dtype=np.int64)
    monkeypatch.setattr(audio, "log_mel", fake_log_mel)
    return train_encoder_head.SplitData(root, "train", "birds")


def _present_batches(split, batch_size, shuffle):
    """SplitData.batches as it stood before it took `order`, item numbers added."""
    from speech_to_image_translation_without_text_amd import audio
    from speech_to_image_translation_without_text_amd.extract_audio_feature import MIN_FRAMES
    order = list(range(len(split)))
    if shuffle:
        random.shuffle(order)
    for s in range(0, len(order), batch_size):
        drawn = [split.draw(i) for i in order[s:s + batch_size]]
        mel, frames = audio.log_mel([w for _, w, _ in drawn], layout="nhwc", device=None)
        image = torch.from_numpy(np.stack([v for v, _, _ in drawn])).float()
        yield order[s:s + batch_size], (mel, (frames // MIN_FRAMES).tolist(), image,
                                        torch.tensor([c for _, _, c in drawn], dtype=torch.int64))


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def _resident(split):
    """A ResidentSpeechSet without its device pool: `mel` answers with the utterance numbers."""
    from speech_to_image_translation_without_text_amd import speech_loader
    rs = object.__new__(speech_loader.ResidentSpeechSet)
    rs.split, rs.device, rs.T = split, torch.device("cpu"), 2048
    rs.frames = speech_loader.scan_frames(split, workers=2)
    rs.mel = lambda utterances: (torch.tensor(utterances, dtype=torch.int64),
                                 np.array([rs.frames[i][u] for i, u in utterances], dtype=np.int64))
    return rs


@pytest.mark.parametrize("shuffle", [False, True])
def test_batches_without_order_are_what_they_were(split, shuffle):
    random.seed(21)
    present = list(_present_batches(split, 2, shuffle))
    state = random.getstate()
    for kwargs in ({}, {"order": None}):
        random.seed(21)
        got = list(split.batches(2, None, shuffle, **kwargs))
        assert random.getstate() == state
        assert len(got) == len(present) == 3 and all(_same(a, b[1]) for a, b in zip(got, present))
    # the resident feeder goes through the same items with the same draws
    rs = _resident(split)
    random.seed(21)
    res = list(rs.batches(2, "cpu", shuffle, order=None))
    assert random.getstate() == state
    assert [b[0][:, 0].tolist() for b in res] == [items for items, _ in present]
    assert all(a[1] == b[1][1] and torch.equal(a[2], b[1][2]) and torch.equal(a[3], b[1][3]) for a, b in zip(res, present))


def test_batches_with_an_order_yield_exactly_those_items(split):
    order = [4, 0, 0, 2, 3]                                  # a rank's share: in the given order, a padded item twice
    rs = _resident(split)
    states = []
    for shuffle in (False, True):                            # not looked at
        random.seed(3)
        host = list(split.batches(2, None, shuffle, order=order))
        state = random.getstate()
        states.append(state)
        random.seed(3)
        res = list(rs.batches(2, "cpu", shuffle, order=order))
        assert random.getstate() == state
        assert [b[0][:, 0].tolist() for b in res] == [[4, 0], [0, 2], [3]]
        assert [b[3].tolist() for b in host] == [[split.labels[i] for i in items] for items in ([4, 0], [0, 2], [3])]
        assert all(a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) for a, b in zip(host, res))
        # the views are the items' own
        for b, items in zip(host, ([4, 0], [0, 2], [3])):
            for row, i in zip(b[2], items):
                assert any(np.array_equal(row.numpy(), v) for v in split.image[i])
    assert states[0] == states[1]                            # no shuffle was drawn in front of the first item


# ---- the C surface, the bindings and the CLI -------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_exported_and_refuses_bad_arguments():
    from speech_to_image_translation_without_text_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    decl = re.search(r"int s2i_adam_l2_step\(([^)]*)\)", header)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == [
        "float* p", "const float* g", "float* m", "float* v", "long long n", "float lr", "float beta1", "float beta2",
        "float eps", "float weight_decay", "int step", "const int* step_dev", "float gscale", "void* stream"]
    assert "train_audio_encoder.py:462" in header
    assert "s2i_adam_l2_step" in _lib.EXPORTED_SYMBOLS and callable(ops.adam_l2_step)
    assert len(_lib._SIGNATURES["s2i_adam_l2_step"][1]) == 14
    lib = _lib.load()
    assert lib.s2i_version() == _lib.ABI_VERSION == 7
    one = 16                                                 # any non-null address: the checks run before a launch
    args = lambda p=one, g=one, m=one, v=one, n=4, step=1, sd=None: (p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-5, step, sd,
                                                                     1.0, None)
    for bad in (args(p=None), args(g=None), args(m=None), args(v=None), args(n=0), args(n=-4)):
        assert lib.s2i_adam_l2_step(*bad) != 0 and b"adam_l2_step: bad args" in lib.s2i_last_error()
    for step in (0, -1):
        assert lib.s2i_adam_l2_step(*args(step=step)) != 0 and b"step must be >= 1" in lib.s2i_last_error()


def test_flatnet_defaults_are_unchanged_and_trainers_take_the_new_arguments():
    import inspect
    from speech_to_image_translation_without_text_amd import encoder_train, trainer
    sig = inspect.signature(trainer.FlatNet.__init__).parameters
    assert sig["weight_decay"].default == 0.0 and sig["params"].default is None and sig["betas"].default == (0.5, 0.999)
    for cls in (encoder_train.HeadTrainer, encoder_train.EncoderTrainer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["fused_adam"].default is False and sig["distributed"].default is False


def test_cli_flags():
    from speech_to_image_translation_without_text_amd import train_encoder as T, train_encoder_head as TH
    a = T.get_parser().parse_args(["--data_dir", "/data"])
    assert not a.fused_adam and not a.distributed and a.dist_backend == "nccl" and a.resume == ""
    assert TH.trainer_kwargs(a)["fused_adam"] is False and TH.trainer_kwargs(a)["distributed"] is False
    b = TH.get_parser().parse_args(["--model", "m.pt", "--fused_adam", "--distributed", "--dist_backend", "gloo", "--resume",
                                    "out/latest.pth"])
    assert b.fused_adam and b.distributed and b.dist_backend == "gloo" and b.resume == "out/latest.pth"
    assert TH.trainer_kwargs(b)["fused_adam"] and TH.trainer_kwargs(b)["distributed"]
    c = TH.get_parser().parse_args(["--resume", "out/latest.pth"])          # --resume stands in for --model
    assert c.model == "" and c.resume == "out/latest.pth"
    with pytest.raises(SystemExit):
        TH.get_parser().parse_args(["--fused_adam"])                          # neither of the two
    for mod in (T, TH):
        assert "torch.distributed.run --nproc-per-node" in mod.__doc__ and "--distributed" in mod.__doc__
        assert "Not built: data-parallel" not in mod.__doc__


def test_resume_epoch_reads_meta(tmp_path):
    from speech_to_image_translation_without_text_amd import train_encoder_head as TH
    path = str(tmp_path / "c.pth")
    torch.save({"meta": {"epoch": 7}, "state_dict": {}}, path)
    assert TH.resume_epoch(path) == 7
    torch.save({"state_dict": {}}, path)
    with pytest.raises(SystemExit):
        TH.resume_epoch(path)


def test_skip_epochs_is_step_lr():
    """The unfused trainer's StepLR after n epochs, and the same rule on a bare learning rate (what the fused trainer keeps;
    it cannot be built here: its buffers live on the device)."""
    from encoder_ref import small_encoder
    from speech_to_image_translation_without_text_amd import encoder_train
    tr = encoder_train.HeadTrainer(small_encoder(True, 64), lr=1e-3, step_size=3, gamma=0.2)
    lrs = []
    for _ in range(7):
        tr.end_epoch()
        lrs.append(tr.lr)
    assert lrs == pytest.approx([1e-3, 1e-3, 2e-4, 2e-4, 2e-4, 4e-5, 4e-5])
    tr2 = encoder_train.HeadTrainer(small_encoder(True, 64), lr=1e-3, step_size=3, gamma=0.2)
    tr2.skip_epochs(6)
    assert tr2.lr == pytest.approx(4e-5) and tr2.epoch == 6 and tr2.steps == 0
