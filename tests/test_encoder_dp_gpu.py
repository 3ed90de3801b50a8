"""The speech encoder's fused optimiser and data-parallel step on the GPU (references: tests/encoder_dp_ref.py).

s2i_adam_l2_step against the fp64 restatement of torch.optim.Adam(weight_decay), per buffer at max|got - ref| / max|ref|:

    buffer   yardstick (CPU fp32 vs fp64)   bound      worst seen on the MI355X
    p        1.49e-7                        2.98e-7    1.21e-7
    m        1.86e-7                        3.72e-7    1.51e-7
    v        2.29e-7                        4.58e-7    2.12e-7

The bound is twice the yardstick (encoder_dp_ref.KERNEL_BOUNDS); every test prints what it measured.  The trainers with
fused_adam are held to the fp64 trajectories of encoder_train_ref / encoder_conv_train_ref at the bounds the unfused
trainers' tests apply (loss scalars, RNN.* after three steps) and, for what those tests do not compare, at twice the fp32
restatement's own error (encoder_dp_ref.TRAJ_BOUNDS, with the reason for its metric).  Two gloo ranks on one GPU, a
world-size-1 RCCL group and the CLIs follow.  Every process started here has its own time limit and nothing is retried.
"""
import copy
import os
import socket
import subprocess
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

import encoder_conv_train_ref as R
import encoder_dp_ref as D
import encoder_ref
import encoder_train_ref as TR
from helpers import assert_close
from speech_loader_ref import make_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech_to_image_translation_without_text_amd"
TRAJ_LOSS = 3.8e-4        # class traj_loss of tests/test_encoder_conv_train_gpu.py
UPDATED = 2.1e-4          # class updated of tests/test_encoder_train_gpu.py: RNN.* after three optimiser steps
SENTINEL = 12345.0
PAD = 64                  # floats in front of and behind every buffer (the buffer itself stays 256-byte aligned)
PROCESS_LIMIT = 300       # seconds for a spawned process


def dev(t, gpu):
    return t.float().contiguous().to(gpu)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
_KERNEL_REF = {}


def kernel_ref(n):
    if n not in _KERNEL_REF:
        _KERNEL_REF[n] = D.kernel_ref(n, torch.float64, D.TEST_WD, D.TEST_GSCALE)
    return _KERNEL_REF[n]


def guarded(values, gpu):
    """-> (whole buffer, the view the kernel is given): `values` between two sentinel regions."""
    n = values.numel()
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32)
    buf[PAD:PAD + n] = values.float()
    buf = buf.to(gpu)
    return buf, buf[PAD:PAD + n]


def guards_intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def run_steps(ops, gpu, n, use_dev, step_fn):
    """KERNEL_STEPS consecutive launches of step_fn(p, g, m, v, step=..., step_dev=...) on guarded buffers from zero moments
    -> (p, m, v) views; asserts the guards and the gradient buffer."""
    p0, grads = D.kernel_case(n)
    bufs = [guarded(t, gpu) for t in (p0, grads[0], torch.zeros(n), torch.zeros(n))]
    (_, p), (_, g), (_, m), (_, v) = bufs
    step_dev = torch.zeros(1, dtype=torch.int32, device=gpu) if use_dev else None
    for k, gk in enumerate(grads):
        g.copy_(gk.float())
        if use_dev:
            ops.increment(step_dev)
        step_fn(p, g, m, v, step=0 if use_dev else k + 1, step_dev=step_dev)
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs), "a launch wrote outside its %d elements" % n
    assert torch.equal(g.cpu(), grads[-1].float()), "the gradient buffer was written"
    if use_dev:
        assert int(step_dev) == D.KERNEL_STEPS
    return p, m, v


@pytest.mark.parametrize("use_dev", [True, False], ids=["step_dev", "host_step"])
@pytest.mark.parametrize("n", D.KERNEL_SIZES)
def test_adam_l2_step_against_fp64(gpu, n, use_dev):
    from speech_to_image_translation_without_text_amd import ops
    a = D.ADAM

    def step_fn(p, g, m, v, step, step_dev):
        ops.adam_l2_step(p, g, m, v, a["lr"], a["b1"], a["b2"], a["eps"], D.TEST_WD, step=step, step_dev=step_dev,
                         gscale=D.TEST_GSCALE)
    got = run_steps(ops, gpu, n, use_dev, step_fn)
    errs = [(k, D.rel_err(x, y)) for k, x, y in zip("pmv", got, kernel_ref(n))]
    for k, e in errs:
        print("n=%d %s %s: %.3e (bound %.2e)" % (n, "step_dev" if use_dev else "host step", k, e, D.KERNEL_BOUNDS[k]))
    bad = ["%s %.3e > %.2e" % (k, e, D.KERNEL_BOUNDS[k]) for k, e in errs if not e <= D.KERNEL_BOUNDS[k]]
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("use_dev", [True, False], ids=["step_dev", "host_step"])
@pytest.mark.parametrize("n", D.KERNEL_SIZES)
def test_without_weight_decay_it_is_adam_step_bit_for_bit(gpu, n, use_dev):
    from speech_to_image_translation_without_text_amd import ops
    a = D.ADAM
    l2 = lambda p, g, m, v, step, step_dev: ops.adam_l2_step(p, g, m, v, a["lr"], a["b1"], a["b2"], a["eps"], 0.0, step=step,
                                                            step_dev=step_dev, gscale=D.TEST_GSCALE)
    plain = lambda p, g, m, v, step, step_dev: ops.adam_step(p, g, m, v, a["lr"], a["b1"], a["b2"], a["eps"], step=step,
                                                             step_dev=step_dev, gscale=D.TEST_GSCALE)
    x = run_steps(ops, gpu, n, use_dev, l2)
    y = run_steps(ops, gpu, n, use_dev, plain)
    p0 = D.kernel_case(n)[0].float()
    assert not torch.equal(x[0].cpu(), p0)
    for k, s, t in zip("pmv", x, y):
        assert torch.equal(s, t), "%s differs from s2i_adam_step at n=%d" % (k, n)


def test_wrapper_refuses_what_the_kernel_refuses(gpu):
    from speech_to_image_translation_without_text_amd import _lib, ops
    t = torch.zeros(8, device=gpu)
    with pytest.raises(_lib.S2IError, match="step must be >= 1"):
        ops.adam_l2_step(t, t.clone(), t.clone(), t.clone(), 1e-3, 0.9, 0.999, 1e-8, 1e-5, step=0)
    with pytest.raises(_lib.S2IError, match="bad args"):
        ops.adam_l2_step(t[:0], t[:0], t[:0], t[:0], 1e-3, 0.9, 0.999, 1e-8, 1e-5, step=1)
    with pytest.raises(_lib.S2IError):
        ops.adam_l2_step(t.cpu(), t.cpu(), t.cpu(), t.cpu(), 1e-3, 0.9, 0.999, 1e-8, 1e-5, step=1)
    assert float(t.abs().sum()) == 0.0


# ---- the fused trainers ------------------------------------------------------------------------------------------------------------
def assert_flat(tr, trained):
    """Every trained parameter and its .grad are views of the flat buffers at the parameter's 16-byte-aligned offset."""
    f = tr.flat
    assert [id(p) for p in f.params] == [id(p) for p in trained]
    for p, o, n in zip(f.params, f.offsets, f.sizes):
        assert o % 4 == 0 and p.numel() == n
        assert p.data_ptr() == f.p.data_ptr() + 4 * o, "a parameter left the flat buffer"
        assert p.grad is not None and p.grad.data_ptr() == f.g.data_ptr() + 4 * o, "a .grad left the flat buffer"
    assert f.p.dtype == torch.float32 and f.p.shape == f.g.shape == f.m.shape == f.v.shape == (f.total,)
    lo, hi = f.p.data_ptr(), f.p.data_ptr() + 4 * f.total
    assert all(lo <= q.data_ptr() < hi for q in tr.params), "ops.lstm_params was fetched before the re-homing"


def test_fused_encoder_trainer_follows_the_fp64_trajectory(gpu):
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer
    net = R.stack_net(bidirectional=True, nhidden=512)
    mel, lens, image, label = R.trainer_case()
    ref_losses, ref_state = R.trajectory(net, mel, lens, image, label, R.TRAINER_STEPS, torch.float64, **R.TRAINER_LOSS)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    model = copy.deepcopy(net).to(gpu)
    trainer = EncoderTrainer(model, fused_adam=True, **R.TRAINER_LOSS)
    assert trainer.optimizer is None and trainer.flat.weight_decay == 1e-5 and trainer.lr == 1e-3
    assert_flat(trainer, list(model.parameters()))
    mel_d = dev(mel, gpu)
    errs = []
    for step in range(R.TRAINER_STEPS):
        got = trainer.step(mel_d, lens, image.float(), label)
        assert_flat(trainer, list(model.parameters()))            # after zero_grad and backward the views still alias
        for k in ("loss", "loss_jel", "loss_l1"):
            errs.append((TRAJ_LOSS, "step %d %s (%.6f)" % (step, k, float(got[k])),
                         abs(float(got[k]) - float(ref_losses[step][k])) / abs(float(ref_losses[step]["loss"]))))
    torch.cuda.synchronize()
    assert int(trainer.flat.step_dev) == trainer.steps == R.TRAINER_STEPS and not model.training
    after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    assert not [n for n in start if torch.equal(after[n], start[n])], "parameters the steps left unchanged"
    assert int(after["Conv.0.num_batches_tracked"]) == R.TRAINER_STEPS
    errs.append((D.TRAJ_BOUNDS["traj_update"], "parameters, update_err", D.update_err(after, ref_state, start, list(start))))
    errs.append((D.TRAJ_BOUNDS["traj_running"], "running statistics, worst rel_err",
                 max(R.rel_err(after[n], ref_state[n]) for n in ref_state if "running_" in n)))
    # the inference path folds the weights and running statistics the kernels have written through raw pointers
    emb = trainer.embed(mel_d, lens)
    cpu_model = copy.deepcopy(net)
    cpu_model.load_state_dict(after)
    _, sent = encoder_ref.encode(encoder_ref.fold(cpu_model), mel, lens)
    assert_close(emb, sent, rtol=1e-3, atol=1e-5, what="embedding after %d fused steps" % R.TRAINER_STEPS)
    # StepLR on the host-side learning rate
    trainer.step_size, trainer.gamma = 2, 0.5
    lrs = []
    for _ in range(4):
        trainer.end_epoch()
        lrs.append(trainer.lr)
    assert lrs == pytest.approx([1e-3, 5e-4, 5e-4, 2.5e-4])
    for bound, what, e in errs:
        print("%s: %.3e (bound %.2e)" % (what, e, bound))
    bad = ["%s %.3e > %.2e" % (what, e, bound) for bound, what, e in errs if not e <= bound]
    assert not bad, "; ".join(bad)


def test_fused_head_trainer_three_steps_and_a_fresh_embedding(gpu):
    """tests/test_encoder_train_gpu.py's three steps through the frozen conv stack, with fused_adam: RNN.* at its `updated`
    bound; and `embed` afterwards uses the new weights, although no version counter has moved."""
    import test_encoder_train_gpu as HT
    from speech_to_image_translation_without_text_amd import encoder_train
    net = encoder_ref.small_encoder(True, 64).to(gpu)
    tr = encoder_train.HeadTrainer(net, fused_adam=True)
    assert_flat(tr, list(net.RNN.parameters()))
    start = [p.detach().double().cpu() for p in tr.params]
    frozen = HT._frozen_state(net)
    g = torch.Generator().manual_seed(31)
    batches, losses = [], []
    probe = (torch.randn(8, 1, 512, 40, generator=g) * 20 - 40).to(gpu)
    probe_lens = TR.case_lens(8, 8)
    before = tr.embed(probe, probe_lens).clone()                   # fills the cache of folded weights
    for _, lens, image, label in TR.train_case():
        mel = (torch.randn(8, 1, 512, 40, generator=g) * 20 - 40).to(gpu)
        feat = tr.features(mel)
        batches.append((feat[:, 0].double().cpu(), lens, image, label))
        losses.append(tr.step(mel, lens, image.float(), label)["loss"].double().cpu())
        assert_flat(tr, list(net.RNN.parameters()))
    torch.cuda.synchronize()
    assert HT.BOUNDS["updated"] == UPDATED
    HT._check_training(net, tr, losses, batches, start, {}, frozen)
    after = tr.embed(probe, probe_lens)
    fresh = encoder_ref.small_encoder(True, 64)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    expect = encoder_train.HeadTrainer(fresh.to(gpu)).embed(probe, probe_lens)
    e_new, e_old = R.rel_err(after, expect), R.rel_err(before, expect)
    print("embed after the steps against a fresh model of the same weights: %.3e; the embedding of the old weights: %.3e"
          % (e_new, e_old))
    assert e_old > 1e-3, "stale folded weights would not show in this test"
    assert e_new <= 1e-6, "embed ran on stale folded weights"


# ---- spawned processes ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn(fn, args, nprocs):
    """mp.spawn with a time limit of its own: past it the processes are killed and the test fails."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + PROCESS_LIMIT
    while not ctx.join(timeout=2):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a spawned rank ran past %d s" % PROCESS_LIMIT)


def _two_rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import encoder_conv_train_ref as R
    import encoder_dp_ref as D
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        gpu = torch.device("cuda:0")
        torch.cuda.set_device(0)
        model = copy.deepcopy(R.stack_net(bidirectional=True, nhidden=512)).to(gpu)
        if rank != 0:                 # rank 0's parameters and BatchNorm buffers must arrive with the broadcast
            with torch.no_grad():
                for p in model.parameters():
                    p.mul_(1.5)
                for b in model.buffers():
                    b.add_(1)
        tr = EncoderTrainer(model, weight_decay=D.TEST_WD, distributed=True, **R.TRAINER_LOSS)
        assert tr.flat is not None and tr.world == world
        mel, lens, image, label = D.dp_case(rank)                 # different data on every rank
        mel_d = mel.float().to(gpu)
        losses = []
        for _ in range(D.DP_STEPS):
            got = tr.step(mel_d, lens, image.float(), label)
            losses.append([float(got[k]) for k in ("loss", "loss_jel", "loss_l1")])
        torch.cuda.synchronize()
        mine = tr.flat.p.detach().cpu()
        gathered = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(gathered, mine)
        assert all(torch.equal(gathered[0], t) for t in gathered), "the replicas diverged"
        lt = torch.tensor(losses, dtype=torch.float64)
        gl = [torch.zeros_like(lt) for _ in range(world)]
        torch.distributed.all_gather(gl, lt)
        assert not torch.equal(gl[0], gl[1]), "the ranks saw the same data"
        if rank == 0:
            torch.save({"state": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "losses": [t.tolist() for t in gl]},
                       os.path.join(out_dir, "rank0.pt"))
        with open(os.path.join(out_dir, "ok%d" % rank), "w") as fh:
            fh.write("ok")
    finally:
        torch.distributed.destroy_process_group()


def test_two_gloo_ranks_on_one_gpu_follow_the_fp64_data_parallel_step(gpu, tmp_path):
    """Replicas bit-identical, losses different, and rank 0 on the fp64 trajectory of the averaged gradients: without the
    all-reduce or without 1 / world the fp64 restatement's parameters lie 0.78 / 0.29 update lengths away
    (tests/test_encoder_dp_cpu.py), against a bound of 1.1e-3."""
    world = D.DP_WORLD
    spawn(_two_rank_worker, (world, _free_port(), str(tmp_path)), world)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(world))
    out = torch.load(str(tmp_path / "rank0.pt"), map_location="cpu", weights_only=True)
    net = R.stack_net(bidirectional=True, nhidden=512)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    ref_losses, ref_params, ref_running = D.dp_steps(net, [D.dp_case(r) for r in range(world)], D.DP_STEPS, torch.float64,
                                                     **R.TRAINER_LOSS)
    errs = [(D.TRAJ_BOUNDS["dp_update"], "rank 0's parameters, update_err", D.update_err(out["state"], ref_params, start, list(start))),
            (D.TRAJ_BOUNDS["dp_running"], "rank 0's running statistics, worst rel_err",
             max(R.rel_err(out["state"][n], ref_running[n]) for n in ref_running))]
    for r in range(world):
        for s in range(D.DP_STEPS):
            for j, k in enumerate(("loss", "loss_jel", "loss_l1")):
                ref = ref_losses[s][r]
                errs.append((TRAJ_LOSS, "rank %d step %d %s (%.6f)" % (r, s, k, out["losses"][r][s][j]),
                             abs(out["losses"][r][s][j] - float(ref[k])) / abs(float(ref["loss"]))))
    for bound, what, e in errs:
        print("%s: %.3e (bound %.2e)" % (what, e, bound))
    bad = ["%s %.3e > %.2e" % (what, e, bound) for bound, what, e in errs if not e <= bound]
    assert not bad, "; ".join(bad)


def _rccl_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    gpu = torch.device("cuda:0")
    torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=gpu)      # before any other GPU call
    try:
        import encoder_conv_train_ref as R
        import encoder_dp_ref as D
        from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer
        torch.cuda.set_device(0)
        net = R.stack_net(bidirectional=True, nhidden=512)
        mel, lens, image, label = R.trainer_case()
        mel_d = mel.float().to(gpu)
        finals = []
        for distributed in (True, False):
            model = copy.deepcopy(net).to(gpu)
            tr = EncoderTrainer(model, weight_decay=D.TEST_WD, fused_adam=True, distributed=distributed, **R.TRAINER_LOSS)
            for _ in range(2):
                got = tr.step(mel_d, lens, image.float(), label)
            torch.cuda.synchronize()
            finals.append([tr.flat.p.clone(), tr.flat.m.clone(), tr.flat.v.clone(),
                           torch.stack([got[k].reshape(()) for k in ("loss", "loss_jel", "loss_l1", "accu")])])
        assert float(finals[0][1].abs().sum()) > 0
        for a, c in zip(*finals):
            assert torch.equal(a, c), "the RCCL path changed the result of a world-size-1 step"
        with open(os.path.join(out_dir, "ok%d" % rank), "w") as fh:
            fh.write("ok rccl %s" % ".".join(str(v) for v in torch.cuda.nccl.version()))
    finally:
        torch.distributed.destroy_process_group()


def test_world_size_one_rccl_group_matches_the_fused_step(gpu, tmp_path):
    spawn(_rccl_worker, (1, _free_port(), str(tmp_path)), 1)
    assert (tmp_path / "ok0").exists()
    print((tmp_path / "ok0").read_text())


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------
CLIPS = [1.0, 1.25, 0.3, 1.5]


def _cli_tree(root):
    make_tree(root, "train", [CLIPS[k:] + CLIPS[:k] for k in range(4)] + [[1.1, 0.9]], seed=1)      # five items
    make_tree(root, "test", [CLIPS[k:] + CLIPS[:k] for k in range(2)], seed=2)


def _epoch_lines(text):
    return [ln.split(":")[0] for ln in text.splitlines() if ln.startswith("epoch ")]


def test_cli_fused_adam_then_resume(gpu, tmp_path, capsys):
    from speech_to_image_translation_without_text_amd import extract_audio_feature, train_encoder
    root = str(tmp_path)
    _cli_tree(root)
    out_dir = os.path.join(root, "out")
    common = ["--dataset", "birds", "--data_dir", root, "--output_dir", out_dir, "--batch_size", "2", "--bidirectional",
              "--jel_flag", "--seed", "3", "--fused_adam", "--lr_scheduler_step_size", "1"]
    best = train_encoder.main(common + ["--epoch", "1"])
    assert 0.0 <= best <= 100.0 and _epoch_lines(capsys.readouterr().out) == ["epoch 1"]
    first = {}
    for name in ("epoch_1.pth", "latest.pth", "best.pth"):
        path = os.path.join(out_dir, name)
        assert os.path.exists(path), name
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        assert ckpt["meta"] == {"epoch": 1} and set(ckpt) == {"meta", "state_dict"}
        model = extract_audio_feature.load_encoder(path, True, 1, gpu)
        first = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        assert all(bool(torch.isfinite(v.float()).all()) for v in first.values())
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    torch.manual_seed(3)
    seeded = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True)
    init, names = seeded.state_dict(), [n for n, _ in seeded.named_parameters()]
    assert list(first) == list(init)
    changed = [k for k in names if not torch.equal(init[k], first[k])]
    assert any(k.startswith("Conv.") and k.endswith(".0.weight") for k in changed) and any(k.startswith("RNN.") for k in changed)
    train_encoder.main(common + ["--epoch", "2", "--resume", os.path.join(out_dir, "latest.pth")])
    assert _epoch_lines(capsys.readouterr().out) == ["epoch 2"]
    second = torch.load(os.path.join(out_dir, "latest.pth"), map_location="cpu", weights_only=True)
    assert second["meta"] == {"epoch": 2} and os.path.exists(os.path.join(out_dir, "epoch_2.pth"))
    assert int(second["state_dict"]["Conv.0.num_batches_tracked"]) == 2 * int(first["Conv.0.num_batches_tracked"]) == 6
    # Epoch 2 ran at StepLR's second value, lr * gamma = 2e-4, with fresh moments.  Within its first three steps Adam moves
    # no element by more than 1.004 lr a step (Cauchy-Schwarz on the bias-corrected moments' weights), and an element whose
    # gradient keeps its sign moves by about that: the largest move tells 2e-4 from the 1e-3 of a schedule not advanced.
    moved = max(float((second["state_dict"][k] - first[k]).abs().max()) for k in names)
    print("largest parameter move in the resumed epoch: %.3e" % moved)
    assert 2e-4 < moved <= 3 * 2e-4 * 1.01


def test_cli_two_distributed_ranks(gpu, tmp_path):
    """Two processes as torch.distributed.run would start them (gloo, both on GPU 0): five items make three per rank, at
    --batch_size 2 two steps each, the last one ragged."""
    root = str(tmp_path)
    _cli_tree(root)
    port = _free_port()
    outs = [os.path.join(root, "out%d" % r) for r in range(2)]
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        cmd = [sys.executable, "-m", PKG + ".train_encoder", "--distributed", "--dist_backend", "gloo", "--dataset", "birds",
               "--data_dir", root, "--output_dir", outs[r], "--epoch", "1", "--batch_size", "2", "--bidirectional", "--jel_flag",
               "--seed", "3"]
        procs.append(subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    texts = []
    deadline = time.monotonic() + PROCESS_LIMIT
    try:
        for p in procs:
            texts.append(p.communicate(timeout=max(1.0, deadline - time.monotonic())))
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        pytest.fail("a rank of the distributed CLI ran past %d s" % PROCESS_LIMIT)
    for r, (p, (out, err)) in enumerate(zip(procs, texts)):
        assert p.returncode == 0, "rank %d: exit %s\n%s\n%s" % (r, p.returncode, out[-2000:], err[-4000:])
    out0, out1 = texts[0][0], texts[1][0]
    assert _epoch_lines(out0) == ["epoch 1"] and '"test_accu"' in out0
    assert "rank 0 of 2: 2 steps" in out0 and "rank 1 of 2: 2 steps" in out1
    # rank 1 says nothing else (gloo itself reports its connections on stdout)
    assert [ln for ln in out1.splitlines() if ln.strip() and not ln.startswith("[Gloo]")] == ["rank 1 of 2: 2 steps"], out1
    assert sorted(os.listdir(outs[0])) == ["best.pth", "epoch_1.pth", "latest.pth"]
    assert not os.path.exists(outs[1])
