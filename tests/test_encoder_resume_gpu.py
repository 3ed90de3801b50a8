"""Exact resume of speech-encoder training: HeadTrainer / EncoderTrainer.state_dict and load_state_dict, with torch.optim.Adam
and with the fused flat Adam, and `--state_every` / `--resume state.pth` of the CLIs, single process and two ranks.

The bound is equality (the steps are bitwise reproducible): stopping behind an epoch and resuming in a fresh trainer or process
must give the bits of the run that was never stopped.  The CLI comparisons carry their control: the stopped run's own epochs
print the straight run's lines."""
import copy
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import encoder_conv_train_ref as R
from speech_loader_ref import make_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech_to_image_translation_without_text_amd"
PROCESS_LIMIT = 300       # seconds for a started process


@pytest.fixture(scope="module")
def net():
    return R.stack_net(bidirectional=True, nhidden=512)


@pytest.fixture(scope="module")
def case(gpu):
    mel, lens, image, label = R.trainer_case()
    return mel.float().contiguous().to(gpu), lens, image.float(), label


def trainers():
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer, HeadTrainer
    return {"head": HeadTrainer, "encoder": EncoderTrainer}


def make(kind, net, gpu, fused):
    return trainers()[kind](copy.deepcopy(net).to(gpu), step_size=1, fused_adam=fused, **R.TRAINER_LOSS)


def steps(tr, case, n):
    for _ in range(n):
        tr.step(*case)
    tr.end_epoch()


def leaves(obj, prefix=""):
    """A nest of dicts, lists and tuples as {path: leaf}."""
    if isinstance(obj, dict):
        items = [(str(k), v) for k, v in obj.items()]
    elif isinstance(obj, (list, tuple)):
        items = [(str(k), v) for k, v in enumerate(obj)]
    else:
        return {prefix: obj}
    out = {}
    for k, v in items:
        out.update(leaves(v, prefix + "/" + k))
    return out


def first_difference(a, b):
    a, b = leaves(a), leaves(b)
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for k in a:
        same = torch.equal(a[k].cpu(), b[k].cpu()) if torch.is_tensor(a[k]) else a[k] == b[k]
        if not same:
            return k
    return None


@pytest.mark.parametrize("fused", [False, True], ids=["torch_adam", "fused_adam"])
@pytest.mark.parametrize("kind", ["head", "encoder"])
def test_trainer_resumes_bit_for_bit(gpu, tmp_path, net, case, kind, fused):
    straight = make(kind, net, gpu, fused)
    steps(straight, case, 2)
    steps(straight, case, 2)
    stopped = make(kind, net, gpu, fused)
    steps(stopped, case, 2)
    path = str(tmp_path / "state.pt")
    torch.save(stopped.state_dict(), path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert set(state) == {"state_dict", "epoch", "steps", "lr", "optimizer"}
    assert (state["epoch"], state["steps"]) == (1, 2) and state["lr"] == 1e-3 * 0.2
    n_trained = len(stopped._trained())
    assert sorted(state["optimizer"]["state"]) == list(range(n_trained)) and state["optimizer"]["param_groups"][0]["lr"] == state["lr"]
    assert all(float(e["step"]) == 2.0 and e["exp_avg"].shape == p.shape
               for e, p in zip(state["optimizer"]["state"].values(), stopped._trained()))
    resumed = make(kind, net, gpu, fused)
    where = [p.data_ptr() for p in resumed.model.parameters()]
    resumed.load_state_dict(state)
    assert [p.data_ptr() for p in resumed.model.parameters()] == where
    assert (resumed.epoch, resumed.steps, resumed.lr) == (1, 2, state["lr"])
    assert first_difference(resumed.state_dict(), state) is None, "load_state_dict then state_dict gives the state back"
    steps(resumed, case, 2)
    torch.cuda.synchronize()
    a, b = straight.state_dict(), resumed.state_dict()
    # what is compared: every parameter and BatchNorm buffer, exp_avg / exp_avg_sq / step of every trained parameter,
    # epoch, steps and the learning rate
    names = list(a["state_dict"])
    assert any(n.endswith("running_var") for n in names) and any(n.endswith("num_batches_tracked") for n in names)
    assert len(leaves(a["optimizer"]["state"])) == 3 * n_trained and float(a["optimizer"]["state"][0]["step"]) == 4.0
    assert (a["epoch"], a["steps"]) == (2, 4) and a["lr"] == pytest.approx(1e-3 * 0.2 * 0.2) and straight.lr == a["lr"]
    assert first_difference(a, b) is None, "the resumed trainer differs first at %s" % first_difference(a, b)
    # the comparison can fail: fresh moments, as a weights-only checkpoint resumes, end elsewhere
    afresh = make(kind, net, gpu, fused)
    afresh.model.load_state_dict(state["state_dict"])
    afresh._stale()
    afresh.skip_epochs(1)
    steps(afresh, case, 2)
    assert first_difference(a["state_dict"], afresh.state_dict()["state_dict"]) is not None


@pytest.mark.parametrize("kind", ["head", "encoder"])
def test_state_crosses_between_fused_and_torch_adam(gpu, net, case, kind):
    fused = make(kind, net, gpu, True)
    steps(fused, case, 2)
    sf = fused.state_dict()
    plain = make(kind, net, gpu, False)
    plain.load_state_dict(sf)
    # tensor by tensor what the torch-Adam trainer now holds
    held = plain.optimizer.state_dict()
    assert sorted(held["state"]) == sorted(sf["optimizer"]["state"])
    for k, ent in sf["optimizer"]["state"].items():
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(held["state"][k][name].cpu(), ent[name]), (k, name)
        assert held["state"][k]["exp_avg"].device.type == "cuda"
    assert plain.lr == fused.lr == held["param_groups"][0]["lr"] and plain.scheduler.last_epoch == 1
    assert first_difference(plain.state_dict()["optimizer"]["state"], sf["optimizer"]["state"]) is None
    assert first_difference(plain.state_dict()["state_dict"], sf["state_dict"]) is None
    # and back
    back = make(kind, net, gpu, True)
    back.load_state_dict(plain.state_dict())
    assert torch.equal(back.flat.m, fused.flat.m) and torch.equal(back.flat.v, fused.flat.v) and torch.equal(back.flat.p, fused.flat.p)
    assert int(back.flat.step_dev) == back.flat.step_count == 2 and back.lr == fused.lr
    # both go on from it; StepLR continues from the restored epoch
    for tr in (plain, back):
        steps(tr, case, 1)
        assert tr.lr == pytest.approx(1e-3 * 0.04) and tr.steps == 3
        assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    # the reference's resume_model: a stock Adam over the trained parameters reads the fused trainer's entry
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(p)) for p in fused._trained()], lr=1.0)
    opt.load_state_dict(copy.deepcopy(sf["optimizer"]))
    assert opt.param_groups[0]["lr"] == fused.lr and opt.param_groups[0]["weight_decay"] == 1e-5


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------
CLIPS = [1.0, 1.25, 0.3, 1.5]
COMMON = ["--dataset", "birds", "--batch_size", "2", "--seed", "3", "--bidirectional", "--jel_flag", "--lr_scheduler_step_size",
          "1", "--state_every", "1"]


def cli_tree(root):
    make_tree(root, "train", [CLIPS[k:] + CLIPS[:k] for k in range(4)] + [[1.1, 0.9]], seed=1)      # five items
    make_tree(root, "test", [CLIPS[k:] + CLIPS[:k] for k in range(2)], seed=2)


def result_lines(text, first=1):
    """The per-epoch lines and the JSON evaluation lines of epochs >= first."""
    out = []
    for ln in text.splitlines():
        if ln.startswith("epoch "):
            if int(ln.split(":")[0].split()[1]) >= first:
                out.append(ln)
        elif ln.startswith("{") and json.loads(ln)["epoch"] >= first:
            out.append(ln)
    return out


def checkpoints_equal(a, b):
    sa, sb = (torch.load(p, map_location="cpu", weights_only=True) for p in (a, b))
    assert sa["meta"] == sb["meta"]
    diff = first_difference(sa["state_dict"], sb["state_dict"])
    assert diff is None, "%s and %s differ first at %s" % (a, b, diff)


@pytest.mark.parametrize("mode", [[], ["--fused_adam", "--resident"]], ids=["torch_adam", "fused_resident"])
def test_cli_resume_prints_and_writes_what_the_straight_run_does(gpu, tmp_path, capsys, mode):
    from speech_to_image_translation_without_text_amd import train_encoder, train_state
    root = str(tmp_path)
    cli_tree(root)
    out_s, out_r = os.path.join(root, "straight"), os.path.join(root, "stopped")
    common = COMMON + ["--data_dir", root] + mode
    train_encoder.main(common + ["--output_dir", out_s, "--epoch", "4"])
    straight = capsys.readouterr().out
    train_encoder.main(common + ["--output_dir", out_r, "--epoch", "2"])
    leg1 = capsys.readouterr().out
    state = os.path.join(out_r, "state.pth")
    assert sorted(os.listdir(out_r)) == ["best.pth", "epoch_2.pth", "latest.pth", "state.pth"]
    st = torch.load(state, map_location="cpu", weights_only=True)
    assert set(st) == {"format", "meta", "state_dict", "optimizer", "rng"} and st["format"] == train_state.FORMAT
    # taken in front of the closing evaluation of the stopped run, which the straight run never made
    assert st["meta"] == {"epoch": 2, "best_accu": -1.0} and len(st["rng"]) == 1
    assert set(torch.load(os.path.join(out_r, "latest.pth"), map_location="cpu", weights_only=True)) == {"meta", "state_dict"}
    train_encoder.main(common + ["--output_dir", out_r, "--epoch", "4", "--resume", state])
    leg2 = capsys.readouterr().out
    lines = result_lines(straight)
    assert [ln.split(":")[0] for ln in lines] == ["epoch 1", "epoch 2", "epoch 3", "epoch 4", '{"epoch"']
    # the control: the stopped run's own two epochs are the straight run's
    assert [ln for ln in result_lines(leg1) if ln.startswith("epoch ")] == lines[:2]
    assert result_lines(leg2) == result_lines(straight, first=3) == lines[2:], (leg2, straight)
    assert json.loads(lines[-1])["best_accu"] == json.loads(lines[-1])["test_accu"]
    checkpoints_equal(os.path.join(out_s, "epoch_4.pth"), os.path.join(out_r, "epoch_4.pth"))
    ends = [torch.load(os.path.join(d, "state.pth"), map_location="cpu", weights_only=True) for d in (out_s, out_r)]
    assert ends[0]["meta"]["epoch"] == 4 and first_difference(ends[0], ends[1]) is None
    assert "state.pth.tmp" not in " ".join(os.listdir(out_r))
    if not mode:
        # the reference's resume_model: Adam over model.parameters() reads the `optimizer` field
        from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
        model = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True)
        model.load_state_dict(ends[1]["state_dict"])
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
        opt.load_state_dict(ends[1]["optimizer"])
        assert opt.param_groups[0]["lr"] == pytest.approx(1e-3 * 0.2 ** 4)
        assert float(opt.state[next(model.parameters())]["step"]) == 12.0        # three steps an epoch


def test_cli_without_state_every_writes_what_it_wrote(gpu, tmp_path, capsys):
    from speech_to_image_translation_without_text_amd import train_encoder
    root = str(tmp_path)
    cli_tree(root)
    out_dir = os.path.join(root, "out")
    assert COMMON[-2:] == ["--state_every", "1"]
    args = COMMON[:-2] + ["--data_dir", root, "--output_dir", out_dir, "--epoch", "1"]
    train_encoder.main(args)
    capsys.readouterr()
    assert sorted(os.listdir(out_dir)) == ["best.pth", "epoch_1.pth", "latest.pth"]
    ckpt = torch.load(os.path.join(out_dir, "latest.pth"), map_location="cpu", weights_only=True)
    assert set(ckpt) == {"meta", "state_dict"} and ckpt["meta"] == {"epoch": 1}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def two_ranks(root, out_dir, extra):
    """Two processes as torch.distributed.run would start them (gloo, both on GPU 0) -> rank 0's standard output."""
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        cmd = ([sys.executable, "-m", PKG + ".train_encoder", "--distributed", "--dist_backend", "gloo", "--data_dir", root,
                "--output_dir", out_dir if r == 0 else out_dir + "_rank1"] + COMMON + extra)
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
    assert not os.path.exists(out_dir + "_rank1"), "rank 1 writes nothing"
    return texts[0][0]


def test_cli_two_ranks_resume_with_their_own_draws(gpu, tmp_path, capsys):
    from speech_to_image_translation_without_text_amd import train_encoder
    root = str(tmp_path)
    cli_tree(root)
    out_s, out_r = os.path.join(root, "straight"), os.path.join(root, "stopped")
    straight = two_ranks(root, out_s, ["--epoch", "2"])
    two_ranks(root, out_r, ["--epoch", "1"])
    state = os.path.join(out_r, "state.pth")
    st = torch.load(state, map_location="cpu", weights_only=True)
    assert st["meta"] == {"epoch": 1, "best_accu": -1.0} and len(st["rng"]) == 2 and st["rng"][0] != st["rng"][1]
    leg2 = two_ranks(root, out_r, ["--epoch", "2", "--resume", state])
    lines = result_lines(straight, first=2)
    assert [ln.split(":")[0] for ln in lines] == ["epoch 2", '{"epoch"']
    assert result_lines(leg2) == lines, (leg2, straight)
    assert "rank 0 of 2: 4 steps" in straight and "rank 0 of 2: 4 steps" in leg2
    checkpoints_equal(os.path.join(out_s, "epoch_2.pth"), os.path.join(out_r, "epoch_2.pth"))
    # one process cannot continue what two ranks wrote
    with pytest.raises(ValueError, match=r"written by 2 rank\(s\) and cannot be resumed by 1\b"):
        train_encoder.main(COMMON + ["--data_dir", root, "--output_dir", os.path.join(root, "single"), "--epoch", "2", "--fused_adam",
                                     "--resume", state])
    capsys.readouterr()
