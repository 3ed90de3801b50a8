"""Exact resume of GAN training from Model/state.pt (trainer.FlatNet.state_dict / load_state_dict, condGANTrainer.save_state /
load_state, TRAIN.STATE and TRAIN.STATE_EVERY).

The bound is equality: the step is bitwise reproducible, so a run stopped behind an epoch and resumed in a fresh trainer, under
other seeds, must end in the same bits as the run that was never stopped.  Every comparison has its control -- the straight run
twice -- asserted, so that a difference between two straight runs (a determinism finding about a kernel, not about the resume)
cannot be taken for a resume fault.  small3 widths, batch 8, the two-batch in-memory loader of
test_model_gpu.py::test_training_loop_checkpoint_and_resume."""
import os
import random
import shutil
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

from helpers import CASES, configure

pytestmark = pytest.mark.gpu

CASE = dict(CASES['small3'], B=8)
PROCESS_LIMIT = 300       # seconds for the spawned ranks


def make_loader(seed=2):
    g = torch.Generator().manual_seed(seed)

    def sample():
        imgs = [torch.rand(8, 3, 64 << i, 64 << i, generator=g) * 2 - 1 for i in range(3)]
        wrong = [torch.rand(8, 3, 64 << i, 64 << i, generator=g) * 2 - 1 for i in range(3)]
        return imgs, wrong, torch.randn(8, CASE['t'], generator=g), ['k'] * 8, torch.arange(8) % 3
    return [sample(), sample()]


@pytest.fixture(scope="module")
def loader():
    return make_loader()


@pytest.fixture
def clean_cfg():
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd.miscc.config import cfg_reset
    old = ops.ACT_BF16
    yield
    ops.ACT_BF16 = old
    cfg_reset()


# ---- FlatNet ---------------------------------------------------------------------------------------------------------------------
def two_layers(gpu):
    torch.manual_seed(4)
    return nn.Sequential(nn.Linear(3, 5), nn.Linear(5, 3)).to(gpu)       # 15, 5, 15 and 3 elements: none a multiple of 4


def fixed_grads(flat, k):
    g = torch.Generator().manual_seed(50 + k)
    for p in flat.params:
        p.grad.copy_(torch.randn(p.shape, generator=g))


def adam_ema_steps(flat, ks):
    for k in ks:
        flat.zero_grad()
        fixed_grads(flat, k)
        flat.adam()
        flat.ema(0.9)


def addresses(flat):
    return ([t.data_ptr() for t in (flat.p, flat.g, flat.m, flat.v, flat.avg)] + [p.data_ptr() for p in flat.params]
            + [p.grad.data_ptr() for p in flat.params] + [a.data_ptr() for a in flat.avg_params()])


def test_flatnet_state_round_trip_in_place(gpu):
    from speech_to_image_translation_without_text_amd import trainer as T
    a = T.FlatNet(two_layers(gpu), 1e-2, with_ema=True)
    assert a.sizes == [15, 5, 15, 3] and a.total == 16 + 8 + 16 + 4
    adam_ema_steps(a, range(3))
    sd = a.state_dict()
    assert set(sd) == {"p", "m", "v", "avg", "step_count", "lr", "sizes", "offsets"} and sd["step_count"] == 3
    assert sd["p"].data_ptr() != a.p.data_ptr() and torch.equal(sd["p"], a.p), "state_dict returns clones"
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()}      # as a file hands it back
    b = T.FlatNet(two_layers(gpu), 5e-1, with_ema=True)
    with torch.no_grad():
        b.p.add_(1.0)                                # other weights, moments, step count and learning rate than the state's
    adam_ema_steps(b, [7])
    avg_views = b.avg_params()
    before = addresses(b)
    b.load_state_dict(sd)
    assert addresses(b) == before, "load_state_dict must write in place: recorded plans and avg_param_G hold the addresses"
    assert b.step_count == 3 and int(b.step_dev) == 3 and b.lr == 1e-2
    assert all(torch.equal(x, y) for x, y in zip(avg_views, a.avg_params())), "views taken before the load see the state"
    assert all(torch.equal(p, q) for p, q in zip(b.net.parameters(), a.net.parameters()))
    adam_ema_steps(a, [3, 4])
    adam_ema_steps(b, [3, 4])
    torch.cuda.synchronize()
    for name in ("p", "m", "v", "avg", "step_dev"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert int(a.step_dev) == 5 == b.step_count
    fresh = T.FlatNet(two_layers(gpu), 1e-2, with_ema=True)
    adam_ema_steps(fresh, [3, 4])
    assert not torch.equal(fresh.p, a.p), "the two steps must depend on the state"
    # refused: another layout, and a state without the EMA copy this network keeps
    torch.manual_seed(4)
    other = T.FlatNet(nn.Sequential(nn.Linear(3, 5), nn.Linear(5, 2)).to(gpu), 1e-2, with_ema=True)
    kept = other.p.clone()
    with pytest.raises(ValueError, match=r"tensor 2 \(1\.weight\) has 10 elements here and 15 in the state"):
        other.load_state_dict(sd)
    assert torch.equal(other.p, kept) and other.step_count == 0
    with pytest.raises(ValueError, match="EMA"):
        T.FlatNet(two_layers(gpu), 1e-2).load_state_dict(sd)


# ---- condGANTrainer -------------------------------------------------------------------------------------------------------------
def final_state(tr):
    """Everything the runs are compared on, on the CPU."""
    torch.cuda.synchronize()
    out = {}
    for name, f in [("G", tr.flatG)] + [("D%d" % i, f) for i, f in enumerate(tr.flatsD)]:
        for k in ("p", "m", "v", "step_dev"):
            out["%s.%s" % (name, k)] = getattr(f, k).detach().cpu().clone()
        for k, b in f.net.named_buffers():
            out["%s.buffer.%s" % (name, k)] = b.detach().cpu().clone()
    out["G.avg"] = tr.flatG.avg.detach().cpu().clone()
    return out


def run_gan(out_dir, loader, seed, state="", epochs=4, state_every=2, copy_after=None):
    """One condGANTrainer.train() -> (trainer, final state).  copy_after: (epoch, path) copies Model/state.pt as written
    behind that epoch."""
    from speech_to_image_translation_without_text_amd import trainer as T
    cfg = configure(CASE)
    cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.STATE_EVERY, cfg.TRAIN.STATE = epochs, state_every, state
    cfg.TRAIN.SNAPSHOT_INTERVAL, cfg.TRAIN.VIS_COUNT = 6, 8
    torch.manual_seed(seed)
    random.seed(seed)
    tr = T.condGANTrainer(out_dir, loader, 256, False)
    if copy_after is not None:
        inner = tr.save_state

        def save_state(path, epoch, count):
            inner(path, epoch, count)
            if epoch == copy_after[0]:
                shutil.copyfile(path, copy_after[1])
        tr.save_state = save_state
    tr.train()
    return tr, final_state(tr)


def first_difference(a, b):
    assert list(a) == list(b)
    for k in a:
        if not torch.equal(a[k], b[k]):
            return k
    return None


def files_equal(dir_a, dir_b, names):
    for name in names:
        pa, pb = os.path.join(dir_a, name), os.path.join(dir_b, name)
        if name.endswith(".png"):
            assert open(pa, "rb").read() == open(pb, "rb").read(), name
        else:
            sa, sb = (torch.load(p, map_location="cpu", weights_only=True) for p in (pa, pb))
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), name


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_resumed_run_ends_in_the_bits_of_the_straight_run(gpu, tmp_path, loader, clean_cfg, bf16):
    from speech_to_image_translation_without_text_amd import ops, train_state
    ops.ACT_BF16 = bool(bf16)
    dirs = {k: str(tmp_path / k) for k in ("a", "a2", "b")}
    copy = str(tmp_path / "state_after_2.pt")
    _, a = run_gan(dirs["a"], loader, 0, copy_after=(2, copy))
    _, a2 = run_gan(dirs["a2"], loader, 0)
    _, b = run_gan(dirs["b"], loader, 123, state=copy)
    models = ["netG_8.pth"] + ["netD%d.pth" % i for i in range(3)]
    pngs = ["count_%09d_fake_samples%d.png" % (6, i) for i in range(3)]
    # the control: two straight runs agree, so the comparison below can pass
    assert first_difference(a, a2) is None, "two straight runs differ first at %s: a determinism finding" % first_difference(a, a2)
    files_equal(os.path.join(dirs["a"], "Model"), os.path.join(dirs["a2"], "Model"), models)
    files_equal(os.path.join(dirs["a"], "Image"), os.path.join(dirs["a2"], "Image"), pngs)
    # the state taken behind epoch 2
    st = train_state.load(copy)
    assert (st["epoch"], st["count"], st["world"], st["batch_size"]) == (2, 4, 1, 8)
    assert (st["act_bf16"], st["math_planes"]) == (bool(bf16), ops.MATH_PLANES) and len(st["rng"]) == 1
    assert [int(f["step_count"]) for f in st["flats"]] == [4] * 4 and "avg" in st["flats"][0] and "avg" not in st["flats"][1]
    assert int(a["G.step_dev"]) == 8 and not torch.equal(st["flats"][0]["p"], a["G.p"]), "epochs 3 and 4 trained"
    # the resumed run
    assert first_difference(a, b) is None, "the resumed run differs first at %s" % first_difference(a, b)
    files_equal(os.path.join(dirs["a"], "Model"), os.path.join(dirs["b"], "Model"), models)
    files_equal(os.path.join(dirs["a"], "Image"), os.path.join(dirs["b"], "Image"), pngs)
    assert not os.path.exists(os.path.join(dirs["b"], "Model", "netG_4.pth")), "the resumed run began behind epoch 2"
    # and it would go on alike: the closing states agree, generator states included
    enda, endb = (train_state.load(os.path.join(dirs[k], "Model", "state.pt")) for k in ("a", "b"))
    assert (endb["epoch"], endb["count"]) == (4, 8)
    ra, rb = enda["rng"][0], endb["rng"][0]
    assert ra["python"] == rb["python"] and all(torch.equal(ra[k], rb[k]) for k in ("torch", "device"))
    assert torch.equal(ra["numpy"][1], rb["numpy"][1]) and ra["numpy"][2:] == rb["numpy"][2:]
    assert torch.equal(enda["fixed_noise"], endb["fixed_noise"]) and torch.equal(enda["fixed_eps"], endb["fixed_eps"])
    assert sorted(os.listdir(os.path.join(dirs["b"], "Model"))) == sorted(["netG_6.pth", "netG_8.pth", "state.pt"]
                                                                            + ["netD%d.pth" % i for i in range(3)])
    # another math mode, and another batch size, are refused by name
    from speech_to_image_translation_without_text_amd import trainer as T
    ops.ACT_BF16 = not bf16
    tr = T.condGANTrainer(str(tmp_path / "c"), loader, 256, False)
    tr.build()
    with pytest.raises(ValueError, match="ACT_BF16, MATH_PLANES"):
        tr.load_state(copy)
    ops.ACT_BF16 = bool(bf16)
    tr.batch_size = 4
    with pytest.raises(ValueError, match="batch size 8; this run has 4"):
        tr.load_state(copy)


def test_defaults_write_what_they_wrote(gpu, tmp_path, loader, clean_cfg):
    from speech_to_image_translation_without_text_amd.miscc.config import cfg
    from speech_to_image_translation_without_text_amd import trainer as T
    configure(CASE)
    assert cfg.TRAIN.STATE == "" and cfg.TRAIN.STATE_EVERY == 0
    cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.SNAPSHOT_INTERVAL = 2, 1000
    torch.manual_seed(0)
    tr = T.condGANTrainer(str(tmp_path / "run"), loader, 256, False)
    tr.train()
    assert sorted(os.listdir(str(tmp_path / "run" / "Model"))) == ["netD0.pth", "netD1.pth", "netD2.pth", "netG_4.pth"]
    assert sorted(os.listdir(str(tmp_path / "run"))) == ["Image", "Log", "Model"]
    assert os.listdir(str(tmp_path / "run" / "Image")) == [] and os.listdir(str(tmp_path / "run" / "Log")) == []


# ---- two data-parallel ranks ---------------------------------------------------------------------------------------------------
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


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_resume_gpu as me
    from speech_to_image_translation_without_text_amd import trainer as T
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        loader = me.make_loader(seed=2 + rank)                     # different data on every rank
        copy = os.path.join(out_dir, "state_after_1.pt")

        def run(name, seed, state, epochs=2):
            cfg = me.configure(me.CASE)
            cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.STATE_EVERY, cfg.TRAIN.STATE = epochs, 1, state
            cfg.TRAIN.SNAPSHOT_INTERVAL, cfg.TRAIN.VIS_COUNT = 1000, 0
            torch.manual_seed(seed)
            random.seed(seed)
            tr = T.condGANTrainer(os.path.join(out_dir, name), loader, 256, False, local_rank=0, distributed=True)
            tr.d_overlap_min = 0
            if not state:
                inner = tr.save_state

                def save_state(path, epoch, count):
                    inner(path, epoch, count)
                    if epoch == 1 and rank == 0:
                        shutil.copyfile(path, copy)
                tr.save_state = save_state
            tr.train()
            torch.distributed.barrier()
            return me.final_state(tr)
        straight = run("straight", rank, "")
        again = run("again", rank, "")
        resumed = run("resumed", 100 + rank, copy)                # the second epoch alone
        assert me.first_difference(straight, again) is None, "two straight data-parallel runs differ: a determinism finding"
        flat = [k for k in straight if ".buffer." not in k]       # the other ranks' BatchNorm buffers are rank 0's on resume
        keys = list(straight) if rank == 0 else flat
        diff = me.first_difference({k: straight[k] for k in keys}, {k: resumed[k] for k in keys})
        assert diff is None, "rank %d: the resumed run differs first at %s" % (rank, diff)
        assert int(straight["G.step_dev"]) == 4
        with open(os.path.join(out_dir, "ok%d" % rank), "w") as fh:
            fh.write("ok")
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks_resume_and_another_world_size_is_refused(gpu, tmp_path, loader, clean_cfg):
    from speech_to_image_translation_without_text_amd import train_state, trainer as T
    spawn(_dp_worker, (2, _free_port(), str(tmp_path)), 2)
    assert all((tmp_path / ("ok%d" % r)).exists() for r in range(2))
    copy = str(tmp_path / "state_after_1.pt")
    st = train_state.load(copy)
    assert (st["epoch"], st["count"], st["world"]) == (1, 2, 2) and len(st["rng"]) == 2
    assert st["rng"][0]["python"] != st["rng"][1]["python"], "every rank's own generator states"
    assert sorted(os.listdir(str(tmp_path / "resumed" / "Model"))) == ["netD0.pth", "netD1.pth", "netD2.pth", "netG_4.pth", "state.pt"]
    configure(CASE)
    tr = T.condGANTrainer(str(tmp_path / "single"), loader, 256, False)
    tr.build()
    kept = tr.flatG.p.clone()
    with pytest.raises(ValueError, match=r"written by 2 rank\(s\) and cannot be resumed by 1\b"):
        tr.load_state(copy)
    assert torch.equal(tr.flatG.p, kept), "a refused state must leave the trainer as it was"
