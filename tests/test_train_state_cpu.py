"""train_state.py on the CPU: generator round trip, the atomic write under a failing torch.save, the weights_only load, the
format check, the flat <-> torch.optim.Adam.state_dict() conversion on FlatNet's padded layout, and the new flag and keys."""
import copy
import os
import random

import numpy as np
import pytest
import torch

from speech_to_image_translation_without_text_amd import train_state as S

CPU = torch.device("cpu")


def draws():
    return ([random.random() for _ in range(3)] + [random.gauss(0, 1)], np.random.rand(3).tolist() + [float(np.random.randn())],
            torch.rand(3).tolist() + torch.randn(3).tolist())


def test_rng_round_trip_through_a_file(tmp_path):
    random.seed(5), np.random.seed(6), torch.manual_seed(7)
    random.gauss(0, 1), np.random.randn()            # an odd number of gaussians: both generators hold a cached one
    state = S.capture_rng(CPU)
    assert set(state) == {"python", "numpy", "torch"}, "a CPU device has no device generator to capture"
    first = draws()
    assert draws() != first
    S.restore_rng(state, CPU)
    assert draws() == first
    # and through the file, as the trainers carry it
    path = str(tmp_path / "s.pt")
    S.atomic_save({"format": S.FORMAT, "rng": [state]}, path)
    random.seed(99), np.random.seed(99), torch.manual_seed(99)
    S.restore_rng(S.rank_entry(S.load(path)["rng"], 0, 1, path), CPU)
    assert draws() == first


def test_atomic_save_keeps_the_old_file_when_the_write_fails(tmp_path, monkeypatch):
    path = str(tmp_path / "state.pt")
    S.atomic_save({"format": S.FORMAT, "x": torch.arange(5)}, path)
    before = open(path, "rb").read()
    assert os.listdir(str(tmp_path)) == ["state.pt"]
    seen = []

    def failing_save(obj, f, *a, **k):
        if isinstance(f, (str, os.PathLike)):
            seen.append(os.fspath(f))
            with open(f, "wb") as fh:
                fh.write(b"half a file")
        else:
            seen.append(f.name)
            f.write(b"half a file")
            f.flush()
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        S.atomic_save({"format": S.FORMAT, "x": torch.arange(7)}, path)
    monkeypatch.undo()
    assert seen and seen[0] != path and os.path.dirname(seen[0]) == str(tmp_path), "the write must go to a temporary name beside it"
    assert open(path, "rb").read() == before
    assert os.listdir(str(tmp_path)) == ["state.pt"]
    assert torch.equal(S.load(path)["x"], torch.arange(5))


def test_state_loads_under_weights_only(tmp_path):
    """What the trainers put into a state: generator states, an Adam state_dict, tensors, numbers, None."""
    p = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]
    opt = torch.optim.Adam(p, lr=1e-3, weight_decay=1e-5)
    for q in p:
        q.grad = torch.randn_like(q)
    opt.step()
    state = {"format": S.FORMAT, "rng": [S.capture_rng(CPU), S.capture_rng(CPU)], "optimizer": opt.state_dict(),
             "meta": {"epoch": 3, "best_accu": 12.5}, "python_only": [random.getstate()], "fixed_noise": None,
             "flats": [{"p": torch.randn(8), "sizes": [3, 5], "offsets": [0, 4], "lr": 2e-4, "step_count": 1}]}
    path = str(tmp_path / "s.pt")
    S.atomic_save(state, path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    got = S.load(path)
    assert set(got) == set(raw) == set(state) and got["meta"] == state["meta"]
    assert got["python_only"][0] == state["python_only"][0] and got["rng"][1]["python"] == state["rng"][1]["python"]
    assert torch.equal(got["optimizer"]["state"][1]["exp_avg"], opt.state_dict()["state"][1]["exp_avg"])
    assert torch.equal(got["rng"][0]["torch"], state["rng"][0]["torch"])


def test_unknown_format_and_other_world_size_are_refused(tmp_path):
    path = str(tmp_path / "s.pt")
    torch.save({"format": S.FORMAT + 41, "x": 1}, path)
    with pytest.raises(ValueError, match=r"format %d\b" % (S.FORMAT + 41)):
        S.load(path)
    torch.save({"x": 1}, path)
    with pytest.raises(ValueError, match="no `format`"):
        S.load(path)
    with pytest.raises(ValueError, match=r"written by 2 rank\(s\) and cannot be resumed by 1\b"):
        S.rank_entry(["a", "b"], 0, 1)
    assert S.rank_entry(["a", "b"], 1, 2) == "b"


RAGGED = [(1,), (3,), (2, 2), (5,)]          # 1, 3, 4 and 5 elements: FlatNet pads every tensor to 4


def flat_layout(shapes):
    sizes = [int(np.prod(s)) for s in shapes]
    offsets, off = [], 0
    for n in sizes:
        offsets.append(off)
        off += (n + 3) & ~3
    return sizes, offsets, off


def test_flat_moments_round_trip_through_an_adam_state_dict():
    sizes, offsets, total = flat_layout(RAGGED)
    assert (sizes, offsets, total) == ([1, 3, 4, 5], [0, 4, 8, 12], 20)
    g = torch.Generator().manual_seed(3)
    m, v = torch.zeros(total), torch.zeros(total)
    for n, o in zip(sizes, offsets):                  # padding stays zero, as the fused step leaves it
        m[o:o + n] = torch.randn(n, generator=g)
        v[o:o + n] = torch.rand(n, generator=g)
    sd = S.flat_to_adam_state(m, v, 7, RAGGED, offsets, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    # it is what a real torch.optim.Adam over parameters of those shapes writes and reads
    params = [torch.nn.Parameter(torch.zeros(s)) for s in RAGGED]
    opt = torch.optim.Adam(params, lr=1.0, weight_decay=0.5)
    assert set(sd) == set(opt.state_dict()) and set(sd["param_groups"][0]) == set(opt.state_dict()["param_groups"][0])
    opt.load_state_dict(copy.deepcopy(sd))            # torch keeps the `step` tensors it is handed and steps them in place
    group = opt.param_groups[0]
    assert (group["lr"], group["weight_decay"], tuple(group["betas"]), group["eps"]) == (2.5e-4, 1e-5, (0.9, 0.999), 1e-8)
    for k, (p, n, o) in enumerate(zip(params, sizes, offsets)):
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and float(st["step"]) == 7.0
        assert torch.equal(st["exp_avg"].reshape(-1), m[o:o + n]) and torch.equal(st["exp_avg_sq"].reshape(-1), v[o:o + n])
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()                                        # the loaded state steps
    assert float(opt.state[params[0]]["step"]) == 8.0
    # back to the flat form, from the dict itself and from torch's own state_dict of it
    opt2 = torch.optim.Adam([torch.nn.Parameter(torch.zeros(s)) for s in RAGGED])
    opt2.load_state_dict(sd)
    for source in (sd, opt2.state_dict()):
        m2, v2, step = S.adam_state_to_flat(source, sizes, offsets, total)
        assert step == 7 and torch.equal(m2, m) and torch.equal(v2, v)
    # no step taken yet: torch's empty state <-> zero moments
    empty = S.flat_to_adam_state(torch.zeros(total), torch.zeros(total), 0, RAGGED, offsets, lr=1e-3)
    assert empty["state"] == {} == torch.optim.Adam(params).state_dict()["state"]
    m0, v0, step0 = S.adam_state_to_flat(empty, sizes, offsets, total)
    assert step0 == 0 and not m0.any() and not v0.any()
    # what has no flat form is refused
    sd["state"][2]["step"] = torch.tensor(6.0)
    with pytest.raises(ValueError, match="different step counts"):
        S.adam_state_to_flat(sd, sizes, offsets, total)
    with pytest.raises(ValueError, match="parameter 1 has 3 elements"):
        S.adam_state_to_flat(S.flat_to_adam_state(m, v, 7, RAGGED, offsets, lr=1e-3), [1, 2, 4, 5], offsets, total)


def test_new_flag_and_config_keys_default_to_off():
    from speech_to_image_translation_without_text_amd import train_encoder, train_encoder_head
    from speech_to_image_translation_without_text_amd.miscc.config import cfg, cfg_from_dict, cfg_reset
    for mod, argv in ((train_encoder_head, ["--model", "m.pt"]), (train_encoder, [])):
        assert mod.get_parser().parse_args(argv).state_every == 0
        args = mod.get_parser().parse_args(argv + ["--state_every", "3"])
        assert args.state_every == 3
        train_encoder_head.check_args(args)
        with pytest.raises(SystemExit):
            train_encoder_head.check_args(mod.get_parser().parse_args(argv + ["--state_every", "-1"]))
    cfg_reset()
    assert cfg.TRAIN.STATE == "" and cfg.TRAIN.STATE_EVERY == 0
    cfg_from_dict({"TRAIN": {"STATE": "Model/state.pt", "STATE_EVERY": 5}})     # reachable from a YAML file
    assert cfg.TRAIN.STATE == "Model/state.pt" and cfg.TRAIN.STATE_EVERY == 5
    cfg_reset()
    assert cfg.TRAIN.STATE == "" and cfg.TRAIN.STATE_EVERY == 0
