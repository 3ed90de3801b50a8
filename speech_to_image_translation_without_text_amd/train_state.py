"""Full training state for an exact resume: generator states, an atomic write, a safe load, and the conversion between
FlatNet's flat Adam moments and torch.optim.Adam's state_dict (host code; nothing here launches a kernel).

The GAN trainer (trainer.condGANTrainer.save_state / load_state, `Model/state.pt`) and the speech-encoder CLIs
(train_encoder_head.run, `<output_dir>/state.pth`) write their state through this module.  Every file is a dict of tensors,
numbers, strings, lists and tuples, so it loads under torch.load(weights_only=True), and carries `format`, the layout's
version.  What "exact" covers: a run stopped at an epoch boundary and resumed in a fresh process at the same world size ends
in the same bits as the run that was never stopped.
"""
import os
import random

import numpy as np
import torch

FORMAT = 1          # version of the layouts written through this module; `load` refuses any other


# ---- generator states ------------------------------------------------------------------------------------------------------
def capture_rng(device):
    """The state of Python's `random`, numpy's global generator, torch's CPU generator and, unless `device` is a CPU device,
    that device's torch generator -- as tensors and plain tuples."""
    device = torch.device(device)
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    state = {"python": random.getstate(),
             "numpy": (str(kind), torch.from_numpy(np.asarray(keys).astype(np.int64)), int(pos), int(has_gauss), float(cached)),
             "torch": torch.get_rng_state().clone()}
    if device.type != "cpu":
        state["device"] = torch.cuda.get_rng_state(device).clone()
    return state


def as_tuple(v):
    return tuple(as_tuple(x) for x in v) if isinstance(v, (list, tuple)) else v


def restore_rng(state, device):
    """Inverse of capture_rng.  A state captured without a device generator leaves the device's alone."""
    device = torch.device(device)
    random.setstate(as_tuple(state["python"]))
    kind, keys, pos, has_gauss, cached = state["numpy"]
    np.random.set_state((kind, keys.numpy().astype(np.uint32), int(pos), int(has_gauss), float(cached)))
    torch.set_rng_state(state["torch"].to(torch.uint8).cpu())
    if device.type != "cpu" and "device" in state:
        torch.cuda.set_rng_state(state["device"].to(torch.uint8).cpu(), device)


def gather(value, distributed):
    """`value` of every rank as a list indexed by rank, on every rank (all_gather_object); [value] in a single process."""
    if not distributed:
        return [value]
    out = [None] * torch.distributed.get_world_size()
    torch.distributed.all_gather_object(out, value)
    return out


def rank_entry(entries, rank, world, path="the state"):
    """Entry `rank` of a per-rank list written by `world` ranks; another world size is refused."""
    if len(entries) != world:
        raise ValueError("%s was written by %d rank(s) and cannot be resumed by %d: the per-rank generator states do not "
                         "map onto another world size" % (path, len(entries), world))
    return entries[rank]


# ---- files -------------------------------------------------------------------------------------------------------------------
def atomic_save(obj, path):
    """torch.save to a temporary name in `path`'s directory, flushed to the disk, then os.replace: `path` holds either its
    old contents or the whole new file, never a part of one.  If the write raises, the temporary file is removed."""
    path = os.fspath(path)
    tmp = "%s.tmp%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def check_format(obj, path="the state"):
    if not isinstance(obj, dict) or "format" not in obj:
        raise ValueError("%s carries no `format`: not a training state of this package" % path)
    if obj["format"] != FORMAT:
        raise ValueError("%s has format %r; this version reads format %d" % (path, obj["format"], FORMAT))
    return obj


def load(path):
    """The state on the CPU, read with weights_only=True; an unknown `format` is refused."""
    return check_format(torch.load(os.fspath(path), map_location="cpu", weights_only=True), os.fspath(path))


def to_cpu(obj):
    """Detached CPU copies of every tensor in a nest of dicts, lists and tuples."""
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_cpu(v) for v in obj)
    return obj


# ---- flat Adam moments <-> torch.optim.Adam.state_dict() ----------------------------------------------------------------------
def flat_to_adam_state(m, v, step, shapes, offsets, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay).state_dict() after `step` steps, for parameters of `shapes`
    whose moments lie in the flat buffers `m` and `v` at `offsets` (FlatNet's layout: every tensor padded to 4 elements).
    The param_groups entry is the installed torch's own; the state holds clones.  Zero steps give torch's empty state."""
    dummies = [torch.nn.Parameter(torch.empty(0)) for _ in shapes]
    sd = torch.optim.Adam(dummies, lr=float(lr), betas=tuple(betas), eps=float(eps),
                          weight_decay=float(weight_decay)).state_dict()
    state = {}
    if int(step) > 0:
        for k, (shape, o) in enumerate(zip(shapes, offsets)):
            n = int(np.prod(shape)) if len(shape) else 1
            state[k] = {"step": torch.tensor(float(step), dtype=torch.float32),
                        "exp_avg": m[o:o + n].detach().clone().reshape(tuple(shape)),
                        "exp_avg_sq": v[o:o + n].detach().clone().reshape(tuple(shape))}
    sd["state"] = state
    return sd


def adam_state_to_flat(sd, sizes, offsets, total, device=None):
    """Inverse of flat_to_adam_state -> (m, v, step): flat fp32 buffers of `total` elements (padding zero, as FlatNet keeps
    it) and the common step count.  Parameters at different step counts have no flat form and are refused."""
    m = torch.zeros(total, dtype=torch.float32, device=device)
    v = torch.zeros_like(m)
    state = sd["state"]
    if len(state) == 0:
        return m, v, 0
    if sorted(int(k) for k in state) != list(range(len(sizes))):
        raise ValueError("the optimizer state covers parameters %s, the trainer has %d"
                         % (sorted(int(k) for k in state), len(sizes)))
    steps = set()
    for k, (n, o) in enumerate(zip(sizes, offsets)):
        ent = state[k] if k in state else state[str(k)]
        if ent["exp_avg"].numel() != n:
            raise ValueError("optimizer state of parameter %d has %d elements, the trainer's has %d"
                             % (k, ent["exp_avg"].numel(), n))
        m[o:o + n].copy_(ent["exp_avg"].reshape(-1))
        v[o:o + n].copy_(ent["exp_avg_sq"].reshape(-1))
        steps.add(int(ent["step"]))
    if len(steps) != 1:
        raise ValueError("the parameters are at different step counts (%s): no flat form" % sorted(steps))
    return m, v, steps.pop()
