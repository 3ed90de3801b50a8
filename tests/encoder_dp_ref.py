"""References for the speech encoder's fused optimiser and its data-parallel step (tests/test_encoder_dp_*.py).

`adam_l2_ref` restates torch.optim.Adam(weight_decay=wd) on one tensor, in the tensor's own dtype: fp64 is the reference, the
same code in fp32 on the CPU is the yardstick of the kernel's bound.  `mutant` names one deliberate mistake:
  "no_gscale"        the gradient is not scaled (a data-parallel step that forgets 1 / world)
  "adamw"            the decay is applied to the parameter after the moments (decoupled, AdamW style)
  "gscale_on_decay"  gscale multiplies the decay term too
`dp_steps` restates the data-parallel EncoderTrainer step: every rank's gradients from
encoder_conv_train_ref.full_grads on its own batch, their sum, 1 / world folded into adam_l2_ref; its mutants are
  "no_allreduce"     rank 0 steps on its own gradients
  "no_scale"         the summed gradients are not divided by the world size

Metrics.  The kernel is held per buffer at max|got - ref| / max|ref| (the project's metric).  A trajectory of several Adam
steps is not: Adam's first update of an element is lr * sign(gradient), so an element whose fp64 gradient lies inside the
fp32 rounding noise of the backward moves by lr in either direction, and among millions of parameters some always do; the
maximum over elements is then 2 lr whatever is computed, with or without a mistake.  `update_err` measures a trajectory by
||got - ref||_2 / ||ref - start||_2 over ALL trained parameters instead: the error against the length of the update itself.
A few sign flips weigh nothing in it, and a step taken on the wrong gradient weighs O(1).
"""
import ctypes

import torch

import encoder_conv_train_ref as R


def f32(x):
    """x rounded to fp32: the kernel receives its hyperparameters as floats, and the references are given what it receives
    (as tests/elementwise_replay.py does for s2i_adam_step)."""
    return float(ctypes.c_float(x).value)


ADAM = dict(lr=f32(1e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8))     # torch.optim.Adam's defaults, as the trainers use them
TEST_WD = f32(0.1)     # the tests' weight decay: decay and gradient terms are then of one size (test_encoder_dp_cpu.py)
TEST_GSCALE = 0.5
# s2i_elementwise.h grid_for: at most 8 192 blocks of 256 lanes, 4 floats per lane and trip; from this size on lane 0 takes
# a second trip of the grid-stride loop (and the last trip ends in the scalar tail)
SECOND_TRIP = 4 * 256 * 8192 + 5
KERNEL_SIZES = [1, 3, 4, 5, 1023, 1025, SECOND_TRIP]
KERNEL_STEPS = 3
KERNEL_MUTANTS = ("no_gscale", "adamw", "gscale_on_decay")

rel_err = R.rel_err

# Yardsticks: worst max|fp32 - fp64| / max|fp64| of adam_l2_ref on the CPU over KERNEL_SIZES, weight decay TEST_WD with
# gscale TEST_GSCALE and weight decay 0 with gscale 1 (kernel_yardstick; `python tests/encoder_dp_ref.py` prints them all).
# The bounds are twice the yardstick, the project's rule for a kernel whose operations run in another order.
KERNEL_YARDSTICK = {"p": 1.49e-7, "m": 1.86e-7, "v": 2.29e-7}
KERNEL_BOUNDS = {k: 2 * y for k, y in KERNEL_YARDSTICK.items()}
# Trajectories (measure_yardsticks, about 15 s; tests/test_encoder_dp_cpu.py runs it again): the restated trainers in fp32
# against fp64 on the CPU
#   traj_update / traj_running   encoder_conv_train_ref.trajectory, five steps at weight decay 1e-5: update_err of all
#                                parameters, worst rel_err of a running statistic
#   dp_update / dp_running       dp_steps, two ranks, two steps at TEST_WD
# The running statistics inherit the sign flips: one first-layer weight that moves the other way shifts a channel mean.
TRAJ_YARDSTICK = {"traj_update": 6.37e-3, "traj_running": 3.62e-2, "dp_update": 5.54e-4, "dp_running": 1.28e-2}
TRAJ_BOUNDS = {k: 2 * y for k, y in TRAJ_YARDSTICK.items()}


def adam_l2_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gscale=1.0, mutant=None):
    """One step -> (p, m, v), new tensors in p's dtype.  step is 1-based."""
    gg = g if mutant == "no_gscale" else g * gscale
    if mutant == "gscale_on_decay":
        gg = gg + (gscale * wd) * p
    elif mutant != "adamw":
        gg = gg + wd * p
    m = b1 * m + (1 - b1) * gg
    v = b2 * v + (1 - b2) * gg * gg
    bc1 = 1.0 - b1 ** step
    bc2s = (1.0 - b2 ** step) ** 0.5
    if mutant == "adamw":
        p = p - lr * wd * p
    p = p - (lr / bc1) * m / (v.sqrt() / bc2s + eps)
    return p, m, v


def kernel_case(n, seed=0):
    """p and KERNEL_STEPS gradients of n elements in fp64, every value representable in fp32.  An element's p and gradients
    share one random sign and keep away from zero (|p| in [0.05, 0.15), |g| in [2e-3, 1.2e-2)), so that no effective
    gradient gscale g + wd p is a small difference of large terms: Adam divides by its magnitude, and the update of an
    element whose gradient cancels to rounding noise is decided by that noise in any arithmetic."""
    gen = torch.Generator().manual_seed(6100 + seed + n % 9973)
    sign = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    r = lambda lo, width: (sign * (lo + width * torch.rand(n, generator=gen, dtype=torch.float32))).double()
    return r(0.05, 0.1), [r(2e-3, 1e-2) for _ in range(KERNEL_STEPS)]


def kernel_ref(n, dtype, wd, gscale, mutant=None, seed=0):
    """KERNEL_STEPS consecutive steps from zero moments in `dtype` -> (p, m, v)."""
    p, grads = kernel_case(n, seed)
    p = p.to(dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k, g in enumerate(grads):
        p, m, v = adam_l2_ref(p, g.to(dtype), m, v, wd=wd, step=k + 1, gscale=gscale, mutant=mutant, **ADAM)
    return p, m, v


def kernel_yardstick(sizes=KERNEL_SIZES):
    """Worst max|fp32 - fp64| / max|fp64| of the restatement per buffer over every case of the GPU test."""
    Y = {"p": 0.0, "m": 0.0, "v": 0.0}
    for n in sizes:
        for wd, gscale in ((TEST_WD, TEST_GSCALE), (0.0, 1.0)):
            a, b = kernel_ref(n, torch.float32, wd, gscale), kernel_ref(n, torch.float64, wd, gscale)
            for k, x, y in zip("pmv", a, b):
                Y[k] = max(Y[k], rel_err(x, y))
    return Y


# ---- trajectories ------------------------------------------------------------------------------------------------------------
def update_err(got, ref, start, names=None):
    """||got - ref||_2 / ||ref - start||_2 over the tensors `names` (default: all of start) of three dicts."""
    num = den = 0.0
    for n in (names if names is not None else start):
        r = ref[n].detach().double().cpu().reshape(-1)
        num += float(((got[n].detach().double().cpu().reshape(-1) - r) ** 2).sum())
        den += float(((r - start[n].detach().double().cpu().reshape(-1)) ** 2).sum())
    return (num / den) ** 0.5


def param_names(net):
    return [n for n, _ in net.named_parameters()]


def _set_layers(layers, tensors):
    for L in layers:
        if L["kind"] == "block":
            t = tensors[L["name"] + ".0.weight"]
            L["w"] = t[:, 0, :, 0].unsqueeze(2) if t.shape[1] == 1 and t.shape[3] == 1 else t[:, :, 0, :]
            L["gamma"], L["beta"] = tensors[L["name"] + ".1.weight"], tensors[L["name"] + ".1.bias"]
        elif L["kind"] == "bn0":
            L["gamma"], L["beta"] = tensors[L["name"] + ".weight"], tensors[L["name"] + ".bias"]


DP_STEPS = 2
DP_WORLD = 2


def dp_case(rank):
    """Rank `rank`'s fixed batch: encoder_conv_train_ref.trainer_case under another seed."""
    return R.trainer_case(seed=10 + rank)


def dp_steps(net, cases, steps, dtype, wd=TEST_WD, mutant=None, **loss_args):
    """`steps` data-parallel steps of len(cases) ranks from net's state, rank r always on cases[r] ->
    ([per step: loss dict per rank], final parameters by name, rank 0's running statistics by name)."""
    world = len(cases)
    sd = net.state_dict()
    order = param_names(net)
    tensors = {n: sd[n].detach().to(dtype).clone() for n in order}
    m = {n: torch.zeros_like(t) for n, t in tensors.items()}
    v = {n: torch.zeros_like(t) for n, t in tensors.items()}
    layers = [R.stack_layers(net, dtype) for _ in range(world)]          # each rank's own running statistics
    rnn_names = R.rnn_params(net, dtype)[0]
    losses = []
    for step in range(1, steps + 1):
        total, row = None, []
        for r, (mel, lens, image, label) in enumerate(cases):
            _set_layers(layers[r], tensors)
            res, grads, cache = R.full_grads(layers[r], (rnn_names, [tensors[n] for n in rnn_names]), mel.to(dtype), lens,
                                             image.to(dtype), label, **loss_args)
            for L, c in zip(layers[r], cache):
                if L["kind"] != "pool":
                    L["running"] = c["running"]
            row.append(res)
            if mutant == "no_allreduce" and r > 0:
                continue
            grads = {n: grads[n].reshape(tensors[n].shape) for n in order}
            total = grads if total is None else {n: total[n] + grads[n] for n in order}
        gscale = 1.0 if mutant == "no_scale" else 1.0 / world
        for n in order:
            tensors[n], m[n], v[n] = adam_l2_ref(tensors[n], total[n], m[n], v[n], wd=wd, step=step, gscale=gscale, **ADAM)
        losses.append(row)
    running = {}
    for L in layers[0]:
        if L["kind"] != "pool":
            pre = L["name"] + ("." if L["kind"] == "bn0" else ".1.")
            running[pre + "running_mean"], running[pre + "running_var"] = L["running"][0], L["running"][1]
    return losses, tensors, running


def measure_yardsticks():
    """The fp32 restatement against its fp64 run on the CPU for every bound of tests/test_encoder_dp_gpu.py."""
    Y = dict(("adam_" + k, e) for k, e in kernel_yardstick().items())
    net = R.stack_net(bidirectional=True, nhidden=512)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    names = list(start)
    # the single-process trainer: encoder_conv_train_ref.trajectory (weight decay 1e-5)
    mel, lens, image, label = R.trainer_case()
    _, s64 = R.trajectory(net, mel, lens, image, label, R.TRAINER_STEPS, torch.float64, **R.TRAINER_LOSS)
    _, s32 = R.trajectory(net, mel, lens, image, label, R.TRAINER_STEPS, torch.float32, **R.TRAINER_LOSS)
    Y["traj_update"] = update_err(s32, s64, start, names)
    Y["traj_running"] = max(rel_err(s32[n], s64[n]) for n in s64 if "running_" in n)
    # two ranks
    cases = [dp_case(r) for r in range(DP_WORLD)]
    l64, p64, r64 = dp_steps(net, cases, DP_STEPS, torch.float64, **R.TRAINER_LOSS)
    l32, p32, r32 = dp_steps(net, cases, DP_STEPS, torch.float32, **R.TRAINER_LOSS)
    Y["dp_update"] = update_err(p32, p64, start, names)
    Y["dp_running"] = max(rel_err(r32[n], r64[n]) for n in r64)
    Y["dp_loss"] = max(abs(float(a[0][k]) - float(b[0][k])) / abs(float(b[0]["loss"]))
                       for a, b in zip(l32, l64) for k in ("loss", "loss_jel", "loss_l1"))
    for mutant in ("no_allreduce", "no_scale"):
        _, pm, _ = dp_steps(net, cases, DP_STEPS, torch.float64, mutant=mutant, **R.TRAINER_LOSS)
        Y["_dp_mutant_" + mutant] = update_err(pm, p64, start, names)
    Y["_dp_losses"] = [[float(res["loss"]) for res in row] for row in l64]
    return Y


if __name__ == "__main__":
    for k, val in measure_yardsticks().items():
        print("%-24s %s" % (k, "%.3e" % val if isinstance(val, float) else val))
