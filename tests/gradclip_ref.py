"""References for gradient-norm clipping, accumulation and the non-finite guard of the fused optimiser
(tests/test_gradclip_*.py; kernels: s2i_grad_sumsq, s2i_grad_clip_scale, s2i_adam_step_dev / s2i_adam_l2_step_dev).

`clipped_step` restates one guarded optimiser step over a list of tensors in the tensors' own dtype: the sum of squares and
everything up to `scale` in fp64 as the kernels compute it, torch.nn.utils.clip_grad_norm_'s rule on the norm of gscale * g,
then encoder_dp_ref.adam_l2_ref with `scale` as its gscale; a gradient whose sum of squares is not finite changes nothing.
In fp64 it is the reference; in fp32 on the CPU (torch's IEEE single, elementwise as numpy's) it is the yardstick of the
GPU bound.  `mutant` names one deliberate mistake:
  "norm_before_gscale"   the norm is taken of g, not of gscale * g
  "per_tensor"           every tensor is clipped by its own norm
  "no_eps"               coef = max_norm / norm, without the 1e-6
  "coef_on_decay"        coef multiplies the weight-decay term too
  "skip_advances_step"   a skipped step still counts as an Adam step
  "skip_decays"          a skipped step still applies weight decay (an Adam step on a zero gradient)
and accum_gscale's "accum_full_n" divides an incomplete group of k micro-batches by N.

The norm's bound is derived, not measured: the squares of fp32 values are exact in fp64, the terms are non-negative, so a
sum of n of them in ANY order carries a relative error of at most (n - 1) u, u = 2**-53; sqrt, the multiplication by |gscale|
and the rounding of the reference itself add at most one u each: |norm - ref| <= (n + 4) u ref (norm_bound).
"""
import math

import torch

import encoder_conv_train_ref as R
import encoder_dp_ref as D
from encoder_dp_ref import ADAM, TEST_WD, adam_l2_ref, f32, kernel_case

CHUNK = 4096                      # ops.GRAD_CHUNK (tests/test_gradclip_cpu.py holds the two together)
BIG = 4 * 256 * 8192 + 5          # encoder_dp_ref.SECOND_TRIP: the Adam kernel's second grid-stride trip and scalar tail
SINGLE_SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, BIG]
MULTI = [1, 3, 5, 4097, 7]
SMALL_LAYOUTS = [[n] for n in SINGLE_SIZES[:-1]] + [MULTI]
UPDATE_LAYOUTS = SMALL_LAYOUTS + [[BIG]]           # the cases of the update-against-fp64 test and of the yardstick
GSCALE = 0.5
STEPS = D.KERNEL_STEPS
U = 2.0 ** -53
MUTANTS = ("norm_before_gscale", "per_tensor", "no_eps", "coef_on_decay", "skip_advances_step", "skip_decays")

# Yardstick of the clipped update: worst max|fp32 - fp64| / max|fp64| per buffer of three clipped steps (coef < 1 at every
# one) over UPDATE_LAYOUTS, weight decay TEST_WD and 0 (clip_yardstick; tests/test_gradclip_cpu.py re-measures it;
# `python tests/gradclip_ref.py` prints it).  The bound is twice the yardstick.
CLIP_YARDSTICK = {"p": 1.53e-7, "m": 1.81e-7, "v": 2.60e-7}
CLIP_BOUNDS = {k: 2 * y for k, y in CLIP_YARDSTICK.items()}


def layout(sizes):
    """trainer.FlatNet's layout -> (offsets, total): every tensor at the next multiple of 4 elements."""
    offsets, off = [], 0
    for n in sizes:
        offsets.append(off)
        off += (n + 3) & ~3
    return offsets, off


_REAL = {}


def real_sizes(which):
    """The sizes of the real FlatNet layouts: "head" (RNN.*, 8 tensors, 6.30 M elements) and "encoder" (every parameter of
    the bidirectional CNNRNN, 11.67 M)."""
    if not _REAL:
        net = R.stack_net(bidirectional=True, nhidden=1024)
        _REAL["head"] = [p.numel() for p in net.RNN.parameters()]
        _REAL["encoder"] = [p.numel() for p in net.parameters()]
    return _REAL[which]


def norm_bound(n):
    return (n + 4) * U


def flat_case(sizes, kind="normal", seed=0):
    """A flat fp32 gradient buffer of the layout, padding elements NaN.  kind: "normal" (|g| in [2e-3, 1.2e-2)), "tiny"
    (every element 1e-25: the squares underflow fp32), "huge" (1e+25: they overflow it), "mixed" (both, alternating),
    "zero"."""
    offsets, total = layout(sizes)
    flat = torch.full((total,), float("nan"), dtype=torch.float32)
    gen = torch.Generator().manual_seed(7300 + seed + sum(sizes) % 9973)
    for o, n in zip(offsets, sizes):
        if kind == "normal":
            sign = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
            t = sign * (2e-3 + 1e-2 * torch.rand(n, generator=gen, dtype=torch.float32))
        elif kind == "zero":
            t = torch.zeros(n)
        else:
            t = torch.full((n,), 1e-25 if kind == "tiny" else 1e25, dtype=torch.float32)
            if kind == "mixed":
                t[1::2] = 1e-25
        flat[o:o + n] = t
    return flat


def exact_sumsq(x):
    """The exactly rounded sum of the squares of an fp32 tensor: the squares are exact in fp64, math.fsum rounds once."""
    d = x.double()
    return math.fsum((d * d).tolist())


def exact_norms(flat, sizes, gscale=1.0):
    """-> (norm of the whole layout, per-tensor norms) from exactly rounded sums, times |gscale|."""
    offsets, _ = layout(sizes)
    sums = [exact_sumsq(flat[o:o + n]) for o, n in zip(offsets, sizes)]
    return math.sqrt(math.fsum(sums)) * abs(gscale), [math.sqrt(s) * abs(gscale) for s in sums]


def clip_coef(norm, max_norm, mutant=None):
    """torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1); no clipping for max_norm <= 0."""
    if not max_norm > 0:
        return 1.0
    return min(1.0, max_norm / (norm + (0.0 if mutant == "no_eps" else 1e-6)))


def clip_scale(sumsq, gscale, max_norm, mutant=None):
    """-> (norm, coef, scale as the fp32 value the kernel stores) from a sum of squares."""
    norm = math.sqrt(sumsq) * (1.0 if mutant == "norm_before_gscale" else abs(gscale))
    coef = clip_coef(norm, max_norm, mutant)
    return norm, coef, f32(gscale * coef)


def accum_gscale(world, pending, accum, mutant=None):
    """The factor of a group of `pending` micro-batches out of `accum`: 1 / (world * pending)."""
    return 1.0 / (world * (accum if mutant == "accum_full_n" else pending))


def clipped_step(ps, gs, ms, vs, step, gscale, max_norm, wd, mutant=None):
    """One guarded step over lists of tensors -> (ps, ms, vs, step, info).  `step` is the number of applied updates before
    the call and after it."""
    sums = [float((g.double() * g.double()).sum()) for g in gs]
    total = math.fsum(sums)
    if not math.isfinite(total):
        info = {"apply": 0, "norm": math.sqrt(total) * abs(gscale) if total == total else total}
        if mutant == "skip_advances_step":
            step += 1
        if mutant == "skip_decays":
            out = [adam_l2_ref(p, torch.zeros_like(p), m, v, wd=wd, step=max(step, 1), gscale=0.0, **ADAM)
                   for p, m, v in zip(ps, ms, vs)]
            ps, ms, vs = [list(t) for t in zip(*out)]
        return ps, ms, vs, step, info
    norm, coef, scale = clip_scale(total, gscale, max_norm, mutant)
    step += 1
    out = []
    for p, g, m, v, s in zip(ps, gs, ms, vs, sums):
        sc, c = scale, coef
        if mutant == "per_tensor":
            _, c, sc = clip_scale(s, gscale, max_norm)
        out.append(adam_l2_ref(p, g, m, v, wd=wd * c if mutant == "coef_on_decay" else wd, step=step, gscale=sc, **ADAM))
    ps, ms, vs = [list(t) for t in zip(*out)]
    return ps, ms, vs, step, {"apply": 1, "norm": norm, "coef": coef, "scale": scale}


# ---- the update cases --------------------------------------------------------------------------------------------------------
def update_case(sizes):
    """Per tensor encoder_dp_ref.kernel_case: p and STEPS gradients in fp64, fp32-representable -> (ps, [gs per step])."""
    cases = [kernel_case(n, seed=k) for k, n in enumerate(sizes)]
    return [c[0] for c in cases], [[c[1][s] for c in cases] for s in range(STEPS)]


def case_max_norm(sizes, gscale=GSCALE):
    """Half the smallest norm of gscale * g over the case's steps: coef < 1 at every step."""
    _, grads = update_case(sizes)
    return 0.5 * min(math.sqrt(math.fsum(float((g * g).sum()) for g in gs)) * abs(gscale) for gs in grads)


def update_ref(sizes, dtype, wd, gscale=GSCALE, max_norm=None, mutant=None, grads=None, step0=0):
    """STEPS guarded steps from zero moments in `dtype` -> (ps, ms, vs, step, [info per step]).  `grads` replaces the
    case's gradients (lists of fp64 tensors per step; a non-finite one makes a skipped step)."""
    ps, case_grads = update_case(sizes)
    grads = case_grads if grads is None else grads
    max_norm = case_max_norm(sizes, gscale) if max_norm is None else max_norm
    ps = [p.to(dtype) for p in ps]
    ms, vs, step, infos = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], step0, []
    for gs in grads:
        ps, ms, vs, step, info = clipped_step(ps, [g.to(dtype) for g in gs], ms, vs, step, gscale, max_norm, wd, mutant)
        infos.append(info)
    return ps, ms, vs, step, infos


def flatten(tensors, sizes, fill=0.0):
    """A list of per-tensor values in the layout's flat buffer (padding `fill`)."""
    offsets, total = layout(sizes)
    flat = torch.full((total,), fill, dtype=tensors[0].dtype)
    for t, o, n in zip(tensors, offsets, sizes):
        flat[o:o + n] = t.reshape(-1)
    return flat


def buffer_errs(got, ref, sizes):
    """max|got - ref| / max|ref| per buffer (encoder_dp_ref's kernel metric) over the layout's elements: got and ref are
    (p, m, v), each a flat buffer or a list of tensors."""
    offsets, _ = layout(sizes)
    out = {}
    for k, a, b in zip("pmv", got, ref):
        a = a if isinstance(a, (list, tuple)) else [a[o:o + n] for o, n in zip(offsets, sizes)]
        b = b if isinstance(b, (list, tuple)) else [b[o:o + n] for o, n in zip(offsets, sizes)]
        num = max(float((x.detach().double().cpu().reshape(-1) - y.detach().double().cpu().reshape(-1)).abs().max())
                  for x, y in zip(a, b))
        den = max(float(y.detach().double().abs().max()) for y in b)
        out[k] = num / den
    return out


def clip_yardstick(layouts=UPDATE_LAYOUTS):
    Y = {"p": 0.0, "m": 0.0, "v": 0.0}
    for sizes in layouts:
        for wd in (TEST_WD, 0.0):
            a, b = update_ref(sizes, torch.float32, wd), update_ref(sizes, torch.float64, wd)
            assert all(i["coef"] < 1.0 for i in b[4])
            for k, e in buffer_errs(a[:3], b[:3], sizes).items():
                Y[k] = max(Y[k], e)
    return Y


def measure_yardsticks():
    return clip_yardstick()


def ulp32(x):
    """The spacing of fp32 at |x|."""
    x = abs(float(x))
    if x == 0.0:
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


# ---- the trainers ------------------------------------------------------------------------------------------------------------
def clipped_trajectory(net, mel, lens, image, label, steps, dtype, max_norm, lr=1e-3, weight_decay=1e-5, **loss_args):
    """encoder_conv_train_ref.trajectory with torch.nn.utils.clip_grad_norm_(parameters, max_norm) in front of every
    optimiser step -> ([loss dict per step], final state, [gradient norm per step])."""
    layers = R.stack_layers(net, dtype)
    names, params = R.rnn_params(net, dtype)
    leaves = {}
    for L in layers:
        if L["kind"] == "block":
            leaves[L["name"] + ".0.weight"] = ("w", L)
            leaves[L["name"] + ".1.weight"], leaves[L["name"] + ".1.bias"] = ("gamma", L), ("beta", L)
        elif L["kind"] == "bn0":
            leaves[L["name"] + ".weight"], leaves[L["name"] + ".bias"] = ("gamma", L), ("beta", L)
    tensors = {}
    for n, (key, L) in leaves.items():
        tensors[n] = (L[key].reshape(L["wshape"]) if key == "w" else L[key]).clone().requires_grad_(True)
    for n, p in zip(names, params):
        tensors[n] = p.clone().requires_grad_(True)
    order = [n for n, _ in net.named_parameters()]
    opt = torch.optim.Adam([tensors[n] for n in order], lr=lr, weight_decay=weight_decay)
    losses, norms = [], []
    mel, image = mel.to(dtype), image.to(dtype)
    for _ in range(steps):
        D._set_layers(layers, {n: t.detach() for n, t in tensors.items()})
        res, grads, cache = R.full_grads(layers, (names, [tensors[n].detach() for n in names]), mel, lens, image, label,
                                         **loss_args)
        for L, c in zip(layers, cache):
            if L["kind"] != "pool":
                L["running"] = c["running"]
        opt.zero_grad()
        for n in order:
            tensors[n].grad = grads[n].reshape(tensors[n].shape).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([tensors[n] for n in order], max_norm)))
        opt.step()
        losses.append(res)
    state = {n: t.detach().clone() for n, t in tensors.items()}
    for L in layers:
        if L["kind"] != "pool":
            pre = L["name"] + ("." if L["kind"] == "bn0" else ".1.")
            state[pre + "running_mean"], state[pre + "running_var"] = L["running"][0], L["running"][1]
    return losses, state, norms


def dp_clipped_steps(net, cases, steps, dtype, max_norm, wd=TEST_WD, **loss_args):
    """encoder_dp_ref.dp_steps with the clip: the ranks' gradients are summed, the norm is that of sum / world, and every
    tensor steps with scale = f32(coef / world) -> (final parameters by name, [info per step])."""
    world = len(cases)
    sd = net.state_dict()
    order = D.param_names(net)
    tensors = {n: sd[n].detach().to(dtype).clone() for n in order}
    layers = [R.stack_layers(net, dtype) for _ in range(world)]
    rnn_names = R.rnn_params(net, dtype)[0]
    ps = [tensors[n] for n in order]
    ms, vs, step, infos = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], 0, []
    for _ in range(steps):
        total = None
        for r, (mel, lens, image, label) in enumerate(cases):
            D._set_layers(layers[r], tensors)
            _, grads, cache = R.full_grads(layers[r], (rnn_names, [tensors[n] for n in rnn_names]), mel.to(dtype), lens,
                                           image.to(dtype), label, **loss_args)
            for L, c in zip(layers[r], cache):
                if L["kind"] != "pool":
                    L["running"] = c["running"]
            grads = [grads[n].reshape(tensors[n].shape) for n in order]
            total = grads if total is None else [a + b for a, b in zip(total, grads)]
        ps, ms, vs, step, info = clipped_step(ps, total, ms, vs, step, 1.0 / world, max_norm, wd)
        tensors = dict(zip(order, ps))
        infos.append(info)
    return tensors, infos


if __name__ == "__main__":
    for k, val in measure_yardsticks().items():
        print("%-8s %.3e" % (k, val))
