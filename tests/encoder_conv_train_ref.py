"""Plain-torch restatement of the speech encoder's conv stack in TRAINING mode, forward and backward written out by hand
(tests/test_encoder_conv_train_*.py): one function per launch of ops.conv_stack_train and its backward, taking the operands
the kernels see (activations NHWC [B, 1, W, C], weights (O, C, k) in torch's order), and the whole stack composed from them.
Any dtype, any device; nothing here uses autograd, so the ReLU masks and pool maxima of the backward can be REPLAYED from
another run (`decisions`), and mutants can be made.  `mutant` names one deliberate mistake:
  "pad_m1"      the temporal-conv input gradient uses pad - 1
  "no_parity"   ... or ignores the parity rule of a strided convolution ((i + pad - t) // s for every tap)
  "bn_no_xhat"  the BatchNorm backward drops the mean(dz * xhat) term
  "pool_no_add" the pool backward assigns instead of adding where two windows meet
  "biased_var"  the running variance is updated with the biased batch variance
  "bn0_dropped" the leading BatchNorm2d(1) gets no gradients
  "pad_even"    the input gradient gives every tap the rows of its parity as if pad were even ((i - t) % s == 0)
  "even_k_drop" ... or loses the last tap of an even k
  "col_tail_zero" the weight gradient leaves the columns c >= 64 * (Cin // 64) zero (a whole-tile-only column clip)
The last three are inert at the seven layer geometries (every pad even, every k odd, every Cin a multiple of 64) and are
what the edge cases below exist for.
tests/test_encoder_conv_train_cpu.py pins the composition to torch autograd through the model's own nn.Sequential.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import encoder_ref
import encoder_train_ref as TR

BN_EPS = 1e-5
BN_MOMENTUM = 0.1

# (Cin, Cout, (k, stride, pad)) of the seven temporal convolutions (Audio_to_Image/speech_encoder.py:26-37)
LAYER_GEOMS = [(64, 64, (3, 1, 1)), (64, 128, (17, 2, 8)), (128, 256, (13, 2, 6)), (256, 256, (3, 1, 1)),
               (256, 512, (9, 2, 4)), (512, 512, (3, 1, 1)), (512, 1024, (5, 2, 2))]

rel_err = TR.rel_err


# ---- launches --------------------------------------------------------------------------------------------------------
def conv_fwd(x, w, geom):
    """Raw temporal convolution, no bias.  w (O, C, k)."""
    return encoder_ref.conv1d_pre(x, w, None, *geom)


def conv_dgrad(dy, w, geom, W, mutant=None):
    """dx[b, i, c] = sum_t sum_o dy[b, (i + pad - t) / s, o] w[o, c, t] over the taps with (i + pad - t) % s == 0 and the
    quotient in [0, Wo).  dy [B, 1, Wo, O], w (O, C, k) -> [B, 1, W, C]."""
    k, s, pad = geom
    if mutant == "pad_m1":
        pad = pad - 1
    B, _, Wo, O = dy.shape
    i = torch.arange(W, device=dy.device)
    dx = dy.new_zeros((B, W, w.shape[1]))
    for t in range(k - 1 if (mutant == "even_k_drop" and k % 2 == 0) else k):
        num = i + pad - t
        j = torch.div(num, s, rounding_mode="floor")
        ok = (j >= 0) & (j < Wo)
        if mutant != "no_parity":
            ok = ok & ((i - t if mutant == "pad_even" else num) % s == 0)
        if bool(ok.any()):
            dx[:, ok] += dy[:, 0, j[ok]] @ w[:, :, t]
    return dx.unsqueeze(1)


def conv_wgrad(x, dy, geom, mutant=None):
    """dW[o, c, 0, t] = sum_{b, ox} dy[b, ox, o] x[b, ox s - pad + t, c] -> (O, C, 1, k)."""
    k, s, pad = geom
    B, _, Wo, O = dy.shape
    xp = F.pad(x[:, 0], (0, 0, pad, pad))
    g = dy[:, 0].reshape(B * Wo, O)
    dw = [g.t() @ xp[:, t:t + s * (Wo - 1) + 1:s].reshape(B * Wo, -1) for t in range(k)]
    dw = torch.stack(dw, 2).unsqueeze(2)
    if mutant == "col_tail_zero":
        dw[:, 64 * (x.shape[3] // 64):] = 0
    return dw


def bn_finalize(y, gamma, beta, running, mutant=None):
    """Batch statistics of y [..., C] over its rows -> coef = (mean, invstd, scale, shift) and the updated
    (running_mean, running_var, num_batches_tracked) as nn.BatchNorm2d(momentum 0.1) in training mode leaves them."""
    C = y.shape[-1]
    y2 = y.reshape(-1, C)
    n = y2.shape[0]
    mean = y2.mean(0)
    var = ((y2 - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    scale = gamma * invstd
    rm, rv, nbt = running
    unb = var if (mutant == "biased_var" or n == 1) else var * n / (n - 1)
    new = ((1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mean, (1 - BN_MOMENTUM) * rv + BN_MOMENTUM * unb, nbt + 1)
    return (mean, invstd, scale, beta - mean * scale), new


def bn_relu_forward(y, coef):
    """-> (z, out): the BatchNorm output before the ReLU (the quantity a decision depends on) and after it."""
    z = y * coef[2] + coef[3]
    return z, torch.relu(z)


def bn_relu_backward(y, mask, dout, coef, mutant=None):
    """mask: out > 0.  -> (dy, dgamma, dbeta)."""
    C = y.shape[-1]
    mean, invstd, scale, _ = coef
    dz = torch.where(mask, dout, torch.zeros_like(dout)).reshape(-1, C)
    xhat = ((y - mean) * invstd).reshape(-1, C)
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    m1, m2 = dz.mean(0), (dz * xhat).mean(0)
    if mutant == "bn_no_xhat":
        m2 = torch.zeros_like(m2)
    return (scale * (dz - m1 - xhat * m2)).reshape(y.shape), dgamma, dbeta


def bn_plain_backward(x, dout, coef):
    """BatchNorm backward without an activation (the leading BatchNorm2d(1), C = 1 over every element)."""
    return bn_relu_backward(x, torch.ones_like(x, dtype=torch.bool), dout, coef)


def pool_windows(x):
    """The three candidates of every window, [B, H, Wo, 3, C] with -inf at the padding, and their positions [Wo, 3]."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1), value=float("-inf"))
    cand = torch.stack([xp[:, :, t:t + W:2] for t in range(3)], 3)
    pos = 2 * torch.arange(W // 2, device=x.device).unsqueeze(1) + torch.arange(-1, 2, device=x.device).unsqueeze(0)
    return cand, pos


def pool_argmax(x):
    """Position of every window's maximum, lowest position on a tie (torch's max_pool2d rule) -> int64 [B, H, Wo, C]."""
    cand, pos = pool_windows(x)
    m = cand.max(3, keepdim=True)[0]
    first = (cand == m).to(torch.int8).argmax(3)                      # the first of equal entries
    return pos[:, 0].view(1, 1, -1, 1) + first


def pool_gap(x):
    """Difference between the two largest entries of every window (inf where the window has one entry)."""
    cand, _ = pool_windows(x)
    top = cand.topk(2, dim=3)[0]
    return top[:, :, :, 0] - top[:, :, :, 1]


def pool_backward(shape, idx, dy, mutant=None):
    B, H, W, C = shape
    dx = dy.new_zeros((B, H, W, C))
    if mutant == "pool_no_add":
        return dx.scatter(2, idx, dy)
    return dx.scatter_add(2, idx, dy)


# ---- the whole stack ---------------------------------------------------------------------------------------------------
def stack_layers(net, dtype=torch.float64, device="cpu"):
    """CNNRNN.Conv as a list of dicts in module order: kind "bn0" | "block" | "pool", parameter tensors (detached copies in
    `dtype`), running statistics, state_dict names and, for a block, geom (None for the first (n_mels x 1) layer)."""
    c = lambda t: t.detach().to(device=device, dtype=dtype).clone()
    layers = []
    for i, m in enumerate(net.Conv):
        if isinstance(m, nn.BatchNorm2d):
            layers.append(dict(kind="bn0", name="Conv.%d" % i, gamma=c(m.weight), beta=c(m.bias),
                               running=(c(m.running_mean), c(m.running_var), int(m.num_batches_tracked))))
        elif isinstance(m, nn.MaxPool2d):
            layers.append(dict(kind="pool"))
        else:
            conv, bn = m[0], m[1]
            first = conv.in_channels == 1
            w = c(conv.weight)
            layers.append(dict(kind="block", name="Conv.%d" % i, wshape=tuple(w.shape),
                               w=w[:, 0, :, 0].unsqueeze(2) if first else w[:, :, 0, :],
                               geom=(1, 1, 0) if first else (conv.kernel_size[1], conv.stride[1], conv.padding[1]),
                               gamma=c(bn.weight), beta=c(bn.bias),
                               running=(c(bn.running_mean), c(bn.running_var), int(bn.num_batches_tracked))))
    return layers


def stack_forward(layers, mel, mutant=None):
    """mel [B, 1, T, n_mels] -> (features [B, 1, T/64, 1024], cache).  cache[i] of layer i holds what its backward needs,
    the layer's own decisions (mask / idx), the quantity they depend on (z / gap) and the updated running statistics."""
    h = mel
    cache = []
    for L in layers:
        if L["kind"] == "bn0":
            coef, new = bn_finalize(h.reshape(-1, 1), L["gamma"], L["beta"], L["running"], mutant)
            out = h * coef[2] + coef[3]
            cache.append(dict(x=h, coef=coef, running=new, out=out))
        elif L["kind"] == "pool":
            out = encoder_ref.maxpool_w3s2(h)
            cache.append(dict(x=h, idx=pool_argmax(h), gap=pool_gap(h), out=out))
        else:
            y = conv_fwd(h, L["w"], L["geom"])
            coef, new = bn_finalize(y, L["gamma"], L["beta"], L["running"], mutant)
            z, out = bn_relu_forward(y, coef)
            cache.append(dict(x=h, y=y, z=z, out=out, mask=out > 0, coef=coef, running=new))
        h = out
    return h, cache


MASS = "_mass."   # prefix of the entries of a gradient dict that are no gradients (see stack_backward)


def stack_backward(layers, cache, dfeat, decisions=None, mutant=None):
    """-> (grads keyed by state_dict name, d mel).  decisions[i], where given, replaces layer i's own mask / idx.
    The gradient of the leading BatchNorm's bias is structurally ZERO: a constant added to the first convolution's input is
    removed by that block's own BatchNorm, so sum(dout) cancels to rounding noise and max|ref| is no scale for it.  The
    entry MASS + name holds sum|dout|, the mass of the terms that cancel: grad_err measures that gradient against it."""
    g = dfeat
    grads = {}
    for i in range(len(layers) - 1, -1, -1):
        L, c = layers[i], cache[i]
        dec = decisions[i] if decisions is not None and decisions[i] is not None else None
        if L["kind"] == "pool":
            g = pool_backward(c["x"].shape, c["idx"] if dec is None else dec, g, mutant)
        elif L["kind"] == "block":
            dy, dgamma, dbeta = bn_relu_backward(c["y"], c["mask"] if dec is None else dec, g, c["coef"], mutant)
            grads[L["name"] + ".0.weight"] = conv_wgrad(c["x"], dy, L["geom"]).reshape(L["wshape"])
            grads[L["name"] + ".1.weight"], grads[L["name"] + ".1.bias"] = dgamma, dbeta
            g = conv_dgrad(dy, L["w"], L["geom"], c["x"].shape[2], mutant)
        else:
            grads[MASS + L["name"] + ".bias"] = g.abs().sum()
            g, dgamma, dbeta = bn_plain_backward(c["x"].reshape(-1, 1), g.reshape(-1, 1), c["coef"])
            g = g.reshape(c["x"].shape)
            if mutant == "bn0_dropped":
                dgamma, dbeta = torch.zeros_like(dgamma), torch.zeros_like(dbeta)
            grads[L["name"] + ".weight"], grads[L["name"] + ".bias"] = dgamma, dbeta
    return grads, g


def grad_err(name, got, ref_grads):
    """rel_err of gradient `name`, except where ref_grads carries a cancelling-sum mass for it (stack_backward)."""
    ref = ref_grads[name]
    mass = ref_grads.get(MASS + name)
    if mass is None:
        return rel_err(got.reshape(ref.shape), ref)
    return float((got.detach().double().cpu().reshape(ref.shape) - ref.double().cpu()).abs().max()) / float(mass)


def grad_names(grads):
    return [n for n in grads if not n.startswith(MASS)]


def own_decisions(layers, cache):
    return [c["mask"] if L["kind"] == "block" else (c["idx"] if L["kind"] == "pool" else None) for L, c in zip(layers, cache)]


def running_state(layers, cache):
    """state_dict entries of the running statistics after the call."""
    out = {}
    for L, c in zip(layers, cache):
        if L["kind"] == "pool":
            continue
        pre = L["name"] + ("." if L["kind"] == "bn0" else ".1.")
        out[pre + "running_mean"], out[pre + "running_var"] = c["running"][0], c["running"][1]
        out[pre + "num_batches_tracked"] = torch.tensor(c["running"][2])
    return out


# ---- stack + LSTM head + loss, and optimiser trajectories ---------------------------------------------------------------
def rnn_params(net, dtype=torch.float64):
    sfx = ["", "_reverse"][:net.num_direction]
    names = ["RNN.%s_l0%s" % (n, s) for s in sfx for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    sd = net.state_dict()
    return names, [sd[n].detach().to(dtype).clone() for n in names]


def full_grads(layers, rnn, mel, lens, image, label, decisions=None, mutant=None, **loss_args):
    """Stack (by hand) -> lstm_head and encoder_loss of encoder_train_ref (autograd from the features on) -> every
    gradient.  Returns (loss dict, grads by name, cache)."""
    names, params = rnn
    feat, cache = stack_forward(layers, mel, mutant)
    leaf = feat.detach().clone().requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    _, sent, _, _ = TR.lstm_head(leaf[:, 0], lens, ps)
    res = TR.encoder_loss(sent, image, label, **loss_args)
    gs = torch.autograd.grad(res["loss"], [leaf] + ps)
    grads, _ = stack_backward(layers, cache, gs[0].detach(), decisions, mutant)
    grads.update(dict(zip(names, gs[1:])))
    return {k: v.detach() for k, v in res.items()}, grads, cache


def trajectory(net, mel, lens, image, label, steps, dtype, lr=1e-3, weight_decay=1e-5, **loss_args):
    """`steps` optimiser steps on one fixed batch with stock torch.optim.Adam on the CPU in `dtype`, the gradients from
    full_grads -> ([loss dict per step], final state: every Conv.* / RNN.* tensor by state_dict name)."""
    layers = stack_layers(net, dtype)
    names, params = rnn_params(net, dtype)
    leaves = {}
    for L in layers:
        if L["kind"] == "block":
            leaves[L["name"] + ".0.weight"] = ("w", L)
            leaves[L["name"] + ".1.weight"], leaves[L["name"] + ".1.bias"] = ("gamma", L), ("beta", L)
        elif L["kind"] == "bn0":
            leaves[L["name"] + ".weight"], leaves[L["name"] + ".bias"] = ("gamma", L), ("beta", L)
    # the optimiser sees the tensors in the parameter's own shape and in model.parameters() order
    tensors = {}
    for n, (key, L) in leaves.items():
        tensors[n] = (L[key].reshape(L["wshape"]) if key == "w" else L[key]).clone().requires_grad_(True)
    for n, p in zip(names, params):
        tensors[n] = p.clone().requires_grad_(True)
    order = [n for n, _ in net.named_parameters()]
    opt = torch.optim.Adam([tensors[n] for n in order], lr=lr, weight_decay=weight_decay)
    losses = []
    mel, image = mel.to(dtype), image.to(dtype)
    for _ in range(steps):
        for n, (key, L) in leaves.items():
            t = tensors[n].detach()
            if key == "w":
                t = t[:, 0, :, 0].unsqueeze(2) if t.shape[1] == 1 and t.shape[3] == 1 else t[:, :, 0, :]
            L[key] = t
        res, grads, cache = full_grads(layers, (names, [tensors[n].detach() for n in names]), mel, lens, image, label,
                                       **loss_args)
        for L, c in zip(layers, cache):
            if L["kind"] != "pool":
                L["running"] = c["running"]
        opt.zero_grad()
        for n in order:
            tensors[n].grad = grads[n].reshape(tensors[n].shape).clone()
        opt.step()
        losses.append(res)
    state = {n: t.detach().clone() for n, t in tensors.items()}
    for L in layers:
        if L["kind"] != "pool":
            pre = L["name"] + ("." if L["kind"] == "bn0" else ".1.")
            state[pre + "running_mean"], state[pre + "running_var"] = L["running"][0], L["running"][1]
            state[pre + "num_batches_tracked"] = torch.tensor(L["running"][2])
    return losses, state


BN_MARGIN = 5e-4   # bn_case clears this much around zero; the GPU test asserts its own (smaller) m on the fp64 values


# ---- seeded inputs -------------------------------------------------------------------------------------------------------
def margin_ok(z, m):
    return bool((z.abs() >= m).all())


def conv_case(cin, cout, geom, B, Wo, seed=0):
    """x [B, 1, W, cin], w (cout, cin, k) and a cotangent dy [B, 1, Wo, cout] in fp64, every value representable in fp32."""
    k, s, pad = geom
    W = Wo * s
    g = torch.Generator().manual_seed(9000 + seed + 7 * cin + 13 * cout + Wo)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    return r(B, 1, W, cin), r(cout, cin, k) * 0.02, r(B, 1, Wo, cout)


def bn_case(M, C, seed=0, m=BN_MARGIN):
    """y [M rows, C], gamma, beta, dout and running statistics; elements of y whose BatchNorm output would fall within m of
    zero are nudged away (by 4 m / scale) until none is left."""
    g = torch.Generator().manual_seed(9500 + seed + M + C)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    y = r(1, 1, M, C) * 1.5 + 0.3
    gamma, beta = 1.0 + 0.1 * r(C), 0.2 * r(C)
    gamma, beta = gamma.float().double(), beta.float().double()
    dout = r(1, 1, M, C)
    running = (0.2 * r(C), 0.5 + r(C).abs(), 3)
    for _ in range(20):
        coef, _ = bn_finalize(y, gamma, beta, running)
        z = y * coef[2] + coef[3]
        near = z.abs() < m
        if not bool(near.any()):
            break
        y = torch.where(near, y + 4 * m / coef[2] * torch.where(z >= 0, 1.0, -1.0), y).float().double()
    else:
        raise RuntimeError("bn_case: could not clear the margin")
    return y, gamma, beta, dout, running


def pool_case(B, W, C, seed=0, ties=False, H=1):
    """Pool input [B, H, W, C] and a cotangent.  The values are a random permutation of an even grid over [-2, 2), so any two
    differ by at least 4 / (B H W C); with `ties` the input is post-ReLU (every negative value an exact zero: windows of
    zeros tie) and one positive tie is constructed at positions 0 and 1 of (b, c) = (0, 0)."""
    g = torch.Generator().manual_seed(9800 + seed + 3 * W + C)
    n = B * H * W * C
    x = (torch.randperm(n, generator=g).double() * (4.0 / n) - 2.0).view(B, H, W, C).float().double()
    if ties:
        x = torch.relu(x)
        x[0, 0, 0, 0] = x[0, 0, 1, 0] = 2.5
    dy = torch.randn(B, H, W // 2, C, generator=g, dtype=torch.float32).double()
    return x, dy


def mel_case(B, T, n_mels=40, seed=0):
    """Log-mel-like input: values in [-80, 0] dB, fp32-representable."""
    g = torch.Generator().manual_seed(9900 + seed)
    return (-80.0 * torch.rand(B, 1, T, n_mels, generator=g, dtype=torch.float32)).double()


def stack_net(bidirectional=True, nhidden=1024, seed=11):
    """A seeded CNNRNN at full conv widths (fresh running statistics, as training from scratch starts)."""
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    torch.manual_seed(seed)
    return CNNRNN(40, embedding_dim=1024, nhidden=nhidden, nsent=nhidden, bidirectional=bidirectional, rnn_layers=1).eval()


def trainer_case(B=4, T=128, H=512, seed=0):
    """One fixed batch for the EncoderTrainer tests: mel, lengths (sorted descending), image features, labels."""
    g = torch.Generator().manual_seed(9950 + seed)
    mel = mel_case(B, T, seed=seed + 1)
    L = T // 64
    lens = sorted(torch.randint(1, L + 1, (B,), generator=g).tolist(), reverse=True)
    lens[0] = L
    image = torch.randn(B, H, generator=g, dtype=torch.float32).double()
    label = torch.tensor([0, 1, 0, 2][:B] if B <= 4 else torch.randint(0, 3, (B,), generator=g).tolist())
    return mel, lens, image, label


# ---- the cases of the GPU tests and the fp32 yardstick of their bounds ------------------------------------------------------
CONV_CASES = ([(cin, cout, geom, 3, Wo) for cin, cout, geom in LAYER_GEOMS for Wo in (1, 8)]
              + [(64, 64, (3, 1, 1), 3, 2048), (512, 1024, (5, 2, 2), 33, 32)])
BN_CASES = [(24, 64), (24, 1024), (6144, 64), (6144, 1024)]
BN0_CASE = (3, 64)                    # B, T of the scalar input BatchNorm
POOL_CASES = [(3, W, C, ties) for C in (64, 512) for W in (2, 16) for ties in (False, True)]
STACK_CASE = (4, 128)

# Off the layer shapes.  (cin, cout, (k, s, pad), B, Wo), W = Wo s:
CONV_EDGE_CASES = [
    (32, 32, (1, 1, 0), 3, 8),         # kw = 1; Cin < 64 in the 64-wide dgrad template; one K chunk
    (4, 32, (2, 2, 0), 3, 8),          # kw == stride: one tap per phase; the smallest Cin
    (36, 96, (4, 2, 1), 5, 8),         # even k, odd pad; 3 chunks per tap; wgrad 128 x 64 tile partial in both axes
    (68, 32, (3, 2, 1), 3, 16),        # odd pad (r != ph); Cin = 68 in the 128-wide template; wgrad 64 x 64 + a 4-column tile
    (192, 160, (31, 2, 15), 2, 4),     # kw = 31 with W < kw; partial second column tile; wgrad 128 x 128 partial in both axes
    (64, 128, (30, 2, 14), 3, 4),      # wide even k
    (64, 64, (3, 1, 1), 33, 16),       # M = 528: 17 chunks in 4 splits, the last chunk half full
    (64, 64, (3, 1, 1), 5, 32),        # Mq = 160: partial second dgrad row tile, a batch boundary inside a tile
    (64, 64, (3, 1, 1), 1, 1),         # B = Wo = 1
]
# s2i_conv1d_wgrad takes these, s2i_conv1d_dgrad refuses them (Cout % 32 != 0; stride 4): DESIGN.md 8b3
WGRAD_ONLY_CASES = [(64, 36, (3, 1, 1), 3, 8), (8, 8, (4, 4, 0), 3, 8)]
# (M, C): Q = 1; Q = 3 with idle lanes; Q = 513 (gy = 3, one live quad in the last block) and a chunk of 65 that does not
# divide M; nparts = 1024 with trailing empty parts
BN_EDGE_CASES = [(8, 4), (65, 12), (129, 2052), (65537, 4)]
BN0_EDGE_CASES = [(1, 2), (7, 40)]    # R = 20 in one part; R = 2 800 in 43 parts of 66 with a ragged last one
POOL_EDGE_CASES = [(B, H, W, C, ties) for B, H, W, C in ((3, 2, 4, 4), (1, 1, 2, 4), (2, 1, 64, 68)) for ties in (False, True)]
# one block as ops.temporal_conv_bn_relu runs it: (cin, cout, geom or None for the first (n_mels x 1) layer, B, Wo)
BLOCK_CASES = ([(40, 64, None, B, T) for B, T in ((3, 8), (33, 32))]
               + [(cin, cout, geom, B, Wo) for cin, cout, geom in (LAYER_GEOMS[1], LAYER_GEOMS[6]) for B, Wo in ((3, 8), (33, 32))])
# the edge case at which each of the edge mutants leaves its bound (tests/test_encoder_conv_train_cpu.py asserts it)
MUTANT_KILLS = {"pad_even": (68, 32, (3, 2, 1), 3, 16), "even_k_drop": (36, 96, (4, 2, 1), 5, 8),
                "col_tail_zero": (68, 32, (3, 2, 1), 3, 16)}
TRAINER_STEPS = 5
TRAINER_LOSS = dict(jel=True, l1=True)


def bn0_case(B, T, seed=0):
    g = torch.Generator().manual_seed(9700 + seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    x = mel_case(B, T, seed=seed + 5)
    return x, (1.0 + 0.1 * r(1)).float().double(), (0.2 * r(1)).float().double(), r(B, 1, T, 40), (0.2 * r(1), 0.5 + r(1).abs(), 3)


def block_case(cin, cout, geom, B, Wo, seed=0):
    """x [B, 1, W, cin], w (cout, cin, k), gamma, beta, a cotangent of the block's output and running statistics."""
    x, w, dout = conv_case(cin, cout, geom or (1, 1, 0), B, Wo, seed=seed + 100)
    g = torch.Generator().manual_seed(9600 + seed + cin + cout + Wo)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    gamma, beta = (1.0 + 0.1 * r(cout)).float().double(), (0.2 * r(cout)).float().double()
    return x, w, gamma, beta, dout, (0.2 * r(cout), 0.5 + r(cout).abs(), 3)


def block_all(x, w, gamma, beta, dout, running, geom, dtype, mask=None):
    """Conv + train-mode BatchNorm + ReLU forward and backward in `dtype`; `mask` replaces the run's own out > 0."""
    c = lambda t: t.to(dtype)
    geom = geom or (1, 1, 0)
    y = conv_fwd(c(x), c(w), geom)
    coef, new = bn_finalize(y, c(gamma), c(beta), (c(running[0]), c(running[1]), running[2]))
    z, out = bn_relu_forward(y, coef)
    dy, dgamma, dbeta = bn_relu_backward(y, out > 0 if mask is None else mask, c(dout), coef)
    return dict(z=z, out=out, mask=out > 0, dx=conv_dgrad(dy, c(w), geom, x.shape[2]), dw=conv_wgrad(c(x), dy, geom),
                dgamma=dgamma, dbeta=dbeta, running_mean=new[0], running_var=new[1], nbt=new[2])


def block_errs(got, ref, what=""):
    """[(class, what, rel_err)] of one block's compared tensors."""
    e = lambda k: rel_err(got[k].reshape(ref[k].shape), ref[k])
    return [("block_out", what + " out", e("out")), ("block_dx", what + " dx", e("dx")), ("block_dw", what + " dW", e("dw")),
            ("block_dparam", what + " dgamma", e("dgamma")), ("block_dparam", what + " dbeta", e("dbeta")),
            ("block_running", what + " running_mean", e("running_mean")), ("block_running", what + " running_var", e("running_var"))]


def bn_all(y, gamma, beta, dout, running, dtype, relu=True):
    """One BatchNorm (+ ReLU) case forward and backward in `dtype` -> dict of the compared tensors (and z)."""
    c = lambda t: t.to(dtype)
    shape = y.shape
    if not relu:
        y, dout = y.reshape(-1, 1), dout.reshape(-1, 1)
    coef, new = bn_finalize(c(y), c(gamma), c(beta), (c(running[0]), c(running[1]), running[2]))
    if relu:
        z, out = bn_relu_forward(c(y), coef)
        dy, dgamma, dbeta = bn_relu_backward(c(y), out > 0, c(dout), coef)
    else:
        z = out = (c(y) * coef[2] + coef[3]).reshape(shape)
        dy, dgamma, dbeta = bn_plain_backward(c(y), c(dout), coef)
        dy = dy.reshape(shape)
    return dict(z=z, out=out, dy=dy, dgamma=dgamma, dbeta=dbeta, running_mean=new[0], running_var=new[1], nbt=new[2])


def stack_z_margins(cache64, yard_z):
    """m per layer: 100 x the forward yardstick x the layer's largest |z| (blocks) or |x| (pools)."""
    out = []
    for c in cache64:
        out.append(100 * yard_z * float((c["z"] if "z" in c else c["x"]).abs().max()) if ("z" in c or "idx" in c) else None)
    return out


def decision_report(layers, cache64, decisions, margins):
    """Per layer with decisions: (layer index, kind, elements, flipped, flipped outside the margin).  A block's decision
    differs from the fp64 forward's own where mask != (z > 0); a pool's where idx != argmax; `outside`: |z| (or the
    window's top-two gap) is not below the layer's m."""
    rep = []
    for i, (L, c) in enumerate(zip(layers, cache64)):
        if L["kind"] == "block":
            flip = decisions[i].cpu() != c["mask"]
            rep.append((i, "block", flip.numel(), int(flip.sum()), int((flip & ~(c["z"].abs() < margins[i])).sum())))
        elif L["kind"] == "pool":
            flip = decisions[i].cpu() != c["idx"]
            rep.append((i, "pool", flip.numel(), int(flip.sum()), int((flip & ~(c["gap"] < margins[i])).sum())))
    return rep


def measure_yardsticks(verbose=True):
    """The restatement in fp32 against its fp64 run on the CPU over every case of tests/test_encoder_conv_train_gpu.py ->
    {tensor class: worst max|fp32 - fp64| / max|fp64|}.  The GPU module's BOUNDS are twice these."""
    Y = {}

    def put(cls, e):
        Y[cls] = max(Y.get(cls, 0.0), e)

    f = lambda t: t.float()
    for case in CONV_CASES + CONV_EDGE_CASES + WGRAD_ONLY_CASES:
        cin, cout, geom, B, Wo = case
        x, w, dy = conv_case(cin, cout, geom, B, Wo)
        if case not in WGRAD_ONLY_CASES:
            put("dgrad", rel_err(conv_dgrad(f(dy), f(w), geom, x.shape[2]), conv_dgrad(dy, w, geom, x.shape[2])))
        put("wgrad", rel_err(conv_wgrad(f(x), f(dy), geom), conv_wgrad(x, dy, geom)))
    cases = ([bn_case(M, C) + (True,) for M, C in BN_CASES + BN_EDGE_CASES]
             + [bn0_case(B, T) + (False,) for B, T in [BN0_CASE] + BN0_EDGE_CASES])
    for y, gamma, beta, dout, running, relu in cases:
        a, b = bn_all(y, gamma, beta, dout, running, torch.float32, relu), bn_all(y, gamma, beta, dout, running, torch.float64, relu)
        assert relu is False or torch.equal(a["out"] > 0, b["out"] > 0)
        put("bn_out", rel_err(a["out"], b["out"]))
        put("bn_dy", rel_err(a["dy"], b["dy"]))
        put("bn_dparam", max(rel_err(a["dgamma"], b["dgamma"]), rel_err(a["dbeta"], b["dbeta"])))
        put("running", max(rel_err(a["running_mean"], b["running_mean"]), rel_err(a["running_var"], b["running_var"])))
    for B, H, W, C, ties in [(B, 1, W, C, ties) for B, W, C, ties in POOL_CASES] + POOL_EDGE_CASES:
        x, dy = pool_case(B, W, C, ties=ties, H=H)
        idx = pool_argmax(x)
        put("pool_dx", rel_err(pool_backward(x.shape, idx, f(dy)), pool_backward(x.shape, idx, dy)))
    # one block: the fp32 run's own ReLU decisions replayed into the fp64 backward
    Y["_block_flips"] = []
    for case in BLOCK_CASES:
        inputs = block_case(*case)
        a = block_all(*inputs, case[2], torch.float32)
        b = block_all(*inputs, case[2], torch.float64, mask=a["mask"])
        Y["_block_flips"].append((case, int((a["mask"] != b["mask"]).sum())))
        for cls, _, e in block_errs(a, b):
            put(cls, e)
    # whole stack: the fp32 run's own decisions replayed into the fp64 backward
    net = stack_net(bidirectional=True, nhidden=512)
    mel = mel_case(*STACK_CASE)
    l64, l32 = stack_layers(net), stack_layers(net, torch.float32)
    f64, c64 = stack_forward(l64, mel)
    f32, c32 = stack_forward(l32, f(mel))
    put("stack_feat", rel_err(f32, f64))
    for a, b in zip(c32, c64):
        if "z" in a:
            put("stack_z", rel_err(a["z"], b["z"]))
    dfeat = stack_dfeat(f64.shape)
    dec = own_decisions(l32, c32)
    g64, _ = stack_backward(l64, c64, dfeat, dec)
    g32, _ = stack_backward(l32, c32, f(dfeat))
    for n in grad_names(g64):
        cls = {"Conv.0.weight": "stack_bn0_dgamma", "Conv.0.bias": "stack_bn0_dbeta"}.get(n, "stack_grad")
        put(cls, grad_err(n, g32[n], g64))
    r64, r32 = running_state(l64, c64), running_state(l32, c32)
    for n in r64:
        if not n.endswith("num_batches_tracked"):
            put("stack_running", rel_err(r32[n], r64[n]))
    rep = decision_report(l64, c64, dec, stack_z_margins(c64, Y["stack_z"]))
    if verbose:
        for row in rep:
            print("decisions layer %d %s: %d elements, %d differ (%.4f %%), %d outside the margin" %
                  (row[0], row[1], row[2], row[3], 100.0 * row[3] / row[2], row[4]))
    Y["_decisions"] = rep
    # optimiser trajectory
    mel_t, lens, image, label = trainer_case()
    t64, _ = trajectory(net, mel_t, lens, image, label, TRAINER_STEPS, torch.float64, **TRAINER_LOSS)
    t32, _ = trajectory(net, mel_t, lens, image, label, TRAINER_STEPS, torch.float32, **TRAINER_LOSS)
    for a, b in zip(t32, t64):
        if verbose:
            print("trajectory fp64 / fp32:", {k: (float(b[k]), float(a[k])) for k in ("loss", "loss_jel", "loss_l1", "accu")})
        for k in ("loss", "loss_jel", "loss_l1"):          # each scalar against the step's total loss
            put("traj_loss", abs(float(a[k]) - float(b[k])) / abs(float(b["loss"])))
    return Y


def stack_dfeat(shape):
    g = torch.Generator().manual_seed(4242)
    return torch.randn(shape, generator=g, dtype=torch.float32).double()


if __name__ == "__main__":
    for k, v in measure_yardsticks().items():
        if not k.startswith("_"):
            print("%-18s %.3e" % (k, v))
