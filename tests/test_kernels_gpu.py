"""Per-operator parity of the HIP kernels (through the C-ABI) against plain torch fp32 on the CPU.

Tolerance: the north-star bound rtol=1e-3 / atol=1e-4 is for the 256x256 outputs of the whole
network; single operators are held to a tighter rtol=2e-4 / atol=2e-5 (fp32 MFMA is an exact fma
chain; only summation order differs from MKLDNN).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(a, b, rtol=RTOL, atol=ATOL, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().item() + 1e-30
    err = (a - b).abs()
    bound = atol * max(1.0, scale) + rtol * b.abs()
    bad = err > bound
    assert not bad.any(), "%s: max err %.3e (ref scale %.3e), %d/%d out of tolerance" % (
        what, err.max().item(), scale, int(bad.sum()), bad.numel())


def ref_block(x, cvec, w, gamma, beta, residual, kind, act, bias=None):
    """Reference restatement with stock torch ops, NCHW (model.py:125-169, 358-376)."""
    if cvec is not None:
        B, _, H, W = x.shape
        x = torch.cat((cvec.view(B, -1, 1, 1).repeat(1, 1, H, W), x), 1)
    if kind == "up":
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    elif kind == "k3s1":
        y = F.conv2d(x, w, padding=1)
    elif kind == "k4s2":
        y = F.conv2d(x, w, stride=2, padding=1)
    else:
        y = F.conv2d(x, w.view(w.shape[0], w.shape[1], 1, 1))
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if gamma is not None:
        y = F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5)
    if act == "glu":
        c = y.shape[1] // 2
        y = y[:, :c] * torch.sigmoid(y[:, c:])
    elif act == "lrelu":
        y = F.leaky_relu(y, 0.2)
    elif act == "tanh":
        y = torch.tanh(y)
    if residual is not None:
        y = y + residual
    return y


ACT = {"none": 0, "glu": 1, "lrelu": 2, "tanh": 3}

CASES = [
    # kind, B, H, Cx, Cc, Cout, act, residual
    ("k3s1", 2, 8, 16, 0, 32, "glu", False),
    ("k3s1", 3, 16, 8, 8, 24, "glu", False),      # broadcast vector concatenated first (factored path)
    ("k3s1", 2, 32, 32, 128, 64, "glu", False),   # G jointConv shape class: c_code folded into a class bias
    ("k3s1", 2, 8, 16, 0, 16, "none", True),       # ResBlock second half
    ("k3s1", 4, 4, 160, 0, 64, "lrelu", False),    # D tail: tiny map, big K -> split-K
    ("k3s1", 4, 4, 128, 32, 64, "lrelu", False),   # D jointConv with c_code
    ("k4s2", 2, 16, 8, 0, 16, "lrelu", False),
    ("k4s2", 4, 8, 192, 0, 256, "lrelu", False),   # split-K + BN stats via colstats
    ("up", 2, 4, 32, 0, 32, "glu", False),
    ("up", 3, 8, 16, 0, 8, "glu", False),
    ("up", 2, 32, 8, 0, 8, "glu", False),
    ("k1", 4, 1, 12, 16, 64, "glu", False),        # INIT_STAGE_G.fc: cat(c_code, z) -> Linear -> BN1d -> GLU
    ("k3s1", 2, 64, 8, 0, 8, "glu", False),        # many row tiles -> multi-part statistics
    ("k3s1", 2, 16, 32, 0, 64, "glu", False),      # K = 9 x 32 = 288: weight gradient on 96-row tiles (96x64)
    ("k3s1", 2, 16, 32, 0, 32, "none", True),      # ... 96x32
    ("k3s1", 2, 32, 32, 0, 32, "none", True),      # wide map, thin layer: row-segment weight gradient <32,32>
    ("k3s1", 3, 64, 32, 0, 64, "glu", False),      # ... <32,64>
    ("k3s1", 2, 32, 64, 0, 128, "glu", False),     # ... <64,128>
    ("k3s1", 2, 32, 64, 0, 64, "none", True),      # ... <64,64>
    ("k3s1", 2, 32, 64, 0, 32, "none", False),     # ... <64,32>
    # full-width D64 layers at batch 4 (BASELINE config 1 shapes)
    ("k4s2", 4, 32, 64, 0, 128, "lrelu", False),
    ("k4s2", 4, 16, 128, 0, 256, "lrelu", False),
    ("k4s2", 4, 8, 256, 0, 512, "lrelu", False),
    ("k3s1", 4, 4, 512, 128, 512, "lrelu", False),
    # full-width G layers at batch 4
    ("k1", 4, 1, 100, 128, 2048, "glu", False),
    ("up", 4, 4, 1024, 0, 1024, "glu", False),
    ("up", 4, 32, 128, 0, 128, "glu", False),
]


@pytest.fixture(params=[0, 3], ids=["f32", "bf16x3"])
def math_planes(request):
    """Native fp32 MFMA products, and the opt-in split-bf16 mode (3 planes: fp32-grade accuracy, same tolerances)."""
    from speech_to_image_translation_without_text_amd import ops
    old = ops.MATH_PLANES
    ops.MATH_PLANES = request.param
    yield request.param
    ops.MATH_PLANES = old


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_conv_bn_act_fwd_bwd(gpu, case, math_planes):
    from speech_to_image_translation_without_text_amd import ops
    kind, B, H, Cx, Cc, Cout, act, use_res = case
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()) % 100000)  # stable across processes
    kk = {"k3s1": 3, "k4s2": 4, "up": 3, "k1": 1}[kind]
    x = torch.randn(B, Cx, H, H, generator=g)
    cvec = torch.randn(B, Cc, generator=g) if Cc else None
    w = torch.randn(Cout, Cx + Cc, kk, kk, generator=g) * (1.0 / (kk * (Cx + Cc) ** 0.5))
    if kind == "k1":
        w = w.view(Cout, Cx + Cc)
    gamma = 1 + 0.1 * torch.randn(Cout, generator=g)
    beta = 0.1 * torch.randn(Cout, generator=g)
    Ho = {"k3s1": H, "k4s2": H // 2, "up": 2 * H, "k1": H}[kind]
    Cact = Cout // 2 if act == "glu" else Cout
    res = torch.randn(B, Cact, Ho, Ho, generator=g) if use_res else None
    gout = torch.randn(B, Cact, Ho, Ho, generator=g)

    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, cvec, w, gamma, beta, res)]
    ref = ref_block(*leaves, kind, act)
    ref.backward(gout)

    dl = [t.clone().to(gpu).requires_grad_(True) if t is not None else None for t in (x, cvec, w, gamma, beta, res)]
    xg = nhwc(dl[0].detach()).requires_grad_(True)
    resg = nhwc(dl[5].detach()).requires_grad_(True) if use_res else None
    rm = torch.zeros(Cout, device=gpu)
    rv = torch.ones(Cout, device=gpu)
    nbt = torch.zeros((), dtype=torch.long, device=gpu)
    out = ops.ConvBnAct.apply(xg, dl[1], dl[2], dl[3], dl[4], resg, kind, ACT[act], (rm, rv, nbt), True)
    out.backward(nhwc(gout.to(gpu)))
    torch.cuda.synchronize()

    close(nchw(out), ref, what="out")
    close(nchw(xg.grad), leaves[0].grad, what="dx")
    if Cc:
        close(dl[1].grad, leaves[1].grad, what="dcvec")
    close(dl[2].grad, leaves[2].grad, what="dw")
    close(dl[3].grad, leaves[3].grad, what="dgamma", atol=1e-4)
    close(dl[4].grad, leaves[4].grad, what="dbeta", atol=1e-4)
    if use_res:
        close(nchw(resg.grad), leaves[5].grad, what="dres")
    # running statistics follow torch's momentum rule with the unbiased variance
    with torch.no_grad():
        xin = leaves[0] if cvec is None else torch.cat(
            (leaves[1].view(B, -1, 1, 1).repeat(1, 1, H, H), leaves[0]), 1)
        yraw = ref_block(xin, None, leaves[2], None, None, None, kind, "none")
        m = yraw.transpose(0, 1).reshape(Cout, -1)
        close(rm, 0.1 * m.mean(1), what="running_mean", atol=1e-5)
        close(rv, 0.9 + 0.1 * m.var(1, unbiased=True), what="running_var", atol=1e-5)
    assert int(nbt.item()) == 1


TILE96 = [
    # kind, B, H, Cx, Cout, wmode, groups: 96-row tiles of the fp32 matrix kernel (plan_fwd picks them where 128-row tiles
    # end on a fraction of a round of the chip; forced here through the descriptor's tile_rows)
    ("k4s2", 6, 16, 64, 128, 0, 3),     # 384 rows = 4 x 96, three BatchNorm groups of 128 rows... not a multiple of 96 per group
    ("k4s2", 9, 16, 64, 128, 0, 3),     # 576 rows, groups of 192 = 2 x 96
    ("k3s1", 3, 16, 32, 256, 0, 1),     # 768 rows, two column tiles
    ("k3s1", 5, 8, 40, 136, 0, 1),      # ragged: 320 rows (last tile 32 rows), 136 columns, K = 360 (not a multiple of 32)
    ("tconv", 3, 8, 64, 128, 1, 1),     # input gradient of a stride-2 conv: four phases
    ("k4s2", 3, 8, 512, 256, 0, 1),     # 48 rows: too few for two tiles -> planner keeps 128 even when 96 is asked
]


@pytest.mark.parametrize("case", TILE96, ids=lambda c: "-".join(str(v) for v in c))
def test_tile_rows_96_equals_128(gpu, case):
    """The 96-row tile runs the same K loop per output element as the 128-row tile: results are bit-identical, and the
    BatchNorm partial sums add up to the same column sums."""
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd._lib import CONV_K3S1, CONV_K4S2, TCONV_K4S2
    kind, B, H, Cx, N, wmode, groups = case
    k = {"k3s1": CONV_K3S1, "k4s2": CONV_K4S2, "tconv": TCONV_K4S2}[kind]
    T = {"k3s1": 9, "k4s2": 16, "tconv": 16}[kind]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, H, H, Cx, generator=g).to(gpu)
    Np = (N + 3) & ~3
    packed = (torch.randn(T, Cx, Np, generator=g) * 0.05).to(gpu) if not wmode else (torch.randn(T, N, Cx, generator=g) * 0.05).to(gpu)
    outs = []
    for rows in (128, 96):
        ops.TILE_ROWS = rows
        try:
            stats = wmode == 0
            grp_ok = groups == 1 or ((x.shape[0] * (H // 2 if kind == "k4s2" else H) ** 2 // groups) % rows == 0)
            y, part, nparts = ops.conv_raw(k, x, None, packed, N, wmode=wmode, wR=packed.shape[1], ldw=packed.shape[2],
                                           stats=stats, groups=groups if grp_ok else 1)
            torch.cuda.synchronize()
            outs.append((y.clone(), None if part is None else part.double().sum(1).clone()))
        finally:
            ops.TILE_ROWS = 0
    assert torch.equal(outs[0][0], outs[1][0])
    if outs[0][1] is not None:
        close(outs[1][1].float(), outs[0][1].float(), rtol=1e-5, atol=1e-5, what="column sums")


WGRAD_TILES = [
    # kind, B, H, Cin, Cout      (taps x Cin a multiple of 256; the last two also have 256 | Cout)
    ("k4s2", 3, 32, 64, 128),
    ("k4s2", 5, 16, 128, 256),
    ("k3s1", 6, 8, 256, 512),
]


@pytest.mark.parametrize("case", WGRAD_TILES, ids=lambda c: "-".join(str(v) for v in c))
def test_weight_gradient_tile_shapes_against_torch(gpu, case):
    """igemm_wgrad_kernel with 128 x 128, 256 x 128 (512 threads) and 256 x 256 (1024 threads) tiles -- wgrad_bm forces each where
    the shape allows, 0 lets the planner's cost model choose -- against torch's fp32 weight gradient."""
    import torch.nn.functional as F
    from speech_to_image_translation_without_text_amd import _lib, ops
    from speech_to_image_translation_without_text_amd._lib import CONV_K3S1, CONV_K4S2
    kind, B, H, Cin, Cout = case
    g = torch.Generator().manual_seed(5)
    kk = 4 if kind == "k4s2" else 3
    Ho = H // 2 if kind == "k4s2" else H
    x = torch.randn(B, Cin, H, H, generator=g)
    gy = torch.randn(B, Cout, Ho, Ho, generator=g)
    w = torch.zeros(Cout, Cin, kk, kk, requires_grad=True)
    (F.conv2d(x, w, stride=2 if kind == "k4s2" else 1, padding=1) * gy).sum().backward()
    a = x.permute(0, 2, 3, 1).contiguous().to(gpu)
    gg = gy.permute(0, 2, 3, 1).contiguous().to(gpu)
    results = {}
    for bm in (128, 256, 512, 0):
        with _lib.tuning(wgrad_bm=bm):
            out = ops.wgrad_raw(CONV_K4S2 if kind == "k4s2" else CONV_K3S1, a, None, gg, (Cout, Cin, kk, kk))
        torch.cuda.synchronize()
        results[bm] = out.cpu()
        close(out.cpu(), w.grad, rtol=1e-3, atol=1e-3 * float(w.grad.abs().max()), what="dW (wgrad_bm=%d)" % bm)
    # one pixel order per output element whatever the tile: the shapes differ only in how the pixel range is split
    close(results[256], results[128], rtol=1e-4, atol=1e-4 * float(w.grad.abs().max()), what="256 x 128 against 128 x 128")


CONVACT = [
    # kind, B, H, Cin(true), Cin padded, Cout(true), n_out, act, bias
    ("k4s2", 2, 16, 3, 4, 16, 16, "lrelu", False),   # first D conv on an NHWC4 image
    ("k3s1", 2, 16, 16, 16, 3, 4, "tanh", False),    # GET_IMAGE_G -> NHWC4 image
    ("k1", 4, 1, 64, 64, 32, 32, "none", True),      # CA_NET.fc
    ("k3s1", 2, 64, 16, 16, 3, 4, "tanh", False),    # GET_IMAGE_G at scale: conv3_n4_tile_kernel<16>; dx on thin_in_kernel<16>
    ("k3s1", 2, 64, 64, 64, 3, 4, "tanh", False),    # M = 8192 gets a K split: small_n_conv_kernel<16>
    ("k4s2", 2, 128, 3, 4, 64, 64, "lrelu", False),  # first D conv at scale: its input gradient is tconv_n4_tile_kernel<64>
    ("k3s1", 2, 128, 16, 16, 3, 4, "tanh", False),   # weight gradient streamed by small_n_wgrad_kernel<4>
    ("k3s1", 2, 128, 32, 32, 3, 4, "tanh", False),   # ... <8>
    ("k3s1", 2, 128, 64, 64, 3, 4, "tanh", False),   # ... <16>
]


@pytest.mark.parametrize("case", CONVACT, ids=lambda c: "-".join(str(v) for v in c))
def test_conv_act_fwd_bwd(gpu, case):
    from speech_to_image_translation_without_text_amd import ops
    kind, B, H, Cin, Cinp, Cout, n_out, act, use_bias = case
    g = torch.Generator().manual_seed(7)
    kk = {"k3s1": 3, "k4s2": 4, "k1": 1}[kind]
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, kk, kk, generator=g) * 0.2
    if kind == "k1":
        w = w.view(Cout, Cin)
    bias = torch.randn(Cout, generator=g) if use_bias else None
    Ho = H // 2 if kind == "k4s2" else H
    gout = torch.randn(B, Cout, Ho, Ho, generator=g)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bl = bias.clone().requires_grad_(True) if use_bias else None
    ref = ref_block(xl, None, wl, None, None, None, kind, act, bias=bl)
    ref.backward(gout)

    xp = torch.zeros(B, Cinp, H, H)
    xp[:, :Cin] = x
    xg = nhwc(xp).to(gpu).requires_grad_(True)
    wg = w.to(gpu).requires_grad_(True)
    bg = bias.to(gpu).requires_grad_(True) if use_bias else None
    out = ops.ConvAct.apply(xg, wg, bg, kind, ACT[act], n_out)
    gp = torch.zeros(B, n_out, Ho, Ho)
    gp[:, :Cout] = gout
    out.backward(nhwc(gp).to(gpu))
    torch.cuda.synchronize()
    close(nchw(out)[:, :Cout], ref, what="out")
    if n_out > Cout:
        assert float(nchw(out.detach())[:, Cout:].abs().max()) == 0.0
    close(nchw(xg.grad)[:, :Cin], xl.grad, what="dx")
    close(wg.grad, wl.grad, what="dw")
    if use_bias:
        close(bg.grad, bl.grad, what="dbias")


def test_heads_and_losses(gpu):
    from speech_to_image_translation_without_text_amd import ops
    g = torch.Generator().manual_seed(3)
    B, C = 8, 32
    x = torch.randn(B, C, 4, 4, generator=g) * 0.3
    w = torch.randn(1, C, 4, 4, generator=g) * 0.1
    b = torch.randn(1, generator=g)
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    p = torch.sigmoid(F.conv2d(xl, wl, bl, stride=4)).view(-1)
    loss = F.binary_cross_entropy(p, torch.ones(B)) + 0.5 * F.binary_cross_entropy(p, torch.zeros(B))
    loss.backward()

    xg = nhwc(x).to(gpu).requires_grad_(True)
    wg, bg = w.to(gpu).requires_grad_(True), b.to(gpu).requires_grad_(True)
    pg = ops.LogitHead.apply(xg, wg, bg)
    lg = ops.BCELoss.apply(pg, 1.0, 1.0) + ops.BCELoss.apply(pg, 0.0, 0.5)
    lg.backward()
    torch.cuda.synchronize()
    close(pg, p, what="prob")
    close(lg, loss, what="bce")
    close(nchw(xg.grad), xl.grad, what="dx")
    close(wg.grad, wl.grad, what="dw")
    close(bg.grad, bl.grad, what="dbias")


def ref_class_aware(x, labels):
    """trainer.py:298-311 restated with boolean masks."""
    B, D = x.shape
    scores = x @ x.t()
    lab = torch.as_tensor(labels)
    pair = (lab[:, None] == lab[None, :]) & ~torch.eye(B, dtype=torch.bool)
    if pair.sum() > 0:
        return torch.clamp(scores.mean() - scores[pair].mean(), min=0).div(D).view(1)
    return torch.zeros(1)


@pytest.mark.parametrize("labels", [[0, 1, 2, 0, 1, 2, 0, 1], [0, 1, 2, 3, 4, 5, 6, 7], [0] * 8])
def test_class_aware_loss(gpu, labels):
    from speech_to_image_translation_without_text_amd import ops
    g = torch.Generator().manual_seed(11)
    B, D = 8, 512
    x = torch.randn(B, D, generator=g)
    # make same-class rows anti-correlated so that the hinge is active for the first label set
    xl = x.clone().requires_grad_(True)
    ref = ref_class_aware(xl, labels) * 3.0
    if ref.requires_grad:
        ref.backward()
    xg = x.to(gpu).requires_grad_(True)
    lab = torch.tensor(labels, dtype=torch.int32, device=gpu)
    out = ops.ClassAwareLoss.apply(xg, lab) * 3.0
    out.backward()
    torch.cuda.synchronize()
    close(out, ref, what="cal")
    close(xg.grad, xl.grad if xl.grad is not None else torch.zeros_like(x), what="dX")


def test_ca_net_pieces(gpu):
    from speech_to_image_translation_without_text_amd import ops
    g = torch.Generator().manual_seed(5)
    B, E = 6, 16
    pre = torch.randn(B, 4 * E, generator=g)
    eps = torch.randn(B, E, generator=g)
    pl = pre.clone().requires_grad_(True)
    h = pl[:, :2 * E] * torch.sigmoid(pl[:, 2 * E:])
    mu, lv = h[:, :E], h[:, E:]
    c = eps * torch.exp(0.5 * lv) + mu
    kl = torch.mean(1 + lv - mu.pow(2) - lv.exp()) * -0.5
    gc = torch.randn(B, E, generator=g)
    ((c * gc).sum() + 2.0 * kl + (mu * 0.3).sum()).backward()

    pg = pre.to(gpu).requires_grad_(True)
    hg = ops.Glu2d.apply(pg)
    mug, lvg = hg[:, :E], hg[:, E:]
    cg = ops.Reparam.apply(hg, eps.to(gpu))
    klg = ops.KLLoss.apply(mug, lvg)
    ((cg * gc.to(gpu)).sum() + 2.0 * klg + (mug * 0.3).sum()).backward()
    torch.cuda.synchronize()
    close(cg, c, what="c")
    close(klg, kl, what="kl")
    close(pg.grad, pl.grad, what="dpre")


def test_layout_and_optimizer(gpu):
    from speech_to_image_translation_without_text_amd import ops
    g = torch.Generator().manual_seed(9)
    img = torch.randn(2, 3, 16, 16, generator=g)
    ig = img.to(gpu).requires_grad_(True)
    n = ops.ToNHWC.apply(ig, 4)
    assert n.shape == (2, 16, 16, 4)
    close(n[..., :3], img.permute(0, 2, 3, 1), what="nhwc4")
    assert float(n[..., 3].abs().max()) == 0.0
    back = ops.ToNCHW.apply(n, 3)
    close(back, img, what="roundtrip")
    back.backward(torch.ones_like(back))
    close(ig.grad, torch.ones_like(img), what="layout grad")

    # fused Adam against torch.optim.Adam, 3 steps, odd length
    p0 = torch.randn(1003, generator=g)
    grads = [torch.randn(1003, generator=g) for _ in range(3)]
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=2e-4, betas=(0.5, 0.999))
    for gr in grads:
        pr.grad = gr.clone()
        opt.step()
    p = p0.to(gpu)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    step_dev = torch.zeros(1, dtype=torch.int32, device=gpu)
    for i, gr in enumerate(grads):
        ops.increment(step_dev)
        ops.adam_step(p, gr.to(gpu), m, v, 2e-4, 0.5, 0.999, 1e-8, step_dev=step_dev)
    torch.cuda.synchronize()
    close(p, pr, what="adam", rtol=1e-5, atol=1e-6)
    avg = p0.to(gpu).clone()
    ops.ema_update(avg, p, 0.999)
    close(avg, 0.999 * p0 + 0.001 * p.cpu(), what="ema", rtol=1e-6, atol=1e-6)


def test_split_bf16_products_against_fp64(gpu):
    """The opt-in split-bf16 matrix products (include/s2i_hip.h): a 4096 x 2048 x 1024 GEMM and a D-tower conv with its
    input- and weight-gradient against fp64.  Three planes must be at least as accurate as the native fp32 MFMA path
    (within 1.5x of its error); two planes are TF32-class (mean error below 2e-5 of mean |y|)."""
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd._lib import CONV_K1, CONV_K4S2, TCONV_K4S2
    g = torch.Generator(device=gpu).manual_seed(3)
    old = ops.MATH_PLANES
    try:
        # GEMM
        x = torch.randn(4, 32, 32, 2048, device=gpu, generator=g)
        w = torch.randn(1024, 2048, device=gpu, generator=g) / 2048 ** 0.5
        packed = ops.pack_weight(w, ops.PACK_PLAIN)
        ref = (x.view(-1, 2048).double() @ w.double().t())
        errs = {}
        for planes in (0, 1, 2, 3):
            ops.MATH_PLANES = planes
            y = ops.conv_raw(CONV_K1, x, None, packed, 1024, wR=packed.shape[1], ldw=packed.shape[2])[0]
            errs[planes] = float((y.view(-1, 1024).double() - ref).abs().mean() / ref.abs().mean())
        assert errs[3] <= 1.5 * errs[0], errs
        assert errs[2] <= 2e-5, errs
        assert 1e-4 <= errs[1] <= 5e-3, errs   # one plane = plain bf16 operands (2^-9 per factor)
        # conv forward / input gradient / weight gradient of Conv2d(64,128,k4,s2,p1) on (8,64,64,64)
        xc = torch.randn(8, 64, 64, 64, device=gpu, generator=g)
        wc = torch.randn(128, 64, 4, 4, device=gpu, generator=g) / 32.0
        gy = torch.randn(8, 32, 32, 128, device=gpu, generator=g)
        pk = ops.pack_weight(wc, ops.PACK_PLAIN)
        xn, wn, gn = (t.double().cpu() for t in (xc.permute(0, 3, 1, 2), wc, gy.permute(0, 3, 1, 2)))
        xn.requires_grad_(True)
        wn.requires_grad_(True)
        yref = torch.nn.functional.conv2d(xn, wn, stride=2, padding=1)
        yref.backward(gn)
        refs = (yref.detach(), xn.grad, wn.grad)
        cerr = {}
        for planes in (0, 3):
            ops.MATH_PLANES = planes
            y = ops.conv_raw(CONV_K4S2, xc, None, pk, 128, wR=pk.shape[1], ldw=pk.shape[2])[0]
            dx = ops.conv_raw(TCONV_K4S2, gy, None, pk, 64, wmode=1, wR=pk.shape[1], ldw=pk.shape[2])[0]
            dw = ops.wgrad_raw(CONV_K4S2, xc, None, gy, tuple(wc.shape))
            outs = (y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2), dw)
            cerr[planes] = [float((o.double().cpu() - r).abs().mean() / r.abs().mean()) for o, r in zip(outs, refs)]
        for e3, e0 in zip(cerr[3], cerr[0]):
            assert e3 <= 1.5 * e0 + 1e-9, cerr
    finally:
        ops.MATH_PLANES = old


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("act", ["none", "glu", "lrelu"])
def test_batchnorm_passes_against_formulas(gpu, act, dtype):
    """The three BatchNorm / activation passes (forward apply, backward column reduction, backward apply) on raw buffers with
    three BatchNorm groups, against their formulas evaluated in fp64 by torch: out = act(s y + t);
    part = (sum dz, sum dz xhat) per group; dy = s (dz - m0 - xhat m1)."""
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd._lib import ACT_GLU, ACT_LRELU, ACT_NONE, DT_BF16, DT_F32, check, ptr, stream
    lib = ops._lib_ready()
    a = {"none": ACT_NONE, "glu": ACT_GLU, "lrelu": ACT_LRELU}[act]
    dt, tdt = (DT_F32, torch.float32) if dtype == "f32" else (DT_BF16, torch.bfloat16)
    g = torch.Generator(device=gpu).manual_seed(3)
    G, M, C = 3, 3 * 520, 64                   # 520 rows per group: not a multiple of any block's row count
    Co = C // 2 if a == ACT_GLU else C
    y = torch.randn(M, C, device=gpu, generator=g).to(tdt)
    dout = torch.randn(M, Co, device=gpu, generator=g).to(tdt)
    coef = torch.randn(G, 4, C, device=gpu, generator=g)
    coef[:, 1].abs_().add_(0.5)
    red2 = torch.randn(G, 2, C, device=gpu, generator=g) * 0.1
    nparts = 4 * G
    part = torch.zeros(2, nparts, C, device=gpu)
    check(lib.s2i_bn_act_bwd_reduce_dt(dt, ptr(y), ptr(dout), Co, M, G, C, ptr(coef), a, ptr(part), nparts, stream()), "reduce")
    dy = torch.empty(M, C, device=gpu, dtype=tdt)
    check(lib.s2i_bn_act_bwd_apply_dt(dt, ptr(y), ptr(dout), Co, M, G, C, ptr(coef), ptr(red2), a, ptr(dy), stream()), "apply")
    out = torch.empty(M, Co, device=gpu, dtype=tdt)
    check(lib.s2i_bn_act_forward_dt(dt, ptr(y), M, G, C, ptr(coef), a, None, ptr(out), stream()), "forward")
    torch.cuda.synchronize()

    yd, dd = y.double().view(G, M // G, C), dout.double().view(G, M // G, Co)
    mean, istd, sc, sh = (coef[:, k].double().view(G, 1, C) for k in range(4))
    z = sc * yd + sh
    xh = (yd - mean) * istd
    if a == ACT_GLU:
        h = C // 2
        sg = torch.sigmoid(z[..., h:])
        ref_out = z[..., :h] * sg
        dz = torch.cat((dd * sg, dd * z[..., :h] * sg * (1 - sg)), -1)
    elif a == ACT_LRELU:
        ref_out = torch.where(z > 0, z, 0.2 * z)
        dz = torch.where(z > 0, dd, 0.2 * dd)
    else:
        ref_out, dz = z, dd
    ref_dy = sc * (dz - red2[:, 0].double().view(G, 1, C) - xh * red2[:, 1].double().view(G, 1, C))
    ref_part = torch.stack((dz.sum(1), (dz * xh).sum(1)))            # (2, G, C)
    got_part = part.double().view(2, G, nparts // G, C).sum(2)
    tol = 2e-2 if dtype == "bf16" else 1e-5    # bf16: the results are rounded to 8 significant bits
    for what, got, ref in (("forward", out.double().view(G, -1, Co), ref_out), ("apply", dy.double().view(G, -1, C), ref_dy),
                           ("reduce", got_part, ref_part)):
        scale = float(ref.abs().max()) + 1e-12
        rt = 1e-4 if what == "reduce" else tol
        assert float((ref - got).abs().max()) <= rt * scale, (what, float((ref - got).abs().max()), scale)
