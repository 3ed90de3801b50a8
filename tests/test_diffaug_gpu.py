"""GPU suite of the differentiable augmentation fused into the image layout conversion (csrc/s2i_diffaug.hip,
ops.DiffAugToNHWC, _DNet.forward(aug=...), TRAIN.DIFFAUG) against tests/diffaug_ref.py.

Bounds.  Policies without COLOR move and zero values and do no arithmetic: forward and backward equal the reference bit
for bit.  Policies with COLOR: inputs in [-1, 1], the chain is fewer than ten fp32 roundings on magnitudes below 4 plus a
tree-summed mean, under 3e-6 in all; the bound is 1e-5 absolute on the forward and 1e-5 max |dy| on the backward.  Every
mutant of the reference is held against the same comparison and must fail it.

Measured on an MI355X (worst over the three shapes and the four colour policies): forward 2.45e-7, backward
1.79e-7 max |dy| with fp32 gradient rows: 2.5 % and 1.8 % of the bounds."""
import random

import numpy as np
import pytest
import torch

import diffaug_ref as R
from helpers import CASES, configure

pytestmark = pytest.mark.gpu

COLOUR_POLICIES = (1, 3, 5, 7)
PLAIN_POLICIES = (0, 2, 4, 6)


@pytest.fixture(scope="module")
def cases(gpu):
    """Per shape: the inputs on the host and on the device, and a cache of fp64 references per (direction, policy)."""
    out = {}
    for N, H in R.SHAPES:
        x, table, dy = R.make_case(N, H)
        out[(N, H)] = dict(x=x, table=table, dy=dy, xd=torch.from_numpy(x).to(gpu), td=torch.from_numpy(table).to(gpu),
                           dyd=torch.from_numpy(dy).to(gpu), ref={})
    return out


def ref_of(c, direction, policy):
    key = (direction, policy)
    if key not in c["ref"]:
        c["ref"][key] = (R.forward(c["x"], c["table"], policy) if direction == "fwd"
                         else R.adjoint(c["dy"], c["table"], policy))
    return c["ref"][key]


def run_forward(c, policy):
    from speech_to_image_translation_without_text_amd import ops
    return ops.DiffAugToNHWC.apply(c["xd"], c["td"], policy)


def run_backward(c, policy, dy):
    """dx of the operator through autograd for a contiguous fp32 NHWC gradient dy."""
    from speech_to_image_translation_without_text_amd import ops
    x = c["xd"].clone().requires_grad_(True)
    y = ops.DiffAugToNHWC.apply(x, c["td"], policy)
    dx, = torch.autograd.grad(y, x, dy)
    return dx


def raw_backward(c, policy, rows, ld):
    """s2i_diffaug_backward on the gradient rows `rows` ([N][H][H][ld], fp32 or bf16) as they lie in memory: autograd would
    cast a bf16 gradient of the fp32 output before the operator saw it."""
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    N, H = rows.shape[0], rows.shape[1]
    assert rows.is_contiguous() and rows.shape[3] == ld
    dx = torch.full((N, 3, H, H), float("nan"), device=rows.device)
    ws = torch.empty((lib.s2i_diffaug_workspace_bytes(N, H, H) // 4 + 1,), device=rows.device)
    dt = _lib.DT_BF16 if rows.dtype == torch.bfloat16 else _lib.DT_F32
    _lib.check(lib.s2i_diffaug_backward(dt, rows.data_ptr(), ld, c["td"].data_ptr(), policy, dx.data_ptr(), N, H, H,
                                        ws.data_ptr(), ws.numel() * 4, _lib.stream()), "s2i_diffaug_backward")
    torch.cuda.synchronize()
    return dx


def widened(dy, ld, dtype):
    """dy's four channels in rows of pixel stride ld; the columns behind them hold 7, which no kernel may read into dx."""
    wide = torch.full(tuple(dy.shape[:3]) + (ld,), 7.0, dtype=dtype, device=dy.device)
    wide[..., :4] = dy.to(dtype)
    return wide


SHAPE_IDS = ["N%d_H%d" % s for s in R.SHAPES]


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_policies_without_colour_are_bit_exact(gpu, cases, shape):
    from speech_to_image_translation_without_text_amd import ops
    c = cases[shape]
    N, H = shape
    for policy in PLAIN_POLICIES:
        y = run_forward(c, policy)
        assert y.dtype == torch.float32 and tuple(y.shape) == (N, H, H, 4)
        assert R.same_bits(y.cpu().numpy(), ref_of(c, "fwd", policy)), "forward, policy %d" % policy
        assert not y[..., 3].any() and not torch.signbit(y[..., 3]).any()
        if policy == 0:
            assert torch.equal(y, ops.ToNHWC.apply(c["xd"], 4)), "policy 0 is the plain conversion"
        # the backward is a permutation with zeros: fp32 rows, and bf16 rows with pixel strides 4 and 8
        dx = run_backward(c, policy, c["dyd"])
        assert R.same_bits(dx.cpu().numpy(), ref_of(c, "bwd", policy)), "backward fp32, policy %d" % policy
        d16 = c["dyd"].to(torch.bfloat16)
        ref16 = R.adjoint(d16.float().cpu().numpy(), c["table"], policy)
        for ld in (4, 8):
            dx = raw_backward(c, policy, widened(d16, ld, torch.bfloat16), ld)
            assert R.same_bits(dx.cpu().numpy(), ref16), "backward bf16 ld %d, policy %d" % (ld, policy)
    for mutant in ("translation_sign", "cutout_row_shift", "cutout_before_translation"):
        y = run_forward(c, 6)
        assert not R.same_bits(y.cpu().numpy(), R.forward(c["x"], c["table"], 6, mutant)), mutant


def test_fp32_gradient_rows_with_a_wider_stride(gpu, cases):
    """fp32 dy as a channel slice (pixel stride 8) and as an odd-stride copy (5: the scalar-load path)."""
    c = cases[(3, 8)]
    for ld in (8, 5):
        for policy in (6, 7):
            dx = raw_backward(c, policy, widened(c["dyd"], ld, torch.float32), ld)
            ref = ref_of(c, "bwd", policy)
            if policy == 6:
                assert R.same_bits(dx.cpu().numpy(), ref), ld
            else:
                assert R.within(dx.cpu().numpy(), ref, R.BWD_TOL * float(np.abs(c["dy"]).max())), ld


def test_side_that_is_no_multiple_of_four(gpu):
    """H = 6: the backward writes one pixel per thread instead of four (no 16-byte plane stores), and the cutout side
    c = 3 is odd, so the window has 6 positions per axis and c / 2 rounds down."""
    assert R.geometry(6) == (1, 3, 3, 6)
    x, table, dy = R.make_case(2, 6)
    c = dict(x=x, table=table, dy=dy, xd=torch.from_numpy(x).to(gpu), td=torch.from_numpy(table).to(gpu),
             dyd=torch.from_numpy(dy).to(gpu))
    dmax = float(np.abs(dy).max())
    for policy in R.POLICIES:
        y = run_forward(c, policy).cpu().numpy()
        dx = run_backward(c, policy, c["dyd"]).cpu().numpy()
        d16 = c["dyd"].to(torch.bfloat16)
        dx16 = raw_backward(c, policy, widened(d16, 8, torch.bfloat16), 8).cpu().numpy()
        ref, bref = R.forward(x, table, policy), R.adjoint(dy, table, policy)
        bref16 = R.adjoint(d16.float().cpu().numpy(), table, policy)
        if policy & R.COLOR:
            assert R.within(y, ref, R.FWD_TOL) and R.within(dx, bref, R.BWD_TOL * dmax) and R.within(dx16, bref16, R.BWD_TOL * dmax)
            assert not y[ref == 0.0].any()
        else:
            assert R.same_bits(y, ref) and R.same_bits(dx, bref) and R.same_bits(dx16, bref16), policy
    for mutant in R.MUTANTS:
        if mutant == "adjoint_without_mean":
            assert not R.within(dx, R.adjoint(dy, table, 7, mutant), R.BWD_TOL * dmax), mutant
        else:
            assert not R.within(y, R.forward(x, table, 7, mutant), R.FWD_TOL), mutant


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_policies_with_colour_are_within_the_bound(gpu, cases, shape):
    c = cases[shape]
    dmax = float(np.abs(c["dy"]).max())
    worst_f = worst_b = 0.0
    for policy in COLOUR_POLICIES:
        y = run_forward(c, policy).cpu().numpy()
        ref = ref_of(c, "fwd", policy)
        worst_f = max(worst_f, R.max_err(y, ref))
        assert not y[..., 3].any()
        assert not y[ref == 0.0].any(), "every exact zero of the reference (no source, cut out, channel 3) is an exact zero"
        dx = run_backward(c, policy, c["dyd"]).cpu().numpy()
        bref = ref_of(c, "bwd", policy)
        worst_b = max(worst_b, R.max_err(dx, bref) / dmax)
        print("diffaug N%d H%d policy %d: forward max err %.3e, backward %.3e max|dy|"
              % (shape + (policy, R.max_err(y, ref), R.max_err(dx, bref) / dmax)))
        assert R.within(y, ref, R.FWD_TOL), "forward, policy %d: %.3e" % (policy, R.max_err(y, ref))
        assert R.within(dx, bref, R.BWD_TOL * dmax), "backward, policy %d: %.3e" % (policy, R.max_err(dx, bref))
        if policy == 7:
            for mutant in R.MUTANTS:
                if mutant == "adjoint_without_mean":
                    assert not R.within(dx, R.adjoint(c["dy"], c["table"], 7, mutant), R.BWD_TOL * dmax), mutant
                else:
                    assert not R.within(y, R.forward(c["x"], c["table"], 7, mutant), R.FWD_TOL), mutant
    print("diffaug N%d H%d worst: forward %.3e (bound %.0e), backward %.3e max|dy| (bound %.0e)"
          % (shape + (worst_f, R.FWD_TOL, worst_b, R.BWD_TOL)))
    # bf16 gradient rows under the full policy: the same arithmetic on the rounded gradient
    d16 = c["dyd"].to(torch.bfloat16)
    dx = raw_backward(c, 7, d16.contiguous(), 4).cpu().numpy()
    ref16 = R.adjoint(d16.float().cpu().numpy(), c["table"], 7)
    assert R.within(dx, ref16, R.BWD_TOL * dmax)


def test_same_call_twice_gives_the_same_bits(gpu, cases):
    c = cases[(2, 256)]
    a, b = run_forward(c, 7), run_forward(c, 7)
    assert torch.equal(a, b)
    ga, gb = run_backward(c, 7, c["dyd"]), run_backward(c, 7, c["dyd"])
    assert torch.equal(ga, gb)


def test_backward_kernels_do_not_run_without_a_gradient_for_x(gpu, cases, monkeypatch):
    """Real and wrong images need no gradient: the recorder sees the forward's entry point and never the backward's."""
    from launch_harness import LibRecorder, install
    from speech_to_image_translation_without_text_amd import _lib, ops
    recs = []
    args = {"s2i_diffaug_forward": "x table policy y N H W ws ws_bytes",
            "s2i_diffaug_backward": "dtype dy ld table policy dx N H W ws ws_bytes",
            "s2i_diffaug_workspace_bytes": "N H"}
    proxy = LibRecorder(_lib.load(), recs, args, passed=lambda name: name not in ("s2i_diffaug_forward", "s2i_diffaug_backward"))
    install(monkeypatch, proxy)
    c = cases[(3, 8)]
    w = torch.ones(4, device=gpu, requires_grad=True)
    y = ops.DiffAugToNHWC.apply(c["xd"], c["td"], 7)
    assert not y.requires_grad
    (y * w).sum().backward()                     # a backward pass that reaches the operator's output
    assert c["xd"].grad is None and w.grad is not None
    assert [r["fn"] for r in recs] == ["s2i_diffaug_forward"]
    x = c["xd"].clone().requires_grad_(True)
    (ops.DiffAugToNHWC.apply(x, c["td"], 7) * w).sum().backward()
    assert [r["fn"] for r in recs] == ["s2i_diffaug_forward"] * 2 + ["s2i_diffaug_backward"] and x.grad is not None
    assert recs[-1]["ld"] == 4 and recs[-1]["policy"] == 7 and recs[-1]["N"] == 3


def test_bad_arguments_on_device_pointers(gpu, cases):
    from speech_to_image_translation_without_text_amd import _lib, ops
    c = cases[(3, 8)]
    lib = _lib.load()
    y = torch.empty((3, 8, 8, 4), device=gpu)
    s = _lib.stream()
    assert lib.s2i_diffaug_forward(c["xd"].data_ptr(), c["td"].data_ptr(), 1, y.data_ptr(), 3, 8, 8, None, 0, s) != 0
    assert b"workspace" in lib.s2i_last_error()
    assert lib.s2i_diffaug_forward(c["xd"].data_ptr(), c["td"].data_ptr(), 9, y.data_ptr(), 3, 8, 8, None, 0, s) != 0
    with pytest.raises(_lib.S2IError, match="table"):
        ops.DiffAugToNHWC.apply(c["xd"], c["td"][:2], 7)
    with pytest.raises(_lib.S2IError, match="3-channel"):
        ops.DiffAugToNHWC.apply(torch.zeros(3, 4, 8, 8, device=gpu), c["td"], 7)


# ---- network level --------------------------------------------------------------------------------------------------------
def ref_aug(x, table, policy):
    """The translation and cutout of the operator written with torch indexing (no colour): differentiable, exact zeros."""
    N, _, H, _ = x.shape
    d = R.draws(table.cpu().numpy(), policy, H)
    ar = torch.arange(H, device=x.device)
    out = []
    for n in range(N):
        rs, qs = ar + int(d["ty"][n]), ar + int(d["tx"][n])
        live = ((rs >= 0) & (rs < H))[:, None] & ((qs >= 0) & (qs < H))[None, :]
        cut = (((ar >= int(d["r0"][n])) & (ar < int(d["r1"][n])))[:, None]
               & ((ar >= int(d["q0"][n])) & (ar < int(d["q1"][n])))[None, :])
        moved = x[n].index_select(1, rs.clamp(0, H - 1)).index_select(2, qs.clamp(0, H - 1))
        out.append(torch.where((live & ~cut)[None], moved, torch.zeros((), device=x.device)))
    return torch.stack(out)


@pytest.fixture
def small_d(gpu):
    from speech_to_image_translation_without_text_amd import model, trainer
    from speech_to_image_translation_without_text_amd.miscc.config import cfg_reset
    cfg = configure(CASES["small3"])
    assert cfg.GAN.DF_DIM == 8
    torch.manual_seed(3)
    d = model.D_NET64()
    d.apply(trainer.weights_init)
    for p in d.parameters():
        p.requires_grad_(False)              # only the gradient to the image is taken
    yield d.to(gpu), cfg
    cfg_reset()


def test_discriminator_logits_and_input_gradient_are_bit_identical(gpu, small_d):
    netD, cfg = small_d
    policy = R.TRANSLATION | R.CUTOUT
    g = torch.Generator().manual_seed(11)
    # the stacked pass: 3 groups of B = 8, one table of 24 rows in real | wrong | fake order
    B = 8
    x = (torch.rand(3 * B, 3, 64, 64, generator=g) * 2 - 1).to(gpu)
    mu = torch.randn(B, cfg.GAN.EMBEDDING_DIM, generator=g).to(gpu)
    table = torch.from_numpy(R.make_table(3 * B, 64, 5)).to(gpu)
    state = {k: v.clone() for k, v in netD.state_dict().items()}
    with torch.no_grad():
        got, _ = netD(x, mu.repeat(3, 1), groups=3, need_features=False, aug=(table, policy))
        netD.load_state_dict(state)                  # the BatchNorm running statistics moved: the same start for both
        want, _ = netD(ref_aug(x, table, policy), mu.repeat(3, 1), groups=3, need_features=False)
        netD.load_state_dict(state)
        plain, _ = netD(x, mu.repeat(3, 1), groups=3, need_features=False)
        netD.load_state_dict(state)
    assert len(got) == 2
    for a, b, p in zip(got, want, plain):
        assert torch.equal(a, b) and not torch.equal(a, p)
    # the plain pass at B = 3, with the gradient to the image
    B = 3
    x = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1).to(gpu)
    mu = torch.randn(B, cfg.GAN.EMBEDDING_DIM, generator=g).to(gpu)
    table = torch.from_numpy(R.make_table(B, 64, 6)).to(gpu)
    outs = []
    for use_op in (True, False):
        netD.load_state_dict(state)
        xv = x.clone().requires_grad_(True)
        logits, feats = netD(xv, mu, aug=(table, policy)) if use_op else netD(ref_aug(xv, table, policy), mu)
        loss = logits[0].sum() + 0.5 * logits[1].sum() + feats.square().mean()
        gx, = torch.autograd.grad(loss, xv)
        outs.append((logits, feats, gx))
    netD.load_state_dict(state)
    (la, fa, ga), (lb, fb, gb) = outs
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and torch.equal(fa, fb)
    assert torch.equal(ga, gb) and float(ga.abs().max()) > 0
    d = R.draws(table.cpu().numpy(), policy, 64)
    assert not ga[0, :, :d["ty"][0], :].any(), "rows translated out of the picture receive no gradient"


# ---- trainer level --------------------------------------------------------------------------------------------------------
CASE = dict(CASES["small3"], branch=2, B=8)


def make_loader(seed=2):
    g = torch.Generator().manual_seed(seed)

    def sample():
        imgs = [torch.rand(8, 3, 64 << i, 64 << i, generator=g) * 2 - 1 for i in range(2)]
        wrong = [torch.rand(8, 3, 64 << i, 64 << i, generator=g) * 2 - 1 for i in range(2)]
        return imgs, wrong, torch.randn(8, CASE["t"], generator=g), ["k"] * 8, torch.arange(8) % 3
    return [sample(), sample()]


@pytest.fixture(scope="module")
def loader():
    return make_loader()


@pytest.fixture
def clean_cfg():
    from speech_to_image_translation_without_text_amd.miscc.config import cfg_reset
    yield
    cfg_reset()


def final_state(tr):
    torch.cuda.synchronize()
    out = {}
    for name, f in [("G", tr.flatG)] + [("D%d" % i, f) for i, f in enumerate(tr.flatsD)]:
        for k in ("p", "m", "v", "step_dev"):
            out["%s.%s" % (name, k)] = getattr(f, k).detach().cpu().clone()
        for k, b in f.net.named_buffers():
            out["%s.buffer.%s" % (name, k)] = b.detach().cpu().clone()
    out["G.avg"] = tr.flatG.avg.detach().cpu().clone()
    return out


def first_difference(a, b):
    assert list(a) == list(b)
    for k in a:
        if not torch.equal(a[k], b[k]):
            return k
    return None


def run_gan(out_dir, loader, seed, policy, epochs, state="", state_every=0, stack=True, before=None):
    from speech_to_image_translation_without_text_amd import trainer as T
    cfg = configure(CASE)
    cfg.TRAIN.MAX_EPOCH, cfg.TRAIN.STATE_EVERY, cfg.TRAIN.STATE = epochs, state_every, state
    cfg.TRAIN.SNAPSHOT_INTERVAL, cfg.TRAIN.VIS_COUNT = 1000, 0
    cfg.TRAIN.DIFFAUG = policy
    torch.manual_seed(seed)
    random.seed(seed)
    tr = T.condGANTrainer(out_dir, loader, 256, False)
    tr.stack_d_passes = stack
    if before is not None:
        before(tr)
    tr.train()
    return tr, final_state(tr)


def three_steps(loader):
    return [loader[0], loader[1], loader[0]]


def test_seeded_runs_with_the_policy_agree_and_differ_from_the_run_without(gpu, tmp_path, loader, clean_cfg):
    steps = three_steps(loader)
    full = "color,translation,cutout"
    _, a = run_gan(str(tmp_path / "a"), steps, 0, full, 1)
    _, a2 = run_gan(str(tmp_path / "a2"), steps, 0, full, 1)
    _, off = run_gan(str(tmp_path / "off"), steps, 0, "", 1)
    assert int(a["G.step_dev"]) == 3
    assert first_difference(a, a2) is None, "two seeded runs with the policy differ first at %s" % first_difference(a, a2)
    assert first_difference(a, off) is not None, "the policy must change the run"
    assert not torch.equal(a["D0.p"], off["D0.p"]) and not torch.equal(a["G.p"], off["G.p"])
    # the three un-stacked passes draw from the same tables: the same augmentation, another launch order
    _, u = run_gan(str(tmp_path / "u"), steps, 0, full, 1, stack=False)
    _, u2 = run_gan(str(tmp_path / "u2"), steps, 0, full, 1, stack=False)
    assert first_difference(u, u2) is None


def test_seeded_runs_in_bf16_activation_mode(gpu, tmp_path, loader, clean_cfg, monkeypatch):
    """bf16 activations: the images stay fp32 NHWC4, the gradient that reaches the operator is whatever the first
    convolution's backward hands over.  Same two properties as in fp32."""
    from speech_to_image_translation_without_text_amd import ops
    monkeypatch.setattr(ops, "ACT_BF16", True)
    steps = three_steps(loader)
    _, a = run_gan(str(tmp_path / "a"), steps, 0, "color,translation,cutout", 1)
    _, a2 = run_gan(str(tmp_path / "a2"), steps, 0, "color,translation,cutout", 1)
    _, off = run_gan(str(tmp_path / "off"), steps, 0, "", 1)
    assert first_difference(a, a2) is None, "two seeded bf16 runs with the policy differ first at %s" % first_difference(a, a2)
    assert not torch.equal(a["D0.p"], off["D0.p"]) and not torch.equal(a["G.p"], off["G.p"])
    assert all(bool(torch.isfinite(v).all()) for v in a.values())


def test_resumed_run_with_the_policy_ends_in_the_bits_of_the_straight_run(gpu, tmp_path, loader, clean_cfg):
    import os
    import shutil
    full = "color,translation,cutout"
    copy = str(tmp_path / "state_after_1.pt")

    def keep_epoch_1(tr):
        inner = tr.save_state

        def save_state(path, epoch, count):
            inner(path, epoch, count)
            if epoch == 1:
                shutil.copyfile(path, copy)
        tr.save_state = save_state
    _, a = run_gan(str(tmp_path / "a"), loader, 0, full, 2, state_every=1, before=keep_epoch_1)
    assert os.path.exists(copy) and int(a["G.step_dev"]) == 4
    _, b = run_gan(str(tmp_path / "b"), loader, 123, full, 2, state=copy, state_every=1)
    assert first_difference(a, b) is None, "the resumed run differs first at %s" % first_difference(a, b)
    # under other uniforms the second epoch ends elsewhere: the comparison above can fail
    _, c = run_gan(str(tmp_path / "c"), loader, 123, "cutout", 2, state=copy, state_every=1)
    assert first_difference(a, c) is not None


def test_recorded_step_is_refused_while_the_policy_is_set(gpu, loader, clean_cfg):
    from helpers import build_nets
    from speech_to_image_translation_without_text_amd import _lib, trainer as T
    netG, netsD = build_nets(CASE)
    cfg = configure(CASE)
    tr = T.condGANTrainer(None, None, 256, False)
    tr.build(netG.to(gpu), [d.to(gpu) for d in netsD])
    tr.enable_graph()                          # no policy: allowed, as before
    assert tr._graph is not None
    cfg.TRAIN.DIFFAUG = "color,cutout"
    imgs, wrong, emb, _, labels = loader[0]
    real = [t.to(gpu) for t in imgs]
    wrong = [t.to(gpu) for t in wrong]
    noise = torch.randn(8, cfg.GAN.Z_DIM, device=gpu)
    aug = tr.draw_aug(8, gpu)
    before = final_state(tr)
    with pytest.raises(_lib.S2IError, match="stale uniforms"):
        tr.train_step(real, wrong, emb.to(gpu).requires_grad_(True), labels, noise, aug=aug)
    assert first_difference(before, final_state(tr)) is None, "the refused step changed nothing"
    tr._graph = None
    with pytest.raises(_lib.S2IError, match="DIFFAUG"):
        tr.enable_graph()
    assert tr._graph is None
    tr.train_step(real, wrong, emb.to(gpu).requires_grad_(True), labels, noise, aug=aug)      # the eager step runs
    assert first_difference(before, final_state(tr)) is not None
