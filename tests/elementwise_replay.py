"""The non-matrix entry points of the train step (csrc/s2i_bn.hip, s2i_layout.hip, s2i_cvec.hip, s2i_losses.hip,
s2i_optim.hip): their argument lists, the gamma of each
family and the replay of one record against tests/elementwise_ref.py in fp64.  tests/test_step_elementwise_gpu.py documents
the operands, the bound and the mutations and runs the replays over the train step; tests/test_eval_launches_gpu.py runs
them over the eval-mode generator; tests/test_elementwise_edges_gpu.py runs them over the table of tests/elementwise_edges.py
(shapes off the step's) and the B = 23 step.  run() notes what it measured in the ledger of the suite that called it, and
hands every output out between guard margins that Check.done() compares (Ops.full, Ops.guard)."""
import ctypes

import torch

import elementwise_edges as E
import elementwise_ref as R
import launch_harness as LH
from launch_harness import BF16_ROUND, P, call
from speech_to_image_translation_without_text_amd import _lib
from speech_to_image_translation_without_text_amd._lib import ACT_GLU, ACT_LRELU, ACT_TANH, DT_BF16, DT_F32

# argument names of the recorded entry points (include/s2i_hip.h order, the trailing stream left out); a pointer is
# recorded as whether it is non-NULL, a scalar by value; workspaces and their sizes are not recorded
ARGS = {
    "s2i_bn_finalize": "part nparts groups C count gamma beta running_mean running_var nbt momentum eps out",
    "s2i_bn_bwd_finalize": "part nparts groups C count dgamma dbeta accumulate red2",
    "s2i_bn_act_forward_dt": "dtype y M groups C coef act residual out",
    "s2i_bn_act_bwd_reduce_dt": "dtype y dout lddout M groups C coef act part nparts",
    "s2i_bn_act_bwd_apply_dt": "dtype y dout lddout M groups C coef red2 act dy",
    "s2i_act_backward_dt": "dtype out dout lddout M C act dy",
    "s2i_colstats": "y M C ldy part nparts",
    "s2i_axpby": "y x n a b",
    "s2i_spatial_sum_dt": "dtype src ld B HW C dst ws ws_bytes",
    "s2i_tap_sums_dt": "dtype dy B H W C tapsum ws ws_bytes",
    "s2i_cvec_bias_table": "cvec packed B Cc Ip Op N table ws ws_bytes",
    "s2i_cvec_grads": "cvec packed tapsum B Cc Ip Op N O I_total dc dw accumulate",
    "s2i_glu_forward": "x M C out",
    "s2i_glu_backward": "x dout M C dx",
    "s2i_reparam_forward": "h eps B E c",
    "s2i_reparam_backward": "h eps dc dmu dlogvar B E dh",
    "s2i_kl_forward": "mu ldmu logvar ldlv B E kl",
    "s2i_kl_backward": "mu ldmu logvar ldlv B E gout dmu dlogvar",
    "s2i_logit_forward": "x w bias B C prob",
    "s2i_logit_backward": "x w prob dprob B C dx acc_dx dw dbias acc_dw",
    "s2i_bce_forward": "prob target B weight loss accumulate",
    "s2i_bce_backward": "prob target B weight gout dprob",
    "s2i_bce_multi_forward": "probs target weight G H B loss",
    "s2i_bce_multi_backward": "probs target weight G H B gout dprobs",
    "s2i_cal_loss": "scores labels B D loss accumulate dscores",
    "s2i_scale_dev": "y x n a",
    "s2i_adam_step": "p g m v n lr beta1 beta2 eps step step_dev gscale",
    "s2i_increment": "counter",
    "s2i_ema_update": "avg p n decay",
    "s2i_nchw_to_nhwc_dt": "dtype src dst B C H W Cp",
    "s2i_nhwc_to_nchw_dt": "dtype src lds dst B C H W",
    "s2i_cast": "src src_dtype dst dst_dtype n",
}
NOT_RECORDED = ("ws", "ws_bytes")

# gamma per family, about 2x the worst ratio measured on one MI355X (census and edge cases together)
GAMMA = {
    "bn_finalize": 5.5e-7,      # worst 2.7e-7 (running_mean after three group updates)
    "bn_bwd_finalize": 1.3e-7,  # 6.2e-8
    "bn_forward": 1.7e-7,       # 8.2e-8
    "bn_reduce": 4.2e-7,        # 2.1e-7
    "bn_apply": 4e-7,           # 2.0e-7
    "bn_chain": 2.5e-7,         # 1.2e-7
    "act_backward": 1.8e-7,     # 8.9e-8
    "colstats": 3.4e-7,         # 1.7e-7
    "axpby": 1.2e-7,            # 5.9e-8
    "spatial_sum": 2.2e-7,      # 1.1e-7
    # of the image's total |dy|.  1.5e-8 on the step's 64 x 64 and 128 x 128 maps, where that total is ~60 x the result;
    # 1.6e-7 = 2.7 x 2^-24 on the 4 x 4 map of tests/elementwise_edges.py (C = 1028: one lane adds all 16 pixels, then
    # total - row - column + corner: at most 18 roundings of 2^-24 of the total each)
    "tap_sums": 3.2e-7,
    "cvec_table": 1e-7,         # 4.9e-8
    "cvec_grads": 6.6e-7,       # 3.3e-7
    "ca_net": 3e-7,             # 1.4e-7
    "logit": 4.2e-7,            # 2.1e-7
    "bce": 3.3e-7,              # 1.6e-7
    "cal_loss": 7.5e-8,         # 3.6e-8
    "adam": 4e-7,               # 2.0e-7
    "ema": 2.4e-7,              # 1.2e-7
    "scale_dev": 1.2e-7,        # 6.0e-8
}


def is_matrix(name):
    """Entry points the non-matrix replay sets aside.  The s2i_pack* launches among them are held, bit for bit, by
    tests/test_weight_pack_gpu.py."""
    return (name.startswith("s2i_conv_") or name.startswith("s2i_pack") or name == "s2i_split_packed_weight"
            or "workspace_bytes" in name or name.endswith("_eligible") or "_stat_parts" in name or "_weight_" in name
            or name in ("s2i_check_device", "s2i_last_error"))


# ---- operands ----------------------------------------------------------------------------------------------------------
def tdt(code):
    return {DT_F32: torch.float32, DT_BF16: torch.bfloat16}[code]


class Ops:
    """Operands of one replay.  Outputs (full, guard) are views into a buffer with LH.GUARD_BYTES of a fixed bit pattern on
    both sides; with a Check given, its done() asserts that both margins are still bit-identical."""

    def __init__(self, gen, dev, chk=None):
        self.gen, self.dev, self.chk = gen, dev, chk

    def randn(self, shape, dtype=torch.float32, scale=1.0):
        t = torch.randn(tuple(shape), generator=self.gen, device=self.dev) * scale
        return t.to(dtype)

    def rand(self, shape, lo=0.0, hi=1.0):
        return lo + (hi - lo) * torch.rand(tuple(shape), generator=self.gen, device=self.dev)

    def randint(self, lo, hi, shape):
        return torch.randint(lo, hi, tuple(shape), generator=self.gen, device=self.dev)

    def grid(self, shape, dtype):
        """Activations on the bf16 grid (stored as `dtype`): scale * y + shift is then exact in fp32."""
        return self.randn(shape).to(torch.bfloat16).to(dtype)

    def coef(self, G, C):
        """[G][4][C]: mean, invstd (any), scale = +-k / 16 (some negative), shift = j / 32; independent per group."""
        mean = self.randn((G, C), scale=0.5)
        invstd = self.rand((G, C), 0.5, 2.0)
        sc = self.randint(1, 17, (G, C)).float() / 16 * (self.randint(0, 2, (G, C)).float() * 2 - 1)
        sh = self.randint(-32, 33, (G, C)).float() / 32
        return torch.stack((mean, invstd, sc, sh), 1).contiguous()

    def _guarded(self, shape, dtype):
        n = torch.empty((), dtype=dtype).element_size()
        for d in shape:
            n *= d
        buf = torch.full((n + 2 * LH.GUARD_BYTES,), LH.GUARD_BYTE, dtype=torch.uint8, device=self.dev)
        if self.chk is not None:
            self.chk.watch(buf, LH.GUARD_BYTES, n)
        return buf[LH.GUARD_BYTES:LH.GUARD_BYTES + n].view(dtype).view(tuple(shape))

    def full(self, shape, dtype=torch.float32, value=float("nan")):
        return self._guarded(tuple(shape), dtype).fill_(value)

    def guard(self, t):
        """A copy of t between guard margins, for a buffer the launch updates in place (None stays None)."""
        return None if t is None else self._guarded(t.shape, t.dtype).copy_(t)


def swap_halves(t):
    h = t.shape[-1] // 2
    return torch.cat((t[..., h:], t[..., :h]), -1)


def drop_last_row(ref, G=1):
    """The same reference with each group's last row zeroed (a dropped row chunk)."""
    m = ref.clone()
    v = m.reshape(G, -1, *m.shape[1:]) if m.dim() > 1 else m.view(G, -1)
    v[:, -1] = 0
    return m


def _drop_last_segment(v, B, n, S):
    """v [B * n][...] with the rows of each image's last non-empty segment (E.segments(n, S)) zeroed."""
    r0, r1 = [seg for seg in E.segments(n, S)[1] if seg[1] > seg[0]][-1]
    m = v.clone(memory_format=torch.contiguous_format)
    m.view(B, n, -1)[:, r0:r1] = 0
    return m


def _drop_last_part(part, G):
    m = part.clone()
    m.view(2, G, -1, part.shape[-1])[:, :, -1] = 0
    return m


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------
def _abs_parts(y, dout, G, coef, act):
    """|operand| forms of dz and xhat: [G][Rg][C] each."""
    C = y.shape[-1]
    Y = R._rows(y, G)
    zabs = Y.abs() * coef[:, 2:3].abs() + coef[:, 3:4].abs()
    xh = (Y.abs() + coef[:, 0:1].abs()) * coef[:, 1:2].abs()
    cout = C // 2 if act == ACT_GLU else C
    d = R._rows(dout[:, :cout], G).abs()
    if act == ACT_GLU:
        h = C // 2
        mag = 1 + zabs[..., h:]                # sigmoid and its derivative, and their sensitivity to the gate
        dz = torch.cat((d * mag, d * zabs[..., :h] * mag), -1)
    else:
        dz = d
    return dz, xh, zabs


def _mut_dz_on_y(y, dout, G, coef):
    """LeakyReLU decided on y instead of scale * y + shift."""
    return torch.where(R._rows(y, G) > 0, R._rows(dout[:, :y.shape[-1]], G), R.SLOPE * R._rows(dout[:, :y.shape[-1]], G))


def _bn_operands(rec, o):
    dt = tdt(rec["dtype"])
    M, G, C = rec["M"], rec["groups"], rec["C"]
    y = o.grid((M, C), dt)
    coef = o.coef(G, C)
    return dt, M, G, C, y, coef


def replay_bn_act_forward(rec, o, chk):
    dt, M, G, C, y, coef = _bn_operands(rec, o)
    act = rec["act"]
    cout = C // 2 if act == ACT_GLU else C
    res = o.randn((M, C), dt) if rec["residual"] else None
    out = o.full((M, cout), dt)
    call("s2i_bn_act_forward_dt", rec["dtype"], P(y), M, G, C, P(coef), act, P(res), P(out))
    yd, cd = y.double(), coef.double()
    rd = None if res is None else res.double()
    ref = R.bn_act_forward(yd, G, cd, act, rd)
    _, _, zabs = _abs_parts(yd, yd, G, cd, act)
    if act == ACT_GLU:
        h = C // 2
        absref = (zabs[..., :h] * (1 + zabs[..., h:])).reshape(M, cout)
    else:
        absref = zabs.reshape(M, C) + (0 if rd is None else rd.abs())
    mut = {"last row of each group missing": drop_last_row(ref, G)}
    if G > 1:
        mut["every group with group 0's coefficients"] = R.bn_act_forward(yd, G, cd[:1].expand(G, 4, C), act, rd)
    if act == ACT_GLU:
        mut["GLU value and gate halves swapped"] = R.bn_act_forward(swap_halves(yd), G, swap_halves(cd), act)
    if act == ACT_LRELU:
        z = R.pre_act(yd, cd, G)
        m = torch.where(R._rows(yd, G) > 0, z, R.SLOPE * z).reshape(M, C)
        mut["LeakyReLU decided on y"] = m if rd is None else m + rd
    chk.close("bn_forward", "out", out, ref, absref, BF16_ROUND if dt == torch.bfloat16 else 0.0, mut)


def _dout(rec, o, dt, M):
    return o.randn((M, rec["lddout"]), dt)


def replay_bn_act_bwd_reduce(rec, o, chk):
    dt, M, G, C, y, coef = _bn_operands(rec, o)
    act, nparts = rec["act"], rec["nparts"]
    dout = _dout(rec, o, dt, M)
    part = o.full((2, nparts, C))
    call("s2i_bn_act_bwd_reduce_dt", rec["dtype"], P(y), P(dout), rec["lddout"], M, G, C, P(coef), act, P(part), nparts)
    yd, dd, cd = y.double(), dout.double(), coef.double()
    ref = R.bn_act_bwd_reduce(yd, dd, G, cd, act, nparts)
    dza, xha, _ = _abs_parts(yd, dd, G, cd, act)
    absref = torch.stack((R.chunk_sums(dza, nparts // G), R.chunk_sums(dza * xha, nparts // G)))
    mut = {"each group missing its last row chunk": _drop_last_part(ref, G)}
    if G > 1:
        mut["every group with group 0's coefficients"] = R.bn_act_bwd_reduce(yd, dd, G, cd[:1].expand(G, 4, C), act, nparts)
    if act == ACT_GLU:
        mut["GLU value and gate halves swapped"] = R.bn_act_bwd_reduce(swap_halves(yd), dd, G, swap_halves(cd), act,
                                                                       nparts)
    if act == ACT_LRELU:
        dz = _mut_dz_on_y(yd, dd, G, cd)
        mut["LeakyReLU decided on y"] = torch.stack((R.chunk_sums(dz, nparts // G),
                                                     R.chunk_sums(dz * R.xhat(yd, cd, G), nparts // G)))
    chk.close("bn_reduce", "part", part, ref, absref, 0.0, mut)


def replay_bn_act_bwd_apply(rec, o, chk):
    dt, M, G, C, y, coef = _bn_operands(rec, o)
    act = rec["act"]
    dout = _dout(rec, o, dt, M)
    red2 = o.randn((G, 2, C), scale=0.3)
    dy = o.full((M, C), dt)
    call("s2i_bn_act_bwd_apply_dt", rec["dtype"], P(y), P(dout), rec["lddout"], M, G, C, P(coef), P(red2), act, P(dy))
    yd, dd, cd, r2 = y.double(), dout.double(), coef.double(), red2.double()
    ref = R.bn_act_bwd_apply(yd, dd, G, cd, r2, act)
    dza, xha, _ = _abs_parts(yd, dd, G, cd, act)
    absref = (cd[:, 2:3].abs() * (dza + r2[:, 0:1].abs() + xha * r2[:, 1:2].abs())).reshape(M, C)
    mut = {"each group missing its last row": drop_last_row(ref, G)}
    if G > 1:
        mut["every group with group 0's coefficients"] = R.bn_act_bwd_apply(yd, dd, G, cd[:1].expand(G, 4, C),
                                                                            r2[:1].expand(G, 2, C), act)
    if act == ACT_GLU:
        mut["GLU value and gate halves swapped"] = R.bn_act_bwd_apply(swap_halves(yd), dd, G, swap_halves(cd),
                                                                      swap_halves(r2), act)
    if act == ACT_LRELU:
        dz = _mut_dz_on_y(yd, dd, G, cd)
        m = cd[:, 2:3] * (dz - r2[:, 0:1] - R.xhat(yd, cd, G) * r2[:, 1:2])
        mut["LeakyReLU decided on y"] = m.reshape(M, C)
    chk.close("bn_apply", "dy", dy, ref, absref, BF16_ROUND if dt == torch.bfloat16 else 0.0, mut)


def run_bn_chain(rec, o, chk):
    """reduce -> bwd_finalize -> apply of one recorded reduce launch, against the fp64 backward of the whole chain."""
    dt, M, G, C, y, coef = _bn_operands(rec, o)
    act, nparts, ldd = rec["act"], rec["nparts"], rec["lddout"]
    dout = _dout(rec, o, dt, M)
    part = o.full((2, nparts, C))
    red2 = o.full((G, 2, C))
    dg, db = o.full((C,)), o.full((C,))
    dy = o.full((M, C), dt)
    call("s2i_bn_act_bwd_reduce_dt", rec["dtype"], P(y), P(dout), ldd, M, G, C, P(coef), act, P(part), nparts)
    call("s2i_bn_bwd_finalize", P(part), nparts, G, C, M // G, P(dg), P(db), 0, P(red2))
    call("s2i_bn_act_bwd_apply_dt", rec["dtype"], P(y), P(dout), ldd, M, G, C, P(coef), P(red2), act, P(dy))
    yd, dd, cd = y.double(), dout.double(), coef.double()
    dz = R.dz_of(yd, dd, G, cd, act)
    xh = R.xhat(yd, cd, G)
    m0, m1 = dz.mean(1, keepdim=True), (dz * xh).mean(1, keepdim=True)
    ref = (cd[:, 2:3] * (dz - m0 - xh * m1)).reshape(M, C)
    dza, xha, _ = _abs_parts(yd, dd, G, cd, act)
    absref = (cd[:, 2:3].abs() * (dza + dza.mean(1, keepdim=True) + xha * (dza * xha).mean(1, keepdim=True))).reshape(M, C)
    chk.close("bn_chain", "dy", dy, ref, absref, BF16_ROUND if dt == torch.bfloat16 else 0.0,
              {"each group missing its last row": drop_last_row(ref, G)})
    chk.close("bn_chain", "dgamma", dg, (dz * xh).sum((0, 1)), (dza * xha).sum((0, 1)))
    chk.close("bn_chain", "dbeta", db, dz.sum((0, 1)), dza.sum((0, 1)))


def _finalize_partials(o, G, C, nparts, count):
    """Partial sums of G groups with means ~N(0,1) and variances in [0.5, 2]: [2][nparts][C] fp32."""
    ppg = nparts // G
    mu = o.randn((G, 1, C))
    var = o.rand((G, 1, C), 0.5, 2.0)
    n = count / ppg
    p0 = n * mu * (1 + 0.01 * o.randn((G, ppg, C)))
    p1 = n * (var + mu * mu) * (1 + 0.01 * o.randn((G, ppg, C)))
    return torch.stack((p0.reshape(nparts, C), p1.reshape(nparts, C))).contiguous()


def replay_bn_finalize(rec, o, chk):
    G, C, nparts, count = rec["groups"], rec["C"], rec["nparts"], rec["count"]
    mom, eps = rec["momentum"], rec["eps"]
    part = _finalize_partials(o, G, C, nparts, count)
    gamma, beta = o.randn((C,)), o.randn((C,))
    rm0 = o.randn((C,)) if rec["running_mean"] else None
    rv0 = o.rand((C,), 0.0, 0.05) if rec["running_var"] else None      # small: the update dominates running_var
    rm, rv = (None, None) if rm0 is None else (rm0.clone(), rv0.clone())
    nbt = torch.tensor([5], dtype=torch.int64, device=o.dev) if rec["nbt"] else None
    out = o.full((G, 4, C))
    call("s2i_bn_finalize", P(part), nparts, G, C, count, P(gamma), P(beta), P(rm), P(rv), P(nbt), mom, eps, P(out))
    pd, gd, bd = part.double(), gamma.double(), beta.double()
    d = lambda t: None if t is None else t.double()
    coef, rmr, rvr, _ = R.bn_finalize(pd, G, count, gd, bd, d(rm0), d(rv0), None, mom, eps)
    mean, invstd, sc = coef[:, 0], coef[:, 1], coef[:, 2]
    cabs = torch.stack((mean.abs(), invstd, sc.abs(), bd.abs() + (mean * sc).abs()), 1)
    mut = {"each group missing its last row chunk": R.bn_finalize(_drop_last_part(pd, G), G, count, gd, bd)[0]}
    if G > 1:
        p0 = pd.view(2, G, -1, C)[:, :1].expand(2, G, nparts // G, C).reshape(2, nparts, C)
        mut["every group with group 0's statistics"] = R.bn_finalize(p0, G, count, gd, bd)[0]
    chk.close("bn_finalize", "coef", out, coef, cabs, 0.0, mut)
    if rm0 is not None:
        am, av = rm0.double().abs(), rv0.double()
        unb = (coef[:, 1] ** -2 - eps) * count / (count - 1)
        for g in range(G):
            am = (1 - mom) * am + mom * mean[g].abs()
            av = (1 - mom) * av + mom * unb[g].abs()
        chk.close("bn_finalize", "running_mean", rm, rmr, am)
        biased = R.bn_finalize(pd, G, count, gd, bd, d(rm0), d(rv0), None, mom, eps, biased_running=True)[2]
        # the unbiased factor count / (count - 1) moves running_var by about 1 / count of itself: visible in fp32 while
        # that exceeds the bound (count < ~1e6); the larger counts of the step are below fp32 resolution there
        mut = {"biased var in the running var": biased} if 1.0 / (count - 1) > 2 * GAMMA["bn_finalize"] else {}
        chk.close("bn_finalize", "running_var", rv, rvr, av, 0.0, mut)
    if nbt is not None:
        chk.equal("num_batches_tracked", nbt, torch.tensor([5 + G], dtype=torch.int64, device=o.dev))


def replay_bn_bwd_finalize(rec, o, chk):
    G, C, nparts, count, acc = rec["groups"], rec["C"], rec["nparts"], rec["count"], rec["accumulate"]
    part = o.randn((2, nparts, C))
    dg0 = o.randn((C,)) if rec["dgamma"] else None
    db0 = o.randn((C,)) if rec["dbeta"] else None
    dg = None if dg0 is None else dg0.clone()
    db = None if db0 is None else db0.clone()
    red2 = o.full((G, 2, C))
    call("s2i_bn_bwd_finalize", P(part), nparts, G, C, count, P(dg), P(db), acc, P(red2))
    pd = part.double()
    d = lambda t: None if t is None else t.double()
    r2, dgr, dbr = R.bn_bwd_finalize(pd, G, count, d(dg0), d(db0), acc)
    a2, dga, dba = R.bn_bwd_finalize(pd.abs(), G, count, None if dg0 is None else d(dg0).abs(),
                                     None if db0 is None else d(db0).abs(), acc)
    mpart = _drop_last_part(pd, G)
    chk.close("bn_bwd_finalize", "red2", red2, r2, a2, 0.0,
              {"each group missing its last row chunk": R.bn_bwd_finalize(mpart, G, count)[0]})
    for name, got, ref, ab, pre in (("dgamma", dg, dgr, dga, dg0), ("dbeta", db, dbr, dba, db0)):
        if got is None:
            continue
        k = 1 if name == "dgamma" else 2
        mut = {"each group missing its last row chunk": R.bn_bwd_finalize(mpart, G, count, d(dg0), d(db0), acc)[k]}
        if acc:
            mut["accumulate treated as assign"] = R.bn_bwd_finalize(pd, G, count)[k]
        chk.close("bn_bwd_finalize", name, got, ref, ab, 0.0, mut)


def replay_act_backward(rec, o, chk):
    dt = tdt(rec["dtype"])
    M, C, act, ldd = rec["M"], rec["C"], rec["act"], rec["lddout"]
    out = o.randn((M, C), dt) if act == ACT_LRELU else torch.tanh(o.randn((M, C))).to(dt)
    dout = o.randn((M, ldd), dt)
    dy = o.full((M, C), dt)
    call("s2i_act_backward_dt", rec["dtype"], P(out), P(dout), ldd, M, C, act, P(dy))
    od, dd = out.double(), dout.double()[:, :C]
    ref = R.act_backward(od, dd, act)
    absref = dd.abs() * (1 + od * od) if act == ACT_TANH else dd.abs()
    mut = {"last row missing": drop_last_row(ref)}
    if act == ACT_LRELU:
        mut["slope decided on dout"] = torch.where(dd > 0, dd, R.SLOPE * dd)
    chk.close("act_backward", "dy", dy, ref, absref, BF16_ROUND if dt == torch.bfloat16 else 0.0, mut)


# ---- sums ------------------------------------------------------------------------------------------------------------
def replay_colstats(rec, o, chk):
    M, C, ldy, nparts = rec["M"], rec["C"], rec["ldy"], rec["nparts"]
    y = o.randn((M, ldy))
    part = o.full((2, nparts, C))
    call("s2i_colstats", P(y), M, C, ldy, P(part), nparts)
    yd = y.double()[:, :C]
    chk.close("colstats", "part", part, R.colstats(yd, nparts), R.colstats(yd.abs(), nparts), 0.0,
              {"last row missing": R.colstats(drop_last_row(yd), nparts),
               "last row chunk left out": R.colstats(_drop_last_segment(yd, 1, M, nparts), nparts)})


def replay_axpby(rec, o, chk):
    n, a, b = rec["n"], rec["a"], rec["b"]
    x = o.randn((n,))
    y0 = o.randn((n,)) if b != 0 else o.full((n,))
    y = o.guard(y0)
    call("s2i_axpby", P(y), P(x), n, a, b)
    xd, yd = x.double(), y0.double()
    ref = R.axpby(yd, xd, a, b)
    absref = abs(a) * xd.abs() + (abs(b) * yd.abs() if b != 0 else 0)
    mut = {"last element missing": drop_last_row(ref)}
    if b != 0:
        mut["accumulate treated as assign"] = R.axpby(yd, xd, a, 0.0)
    chk.close("axpby", "y", y, ref, absref, 0.0, mut)


def replay_spatial_sum(rec, o, chk):
    dt = tdt(rec["dtype"])
    B, HW, C, ld = rec["B"], rec["HW"], rec["C"], rec["ld"]
    src = o.randn((B * HW, ld), dt)
    dst = o.full((B, C))
    lib = _lib.load()
    ws = o.full((lib.s2i_spatial_sum_workspace_bytes(B, HW, C) // 4,))      # exactly what the library asks for
    call("s2i_spatial_sum_dt", rec["dtype"], P(src), ld, B, HW, C, P(dst), P(ws), ws.numel() * 4)
    sd = src.double()
    chk.close("spatial_sum", "dst", dst, R.spatial_sum(sd, B, C), R.spatial_sum(sd.abs(), B, C), 0.0,
              {"last row of each image missing": R.spatial_sum(drop_last_row(sd, B), B, C),
               "last segment of each image left out": R.spatial_sum(_drop_last_segment(sd, B, HW, E.spatial_segments(HW)),
                                                                    B, C)})


def replay_tap_sums(rec, o, chk):
    dt = tdt(rec["dtype"])
    B, H, W, C = rec["B"], rec["H"], rec["W"], rec["C"]
    dy = o.randn((B, H, W, C), dt)
    out = o.full((B, 9, C))
    lib = _lib.load()
    ws = o.full((lib.s2i_border_sums_workspace_bytes(B, H, W, C) // 4,))    # exactly what the library asks for
    call("s2i_tap_sums_dt", rec["dtype"], P(dy), B, H, W, C, P(out), P(ws), ws.numel() * 4)
    dd = dy.double()
    # inclusion and exclusion from the image total: the error scales with the total of |dy|
    absref = dd.abs().sum((1, 2)).unsqueeze(1).expand(B, 9, C)
    band = _drop_last_segment(dd.reshape(B * H, W * C), B, H, E.border_segments(H)).view(B, H, W, C)
    mut = {"top and bottom border classes swapped": R.tap_sums(dd, swap_top_bottom=True),
           "last row band of each image left out": R.tap_sums(band)}
    if H != W:
        mut["H and W exchanged"] = R.tap_sums(dd.reshape(B, W, H, C))      # the same buffer read as W rows of H pixels
    chk.close("tap_sums", "tapsum", out, R.tap_sums(dd), absref, 0.0, mut)


def replay_cvec_bias_table(rec, o, chk):
    B, Cc, Ip, Op, N = rec["B"], rec["Cc"], rec["Ip"], rec["Op"], rec["N"]
    cvec = o.randn((B, Cc))
    packed = o.randn((9, Ip, Op), scale=0.1)
    table = o.full((B, 9, N))
    ws = o.full((B * 9 * N,))                                               # exactly what the entry point requires
    call("s2i_cvec_bias_table", P(cvec), P(packed), B, Cc, Ip, Op, N, P(table), P(ws), ws.numel() * 4)
    cd, pd = cvec.double(), packed.double()
    ref = R.cvec_bias_table(cd, pd, Cc, N)
    # the table of a map whose H and W are exchanged: row class and column class change places
    mut = {"top and bottom border classes swapped": R.cvec_bias_table(cd, pd, Cc, N, swap_top_bottom=True),
           "H and W exchanged": ref.view(B, 3, 3, N).transpose(1, 2).reshape(B, 9, N)}
    if Cc % 4:
        mc = cd.clone()
        mc[:, Cc - Cc % 4:] = 0
        mut["last Cc % 4 channels left out"] = R.cvec_bias_table(mc, pd, Cc, N)
    chk.close("cvec_table", "table", table, ref, R.cvec_bias_table(cd.abs(), pd.abs(), Cc, N), 0.0, mut)


def replay_cvec_grads(rec, o, chk):
    B, Cc, Ip, Op, N, O, It, acc = (rec[k] for k in ("B", "Cc", "Ip", "Op", "N", "O", "I_total", "accumulate"))
    cvec = o.randn((B, Cc))
    packed = o.randn((9, Ip, Op), scale=0.1)
    tapsum = o.randn((B, 9, N), scale=8.0)
    dc = o.full((B, Cc)) if rec["dc"] else None
    dw0 = o.randn((O, It, 3, 3)) if rec["dw"] else None
    dw = o.guard(dw0)
    call("s2i_cvec_grads", P(cvec), P(packed), P(tapsum), B, Cc, Ip, Op, N, O, It, P(dc), P(dw), acc)
    cd, pd, td = cvec.double(), packed.double(), tapsum.double()
    if dc is not None:
        mt = td.clone()
        mt[:, 8] = 0
        ref = R.cvec_dc(pd, td, Cc, N)
        mut = {"last tap missing": R.cvec_dc(pd, mt, Cc, N)}
        if Cc > 64:
            mut["channels from 64 on left out"] = torch.cat((ref[:, :64], torch.zeros_like(ref[:, 64:])), 1)
        chk.close("cvec_grads", "dc", dc, ref, R.cvec_dc(pd.abs(), td.abs(), Cc, N), 0.0, mut)
    if dw is not None:
        base = dw0.double()[:, :Cc] if acc else 0
        ref = base + R.cvec_dw(cd, td, O)
        absref = R.cvec_dw(cd.abs(), td.abs(), O) + (dw0.double()[:, :Cc].abs() if acc else 0)
        mc = cd.clone()
        mc[-1] = 0
        mut = {"last image missing": base + R.cvec_dw(mc, td, O)}
        if acc:
            mut["accumulate treated as assign"] = R.cvec_dw(cd, td, O)
        chk.close("cvec_grads", "dw[:, :Cc]", dw[:, :Cc], ref, absref, 0.0, mut)
        chk.equal("dw[:, Cc:] (not written)", dw[:, Cc:], dw0[:, Cc:])


# ---- CA_NET, heads, losses ---------------------------------------------------------------------------------------------
def replay_glu_forward(rec, o, chk):
    M, C = rec["M"], rec["C"]
    x = o.randn((M, C))
    out = o.full((M, C // 2))
    call("s2i_glu_forward", P(x), M, C, P(out))
    xd = x.double()
    h = C // 2
    chk.close("ca_net", "glu", out, R.glu(xd), xd[:, :h].abs() * (1 + xd[:, h:].abs()), 0.0,
              {"GLU value and gate halves swapped": R.glu(swap_halves(xd))})


def replay_glu_backward(rec, o, chk):
    M, C = rec["M"], rec["C"]
    x, dout = o.randn((M, C)), o.randn((M, C // 2))
    dx = o.full((M, C))
    call("s2i_glu_backward", P(x), P(dout), M, C, P(dx))
    xd, dd = x.double(), dout.double()
    h = C // 2
    mag = 1 + xd[:, h:].abs()
    absref = torch.cat((dd.abs() * mag, dd.abs() * xd[:, :h].abs() * mag), 1)
    chk.close("ca_net", "glu dx", dx, R.glu_backward(xd, dd), absref, 0.0,
              {"GLU value and gate halves swapped": swap_halves(R.glu_backward(swap_halves(xd), dd))})


def replay_reparam_forward(rec, o, chk):
    B, E = rec["B"], rec["E"]
    h, eps = o.randn((B, 2 * E)), o.randn((B, E))
    c = o.full((B, E))
    call("s2i_reparam_forward", P(h), P(eps), B, E, P(c))
    hd, ed = h.double(), eps.double()
    ref = R.reparam_forward(hd, ed)
    absref = ed.abs() * torch.exp(0.5 * hd[:, E:]) * (1 + hd[:, E:].abs()) + hd[:, :E].abs()
    chk.close("ca_net", "c", c, ref, absref, 0.0, {"last row missing": drop_last_row(ref)})


def replay_reparam_backward(rec, o, chk):
    B, E = rec["B"], rec["E"]
    h, eps = o.randn((B, 2 * E)), o.randn((B, E))
    dc = o.randn((B, E)) if rec["dc"] else None
    dmu = o.randn((B, E)) if rec["dmu"] else None
    dlv = o.randn((B, E)) if rec["dlogvar"] else None
    dh = o.full((B, 2 * E))
    call("s2i_reparam_backward", P(h), P(eps), P(dc), P(dmu), P(dlv), B, E, P(dh))
    hd, ed = h.double(), eps.double()
    cd = torch.zeros_like(ed) if dc is None else dc.double()       # a NULL dc is a zero gradient
    ref = R.reparam_backward(hd, ed, cd)
    ex = torch.exp(0.5 * hd[:, E:])
    absref = torch.cat((cd.abs(), cd.abs() * ed.abs() * 0.5 * ex * (1 + hd[:, E:].abs())), 1)
    if dmu is not None:
        ref[:, :E] += dmu.double()
        absref[:, :E] += dmu.double().abs()
    if dlv is not None:
        ref[:, E:] += dlv.double()
        absref[:, E:] += dlv.double().abs()
    chk.close("ca_net", "dh", dh, ref, absref, 0.0, {"last row missing": drop_last_row(ref)})


def _kl_operands(rec, o):
    B, E = rec["B"], rec["E"]
    mu_buf, lv_buf = o.randn((B, rec["ldmu"])), o.randn((B, rec["ldlv"]), scale=0.5)
    return B, E, mu_buf, lv_buf, mu_buf.double()[:, :E], lv_buf.double()[:, :E]


def replay_kl_forward(rec, o, chk):
    B, E, mb, lb, mu, lv = _kl_operands(rec, o)
    kl = o.full(())
    call("s2i_kl_forward", P(mb), rec["ldmu"], P(lb), rec["ldlv"], B, E, P(kl))
    ref = R.kl_forward(mu, lv)
    absref = 0.5 * torch.mean(1 + lv.abs() + mu * mu + torch.exp(lv) * (1 + lv.abs()))
    mut = {"last row missing": R.kl_forward(drop_last_row(mu), lv)}
    if B * E > 256:
        terms = (1 + lv - mu * mu - torch.exp(lv)).reshape(-1)
        mut["items from 256 on left out"] = -0.5 * terms[:256].sum() / (B * E)
    chk.close("ca_net", "kl", kl, ref, absref, 0.0, mut)


def replay_kl_backward(rec, o, chk):
    B, E, mb, lb, mu, lv = _kl_operands(rec, o)
    gout = o.randn((1,))
    dmu, dlv = o.full((B, E)), o.full((B, E))
    call("s2i_kl_backward", P(mb), rec["ldmu"], P(lb), rec["ldlv"], B, E, P(gout), P(dmu), P(dlv))
    g = float(gout)
    rmu, rlv = R.kl_backward(mu, lv, g)
    s = abs(g) * 0.5 / (B * E)
    chk.close("ca_net", "kl dmu", dmu, rmu, s * 2 * mu.abs(), 0.0, {"last row missing": drop_last_row(rmu)})
    chk.close("ca_net", "kl dlogvar", dlv, rlv, s * (1 + torch.exp(lv) * (1 + lv.abs())), 0.0,
              {"last row missing": drop_last_row(rlv)})


def replay_logit_forward(rec, o, chk):
    B, C = rec["B"], rec["C"]
    x, w = o.randn((B, 4, 4, C)), o.randn((1, C, 4, 4), scale=0.05)
    bias = o.randn((1,)) if rec["bias"] else None
    prob = o.full((B,))
    call("s2i_logit_forward", P(x), P(w), P(bias), B, C, P(prob))
    xd, wd = x.double(), w.double()
    bd = None if bias is None else bias.double()
    ref = R.logit_forward(xd, wd, bd)
    zabs = torch.einsum("bhwc,chw->b", xd.abs(), wd[0].abs()) + (0 if bd is None else bd.abs())
    mw = wd.clone()
    mw[:, -1] = 0
    chk.close("logit", "prob", prob, ref, ref * (1 - ref) * zabs + ref, 0.0,
              {"last channel missing": R.logit_forward(xd, mw, bd)})


def replay_logit_backward(rec, o, chk):
    B, C = rec["B"], rec["C"]
    x, w = o.randn((B, 4, 4, C)), o.randn((1, C, 4, 4), scale=0.05)
    prob, dprob = o.rand((B,), 0.05, 0.95), o.randn((B,))
    dx0 = o.randn((B, 4, 4, C)) if rec["dx"] else None
    dw0 = o.randn((1, C, 4, 4)) if rec["dw"] else None
    db0 = o.randn((1,)) if rec["dbias"] else None
    pre = lambda t, acc: None if t is None else o.guard(t if acc else torch.full_like(t, float("nan")))
    dx, dw, db = pre(dx0, rec["acc_dx"]), pre(dw0, rec["acc_dw"]), pre(db0, rec["acc_dw"])
    call("s2i_logit_backward", P(x), P(w), P(prob), P(dprob), B, C, P(dx), rec["acc_dx"], P(dw), P(db), rec["acc_dw"])
    xd, wd, pd, gd = x.double(), w.double(), prob.double(), dprob.double()
    dl, rdx, rdw, rdb = R.logit_backward(xd, wd, pd, gd)
    adl, adx, adw, adb = R.logit_backward(xd.abs(), wd.abs(), pd, gd.abs())
    mx = xd.clone()
    mx[-1] = 0
    for name, got, ref, ab, pre, acc, k in (("dx", dx, rdx, adx, dx0, rec["acc_dx"], 1), ("dw", dw, rdw, adw, dw0, rec["acc_dw"], 2),
                                            ("dbias", db, rdb, adb, db0, rec["acc_dw"], 3)):
        if got is None:
            continue
        base = pre.double() if acc else 0
        if k == 1:
            mut = {"last image missing": drop_last_row(base + ref)}
        elif k == 2:
            mut = {"last image missing": base + R.logit_backward(mx, wd, pd, gd)[2]}
        else:
            mut = {"last image missing": base + dl[:-1].sum().view(1)}
        if acc:
            mut["accumulate treated as assign"] = ref
        if B > 256:
            if k == 1:
                m = ref.clone()
                m[256:] = 0
            else:
                m = R.logit_backward(xd[:256], wd, pd[:256], gd[:256])[k]
            mut["images from 256 on left out"] = base + m
        chk.close("logit", name, got, base + ref, ab + (pre.double().abs() if acc else 0), 0.0, mut)


def _probs(o, n):
    """Probabilities in [0.02, 0.98] with exact 0 and 1 at two places (torch's log clamp at -100)."""
    p = o.rand((n,), 0.02, 0.98)
    if n >= 4:
        p[1], p[2] = 0.0, 1.0
    else:                         # what fits: 1 at the end, 0 at the start (n = 1: the 0)
        p[-1] = 1.0
        p[0] = 0.0
    return p


def _bce_abs(p, t):
    lp = torch.log(p).clamp_min(R.LOG_CLAMP).abs()
    lq = torch.log(1 - p).clamp_min(R.LOG_CLAMP).abs()
    return t.abs() * lp + (1 - t).abs() * lq + 1       # + 1: the absolute error of a log near 1


def replay_bce_forward(rec, o, chk):
    B, t, wgt, acc = rec["B"], rec["target"], rec["weight"], rec["accumulate"]
    prob = _probs(o, B)
    loss0 = o.randn(())
    loss = o.guard(loss0) if acc else o.full(())
    call("s2i_bce_forward", P(prob), t, B, wgt, P(loss), acc)
    pd = prob.double()
    base = loss0.double() if acc else 0
    ref = base + R.bce_forward(pd, t, wgt)
    absref = abs(wgt) * _bce_abs(pd, torch.tensor(t, dtype=torch.float64)).mean() + (loss0.double().abs() if acc else 0)
    mut = {"last element missing": base + wgt * R.bce_terms(pd[:-1], t).sum() / B}
    if B > 256:
        mut["items from 256 on left out"] = base + wgt * R.bce_terms(pd[:256], t).sum() / B
    chk.close("bce", "loss", loss, ref, absref, 0.0, mut)


def replay_bce_backward(rec, o, chk):
    B, t, wgt = rec["B"], rec["target"], rec["weight"]
    prob, gout = _probs(o, B), o.randn((1,))
    dprob = o.full((B,))
    call("s2i_bce_backward", P(prob), t, B, wgt, P(gout), P(dprob))
    ref = R.bce_backward(prob.double(), t, wgt, float(gout))
    chk.close("bce", "dprob", dprob, ref, ref.abs(), 0.0, {"last element missing": drop_last_row(ref)})


def _bce_multi_operands(rec, o):
    G, H, B = rec["G"], rec["H"], rec["B"]
    probs = [_probs(o, G * B) for _ in range(H)]
    target = (o.randint(0, 2, (G * H,)).float())
    target[-1] = 0.0
    target[0] = 1.0
    weight = 0.5 + 0.37 * ((5 * torch.arange(G * H, device=o.dev)) % (G * H)).float()     # distinct, shuffled
    arr = (ctypes.c_void_p * H)(*[P(p) for p in probs])
    wmut = weight.double().clone()
    if G * H > 1:
        wmut[0], wmut[1] = weight[1].double(), weight[0].double()
        return G, H, B, probs, target, weight, arr, ("two terms' weights swapped", wmut)
    return G, H, B, probs, target, weight, arr, ("the one term's weight taken as 1", torch.ones_like(wmut))


def replay_bce_multi_forward(rec, o, chk):
    G, H, B, probs, target, weight, arr, (mname, wmut) = _bce_multi_operands(rec, o)
    loss = o.full(())
    call("s2i_bce_multi_forward", arr, P(target), P(weight), G, H, B, P(loss))
    pd = [p.double() for p in probs]
    td, wd = target.double(), weight.double()
    ref = R.bce_multi_forward(pd, td, wd, G, B)
    absref = 0
    for g in range(G):
        for h in range(H):
            absref = absref + wd[g * H + h] * _bce_abs(pd[h][g * B:(g + 1) * B], td[g * H + h]).mean()
    mut = {mname: R.bce_multi_forward(pd, td, wmut, G, B)}
    if G * H * B > 256:
        # the kernel's item e = (g H + h) B + b
        flat = torch.stack([wd[g * H + h] * R.bce_terms(pd[h][g * B:(g + 1) * B], td[g * H + h])
                            for g in range(G) for h in range(H)]).reshape(-1)
        mut["items from 256 on left out"] = flat[:256].sum() / B
    chk.close("bce", "multi loss", loss, ref, absref, 0.0, mut)


def replay_bce_multi_backward(rec, o, chk):
    G, H, B, probs, target, weight, arr, (mname, wmut) = _bce_multi_operands(rec, o)
    gout = o.randn((1,))
    grads = [o.full((G * B,)) for _ in range(H)]
    parr = (ctypes.c_void_p * H)(*[P(t) for t in grads])
    call("s2i_bce_multi_backward", arr, P(target), P(weight), G, H, B, P(gout), parr)
    pd = [p.double() for p in probs]
    td, wd = target.double(), weight.double()
    ref = torch.cat(R.bce_multi_backward(pd, td, wd, G, B, float(gout)))
    mref = torch.cat(R.bce_multi_backward(pd, td, wmut, G, B, float(gout)))
    chk.close("bce", "multi dprobs", torch.cat(grads), ref, ref.abs(), 0.0, {mname: mref})


def replay_cal_loss(rec, o, chk):
    B, D, acc = rec["B"], rec["D"], rec["accumulate"]
    X = o.randn((B, D)).double()
    S = (X @ X.t()).float()
    labels = o.randint(0, max(2, B // 4), (B,)).int()
    if B == 2:
        labels = torch.zeros_like(labels)          # the only draw with a same-label pair
    same = (labels.view(-1, 1) == labels.view(1, -1)) & ~torch.eye(B, dtype=torch.bool, device=o.dev)
    n = int(same.sum())
    diff = S.double().mean() - S.double()[same].sum() / max(n, 1)
    if n and diff <= 0:
        # a draw that leaves the loss inactive (small D: the diagonal no longer dominates): lower the same-label scores by
        # c, which raises diff by c (1 - n / B^2), to half the mean |score|
        c = (0.5 * S.double().abs().mean() - diff) / (1 - n / (B * B))
        S = (S.double() - c * same).float()
    loss0 = o.randn((1,))
    loss = o.guard(loss0) if acc else o.full((1,))
    dS = o.full((B, B)) if rec["dscores"] else None
    call("s2i_cal_loss", P(S), P(labels), B, D, P(loss), acc, P(dS))
    Sd = S.double()
    lref, dref = R.cal_loss(Sd, labels, D)
    base = loss0.double() if acc else 0
    labs = (Sd.abs().mean() + Sd.abs()[same].sum() / max(n, 1)) / D
    assert float(lref) > 0, "cal_loss operands leave the loss inactive"
    ml, md = R.cal_loss(Sd, labels, D, count_diagonal=True)
    mut = {"diagonal pairs counted": base + ml.view(1)}
    if B * B > 256:
        # the sums over S, the pairs and their count stop at item 256 (the divisor B * B is a launch constant)
        flat, fsame = Sd.reshape(-1)[:256], same.reshape(-1)[:256]
        diff = flat.sum() / (B * B) - flat[fsame].sum() / max(int(fsame.sum()), 1)
        mut["items from 256 on left out"] = base + (diff.clamp_min(0) / D).view(1)
    chk.close("cal_loss", "loss", loss, base + lref.view(1), labs + (loss0.double().abs() if acc else 0), 0.0, mut)
    if dS is not None:
        chk.close("cal_loss", "dS", dS, dref, torch.full_like(dref, 2 * (1.0 / (B * B) + 1.0 / n) / D), 0.0,
                  {"diagonal pairs counted": md})


def replay_scale_dev(rec, o, chk):
    n = rec["n"]
    x0, a = o.randn((n,)), o.randn((1,))
    x = o.guard(x0)
    call("s2i_scale_dev", P(x), P(x), n, P(a))          # in place, as ClassAwareLoss.backward runs it
    ref = R.scale_dev(x0.double(), float(a))
    chk.close("scale_dev", "y", x, ref, ref.abs(), 0.0, {"last element missing": drop_last_row(ref)})


def _f32(v):
    return float(ctypes.c_float(v).value)


def run_adam(o, chk, n, lr, b1, b2, eps, step, use_dev, gscale):
    lr, b1, b2, eps, gscale = (_f32(v) for v in (lr, b1, b2, eps, gscale))     # what the kernel receives
    p, g = o.randn((n,)), o.randn((n,), scale=1e-2)
    m, v = o.randn((n,), scale=1e-2), o.rand((n,), 0.0, 1e-4)
    p0, m0, v0 = p, m, v
    p, m, v = o.guard(p0), o.guard(m0), o.guard(v0)
    t = 3 if use_dev else step
    sd = torch.tensor([t], dtype=torch.int32, device=o.dev) if use_dev else None
    call("s2i_adam_step", P(p), P(g), P(m), P(v), n, lr, b1, b2, eps, 0 if use_dev else step, P(sd), gscale)
    pd, gd, md, vd = p0.double(), g.double(), m0.double(), v0.double()
    rp, rm, rv = R.adam_step(pd, gd, md, vd, lr, b1, b2, eps, t, gscale)
    am = b1 * md.abs() + (1 - b1) * (gd * gscale).abs()
    av = b2 * vd + (1 - b2) * (gd * gscale) ** 2
    upd = (lr / (1 - b1 ** t)) * rm.abs() / (torch.sqrt(rv) / (1 - b2 ** t) ** 0.5 + eps)
    off = R.adam_step(pd, gd, md, vd, lr, b1, b2, eps, t + 1, gscale)[0]
    chk.close("adam", "p", p, rp, pd.abs() + upd, 0.0, {"bias correction one step off": off})
    chk.close("adam", "m", m, rm, am, 0.0, {"last element missing": drop_last_row(rm)})
    chk.close("adam", "v", v, rv, av, 0.0, {"last element missing": drop_last_row(rv)})
    if sd is not None:
        chk.equal("step_dev (read only)", sd, torch.tensor([t], dtype=torch.int32, device=o.dev))


def replay_adam_step(rec, o, chk):
    run_adam(o, chk, rec["n"], rec["lr"], rec["beta1"], rec["beta2"], rec["eps"], rec["step"], rec["step_dev"],
             rec["gscale"])


def replay_ema_update(rec, o, chk):
    n, dec = rec["n"], rec["decay"]
    a0, p = o.randn((n,)), o.randn((n,))
    avg = o.guard(a0)
    call("s2i_ema_update", P(avg), P(p), n, dec)
    ad, pd = a0.double(), p.double()
    chk.close("ema", "avg", avg, R.ema_update(ad, pd, dec), dec * ad.abs() + (1 - dec) * pd.abs(), 0.0,
              {"decay and 1 - decay swapped": R.ema_update(ad, pd, 1 - dec)})


def replay_increment(rec, o, chk):
    c = torch.tensor([7], dtype=torch.int32, device=o.dev)
    call("s2i_increment", P(c))
    chk.equal("counter", c, torch.tensor([8], dtype=torch.int32, device=o.dev))


def replay_nchw_to_nhwc(rec, o, chk):
    dt = tdt(rec["dtype"])
    B, C, H, W, Cp = rec["B"], rec["C"], rec["H"], rec["W"], rec["Cp"]
    src = o.randn((B, C, H, W))
    dst = o.full((B, H, W, Cp), dt)
    call("s2i_nchw_to_nhwc_dt", rec["dtype"], P(src), P(dst), B, C, H, W, Cp)
    chk.equal("nhwc (round to nearest even, zero pad channels)", dst, R.nchw_to_nhwc(src, Cp).to(dt))
    # torch.equal takes -0 for +0: the pad channels as integers
    pad = dst[..., C:].contiguous().view(torch.int32 if dt == torch.float32 else torch.int16)
    chk.equal("nhwc pad channels (+0 bit patterns)", pad, torch.zeros_like(pad))


def replay_nhwc_to_nchw(rec, o, chk):
    dt = tdt(rec["dtype"])
    B, C, H, W, lds = rec["B"], rec["C"], rec["H"], rec["W"], rec["lds"]
    src = o.randn((B * H * W, lds), dt)
    dst = o.full((B, C, H, W))
    call("s2i_nhwc_to_nchw_dt", rec["dtype"], P(src), lds, P(dst), B, C, H, W)
    chk.equal("nchw", dst, R.nhwc_to_nchw(src.float(), B, C, H, W))


def replay_cast(rec, o, chk):
    sdt, ddt, n = tdt(rec["src_dtype"]), tdt(rec["dst_dtype"]), rec["n"]
    src = o.randn((n,), scale=3.0)
    if sdt == torch.float32 and n >= 8:
        # exact ties of the bf16 rounding (round half to even) and values that round up into the next binade
        src[:6] = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 2 - 2 ** -9, 3.0e38, -1.0e-30], device=o.dev)
    src = src.to(sdt)
    dst = o.full((n,), ddt)
    call("s2i_cast", P(src), rec["src_dtype"], P(dst), rec["dst_dtype"], n)
    chk.equal("cast", dst, R.cast(src, ddt))


REPLAY = {
    "s2i_bn_finalize": replay_bn_finalize,
    "s2i_bn_bwd_finalize": replay_bn_bwd_finalize,
    "s2i_bn_act_forward_dt": replay_bn_act_forward,
    "s2i_bn_act_bwd_reduce_dt": replay_bn_act_bwd_reduce,
    "s2i_bn_act_bwd_apply_dt": replay_bn_act_bwd_apply,
    "s2i_act_backward_dt": replay_act_backward,
    "s2i_colstats": replay_colstats,
    "s2i_axpby": replay_axpby,
    "s2i_spatial_sum_dt": replay_spatial_sum,
    "s2i_tap_sums_dt": replay_tap_sums,
    "s2i_cvec_bias_table": replay_cvec_bias_table,
    "s2i_cvec_grads": replay_cvec_grads,
    "s2i_glu_forward": replay_glu_forward,
    "s2i_glu_backward": replay_glu_backward,
    "s2i_reparam_forward": replay_reparam_forward,
    "s2i_reparam_backward": replay_reparam_backward,
    "s2i_kl_forward": replay_kl_forward,
    "s2i_kl_backward": replay_kl_backward,
    "s2i_logit_forward": replay_logit_forward,
    "s2i_logit_backward": replay_logit_backward,
    "s2i_bce_forward": replay_bce_forward,
    "s2i_bce_backward": replay_bce_backward,
    "s2i_bce_multi_forward": replay_bce_multi_forward,
    "s2i_bce_multi_backward": replay_bce_multi_backward,
    "s2i_cal_loss": replay_cal_loss,
    "s2i_scale_dev": replay_scale_dev,
    "s2i_adam_step": replay_adam_step,
    "s2i_ema_update": replay_ema_update,
    "s2i_increment": replay_increment,
    "s2i_nchw_to_nhwc_dt": replay_nchw_to_nhwc,
    "s2i_nhwc_to_nchw_dt": replay_nhwc_to_nchw,
    "s2i_cast": replay_cast,
}


def run(rec, what, ledger, fn=None):
    """Replay one record (through fn, or the replay of its entry point) on operands seeded by the record."""
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0, "the replay runs the default planner"
    dev = torch.device("cuda:0")
    chk = LH.Check(what, GAMMA, ledger)
    with torch.no_grad():
        (fn or REPLAY[rec["fn"]])(rec, Ops(LH.gen_rec(dev, rec), dev, chk), chk)
    torch.cuda.empty_cache()
    chk.done()
