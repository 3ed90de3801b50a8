"""The train step's dispatcher launches (ops.conv_any / conv_raw / wgrad_any / wgrad_raw): the recorder that takes their
census and the replay of one record against tests/launch_ref.py in fp64.  tests/test_step_launches_gpu.py documents the
operands, the bound and the power checks and runs them over the train step; tests/test_eval_launches_gpu.py runs
replay_conv over the eval-mode generator.  Each replay notes what it measured in the ledger of the suite that called it."""
import pytest
import torch

import launch_harness as LH
import launch_ref as R

# gamma per (matrix-core operand type, output kind), about 2x the worst ratio measured on one MI355X (the module prints
# them): fp32 forward / input gradient 4.8e-7, fp32 weight gradient 4.0e-7, bf16 forward / input gradient 5.1e-8, bf16
# weight gradient 1.6e-7, BatchNorm partial sums 7.4e-8
GAMMA = {
    "fp32/conv": 2 ** -20,
    "fp32/wgrad": 8e-7,
    "bf16/conv": 1e-7,
    "bf16/wgrad": 3.2e-7,
    # the split-bf16 matrix modes (ops.MATH_PLANES = 3 / 1), worst of the edge replay and the plane probe of
    # tests/test_split_planes_gpu.py: three planes forward / input gradient 4.6e-7, weight gradient 5.0e-7 (both held at the
    # native fp32 constants, which DESIGN.md section 9 claims for them); one plane 3.3e-8 and 9.3e-8
    "split3/conv": 2 ** -20,
    "split3/wgrad": 8e-7,
    "split1/conv": 7e-8,
    "split1/wgrad": 1.9e-7,
}
GAMMA_STATS = 1.5e-7


def _dtname(t):
    return {torch.float32: "f32", torch.bfloat16: "bf16"}[t.dtype]


def _desc(t):
    return [list(t.shape), _dtname(t)]


def wrap_dispatchers(mp, recs):
    """Wrap the dispatchers of ops.py so that every call appends its full argument description to recs."""
    from speech_to_image_translation_without_text_amd import ops
    orig = {k: getattr(ops, k) for k in ("conv_any", "conv_raw", "wgrad_any", "wgrad_raw", "packed_weight", "bf16_weight")}
    fast = [False]

    def packed_weight(w, mode=0):
        p = orig["packed_weight"](w, mode)
        p._census = (list(w.shape), int(mode))
        return p

    def bf16_weight(packed, d, w_offset):
        fast[0] = True
        return orig["bf16_weight"](packed, d, w_offset)

    def wdesc(packed):
        tag = getattr(packed, "_census", None)
        return dict(packed=list(packed.shape), oihw=tag[0] if tag else None, mode=tag[1] if tag else None)

    def conv_any(kind, x, packed, N, *, wmode=0, flip=0, bias=None, act=0, stats=False, groups=1, w_offset=0,
                 cls_bias=None, out_dtype=torch.float32):
        fast[0] = False
        res = orig["conv_any"](kind, x, packed, N, wmode=wmode, flip=flip, bias=bias, act=act, stats=stats, groups=groups,
                               w_offset=w_offset, cls_bias=cls_bias, out_dtype=out_dtype)
        recs.append(dict(fn="conv_any", kind=int(kind), wmode=int(wmode), flip=int(flip), x=_desc(x), w=wdesc(packed),
                         N=int(N), out_dtype=_dtname(res[0]), stats=bool(stats), groups=int(groups),
                         w_offset=int(w_offset), cvec=0, cls_bias=cls_bias is not None,
                         bias=0 if bias is None else int(bias.numel()), act=int(act), fast=fast[0]))
        return res

    def conv_raw(kind, x, cvec, packed, N, *, wmode=0, flip=0, wR, ldw, bias=None, act=0, stats=False, groups=1,
                 w_offset=0, cls_bias=None, conv1d=None, in_src=None):
        assert conv1d is None and in_src is None, "opt-in / encoder launch inside the train step"
        res = orig["conv_raw"](kind, x, cvec, packed, N, wmode=wmode, flip=flip, wR=wR, ldw=ldw, bias=bias, act=act,
                               stats=stats, groups=groups, w_offset=w_offset, cls_bias=cls_bias)
        recs.append(dict(fn="conv_raw", kind=int(kind), wmode=int(wmode), flip=int(flip), x=_desc(x), w=wdesc(packed),
                         N=int(N), out_dtype=_dtname(res[0]), stats=bool(stats), groups=int(groups),
                         w_offset=int(w_offset), cvec=0 if cvec is None else int(cvec.shape[1]),
                         cls_bias=cls_bias is not None, bias=0 if bias is None else int(bias.numel()), act=int(act),
                         wR=int(wR), ldw=int(ldw), fast=False))
        return res

    def wrec(fn, kind, a, cvec, g, grad_shape, swap, fold, out, accumulate, i_off, I_total):
        recs.append(dict(fn=fn, kind=int(kind), a=_desc(a), cvec=0 if cvec is None else int(cvec.shape[1]), g=_desc(g),
                         grad_shape=[int(v) for v in grad_shape], swap=int(swap), fold=int(fold), out=out is not None,
                         accumulate=bool(accumulate), i_off=int(i_off), I_total=int(I_total)))

    def wgrad_any(kind, a, g, grad_shape, *, swap=0, fold=0, out=None, accumulate=False, i_off=0, I_total=0):
        wrec("wgrad_any", kind, a, None, g, grad_shape, swap, fold, out, accumulate, i_off, I_total)
        return orig["wgrad_any"](kind, a, g, grad_shape, swap=swap, fold=fold, out=out, accumulate=accumulate,
                                 i_off=i_off, I_total=I_total)

    def wgrad_raw(kind, a, cvec, g, grad_shape, *, swap=0, fold=0, out=None, accumulate=False, i_off=0, I_total=0,
                  a_src=None):
        assert a_src is None, "apply-on-load launch inside the default train step"
        wrec("wgrad_raw", kind, a, cvec, g, grad_shape, swap, fold, out, accumulate, i_off, I_total)
        return orig["wgrad_raw"](kind, a, cvec, g, grad_shape, swap=swap, fold=fold, out=out, accumulate=accumulate,
                                 i_off=i_off, I_total=I_total)

    for name, fn in (("packed_weight", packed_weight), ("bf16_weight", bf16_weight), ("conv_any", conv_any),
                     ("conv_raw", conv_raw), ("wgrad_any", wgrad_any), ("wgrad_raw", wgrad_raw)):
        mp.setattr(ops, name, fn)


def _operand(desc, gen, dev):
    shape, dt = desc
    t = torch.randn(shape, generator=gen, device=dev)
    return t.to(torch.bfloat16) if dt == "bf16" else t


def _nchw(t):
    return LH.nchw(t.double())


def conv_ref(rec, op, layer, x, cvec, W, Op, table, bias, mutate=False):
    """(pre, y) in fp64 NCHW: pre = convolution (+ class bias), the rows the statistics see; y = act(pre + bias)."""
    B = x.shape[0]
    N = rec["N"]
    if op == "matmul":
        x2 = x.reshape(B, -1).clone()
        if mutate:
            x2[:, -1] = 0
        y = x2 @ W[:N].t() if rec["wmode"] else x2 @ W[:x2.shape[1]]
        pre = y.reshape(B, -1, 1, 1)
    else:
        r0 = rec["w_offset"] // Op
        O = W.shape[0]
        if op == "fwd":
            xin = x if cvec is None else torch.cat((cvec.view(B, -1, 1, 1).expand(-1, -1, x.shape[2], x.shape[3]), x), 1)
            Wu = W[:, r0:r0 + xin.shape[1]]
            xin = xin[:, :Wu.shape[1]].clone()
            if mutate:
                xin[:, -1] = 0
            pre = R.fwd(layer, xin, Wu)
        else:
            dy = x[:, :O].clone()
            if mutate:
                dy[:, -1] = 0
            pre = R.dgrad(layer, dy, W[:, r0:r0 + N])
        pre = R.pad_channels(pre, N)
        if table is not None:
            pre = R.add_class_bias(pre, table)
    y = pre if bias is None else pre + R.pad_channels(bias.view(1, -1, 1, 1), N)
    return pre, y


def randn_weight(shape, gen, dev):
    """N(0, 1) / (k sqrt(I)) weights of an (O, I, k, k) layer: full 24-bit significands, where LH.dyadic fits one bf16."""
    return torch.randn(tuple(shape), generator=gen, device=dev) / (shape[2] * shape[1] ** 0.5)


def replay_conv(rec, gen, dev, what, ledger, extra=None, *, weights="dyadic", operands=None, cls=None):
    """extra(ctx), if given, runs before the assertions with the operands, the output and the bound of this replay
    (tests/test_eval_launches_gpu.py and tests/test_conv_edges_gpu.py add their power checks there) and returns a list of
    failure messages.  Opt-in (tests/test_split_planes_gpu.py): weights = "randn" draws the OIHW weight with randn_weight;
    operands = dict(x=, cvec=) takes these prepared tensors in place of the drawn ones; cls names the class whose GAMMA
    bounds the replay and under which the ledger notes it."""
    from speech_to_image_translation_without_text_amd import ops
    given = operands or {}
    op, layer = R.layer_op(rec)
    x = given["x"] if "x" in given else _operand(rec["x"], gen, dev)
    # an fp32 image operand with a bf16 output (the first discriminator conv, the input gradient of GET_IMAGE_G) runs on
    # the bf16 matrix cores, which read it as bf16: it is drawn on the bf16 grid
    mixed = _dtname(x) != rec["out_dtype"]
    if mixed and x.dtype == torch.float32:
        x = x.bfloat16().float()
    B = x.shape[0]
    wd = rec["w"]
    if wd["oihw"] is None:
        packed = torch.randn(wd["packed"], generator=gen, device=dev)
        W = packed.double()
    else:
        mode = R.pack_mode(op, layer)
        assert mode == wd["mode"], (what, mode, wd)
        w = (LH.dyadic if weights == "dyadic" else randn_weight)(wd["oihw"], gen, dev)
        packed = ops.pack_weight(w, mode)
        assert list(packed.shape) == wd["packed"], (what, list(packed.shape), wd)
        W = w.double()
    N = rec["N"]
    cvec = torch.randn((B, rec["cvec"]), generator=gen, device=dev) if rec["cvec"] else None
    if "cvec" in given:
        cvec = given["cvec"]
    table = torch.randn((B, 9, N), generator=gen, device=dev) if rec["cls_bias"] else None
    bias = torch.randn((rec["bias"],), generator=gen, device=dev) if rec["bias"] else None
    kw = dict(wmode=rec["wmode"], flip=rec["flip"], bias=bias, act=rec["act"], stats=rec["stats"], groups=rec["groups"],
              w_offset=rec["w_offset"], cls_bias=table)
    fast = [False]
    orig_b16 = ops.bf16_weight

    def bf16_weight(packed_, d, w_offset):
        fast[0] = True
        return orig_b16(packed_, d, w_offset)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "bf16_weight", bf16_weight)
        if rec["fn"] == "conv_any":
            y, part, nparts = ops.conv_any(rec["kind"], x, packed, N, out_dtype=getattr(torch, {"f32": "float32",
                                           "bf16": "bfloat16"}[rec["out_dtype"]]), **kw)
        else:
            y, part, nparts = ops.conv_raw(rec["kind"], x, cvec, packed, N, wR=rec["wR"], ldw=rec["ldw"], **kw)
    torch.cuda.synchronize()
    assert fast[0] == rec["fast"], (what, "bf16 fast path taken: %s, census: %s" % (fast[0], rec["fast"]))
    assert _dtname(y) == rec["out_dtype"]
    Op = packed.shape[-1]
    d = lambda t: None if t is None else t.double()
    xd = _nchw(x) if x.dim() == 4 else x.double()
    pre, ref = conv_ref(rec, op, layer, xd, d(cvec), W, Op, d(table), d(bias))
    apre, _ = conv_ref(rec, op, layer, xd.abs(), None if cvec is None else d(cvec).abs(), W.abs(), Op,
                        None if table is None else d(table).abs(), None)
    absref = apre + (0 if bias is None else R.pad_channels(d(bias).abs().view(1, -1, 1, 1), N))
    ref = R.act(ref, rec["act"])
    out = _nchw(y)
    rnd = LH.BF16_ROUND if y.dtype == torch.bfloat16 else 0.0
    cls = cls or ("bf16" if (rec["fast"] or mixed) else "fp32") + "/conv"
    gamma = GAMMA[cls]
    ratio, ok = LH.compare(out, ref, absref, rnd, gamma)
    ledger.note(cls, ratio, what, gamma)
    print("%s: ratio %.3e (gamma %.3e)" % (what, ratio, gamma))
    # power: one input channel's contribution removed
    _, mref = conv_ref(rec, op, layer, xd, d(cvec), W, Op, d(table), d(bias), mutate=True)
    sees_channel = LH.fails(out, R.act(mref, rec["act"]), absref, rnd, gamma)
    stats_ok, stats = True, None
    if rec["stats"]:
        G = max(rec["groups"], 1)
        assert part is not None and nparts % G == 0, (what, nparts, G)
        got = part.double().view(2, G, nparts // G, N).sum(2)
        sref = R.group_stats(pre, G)
        den = torch.stack((R.group_stats(absref, G)[0], 2 * (absref * pre.abs()).reshape(G, B // G, N, -1).sum((1, 3))))
        sratio, stats_ok = LH.compare(got, sref, den, 0.0, GAMMA_STATS)
        stats = dict(got=got, den=den, groups=G)
        ledger.note("stats", sratio, what, GAMMA_STATS)
        print("%s: stats ratio %.3e (gamma %.3e)" % (what, sratio, GAMMA_STATS))
    more = [] if extra is None else extra(dict(rec=rec, op=op, layer=layer, x=xd, cvec=d(cvec), W=W, Op=Op, table=d(table),
                                               bias=d(bias), out=out, ref=ref, absref=absref, rnd=rnd, gamma=gamma,
                                               ratio=ratio, cls=cls, pre=pre, stats=stats))
    assert ok, "%s: element error %.3e x absref > gamma %.3e" % (what, ratio, gamma)
    assert stats_ok, "%s: BatchNorm partial sums off" % what
    assert not more, "%s: %s" % (what, "; ".join(more))
    assert sees_channel, "%s: the bound cannot see one input channel's contribution" % what


def wgrad_family(rec):
    """The family of the kernel plan_wgrad names for this launch under the knobs in force ("f32", "rows3", "b16", "b16d1",
    "split", "smalln"): the first part of its _lib.WGRAD_KERNELS name, asked of s2i_wgrad_plan_query."""
    from speech_to_image_translation_without_text_amd import _lib, ops
    B, H, W, Ca = rec["a"][0]
    N, gs = rec["g"][0][3], rec["grad_shape"]
    O, I, KH, KW = gs if len(gs) == 4 else (gs[0], gs[1], 1, 1)
    d = _lib.WgradDesc(rec["kind"], B, H, W, Ca, rec["cvec"], N, N, rec["swap"], rec["fold"], O, I, KH, KW, int(rec["accumulate"]),
                       rec["i_off"], rec["I_total"], 0, 0)
    a16, g16 = rec["a"][1] == "bf16", rec["g"][1] == "bf16"
    told = _lib.wgrad_plan(d, int(a16), int(g16), 0 if (a16 or g16) else ops.MATH_PLANES)
    assert told is not None, (_lib.load().s2i_last_error(), rec)
    return told["kernel"].split("-")[0]


def wgrad_on_f32(rec):
    """The launch runs on the fp32 matrix cores (f32-*, rows3-*): a bf16 operand is converted up as it is staged, an fp32
    operand is read whole, and the bound is that of the fp32 class whatever the operands' storage."""
    return wgrad_family(rec) in ("f32", "rows3")


def wgrad_dw(rec, layer, ad, gd, cd=None):
    """dw(absval, channel, image, a=, g=): the fp64 weight gradient of record rec from its fp64 NCHW operands ad, gd (and the
    broadcast vector cd), in rec["grad_shape"]; of |a| and |g|; with the last input channel or the last image removed; with
    an operand replaced."""
    gs = rec["grad_shape"]
    O, I = gs[0], gs[1]
    kh = gs[2] if len(gs) == 4 else 1
    B = ad.shape[0]

    def dw(absval=False, channel=False, image=False, a=None, g=None):
        A, G = ad if a is None else a, gd if g is None else g
        if rec["swap"]:
            X, dy = G[:, :I], A[:, :O]
        else:
            X = A if cd is None else torch.cat((cd.view(B, -1, 1, 1).expand(-1, -1, A.shape[2], A.shape[3]), A), 1)
            X, dy = X[:, :I], G[:, :O]
        if absval:
            X, dy = X.abs(), dy.abs()
        if channel or image:
            X = X.clone()
            if channel:
                X[:, -1] = 0
            if image:
                X[-1] = 0
        r = R.wgrad(layer, X, dy, kh)
        return r.view(O, I) if len(gs) == 2 else r
    return dw


def replay_wgrad(rec, gen, dev, what, ledger, extra=None, *, operands=None, cls=None):
    """extra(ctx), if given, runs before the assertions, as in replay_conv, and returns a list of failure messages;
    operands = dict(a=, g=, cvec=) and cls as in replay_conv.  Without cls the class of the bound follows the kernel family
    the plan names: "fp32/wgrad" on f32-* and rows3-*, also where they read a bf16 operand; elsewhere "bf16/wgrad" with a
    bf16 operand (b16-*, b16d1-*, the stream kernels on a bf16 input) and "fp32/wgrad" without."""
    from speech_to_image_translation_without_text_amd import ops
    given = operands or {}
    op, layer = R.layer_op(rec)
    a = given["a"] if "a" in given else _operand(rec["a"], gen, dev)
    g = given["g"] if "g" in given else _operand(rec["g"], gen, dev)
    # one bf16 operand on the bf16 matrix cores (b16d1-64x64: the first discriminator conv's fp32 image x its bf16 output
    # gradient): the kernel reads the fp32 operand as bf16, so that operand is drawn on the bf16 grid.  An f32-* kernel
    # converts the bf16 operand up, and the fp32 one keeps its full significand: a kernel that truncated it would show.
    mixed = a.dtype != g.dtype
    any16 = torch.bfloat16 in (a.dtype, g.dtype)
    on_f32 = wgrad_on_f32(rec)
    if mixed and not on_f32:
        a, g = [t if t.dtype == torch.bfloat16 else t.bfloat16().float() for t in (a, g)]
    B = a.shape[0]
    cvec = torch.randn((B, rec["cvec"]), generator=gen, device=dev) if rec["cvec"] else None
    if "cvec" in given:
        cvec = given["cvec"]
    gs = rec["grad_shape"]
    O, I = gs[0], gs[1]
    kh = gs[2] if len(gs) == 4 else 1
    i_off, I_total = rec["i_off"], rec["I_total"]
    full = list(gs)
    if I_total:
        full[1] = I_total
    prefill = torch.randn(full, generator=gen, device=dev) if rec["out"] else None
    out = None if prefill is None else prefill.clone()
    kw = dict(swap=rec["swap"], fold=rec["fold"], out=out, accumulate=rec["accumulate"], i_off=i_off, I_total=I_total)
    if rec["fn"] == "wgrad_any":
        res = ops.wgrad_any(rec["kind"], a, g, tuple(gs), **kw)
    else:
        res = ops.wgrad_raw(rec["kind"], a, cvec, g, tuple(gs), **kw)
    torch.cuda.synchronize()
    assert out is None or res.data_ptr() == out.data_ptr()
    ad, gd = _nchw(a), _nchw(g)
    cd = None if cvec is None else cvec.double()

    dw = wgrad_dw(rec, layer, ad, gd, cd)
    resd = res.double()
    sl = (slice(None), slice(i_off, i_off + I)) if I_total else (slice(None),)
    got = resd[sl]
    base = prefill.double()[sl] if rec["accumulate"] else 0.0
    true = dw()
    ref = base + true
    absref = dw(absval=True)
    rnd = 2 * LH.U if rec["accumulate"] else 0.0      # the one rounding of prefill + gradient
    cls = cls or ("bf16" if any16 and not on_f32 else "fp32") + "/wgrad"
    gamma = GAMMA[cls]
    ratio, ok = LH.compare(got, ref, absref, rnd, gamma)
    ledger.note(cls, ratio, what, gamma)
    print("%s: ratio %.3e (gamma %.3e)" % (what, ratio, gamma))
    untouched_ok = True
    if I_total and prefill is not None:
        keep = torch.ones(full, dtype=torch.bool, device=dev)
        keep[sl] = False
        untouched_ok = torch.equal(res[keep], prefill[keep])
    sees_channel = LH.fails(got, base + dw(channel=True), absref, rnd, gamma)
    sees_image = LH.fails(got, base + dw(image=True), absref, rnd, gamma)
    more = [] if extra is None else extra(dict(rec=rec, layer=layer, a=ad, g=gd, kh=kh, got=got, base=base, ref=ref, absref=absref,
                                               rnd=rnd, gamma=gamma, ratio=ratio, cls=cls, dw=dw, true=true))
    assert ok, "%s: element error %.3e x absref > gamma %.3e" % (what, ratio, gamma)
    assert not more, "%s: %s" % (what, "; ".join(more))
    assert untouched_ok, "%s: elements outside input channels [%d, %d) changed" % (what, i_off, i_off + I)
    assert sees_channel, "%s: the bound cannot see one input channel's contribution" % what
    assert sees_image, "%s: the bound cannot see one image's contribution" % what
