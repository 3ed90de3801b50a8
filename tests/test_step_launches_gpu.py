"""Every convolution launch of the train step, at its production shape, against a plain fp64 reference.

The kernels' variants (fp32 96 / 128-row tiles and split-K, weight-gradient tile shapes, the bf16 load-aware K split,
the persistent 256-pixel kernel, XCD remapping, BatchNorm partial sums per group) are chosen by the C planners from the
launch's shape, so they are tested here at the shapes the step really launches, with the default planner:

  * census: one eager train_step of each BASELINE workload (config 2: fp32, batch 24; config 4: bf16 activations,
    batch 48) with the four dispatchers of ops.py wrapped; each call's full argument description, deduplicated, is
    tests/step_launches.json.  test_census_matches_committed_file fails on any new or vanished launch, so a new shape
    shows up as a diff of that file.  Regenerate it with `python tests/test_step_launches_gpu.py`.
  * replay: every census entry re-run through the same dispatcher on fresh seeded operands.  Weights are integers in
    [-16, 16] times 2^-6, so their bf16 rounding and the up-block's 4-tap fold sums are exact; bf16 activations are
    drawn as bf16.  The reference (tests/launch_ref.py) sees exactly the values the kernel sees.
  * bound, element-wise: |out - ref| <= rnd * |ref| + gamma * absref, rnd = 2^-8 for a bf16 output and 0 for fp32,
    absref = the same operation on |operands| in fp64, gamma one constant per (matrix-core type, forward | weight
    gradient), at about 2x the worst ratio measured.  BatchNorm partial sums (summed per group) and accumulation into a
    prefilled gradient (the written slice = prefill + gradient, every other element bit-identical) are checked too.
  * power: the same comparison must FAIL against a reference with one input channel's contribution removed (a dropped
    K chunk) and, for weight gradients, one image's contribution removed (a dropped pixel-range split).
"""
import json
import os
import sys
import time
import zlib

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import launch_ref as R  # noqa: E402
from helpers import CASES, build_nets, make_batch  # noqa: E402

pytestmark = pytest.mark.gpu

CENSUS_FILE = os.path.join(HERE, "step_launches.json")

# mode name -> (case, bf16 activations): BASELINE configs 2 and 4
MODES = {
    "fp32_b24": (dict(CASES["full3_fwd"], B=24), False),
    "bf16_b48": (dict(CASES["full3_fwd"], B=48), True),
}

# gamma per (matrix-core operand type, output kind), about 2x the worst ratio measured on one MI355X (the module prints
# them): fp32 forward / input gradient 4.8e-7, fp32 weight gradient 4.0e-7, bf16 forward / input gradient 5.1e-8, bf16
# weight gradient 1.6e-7, BatchNorm partial sums 7.4e-8
GAMMA = {
    "fp32/conv": 2 ** -20,
    "fp32/wgrad": 8e-7,
    "bf16/conv": 1e-7,
    "bf16/wgrad": 3.2e-7,
}
GAMMA_STATS = 1.5e-7
BF16_ROUND = 2.0 ** -8       # round to nearest bf16 (8 significant bits): |rounded - v| <= 2^-8 |v|
FP32_ROUND = 2.0 ** -24

_WORST = {}


def _dtname(t):
    return {torch.float32: "f32", torch.bfloat16: "bf16"}[t.dtype]


def _desc(t):
    return [list(t.shape), _dtname(t)]


# ---- census ----------------------------------------------------------------------------------------------------------
def wrap_dispatchers(mp, recs):
    """Wrap the dispatchers of ops.py so that every call appends its full argument description to recs (also used by
    tests/test_eval_launches_gpu.py for the eval-mode generator)."""
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


def _record_step(gpu, case, bf16, mp):
    """One eager train_step (the pattern of test_bf16_gpu._run_steps) with the dispatchers wrapped -> list of records."""
    from speech_to_image_translation_without_text_amd import ops, trainer as T
    recs = []
    wrap_dispatchers(mp, recs)
    mp.setattr(ops, "ACT_BF16", bf16)
    netG, netsD = build_nets(case)
    batch = make_batch(case)
    netG.to(gpu)
    for d in netsD:
        d.to(gpu)
    tr = T.condGANTrainer(None, None, 256, False)
    tr.build(netG, netsD)
    b = {k: ([t.to(gpu) for t in v] if isinstance(v, list) and torch.is_tensor(v[0]) else
             (v.to(gpu) if torch.is_tensor(v) else v)) for k, v in batch.items()}
    emb = b["emb"].clone().requires_grad_(True)
    tr.train_step(b["real"], b["wrong"], emb, batch["labels"], b["noise"], b["eps"])
    torch.cuda.synchronize()
    return recs


def _canon(rec):
    return json.dumps(rec, sort_keys=True)


def take_census(gpu):
    """{mode: deduplicated, sorted list of launch records}, and {mode: launches per step}."""
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0 and not ops.DEFER_ACT, "census needs the default paths"
    out, calls = {}, {}
    for mode, (case, bf16) in MODES.items():
        with pytest.MonkeyPatch.context() as mp:
            recs = _record_step(gpu, case, bf16, mp)
        calls[mode] = len(recs)
        out[mode] = [json.loads(s) for s in sorted({_canon(r) for r in recs})]
        torch.cuda.empty_cache()
    return out, calls


def _load_census():
    if not os.path.exists(CENSUS_FILE):
        return {}
    with open(CENSUS_FILE) as fp:
        return json.load(fp)


def test_census_matches_committed_file(gpu):
    live, calls = take_census(gpu)
    for mode, recs in live.items():
        print("census %s: %d dispatcher calls per step, %d distinct launches" % (mode, calls[mode], len(recs)))
    committed = _load_census()
    for mode in MODES:
        have = {_canon(r) for r in committed.get(mode, [])}
        now = {_canon(r) for r in live[mode]}
        assert now == have, "%s: launches not in tests/step_launches.json: %s; listed but not launched: %s" % (
            mode, sorted(now - have)[:5], sorted(have - now)[:5])


# ---- replay ----------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for mode, recs in _load_census().items():
        for i, rec in enumerate(recs):
            op, layer = R.layer_op(rec)
            out.append(pytest.param(mode, i, id="%s-%03d-%s-%s-%s" % (mode, i, rec["fn"], op, layer)))
    return out


def _operand(desc, gen, dev):
    shape, dt = desc
    t = torch.randn(shape, generator=gen, device=dev)
    return t.to(torch.bfloat16) if dt == "bf16" else t


def _dyadic(shape, gen, dev):
    return torch.randint(-16, 17, tuple(shape), generator=gen, device=dev).float() * 2.0 ** -6


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _compare(out, ref, absref, rnd, gamma):
    """(ratio, ok): ratio = max (|out - ref| - rnd |ref|) / absref, the gamma this element needs."""
    err = (out - ref).abs() - rnd * ref.abs()
    ratio = float((err / absref.clamp_min(1e-300)).clamp_min(0).max()) if err.numel() else 0.0
    return ratio, bool((err <= gamma * absref).all())


def _fails(out, mref, absref, rnd, gamma):
    return not _compare(out, mref, absref, rnd, gamma)[1]


def _note(cls, ratio, what):
    if ratio > _WORST.get(cls, (0.0, ""))[0]:
        _WORST[cls] = (ratio, what)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print("\nstep launch replay: worst measured ratio per bound (gamma in use), %.0f s" % (time.time() - t0))
    for cls in sorted(_WORST):
        g = GAMMA_STATS if cls == "stats" else GAMMA[cls]
        print("  %-18s %.3e  (gamma %.3e)  %s" % (cls, _WORST[cls][0], g, _WORST[cls][1]))


def _conv_ref(rec, op, layer, x, cvec, W, Op, table, bias, mutate=False):
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


def _replay_conv(rec, gen, dev, what, extra=None):
    """extra(ctx), if given, runs before the assertions with the operands, the output and the bound of this replay
    (tests/test_eval_launches_gpu.py adds its power checks there) and returns a list of failure messages."""
    from speech_to_image_translation_without_text_amd import ops
    op, layer = R.layer_op(rec)
    x = _operand(rec["x"], gen, dev)
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
        w = _dyadic(wd["oihw"], gen, dev)
        packed = ops.pack_weight(w, mode)
        assert list(packed.shape) == wd["packed"], (what, list(packed.shape), wd)
        W = w.double()
    N = rec["N"]
    cvec = torch.randn((B, rec["cvec"]), generator=gen, device=dev) if rec["cvec"] else None
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
    pre, ref = _conv_ref(rec, op, layer, xd, d(cvec), W, Op, d(table), d(bias))
    apre, _ = _conv_ref(rec, op, layer, xd.abs(), None if cvec is None else d(cvec).abs(), W.abs(), Op,
                        None if table is None else d(table).abs(), None)
    absref = apre + (0 if bias is None else R.pad_channels(d(bias).abs().view(1, -1, 1, 1), N))
    ref = R.act(ref, rec["act"])
    out = _nchw(y)
    rnd = BF16_ROUND if y.dtype == torch.bfloat16 else 0.0
    cls = ("bf16" if (rec["fast"] or mixed) else "fp32") + "/conv"
    gamma = GAMMA[cls]
    ratio, ok = _compare(out, ref, absref, rnd, gamma)
    _note(cls, ratio, what)
    print("%s: ratio %.3e (gamma %.3e)" % (what, ratio, gamma))
    # power: one input channel's contribution removed
    _, mref = _conv_ref(rec, op, layer, xd, d(cvec), W, Op, d(table), d(bias), mutate=True)
    sees_channel = _fails(out, R.act(mref, rec["act"]), absref, rnd, gamma)
    stats_ok = True
    if rec["stats"]:
        G = max(rec["groups"], 1)
        assert part is not None and nparts % G == 0, (what, nparts, G)
        got = part.double().view(2, G, nparts // G, N).sum(2)
        sref = R.group_stats(pre, G)
        den = torch.stack((R.group_stats(absref, G)[0], 2 * (absref * pre.abs()).reshape(G, B // G, N, -1).sum((1, 3))))
        sratio, stats_ok = _compare(got, sref, den, 0.0, GAMMA_STATS)
        _note("stats", sratio, what)
        print("%s: stats ratio %.3e (gamma %.3e)" % (what, sratio, GAMMA_STATS))
    more = [] if extra is None else extra(dict(rec=rec, op=op, layer=layer, x=xd, cvec=d(cvec), W=W, Op=Op, table=d(table),
                                               bias=d(bias), out=out, ref=ref, absref=absref, rnd=rnd, gamma=gamma,
                                               ratio=ratio, cls=cls))
    assert ok, "%s: element error %.3e x absref > gamma %.3e" % (what, ratio, gamma)
    assert stats_ok, "%s: BatchNorm partial sums off" % what
    assert not more, "%s: %s" % (what, "; ".join(more))
    assert sees_channel, "%s: the bound cannot see one input channel's contribution" % what


def _replay_wgrad(rec, gen, dev, what):
    from speech_to_image_translation_without_text_amd import ops
    op, layer = R.layer_op(rec)
    a = _operand(rec["a"], gen, dev)
    g = _operand(rec["g"], gen, dev)
    # one bf16 operand (the first discriminator conv's fp32 image x its bf16 output gradient): the launch runs on the bf16
    # matrix cores and reads the fp32 operand as bf16, so that operand is drawn on the bf16 grid
    mixed = a.dtype != g.dtype
    if mixed:
        a, g = [t if t.dtype == torch.bfloat16 else t.bfloat16().float() for t in (a, g)]
    B = a.shape[0]
    cvec = torch.randn((B, rec["cvec"]), generator=gen, device=dev) if rec["cvec"] else None
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

    def dw(absval=False, channel=False, image=False):
        if rec["swap"]:
            X, dy = gd[:, :I], ad[:, :O]
        else:
            X = ad if cd is None else torch.cat((cd.view(B, -1, 1, 1).expand(-1, -1, ad.shape[2], ad.shape[3]), ad), 1)
            X, dy = X[:, :I], gd[:, :O]
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

    resd = res.double()
    sl = (slice(None), slice(i_off, i_off + I)) if I_total else (slice(None),)
    got = resd[sl]
    base = prefill.double()[sl] if rec["accumulate"] else 0.0
    ref = base + dw()
    absref = dw(absval=True)
    rnd = 2 * FP32_ROUND if rec["accumulate"] else 0.0      # the one rounding of prefill + gradient
    cls = ("bf16" if (mixed or a.dtype == torch.bfloat16) else "fp32") + "/wgrad"
    gamma = GAMMA[cls]
    ratio, ok = _compare(got, ref, absref, rnd, gamma)
    _note(cls, ratio, what)
    print("%s: ratio %.3e (gamma %.3e)" % (what, ratio, gamma))
    untouched_ok = True
    if I_total and prefill is not None:
        keep = torch.ones(full, dtype=torch.bool, device=dev)
        keep[sl] = False
        untouched_ok = torch.equal(res[keep], prefill[keep])
    sees_channel = _fails(got, base + dw(channel=True), absref, rnd, gamma)
    sees_image = _fails(got, base + dw(image=True), absref, rnd, gamma)
    assert ok, "%s: element error %.3e x absref > gamma %.3e" % (what, ratio, gamma)
    assert untouched_ok, "%s: elements outside input channels [%d, %d) changed" % (what, i_off, i_off + I)
    assert sees_channel, "%s: the bound cannot see one input channel's contribution" % what
    assert sees_image, "%s: the bound cannot see one image's contribution" % what


@pytest.mark.parametrize("mode,index", _cases())
def test_launch_replay_matches_fp64(gpu, mode, index):
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0, "the replay runs the default planner"
    assert os.environ.get("S2I_TUNE", "") == "", "the replay runs the default planner"
    rec = _load_census()[mode][index]
    what = "%s[%d] %s %s" % (mode, index, rec["fn"], "%s/%s" % R.layer_op(rec))
    gen = torch.Generator(device=gpu).manual_seed(zlib.crc32(_canon(rec).encode()))
    with torch.no_grad():
        if rec["fn"].startswith("conv"):
            _replay_conv(rec, gen, gpu, what)
        else:
            _replay_wgrad(rec, gen, gpu, what)
    torch.cuda.empty_cache()


def test_fp64_reference_gpu_equals_cpu(gpu):
    """The fp64 reference computed by torch on the GPU equals the CPU one (small shapes, every operation and layer)."""
    g = torch.Generator().manual_seed(5)
    for layer in R.LAYERS:
        kh = {"k1": 1, "k3s1": 3, "k4s2": 4, "up": 3}[layer]
        x = torch.randn(3, 6, 8, 8, generator=g, dtype=torch.float64)
        w = torch.randn(5, 6, kh, kh, generator=g, dtype=torch.float64)
        y = R.fwd(layer, x, w)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        for name, fn, args in (("fwd", R.fwd, (x, w)), ("dgrad", R.dgrad, (dy, w)), ("wgrad", R.wgrad, (x, dy, kh))):
            c = fn(layer, *args)
            d = fn(layer, *[t.to(gpu) if torch.is_tensor(t) else t for t in args]).cpu()
            assert torch.allclose(c, d, rtol=1e-12, atol=1e-12), (layer, name, float((c - d).abs().max()))


if __name__ == "__main__":
    # regenerate tests/step_launches.json (or the path given) from one eager step of each workload
    from speech_to_image_translation_without_text_amd import _lib
    _lib.load()
    _lib.require_device()
    census, calls = take_census(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else CENSUS_FILE
    with open(path, "w") as fp:
        fp.write("{\n" + ",\n".join('  "%s": [\n%s\n  ]' % (m, ",\n".join("    " + _canon(r) for r in recs))
                                    for m, recs in census.items()) + "\n}\n")
    for mode, recs in census.items():
        print("census %s: %d dispatcher calls per step, %d distinct launches -> %s" % (mode, calls[mode], len(recs), path))
