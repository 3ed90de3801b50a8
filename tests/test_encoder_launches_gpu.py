"""Every launch of the speech encoder (speech_encoder.CNNRNN._encode), at its production shapes, against plain fp64.

The encoder's CLIs run it at T = 2048 with batches of 240 (extract_audio_feature's default), a ragged last batch, or a
single WAV, unidirectional (Hd = 1024) by default and bidirectional (Hd = 512) on request; the planner of the matrix
kernel and the choice between the fused step kernel and the GEMM + cell fallback depend on those shapes.  So:

  * table: launch_table() derives every launch of a configuration (bidirectional, B) from the module's own layers;
    test_recorded_launches_equal_the_table runs a real forward_nhwc with ops.conv_raw and the four s2i_* entry points
    wrapped and requires the recorded set to equal it: a changed layer or a new launch fails here first.
  * matrix launches (the 40-channel K1, the seven CONV_1D layers, the input projection, the fallback's recurrent GEMM):
    replayed on fresh operands of both signs with dyadic weights, |out - ref| <= 2^-20 * absref as the train step's
    replay (GAMMA["fp32/conv"] of tests/conv_replay.py).  Power: the bound rejects a reference without the
    last input channel, without the last tap, and with one border tap missing in the first and the last output column.
  * s2i_maxpool_w3s2: bit-identical to max_pool2d, nothing written past the output; rejects zero padding and a dropped
    right tap in the last column.
  * s2i_lstm_step / s2i_lstm_cell, one step from a given state: the packed-sequence rule (live, finishing and finished
    sequences, forward and reverse time index, state of a finished sequence carried bit-identically), row strides wider
    than the payload, every element outside the written rows still the sentinel.  Bound: the propagated rounding of the
    pre-activation (see _gate_bound) plus LSTM_FN_TOL for the device's sigmoid / tanh.  Rejects one missing k term of the
    recurrent dot, gates f and i swapped, and the reverse index taken as L - 1 - step.
  * whole recurrence over L = 32 steps through both drivers of _encode, s2i_time_mean, and the whole encoder at the
    production batches, every utterance, words and sent, plus batch independence (B = 240 rows against B = 1 runs).

Measured constants (one MI355X; the module prints the values behind them at the end of a run): see LSTM_FN_*,
RECURRENCE_* and ENCODER_* below, each 2x the worst value measured against the fp64 reference.

Measured: 42 distinct matrix launches, worst ratio 4.1e-7 (9-tap layer at B = 240) against gamma 9.5e-7; one LSTM step
reaches 0.32 of its propagated bound at most; whole recurrence 2.0e-7; whole encoder words 3.4e-6, sent 9.7e-7; B = 240
rows against B = 1 runs 2.5e-6; time mean 0.10 of its bound.  No kernel bug was found.  With `x0 + 2 < W` changed to
`x0 + 2 < W - 1` in maxpool_w3s2_kernel and `len - 1 - step` to `T - 1 - step` in lstm_step_kernel (tried together, then
reverted) the four max-pool replays, the twelve D = 2 step replays, two recurrence and four whole-encoder cases fail.  The
module runs in about 6 s.
"""
import copy
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import encoder_ref as E  # noqa: E402
import launch_harness as LH  # noqa: E402
from conv_replay import GAMMA  # noqa: E402
from launch_harness import U  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import (ACT_NONE, ACT_RELU, CONV_1D, CONV_K1,  # noqa: E402
                                                                PACK_PLAIN)

pytestmark = pytest.mark.gpu

T_FRAMES = 2048                                     # audio.TARGET_LENGTH
PRODUCTION = [(bi, B) for bi in (True, False) for B in (1, 24, 37, 240)]
GAMMA_CONV = GAMMA["fp32/conv"]                     # 2^-20: same kernel family, same fp32 MFMA accumulation
SENTINEL = -12345.0

# Measured on one MI355X against the fp64 reference; the value in use is 2x the worst value measured.
# error of the device sigmoidf_ / tanhf beyond the propagated pre-activation rounding, all single-step cases: none.  The
# error never left the propagated bound (worst |got - ref| / bound: see "lstm err / propagated bound" in the report), so
# the functions' own error is hidden below the rounding of the Hd-term dot and nothing is added to the bound.
LSTM_FN_MEASURED = 0.0
LSTM_FN_TOL = 2 * LSTM_FN_MEASURED
# worst |got - ref| of the out tensor after all 32 steps, both drivers, all cases (|h| < 1):
RECURRENCE_MEASURED = 2.0e-7
RECURRENCE_TOL = 2 * RECURRENCE_MEASURED
# whole encoder: worst |got - ref| / (|ref| + rms(ref)) over words and sent of the five production runs:
# (words 3.4e-6 at B = 240, sent 9.7e-7): ENCODER_TOL is 145 times below the 1e-3 of tests/test_encoder.py
ENCODER_MEASURED = 3.45e-6
ENCODER_TOL = 2 * ENCODER_MEASURED
# BatchNorm folding in fp32 against fp64: fewer than 64 roundings (a 40-term sum, one sqrt, two divisions, five products)
FOLD_TOL = 64 * U

LEDGER = LH.Ledger()


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("encoder launch replay")
    print("  constants in use: gamma conv %.3e; LSTM function error %.3e (measured %.3e); recurrence %.3e (measured "
          "%.3e); encoder %.3e (measured %.3e)" % (GAMMA_CONV, LSTM_FN_TOL, LSTM_FN_MEASURED, RECURRENCE_TOL,
                                                   RECURRENCE_MEASURED, ENCODER_TOL, ENCODER_MEASURED))


@functools.lru_cache(maxsize=None)
def _cpu_net(bidirectional):
    """The CLIs' encoder (nhidden = nsent = 1024), seeded, with non-trivial running statistics, on the CPU."""
    return E.small_encoder(bidirectional, 1024)


def _gpu_net(bidirectional, gpu):
    return copy.deepcopy(_cpu_net(bidirectional)).to(gpu)


def _roundup4(v):
    return (v + 3) // 4 * 4


# ---- launch table ----------------------------------------------------------------------------------------------------
def launch_table(net, B, T=T_FRAMES):
    """The distinct launches of net.forward_nhwc on [B, 1, T, n_mels], from the module's own layers."""
    recs = []

    def conv(kind, x, N, conv1d, bias, act):
        recs.append(dict(fn="conv_raw", kind=kind, x=list(x), N=N, conv1d=conv1d, bias=N if bias else 0, act=act,
                         wR=_roundup4(x[3]), ldw=_roundup4(N)))

    W, C = T, None
    for m in net.Conv:
        if isinstance(m, nn.BatchNorm2d):
            continue                                                   # folded into the first convolution
        if isinstance(m, nn.MaxPool2d):
            assert (m.kernel_size, m.stride, m.padding) == ((1, 3), (1, 2), (0, 1)), m
            recs.append(dict(fn="s2i_maxpool_w3s2", B=B, H=1, W=W, C=C))
            W //= 2
            continue
        cv = m[0]
        assert isinstance(m[1], nn.BatchNorm2d) and isinstance(m[2], nn.ReLU) and cv.bias is None, m
        if C is None:                                                  # (n_mels x 1) kernel = 1x1 conv over n_mels channels
            assert cv.in_channels == 1 and cv.kernel_size[1] == 1 and cv.stride == (1, 1) and cv.padding == (0, 0), cv
            conv(CONV_K1, (B, 1, W, cv.kernel_size[0]), cv.out_channels, None, True, ACT_RELU)
        else:
            assert cv.in_channels == C and cv.kernel_size[0] == 1, cv
            k, st, pd = cv.kernel_size[1], cv.stride[1], cv.padding[1]
            conv(CONV_1D, (B, 1, W, C), cv.out_channels, [k, st, pd], True, ACT_RELU)
            W = (W + 2 * pd - k) // st + 1
        C = cv.out_channels
    L, D, Hd = W, net.num_direction, net.nhidden
    assert C == net.RNN.input_size and Hd == net.RNN.hidden_size and D == (2 if net.RNN.bidirectional else 1)
    conv(CONV_K1, (B, 1, L, C), D * 4 * Hd, None, True, ACT_NONE)        # input projections, all steps and directions
    if B <= 32 and Hd % 8 == 0 and Hd <= 512:                          # the step kernel's limits (include/s2i_hip.h)
        recs.append(dict(fn="s2i_lstm_step", ldx=D * 4 * Hd, B=B, T=L, Hd=Hd, D=D, ldo=D * Hd))
    else:
        conv(CONV_K1, (B, 1, 1, Hd), 4 * Hd, None, False, ACT_NONE)
        for d in range(D):
            recs.append(dict(fn="s2i_lstm_cell", ldx=D * 4 * Hd, B=B, T=L, Hd=Hd, reverse=d, ldo=D * Hd))
    recs.append(dict(fn="s2i_time_mean", B=B, T=L, C=D * Hd))
    return LH.dedup(recs)


# scalar arguments recorded per entry point (include/s2i_hip.h order, the step index and the stream left out)
_ARGS = {
    "s2i_maxpool_w3s2": "x B H W C y",
    "s2i_lstm_cell": "xproj ldx hproj lens B T Hd step reverse h c out ldo",
    "s2i_lstm_step": "xproj ldx whh_fwd whh_rev lens B T Hd D step h_in h_out c out ldo",
    "s2i_time_mean": "x B T C y",
}


def _passed(name):
    return name in ("s2i_last_error", "s2i_check_device")


def _record_forward(net, x, lens, mp):
    from speech_to_image_translation_without_text_amd import ops, speech_encoder as se
    recs = []
    orig = ops.conv_raw

    def conv_raw(kind, x_, cvec, packed, N, *, wR, ldw, bias=None, act=ACT_NONE, conv1d=None, **other):
        assert cvec is None and not other, ("encoder launch with arguments the table does not describe", other)
        recs.append(dict(fn="conv_raw", kind=int(kind), x=list(x_.shape), N=int(N),
                         conv1d=None if conv1d is None else [int(v) for v in conv1d],
                         bias=0 if bias is None else int(bias.numel()), act=int(act), wR=int(wR), ldw=int(ldw)))
        return orig(kind, x_, cvec, packed, N, wR=wR, ldw=ldw, bias=bias, act=act, conv1d=conv1d)

    mp.setattr(ops, "conv_raw", conv_raw)
    spy = LH.LibRecorder(_lib.load(), recs, _ARGS, _passed, skip=("step",), null_ok=False,
                        unlisted="entry point %s launched by the encoder has no place in the table")
    mp.setattr(se, "_lib", LH.ModuleSpy(spy))
    res = net.forward_nhwc(x, lens)
    torch.cuda.synchronize()
    return recs, res


def _mel(B, gen, gpu):
    return torch.randn((B, 1, T_FRAMES, 40), generator=gen, device=gpu) * 20 - 40


def _lens(B, gen, gpu):
    n_frames = torch.sort(torch.randint(64, T_FRAMES + 1, (B,), generator=gen, device=gpu), descending=True)[0]
    return (n_frames // 64).cpu()


@pytest.mark.parametrize("bidirectional,B", PRODUCTION)
def test_recorded_launches_equal_the_table(gpu, bidirectional, B):
    net = _gpu_net(bidirectional, gpu)
    gen = LH.gen_key(gpu, "table", bidirectional, B)
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        recs, (words, sent) = _record_forward(net, _mel(B, gen, gpu), _lens(B, gen, gpu), mp)
    D, Hd = net.num_direction, net.nhidden
    assert words.shape == (B, D * Hd, T_FRAMES // 64) and sent.shape == (B, D * Hd)
    now = {LH.canon(r) for r in recs}
    table = {LH.canon(r) for r in launch_table(_cpu_net(bidirectional), B)}
    print("bidirectional=%s B=%d: %d library calls, %d distinct launches" % (bidirectional, B, len(recs), len(now)))
    assert now == table, "launched but not in the table: %s; in the table but not launched: %s" % (
        sorted(now - table), sorted(table - now))


# ---- matrix launches -------------------------------------------------------------------------------------------------
def _matrix_launches():
    seen = {}
    for bi, B in PRODUCTION:
        for rec in launch_table(_cpu_net(bi), B):
            if rec["fn"] == "conv_raw":
                seen.setdefault(LH.canon(rec), rec)
    return [seen[k] for k in sorted(seen)]


MATRIX = _matrix_launches()


def _matrix_id(rec):
    geom = "k1" if rec["conv1d"] is None else "c1d-%d-%d-%d" % tuple(rec["conv1d"])
    return "%s-B%d-W%d-C%d-N%d" % (geom, rec["x"][0], rec["x"][2], rec["x"][3], rec["N"])


def _tap_term(xd, wd, t, stride, pad, Wo):
    """The contribution of tap t alone: [B, 1, Wo, N]."""
    xp = F.pad(xd[:, 0], (0, 0, pad, pad))
    return (xp[:, t:t + stride * (Wo - 1) + 1:stride] @ wd[:, :, t].t()).unsqueeze(1)


@pytest.mark.parametrize("index", range(len(MATRIX)), ids=[_matrix_id(r) for r in MATRIX])
def test_matrix_launch_replay_matches_fp64(gpu, index):
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0 and os.environ.get("S2I_TUNE", "") == "", "default planner"
    rec = MATRIX[index]
    what = _matrix_id(rec)
    gen = LH.gen_key(gpu, "matrix", LH.canon(rec))
    B, H, W, Cx = rec["x"]
    N = rec["N"]
    k, st, pd = rec["conv1d"] if rec["conv1d"] is not None else (1, 1, 0)
    with torch.no_grad():
        x = torch.randn((B, H, W, Cx), generator=gen, device=gpu)                   # both signs
        w = LH.dyadic((N, Cx, 1, k), gen, gpu)
        bias = torch.randn((N,), generator=gen, device=gpu) if rec["bias"] else None
        packed = ops.pack_weight(w if rec["conv1d"] is not None else w.view(N, Cx), PACK_PLAIN)
        assert (packed.shape[1], packed.shape[2]) == (rec["wR"], rec["ldw"]), (what, tuple(packed.shape))
        y, _, _ = ops.conv_raw(rec["kind"], x, None, packed, N, wR=rec["wR"], ldw=rec["ldw"], bias=bias, act=rec["act"],
                               conv1d=None if rec["conv1d"] is None else tuple(rec["conv1d"]))
        torch.cuda.synchronize()
        xd, wd = x.double(), w.double().view(N, Cx, k)
        bd = None if bias is None else bias.double()
        if rec["conv1d"] is None:
            pre = E.k1(xd, wd[:, :, 0], bd)
            absref = E.k1(xd.abs(), wd[:, :, 0].abs(), None if bd is None else bd.abs())
        else:
            pre = E.conv1d_pre(xd, wd, bd, k, st, pd)
            absref = E.conv1d_pre(xd.abs(), wd.abs(), bd.abs(), k, st, pd)
        Wo = pre.shape[2]
        assert tuple(y.shape) == tuple(pre.shape), (what, tuple(y.shape), tuple(pre.shape))
        act = torch.relu if rec["act"] == ACT_RELU else (lambda t: t)
        out = y.double()
        ratio, ok = LH.compare(out, act(pre), absref, 0.0, GAMMA_CONV)
        LEDGER.note("matrix ratio (gamma 2^-20)", ratio, what)
        print("%s: ratio %.3e (gamma %.3e)" % (what, ratio, GAMMA_CONV))
        # power (a): the last input channel's contribution removed
        chan = E.conv1d_pre(xd[..., -1:].contiguous(), wd[:, -1:, :].contiguous(), None, k, st, pd)
        sees_channel = LH.fails(out, act(pre - chan), absref, 0.0, GAMMA_CONV)
        sees_tap = sees_border = True
        if rec["conv1d"] is not None:
            # (b) the last tap removed
            sees_tap = LH.fails(out, act(pre - _tap_term(xd, wd, k - 1, st, pd, Wo)), absref, 0.0, GAMMA_CONV)
            # (c) only the first in-bounds tap of output column 0 and the last in-bounds tap of the last column removed
            assert pd > 0
            m = pre.clone()
            m[:, 0, 0] -= xd[:, 0, 0] @ wd[:, :, pd].t()
            start = (Wo - 1) * st - pd
            t1 = min(k - 1, W - 1 - start)
            m[:, 0, Wo - 1] -= xd[:, 0, start + t1] @ wd[:, :, t1].t()
            first_only, last_only = pre.clone(), pre.clone()
            first_only[:, 0, 0], last_only[:, 0, Wo - 1] = m[:, 0, 0], m[:, 0, Wo - 1]
            sees_border = all(LH.fails(out, act(r), absref, 0.0, GAMMA_CONV) for r in (m, first_only, last_only))
    assert ok, "%s: element error %.3e x absref > gamma %.3e" % (what, ratio, GAMMA_CONV)
    assert sees_channel, "%s: the bound cannot see one input channel's contribution" % what
    assert sees_tap, "%s: the bound cannot see the last tap" % what
    assert sees_border, "%s: the bound cannot see a border tap of the first / last output column" % what
    for m in ["matrix: last input channel removed"] + (["CONV_1D: last tap removed",
              "CONV_1D: border tap of column 0 / of the last column removed"] if rec["conv1d"] is not None else []):
        LEDGER.reject(m)
    torch.cuda.empty_cache()


def test_fp64_reference_gpu_equals_cpu(gpu):
    """tests/encoder_ref.py computed by torch on the GPU equals the CPU result (small shapes, every function)."""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    same = lambda a, b: torch.allclose(a, b.cpu(), rtol=1e-12, atol=1e-12)
    x = r(3, 1, 64, 8)
    for k, st, pd in ((3, 1, 1), (17, 2, 8), (13, 2, 6), (9, 2, 4), (5, 2, 2)):
        w, b = r(12, 8, k), r(12)
        assert same(E.conv1d(x, w, b, k, st, pd), E.conv1d(x.to(gpu), w.to(gpu), b.to(gpu), k, st, pd)), (k, st, pd)
    w, b = r(12, 8), r(12)
    assert same(E.k1(x, w, b, relu=True), E.k1(x.to(gpu), w.to(gpu), b.to(gpu), relu=True))
    assert torch.equal(E.maxpool_w3s2(x), E.maxpool_w3s2(x.to(gpu)).cpu())
    Hd, L, lens = 8, 6, [6, 4, 1]
    xp, whh = r(3, L, 8 * Hd), [r(4 * Hd, Hd) * 0.3, r(4 * Hd, Hd) * 0.3]
    h, c = r(3, Hd), r(3, Hd)
    for a, b_ in zip(E.lstm_step(xp[:, 0, :4 * Hd], h, c, whh[0]),
                     E.lstm_step(xp[:, 0, :4 * Hd].to(gpu), h.to(gpu), c.to(gpu), whh[0].to(gpu))):
        assert same(a, b_)
    seq = E.lstm_sequence(xp, lens, whh, Hd)
    assert same(seq, E.lstm_sequence(xp.to(gpu), lens, [t.to(gpu) for t in whh], Hd))
    assert same(E.time_mean(seq), E.time_mean(seq.to(gpu)))


# ---- max pooling -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 240])
@pytest.mark.parametrize("W,C", [(2048, 64), (128, 512)])
def test_maxpool_replay_is_bit_identical(gpu, W, C, B):
    lib = _lib.load()
    gen = LH.gen_key(gpu, "pool", W, C, B)
    x = torch.randn((B, 1, W, C), generator=gen, device=gpu)
    x[..., ::3] = -1.0 - x[..., ::3].abs()              # strictly negative channels: a zero padding would win at the borders
    x[:, :, -1, 1] = 9.0                                 # and the last position holds the maximum of the last window
    n = B * (W // 2) * C
    buf = torch.full((n + 4096,), SENTINEL, device=gpu)
    _lib.check(lib.s2i_maxpool_w3s2(_lib.ptr(x), B, 1, W, C, _lib.ptr(buf), _lib.stream()), "s2i_maxpool_w3s2")
    torch.cuda.synchronize()
    y = buf[:n].view(B, 1, W // 2, C)
    ref = E.maxpool_w3s2(x)
    assert torch.equal(ref, F.max_pool2d(x.permute(0, 3, 1, 2), (1, 3), (1, 2), (0, 1)).permute(0, 2, 3, 1))
    assert torch.equal(y, ref), "maxpool differs in %d elements" % int((y != ref).sum())
    assert bool((buf[n:] == SENTINEL).all()), "written past B*H*(W/2)*C"
    zero_pad = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1)), (1, 3), (1, 2)).permute(0, 2, 3, 1)
    short = ref.clone()
    short[:, :, -1] = torch.maximum(x[:, :, W - 3], x[:, :, W - 2])
    assert not torch.equal(y, zero_pad) and not torch.equal(y, short)
    LEDGER.reject("maxpool: zero instead of -inf padding")
    LEDGER.reject("maxpool: right tap of the last column dropped")


# ---- one LSTM step ---------------------------------------------------------------------------------------------------
L_STEPS = T_FRAMES // 64


def _gate_bound(xp, h, c, w, ez):
    """Propagated rounding of one cell update, fp64 tensors.  ez (B, 4*Hd) bounds the error of the gate pre-activations
    z = xp + h . w^T.  sigmoid' <= 1/4 and tanh' <= 1 carry it into the gates: e_i = ez_i / 4, e_f = ez_f / 4,
    e_g = ez_g, e_o = ez_o / 4.  c' = f c + i g (two products, one sum, each rounded):
        e_c = e_f |c| + e_i |g| + e_g |i| + 3 U (|f c| + |i g|);
    h' = o tanh(c') (tanh' <= 1, one product): e_h = e_o |tanh c'| + |o| e_c + 2 U |h'|.  Returns (e_h, e_c); what is
    left, the error of the device's sigmoidf_ / tanhf themselves, is what LSTM_FN_TOL holds."""
    Hd = h.shape[1]
    z = xp + h @ w.t()
    i, f, g, o = torch.sigmoid(z[:, :Hd]), torch.sigmoid(z[:, Hd:2 * Hd]), torch.tanh(z[:, 2 * Hd:3 * Hd]), \
        torch.sigmoid(z[:, 3 * Hd:])
    ei, ef, eg, eo = ez[:, :Hd] / 4, ez[:, Hd:2 * Hd] / 4, ez[:, 2 * Hd:3 * Hd], ez[:, 3 * Hd:] / 4
    c2 = f * c + i * g
    ec = ef * c.abs() + ei * g.abs() + eg * i + 3 * U * ((f * c).abs() + (i * g).abs())
    eh = eo * torch.tanh(c2).abs() + o * ec + 2 * U * (o * torch.tanh(c2)).abs()
    return eh, ec


def _lens_for(B, L, step, rot, gen, gpu):
    """Lengths mixing a sequence that finishes exactly at this step, a full one, a finished one (for step >= 1), 1 and
    one still live after this step; the rest random in [1, L]."""
    pattern = [step + 1, L, max(step, 1), 1, min(step + 2, L)]
    pattern = pattern[rot:] + pattern[:rot]
    extra = torch.randint(1, L + 1, (max(B - 5, 0),), generator=gen, device=gpu).tolist()
    return (pattern + extra)[:B]


def _t_index(lens, step, reverse, L=None):
    """Time position per sequence (0 for finished ones, which are masked out), and the live mask."""
    ts = [E.time_index(step, n, reverse) for n in lens]
    live = [t is not None for t in ts]
    if L is not None:                                   # the mutant: reverse index from the padded end
        ts = [None if t is None else (L - 1 - step if reverse else t) for t in ts]
    return [0 if t is None else t for t in ts], live


def _check_step(got_h, got_c, out, xproj, h_in, c_in, w, lens, step, d, Hd, ez_fn, what, power):
    """Compare one direction of one step with encoder_ref.lstm_step; returns the excess over the propagated bound."""
    B = len(lens)
    dev = xproj.device
    idx = torch.arange(B, device=dev)
    cols = slice(d * 4 * Hd, (d + 1) * 4 * Hd)
    ts, live = _t_index(lens, step, d == 1)
    tt, lv = torch.tensor(ts, device=dev), torch.tensor(live, device=dev)
    xp = xproj[idx, tt][:, cols].double()
    hd_, cd_, wd = h_in.double(), c_in.double(), w.double()
    rh, rc = E.lstm_step(xp, hd_, cd_, wd)
    eh, ec = _gate_bound(xp, hd_, cd_, wd, ez_fn(xp, hd_, wd))
    got_o = out[idx, tt][:, d * Hd:(d + 1) * Hd].double()
    errs = {"h": (got_h.double() - rh).abs(), "c": (got_c.double() - rc).abs(), "out": (got_o - rh).abs()}
    bounds = {"h": eh, "c": ec, "out": eh}
    excess = 0.0
    if lv.any():
        for key in errs:
            excess = max(excess, float((errs[key] - bounds[key])[lv].max()))
            LEDGER.note("lstm err / propagated bound", float((errs[key] / bounds[key])[lv].max()), what)
        assert torch.equal(got_o[lv], got_h.double()[lv]), "%s: out row differs from h'" % what
    # finished sequences: the cell state is carried bit-identically
    assert torch.equal(got_c[~lv], c_in[~lv]), "%s: c of a finished sequence changed" % what

    def rejected(mh, mc):
        return bool((((got_h.double() - mh).abs() > eh + LSTM_FN_TOL) | ((got_c.double() - mc).abs() > ec + LSTM_FN_TOL))[lv].any())

    if power and lv.any():
        h_drop = hd_.clone()
        h_drop[:, -1] = 0
        assert rejected(*E.lstm_step(xp, h_drop, cd_, wd)), "%s: cannot see one k term of the recurrent dot" % what
        xs = torch.cat((xp[:, Hd:2 * Hd], xp[:, :Hd], xp[:, 2 * Hd:]), 1)
        ws = torch.cat((wd[Hd:2 * Hd], wd[:Hd], wd[2 * Hd:]), 0)
        assert rejected(*E.lstm_step(xs, hd_, cd_, ws)), "%s: cannot see gates f and i swapped" % what
        LEDGER.reject("lstm: one k term of the recurrent dot removed")
        LEDGER.reject("lstm: gates f and i swapped")
        L = xproj.shape[1]
        if d == 1 and any(lv_ and n < L for lv_, n in zip(live, lens)):
            mt = torch.tensor(_t_index(lens, step, True, L)[0], device=dev)
            assert rejected(*E.lstm_step(xproj[idx, mt][:, cols].double(), hd_, cd_, wd)), \
                "%s: cannot see the reverse index taken as L - 1 - step" % what
            LEDGER.reject("lstm: reverse time index L - 1 - step")
    return max(excess, 0.0), ts, live, lv


def _untouched(out, written, what):
    """Every element of out outside the written (b, t, column block) entries is still the sentinel."""
    keep = torch.ones_like(out, dtype=torch.bool)
    for b, t, c0, c1 in written:
        keep[b, t, c0:c1] = False
    assert bool((out[keep] == SENTINEL).all()), "%s: out written outside its rows / columns" % what
    assert bool((out[~keep] != SENTINEL).all()), "%s: an expected out row was not written" % what


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("B", [1, 5, 31, 32])
@pytest.mark.parametrize("Hd", [8, 64, 512])
def test_lstm_step_single_step(gpu, Hd, B, D):
    lib = _lib.load()
    L = L_STEPS
    ez_fn = lambda xp, h, w: (Hd / 4 + 4) * U * (xp.abs() + h.abs() @ w.abs().t())   # fp32 dot of Hd terms in four lanes
    worst = 0.0
    for step in (0, 1, L - 1):
        for wide in (False, True):
            for rot in (0, 2):
                what = "lstm_step Hd=%d B=%d D=%d step=%d wide=%s rot=%d" % (Hd, B, D, step, wide, rot)
                gen = LH.gen_key(gpu, what)
                ldx, ldo = D * 4 * Hd + (8 if wide else 0), D * Hd + (4 if wide else 0)
                lens = _lens_for(B, L, step, rot, gen, gpu)
                xproj = torch.randn((B, L, ldx), generator=gen, device=gpu)
                w = [torch.randn((4 * Hd, Hd), generator=gen, device=gpu) / math.sqrt(Hd) for _ in range(D)]
                h_in = torch.rand((D, B, Hd), generator=gen, device=gpu) * 2 - 1
                c_in = torch.randn((D, B, Hd), generator=gen, device=gpu)
                c = c_in.clone()
                h_out = torch.full((D, B, Hd), SENTINEL, device=gpu)
                out = torch.full((B, L, ldo), SENTINEL, device=gpu)
                lens_dev = torch.tensor(lens, dtype=torch.int32, device=gpu)
                _lib.check(lib.s2i_lstm_step(_lib.ptr(xproj), ldx, _lib.ptr(w[0]), _lib.ptr(w[-1]), _lib.ptr(lens_dev), B, L,
                                             Hd, D, step, _lib.ptr(h_in), _lib.ptr(h_out), _lib.ptr(c), _lib.ptr(out), ldo,
                                             _lib.stream()), "s2i_lstm_step")
                torch.cuda.synchronize()
                written = []
                for d in range(D):
                    ex, ts, live, lv = _check_step(h_out[d], c[d], out, xproj, h_in[d], c_in[d], w[d], lens, step, d, Hd, ez_fn,
                                             what, power=True)
                    worst = max(worst, ex)
                    assert torch.equal(h_out[d][~lv], h_in[d][~lv]), "%s: h of a finished sequence not carried" % what
                    written += [(b, ts[b], d * Hd, (d + 1) * Hd) for b in range(B) if live[b]]
                _untouched(out, written, what)
    LEDGER.note("lstm function error (step)", worst, "Hd=%d B=%d D=%d" % (Hd, B, D))
    print("lstm_step Hd=%d B=%d D=%d: error beyond the propagated bound %.3e (allowed %.3e)" % (Hd, B, D, worst, LSTM_FN_TOL))
    assert worst <= LSTM_FN_TOL


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("B", [1, 37, 240])
@pytest.mark.parametrize("Hd", [512, 1024])
def test_lstm_cell_single_step(gpu, Hd, B, D):
    """The fallback's step as _encode forms it: the recurrent projection by the K1 GEMM (held to 2^-20 of sum |h||w| by the
    matrix replay), then s2i_lstm_cell per direction on xproj + d*4*Hd and out + d*Hd."""
    from speech_to_image_translation_without_text_amd import ops
    lib = _lib.load()
    L = L_STEPS
    ez_fn = lambda xp, h, w: GAMMA_CONV * (h.abs() @ w.abs().t()) + 2 * U * (xp.abs() + h.abs() @ w.abs().t())
    worst = 0.0
    for step in (0, 1, L - 1):
        for wide in (False, True):
            for rot in (0, 2):
                what = "lstm_cell Hd=%d B=%d D=%d step=%d wide=%s rot=%d" % (Hd, B, D, step, wide, rot)
                gen = LH.gen_key(gpu, what)
                ldx, ldo = D * 4 * Hd + (8 if wide else 0), D * Hd + (4 if wide else 0)
                lens = _lens_for(B, L, step, rot, gen, gpu)
                xproj = torch.randn((B, L, ldx), generator=gen, device=gpu)
                out = torch.full((B, L, ldo), SENTINEL, device=gpu)
                lens_dev = torch.tensor(lens, dtype=torch.int32, device=gpu)
                written = []
                for d in range(D):
                    w = torch.randn((4 * Hd, Hd), generator=gen, device=gpu) / math.sqrt(Hd)
                    packed = ops.pack_weight(w, PACK_PLAIN)
                    h_in = torch.rand((B, 1, 1, Hd), generator=gen, device=gpu) * 2 - 1
                    c_in = torch.randn((B, Hd), generator=gen, device=gpu)
                    hs, c = h_in.clone(), c_in.clone()
                    hproj, _, _ = ops.conv_raw(CONV_K1, hs, None, packed, 4 * Hd, wR=packed.shape[1], ldw=packed.shape[2])
                    _lib.check(lib.s2i_lstm_cell(_lib.ptr(xproj) + 4 * d * 4 * Hd, ldx, _lib.ptr(hproj), _lib.ptr(lens_dev), B, L,
                                                 Hd, step, d, _lib.ptr(hs), _lib.ptr(c), _lib.ptr(out) + 4 * d * Hd, ldo,
                                                 _lib.stream()), "s2i_lstm_cell")
                    torch.cuda.synchronize()
                    ex, ts, live, lv = _check_step(hs.view(B, Hd), c, out, xproj, h_in.view(B, Hd), c_in, w, lens, step, d, Hd,
                                             ez_fn, what, power=True)
                    worst = max(worst, ex)
                    assert torch.equal(hs.view(B, Hd)[~lv], h_in.view(B, Hd)[~lv]), "%s: h of a finished sequence touched" % what
                    written += [(b, ts[b], d * Hd, (d + 1) * Hd) for b in range(B) if live[b]]
                _untouched(out, written, what)
    LEDGER.note("lstm function error (cell)", worst, "Hd=%d B=%d D=%d" % (Hd, B, D))
    print("lstm_cell Hd=%d B=%d D=%d: error beyond the propagated bound %.3e (allowed %.3e)" % (Hd, B, D, worst, LSTM_FN_TOL))
    assert worst <= LSTM_FN_TOL


# ---- the whole recurrence --------------------------------------------------------------------------------------------
def _drive_step(xproj, raw, lens_dev, nsteps, B, L, Hd, D):
    """The fused branch of CNNRNN._encode: one s2i_lstm_step per step, h double-buffered."""
    lib = _lib.load()
    dev = xproj.device
    out = torch.zeros((B, L, D * Hd), dtype=torch.float32, device=dev)
    hbuf = torch.zeros((2, D, B, Hd), dtype=torch.float32, device=dev)
    cs = torch.zeros((D, B, Hd), dtype=torch.float32, device=dev)
    for step in range(nsteps):
        _lib.check(lib.s2i_lstm_step(_lib.ptr(xproj), D * 4 * Hd, _lib.ptr(raw[0]), _lib.ptr(raw[-1]), _lib.ptr(lens_dev), B, L,
                                     Hd, D, step, _lib.ptr(hbuf[step & 1]), _lib.ptr(hbuf[(step + 1) & 1]), _lib.ptr(cs),
                                     _lib.ptr(out), D * Hd, _lib.stream()), "s2i_lstm_step")
    return out


def _drive_fallback(xproj, raw, lens_dev, nsteps, B, L, Hd, D):
    """The fallback branch of CNNRNN._encode: per direction and step a K1 GEMM and s2i_lstm_cell."""
    from speech_to_image_translation_without_text_amd import ops
    lib = _lib.load()
    dev = xproj.device
    out = torch.zeros((B, L, D * Hd), dtype=torch.float32, device=dev)
    for d in range(D):
        hs = torch.zeros((B, 1, 1, Hd), dtype=torch.float32, device=dev)
        cs = torch.zeros((B, Hd), dtype=torch.float32, device=dev)
        w_hh = ops.pack_weight(raw[d], PACK_PLAIN)
        for step in range(nsteps):
            hproj, _, _ = ops.conv_raw(CONV_K1, hs, None, w_hh, 4 * Hd, wR=w_hh.shape[1], ldw=w_hh.shape[2])
            _lib.check(lib.s2i_lstm_cell(_lib.ptr(xproj) + 4 * d * 4 * Hd, D * 4 * Hd, _lib.ptr(hproj), _lib.ptr(lens_dev), B, L,
                                         Hd, step, d, _lib.ptr(hs), _lib.ptr(cs), _lib.ptr(out) + 4 * d * Hd, D * Hd,
                                         _lib.stream()), "s2i_lstm_cell")
    return out


def _ragged(B, L):
    """Descending lengths from L down to 1 (both included once B >= 2)."""
    return [L] if B == 1 else [max(1, round(L - b * (L - 1) / (B - 1))) for b in range(B)]


@pytest.mark.parametrize("B,Hd,D", [(24, 512, 2), (1, 512, 2), (240, 512, 2), (1, 1024, 1), (240, 1024, 1)])
def test_whole_recurrence_against_fp64(gpu, B, Hd, D):
    L = L_STEPS
    worst = 0.0
    for lens in ([_ragged(B, L)] if B > 1 else [[L], [19], [1]]):
        what = "recurrence B=%d Hd=%d D=%d lens=%d..%d" % (B, Hd, D, lens[0], lens[-1])
        gen = LH.gen_key(gpu, what)
        xproj = torch.randn((B, L, D * 4 * Hd), generator=gen, device=gpu)
        raw = [(torch.rand((4 * Hd, Hd), generator=gen, device=gpu) * 2 - 1) / math.sqrt(Hd) for _ in range(D)]
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=gpu)
        ref = E.lstm_sequence(xproj.double(), lens, [w.double() for w in raw], Hd)
        got = {"fallback": _drive_fallback(xproj, raw, lens_dev, max(lens), B, L, Hd, D)}
        if B <= 32 and Hd <= 512:
            got["step"] = _drive_step(xproj, raw, lens_dev, max(lens), B, L, Hd, D)
        torch.cuda.synchronize()
        pad = torch.arange(L, device=gpu).view(1, L) >= lens_dev.view(B, 1)
        for path, o in got.items():
            err = float((o.double() - ref).abs().max())
            worst = max(worst, err)
            print("%s %s: max |got - ref| %.3e (allowed %.3e)" % (what, path, err, RECURRENCE_TOL))
            assert err <= RECURRENCE_TOL, (what, path, err)
            assert bool((o[pad] == 0).all()), "%s %s: a padded position is not zero" % (what, path)
            assert bool((o[~pad] != 0).all()), "%s %s: a valid position was not written" % (what, path)
        if "step" in got:
            diff = float((got["step"] - got["fallback"]).abs().max())
            print("%s: step kernel vs fallback %.3e" % (what, diff))
            assert diff <= RECURRENCE_TOL, (what, diff)
    LEDGER.note("whole recurrence |got - ref|", worst, "B=%d Hd=%d D=%d" % (B, Hd, D))


# ---- time mean -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,C", [(1, 32, 1024), (240, 32, 1024), (37, 32, 1024)])
def test_time_mean_replay(gpu, B, T, C):
    lib = _lib.load()
    gen = LH.gen_key(gpu, "mean", B, T, C)
    x = torch.randn((B, T, C), generator=gen, device=gpu)
    lens = torch.tensor(_ragged(B, T) if B > 1 else [T // 2], device=gpu)
    x[torch.arange(T, device=gpu).view(1, T) >= lens.view(B, 1)] = 0           # trailing zeros, as the LSTM leaves them
    buf = torch.full((B * C + 1024,), SENTINEL, device=gpu)
    _lib.check(lib.s2i_time_mean(_lib.ptr(x), B, T, C, _lib.ptr(buf), _lib.stream()), "s2i_time_mean")
    torch.cuda.synchronize()
    got = buf[:B * C].view(B, C).double()
    xd = x.double()
    bound = (T + 1) * U * xd.abs().mean(1)                                     # sequential fp32 sum, one division
    err = (got - E.time_mean(xd)).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    LEDGER.note("time_mean err / bound", ratio, "B=%d" % B)
    print("time_mean B=%d: worst err / bound %.3f" % (B, ratio))
    assert bool((err <= bound).all()) and bool((buf[B * C:] == SENTINEL).all())
    over_len = xd.sum(1) / lens.view(B, 1).double()
    no_last = xd[:, :-1].sum(1) / T
    assert not bool(((got - over_len).abs() <= bound).all()), "cannot see a mean over the valid positions only"
    if int(lens.max()) == T:
        assert not bool(((got - no_last).abs() <= bound).all()), "cannot see the last position dropped"
    LEDGER.reject("time_mean: mean over len instead of T")
    LEDGER.reject("time_mean: last position dropped")


# ---- the whole encoder -----------------------------------------------------------------------------------------------
def _unpacked(net):
    """The operands the kernels see, read back from CNNRNN._prepare(): packed weights P[tap][Cin][Cout] -> (O, I, taps)."""
    prep = net._prepare()
    layers = []
    for layer in prep["layers"]:
        if layer[0] == "pool":
            layers.append(layer)
        elif layer[0] == "k1":
            layers.append(("k1", layer[1][0, :, :layer[3]].t().double(), layer[2].double()))
        else:
            layers.append(("c1d", layer[1][:, :, :layer[3]].permute(2, 1, 0).double(), layer[2].double(), layer[4]))
    return dict(layers=layers, w_ih=prep["w_ih"][0].t().double(), b_ih=prep["b_ih"].double(),
                w_hh=[w.double() for w in prep["w_hh_raw"]])


def _hybrid(got, ref):
    """max |got - ref| / (|ref| + rms(ref)): an element-wise relative error floored at the tensor's own scale."""
    return float(((got.double() - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())).max())


@pytest.mark.parametrize("bidirectional", [True, False])
def test_prepare_folds_as_the_reference_does(gpu, bidirectional):
    """CNNRNN._prepare() (fp32, on the GPU, packed) against encoder_ref.fold (fp64, from the modules)."""
    got = _unpacked(_gpu_net(bidirectional, gpu))
    ref = E.fold(_cpu_net(bidirectional))
    for lg, lr in zip(got["layers"], ref["layers"]):
        assert lg[0] == lr[0]
        if lg[0] == "pool":
            continue
        w, b = lr[1].to(gpu), lr[2].to(gpu)
        assert bool(((lg[1] - w).abs() <= FOLD_TOL * w.abs()).all()), lg[0]
        # the bias is a difference (and for the first layer a 40-term sum): bounded by the magnitude of its terms
        assert bool(((lg[2] - b).abs() <= FOLD_TOL * (b.abs() + b.abs().max())).all()), lg[0]
        assert lg[0] == "k1" or tuple(lg[3]) == tuple(lr[3])
    assert torch.equal(got["w_ih"], ref["w_ih"].to(gpu)) and all(torch.equal(a, b.to(gpu)) for a, b in zip(got["w_hh"], ref["w_hh"]))
    assert bool(((got["b_ih"] - ref["b_ih"].to(gpu)).abs() <= 2 * U * ref["b_ih"].to(gpu).abs().max()).all())


@pytest.mark.parametrize("bidirectional,B", [(True, 240), (False, 240), (True, 1), (False, 1), (True, 37)])
def test_whole_encoder_at_production_batches(gpu, bidirectional, B):
    net = _gpu_net(bidirectional, gpu)
    what = "encoder bidirectional=%s B=%d" % (bidirectional, B)
    gen = LH.gen_key(gpu, what)
    with torch.no_grad():
        mel, lens = _mel(B, gen, gpu), _lens(B, gen, gpu)
        words, sent = net.forward_nhwc(mel, lens)
        torch.cuda.synchronize()
        prep = _unpacked(net)
        rw, rs = [], []
        for b0 in range(0, B, 48):                                            # every utterance, in chunks
            w_, s_ = E.encode(prep, mel[b0:b0 + 48].double(), lens[b0:b0 + 48].tolist())
            rw.append(w_)
            rs.append(s_)
        rw, rs = torch.cat(rw), torch.cat(rs)
        ew, es = _hybrid(words, rw), _hybrid(sent, rs)
        LEDGER.note("whole encoder words", ew, what)
        LEDGER.note("whole encoder sent", es, what)
        print("%s: words %.3e, sent %.3e (allowed %.3e; max |words| %.3f)" % (what, ew, es, ENCODER_TOL, float(rw.abs().max())))
        assert ew <= ENCODER_TOL and es <= ENCODER_TOL, (what, ew, es)
        for b in range(B):
            assert float(words[b, :, int(lens[b]):].abs().sum()) == 0.0, "%s: padded steps of row %d not zero" % (what, b)
        if B == 240:
            # batch independence: the same utterances alone take other planner variants (and, bidirectional, the fused
            # step kernel instead of the fallback) and give the same numbers
            scale_w, scale_s = rw.pow(2).mean().sqrt(), rs.pow(2).mean().sqrt()
            for b in (0, 119, 239):
                w1, s1 = net.forward_nhwc(mel[b:b + 1].contiguous(), lens[b:b + 1])
                dw = float(((w1[0].double() - words[b].double()).abs() / (rw[b].abs() + scale_w)).max())
                ds = float(((s1[0].double() - sent[b].double()).abs() / (rs[b].abs() + scale_s)).max())
                LEDGER.note("batch independence", max(dw, ds), what + " row %d" % b)
                assert dw <= ENCODER_TOL and ds <= ENCODER_TOL, (what, b, dw, ds)
    torch.cuda.empty_cache()
