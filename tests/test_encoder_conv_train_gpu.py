"""The speech encoder's conv-stack training kernels on the GPU against their fp64 restatement
(tests/encoder_conv_train_ref.py): temporal-conv input and weight gradients, train-mode BatchNorm + ReLU, the scalar input
BatchNorm, the pool backward, ops.conv_stack_train as a whole with replayed decisions, run-to-run determinism and
encoder_train.EncoderTrainer.

Metric: max|got - ref| / max|ref| per tensor.  BOUNDS holds, per tensor class, TWICE the worst value the same restatement
run in fp32 on the CPU shows against its fp64 run over every case of this module (the yardstick,
encoder_conv_train_ref.measure_yardsticks; the factor of two is for the kernels' different summation order).  The bounds
come from that yardstick alone, never from what the kernels give; every test prints what it measured.

    class             yardstick (CPU fp32 vs fp64)   bound      worst seen on the MI355X: layer cases / edge cases
    dgrad             5.64e-7                        1.13e-6    6.14e-7 / 5.54e-7 (64 -> 64 k3, 528 rows)
    wgrad             6.22e-7                        1.24e-6    5.11e-7 / 4.07e-7 (64 -> 64 k3, 160 rows)
    bn_out            1.74e-7                        3.5e-7     1.14e-7 / 1.39e-7 (M = 129, C = 2052)
    bn_dy             1.69e-7                        3.4e-7     1.49e-7 / 1.57e-7 (M = 129, C = 2052)
    bn_dparam         3.27e-7                        6.5e-7     1.47e-7 / 2.14e-7 (M = 129, C = 2052)
    running           1.16e-7                        2.3e-7     9.58e-8 / 8.22e-8 (input BatchNorm, B = 7, T = 40)
    pool_dx           4.73e-8                        9.5e-8     4.73e-8 / 4.67e-8
    block_out         4.16e-7                        8.33e-7    4.13e-7
    block_running     1.03e-7                        2.05e-7    1.02e-7
    block_dx          4.86e-7                        9.73e-7    4.59e-7
    block_dw          8.09e-7                        1.62e-6    5.33e-7
    block_dparam      3.64e-7                        7.28e-7    3.85e-7
    stack_feat        3.76e-6                        7.5e-6     4.59e-6
    stack_grad        2.58e-6                        5.2e-6     3.04e-6
    stack_bn0_dgamma  4.04e-3                        8.1e-3     5.98e-3
    stack_bn0_dbeta   2.84e-9                        5.7e-9     1.55e-9
    stack_running     1.14e-6                        2.3e-6     1.78e-6
    traj_loss         1.92e-4                        3.8e-4     1.42e-4

The edge cases (encoder_conv_train_ref.CONV_EDGE_CASES, WGRAD_ONLY_CASES, BN_EDGE_CASES, BN0_EDGE_CASES, POOL_EDGE_CASES)
leave the layer shapes: even k, odd pad, k == stride, k = 1, 30 and 31, widths that fill no tile, ragged row chunks; they
raise no yardstick past half its bound (bn_out goes from 1.737e-7 to 1.745e-7).  Every buffer a launch of these operators
writes lies between two NaN guard bands of 128 rows, which must come back untouched.  The block_* classes are one block as
ops.temporal_conv_bn_relu runs it (the convolution's statistics epilogue included) with the GPU's ReLU mask replayed into
the fp64 backward.  The input BatchNorm at B = 1, T = 2 (80 elements) first measured 2.46e-7 on `running`: its variance
was E[x^2] - mean^2 from fp32 sums of fp32 squares (s2i_colstats), on log-mel input whose mean^2 is 4.8 x its variance;
s2i_bn1_stats now forms both sums in double (4.1e-8 there, and B = 3, T = 64 went from 1.44e-7 to 3.7e-9).

stack_bn0_dgamma / stack_bn0_dbeta are the leading BatchNorm2d(1)'s gradients inside the whole stack.  The block behind it
normalises its own output, so the loss does not depend on a shift of its input at all and on a scale only through eps:
d bias is structurally zero (measured against the mass sum|dout| of the terms that cancel) and d weight is a cancelling sum
(its fp32 yardstick is 4e-3).  With the scalar BatchNorm's backward sums taken by the C = 4 walk of
s2i_bn_act_bwd_reduce (one fp32 chain per block) the per-operator d weight measured 7.42e-7 against bn_dparam's 6.5e-7;
s2i_bn1_bwd_reduce adds a block's terms in double instead.  traj_loss is each loss scalar's error relative to the step's total loss.

Decisions: the per-operator inputs keep every fp64 BatchNorm output at least m away from zero and every pool window's two
largest entries at least m apart (or exactly tied), m = 100 x the forward yardstick x max|tensor|; the tests assert it.
The whole-stack test replays the GPU's ReLU masks and pool maxima (ops.CONV_STACK_LOG) into the fp64 backward and asserts
that they differ from the fp64 forward's own only inside the margin and at no more than 0.1 % of a layer's elements (on
the CPU, fp32 standing in for the GPU: none differ).
"""
import pytest
import torch

import encoder_conv_train_ref as R
import encoder_ref
from helpers import assert_close

BOUNDS = {
    "dgrad": 1.13e-6, "wgrad": 1.24e-6, "bn_out": 3.5e-7, "bn_dy": 3.4e-7, "bn_dparam": 6.5e-7, "running": 2.3e-7,
    "pool_dx": 9.5e-8, "stack_feat": 7.5e-6, "stack_grad": 5.2e-6, "stack_bn0_dgamma": 8.1e-3, "stack_bn0_dbeta": 5.7e-9,
    "stack_running": 2.3e-6, "traj_loss": 3.8e-4,
    "block_out": 8.33e-7, "block_running": 2.05e-7, "block_dx": 9.73e-7, "block_dw": 1.62e-6, "block_dparam": 7.28e-7,
}
YARD_Z = 3.54e-6          # forward yardstick of the whole stack's BatchNorm outputs (class stack_z)
FLIP_CAP = 1e-3           # at most 0.1 % of a layer's decisions may differ from the fp64 forward's own

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _env():
    from speech_to_image_translation_without_text_amd import _lib, ops
    return _lib.load(), _lib, ops


def dev(t, gpu):
    return t.float().contiguous().to(gpu)


def nan_like(shape, gpu):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=gpu)


def guarded(shape, row, gpu):
    """A NaN-filled tensor of `shape` for a kernel to write, cut out of a larger NaN-filled allocation with a full tile of
    rows (128 x `row` floats) in front of it and behind it -> (whole allocation, the tensor)."""
    n = 1
    for v in shape:
        n *= v
    band = 128 * row
    assert band % 4 == 0
    whole = nan_like((band + n + band,), gpu)
    return whole, whole[band:band + n].view(tuple(shape))


def assert_guarded(whole, inner, what):
    """Every element of the tensor written, nothing written outside it."""
    band = (whole.numel() - inner.numel()) // 2
    assert bool(torch.isfinite(inner).all()), "%s holds elements no launch wrote" % what
    assert bool(torch.isnan(whole[:band]).all()), "%s: a launch wrote in front of the tensor" % what
    assert bool(torch.isnan(whole[band + inner.numel():]).all()), "%s: a launch wrote behind the tensor" % what


def report(errs):
    """errs: [(class, what, value)] -> prints every figure, then asserts the bounds."""
    for cls, what, e in errs:
        print("%s: %.3e (bound %.2e, class %s)" % (what, e, BOUNDS[cls], cls))
    bad = ["%s %.3e > %.2e" % (what, e, BOUNDS[cls]) for cls, what, e in errs if not e <= BOUNDS[cls]]
    assert not bad, "; ".join(bad)


# ---- temporal-conv gradients ------------------------------------------------------------------------------------------------
_CONV_REF = {}


def conv_ref(case):
    if case not in _CONV_REF:
        cin, cout, geom, B, Wo = case
        x, w, dy = R.conv_case(cin, cout, geom, B, Wo)
        _CONV_REF[case] = (x, w, dy, R.conv_dgrad(dy, w, geom, x.shape[2]), R.conv_wgrad(x, dy, geom))
    return _CONV_REF[case]


def _case_id(c):
    return "%dto%d_k%ds%d_B%d_Wo%d" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4])


def run_dgrad(gpu, case):
    """s2i_conv1d_dgrad at `case` into a guarded dx."""
    lib, _lib, ops = _env()
    cin, cout, (k, s, pad), B, Wo = case
    x, w, dy = conv_ref(case)[:3]
    W = x.shape[2]
    packed = ops.pack_weight(dev(w.unsqueeze(2), gpu), _lib.PACK_PLAIN)
    dy_d = dev(dy, gpu)
    whole, dx = guarded((B, 1, W, cin), cin, gpu)
    _lib.check(lib.s2i_conv1d_dgrad(_lib.ptr(dy_d), _lib.ptr(packed), _lib.ptr(dx), B, W, cin, cout, packed.shape[1],
                                    packed.shape[2], k, s, pad, _lib.stream()), "s2i_conv1d_dgrad")
    torch.cuda.synchronize()
    assert_guarded(whole, dx, "dx")
    return dx


def run_wgrad(gpu, case):
    """s2i_conv1d_wgrad at `case` into a guarded dW through a guarded workspace -> (dW, workspace bytes)."""
    lib, _lib, ops = _env()
    cin, cout, (k, s, pad), B, Wo = case
    x, w, dy = conv_ref(case)[:3]
    W = x.shape[2]
    x_d, dy_d = dev(x, gpu), dev(dy, gpu)
    whole_dw, dw = guarded((cout, cin, 1, k), cin * k, gpu)
    wsb = lib.s2i_conv1d_wgrad_workspace_bytes(B, W, cin, cout, k, s, pad)
    assert wsb > 0 and wsb % (cout * k * cin * 4) == 0
    whole_ws, ws = guarded((wsb // 4,), cin * k, gpu)
    _lib.check(lib.s2i_conv1d_wgrad(_lib.ptr(x_d), _lib.ptr(dy_d), _lib.ptr(dw), B, W, cin, cout, k, s, pad, _lib.ptr(ws), wsb,
                                    _lib.stream()), "s2i_conv1d_wgrad")
    torch.cuda.synchronize()
    assert_guarded(whole_dw, dw, "dW")
    assert_guarded(whole_ws, ws, "the weight-gradient workspace")
    return dw, wsb


@pytest.mark.parametrize("case", R.CONV_CASES + R.CONV_EDGE_CASES, ids=_case_id)
def test_conv1d_dgrad_against_fp64(gpu, case):
    dx = run_dgrad(gpu, case)
    assert bool(torch.isfinite(dx).all()), "dx holds elements no phase wrote"
    report([("dgrad", "dx %s" % _case_id(case), R.rel_err(dx, conv_ref(case)[3]))])


@pytest.mark.parametrize("case", R.CONV_CASES + R.CONV_EDGE_CASES + R.WGRAD_ONLY_CASES, ids=_case_id)
def test_conv1d_wgrad_against_fp64(gpu, case):
    cin, cout, (k, s, pad), B, Wo = case
    dw, wsb = run_wgrad(gpu, case)
    if case == (64, 64, (3, 1, 1), 3, 2048):
        assert wsb == 48 * 64 * 64 * 3 * 4, "6 144 rows of a 3-tile result: the row reduction is split into 48 slabs"
    if case == (64, 64, (3, 1, 1), 33, 16):
        assert wsb == 4 * 64 * 64 * 3 * 4, "528 rows: 17 chunks in 4 slabs of 5, 5, 5 and 2, the last chunk half full"
    assert bool(torch.isfinite(dw).all()), "dW holds elements no tile wrote"
    report([("wgrad", "dW %s" % _case_id(case), R.rel_err(dw, conv_ref(case)[4]))])


@pytest.mark.parametrize("mutant", sorted(R.MUTANT_KILLS))
def test_edge_mutants_are_rejected_against_the_gpu_result(gpu, mutant):
    """The GPU's result at the case that rejects the mutant on the CPU is further from the mutant's fp64 result than the
    class bound: a kernel with that mistake could not pass the case."""
    case = R.MUTANT_KILLS[mutant]
    x, w, dy = conv_ref(case)[:3]
    if mutant == "col_tail_zero":
        cls, got, bad = "wgrad", run_wgrad(gpu, case)[0], R.conv_wgrad(x, dy, case[2], mutant)
    else:
        cls, got, bad = "dgrad", run_dgrad(gpu, case), R.conv_dgrad(dy, w, case[2], x.shape[2], mutant)
    e = R.rel_err(got, bad)
    print("%s at %s: %.3e from the GPU result (bound %.2e)" % (mutant, _case_id(case), e, BOUNDS[cls]))
    assert e > BOUNDS[cls]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
DGRAD_OK = dict(B=3, W=16, Cin=64, Cout=64, wR=64, ldw=64, kw=3, stride=1, pad=1)
DGRAD_REFUSED = [
    ("Cout = 36", dict(Cout=36, ldw=36), b"multiple of 32"),
    ("stride 3", dict(kw=3, stride=3), b"bad kw/stride/pad"),
    ("stride 4", dict(W=32, Cin=8, Cout=32, wR=8, ldw=32, kw=4, stride=4, pad=0), b"bad kw/stride/pad"),
    ("kw < stride", dict(kw=1, stride=2, pad=0), b"bad kw/stride/pad"),
    ("kw = 32", dict(kw=32, pad=16), b"bad kw/stride/pad"),
    ("W = 48", dict(W=48), b"bad extent"),
    ("Wo = 14", dict(pad=0), b"output width 14"),
    ("wR < Cin", dict(wR=32), b"too small"),
    ("ldw % 4 != 0", dict(Cout=32, ldw=34), b"too small"),
]


def test_conv1d_gradients_refuse_what_they_do_not_take(gpu):
    """Real device tensors far larger than any of the extents, NaN-prefilled outputs: a non-zero return, a message, and
    nothing written."""
    lib, _lib, ops = _env()
    n = 1 << 16
    p, st = _lib.ptr, _lib.stream
    a, b = torch.randn(n, device=gpu), torch.randn(n, device=gpu)
    a0, b0 = a.clone(), b.clone()
    out, ws = nan_like((n,), gpu), nan_like((n,), gpu)

    def untouched(what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), "%s: refused, yet an output was written" % what
        assert torch.equal(a, a0) and torch.equal(b, b0), what

    g = DGRAD_OK
    assert max(g["B"] * g["W"] * g["Cin"], g["kw"] * g["wR"] * g["ldw"]) <= n
    for what, change, message in DGRAD_REFUSED:
        g = dict(DGRAD_OK, **change)
        rc = lib.s2i_conv1d_dgrad(p(a), p(b), p(out), g["B"], g["W"], g["Cin"], g["Cout"], g["wR"], g["ldw"], g["kw"],
                                  g["stride"], g["pad"], st())
        assert rc != 0, "dgrad took %s" % what
        err = lib.s2i_last_error()
        print("dgrad %s: %s" % (what, err.decode()))
        assert b"conv1d dgrad" in err and message in err, (what, err)
        untouched("dgrad " + what)
    for cin, cout, (k, s, pad), B, Wo in R.WGRAD_ONLY_CASES:      # what the weight gradient takes and the input gradient does not
        assert lib.s2i_conv1d_dgrad(p(a), p(b), p(out), B, Wo * s, cin, cout, cin, cout, k, s, pad, st()) != 0
        assert b"conv1d dgrad" in lib.s2i_last_error()
        untouched("dgrad %d -> %d k%d s%d" % (cin, cout, k, s))
    # weight gradient: x = a, dy = b, dW = out
    assert lib.s2i_conv1d_wgrad(p(a), p(b), p(out), 3, 16, 6, 64, 3, 1, 1, p(ws), n * 4, st()) != 0
    err = lib.s2i_last_error()
    assert b"conv1d wgrad" in err and b"bad extent" in err, err
    untouched("wgrad Cin = 6")
    need = lib.s2i_conv1d_wgrad_workspace_bytes(3, 16, 64, 64, 3, 1, 1)
    assert 0 < need <= n * 4
    assert lib.s2i_conv1d_wgrad(p(a), p(b), p(out), 3, 16, 64, 64, 3, 1, 1, p(ws), need - 4, st()) != 0
    err = lib.s2i_last_error()
    assert b"workspace too small" in err, err
    untouched("wgrad with a workspace 4 bytes short")


# ---- train-mode BatchNorm + ReLU ----------------------------------------------------------------------------------------------
def bn_margin(ref):
    return 100 * (BOUNDS["bn_out"] / 2) * float(ref["out"].abs().max())


def bn_gpu(lib, _lib, ops, gpu, y, gamma, beta, dout, running, relu):
    """The launches of one block's BatchNorm, forward and backward, every output prefilled with NaN."""
    C = y.shape[-1] if relu else 4
    y_d, dout_d = dev(y, gpu), dev(dout, gpu)
    M = y_d.numel() // C
    gamma_d, beta_d = dev(gamma, gpu), dev(beta, gpu)
    rm, rv = dev(running[0], gpu), dev(running[1], gpu)
    nbt = torch.tensor(running[2], dtype=torch.int64, device=gpu)
    nparts = ops._num_parts(M)
    ck, p, st = _lib.check, _lib.ptr, _lib.stream
    # every buffer a kernel of this file (or the statistics pass in front of them) fills sits between guard bands
    G = {k: guarded(shape, C, gpu) for k, shape in (("part", (2, nparts, C)), ("out", tuple(y_d.shape)), ("dy", tuple(y_d.shape)),
                                                    ("part2", (2, nparts, C)))}
    part, out, dy, part2 = (G[k][1] for k in ("part", "out", "dy", "part2"))
    if relu:
        ck(lib.s2i_colstats(p(y_d), M, C, C, p(part), nparts, st()), "s2i_colstats")
    else:
        ck(lib.s2i_bn1_stats(p(y_d), y_d.numel(), p(part), nparts, st()), "s2i_bn1_stats")
    coef, red2 = nan_like((4, C), gpu), nan_like((2, C), gpu)
    dgamma, dbeta = nan_like(gamma_d.shape, gpu), nan_like(gamma_d.shape, gpu)
    if relu:
        ck(lib.s2i_bn_finalize(p(part), nparts, 1, C, M, p(gamma_d), p(beta_d), p(rm), p(rv), p(nbt), 0.1, 1e-5, p(coef), st()),
           "s2i_bn_finalize")
        ck(lib.s2i_bn_relu_forward(p(y_d), M, C, p(coef), p(out), st()), "s2i_bn_relu_forward")
        ck(lib.s2i_bn_relu_bwd_reduce(p(y_d), p(out), p(dout_d), M, C, p(coef), p(part2), nparts, st()), "s2i_bn_relu_bwd_reduce")
        ck(lib.s2i_bn_bwd_finalize(p(part2), nparts, 1, C, M, p(dgamma), p(dbeta), 0, p(red2), st()), "s2i_bn_bwd_finalize")
        ck(lib.s2i_bn_relu_bwd_apply(p(y_d), p(out), p(dout_d), M, C, p(coef), p(red2), p(dy), st()), "s2i_bn_relu_bwd_apply")
        torch.cuda.synchronize()
        for k, (whole, inner) in G.items():
            assert_guarded(whole, inner, "BatchNorm " + k)
    else:
        # the launches of ops.InputBatchNorm on guarded buffers ...
        n = y_d.numel()
        rm1, rv1, nbt1 = rm.clone(), rv.clone(), nbt.clone()
        ck(lib.s2i_bn1_finalize(p(part), nparts, n, p(gamma_d), p(beta_d), p(rm1), p(rv1), p(nbt1), 0.1, 1e-5, p(coef), st()),
           "s2i_bn1_finalize")
        ck(lib.s2i_bn_act_forward(p(y_d), M, 1, 4, p(coef), ops.ACT_NONE, None, p(out), st()), "s2i_bn_act_forward")
        ck(lib.s2i_bn1_bwd_reduce(p(y_d), p(dout_d), n, p(coef), p(part2), nparts, st()), "s2i_bn1_bwd_reduce")
        ck(lib.s2i_bn1_bwd_finalize(p(part2), nparts, n, p(dgamma), p(dbeta), p(red2), st()), "s2i_bn1_bwd_finalize")
        ck(lib.s2i_bn_act_bwd_apply(p(y_d), p(dout_d), 4, M, 1, 4, p(coef), p(red2), ops.ACT_NONE, p(dy), st()),
           "s2i_bn_act_bwd_apply")
        torch.cuda.synchronize()
        for k, (whole, inner) in G.items():
            assert_guarded(whole, inner, "input BatchNorm " + k)
        direct = (out, dy, dgamma, dbeta, rm1, rv1)
        # ... and the operator itself, which must give the same bits
        x = y_d.clone().requires_grad_(True)
        old = ops.CONV_STACK_SENTINEL
        ops.CONV_STACK_SENTINEL = NAN
        try:
            g, b = gamma_d.clone().requires_grad_(True), beta_d.clone().requires_grad_(True)
            out = ops.input_batchnorm(x, g, b, (rm, rv, nbt))
            dy, dgamma, dbeta = torch.autograd.grad(out, [x, g, b], dout_d)
        finally:
            ops.CONV_STACK_SENTINEL = old
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "dy", "dgamma", "dbeta", "running_mean", "running_var"), direct,
                              (out.detach(), dy, dgamma, dbeta, rm, rv)):
            assert torch.equal(a.reshape(-1), b.reshape(-1)), "input BatchNorm %s: the operator and its launches disagree" % name
    torch.cuda.synchronize()
    return dict(out=out.detach(), dy=dy, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv, nbt=int(nbt))


def check_bn(gpu, inputs, relu, what):
    lib, _lib, ops = _env()
    y, gamma, beta, dout, running = inputs
    ref = R.bn_all(y, gamma, beta, dout, running, torch.float64, relu)
    if relu:
        m = bn_margin(ref)
        assert m <= R.BN_MARGIN and R.margin_ok(ref["z"], m), "an fp64 BatchNorm output lies within m = %.2e of zero" % m
    got = bn_gpu(lib, _lib, ops, gpu, y, gamma, beta, dout, running, relu)
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("out", "dy", "dgamma", "dbeta", "running_mean", "running_var"))
    if relu:
        assert torch.equal(got["out"].cpu() > 0, ref["out"] > 0)
    assert got["nbt"] == ref["nbt"] == running[2] + 1
    report([("bn_out", what + " out", R.rel_err(got["out"], ref["out"])), ("bn_dy", what + " dy", R.rel_err(got["dy"], ref["dy"])),
            ("bn_dparam", what + " dgamma", R.rel_err(got["dgamma"], ref["dgamma"])),
            ("bn_dparam", what + " dbeta", R.rel_err(got["dbeta"], ref["dbeta"])),
            ("running", what + " running_mean", R.rel_err(got["running_mean"], ref["running_mean"])),
            ("running", what + " running_var", R.rel_err(got["running_var"], ref["running_var"]))])
    return ref


@pytest.mark.parametrize("M,C", R.BN_CASES + R.BN_EDGE_CASES)
def test_bn_relu_train_against_fp64(gpu, M, C):
    inputs = R.bn_case(M, C)
    ref = check_bn(gpu, inputs, True, "bn M=%d C=%d" % (M, C))
    # the running statistics are nn.BatchNorm2d's
    y, gamma, beta, dout, running = inputs
    bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(running[0])
        bn.running_var.copy_(running[1])
        bn(y.permute(0, 3, 1, 2))
    assert R.rel_err(ref["running_mean"], bn.running_mean) < 1e-12 and R.rel_err(ref["running_var"], bn.running_var) < 1e-12


def test_input_batchnorm_against_fp64(gpu):
    check_bn(gpu, R.bn0_case(*R.BN0_CASE), False, "bn0 B=%d T=%d" % R.BN0_CASE)


@pytest.mark.parametrize("B,T", R.BN0_EDGE_CASES)
def test_input_batchnorm_edges_against_fp64(gpu, B, T):
    check_bn(gpu, R.bn0_case(B, T), False, "bn0 B=%d T=%d" % (B, T))


# ---- pool backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,W,C,ties", R.POOL_CASES)
def test_maxpool_backward_against_fp64(gpu, B, W, C, ties):
    check_pool(gpu, B, 1, W, C, ties)


@pytest.mark.parametrize("B,H,W,C,ties", R.POOL_EDGE_CASES)
def test_maxpool_backward_edges_against_fp64(gpu, B, H, W, C, ties):
    check_pool(gpu, B, H, W, C, ties)


def check_pool(gpu, B, H, W, C, ties):
    lib, _lib, ops = _env()
    x, dy = R.pool_case(B, W, C, ties=ties, H=H)
    gap = R.pool_gap(x)
    m = 100 * 6e-8 * float(x.abs().max())         # the pool forward copies values: fp32 rounding is its only error
    assert bool(((gap >= m) | (gap == 0 if ties else torch.zeros_like(gap, dtype=torch.bool))).all())
    if ties:
        assert bool((gap == 0).any()) and float(gap[0, 0, 0, 0]) == 0.0 and float(x[0, 0, 0, 0]) > 0
    ref = R.pool_backward(x.shape, R.pool_argmax(x), dy)
    x_d = dev(x, gpu).requires_grad_(True)
    old = ops.CONV_STACK_SENTINEL
    ops.CONV_STACK_SENTINEL = NAN
    try:
        out = ops.maxpool_w3s2(x_d)
        (dx,) = torch.autograd.grad(out, [x_d], dev(dy, gpu))
    finally:
        ops.CONV_STACK_SENTINEL = old
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx).all())
    assert torch.equal(out.detach().cpu().double(), encoder_ref.maxpool_w3s2(x))
    # the launch itself into a guarded dx: the same bits, nothing outside
    whole, dx2 = guarded(tuple(x.shape), C, gpu)
    dy_d = dev(dy, gpu)
    _lib.check(lib.s2i_maxpool_w3s2_backward(_lib.ptr(x_d.detach()), _lib.ptr(dy_d), B, H, W, C, _lib.ptr(dx2), _lib.stream()),
               "s2i_maxpool_w3s2_backward")
    torch.cuda.synchronize()
    assert_guarded(whole, dx2, "pool dx")
    assert torch.equal(dx2, dx)
    report([("pool_dx", "pool dx B=%d H=%d W=%d C=%d ties=%s" % (B, H, W, C, ties), R.rel_err(dx, ref))])


# ---- one block as ops.temporal_conv_bn_relu runs it ------------------------------------------------------------------------------
def _block_id(c):
    return "%dto%d_%s_B%d_Wo%d" % (c[0], c[1], "first" if c[2] is None else "k%ds%d" % c[2][:2], c[3], c[4])


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=_block_id)
def test_block_forward_and_backward_against_fp64_with_replayed_mask(gpu, case):
    """Convolution with its statistics epilogue, finalize, apply; the backward in fp64 with the GPU's ReLU mask replayed.
    B and Wo (the first layer: T) as conv_case builds them, W = Wo x stride."""
    lib, _lib, ops = _env()
    cin, cout, geom, B, Wo = case
    inputs = R.block_case(*case)
    x, w, gamma, beta, dout, running = inputs
    own = R.block_all(*inputs, geom, torch.float64)
    weight = w[:, :, 0].reshape(cout, 1, cin, 1) if geom is None else w.unsqueeze(2)
    leaves = [dev(t, gpu).requires_grad_(True) for t in (x, weight, gamma, beta)]
    rm, rv = dev(running[0], gpu), dev(running[1], gpu)
    nbt = torch.tensor(running[2], dtype=torch.int64, device=gpu)
    old = ops.CONV_STACK_SENTINEL
    ops.CONV_STACK_SENTINEL = NAN
    try:
        out = ops.temporal_conv_bn_relu(*leaves, (rm, rv, nbt), geom)
        grads = torch.autograd.grad(out, leaves, dev(dout, gpu))
    finally:
        ops.CONV_STACK_SENTINEL = old
    torch.cuda.synchronize()
    got = dict(out=out.detach(), dx=grads[0], dw=grads[1], dgamma=grads[2], dbeta=grads[3], running_mean=rm, running_var=rv)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert tuple(out.shape) == (B, 1, Wo, cout) and int(nbt) == own["nbt"] == running[2] + 1
    mask = (out.detach() > 0).cpu()
    flip = mask != own["mask"]
    m = 100 * (BOUNDS["block_out"] / 2) * float(own["z"].abs().max())
    outside = int((flip & ~(own["z"].abs() < m)).sum())
    print("%s: %d of %d decisions differ from the fp64 forward's, %d outside m = %.2e" % (_block_id(case), int(flip.sum()),
                                                                                        flip.numel(), outside, m))
    assert outside == 0, "a decision differs where fp64 is not within m of the kink"
    assert int(flip.sum()) <= FLIP_CAP * flip.numel()
    ref = R.block_all(*inputs, geom, torch.float64, mask=mask)
    report(R.block_errs(got, ref, _block_id(case)))


# ---- the whole stack ------------------------------------------------------------------------------------------------------------
_STACK = {}


def stack_gpu_run(gpu, net_gpu, mel, dfeat):
    """ops.conv_stack_train forward + backward with NaN-prefilled buffers -> features, gradients by name, the logged
    decisions (masks, pool argmax positions) in layer order."""
    _, _lib, ops = _env()
    old = ops.CONV_STACK_SENTINEL, ops.CONV_STACK_LOG
    ops.CONV_STACK_SENTINEL, ops.CONV_STACK_LOG = NAN, []
    try:
        feat = ops.conv_stack_train(net_gpu.Conv, dev(mel, gpu))
        names = [n for n, _ in net_gpu.Conv.named_parameters()]
        grads = torch.autograd.grad(feat, list(net_gpu.Conv.parameters()), dev(dfeat, gpu))
        log = list(ops.CONV_STACK_LOG)
    finally:
        ops.CONV_STACK_SENTINEL, ops.CONV_STACK_LOG = old
    torch.cuda.synchronize()
    decisions = []
    for kind, a, out in log:
        decisions.append(None if kind == "bn0" else ((out > 0).cpu() if kind == "block" else R.pool_argmax(a.cpu())))
    return feat.detach(), {"Conv." + n: g for n, g in zip(names, grads)}, decisions


def stack_setup(gpu):
    if "ref" not in _STACK:
        net = R.stack_net(bidirectional=True, nhidden=512)
        mel = R.mel_case(*R.STACK_CASE)
        layers = R.stack_layers(net)
        f64, c64 = R.stack_forward(layers, mel)
        _STACK["ref"] = (net, mel, layers, f64, c64, R.stack_dfeat(f64.shape))
    return _STACK["ref"]


def test_conv_stack_train_against_fp64_with_replayed_decisions(gpu):
    import copy
    net, mel, layers, f64, c64, dfeat = stack_setup(gpu)
    net_gpu = copy.deepcopy(net).to(gpu)
    feat, grads, decisions = stack_gpu_run(gpu, net_gpu, mel, dfeat)
    assert bool(torch.isfinite(feat).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert len(decisions) == len(layers) and tuple(feat.shape) == (4, 1, 2, 1024)
    rep = R.decision_report(layers, c64, decisions, R.stack_z_margins(c64, YARD_Z))
    for i, kind, n, flipped, outside in rep:
        print("layer %d %s: %d of %d decisions differ from the fp64 forward's, %d outside the margin" % (i, kind, flipped, n, outside))
    assert all(outside == 0 for _, _, _, _, outside in rep), "a decision differs where fp64 is not within m of the kink"
    assert all(flipped <= FLIP_CAP * n for _, _, n, flipped, _ in rep)
    g64, _ = R.stack_backward(layers, c64, dfeat, decisions)
    errs = [("stack_feat", "features", R.rel_err(feat, f64))]
    assert set(grads) == set(R.grad_names(g64))
    for n in R.grad_names(g64):
        cls = {"Conv.0.weight": "stack_bn0_dgamma", "Conv.0.bias": "stack_bn0_dbeta"}.get(n, "stack_grad")
        errs.append((cls, "d " + n, R.grad_err(n, grads[n], g64)))
    run = R.running_state(layers, c64)
    sd = net_gpu.state_dict()
    for n, v in run.items():
        if n.endswith("num_batches_tracked"):
            assert int(sd[n]) == int(v) == 1, n
        else:
            errs.append(("stack_running", n, R.rel_err(sd[n], v)))
    report(errs)


def test_conv_stack_backward_is_bit_identical_from_run_to_run(gpu):
    import copy
    net, mel, layers, f64, c64, dfeat = stack_setup(gpu)
    runs = []
    for _ in range(2):
        feat, grads, _ = stack_gpu_run(gpu, copy.deepcopy(net).to(gpu), mel, dfeat)
        runs.append((feat, grads))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


# ---- EncoderTrainer -------------------------------------------------------------------------------------------------------------
def test_encoder_trainer_steps_follow_the_fp64_trajectory(gpu):
    import copy
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer, HeadTrainer
    net = R.stack_net(bidirectional=True, nhidden=512)
    mel, lens, image, label = R.trainer_case()
    ref_losses, _ = R.trajectory(net, mel, lens, image, label, R.TRAINER_STEPS, torch.float64, **R.TRAINER_LOSS)
    model = copy.deepcopy(net).to(gpu)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trainer = EncoderTrainer(model, **R.TRAINER_LOSS)
    mel_d = dev(mel, gpu)
    errs = []
    for step in range(R.TRAINER_STEPS):
        got = trainer.step(mel_d, lens, image.float(), label)
        for k in ("loss", "loss_jel", "loss_l1"):
            errs.append(("traj_loss", "step %d %s (%.6f)" % (step, k, float(got[k])),
                         abs(float(got[k]) - float(ref_losses[step][k])) / abs(float(ref_losses[step]["loss"]))))
    assert not model.training
    after = model.state_dict()
    same = [n for n, _ in model.named_parameters() if torch.equal(after[n], before[n])]
    assert not same, "parameters the steps left unchanged: %s" % same
    assert int(after["Conv.0.num_batches_tracked"]) == R.TRAINER_STEPS
    # the inference path must fold the running statistics training has produced (not a stale cache)
    emb = trainer.embed(mel_d, lens)
    cpu_model = copy.deepcopy(model).cpu()
    _, sent = encoder_ref.encode(encoder_ref.fold(cpu_model), mel, lens)
    assert_close(emb, sent, rtol=1e-3, atol=1e-5, what="embedding after %d steps" % R.TRAINER_STEPS)
    stale = copy.deepcopy(net)
    stale.load_state_dict({k: (v if "running" not in k else before[k].cpu()) for k, v in cpu_model.state_dict().items()})
    _, sent_stale = encoder_ref.encode(encoder_ref.fold(stale), mel, lens)
    assert R.rel_err(sent_stale, sent) > 1e-2, "stale running statistics would not show in this test"
    # HeadTrainer on the same model still leaves the conv stack alone
    conv_before = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith("Conv.")}
    HeadTrainer(model, **R.TRAINER_LOSS).step(mel_d, lens, image.float(), label)
    conv_after = model.state_dict()
    assert all(torch.equal(conv_after[k], v) for k, v in conv_before.items())
    report(errs)
