"""Every non-matrix launch of the train step, at its production shape, against a plain fp64 reference.

The BatchNorm, activation, layout, loss and optimiser kernels of csrc/s2i_bn.hip, s2i_layout.hip, s2i_cvec.hip,
s2i_losses.hip and s2i_optim.hip pick their variants from the
launch's shape (finalize: small kernel up to 8 partial rows per group, else the shuffle or LDS reduction; bf16 forward:
8- or 4-channel row kernel; backward apply: the walker with its rows per block; colreduce: the row chunks per group), so
they are tested at the shapes the step really launches:

  * census: one eager train_step of each BASELINE workload (config 2: fp32, batch 24; config 4: bf16 activations, batch
    48) with ops._lib_ready() returning a proxy that records every call into the library that is not a matrix launch
    (tests/step_launches.json owns those): the entry point, every scalar argument and, for each pointer, whether it is
    NULL.  The deduplicated records are tests/step_elementwise_launches.json; test_census_matches_committed_file fails on
    any new or vanished record.  Regenerate it with `python tests/test_step_elementwise_gpu.py`.
  * replay: every record re-run through the same entry point on fresh seeded operands, compared element by element with
    tests/elementwise_ref.py: |out - ref| <= rnd * |ref| + gamma * absref, rnd = 2^-8 for a bf16 output and 0 for fp32,
    absref = the same operation on |operands| where the operation is a sum, a stated magnitude for sigmoid, exp and log
    terms.  Activations are drawn the way the kernels store them (bf16 activations as bf16); BatchNorm inputs lie on the
    bf16 grid and scale / shift are small dyadic numbers, so scale * y + shift is exact in fp32 and a LeakyReLU decision
    is the reference's.  Scales are negative in some channels and differ per group.  Copies and roundings (layouts, casts,
    counters, every element outside the slice an entry point writes) must be bit-identical.
  * chain: each recorded bn_act_bwd_reduce also runs reduce -> bwd_finalize -> apply against the fp64 backward.
  * power: every comparison must FAIL against deliberately wrong references (a group using group 0's coefficients, a
    missing row chunk, GLU halves swapped, LeakyReLU decided on y, top / bottom border classes swapped, accumulate as
    assign, Adam's bias correction one step off, the biased var in the running var, two bce_multi weights swapped,
    diagonal pairs in the class-aware loss, ...); the module lists every rejected mutation.
  * edges: a short list of shapes that reach planner branches the step may not (see EDGE_* below).

Measured on one MI355X: each mode has 30-32 entry points; fp32_b24 makes 374 library calls per step (215 distinct
records), bf16_b48 404 (221).  Worst ratios (gamma = about twice the worst, see GAMMA; the module prints them): BatchNorm
finalize 2.7e-7, backward finalize 6.2e-8, forward apply 8.2e-8, backward reduce 2.1e-7, backward apply 2.0e-7, chained
backward 1.2e-7, tap sums 1.5e-8, broadcast-channel table 4.9e-8 and gradients 3.3e-7, losses and heads <= 2.1e-7, Adam
2.0e-7.  No kernel bug was found.  The module runs in about 20 s.
"""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import elementwise_replay as ER  # noqa: E402
import launch_harness as LH  # noqa: E402
from launch_harness import P  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import (ACT_GLU, ACT_LRELU, ACT_NONE, ACT_RELU,  # noqa: E402
                                                                ACT_TANH, DT_BF16, DT_F32)

pytestmark = pytest.mark.gpu

CENSUS_FILE = os.path.join(HERE, "step_elementwise_launches.json")

MODES = LH.STEP_MODES

LEDGER = LH.Ledger()


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("elementwise replay")


# ---- census ----------------------------------------------------------------------------------------------------------
def _install_recorder(mp, recs):
    """ops._lib_ready() hands out a proxy that records every call into the library that is not a matrix launch."""
    LH.install(mp, LH.LibRecorder(_lib.load(), recs, ER.ARGS, ER.is_matrix, skip=ER.NOT_RECORDED))


def take_census(gpu):
    return LH.take_step_census(gpu, MODES, _install_recorder)


def test_census_matches_committed_file(gpu):
    live, calls = take_census(gpu)
    for mode, recs in live.items():
        print("census %s: %d library calls per step, %d distinct records" % (mode, calls[mode], len(recs)))
    LH.assert_census_equal(live, LH.load_census(CENSUS_FILE), MODES, "step_elementwise_launches.json")


# ---- replay ----------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for mode, recs in LH.load_census(CENSUS_FILE).items():
        for i, rec in enumerate(recs):
            out.append(pytest.param(mode, i, id="%s-%03d-%s" % (mode, i, rec["fn"][4:])))
    return out


@pytest.mark.parametrize("mode,index", _cases())
def test_replay_matches_fp64(gpu, mode, index):
    rec = LH.load_census(CENSUS_FILE)[mode][index]
    ER.run(rec, "%s[%d] %s" % (mode, index, rec["fn"]), LEDGER)


def _chain_cases():
    return [pytest.param(mode, i, id="%s-%03d" % (mode, i)) for mode, recs in LH.load_census(CENSUS_FILE).items()
            for i, rec in enumerate(recs) if rec["fn"] == "s2i_bn_act_bwd_reduce_dt"]


def _derived(rec):
    """The bwd_finalize and apply launches that follow a reduce launch (ops.ConvBnAct.backward)."""
    fin = dict(fn="s2i_bn_bwd_finalize", nparts=rec["nparts"], groups=rec["groups"], C=rec["C"],
               count=rec["M"] // rec["groups"])
    app = dict(fn="s2i_bn_act_bwd_apply_dt", dtype=rec["dtype"], lddout=rec["lddout"], M=rec["M"], groups=rec["groups"],
               C=rec["C"], act=rec["act"])
    return fin, app


@pytest.mark.parametrize("mode,index", _chain_cases())
def test_bn_backward_chain_matches_fp64(gpu, mode, index):
    recs = LH.load_census(CENSUS_FILE)[mode]
    rec = recs[index]
    for want in _derived(rec):
        assert any(all(r.get(k) == v for k, v in want.items()) for r in recs), \
            "%s: the launch that follows reduce[%d] is not in the census: %s" % (mode, index, want)
    ER.run(rec, "%s[%d] chain" % (mode, index), LEDGER, ER.run_bn_chain)


# ---- edges beyond the census -------------------------------------------------------------------------------------------
def _fin(nparts, G, C, count=4096, rs=True, nbt=True):
    return dict(fn="s2i_bn_finalize", nparts=nparts, groups=G, C=C, count=count, gamma=True, beta=True,
                running_mean=rs, running_var=rs, nbt=nbt, momentum=float(ctypes.c_float(0.1).value),
                eps=float(ctypes.c_float(1e-5).value), out=True, part=True)


def _bfin(nparts, G, C, count=4096, acc=1):
    return dict(fn="s2i_bn_bwd_finalize", nparts=nparts, groups=G, C=C, count=count, dgamma=True, dbeta=True,
                accumulate=acc, red2=True, part=True)


def _bn(fn, dt, M, G, C, act, ldd=None, nparts=None, residual=False):
    r = dict(fn=fn, dtype=dt, M=M, groups=G, C=C, act=act, y=True, coef=True)
    cout = C // 2 if act == ACT_GLU else C
    if fn != "s2i_bn_act_forward_dt":
        r.update(dout=True, lddout=ldd or cout)
    if nparts:
        r.update(nparts=nparts, part=True)
    if fn == "s2i_bn_act_forward_dt":
        r.update(residual=residual, out=True)
    return r


# finalize: ppg 8 | 9 (small / large kernel); Q = C / 4 not a multiple of qpb (C = 132: qpb 2) on the LDS path
# (lpg * qpb % 64 != 0); the shuffle path (C = 64, one group, ppg 100: lpg 128, qpb 1); G = 1, 2, 3; NULL running stats
# and NULL num_batches_tracked
EDGE_FINALIZE = [
    _fin(8, 1, 64), _fin(9, 1, 64), _fin(24, 3, 64), _fin(27, 3, 64),
    _fin(9 * 3, 3, 132), _fin(100, 1, 64), _fin(200, 2, 64), _fin(64 * 3, 3, 1024),
    _fin(27, 3, 132, rs=False, nbt=False), _fin(8, 2, 36, rs=False, nbt=True), _fin(9, 1, 36, rs=True, nbt=False),
    _bfin(8, 1, 64), _bfin(9, 1, 64), _bfin(27, 3, 132), _bfin(100, 1, 64, acc=0), _bfin(200, 2, 64),
]
# walker / colreduce: rows per group (517, 1037) not a multiple of the rows per trip; lddout > C (a channel-slice dout);
# bf16 forward with Cout % 8 == 4 (the 4-channel row kernel); G = 1, 2, 3
EDGE_BN = [
    _bn("s2i_bn_act_bwd_reduce_dt", DT_F32, 3 * 517, 3, 32, ACT_GLU, nparts=3 * 8),
    _bn("s2i_bn_act_bwd_apply_dt", DT_F32, 3 * 517, 3, 32, ACT_GLU),
    _bn("s2i_bn_act_bwd_reduce_dt", DT_BF16, 2 * 1037, 2, 64, ACT_LRELU, ldd=96, nparts=2 * 16),
    _bn("s2i_bn_act_bwd_apply_dt", DT_BF16, 2 * 1037, 2, 64, ACT_LRELU, ldd=96),
    _bn("s2i_bn_act_bwd_reduce_dt", DT_F32, 1037, 1, 48, ACT_NONE, ldd=64, nparts=16),
    _bn("s2i_bn_act_bwd_apply_dt", DT_F32, 1037, 1, 48, ACT_NONE, ldd=64),
    _bn("s2i_bn_act_forward_dt", DT_BF16, 3 * 517, 3, 36, ACT_LRELU),
    _bn("s2i_bn_act_forward_dt", DT_BF16, 2 * 517, 2, 36, ACT_NONE, residual=True),
    _bn("s2i_bn_act_forward_dt", DT_BF16, 3 * 517, 3, 72, ACT_GLU),
    _bn("s2i_bn_act_forward_dt", DT_F32, 2 * 517, 2, 36, ACT_LRELU, residual=True),
]


@pytest.mark.parametrize("rec", EDGE_FINALIZE + EDGE_BN, ids=lambda r: "%s-M%s-G%d-C%d-p%s" % (
    r["fn"][4:], r.get("M", "-"), r["groups"], r["C"], r.get("nparts", "-")))
def test_edge_shape_matches_fp64(gpu, rec):
    ER.run(rec, "edge %s" % LH.canon(rec), LEDGER)
    if rec["fn"] == "s2i_bn_act_bwd_reduce_dt":
        ER.run(rec, "edge chain %s" % LH.canon(rec), LEDGER, ER.run_bn_chain)


def _finalize_threads():
    cur = ctypes.c_int(0)
    _lib.check(_lib.load().s2i_get_tuning(b"finalize_threads", ctypes.byref(cur)), "s2i_get_tuning")
    return cur.value


@pytest.mark.parametrize("threads", [64, 1024])
def test_finalize_thread_cap(gpu, threads):
    """The finalize geometry with its thread cap (S2I_TUNE_FINALIZE_THREADS) at both ends, restored afterwards."""
    before = _finalize_threads()
    with _lib.tuning(finalize_threads=threads):
        assert _finalize_threads() == threads
        for rec in (_fin(27, 3, 132), _fin(200, 2, 64), _fin(64 * 3, 3, 1024), _bfin(100, 1, 64), _bfin(27, 3, 132)):
            ER.run(rec, "finalize_threads=%d %s" % (threads, LH.canon(rec)), LEDGER)
    assert _finalize_threads() == before, "finalize_threads not restored"


@pytest.mark.parametrize("n", [1001, 1002, 1003, 1004])
def test_adam_tail(gpu, n):
    """The float4 body plus the scalar tail (n % 4 = 1, 2, 3), host step and device step count, gscale != 1."""
    dev = torch.device("cuda:0")
    chk = LH.Check("adam n=%d" % n, ER.GAMMA, LEDGER)
    with torch.no_grad():
        ER.run_adam(ER.Ops(torch.Generator(device=dev).manual_seed(n), dev), chk, n, 2e-4, 0.5, 0.999, 1e-8, 4, False, 0.5)
        ER.run_adam(ER.Ops(torch.Generator(device=dev).manual_seed(n + 1), dev), chk, n, 2e-4, 0.5, 0.999, 1e-8, 0, True, 1.0)
    chk.done()


@pytest.mark.parametrize("n", [5, 1023])
def test_cast_refuses_ragged_length(gpu, n):
    """s2i_cast requires n % 4 == 0: anything else is refused and the destination stays untouched."""
    lib = _lib.load()
    for sdt, ddt in ((torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)):
        src = torch.randn(n, device="cuda").to(sdt)
        dst = torch.full((n + 4,), 7.0, device="cuda").to(ddt)
        before = dst.clone()
        code = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}
        rc = lib.s2i_cast(P(src), code[sdt], P(dst), code[ddt], n, _lib.stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.s2i_last_error(), (n, sdt)
        assert torch.equal(dst, before)


# ---- refused activations -----------------------------------------------------------------------------------------------
BAD_BN_ACTS = [ACT_TANH, ACT_RELU, 7, -1]
BAD_ACT_BWD = [ACT_RELU, ACT_GLU, ACT_NONE, 9, -1]


def _refused(rc, act, out, before):
    lib = _lib.load()
    torch.cuda.synchronize()
    msg = (lib.s2i_last_error() or b"").decode()
    assert rc != 0, "act %d accepted" % act
    assert str(act) in msg, "act %d: s2i_last_error() = %r" % (act, msg)
    assert torch.equal(out, before), "act %d: the output buffer was written" % act


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
@pytest.mark.parametrize("act", BAD_BN_ACTS)
def test_bn_entry_points_refuse_activation(gpu, dt, act):
    lib = _lib.load()
    M, G, C = 512, 2, 64
    t = ER.tdt(dt)
    y, dout = torch.randn(M, C, device="cuda").to(t), torch.randn(M, C, device="cuda").to(t)
    coef = torch.randn(G, 4, C, device="cuda")
    red2 = torch.randn(G, 2, C, device="cuda")
    st = _lib.stream()
    out = torch.full((M, C), 3.0, device="cuda").to(t)
    _refused(lib.s2i_bn_act_forward_dt(dt, P(y), M, G, C, P(coef), act, None, P(out), st), act, out, out.clone())
    part = torch.full((2, 16, C), 3.0, device="cuda")
    _refused(lib.s2i_bn_act_bwd_reduce_dt(dt, P(y), P(dout), C, M, G, C, P(coef), act, P(part), 16, st), act, part,
             part.clone())
    _refused(lib.s2i_bn_act_bwd_apply_dt(dt, P(y), P(dout), C, M, G, C, P(coef), P(red2), act, P(out), st), act, out,
             out.clone())
    if dt == DT_F32:
        _refused(lib.s2i_bn_act_forward(P(y), M, G, C, P(coef), act, None, P(out), st), act, out, out.clone())
        _refused(lib.s2i_bn_act_bwd_reduce(P(y), P(dout), C, M, G, C, P(coef), act, P(part), 16, st), act, part,
                 part.clone())
        _refused(lib.s2i_bn_act_bwd_apply(P(y), P(dout), C, M, G, C, P(coef), P(red2), act, P(out), st), act, out,
                 out.clone())


@pytest.mark.parametrize("dt", [DT_F32, DT_BF16])
@pytest.mark.parametrize("act", BAD_ACT_BWD)
def test_act_backward_refuses_activation(gpu, dt, act):
    lib = _lib.load()
    M, C = 256, 32
    t = ER.tdt(dt)
    o, d = torch.randn(M, C, device="cuda").to(t), torch.randn(M, C, device="cuda").to(t)
    dy = torch.full((M, C), 3.0, device="cuda").to(t)
    _refused(lib.s2i_act_backward_dt(dt, P(o), P(d), C, M, C, act, P(dy), _lib.stream()), act, dy, dy.clone())
    if dt == DT_F32:
        _refused(lib.s2i_act_backward(P(o), P(d), C, M, C, act, P(dy), _lib.stream()), act, dy, dy.clone())


if __name__ == "__main__":
    # regenerate tests/step_elementwise_launches.json (or the path given) from one eager step of each workload
    _lib.load()
    _lib.require_device()
    census, calls = take_census(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else CENSUS_FILE
    LH.write_census(path, census)
    for mode, recs in census.items():
        print("census %s: %d library calls per step, %d distinct records -> %s" % (mode, calls[mode], len(recs), path))
