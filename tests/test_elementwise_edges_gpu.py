"""The loss, head, layout and optimiser kernels of the train step off the shapes the step records, against fp64.

tests/test_step_elementwise_gpu.py replays every non-matrix launch of the step at its production shape; its edge lists go
off those shapes only for BatchNorm.  The other entry points (csrc/s2i_layout.hip, s2i_cvec.hip, s2i_losses.hip,
s2i_optim.hip, colstats / act_backward / glu of s2i_bn.hip) are recorded at one operating point, and their thread
layouts, segment counts and loop trips follow from it.  tests/elementwise_edges.py derives what that leaves unreached and
holds the table of the smallest shapes that reach it; tests/test_elementwise_edges_cpu.py checks the derivation and the
reference on the host.  Here:

  * replay: every record of the table through elementwise_replay.run, with the gammas of ER.GAMMA (one moved, see below).
  * guards: every output of a replay (Ops.full, Ops.guard; the census replays of the other suites as well) is a view
    between two 256-byte margins of a fixed bit pattern, and the workspaces of tap_sums, spatial_sum and cvec_bias_table
    are guarded at exactly the size the library asks for; Check.done() compares the margins as integers.
  * power: beside the mutations each replayer already carried, the references with H and W exchanged (tap_sums,
    cvec_bias_table), the last row band / segment / row chunk left out (tap_sums, spatial_sum, colstats), the images from
    256 on left out of dx, dw and dbias (logit_backward), the items from 256 on left out of the one-block reductions
    (bce, bce_multi, cal_loss, kl), the last Cc % 4 channels left out (cvec_bias_table) and the channels from 64 on left
    out of dc (cvec_grads) must all fail the bound; the pad channels of nchw_to_nhwc are compared as integers with +0.
  * class-aware loss: its two inactive branches (no same-label pair; diff <= 0) must give exactly 0 and an all-zero dS,
    with and without accumulation; all labels equal holds the fp64 value.
  * refusals: bad arguments return non-zero, set s2i_last_error() and leave output and margins untouched.
  * twins: the fp32 entry points without _dt give bit-identical results on the same operands.
  * the ragged production batch: one eager train_step of each workload at B = 23 (the last batch of a CUB epoch) is
    recorded into tests/ragged_elementwise_launches.json (regenerate it with `python tests/test_elementwise_edges_gpu.py`);
    every record that is not a BatchNorm launch (EDGE_BN / EDGE_FINALIZE of test_step_elementwise_gpu own those) is
    replayed, none capped.

Measured on one MI355X, worst ratio per family (table | B = 23 census | production worst of ER.GAMMA's comments, bound;
the module prints the first two):

    act_backward   8.8e-8 | 8.8e-8 | 8.9e-8  (1.8e-7)        cvec_table    9.8e-8 | 3.9e-8 | 4.9e-8  (1e-7)
    axpby          6.0e-8 | 5.9e-8 | 5.9e-8  (1.2e-7)        ema           1.2e-7 | 1.2e-7 | 1.2e-7  (2.4e-7)
    bce            1.9e-7 | 1.2e-7 | 1.6e-7  (3.3e-7)        logit         1.9e-7 | 1.8e-7 | 2.1e-7  (4.2e-7)
    ca_net         8.6e-8 | 1.2e-7 | 1.4e-7  (3e-7)          scale_dev     6.0e-8 | 5.9e-8 | 6.0e-8  (1.2e-7)
    cal_loss       3.8e-8 | 4.4e-8 | 3.6e-8  (7.5e-8)        spatial_sum   1.5e-7 | 9.3e-8 | 1.1e-7  (2.2e-7)
    colstats       2.4e-7 | 1.5e-7 | 1.7e-7  (3.4e-7)        tap_sums      1.6e-7 | 1.4e-8 | 1.5e-8  (3.2e-7)
    cvec_grads     1.6e-7 | 2.6e-7 | 3.3e-7  (6.6e-7)        adam               - | 2.0e-7 | 2.0e-7  (4e-7)

No kernel was found wrong.  One constant moved, GAMMA["tap_sums"], from 3e-8 to 3.2e-7.  Its absref is the image's total
|dy|; on the step's 64 x 64 and 128 x 128 maps that total is ~60 times the result, and the old bound, measured there, lay
below one fp32 rounding of a small map's result: the 2 x 2, 3 x 7, 34 x 6 and 4 x 4 (C = 1028) records gave 7.5e-8, 8.2e-8,
4.3e-8 and 1.6e-7 = 2.7 x 2^-24.  From the kernel's summation order (a lane adds its pixels one after another, lane 0 adds
the other lanes' sums, stage 2 adds the S bands, then total - row - column + corner) a tap sum carries at most
(pixels per lane - 1) + (occupied lanes - 1) + (S - 1) + 3 roundings, each at most 2^-24 of the total |dy|: 18 x 2^-24 = 1.1e-6
for the 4 x 4 map at C = 1028, where one lane adds all 16 pixels.  The same order restated in fp32 on the host
(test_elementwise_edges_cpu.test_tap_sums_bound_is_explained_by_rounding) gives 1.1e-7, 7.9e-8, 3.8e-8 and 1.9e-7 on these
shapes, the worst of four draws each, and 1.5e-8 at 64 x 64 x 128, so rounding explains the figures; the new constant is
twice the worst over census and table.

Mutations rejected on the table (cases), beside those each replayer carried before: tap_sums H and W exchanged (5), last
row band left out (7); cvec_table H and W exchanged (4), last Cc % 4 channels left out (4); spatial_sum last segment left
out (6); colstats last row chunk left out (4); logit images from 256 on left out (6: dx, dw, dbias); bce items from 256 on
left out (3, bce_multi among them); cal_loss items from 256 on left out (3); ca_net (kl) items from 256 on left out (2);
cvec_grads channels from 64 on left out (2).  254 tests, none skipped and no record capped; about 11 s, of which 6.6 s
are the two B = 23 train steps of the census test.
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

import elementwise_edges as E  # noqa: E402
import elementwise_ref as R  # noqa: E402
import elementwise_replay as ER  # noqa: E402
import launch_harness as LH  # noqa: E402
from helpers import CASES  # noqa: E402
from launch_harness import P  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import DT_F32  # noqa: E402

pytestmark = pytest.mark.gpu

CENSUS_FILE = os.path.join(HERE, "ragged_elementwise_launches.json")
RAGGED_MODES = {
    "fp32_b23": (dict(CASES["full3_fwd"], B=23), False),
    "bf16_b23": (dict(CASES["full3_fwd"], B=23), True),
}

EDGE_LEDGER = LH.Ledger()
RAGGED_LEDGER = LH.Ledger()


@pytest.fixture(scope="module", autouse=True)
def _report():
    EDGE_LEDGER.start()
    RAGGED_LEDGER.start()
    yield
    EDGE_LEDGER.report("elementwise edge table replay")
    RAGGED_LEDGER.report("ragged batch (B = 23) elementwise replay")


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(E.EDGES)), ids=[E.record_id(i, r) for i, r in enumerate(E.EDGES)])
def test_edge_record_matches_fp64(gpu, index):
    rec = E.EDGES[index]
    ER.run(rec, "edge[%d] %s" % (index, E.record_id(index, rec)), EDGE_LEDGER)


# mutation -> the table records (fn, key scalars) it must be rejected on, and how many comparisons reject it there
LISTED_MUTANTS = {
    "tap_sums: H and W exchanged": (dict(fn="s2i_tap_sums_dt", H=9, W=5), 1),
    "tap_sums: last row band of each image left out": (dict(fn="s2i_tap_sums_dt", H=34, W=6), 1),
    "cvec_table: H and W exchanged": (dict(fn="s2i_cvec_bias_table", Cc=5), 1),
    "cvec_table: last Cc % 4 channels left out": (dict(fn="s2i_cvec_bias_table", Cc=130), 1),
    "spatial_sum: last segment of each image left out": (dict(fn="s2i_spatial_sum_dt", HW=4097), 1),
    "colstats: last row chunk left out": (dict(fn="s2i_colstats", M=1037), 1),
    "logit: images from 256 on left out": (dict(fn="s2i_logit_backward", B=257), 3),       # dx, dw and dbias
    "bce: items from 256 on left out": (dict(fn="s2i_bce_forward", B=257), 1),
    "cal_loss: items from 256 on left out": (dict(fn="s2i_cal_loss", B=17), 1),
    "ca_net: items from 256 on left out": (dict(fn="s2i_kl_forward", B=7), 1),
    "cvec_grads: channels from 64 on left out": (dict(fn="s2i_cvec_grads", Cc=70), 1),
}


def _find(want):
    hits = [r for r in E.EDGES if all(r.get(k) == v for k, v in want.items())]
    assert len(hits) == 1, (want, len(hits))
    return hits[0]


@pytest.mark.parametrize("mutation", sorted(LISTED_MUTANTS))
def test_listed_mutant_is_rejected(gpu, mutation):
    """A replay raises when its bound cannot see one of its mutations; this asserts that the mutation was there to be seen."""
    want, count = LISTED_MUTANTS[mutation]
    ledger = LH.Ledger()
    ER.run(_find(want), "mutant %s" % mutation, ledger)
    assert ledger.rejected.get(mutation, 0) == count, (mutation, ledger.rejected)


def test_bce_multi_mutant_above_one_stride(gpu):
    ledger = LH.Ledger()
    ER.run(_find(dict(fn="s2i_bce_multi_forward", B=130)), "mutant bce_multi", ledger)
    assert ledger.rejected.get("bce: items from 256 on left out", 0) == 1, ledger.rejected


# ---- the class-aware loss off its active branch --------------------------------------------------------------------------
def _run_cal(chk, S, labels, D, acc, loss0=0.375):
    dev = S.device
    o = ER.Ops(None, dev, chk)
    B = S.shape[0]
    loss = o.guard(torch.tensor([loss0], device=dev)) if acc else o.full((1,))
    dS = o.full((B, B))
    LH.call("s2i_cal_loss", P(S), P(labels), B, D, P(loss), acc, P(dS))
    return loss, dS


def _pairs(labels):
    B = labels.numel()
    return (labels.view(-1, 1) == labels.view(1, -1)) & ~torch.eye(B, dtype=torch.bool, device=labels.device)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("case", ["labels distinct", "diff < 0"])
def test_cal_loss_inactive_is_exactly_zero(gpu, case, B, acc):
    dev = torch.device("cuda:0")
    if case == "labels distinct":
        labels = torch.arange(B, dtype=torch.int32, device=dev)
        S = torch.randn(B, B, generator=LH.gen_key(dev, "cal", B), device=dev)
    else:
        labels = (torch.arange(B, device=dev) % 2).to(torch.int32)
        S = 4.0 * _pairs(labels).float()                # same-label off-diagonal scores 4, everything else 0
        assert float(S.double().mean() - S.double()[_pairs(labels)].mean()) < 0
    chk = LH.Check("cal_loss %s B=%d acc=%d" % (case, B, acc), ER.GAMMA, EDGE_LEDGER)
    loss, dS = _run_cal(chk, S, labels, 64, acc)
    assert loss.view(torch.int32).item() == torch.tensor([0.375 if acc else 0.0]).view(torch.int32).item(), float(loss)
    assert not dS.view(torch.int32).any(), "dS is not all +0"
    chk.done()


@pytest.mark.parametrize("acc", [0, 1])
def test_cal_loss_all_labels_equal(gpu, acc):
    dev = torch.device("cuda:0")
    B, D = 17, 64
    X = torch.randn(B, D, generator=LH.gen_key(dev, "cal equal"), device=dev).double()
    S = (X @ X.t()).float()
    labels = torch.full((B,), 3, dtype=torch.int32, device=dev)
    chk = LH.Check("cal_loss all labels equal acc=%d" % acc, ER.GAMMA, EDGE_LEDGER)
    loss, dS = _run_cal(chk, S, labels, D, acc)
    Sd = S.double()
    lref, dref = R.cal_loss(Sd, labels, D)
    assert float(lref) > 0
    n = B * B - B
    labs = (Sd.abs().mean() + Sd.abs()[_pairs(labels)].sum() / n) / D
    base = 0.375 if acc else 0.0
    ml, md = R.cal_loss(Sd, labels, D, count_diagonal=True)       # then every pair counts: diff = 0, the loss inactive
    chk.close("cal_loss", "loss", loss, base + lref.view(1), labs + base, 0.0, {"diagonal pairs counted": base + ml.view(1)})
    chk.close("cal_loss", "dS", dS, dref, torch.full_like(dref, 2 * (1.0 / (B * B) + 1.0 / n) / D), 0.0,
              {"diagonal pairs counted": md})
    chk.done()


# ---- refusals ------------------------------------------------------------------------------------------------------------
class _Refusal:
    """Outputs filled with 3.0 between guard margins; refused() asserts rc != 0, a message, and that nothing was written."""

    def __init__(self, what):
        self.dev = torch.device("cuda:0")
        self.chk = LH.Check(what, ER.GAMMA, EDGE_LEDGER)
        self.o = ER.Ops(LH.gen_key(self.dev, what), self.dev, self.chk)
        self.lib = _lib.load()
        self.st = _lib.stream()

    def out(self, *shape):
        return self.o.full(shape, value=3.0)

    def refused(self, rc, *outs):
        torch.cuda.synchronize()
        assert rc != 0, "%s: accepted" % self.chk.what
        assert self.lib.s2i_last_error(), "%s: no message" % self.chk.what
        for t in outs:
            assert bool((t == 3.0).all()), "%s: the output was written" % self.chk.what
        self.chk.done()


@pytest.mark.parametrize("case", ["H = 1", "W = 1", "C = 6", "workspace one byte short"])
def test_tap_sums_refuses(gpu, case):
    r = _Refusal("tap_sums " + case)
    B, H, W, C = {"H = 1": (1, 1, 4, 4), "W = 1": (1, 4, 1, 4), "C = 6": (1, 4, 4, 6)}.get(case, (1, 34, 6, 64))
    dy = r.o.randn((B, H, W, C + 2))                    # operands with room to spare: only the arguments are at fault
    need = E.border_sums_workspace_bytes(B, H, W, C)
    ws, out = r.out(E.border_sums_workspace_bytes(B, H, W, C + 2) // 4), r.out(B, 9, C + 2)
    nbytes = need - 1 if case == "workspace one byte short" else ws.numel() * 4
    for rc in (r.lib.s2i_tap_sums_dt(DT_F32, P(dy), B, H, W, C, P(out), P(ws), nbytes, r.st),
               r.lib.s2i_tap_sums(P(dy), B, H, W, C, P(out), P(ws), nbytes, r.st)):
        r.refused(rc, out, ws)


@pytest.mark.parametrize("C,ld", [(6, 8), (4, 6), (8, 4)], ids=["C=6", "ld=6", "ld<C"])
def test_spatial_sum_refuses(gpu, C, ld):
    r = _Refusal("spatial_sum C=%d ld=%d" % (C, ld))
    B, HW = 2, 130
    src = r.o.randn((B * HW, 8))
    ws, out = r.out(B * E.spatial_segments(HW) * 8), r.out(B, 8)
    for rc in (r.lib.s2i_spatial_sum_dt(DT_F32, P(src), ld, B, HW, C, P(out), P(ws), ws.numel() * 4, r.st),
               r.lib.s2i_spatial_sum(P(src), ld, B, HW, C, P(out), P(ws), ws.numel() * 4, r.st)):
        r.refused(rc, out, ws)


def test_cvec_grads_refuses_dc_at_n_6(gpu):
    r = _Refusal("cvec_grads dc N=6")
    B, Cc, Ip, Op, N = 2, 5, 8, 8, 6
    cvec, packed, tapsum = r.o.randn((B, Cc)), r.o.randn((9, Ip, Op)), r.o.randn((B, 9, N))
    dc, dw = r.out(B, Cc), r.out(N, Cc, 3, 3)
    r.refused(r.lib.s2i_cvec_grads(P(cvec), P(packed), P(tapsum), B, Cc, Ip, Op, N, N, Cc, P(dc), P(dw), 0, r.st), dc, dw)


def test_bce_multi_refuses_five_heads(gpu):
    r = _Refusal("bce_multi H=5")
    G, H, B = 1, 5, 4
    probs = [r.o.rand((G * B,), 0.1, 0.9) for _ in range(H)]
    grads = [r.out(G * B) for _ in range(H)]
    target, weight, gout, loss = r.o.rand((G * H,)), r.o.rand((G * H,)), r.o.randn((1,)), r.out(1)
    arr = (ctypes.c_void_p * H)(*[P(p) for p in probs])
    garr = (ctypes.c_void_p * H)(*[P(g) for g in grads])
    r.refused(r.lib.s2i_bce_multi_forward(arr, P(target), P(weight), G, H, B, P(loss), r.st), loss)
    r.refused(r.lib.s2i_bce_multi_backward(arr, P(target), P(weight), G, H, B, P(gout), garr, r.st), *grads)


def test_colstats_refuses_no_parts(gpu):
    r = _Refusal("colstats nparts=0")
    y, part = r.o.randn((8, 4)), r.out(2, 1, 4)
    r.refused(r.lib.s2i_colstats(P(y), 8, 4, 4, P(part), 0, r.st), part)


def test_adam_refuses_step_0_without_a_device_counter(gpu):
    r = _Refusal("adam step=0")
    g = r.o.randn((8,))
    p, m, v = r.out(8), r.out(8), r.out(8)
    r.refused(r.lib.s2i_adam_step(P(p), P(g), P(m), P(v), 8, 2e-4, 0.5, 0.999, 1e-8, 0, None, 1.0, r.st), p, m, v)


# ---- the fp32 twins without _dt --------------------------------------------------------------------------------------------
def _first(fn, **want):
    return [r for r in E.EDGES if r["fn"] == fn and all(r[k] == v for k, v in want.items())][0]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("fn", ["s2i_tap_sums", "s2i_spatial_sum", "s2i_nchw_to_nhwc", "s2i_nhwc_to_nchw",
                                "s2i_act_backward"])
def test_fp32_twin_is_bit_identical(gpu, fn):
    dev = torch.device("cuda:0")
    chk = LH.Check("twin " + fn, ER.GAMMA, EDGE_LEDGER)
    o = ER.Ops(LH.gen_key(dev, fn), dev, chk)
    lib, st = _lib.load(), _lib.stream()
    if fn == "s2i_tap_sums":
        rec = _first(fn + "_dt", dtype=DT_F32, H=34)
        B, H, W, C = rec["B"], rec["H"], rec["W"], rec["C"]
        dy = o.randn((B, H, W, C))
        n = E.border_sums_workspace_bytes(B, H, W, C)
        outs = [o.full((B, 9, C)) for _ in range(2)]
        rcs = [lib.s2i_tap_sums_dt(DT_F32, P(dy), B, H, W, C, P(outs[0]), P(o.full((n // 4,))), n, st),
               lib.s2i_tap_sums(P(dy), B, H, W, C, P(outs[1]), P(o.full((n // 4,))), n, st)]
    elif fn == "s2i_spatial_sum":
        rec = _first(fn + "_dt", dtype=DT_F32, HW=130)
        B, HW, C, ld = rec["B"], rec["HW"], rec["C"], rec["ld"]
        src = o.randn((B * HW, ld))
        n = E.spatial_sum_workspace_bytes(B, HW, C)
        outs = [o.full((B, C)) for _ in range(2)]
        rcs = [lib.s2i_spatial_sum_dt(DT_F32, P(src), ld, B, HW, C, P(outs[0]), P(o.full((n // 4,))), n, st),
               lib.s2i_spatial_sum(P(src), ld, B, HW, C, P(outs[1]), P(o.full((n // 4,))), n, st)]
    elif fn == "s2i_nchw_to_nhwc":
        rec = _first(fn + "_dt", dtype=DT_F32, Cp=8, C=3)
        B, C, H, W, Cp = rec["B"], rec["C"], rec["H"], rec["W"], rec["Cp"]
        src = o.randn((B, C, H, W))
        outs = [o.full((B, H, W, Cp)) for _ in range(2)]
        rcs = [lib.s2i_nchw_to_nhwc_dt(DT_F32, P(src), P(outs[0]), B, C, H, W, Cp, st),
               lib.s2i_nchw_to_nhwc(P(src), P(outs[1]), B, C, H, W, Cp, st)]
    elif fn == "s2i_nhwc_to_nchw":
        rec = _first(fn + "_dt", dtype=DT_F32, lds=12)
        B, C, H, W, lds = rec["B"], rec["C"], rec["H"], rec["W"], rec["lds"]
        src = o.randn((B * H * W, lds))
        outs = [o.full((B, C, H, W)) for _ in range(2)]
        rcs = [lib.s2i_nhwc_to_nchw_dt(DT_F32, P(src), lds, P(outs[0]), B, C, H, W, st),
               lib.s2i_nhwc_to_nchw(P(src), lds, P(outs[1]), B, C, H, W, st)]
    else:
        rec = _first(fn + "_dt", dtype=DT_F32, M=23, act=E.ACT_TANH)
        M, C, ldd, act = rec["M"], rec["C"], rec["lddout"], rec["act"]
        out, dout = torch.tanh(o.randn((M, C))), o.randn((M, ldd))
        outs = [o.full((M, C)) for _ in range(2)]
        rcs = [lib.s2i_act_backward_dt(DT_F32, P(out), P(dout), ldd, M, C, act, P(outs[0]), st),
               lib.s2i_act_backward(P(out), P(dout), ldd, M, C, act, P(outs[1]), st)]
    torch.cuda.synchronize()
    assert rcs == [0, 0], (rcs, lib.s2i_last_error())
    assert not torch.isnan(outs[0]).any(), "an element was not written"
    chk.equal("%s against %s_dt" % (fn, fn), _bits(outs[1]), _bits(outs[0]))
    chk.done()


# ---- the ragged production batch -------------------------------------------------------------------------------------
def _install_recorder(mp, recs):
    LH.install(mp, LH.LibRecorder(_lib.load(), recs, ER.ARGS, ER.is_matrix, skip=ER.NOT_RECORDED))


def take_census(gpu):
    return LH.take_step_census(gpu, RAGGED_MODES, _install_recorder)


def test_ragged_census_matches_committed_file(gpu):
    """One train step of each workload at B = 23."""
    live, calls = take_census(gpu)
    for mode, recs in live.items():
        print("census %s: %d library calls per step, %d distinct records" % (mode, calls[mode], len(recs)))
    LH.assert_census_equal(live, LH.load_census(CENSUS_FILE), RAGGED_MODES, "ragged_elementwise_launches.json")


def test_ragged_census_is_committed():
    census = LH.load_census(CENSUS_FILE)
    assert set(census) == set(RAGGED_MODES) and all(census[m] for m in RAGGED_MODES), \
        "tests/ragged_elementwise_launches.json is missing"


def _batchnorm(rec):
    return rec["fn"].startswith("s2i_bn_")


def _ragged_cases():
    return [pytest.param(mode, i, id="%s-%03d-%s" % (mode, i, rec["fn"][4:]))
            for mode, recs in LH.load_census(CENSUS_FILE).items() for i, rec in enumerate(recs) if not _batchnorm(rec)]


@pytest.mark.parametrize("mode,index", _ragged_cases())
def test_ragged_launch_replay_matches_fp64(gpu, mode, index):
    rec = LH.load_census(CENSUS_FILE)[mode][index]
    ER.run(rec, "%s[%d] %s" % (mode, index, rec["fn"]), RAGGED_LEDGER)


if __name__ == "__main__":
    # regenerate tests/ragged_elementwise_launches.json (or the path given) from one eager step of each workload at B = 23
    _lib.load()
    _lib.require_device()
    census, calls = take_census(torch.device("cuda:0"))
    path = sys.argv[1] if len(sys.argv) > 1 else CENSUS_FILE
    LH.write_census(path, census)
    for mode, recs in census.items():
        print("census %s: %d library calls per step, %d distinct records -> %s" % (mode, calls[mode], len(recs), path))
