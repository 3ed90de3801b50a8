"""The image-layer convolution kernels on every branch of their dispatch, against the fp64 reference of the launch-replay
suites.

The convolutions with 3 (4) channels on one side run on ten hand-written kernels (csrc/s2i_conv_thin.hip, small_n_conv_kernel
in s2i_conv_fwd.hip, small_n_wgrad_kernel in s2i_wgrad.hip) that plan_fwd / plan_wgrad choose between on shape and dtype
alone.  tests/test_image_layer_edges_cpu.py derives the branch of every launch of the step census and of
the B = 23 census: production runs the tile kernels (conv3_n4_tile<16|32>, tconv_n4_tile<64>), thin_in_kernel<16|32>,
rgb_in_kernel<1,3>, <2,3>, <2,4> and small_n_wgrad_kernel, all on square maps of 32 x 32 and larger with whole blocks and
without bias.  Asserted there:

  * the censuses never launch thin_out_kernel (either form), rgb_out_kernel<4|8|16|9|18|36>, rgb_in_kernel<1,4>,
    small_n_conv_kernel<16> or the N <= 4 matrix tile;
  * the two operator tests aimed at these layers (test_kernels_gpu.CONVACT, test_bf16_gpu.IMAGE_LAYERS) do launch
    rgb_out_kernel<8> and <36>, rgb_in_kernel<1,4> and small_n_conv_kernel<16>, compared at 1.5e-2 relative L2 or close().
    Neither they nor the censuses launch thin_out_kernel, rgb_out_kernel<4|16|9|18>, thin_in_kernel with a bf16 output or
    small_n_wgrad_kernel with bf16 activations.  (The network-level tests run the same dispatch on maps of 64 x 64 and
    larger; their launches were not derived.)

tests/image_layer_edges.py holds one hand-written record per branch and edge (pixel tails, H != W, the
odd last trip of the weight-gradient stream, strided grids, bias, N = 3 in rows of four, the first M that selects each
kernel); this module replays each through conv_replay.replay_conv / replay_wgrad under the default planner, with the same
bound |out - ref| <= rnd |ref| + gamma x absref and the unchanged constants conv_replay.GAMMA.

  * every output buffer that ops allocates during a replay is prefilled with a sentinel (torch.empty is wrapped), so a
    pixel that a kernel never wrote fails the comparison instead of reading as a lucky zero;
  * N = 3 records run with ldy = 4, which ops never does: they are launched through s2i_conv_forward_dt into a
    sentinel-filled buffer with a guard behind it; column 3 of every row and the guard must be bit-identical afterwards.
    The production form -- 3 real channels of an N = 4 launch -- must leave exact zeros in column 3, as ops.ConvAct promises;
  * power, besides the replay's dropped-channel and dropped-image mutants; each must be REJECTED by the bound: the last
    M % block pixels zeroed (pixtail); the reference computed with H and W exchanged (nonsquare, weight gradient too); output
    phases (0, 1) and (1, 0) exchanged (transposed convs); no bias (bias); one tap's weights zeroed -- for a transposed
    conv the four middle taps, one of each output phase's 2 x 2 (every record off the matrix tiles: a mis-built table or
    fragment).

Measured on one MI355X (worst ratio per class: this table | production worst recorded in conv_replay.py; bound):

    fp32 forward / input gradient   2.5e-7 | 4.8e-7   (2^-20 = 9.5e-7)
    fp32 weight gradient            6.1e-9 | 4.0e-7   (8e-7)
    bf16 forward / input gradient   5.1e-8 | 5.1e-8   (1e-7)
    bf16 weight gradient            4.1e-9 | 1.6e-7   (3.2e-7)

No class needed a wider bound and no kernel was found wrong: all 98 records hold the production constants.  The weight
gradients sit far below their bound because K x N = (9 Ca) x 4 sums are split over 512 slabs.  The 98 replays take about 3 s;
the pixel-tail mutant was rejected in all 29 replays that have one, H and W exchanged in all 31, exchanged phases in all 21,
the missing bias in all 5, the zeroed tap in all 75.  The one dead instantiation the table turned up, thin_in_kernel<64>
(thin_kind admits 16 and 32 outputs only), is removed from the library; small_n_conv_kernel<4> / <8> were reachable only by
a C caller that passed no workspace (tests/image_layer_edges.py); no plan names them now, and the last test below holds the
rule that replaced that fallback: a short workspace is refused.
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

import conv_edges as E  # noqa: E402
import conv_replay as C  # noqa: E402
import image_layer_edges as IE  # noqa: E402
import launch_harness as LH  # noqa: E402
import launch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
GUARD = 4096                                       # sentinel floats behind the last row of an n3 launch
LEDGER = LH.Ledger()
IDS = [IE.record_id(i, r) for i, r in enumerate(IE.RECORDS)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    LEDGER.start()
    yield
    LEDGER.report("image-layer table replay")


def _default_planner():
    from speech_to_image_translation_without_text_amd import ops
    assert ops.TILE_ROWS == 0 and ops.MATH_PLANES == 0, "the replay runs the default planner"
    assert os.environ.get("S2I_TUNE", "") == "", "the replay runs the default planner"


_torch_empty = torch.empty


def _sentinel_empty(made):
    """torch.empty for the duration of a replay: every floating-point tensor comes prefilled (workspaces and packed weights
    too, which is harmless: their kernels write all they read), and its shape and dtype are noted in `made` so that the
    test can tell the compared output was one of them."""
    def empty(*args, **kw):
        t = _torch_empty(*args, **kw)
        if t.is_floating_point():
            t.fill_(SENTINEL)
            made.append((tuple(t.shape), t.dtype))
        return t
    return empty


def _output_of(rec):
    if "x" in rec:
        from speech_to_image_translation_without_text_amd import ops
        B, H, W, _ = rec["x"][0]
        return ((B,) + tuple(ops._geom(rec["kind"], H, W)) + (rec["N"],),
                torch.bfloat16 if rec["out_dtype"] == "bf16" else torch.float32)
    return (tuple(rec["grad_shape"]), torch.float32)


def _launch_ldy(rec, stash, contract=None):
    """Stands in for ops.conv_raw / conv_any for a record with ldy > N: the same descriptor with the record's row stride,
    launched through s2i_conv_forward_dt into a sentinel-filled buffer.  Returns the N written columns as a view.
    contract = a FWD_KERNELS name: the launch gets exactly the workspace s2i_conv_plan_query asks for and must be planned
    onto that kernel; before it, the same call four bytes short must be refused and write nothing."""
    from speech_to_image_translation_without_text_amd import _lib, ops

    def run(kind, x, *args, bias=None, out_dtype=torch.float32, **kw):
        packed, N = args[-2], args[-1]
        assert out_dtype == torch.float32 and N == rec["N"] and kw.get("cls_bias") is None and not kw.get("stats")
        lib = _lib.load()
        _lib.require_device()
        B, H, W, _ = x.shape
        Ho, Wo = ops._geom(kind, H, W)
        ldy = rec["ldy"]
        d = E.conv_desc(rec, ldy=ldy)
        n = B * Ho * Wo * ldy
        buf = torch.full((n + GUARD,), SENTINEL, device=x.device)
        ws_bytes = max(lib.s2i_conv_workspace_bytes(ctypes.byref(d)), 16)
        if contract is not None:
            told = _lib.conv_plan(d, ops._dt(x), _lib.DT_F32, 0, bias is not None)
            assert told["kernel"] == contract and 4 < told["ws_bytes"] <= ws_bytes and told["ws_bytes"] % 4 == 0, told
            ws_bytes = told["ws_bytes"]
        ws = _torch_empty((ws_bytes // 4,), device=x.device)

        def launch(y, nbytes):
            return lib.s2i_conv_forward_dt(ctypes.byref(d), x.data_ptr(), ops._dt(x), None, packed.data_ptr(), LH.P(bias), None,
                                           y.data_ptr(), _lib.DT_F32, None, ws.data_ptr(), nbytes, _lib.stream())
        if contract is not None:
            untouched = torch.full((n + GUARD,), float("nan"), device=x.device)
            assert launch(untouched, ws_bytes - 4) != 0, "a workspace four bytes short was accepted"
            assert b"workspace" in lib.s2i_last_error(), lib.s2i_last_error()
            torch.cuda.synchronize()
            assert bool(torch.isnan(untouched).all()), "the refused launch wrote into y"
            stash["refused"] = True
        _lib.check(launch(buf, ws_bytes), "s2i_conv_forward_dt")
        torch.cuda.synchronize()
        stash.update(buf=buf, y=buf[:n].view(B, Ho, Wo, ldy))
        return stash["y"][..., :N], None, 0
    return run


# ---- power checks ----------------------------------------------------------------------------------------------------
def _swap_hw(t):
    """NCHW view of the NHWC memory of t read with H and W exchanged."""
    B, Cc, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, W, H, Cc).permute(0, 3, 1, 2)


def _conv_extra(plan, stash):
    def extra(ctx):
        rec, bad = ctx["rec"], []
        out, ref = ctx["out"], ctx["ref"]
        B, N, Ho2, Wo2 = ref.shape
        M, nph = plan["M"], plan["nphases"]

        def must_fail(name, mref):
            if LH.fails(out, mref, ctx["absref"], ctx["rnd"], ctx["gamma"]):
                LEDGER.reject("%s: %s" % (ctx["cls"], name))
            else:
                bad.append("the bound cannot see: %s" % name)

        def reference(x=ctx["x"], W=ctx["W"], bias=ctx["bias"]):
            return R.act(C.conv_ref(rec, ctx["op"], ctx["layer"], x, None, W, ctx["Op"], None, bias)[1], rec["act"])

        if "pixtail" in rec["reach"]:
            tail = M % plan["ppb"]
            assert tail
            if nph == 4:      # a row of the GEMM is one input pixel: the 2 x 2 outputs of its four phases
                r = ref.reshape(B, N, Ho2 // 2, 2, Wo2 // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(M, -1).clone()
                r[M - tail:] = 0
                mref = r.view(B, Ho2 // 2, Wo2 // 2, N, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, N, Ho2, Wo2)
            else:
                r = ref.permute(0, 2, 3, 1).reshape(M, N).clone()
                r[M - tail:] = 0
                mref = r.view(B, Ho2, Wo2, N).permute(0, 3, 1, 2)
            must_fail("the last M %% %d pixels zeroed" % plan["ppb"], mref)
        if "nonsquare" in rec["reach"]:
            y = reference(x=_swap_hw(ctx["x"]))
            must_fail("H and W exchanged", y.permute(0, 2, 3, 1).reshape(B, Ho2, Wo2, N).permute(0, 3, 1, 2))
        if nph == 4:
            mref = ref.clone()
            mref[:, :, 0::2, 1::2] = ref[:, :, 1::2, 0::2]
            mref[:, :, 1::2, 0::2] = ref[:, :, 0::2, 1::2]
            must_fail("output phases (0, 1) and (1, 0) exchanged", mref)
        if rec["bias"]:
            must_fail("no bias", reference(bias=None))
        if plan["branch"] not in ("n4-igemm", "igemm"):
            W2 = ctx["W"].clone()
            if nph == 4:
                W2[:, :, 1:3, 1:3] = 0                   # taps (1|2, 1|2): one of the 2 x 2 taps of each output phase
            else:
                W2[:, :, 1, -1] = 0
            must_fail("one tap's weights zeroed", reference(W=W2))
        # the padding column
        oihw = rec["w"]["oihw"]
        real = oihw[0] if rec["wmode"] == 0 else oihw[1]
        if real == 3 and N == 4 and not rec["bias"]:
            if not bool((out[:, 3] == 0).all()):
                bad.append("column 3 of the NHWC4 rows is not exactly zero")
        if "n3" in rec["reach"]:
            if not bool((stash["y"][..., 3] == SENTINEL).all()):
                bad.append("column 3 of rows with ldy = 4 written by an N = 3 launch")
            if not bool((stash["buf"][stash["y"].numel():] == SENTINEL).all()):
                bad.append("rows after the last pixel written")
        return bad
    return extra


def _wgrad_extra(plan):
    def extra(ctx):
        rec, bad = ctx["rec"], []
        if "nonsquare" in rec["reach"]:
            O, I = rec["grad_shape"][:2]
            mref = ctx["base"] + R.wgrad(ctx["layer"], _swap_hw(ctx["a"])[:, :I], _swap_hw(ctx["g"])[:, :O], ctx["kh"])
            if LH.fails(ctx["got"], mref, ctx["absref"], ctx["rnd"], ctx["gamma"]):
                LEDGER.reject("%s: H and W exchanged" % ctx["cls"])
            else:
                bad.append("the bound cannot see: H and W exchanged")
        return bad
    return extra


# ---- the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(IE.RECORDS)), ids=IDS)
def test_image_layer_replay_matches_fp64(gpu, index):
    from speech_to_image_translation_without_text_amd import ops
    _default_planner()
    rec = IE.RECORDS[index]
    what = IDS[index]
    plan = IE.plan(rec)
    assert plan["reach"] == set(rec["reach"]), (what, plan)
    stash, made = {}, []
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "empty", _sentinel_empty(made))
        if "ldy" in rec:
            mp.setattr(ops, "conv_raw", _launch_ldy(rec, stash))
            mp.setattr(ops, "conv_any", _launch_ldy(rec, stash))
        if rec["fn"].startswith("conv"):
            C.replay_conv(rec, LH.gen_rec(gpu, rec), gpu, what, LEDGER, extra=_conv_extra(plan, stash))
        else:
            C.replay_wgrad(rec, LH.gen_rec(gpu, rec), gpu, what, LEDGER, extra=_wgrad_extra(plan))
    if "ldy" not in rec:
        assert _output_of(rec) in made, "%s: the output was not allocated through the sentinel wrapper: %s" % (what, made)
    torch.cuda.empty_cache()


def test_short_workspace_is_refused_and_the_planned_one_suffices(gpu):
    """The plan never looks at the workspace.  GET_IMAGE_G's 3x3 to 3 channels in rows of four floats, one 64 x 64 image of
    16 channels (M = 4096, the smallest M the thin kernels take), is planned onto conv3_n4_tile_kernel<16>, the parent's
    branch tile3-16, whatever the caller passes: four bytes under the planned workspace the call returns non-zero, names the
    workspace and leaves a NaN-filled y untouched (it used to run silently on another kernel); with exactly the planned
    bytes it holds the fp64 bound of the table above."""
    from speech_to_image_translation_without_text_amd import ops
    from speech_to_image_translation_without_text_amd._lib import ACT_TANH
    _default_planner()
    rec = IE.fwd("k3s1", 1, 64, 64, 16, 3, "one 64 x 64 image: the workspace contract", ["tile3-16", "n3", "threshold"], act=ACT_TANH,
                 N=3, ldy=4)
    plan = IE.plan(rec)
    assert plan["reach"] == set(rec["reach"]) and plan["M"] == 4096, plan
    stash = {}
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "empty", _sentinel_empty([]))
        mp.setattr(ops, "conv_raw", _launch_ldy(rec, stash, contract="conv3-n4-16"))
        mp.setattr(ops, "conv_any", _launch_ldy(rec, stash, contract="conv3-n4-16"))
        C.replay_conv(rec, LH.gen_rec(gpu, rec), gpu, "workspace-contract", LEDGER, extra=_conv_extra(plan, stash))
    assert stash.get("refused"), "the replay did not go through the contract launch"
