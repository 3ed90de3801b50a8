"""Host-side operators of the MI355X StackGAN-v2 path: torch.autograd.Functions whose forward and
backward are calls into the C-ABI kernels of include/s2i_hip.h (through _lib.py).

Each Function stands in for a group of stock torch ops of the reference
(StackGAN_v2/model.py:112-551, StackGAN_v2/trainer.py:54-58, 298-311, 394-409):

  ConvBnAct   conv (1x1 / 3x3 / 4x4-s2 / nearest-x2+3x3) + BatchNorm(train) + GLU|LeakyReLU|none
              (+ residual add): upBlock, Block3x3_relu, ResBlock halves, downBlock,
              Block3x3_leakRelu, INIT_STAGE_G.fc
  ConvAct     conv + bias + LeakyReLU|tanh|none: first D conv, GET_IMAGE_G, CA_NET.fc
  Glu2d, Reparam, KLLoss        CA_NET encode / reparametrize, KL_loss
  LogitHead, BCELoss, ClassAwareLoss   logits / uncond_logits + nn.BCELoss, class_aware_loss
  ToNHWC / ToNCHW               layout changes at the module boundary
  LstmSentence, EncoderLoss     the speech encoder's LSTM head and loss (Audio_to_Image/train_audio_encoder.py)
  TemporalConvBnRelu, InputBatchNorm, MaxPoolW3S2, conv_stack_train   its conv stack in training mode
  score_rows, topk_rows         one gallery chunk's scores and their fold into a running top k (retrieval.Gallery)
  rank_rows                     the same scores folded into rank counters of one designated row (Gallery.rank)

Activations between these ops are NHWC; parameters stay in the reference's OIHW layout and are
re-packed to the kernels' layout when their version counter changes.  There is no CPU fallback.
"""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import (ACT_GLU, ACT_LRELU, ACT_NONE, CONV_K1, CONV_K3S1, CONV_K4S2, DT_BF16, DT_F32,
                   PACK_PLAIN, PACK_UPFOLD, TCONV_K4S2, ConvDesc, WgradDesc, check, ptr, stream)

BN_EPS = 1e-5
BN_MOMENTUM = 0.1

# When True (set by the fused trainer), parameter gradients are accumulated by the kernels straight into
# `param.grad` (the flat gradient buffer's views) and backward returns None for them: no temporary
# gradient tensors, no autograd AccumulateGrad add kernels.  Requires zeroed, pre-attached `.grad`.
DIRECT_PARAM_GRAD = False


def _direct(p):
    return (DIRECT_PARAM_GRAD and p is not None and p.requires_grad and p.grad is not None
            and p.grad.is_contiguous())


class param_grad_mode:
    """Scope of the module-level switch: `with param_grad_mode(direct=True): ...` turns the direct accumulation into
    `.grad` on for the body and restores the previous value afterwards, so a later stock-optimiser use of the same
    modules in this process sees the default (autograd-returned gradients)."""

    def __init__(self, direct=True):
        self.new = bool(direct)

    def __enter__(self):
        global DIRECT_PARAM_GRAD
        self.old = DIRECT_PARAM_GRAD
        DIRECT_PARAM_GRAD = self.new
        return self

    def __exit__(self, *exc):
        global DIRECT_PARAM_GRAD
        DIRECT_PARAM_GRAD = self.old
        return False


def _lib_ready():
    lib = _lib.load()
    _lib.require_device()
    return lib


# ---- scratch ------------------------------------------------------------------------------------
class _Workspace:
    """One growable scratch buffer per (device, stream): kernels on a stream use it one after another, and two
    streams never share one.  Once a hipGraph has been captured (`pin_graph_resources`) a buffer that has to grow is
    replaced but never freed: the graph keeps writing split-K slabs through the raw pointer it captured."""

    def __init__(self):
        self.buf = {}
        self.pinned = False
        self.retired = []

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 16)
        key = (device, stream())     # the raw query: a Stream object per scratch request cost 8 us (tools/host_profile.py)
        cur = self.buf.get(key)
        if cur is None or cur.numel() * 4 < nbytes:
            if cur is not None and self.pinned:
                self.retired.append(cur)
            # during hipGraph capture the allocation comes from the graph's private pool and stays reserved for it
            cur = torch.empty((nbytes + 3) // 4 + 1024, dtype=torch.float32, device=device)
            self.buf[key] = cur
        return cur


_ws = _Workspace()


def pin_graph_resources():
    """Called before a hipGraph capture: everything a captured launch reaches through a raw pointer that lives outside
    the graph's own memory pool -- the per-stream workspaces, the device tables of the batched weight packs -- is kept
    alive for the rest of the process (replaced workspaces are retired, not freed; the table caches are no longer cleared)."""
    _ws.pinned = True


def invalidate_derived(params):
    """Drop every weight copy derived from the packed fp32 tensors of these parameters (bf16 stage layouts, split bf16
    planes): they are re-derived from the current packed weights on first use.  Needed before an eager step that follows
    hipGraph replays, which update the masters and re-pack on the device without running the host-side bookkeeping."""
    for p in params:
        packs = getattr(p, '_s2i_packs', None)
        if packs:
            for ent in packs.values():
                ent[0]._s2i_gen = getattr(ent[0], '_s2i_gen', 0) + 1


def _roundup4(v):
    return (v + 3) & ~3


# ---- packed weights ------------------------------------------------------------------------------
# OIHW parameter -> P[tap][Ip][Op].  The packed copy lives ON the parameter object (attribute
# `_s2i_packs`), so it dies with the parameter and can never be mistaken for another network's; it is
# refreshed when torch's version counter or the storage address changes, or explicitly after an update
# that bypasses the version counter (the fused Adam kernel).
def packed_weight(w, mode=0):
    packs = getattr(w, '_s2i_packs', None)
    if packs is None:
        packs = {}
        w._s2i_packs = packs
    ent = packs.get(mode)
    ver, addr = w._version, w.data_ptr()
    if ent is not None and ent[1] == ver and ent[2] == addr and ent[0].device == w.device:
        return ent[0]
    out = ent[0] if ent is not None and ent[0].device == w.device else None
    packed = pack_weight(w, mode, out=out)
    packs[mode] = (packed, ver, addr)
    return packed


_pack_tables = {}


def refresh_packed(params):
    """Re-pack every cached layout of these parameters in place -- one launch for the whole list (the table of
    (parameter, packed copy, shape) entries lives on the device and is rebuilt only when a pointer changes)."""
    entries = []
    for p in params:
        packs = getattr(p, '_s2i_packs', None)
        if packs:
            for mode, ent in list(packs.items()):
                if ent[0].device == p.device:
                    entries.append((p, mode, ent[0]))
                else:
                    del packs[mode]
    if not entries:
        return
    lib = _lib_ready()
    # the shape belongs to the key: the allocator hands the addresses of a dead network to the next one
    key = tuple((p.data_ptr(), p.shape, mode, out.data_ptr()) for p, mode, out in entries)
    tab = _pack_tables.get(key)
    if tab is None:
        items = (_lib.PackItem * len(entries))()
        block0, max_taps = 0, 1
        for k, (p, mode, out) in enumerate(entries):
            if p.dim() == 2:
                O, I, KH, KW = p.shape[0], p.shape[1], 1, 1
            else:
                O, I, KH, KW = p.shape
            Ip, Op = _roundup4(I), _roundup4(O)
            gx = (Op + 63) // 64          # 64-channel tiles (csrc/s2i_pack.hip::pack_tile)
            items[k] = _lib.PackItem(p.data_ptr(), out.data_ptr(), O, I, KH, KW, Ip, mode, gx, block0)
            block0 += gx * ((Ip + 7) // 8)
            max_taps = max(max_taps, KH * KW)
        raw = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(entries[0][0].device)
        tab = (key, raw, len(entries), block0, max_taps)
        # a captured graph reads its table through a raw pointer.  The oldest table goes, never all of them: a trainer's
        # warm-up step files one table per network, and the recording that follows must find every one of them (a table
        # built inside a recording would be a host-to-device copy on a capturing stream).
        while len(_pack_tables) > 64 and not _ws.pinned:
            del _pack_tables[next(iter(_pack_tables))]
        _pack_tables[key] = tab
    check(lib.s2i_pack_conv_weights_batched(ptr(tab[1]), tab[2], tab[3], tab[4], stream()), "s2i_pack_conv_weights_batched")
    for p, mode, out in entries:
        out._s2i_gen = getattr(out, '_s2i_gen', 0) + 1
        p._s2i_packs[mode] = (out, p._version, p.data_ptr())
    _refresh_bf16([out for _, _, out in entries])


_pack16_tables = {}


def _refresh_bf16(packed_list):
    """Every bf16 copy that was ever derived from these packed fp32 tensors (bf16_weight below) re-derived in ONE launch,
    instead of one 10 us launch per layer on its first use after the optimiser step (70 launches per step at config 4)."""
    recs = []
    for packed in packed_list:
        descs = getattr(packed, '_s2i_b16_desc', None)
        if descs:
            for key, (d, w_offset, ent) in descs.items():
                recs.append((packed, key, d, w_offset, ent))
    if not recs:
        return
    lib = _lib_ready()
    tkey = tuple((packed.data_ptr(), packed.shape, key, ent.data_ptr()) for packed, key, _, _, ent in recs)
    tab = _pack16_tables.get(tkey)
    if tab is None:
        items = (_lib.Pack16Item * len(recs))()
        block0 = 0
        for k, (packed, key, d, w_offset, ent) in enumerate(recs):
            nb = lib.s2i_pack16_item_fill(ctypes.byref(d), ptr(packed) + 4 * int(w_offset), packed.shape[1], packed.shape[2],
                                          ptr(ent), ctypes.byref(items[k]))
            if nb <= 0:
                check(1, "s2i_pack16_item_fill")
            items[k].block0 = block0
            block0 += nb
        raw = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(recs[0][0].device)
        tab = (raw, len(recs), block0)
        if len(_pack16_tables) > 64 and not _ws.pinned:
            _pack16_tables.clear()
        _pack16_tables[tkey] = tab
    check(lib.s2i_pack_conv_weights_bf16_batched(ptr(tab[0]), tab[1], tab[2], stream()), "s2i_pack_conv_weights_bf16_batched")
    for packed, key, d, w_offset, ent in recs:
        gen = getattr(packed, '_s2i_gen', 0)
        cache = getattr(packed, '_s2i_b16', None)
        if cache is None or cache[0] != gen:
            cache = (gen, {})
            packed._s2i_b16 = cache
        cache[1][key] = ent


def pack_weight(w, mode, out=None):
    lib = _lib_ready()
    w = w.detach()
    if w.dim() == 2:
        O, I, KH, KW = w.shape[0], w.shape[1], 1, 1
    else:
        O, I, KH, KW = w.shape
    if not w.is_contiguous():
        w = w.contiguous()
    T = 16 if mode == PACK_UPFOLD else KH * KW
    Ip, Op = _roundup4(I), _roundup4(O)
    if out is None or out.numel() != T * Ip * Op:
        out = torch.empty((T, Ip, Op), dtype=torch.float32, device=w.device)
    check(lib.s2i_pack_conv_weight(ptr(w), ptr(out), O, I, KH, KW, Ip, mode, stream()), "s2i_pack_conv_weight")
    out._s2i_gen = getattr(out, '_s2i_gen', 0) + 1  # invalidates the split-bf16 copies derived from it
    return out


# Matrix-product mode of the convolution GEMMs: 0 = native fp32 MFMA (default); 2 / 3 = operands split into that many
# bf16 planes (include/s2i_hip.h, "split-bf16 matrix products").  Opt-in: S2I_MATH_PLANES=2|3.
MATH_PLANES = int(os.environ.get("S2I_MATH_PLANES", "0"))


def split_weight(packed, planes, transpose):
    """bf16 planes of a packed weight tensor P[T][R][C], cached on the tensor object until it is re-packed.  Both operand
    layouts ([plane][T][R][C] for the input gradient, [plane][T][C][R] for the forward) come from one launch."""
    lib = _lib_ready()
    cache = getattr(packed, '_s2i_split', None)
    gen = packed._s2i_gen
    if cache is None or cache[0] != gen or cache[1] != planes:
        T, R, C = packed.shape
        rc, cr = (cache[2], cache[3]) if cache is not None and cache[1] == planes else (
            torch.empty((planes, T, R, C), dtype=torch.int16, device=packed.device),
            torch.empty((planes, T, C, R), dtype=torch.int16, device=packed.device))
        check(lib.s2i_split_packed_weight(ptr(packed), T, R, C, planes, ptr(rc), ptr(cr), stream()), "s2i_split_packed_weight")
        cache = (gen, planes, rc, cr)
        packed._s2i_split = cache
    return cache[3] if transpose else cache[2]


# ---- bf16 activation mode (BASELINE config 4) ------------------------------------------------------------------------
# ACT_BF16 = True (S2I_ACT_BF16=1, bench.py --math bf16): activations between the fused blocks are stored as bf16 NHWC,
# convolutions whose channel counts allow it run on the bf16 matrix cores from bf16 weights (s2i_conv_forward_bf16),
# BatchNorm statistics come from the fp32 accumulators, master weights / gradients / Adam / EMA stay fp32.  fp32 islands:
# CA_NET, INIT_STAGE_G's fc (+ BatchNorm1d), the NHWC4 image tensors, the logit heads and the losses.
ACT_BF16 = os.environ.get("S2I_ACT_BF16", "0") == "1"


def _dt(t):
    if t.dtype == torch.bfloat16:
        return DT_BF16
    if t.dtype != torch.float32:
        raise _lib.S2IError("activation tensors are fp32 or bf16, got %s" % t.dtype)
    return DT_F32


def cast(t, dtype):
    """Contiguous tensor in the other activation dtype (own kernel: torch is not on the product path for arithmetic)."""
    if t.dtype == dtype:
        return t
    lib = _lib_ready()
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=dtype, device=t.device)
    n = t.numel()
    if n % 4 != 0:
        raise _lib.S2IError("cast: %d elements (not a multiple of 4)" % n)
    check(lib.s2i_cast(ptr(t), _dt(t), ptr(out), _dt(out), n, stream()), "s2i_cast")
    return out


_B16_KERNEL, _B16_CK, _B16_PARTS, _B16_NPAD, _B16_W_ELEMS, _B16_WS_BYTES = (
    _lib.B16_PLAN_FIELDS.index(f) for f in ("kernel", "ck", "parts", "npad", "w_elems", "ws_bytes"))


def _bf16_plan(d):
    """The answers of s2i_conv_bf16_plan_query for descriptor d, read by index (_B16_*: no dict on the launch path), or None
    where the bf16 kernels do not take the layer: the plan refuses it or names no kernel.  The answer stays on the descriptor
    (d.b16_plan), so that conv_any and the bf16_weight it calls with d plan once between them."""
    out = (ctypes.c_longlong * 21)()
    if _lib_ready().s2i_conv_bf16_plan_query(ctypes.byref(d), ctypes.byref(out)) or out[_B16_KERNEL] < 0:
        out = None
    d.b16_plan = out
    return out


def bf16_weight(packed, d, w_offset):
    """bf16 weights of one convolution descriptor in the stage order of s2i_conv_forward_bf16, cached on the packed fp32
    tensor until it is re-packed (the fused Adam bumps `_s2i_gen`)."""
    lib = _lib_ready()
    plan = getattr(d, 'b16_plan', None) or _bf16_plan(d)
    if plan is None:
        raise _lib.S2IError("bf16_weight: the bf16 convolution kernels do not take this layer")
    cache = getattr(packed, '_s2i_b16', None)
    gen = getattr(packed, '_s2i_gen', 0)
    if cache is None or cache[0] != gen:
        cache = (gen, {})
        packed._s2i_b16 = cache
    key = (d.kind, d.wmode, d.flip, d.Cx, d.N, int(w_offset), plan[_B16_CK] | plan[_B16_NPAD] << 8)
    ent = cache[1].get(key)
    if ent is None:
        old = getattr(packed, '_s2i_b16_bufs', None)
        if old is None:
            old = packed._s2i_b16_bufs = {}
        ent = old.get(key)               # reuse the allocation across generations
        n = plan[_B16_W_ELEMS]
        if ent is None or ent.numel() != n:
            ent = torch.empty(n, dtype=torch.bfloat16, device=packed.device)
            old[key] = ent
        check(lib.s2i_pack_conv_weight_bf16(ctypes.byref(d), ptr(packed) + 4 * int(w_offset), packed.shape[1],
                                            packed.shape[2], ptr(ent), stream()), "s2i_pack_conv_weight_bf16")
        cache[1][key] = ent
        # remembered for the batched re-derivation after the next optimiser step (_refresh_bf16)
        descs = getattr(packed, '_s2i_b16_desc', None)
        if descs is None:
            descs = packed._s2i_b16_desc = {}
        dd = ConvDesc()
        ctypes.memmove(ctypes.byref(dd), ctypes.byref(d), ctypes.sizeof(ConvDesc))
        descs[key] = (dd, int(w_offset), ent)
    return ent


def conv_any(kind, x, packed, N, *, wmode=0, flip=0, bias=None, act=ACT_NONE, stats=False, groups=1, w_offset=0,
             cls_bias=None, out_dtype=torch.float32):
    """Convolution of an NHWC tensor of either activation dtype (no broadcast vector) -> (y, part, nparts).  bf16 in /
    bf16 out goes to the patch-staged bf16 kernel when the layer is eligible, everything else to the fp32-MFMA kernel
    reading / writing the given dtypes."""
    lib = _lib_ready()
    B, H, W, Cx = x.shape
    Ho, Wo = _geom(kind, H, W)
    wR, ldw = packed.shape[1], packed.shape[2]
    d = ConvDesc(kind, B, H, W, Cx, 0, N, wmode, flip, wR, ldw, act, 1 if stats else 0, N, groups,
                 1 if cls_bias is not None else 0, 0, 0, 0)
    y = torch.empty((B, Ho, Wo, N), dtype=out_dtype, device=x.device)
    # the one planning pass of a bf16 launch: eligibility, partial rows, weight layout and workspace are its answers
    plan = (_bf16_plan(d) if x.dtype == torch.bfloat16 and out_dtype == torch.bfloat16 and bias is None and act == ACT_NONE
            and N % 8 == 0 else None)
    fast = plan is not None
    if EXEC_LOG is not None:
        T = _TAPS[kind]
        _log_exec("conv%s k%d %s[%d,%d,%d,%d]->%d" % ("16" if fast else "", kind, "T" if wmode else "", B, H, W, Cx, N),
                  B * Ho * Wo, N, T * Cx, x.numel(), T * Cx * N * (4 if kind == TCONV_K4S2 else 1), y.numel(),
                  x.element_size(), y.element_size())
    part, nparts = None, 0
    if fast:
        if stats:
            nparts = plan[_B16_PARTS]
            part = torch.empty((2, nparts, N), dtype=torch.float32, device=x.device)
        wb = bf16_weight(packed, d, w_offset)
        ws = _ws.get(plan[_B16_WS_BYTES], x.device)
        check(lib.s2i_conv_forward_bf16(ctypes.byref(d), ptr(x), ptr(wb), ptr(cls_bias), ptr(y), ptr(part), ptr(ws),
                                        ws.numel() * 4, stream()), "s2i_conv_forward_bf16")
        return y, part, nparts
    if stats:
        nparts = lib.s2i_conv_stat_parts(ctypes.byref(d))
        if nparts <= 0:
            check(1, "s2i_conv_stat_parts")
        part = torch.empty((2, nparts, N), dtype=torch.float32, device=x.device)
    ws = _ws.get(lib.s2i_conv_workspace_bytes(ctypes.byref(d)), x.device)
    check(lib.s2i_conv_forward_dt(ctypes.byref(d), ptr(x), _dt(x), None, ptr(packed) + 4 * int(w_offset), ptr(bias),
                                  ptr(cls_bias), ptr(y), _dt(y), ptr(part), ptr(ws), ws.numel() * 4, stream()),
          "s2i_conv_forward_dt")
    return y, part, nparts


def wgrad_any(kind, a, g, grad_shape, *, swap=0, fold=0, out=None, accumulate=False, i_off=0, I_total=0):
    """Weight gradient from operands of either activation dtype (no broadcast vector) into an fp32 OIHW tensor."""
    lib = _lib_ready()
    B, H, W, Ca = a.shape
    N = g.shape[-1]
    if len(grad_shape) == 2:
        O, I, KH, KW = grad_shape[0], grad_shape[1], 1, 1
    else:
        O, I, KH, KW = grad_shape
    d = WgradDesc(kind, B, H, W, Ca, 0, N, N, swap, fold, O, I, KH, KW, 1 if accumulate else 0, i_off, I_total)
    if EXEC_LOG is not None:
        Ho, Wo = _geom(kind, H, W)
        _log_exec("wgrad%s k%d a[%d,%d,%d,%d] g%d" % ("16" if a.dtype == g.dtype == torch.bfloat16 else "", kind, B, H, W,
                                                      Ca, N), B * Ho * Wo, N, _TAPS[kind] * Ca, a.numel(), g.numel(),
                  _TAPS[kind] * Ca * N, a.element_size(), 4)
    if out is None:
        full = grad_shape if not I_total else (O, I_total, KH, KW)
        out = torch.empty(full, dtype=torch.float32, device=a.device)
    wsb = lib.s2i_wgrad_workspace_bytes_dt(ctypes.byref(d), _dt(a), _dt(g))
    if wsb == 0:
        check(1, "s2i_wgrad_workspace_bytes_dt")
    ws = _ws.get(wsb, a.device)
    check(lib.s2i_conv_wgrad_dt(ctypes.byref(d), ptr(a), _dt(a), None, ptr(g), _dt(g), ptr(out), ptr(ws), ws.numel() * 4,
                                stream()), "s2i_conv_wgrad_dt")
    return out


# ---- executed-work accounting ------------------------------------------------------------------------
# bench.py / tools set EXEC_LOG to a list for the duration of ONE step: every matrix-product launch appends
# (what, flops, bytes) with the multiply-add count the kernels really execute (2*M*N*K of the launched GEMM: up-blocks at
# 4 taps per output parity, folded c_code channels and skipped weight gradients NOT counted) and the operand + result
# bytes of the launch.  None (default) costs one comparison per launch.
EXEC_LOG = None
_TAPS = {CONV_K1: 1, CONV_K3S1: 9, CONV_K4S2: 16, TCONV_K4S2: 4}


def _log_exec(what, M, N, K, in_elems, w_elems, out_elems, esize_in=4, esize_out=4):
    if EXEC_LOG is not None:
        EXEC_LOG.append((what, 2.0 * M * N * K, in_elems * esize_in + w_elems * esize_in + out_elems * esize_out, M, N, K))


# ---- raw kernels ------------------------------------------------------------------------------------
def _geom(kind, H, W):
    if kind == CONV_K4S2:
        return H // 2, W // 2
    if kind == TCONV_K4S2:
        return 2 * H, 2 * W
    return H, W


# rows per block of the fp32 matrix kernel: 0 = the planner's choice; tools / tests set 96 or 128 to force a variant
TILE_ROWS = 0


# ---- deferred BatchNorm + activation ("apply-on-load") ------------------------------------------------------------------
# A block whose ONLY consumer is the next convolution can skip its normalise + LeakyReLU pass: ConvBnAct(..., defer=True)
# returns its activated tensor UNWRITTEN, tagged with the raw conv output y and the coefficient table; a consuming
# ConvBnAct gathers y through s2i_conv_forward_in (and s2i_conv_wgrad_in in its backward), which apply scale / shift /
# LeakyReLU while they stage the operand -- the activated tensor is never written or read.  Anything else that touches a
# tagged tensor goes through real(), which runs the skipped pass into the tensor's storage first.  Callers opt in per block
# (model.py: the discriminator towers' chains); fp32 tensors, LeakyReLU, training mode.
# MEASURED (round 3, one MI355X, batch 24): bit-for-rounding equal to the separate pass (tests/test_parity_gpu.py::
# test_apply_on_load_equals_the_separate_activation_pass) and SLOWER: 32.5 vs 31.65 ms per step.  The fp32 matrix kernels
# are bound by the matrix pipe, and an im2col gather sees every input element once per TAP: the fma + LeakyReLU + padding
# select run 9 - 16 times per element in the staging path between two barriers, which costs the 36 fused launches more
# (+7 %) than the 49 removed passes took (0.35 ms of HBM-bound kernels that overlapped other streams anyway).  Off by default
# (S2I_DEFER_ACT=1 turns it on); DESIGN.md section 13 has the byte accounting for the other block types.
DEFER_ACT = os.environ.get("S2I_DEFER_ACT", "0") == "1"


class _Lazy:
    __slots__ = ("y", "coef", "act", "groups", "done")

    def __init__(self, y, coef, act, groups):
        self.y, self.coef, self.act, self.groups, self.done = y, coef, act, groups, False


def real(x):
    """The tensor with its deferred BatchNorm + activation pass executed (no-op for ordinary tensors)."""
    lz = getattr(x, '_s2i_lazy', None)
    if lz is not None and not lz.done:
        lib = _lib_ready()
        C = lz.y.shape[-1]
        M = lz.y.numel() // C
        check(lib.s2i_bn_act_forward_dt(_dt(lz.y), ptr(lz.y), M, lz.groups, C, ptr(lz.coef), lz.act, None, ptr(x),
                                        stream()), "s2i_bn_act_forward")
        lz.done = True
    return x


def _pending(x):
    lz = getattr(x, '_s2i_lazy', None)
    return lz if (lz is not None and not lz.done) else None


def conv_raw(kind, x, cvec, packed, N, *, wmode=0, flip=0, wR, ldw, bias=None, act=ACT_NONE, stats=False, groups=1,
             w_offset=0, cls_bias=None, conv1d=None, in_src=None):
    """x: [B,H,W,Cx] contiguous NHWC.  Returns (y [B,Ho,Wo,N], part or None, nparts).
    w_offset (floats) skips leading weight rows (the c_code rows of a jointConv); cls_bias [B][9][N]
    adds their pre-reduced contribution per border class."""
    lib = _lib_ready()
    B, H, W, Cx = x.shape
    Cc = 0 if cvec is None else cvec.shape[1]
    Ho, Wo = _geom(kind, H, W)
    kw1, st1, pd1 = conv1d if conv1d is not None else (0, 0, 0)
    if conv1d is not None:
        Ho, Wo = H, (W + 2 * pd1 - kw1) // st1 + 1
    d = ConvDesc(kind, B, H, W, Cx, Cc, N, wmode, flip, wR, ldw, act, 1 if stats else 0, N, groups,
                 1 if cls_bias is not None else 0, kw1, st1, pd1, 128 if MATH_PLANES else TILE_ROWS,
                 in_src.act if in_src is not None else 0, in_src.groups if in_src is not None else 0)
    y = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=x.device)
    if EXEC_LOG is not None:
        T = kw1 if conv1d is not None else _TAPS[kind]
        # TCONV: Ho x Wo is the full-resolution output grid and every output pixel sees 4 taps
        _log_exec("conv k%d %s[%d,%d,%d,%d+%d]->%d" % (kind, "T" if wmode else "", B, H, W, Cx, Cc, N), B * Ho * Wo, N,
                  T * (Cx + Cc), x.numel(), T * (Cx + Cc) * N * (4 if kind == TCONV_K4S2 else 1), y.numel())
    part, nparts = None, 0
    if stats:
        nparts = lib.s2i_conv_stat_parts(ctypes.byref(d))
        if nparts <= 0:
            check(1, "s2i_conv_stat_parts")
        part = torch.empty((2, nparts, N), dtype=torch.float32, device=x.device)
    wsb = lib.s2i_conv_workspace_bytes(ctypes.byref(d))
    ws = _ws.get(wsb, x.device)
    if (MATH_PLANES and in_src is None and w_offset == 0 and packed.dim() == 3
            and getattr(packed, '_s2i_gen', None) is not None and lib.s2i_conv_split_eligible(ctypes.byref(d))):
        transpose = wmode == 0
        np_, kp = (packed.shape[2], packed.shape[1]) if transpose else (packed.shape[1], packed.shape[2])
        if kp % 8 == 0:
            wsp = split_weight(packed, MATH_PLANES, transpose)
            check(lib.s2i_conv_forward_split(ctypes.byref(d), ptr(x), ptr(cvec), ptr(wsp), MATH_PLANES, np_, kp, ptr(bias),
                                             ptr(cls_bias), ptr(y), ptr(part), ptr(ws), ws.numel() * 4, stream()),
                  "s2i_conv_forward_split")
            return y, part, nparts
    wp = ptr(packed) + 4 * int(w_offset)
    if in_src is not None:
        # x is the raw output of the producing block: its BatchNorm + LeakyReLU are applied while the operand is staged
        check(lib.s2i_conv_forward_in(ctypes.byref(d), ptr(x), ptr(in_src.coef), wp, ptr(y), ptr(part), ptr(ws),
                                      ws.numel() * 4, stream()), "s2i_conv_forward_in")
        return y, part, nparts
    check(lib.s2i_conv_forward_cls(ctypes.byref(d), ptr(x), ptr(cvec), wp, ptr(bias), ptr(cls_bias), ptr(y), ptr(part),
                                   ptr(ws), ws.numel() * 4, stream()), "s2i_conv_forward")
    return y, part, nparts


def wgrad_raw(kind, a, cvec, g, grad_shape, *, swap=0, fold=0, out=None, accumulate=False, i_off=0, I_total=0, a_src=None,
              g_cols=None):
    """Weight gradient into an OIHW tensor of shape grad_shape.  a: gathered NHWC, g: plain NHWC.
    With I_total > 0 only input channels [i_off, i_off + I) of a wider (O, I_total, KH, KW) tensor are written.
    g_cols = (first, count) takes a column slice of g in place (row stride g.shape[-1]; first a multiple of 4)."""
    lib = _lib_ready()
    B, H, W, Ca = a.shape
    Cc = 0 if cvec is None else cvec.shape[1]
    N = g.shape[-1]
    if g_cols is not None:
        return _wgrad_cols(kind, a, g, grad_shape, g_cols)
    if len(grad_shape) == 2:
        O, I, KH, KW = grad_shape[0], grad_shape[1], 1, 1
    else:
        O, I, KH, KW = grad_shape
    d = WgradDesc(kind, B, H, W, Ca, Cc, N, N, swap, fold, O, I, KH, KW, 1 if accumulate else 0, i_off, I_total,
                  a_src.act if a_src is not None else 0, a_src.groups if a_src is not None else 0)
    if EXEC_LOG is not None:
        Ho, Wo = _geom(kind, H, W)
        _log_exec("wgrad k%d a[%d,%d,%d,%d+%d] g%d" % (kind, B, H, W, Ca, Cc, N), B * Ho * Wo, N, _TAPS[kind] * (Ca + Cc),
                  a.numel(), g.numel(), _TAPS[kind] * (Ca + Cc) * N)
    if out is None:
        full = grad_shape if not I_total else (O, I_total, KH, KW)
        out = torch.empty(full, dtype=torch.float32, device=a.device)
    if a_src is not None:
        # `a` is the producer's raw output; eligibility was checked by the caller (s2i_conv_wgrad_in_eligible)
        wsb = lib.s2i_wgrad_workspace_bytes(ctypes.byref(d))
        if wsb == 0:
            check(1, "s2i_wgrad_workspace_bytes")
        ws = _ws.get(wsb, a.device)
        check(lib.s2i_conv_wgrad_in(ctypes.byref(d), ptr(a), ptr(a_src.coef), ptr(g), ptr(out), ptr(ws), ws.numel() * 4,
                                    stream()), "s2i_conv_wgrad_in")
        return out
    if MATH_PLANES:
        wsb = lib.s2i_wgrad_workspace_bytes_split(ctypes.byref(d), MATH_PLANES)
        if wsb == 0:
            check(1, "s2i_wgrad_workspace_bytes_split")
        ws = _ws.get(wsb, a.device)
        check(lib.s2i_conv_wgrad_split(ctypes.byref(d), MATH_PLANES, ptr(a), ptr(cvec), ptr(g), ptr(out), ptr(ws),
                                       ws.numel() * 4, stream()), "s2i_conv_wgrad_split")
        return out
    wsb = lib.s2i_wgrad_workspace_bytes(ctypes.byref(d))
    if wsb == 0:
        check(1, "s2i_wgrad_workspace_bytes")
    ws = _ws.get(wsb, a.device)
    check(lib.s2i_conv_wgrad(ctypes.byref(d), ptr(a), ptr(cvec), ptr(g), ptr(out), ptr(ws), ws.numel() * 4,
                             stream()), "s2i_conv_wgrad")
    return out


def _wgrad_cols(kind, a, g, grad_shape, g_cols):
    """wgrad_raw on the columns [first, first + count) of g, read through the descriptor's row stride."""
    lib = _lib_ready()
    B, H, W, Ca = a.shape
    first, N = g_cols
    ldg = g.shape[-1]
    if first % 4 or first < 0 or first + N > ldg or MATH_PLANES:
        raise _lib.S2IError("wgrad: column slice (%d, %d) of %d columns (fp32 matrix mode only)" % (first, N, ldg))
    O, I = grad_shape
    d = WgradDesc(kind, B, H, W, Ca, 0, N, ldg, 0, 0, O, I, 1, 1, 0, 0, 0, 0, 0)
    if EXEC_LOG is not None:
        _log_exec("wgrad k%d a[%d,%d,%d,%d] g%d" % (kind, B, H, W, Ca, N), B * H * W, N, Ca, a.numel(), B * H * W * N, Ca * N)
    out = torch.empty(grad_shape, dtype=torch.float32, device=a.device)
    wsb = lib.s2i_wgrad_workspace_bytes(ctypes.byref(d))
    if wsb == 0:
        check(1, "s2i_wgrad_workspace_bytes")
    ws = _ws.get(wsb, a.device)
    check(lib.s2i_conv_wgrad(ctypes.byref(d), ptr(a), None, ptr(g) + 4 * first, ptr(out), ptr(ws), ws.numel() * 4, stream()),
          "s2i_conv_wgrad")
    return out


def _rows_view(t):
    """(tensor usable by the kernels, row stride) for a NHWC gradient that may be a channel slice."""
    C = t.shape[-1]
    if t.is_contiguous():
        return t, C
    st = t.stride()
    if t.dim() >= 2 and st[-1] == 1 and st[-2] % 4 == 0 and t.data_ptr() % (4 * t.element_size()) == 0:
        ld = st[-2]
        ok = True
        expect = ld
        for dim in range(t.dim() - 2, -1, -1):
            if t.shape[dim] != 1 and st[dim] != expect:
                ok = False
                break
            expect *= t.shape[dim]
        if ok:
            return t, ld
    return t.contiguous(), C


def _num_parts(M):
    """Row chunks of the BatchNorm backward reduction: enough blocks to keep the HBM pipes full on the large maps
    (1024 / 2048 / 4096 chunks measured on the bf16 step: no difference)."""
    return int(max(1, min(1024, M // 64)))


# ---- conv + BatchNorm + activation ---------------------------------------------------------------------
_KIND = {"k1": CONV_K1, "k3s1": CONV_K3S1, "k4s2": CONV_K4S2, "up": TCONV_K4S2}


_DGRAD = {"k3s1": (CONV_K3S1, 1), "k4s2": (TCONV_K4S2, 0), "up": (CONV_K4S2, 0), "k1": (CONV_K1, 0)}


def _dgrad(kind_name, dy, w, packed, n_in, out_dtype=None):
    """Input gradient of the conv `kind_name` given dy (NHWC) -> [B,H,W,n_in]."""
    Op = packed.shape[2]
    if dy.shape[-1] != Op:
        raise _lib.S2IError("dgrad: dy has %d channels, packed weight %d" % (dy.shape[-1], Op))
    if out_dtype is not None:     # bf16 activation mode: either dtype on either side
        kind, flip = _DGRAD[kind_name]
        return conv_any(kind, dy, packed, n_in, wmode=1, flip=flip, out_dtype=out_dtype)[0]
    if kind_name == "k3s1":
        y, _, _ = conv_raw(CONV_K3S1, dy, None, packed, n_in, wmode=1, flip=1, wR=packed.shape[1], ldw=Op)
    elif kind_name == "k4s2":
        y, _, _ = conv_raw(TCONV_K4S2, dy, None, packed, n_in, wmode=1, wR=packed.shape[1], ldw=Op)
    elif kind_name == "up":
        y, _, _ = conv_raw(CONV_K4S2, dy, None, packed, n_in, wmode=1, wR=packed.shape[1], ldw=Op)
    else:
        y, _, _ = conv_raw(CONV_K1, dy, None, packed, n_in, wmode=1, wR=packed.shape[1], ldw=Op)
    return y


def _wgrad(kind_name, x, cvec, dy, weight, a_src=None):
    """Weight gradient; accumulated into weight.grad in place (returns None) in direct mode.  a_src: x is the RAW output of
    the producing block (deferred BatchNorm + LeakyReLU, applied by the gather)."""
    out, acc = (weight.grad, True) if _direct(weight) else (None, False)

    def run():
        if a_src is not None:
            return wgrad_raw(_KIND[kind_name], x, None, dy, tuple(weight.shape), out=out, accumulate=acc, a_src=a_src)
        if x.dtype == torch.bfloat16 or dy.dtype == torch.bfloat16:
            if cvec is not None:
                raise _lib.S2IError("wgrad: bf16 operands carry their broadcast vector materialised")
            if kind_name == "up":
                return wgrad_any(CONV_K4S2, dy, x, tuple(weight.shape), swap=1, fold=1, out=out, accumulate=acc)
            g = dy
            if (x.dtype == torch.bfloat16 and dy.dtype == torch.float32 and dy.shape[-1] <= 4
                    and x.shape[-1] % 8 == 0):
                # GET_IMAGE_G's weight gradient (bf16 features x fp32 NHWC4 image gradient): the <= 4 channel stream kernel
                # ran at a tenth of the HBM rate (0.32 ms at 256 px); padded to 8 bf16 channels the image gradient goes
                # through the bf16-MFMA weight-gradient kernel like every other layer's
                g = torch.zeros(dy.shape[:-1] + (8,), dtype=torch.bfloat16, device=dy.device)
                g[..., :dy.shape[-1]] = dy
            return wgrad_any(_KIND[kind_name], x, g, tuple(weight.shape), out=out, accumulate=acc)
        if kind_name == "up":
            return wgrad_raw(CONV_K4S2, dy, None, x, tuple(weight.shape), swap=1, fold=1, out=out, accumulate=acc)
        return wgrad_raw(_KIND[kind_name], x, cvec, dy, tuple(weight.shape), out=out, accumulate=acc)

    dw = run()
    return None if acc else dw


def _split_input_grad(dx_full, Cc):
    """dx of the stored channels and the gradient of the broadcast vector."""
    if Cc == 0:
        return dx_full, None
    lib = _lib_ready()
    B, H, W, Ca = dx_full.shape
    if H * W == 1:
        dc = dx_full.reshape(B, Ca)[:, :Cc].float()
    else:
        dc = torch.empty((B, Cc), dtype=torch.float32, device=dx_full.device)
        wsb = lib.s2i_spatial_sum_workspace_bytes(B, H * W, Cc)
        ws = _ws.get(wsb, dx_full.device)
        check(lib.s2i_spatial_sum_dt(_dt(dx_full), ptr(dx_full), Ca, B, H * W, Cc, ptr(dc), ptr(ws), ws.numel() * 4,
                                     stream()), "s2i_spatial_sum")
    return dx_full[..., Cc:], dc


def _factor_cvec(kind_name, cvec, x):
    """Spatially constant channels of a 3x3 conv are folded into a per-image, per-border-class bias (and
    their gradients taken from border sums of dY) instead of being convolved: on G's jointConv layers
    (model.py:268, 272-279) they are 128 of 192 / 160 input channels."""
    return cvec is not None and kind_name == "k3s1" and x.shape[1] >= 16 and x.shape[2] >= 16 and cvec.shape[1] % 4 == 0


def _tap_sums(dy):
    lib = _lib_ready()
    B, H, W, C = dy.shape
    out = torch.empty((B, 9, C), dtype=torch.float32, device=dy.device)
    wsb = lib.s2i_border_sums_workspace_bytes(B, H, W, C)
    ws = _ws.get(wsb, dy.device)
    check(lib.s2i_tap_sums_dt(_dt(dy), ptr(dy), B, H, W, C, ptr(out), ptr(ws), ws.numel() * 4, stream()), "s2i_tap_sums")
    return out


class ConvBnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cvec, weight, gamma, beta, residual, kind_name, act, bn_buffers, training, groups=1, defer=False):
        lib = _lib_ready()
        # input produced by a block that deferred its BatchNorm + LeakyReLU: gather its raw output instead (apply-on-load)
        in_src = _pending(x)
        if in_src is not None:
            if (cvec is None and residual is None and kind_name in ("k3s1", "k4s2") and not MATH_PLANES and training
                    and in_src.y.dtype == torch.float32 and x.shape[-1] % 32 == 0 and weight.shape[0] > 4
                    and in_src.groups == (groups if groups else 1)):
                x = in_src.y
            else:
                real(x)
                in_src = None
        x = x.contiguous()
        if cvec is not None:
            cvec = cvec.contiguous()
        kind = _KIND[kind_name]
        packed = packed_weight(weight, PACK_UPFOLD if kind_name == "up" else PACK_PLAIN)
        Cout = weight.shape[0]
        factored = _factor_cvec(kind_name, cvec, x)
        # bf16 activation mode: every spatial block stores its raw conv output and its result as bf16 (the fc of
        # INIT_STAGE_G, kind k1, stays an fp32 island)
        bf = (ACT_BF16 and kind_name != "k1") or x.dtype == torch.bfloat16
        if bf and in_src is not None:
            raise _lib.S2IError("ConvBnAct: apply-on-load input in the bf16 activation mode")
        adt = torch.bfloat16 if bf else torch.float32
        cat_cc = 0
        if bf and cvec is not None and not factored:
            # D's jointConv on 4x4 maps: the (c_code, h) concat of model.py:434 is materialised (a few MB) in bf16
            B_, H_, W_, _ = x.shape
            cat_cc = cvec.shape[1]
            x = torch.cat((cast(cvec, adt).view(B_, 1, 1, cat_cc).expand(B_, H_, W_, cat_cc), cast(x, adt)), 3).contiguous()
            cvec_used = None
        else:
            cvec_used = cvec
        if factored:
            B, Cc = cvec.shape
            Ip, Op = packed.shape[1], packed.shape[2]
            table = torch.empty((B, 9, Cout), dtype=torch.float32, device=x.device)
            ws = _ws.get(B * 9 * Cout * 4, x.device)
            check(lib.s2i_cvec_bias_table(ptr(cvec), ptr(packed), B, Cc, Ip, Op, Cout, ptr(table), ptr(ws),
                                          ws.numel() * 4, stream()), "s2i_cvec_bias_table")
            if bf:
                y, part, nparts = conv_any(kind, x, packed, Cout, stats=training, groups=groups, w_offset=Cc * Op,
                                           cls_bias=table, out_dtype=adt)
            else:
                y, part, nparts = conv_raw(kind, x, None, packed, Cout, wR=Ip, ldw=Op, stats=training, groups=groups,
                                           w_offset=Cc * Op, cls_bias=table)
        elif bf:
            y, part, nparts = conv_any(kind, x, packed, Cout, stats=training, groups=groups, out_dtype=adt)
        else:
            y, part, nparts = conv_raw(kind, x, cvec, packed, Cout, wR=packed.shape[1], ldw=packed.shape[2],
                                       stats=training, groups=groups, in_src=in_src)
        M = y.numel() // Cout
        if not training:
            groups = 1
        coef = torch.empty((groups, 4, Cout), dtype=torch.float32, device=x.device)
        rm, rv, nbt = bn_buffers
        if training:
            check(lib.s2i_bn_finalize(ptr(part), nparts, groups, Cout, M // groups, ptr(gamma), ptr(beta), ptr(rm),
                                      ptr(rv), ptr(nbt), BN_MOMENTUM, BN_EPS, ptr(coef), stream()), "s2i_bn_finalize")
        else:
            check(lib.s2i_bn_eval_coeffs(Cout, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), BN_EPS, ptr(coef), stream()),
                  "s2i_bn_eval_coeffs")
        Cact = Cout // 2 if act == ACT_GLU else Cout
        out = torch.empty(y.shape[:-1] + (Cact,), dtype=adt, device=x.device)
        if residual is not None:
            residual = cast(real(residual), adt).contiguous()
        if defer and DEFER_ACT and training and act == ACT_LRELU and residual is None and not bf and not MATH_PLANES:
            # the caller guarantees a single convolution consumer: `out` stays unwritten until real() or never
            out._s2i_lazy = _Lazy(y, coef, act, groups)
        else:
            check(lib.s2i_bn_act_forward_dt(_dt(y), ptr(y), M, groups, Cout, ptr(coef), act, ptr(residual), ptr(out),
                                            stream()), "s2i_bn_act_forward")
        ctx.save_for_backward(x, cvec_used, weight, gamma, y, coef, None if in_src is None else in_src.coef)
        ctx.in_src = None if in_src is None else (in_src.act, in_src.groups)
        ctx.beta_ref = beta
        ctx.kind_name, ctx.act, ctx.training, ctx.has_res = kind_name, act, training, residual is not None
        ctx.groups = groups
        ctx.factored = factored
        ctx.bf, ctx.cat_cc = bf, cat_cc
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        x, cvec, weight, gamma, y, coef, in_coef = ctx.saved_tensors
        if not ctx.training:
            raise _lib.S2IError("ConvBnAct.backward: eval-mode BatchNorm has no backward on this path")
        a_src = None
        if ctx.in_src is not None:
            # x is the producer's RAW output (apply-on-load forward): the weight gradient gathers it the same way where its
            # plan allows, otherwise the activated operand is computed now
            a_src = _Lazy(x, in_coef, ctx.in_src[0], ctx.in_src[1])
        Cout = weight.shape[0]
        M = y.numel() // Cout
        if dout.dtype != y.dtype:
            dout = cast(dout, y.dtype)
        dout_k, ldd = _rows_view(dout)
        G = ctx.groups
        nparts = _num_parts(M // G) * G
        part = torch.empty((2, nparts, Cout), dtype=torch.float32, device=y.device)
        check(lib.s2i_bn_act_bwd_reduce_dt(_dt(y), ptr(y), ptr(dout_k), ldd, M, G, Cout, ptr(coef), ctx.act, ptr(part),
                                           nparts, stream()), "s2i_bn_act_bwd_reduce")
        beta = ctx.beta_ref
        need_gb = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        direct_bn = need_gb and _direct(gamma) and _direct(beta)
        if not need_gb:       # frozen BatchNorm parameters (the discriminators during the G update)
            dgamma = dbeta = None
        else:
            dgamma = gamma.grad if direct_bn else torch.empty_like(gamma)
            dbeta = beta.grad if direct_bn else torch.empty_like(gamma)
        red2 = torch.empty((G, 2, Cout), dtype=torch.float32, device=y.device)
        check(lib.s2i_bn_bwd_finalize(ptr(part), nparts, G, Cout, M // G, ptr(dgamma), ptr(dbeta),
                                      1 if direct_bn else 0, ptr(red2), stream()), "s2i_bn_bwd_finalize")
        if direct_bn:
            dgamma = dbeta = None
        dy = torch.empty_like(y)
        check(lib.s2i_bn_act_bwd_apply_dt(_dt(y), ptr(y), ptr(dout_k), ldd, M, G, Cout, ptr(coef), ptr(red2), ctx.act,
                                          ptr(dy), stream()), "s2i_bn_act_bwd_apply")
        need_x, need_c, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = dc = dw = None
        Cc = 0 if cvec is None else cvec.shape[1]
        bf = ctx.bf
        if bf and not ctx.factored:
            # bf16 activation mode; a broadcast vector (ctx.cat_cc channels) was concatenated in front of x in the forward
            cc = ctx.cat_cc
            if need_x or (need_c and cc):
                packed = packed_weight(weight, PACK_UPFOLD if ctx.kind_name == "up" else PACK_PLAIN)
                dx_full = _dgrad(ctx.kind_name, dy, weight, packed, x.shape[-1], out_dtype=x.dtype)
                dx, dc = _split_input_grad(dx_full, cc)
                if not need_x:
                    dx = None
                if not need_c:
                    dc = None
            if need_w:
                dw = _wgrad(ctx.kind_name, x, None, dy, weight)
            dres = dout if ctx.has_res else None
            return dx, dc, dw, dgamma, dbeta, dres, None, None, None, None, None, None
        if ctx.factored:
            packed = packed_weight(weight, PACK_PLAIN)
            Ip, Op = packed.shape[1], packed.shape[2]
            B, Cx = x.shape[0], x.shape[-1]
            if need_x:
                if bf:
                    dx = conv_any(CONV_K3S1, dy, packed, Cx, wmode=1, flip=1, w_offset=Cc * Op, out_dtype=x.dtype)[0]
                else:
                    dx, _, _ = conv_raw(CONV_K3S1, dy, None, packed, Cx, wmode=1, flip=1, wR=Ip, ldw=Op, w_offset=Cc * Op)
            if need_c or need_w:
                tapsum = _tap_sums(dy)
                direct = need_w and _direct(weight)
                if need_w:
                    dw = weight.grad if direct else torch.empty(tuple(weight.shape), dtype=torch.float32, device=x.device)
                    if bf:
                        wgrad_any(CONV_K3S1, x, dy, (Cout, Cx, 3, 3), out=dw, accumulate=direct, i_off=Cc, I_total=Cc + Cx)
                    else:
                        wgrad_raw(CONV_K3S1, x, None, dy, (Cout, Cx, 3, 3), out=dw, accumulate=direct, i_off=Cc,
                                  I_total=Cc + Cx)
                if need_c:
                    dc = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
                check(lib.s2i_cvec_grads(ptr(cvec), ptr(packed), ptr(tapsum), B, Cc, Ip, Op, Cout, Cout, Cc + Cx, ptr(dc),
                                         ptr(dw) if need_w else None, 1 if direct else 0, stream()), "s2i_cvec_grads")
                if direct:
                    dw = None
        elif need_x or (need_c and cvec is not None):
            packed = packed_weight(weight, PACK_UPFOLD if ctx.kind_name == "up" else PACK_PLAIN)
            dx_full = _dgrad(ctx.kind_name, dy, weight, packed, x.shape[-1] + Cc)
            dx, dc = _split_input_grad(dx_full, Cc)
            if not need_x:
                dx = None
        if need_w and not ctx.factored:
            if a_src is not None:
                B_, H_, W_, Ca_ = x.shape
                O_, I_, KH_, KW_ = weight.shape
                dd = WgradDesc(_KIND[ctx.kind_name], B_, H_, W_, Ca_, 0, dy.shape[-1], dy.shape[-1], 0, 0, O_, I_, KH_, KW_, 0,
                               0, 0, a_src.act, a_src.groups)
                if lib.s2i_conv_wgrad_in_eligible(ctypes.byref(dd)):
                    dw = _wgrad(ctx.kind_name, x, None, dy, weight, a_src=a_src)
                else:
                    xa = torch.empty_like(x)
                    check(lib.s2i_bn_act_forward_dt(_dt(x), ptr(x), x.numel() // Ca_, a_src.groups, Ca_, ptr(in_coef),
                                                    a_src.act, None, ptr(xa), stream()), "s2i_bn_act_forward")
                    dw = _wgrad(ctx.kind_name, xa, None, dy, weight)
            else:
                dw = _wgrad(ctx.kind_name, x, cvec, dy, weight)
        dres = dout if ctx.has_res else None
        return dx, dc, dw, dgamma, dbeta, dres, None, None, None, None, None, None


class ConvAct(torch.autograd.Function):
    """conv (+bias) + LeakyReLU / tanh / none, no BatchNorm."""

    @staticmethod
    def forward(ctx, x, weight, bias, kind_name, act, n_out):
        x = real(x).contiguous()
        kind = _KIND[kind_name]
        packed = packed_weight(weight, PACK_PLAIN)
        if (ACT_BF16 and kind_name != "k1") or x.dtype == torch.bfloat16:
            # bf16 activation mode: feature maps (>= 8 channels) are bf16, NHWC4 images stay fp32
            odt = torch.bfloat16 if n_out >= 8 else torch.float32
            out = conv_any(kind, x, packed, n_out, bias=bias, act=act, out_dtype=odt)[0]
        else:
            out, _, _ = conv_raw(kind, x, None, packed, n_out, wR=packed.shape[1], ldw=packed.shape[2], bias=bias, act=act)
        ctx.save_for_backward(x, weight, out if act != ACT_NONE else None)
        ctx.kind_name, ctx.act, ctx.has_bias, ctx.n_out = kind_name, act, bias is not None, n_out
        ctx.bias_ref = bias
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        x, weight, out = ctx.saved_tensors
        N = ctx.n_out
        M = dout.numel() // N
        if out is not None and dout.dtype != out.dtype:
            dout = cast(dout, out.dtype)
        dout_k, ldd = _rows_view(dout)
        if ctx.act != ACT_NONE:
            dy = torch.empty(dout.shape, dtype=dout.dtype, device=dout.device)
            check(lib.s2i_act_backward_dt(_dt(out), ptr(out), ptr(dout_k), ldd, M, N, ctx.act, ptr(dy), stream()),
                  "s2i_act_backward")
        else:
            dy = dout_k if ldd == N else dout_k.contiguous()
        dx = dw = db = None
        mixed = x.dtype == torch.bfloat16 or dy.dtype == torch.bfloat16
        if ctx.needs_input_grad[0]:
            packed = packed_weight(weight, PACK_PLAIN)
            dx = _dgrad(ctx.kind_name, dy, weight, packed, x.shape[-1], out_dtype=x.dtype if mixed else None)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(ctx.kind_name, x, None, dy, weight)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            part = torch.empty((2, 1, N), dtype=torch.float32, device=dy.device)
            check(lib.s2i_colstats(ptr(cast(dy, torch.float32)), M, N, N, ptr(part), 1, stream()), "s2i_colstats")
            bias = ctx.bias_ref
            O = weight.shape[0]
            if _direct(bias):      # straight into the flat gradient buffer: no temporary, no AccumulateGrad add
                check(lib.s2i_axpby(ptr(bias.grad), ptr(part), O, 1.0, 1.0, stream()), "s2i_axpby")
            else:
                db = torch.empty((O,), dtype=torch.float32, device=dy.device)
                check(lib.s2i_axpby(ptr(db), ptr(part), O, 1.0, 0.0, stream()), "s2i_axpby")
        return dx, dw, db, None, None, None


# ---- CA_NET pieces -----------------------------------------------------------------------------------------
class Glu2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = _lib_ready()
        x = x.contiguous()
        M, C = x.shape
        out = torch.empty((M, C // 2), dtype=torch.float32, device=x.device)
        check(lib.s2i_glu_forward(ptr(x), M, C, ptr(out), stream()), "s2i_glu_forward")
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        (x,) = ctx.saved_tensors
        M, C = x.shape
        dx = torch.empty_like(x)
        check(lib.s2i_glu_backward(ptr(x), ptr(dout.contiguous()), M, C, ptr(dx), stream()), "s2i_glu_backward")
        return dx


class Reparam(torch.autograd.Function):
    """h = [mu | logvar] (B, 2E), eps (B, E) -> c = eps*exp(0.5*logvar) + mu  (model.py:188-195)."""

    @staticmethod
    def forward(ctx, h, eps):
        lib = _lib_ready()
        h = h.contiguous()
        eps = eps.contiguous()
        B, E2 = h.shape
        c = torch.empty((B, E2 // 2), dtype=torch.float32, device=h.device)
        check(lib.s2i_reparam_forward(ptr(h), ptr(eps), B, E2 // 2, ptr(c), stream()), "s2i_reparam_forward")
        ctx.save_for_backward(h, eps)
        return c

    @staticmethod
    def backward(ctx, dc):
        lib = _lib_ready()
        h, eps = ctx.saved_tensors
        B, E2 = h.shape
        dh = torch.empty_like(h)
        check(lib.s2i_reparam_backward(ptr(h), ptr(eps), ptr(dc.contiguous()), None, None, B, E2 // 2, ptr(dh),
                                       stream()), "s2i_reparam_backward")
        return dh, None


class KLLoss(torch.autograd.Function):
    """KL_loss of trainer.py:54-58 on (mu, logvar), each (B, E), possibly column slices of one tensor."""

    @staticmethod
    def forward(ctx, mu, logvar):
        lib = _lib_ready()
        if mu.stride(1) != 1:
            mu = mu.contiguous()
        if logvar.stride(1) != 1:
            logvar = logvar.contiguous()
        B, E = mu.shape
        kl = torch.empty((), dtype=torch.float32, device=mu.device)
        check(lib.s2i_kl_forward(ptr(mu), mu.stride(0), ptr(logvar), logvar.stride(0), B, E, ptr(kl), stream()),
              "s2i_kl_forward")
        ctx.save_for_backward(mu, logvar)
        return kl

    @staticmethod
    def backward(ctx, g):
        lib = _lib_ready()
        mu, logvar = ctx.saved_tensors
        B, E = mu.shape
        dmu = torch.empty((B, E), dtype=torch.float32, device=mu.device)
        dlv = torch.empty((B, E), dtype=torch.float32, device=mu.device)
        check(lib.s2i_kl_backward(ptr(mu), mu.stride(0), ptr(logvar), logvar.stride(0), B, E, ptr(g.contiguous()),
                                  ptr(dmu), ptr(dlv), stream()), "s2i_kl_backward")
        return dmu, dlv


# ---- D heads and losses ---------------------------------------------------------------------------------------
class LogitHead(torch.autograd.Function):
    """Conv2d(C,1,k=4,s=4)+Sigmoid on a (B,4,4,C) NHWC map (model.py:414-422)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib_ready()
        ctx.x_dtype = x.dtype
        x = cast(real(x).contiguous(), torch.float32)   # a (B,4,4,C) map: the heads and the losses are an fp32 island
        B, H, W, C = x.shape
        if H != 4 or W != 4 or tuple(weight.shape) != (1, C, 4, 4):
            raise _lib.S2IError("LogitHead: expects a 4x4 map and a (1,C,4,4) weight")
        prob = torch.empty((B,), dtype=torch.float32, device=x.device)
        check(lib.s2i_logit_forward(ptr(x), ptr(weight.contiguous()), ptr(bias), B, C, ptr(prob), stream()),
              "s2i_logit_forward")
        ctx.save_for_backward(x, weight, prob)
        ctx.has_bias = bias is not None
        ctx.bias_ref = bias
        return prob

    @staticmethod
    def backward(ctx, dprob):
        lib = _lib_ready()
        x, weight, prob = ctx.saved_tensors
        B, _, _, C = x.shape
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        bias = ctx.bias_ref
        want_w = ctx.needs_input_grad[1]
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        direct = want_w and _direct(weight) and (not want_b or _direct(bias))
        if direct:
            dw, db = weight.grad, (bias.grad if want_b else None)
        else:
            dw = torch.empty_like(weight) if want_w else None
            db = torch.empty((1,), dtype=torch.float32, device=x.device) if want_b else None
        check(lib.s2i_logit_backward(ptr(x), ptr(weight.contiguous()), ptr(prob), ptr(dprob.contiguous()), B, C,
                                     ptr(dx), 0, ptr(dw), ptr(db), 1 if direct else 0, stream()), "s2i_logit_backward")
        if direct:
            dw = db = None
        if dx is not None:
            dx = cast(dx, ctx.x_dtype)
        return dx, dw, db


class BCELoss(torch.autograd.Function):
    """weight * nn.BCELoss()(prob, full(target)) (trainer.py:394-409, 439-443)."""

    @staticmethod
    def forward(ctx, prob, target, weight):
        lib = _lib_ready()
        prob = prob.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=prob.device)
        check(lib.s2i_bce_forward(ptr(prob), float(target), prob.numel(), float(weight), ptr(loss), 0, stream()),
              "s2i_bce_forward")
        ctx.save_for_backward(prob)
        ctx.target, ctx.weight = float(target), float(weight)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib_ready()
        (prob,) = ctx.saved_tensors
        dprob = torch.empty_like(prob)
        check(lib.s2i_bce_backward(ptr(prob), ctx.target, prob.numel(), ctx.weight, ptr(g.contiguous()), ptr(dprob),
                                   stream()), "s2i_bce_backward")
        return dprob, None, None


class BCEMulti(torch.autograd.Function):
    """All BCE terms of one discriminator update in one launch: `heads` = H probability vectors of G stacked
    batches (G*B rows each); term (g, h) has target targets[g][h] and weight weights[g][h]
    (trainer.py:394-409 sums six of them)."""

    @staticmethod
    def forward(ctx, targets_dev, weights_dev, G, *heads):
        lib = _lib_ready()
        heads = [h.contiguous() for h in heads]
        H = len(heads)
        B = heads[0].numel() // G
        arr = (ctypes.c_void_p * H)(*[ptr(h) for h in heads])
        loss = torch.empty((), dtype=torch.float32, device=heads[0].device)
        check(lib.s2i_bce_multi_forward(arr, ptr(targets_dev), ptr(weights_dev), G, H, B, ptr(loss), stream()),
              "s2i_bce_multi_forward")
        ctx.save_for_backward(targets_dev, weights_dev, *heads)
        ctx.G = G
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib_ready()
        targets_dev, weights_dev = ctx.saved_tensors[:2]
        heads = ctx.saved_tensors[2:]
        H, G = len(heads), ctx.G
        B = heads[0].numel() // G
        grads = [torch.empty_like(h) for h in heads]
        pin = (ctypes.c_void_p * H)(*[ptr(h) for h in heads])
        pout = (ctypes.c_void_p * H)(*[ptr(t) for t in grads])
        check(lib.s2i_bce_multi_backward(pin, ptr(targets_dev), ptr(weights_dev), G, H, B, ptr(g.contiguous()), pout,
                                         stream()), "s2i_bce_multi_backward")
        return (None, None, None) + tuple(grads)


class ClassAwareLoss(torch.autograd.Function):
    """class_aware_loss of trainer.py:298-311 on features (B, D) and int32 device labels (B,)."""

    @staticmethod
    def forward(ctx, feats, labels):
        lib = _lib_ready()
        feats = feats.contiguous()
        B, D = feats.shape
        x4 = feats.view(B, 1, 1, D)
        # scores = X X^T through the implicit-GEMM kernel: the second operand is X itself, read transposed
        scores, _, _ = conv_raw(CONV_K1, x4, None, feats, B, wmode=1, wR=B, ldw=D)
        loss = torch.empty((1,), dtype=torch.float32, device=feats.device)
        dS = torch.empty((B, B), dtype=torch.float32, device=feats.device)
        check(lib.s2i_cal_loss(ptr(scores), ptr(labels), B, D, ptr(loss), 0, ptr(dS), stream()), "s2i_cal_loss")
        ctx.save_for_backward(feats, dS)
        return loss

    @staticmethod
    def backward(ctx, g):
        feats, dS = ctx.saved_tensors
        B, D = feats.shape
        Bp = _roundup4(B)
        if Bp != B:
            # the gathered operand needs a channel count that is a multiple of 4: zero columns of dS against zero
            # rows of X are exact (ragged last batch of an epoch, trainer.py:543-545: 8855 % 24 = 23 on CUB)
            dS_p = dS.new_zeros((B, Bp))
            dS_p[:, :B] = dS
            feats_p = feats.new_zeros((Bp, D))
            feats_p[:B] = feats
            dS, feats = dS_p, feats_p
        # dX = dS_sym X : K1 conv with gathered operand dS (B x Bp) and weights X used as P[k][n]
        dX, _, _ = conv_raw(CONV_K1, dS.view(B, 1, 1, Bp), None, feats, D, wmode=0, wR=Bp, ldw=D)
        dX = dX.view(B, D)
        lib = _lib_ready()
        # scale by the incoming gradient, read on the device (no host sync)
        check(lib.s2i_scale_dev(ptr(dX), ptr(dX), dX.numel(), ptr(g.contiguous()), stream()), "s2i_scale_dev")
        return dX, None


# ---- layout ---------------------------------------------------------------------------------------------------------
class ToNHWC(torch.autograd.Function):
    """(B,C,H,W) -> (B,H,W,Cp) with zero-filled padding channels."""

    @staticmethod
    def forward(ctx, x, Cp):
        lib = _lib_ready()
        x = x.contiguous()
        B, C, H, W = x.shape
        # bf16 activation mode: feature maps become bf16 here; NHWC4 images stay fp32
        odt = torch.bfloat16 if (ACT_BF16 and Cp >= 8) else torch.float32
        out = torch.empty((B, H, W, Cp), dtype=odt, device=x.device)
        check(lib.s2i_nchw_to_nhwc_dt(_dt(out), ptr(x), ptr(out), B, C, H, W, Cp, stream()), "s2i_nchw_to_nhwc")
        ctx.C = C
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        dk, ld = _rows_view(dout)
        B, H, W, _ = dout.shape
        dx = torch.empty((B, ctx.C, H, W), dtype=torch.float32, device=dout.device)
        check(lib.s2i_nhwc_to_nchw_dt(_dt(dk), ptr(dk), ld, ptr(dx), B, ctx.C, H, W, stream()), "s2i_nhwc_to_nchw")
        return dx, None


_DIFFAUG_BITS = {"color": _lib.DIFFAUG_COLOR, "translation": _lib.DIFFAUG_TRANSLATION, "cutout": _lib.DIFFAUG_CUTOUT}


def diffaug_policy(spec):
    """'color,translation,cutout' (any order, any subset; '' = none) -> the policy mask of s2i_diffaug_forward."""
    policy = 0
    for token in str(spec).split(","):
        token = token.strip()
        if not token:
            continue
        if token not in _DIFFAUG_BITS:
            raise ValueError("unknown augmentation %r: expected a comma-separated subset of %s"
                             % (token, ", ".join(sorted(_DIFFAUG_BITS))))
        policy |= _DIFFAUG_BITS[token]
    return policy


def _diffaug_workspace(lib, policy, B, H, W, device):
    """(pointer, bytes) of the per-image partial sums: only the colour stage reduces."""
    if not policy & _lib.DIFFAUG_COLOR:
        return None, 0
    ws = _ws.get(lib.s2i_diffaug_workspace_bytes(B, H, W), device)
    return ptr(ws), ws.numel() * 4


class DiffAugToNHWC(torch.autograd.Function):
    """ToNHWC of a (B,3,H,H) image batch to NHWC4 with differentiable augmentation applied on the way (s2i_diffaug_forward):
    colour, translation and cutout as `policy` (diffaug_policy) selects, drawn per image from row b of the fp32 device
    `table` (B, 8) of uniforms.  The backward is the exact adjoint, to x only, and launches nothing when x needs no
    gradient (the real and wrong batches)."""

    @staticmethod
    def forward(ctx, x, table, policy):
        lib = _lib_ready()
        x = x.contiguous()
        B, C, H, W = x.shape
        policy = int(policy)
        if C != 3:
            raise _lib.S2IError("DiffAugToNHWC takes 3-channel images, got %d channels" % C)
        if table.dtype != torch.float32 or tuple(table.shape) != (B, 8) or table.device != x.device:
            raise _lib.S2IError("DiffAugToNHWC: the table must be fp32 (%d, 8) on %s, got %s %s on %s"
                                % (B, x.device, table.dtype, tuple(table.shape), table.device))
        table = table.detach().contiguous()
        out = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
        ws, wsb = _diffaug_workspace(lib, policy, B, H, W, x.device)
        check(lib.s2i_diffaug_forward(ptr(x), ptr(table), policy, ptr(out), B, H, W, ws, wsb, stream()),
              "s2i_diffaug_forward")
        ctx.policy = policy
        ctx.save_for_backward(table)
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        lib = _lib_ready()
        table, = ctx.saved_tensors
        dk, ld = _rows_view(dout)
        B, H, W, _ = dout.shape
        dx = torch.empty((B, 3, H, W), dtype=torch.float32, device=dout.device)
        ws, wsb = _diffaug_workspace(lib, ctx.policy, B, H, W, dout.device)
        check(lib.s2i_diffaug_backward(_dt(dk), ptr(dk), ld, ptr(table), ctx.policy, ptr(dx), B, H, W, ws, wsb, stream()),
              "s2i_diffaug_backward")
        return dx, None, None


class ToNCHW(torch.autograd.Function):
    """(B,H,W,Cp) -> (B,C,H,W), dropping padding channels."""

    @staticmethod
    def forward(ctx, x, C):
        lib = _lib_ready()
        xk, ld = _rows_view(real(x))
        B, H, W, Cp = x.shape
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        check(lib.s2i_nhwc_to_nchw_dt(_dt(xk), ptr(xk), ld, ptr(out), B, C, H, W, stream()), "s2i_nhwc_to_nchw")
        ctx.Cp, ctx.x_dtype = Cp, x.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        dout = dout.contiguous()
        B, C, H, W = dout.shape
        dx = torch.empty((B, H, W, ctx.Cp), dtype=ctx.x_dtype, device=dout.device)
        check(lib.s2i_nchw_to_nhwc_dt(_dt(dx), ptr(dout), ptr(dx), B, C, H, W, ctx.Cp, stream()), "s2i_nchw_to_nhwc")
        return dx, None


# ---- speech-encoder head: LSTM with backward through time, and the encoder loss ---------------------------------------
# Tests set LSTM_SENTINEL to a float (NaN): every buffer the step kernels must fill completely, padded positions included
# (out, sent, the previous-state copy, dG), is then allocated filled with it, so an element a kernel skipped shows.
LSTM_SENTINEL = None
# False sends every shape through the per-direction matrix-kernel + cell-kernel path (tests; the fused one-launch step
# takes B <= 32, Hd % 8 == 0, Hd <= 512)
LSTM_FUSED = True


# A list here receives (h_n, c_n), each [D, B, Hd], of every LstmSentence forward: the final state is no output of the op
# (the reference uses only `output`), but the packed-sequence rule "a finished sequence carries its state" shows nowhere else.
LSTM_STATE_LOG = None


def _new(shape, device, dtype=torch.float32):
    if LSTM_SENTINEL is None:
        return torch.empty(shape, dtype=dtype, device=device)
    return torch.full(shape, LSTM_SENTINEL, dtype=dtype, device=device)


def _step_rows(t, B, L):
    """[B, 1, L, C] or [B, L, C] as the 1x1 matrix kernels take it.  They tile spatial extents that are powers of two, and a
    1x1 product sees nothing but rows, so any other L goes in as B * L images of one pixel: the same rows, the same plan
    (it depends on the row count alone).  A power of two keeps its [B, 1, L, C] form."""
    C = t.shape[-1]
    if L & (L - 1):
        return t.view(B * L, 1, 1, C)
    return t.view(B, 1, L, C)


def lstm_params(rnn):
    """The parameters of a one-layer nn.LSTM in the order LstmSentence takes them."""
    if rnn.num_layers != 1 or not rnn.batch_first or getattr(rnn, "proj_size", 0):
        raise _lib.S2IError("lstm_sentence supports a one-layer batch_first nn.LSTM (the reference's default)")
    sfx = ["", "_reverse"][:2 if rnn.bidirectional else 1]
    return [getattr(rnn, n + "_l0" + s_) for s_ in sfx for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


class LstmSentence(torch.autograd.Function):
    """(out [B, L, D*H], sent [B, D*H]) = packed-sequence LSTM over conv features x [B, 1, L, E] and its mean over all L
    steps (Audio_to_Image/speech_encoder.py:84-93), differentiable in x and in every parameter.  params: weight_ih,
    weight_hh, bias_ih, bias_hh of layer 0, then the same four of the reverse direction if bidirectional."""

    @staticmethod
    def forward(ctx, x, cap_lens, *params):
        lib = _lib_ready()
        if len(params) not in (4, 8):
            raise _lib.S2IError("lstm_sentence: 4 parameters per direction, got %d" % len(params))
        D = len(params) // 4
        if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise _lib.S2IError("lstm_sentence: x must be fp32 NHWC [B, 1, L, E], got %s" % (tuple(x.shape),))
        x = x.contiguous()
        B, _, L, E = x.shape
        Hd = params[1].shape[1]
        if tuple(params[0].shape) != (4 * Hd, E) or Hd % 4 or E % 4:
            raise _lib.S2IError("lstm_sentence: weight_ih %s does not fit E=%d, Hd=%d (both multiples of 4)"
                                % (tuple(params[0].shape), E, Hd))
        lens_host = [int(v) for v in (cap_lens.tolist() if torch.is_tensor(cap_lens) else cap_lens)]
        if len(lens_host) != B or max(lens_host) > L or min(lens_host) < 1:
            raise _lib.S2IError("lstm_sentence: cap_lens must hold B values in [1, %d]" % L)
        dev = x.device
        lens_dev = torch.tensor(lens_host, dtype=torch.int32, device=dev)
        G4 = D * 4 * Hd
        with torch.no_grad():
            w_ih = pack_weight(torch.cat([params[4 * d] for d in range(D)], 0), PACK_PLAIN)          # [1][E][D*4H]
            b = torch.cat([params[4 * d + 2] + params[4 * d + 3] for d in range(D)], 0).contiguous()
            # [1][Hd][4*Hd]: the operand of the recurrent matrix product and, read as a matrix, W_hh transposed
            w_hh = [pack_weight(params[4 * d + 1], PACK_PLAIN) for d in range(D)]
            raw = [params[4 * d + 1].detach().contiguous() for d in range(D)]
        xproj, _, _ = conv_raw(CONV_K1, _step_rows(x, B, L), None, w_ih, G4, wR=w_ih.shape[1], ldw=w_ih.shape[2],
                               bias=b)                                  # [B, 1, L, D*4H]
        out = _new((B, L, D * Hd), dev)
        gates = torch.empty((B, L, G4), dtype=torch.float32, device=dev)
        cst = torch.empty((B, L, D * Hd), dtype=torch.float32, device=dev)
        hprev = _new((D, B, L, Hd), dev)
        fused = LSTM_FUSED and B <= 32 and Hd % 8 == 0 and Hd <= 512
        steps = max(lens_host)
        if fused:
            hbuf = torch.zeros((2, D, B, Hd), dtype=torch.float32, device=dev)
            cs = torch.zeros((D, B, Hd), dtype=torch.float32, device=dev)
            for step in range(steps):
                check(lib.s2i_lstm_train_step(ptr(xproj), G4, ptr(raw[0]), ptr(raw[-1]), ptr(lens_dev), B, L, Hd, D, step,
                                              ptr(hbuf[step & 1]), ptr(hbuf[(step + 1) & 1]), ptr(cs), ptr(out), D * Hd,
                                              ptr(gates), ptr(cst), ptr(hprev), stream()), "s2i_lstm_train_step")
            if LSTM_STATE_LOG is not None:
                LSTM_STATE_LOG.append((hbuf[steps & 1].clone(), cs.clone()))
        else:
            hs_all = torch.zeros((D, B, 1, 1, Hd), dtype=torch.float32, device=dev)
            cs_all = torch.zeros((D, B, Hd), dtype=torch.float32, device=dev)
            for d in range(D):
                hs, cs = hs_all[d], cs_all[d]
                for step in range(steps):
                    hproj, _, _ = conv_raw(CONV_K1, hs, None, w_hh[d], 4 * Hd, wR=w_hh[d].shape[1], ldw=w_hh[d].shape[2])
                    check(lib.s2i_lstm_train_cell(ptr(xproj) + 4 * d * 4 * Hd, G4, ptr(hproj), ptr(lens_dev), B, L, Hd, step,
                                                  d, ptr(hs), ptr(cs), ptr(out) + 4 * d * Hd, D * Hd,
                                                  ptr(gates) + 4 * d * 4 * Hd, ptr(cst) + 4 * d * Hd, ptr(hprev[d]), stream()),
                          "s2i_lstm_train_cell")
            if LSTM_STATE_LOG is not None:
                LSTM_STATE_LOG.append((hs_all.view(D, B, Hd).clone(), cs_all.clone()))
        sent = _new((B, D * Hd), dev)
        check(lib.s2i_time_mean(ptr(out), B, L, D * Hd, ptr(sent), stream()), "s2i_time_mean")
        ctx.save_for_backward(x, gates, cst, hprev, lens_dev, w_ih, *w_hh)
        ctx.dims = (B, L, E, Hd, D, steps, fused)
        ctx.set_materialize_grads(False)
        return out, sent

    @staticmethod
    def backward(ctx, d_out, d_sent):
        lib = _lib_ready()
        x, gates, cst, hprev, lens_dev, w_ih = ctx.saved_tensors[:6]
        w_hh = ctx.saved_tensors[6:]
        B, L, E, Hd, D, steps, fused = ctx.dims
        dev = x.device
        G4 = D * 4 * Hd
        none = (None,) * (2 + 4 * D)
        if d_out is None and d_sent is None:
            return none
        d_out = None if d_out is None else d_out.float().contiguous()
        d_sent = None if d_sent is None else d_sent.float().contiguous()
        dG = _new((B, L, G4), dev)
        if fused:
            dc = torch.empty((D, B, Hd), dtype=torch.float32, device=dev)
            for step in range(steps - 1, -1, -1):
                check(lib.s2i_lstm_bwd_step(ptr(d_out), ptr(d_sent), ptr(gates), ptr(cst), ptr(w_hh[0]), ptr(w_hh[-1]),
                                            ptr(lens_dev), B, L, Hd, D, step, 1 if step == steps - 1 else 0, ptr(dc), ptr(dG),
                                            stream()), "s2i_lstm_bwd_step")
        else:
            off = lambda t, n: None if t is None else ptr(t) + 4 * n
            for d in range(D):
                dc = torch.empty((B, Hd), dtype=torch.float32, device=dev)
                dgt = torch.empty((B, 1, 1, 4 * Hd), dtype=torch.float32, device=dev)
                dhrec = None
                for step in range(steps - 1, -1, -1):
                    check(lib.s2i_lstm_bwd_cell(off(d_out, d * Hd), off(d_sent, d * Hd), D * Hd, off(gates, d * 4 * Hd), G4,
                                                off(cst, d * Hd), ptr(dhrec), ptr(lens_dev), B, L, Hd, step, d,
                                                1 if step == steps - 1 else 0, ptr(dc), off(dG, d * 4 * Hd), ptr(dgt),
                                                stream()), "s2i_lstm_bwd_cell")
                    if step:    # dh_rec = dG_t . W_hh: the packed W_hh read untransposed
                        dhrec, _, _ = conv_raw(CONV_K1, dgt, None, w_hh[d], Hd, wmode=1, wR=w_hh[d].shape[1],
                                               ldw=w_hh[d].shape[2])
        need = ctx.needs_input_grad
        grads = [None] * (2 + 4 * D)
        dG4 = _step_rows(dG, B, L)
        if need[0]:     # the seam: the gradient for the conv stack's output
            dx, _, _ = conv_raw(CONV_K1, dG4, None, w_ih, E, wmode=1, wR=w_ih.shape[1], ldw=w_ih.shape[2])
            grads[0] = dx.view(B, 1, L, E)
        if any(need[2 + 4 * d] for d in range(D)):
            dw_ih = wgrad_raw(CONV_K1, _step_rows(x, B, L), None, dG4, (G4, E))
            for d in range(D):
                if need[2 + 4 * d]:
                    grads[2 + 4 * d] = dw_ih[d * 4 * Hd:(d + 1) * 4 * Hd]
        for d in range(D):
            if need[3 + 4 * d]:
                grads[3 + 4 * d] = wgrad_raw(CONV_K1, _step_rows(hprev[d], B, L), None, dG4, (4 * Hd, Hd),
                                             g_cols=(d * 4 * Hd, 4 * Hd))
        if any(need[4 + 4 * d] or need[5 + 4 * d] for d in range(D)):
            db_all = torch.empty((G4,), dtype=torch.float32, device=dev)
            check(lib.s2i_lstm_bias_grad(ptr(dG), B * L, G4, ptr(db_all), stream()), "s2i_lstm_bias_grad")
            for d in range(D):
                db = db_all[d * 4 * Hd:(d + 1) * 4 * Hd]
                grads[4 + 4 * d] = db if need[4 + 4 * d] else None
                grads[5 + 4 * d] = db.clone() if need[5 + 4 * d] else None   # db_hh = db_ih, its own tensor
        return tuple(grads)


def lstm_sentence(x, cap_lens, *params):
    """LstmSentence on the parameters of a one-layer nn.LSTM (`lstm_params(rnn)`) or that module itself."""
    if len(params) == 1 and isinstance(params[0], torch.nn.LSTM):
        params = lstm_params(params[0])
    return LstmSentence.apply(x, cap_lens, *params)


class EncoderLoss(torch.autograd.Function):
    """The five scalars of the reference's LossFunc (train_audio_encoder.py:308-361) as one device tensor
    [total, jel, l1, distill, accu]; differentiable in `audio` through the total."""

    @staticmethod
    def forward(ctx, audio, image, label, c_diff, c_same, flags, lambda_l1, lambda_distill, distill_T):
        lib = _lib_ready()
        if audio.dim() != 2 or audio.shape != image.shape or label.shape[0] != audio.shape[0]:
            raise _lib.S2IError("encoder_loss: audio %s, image %s, label %s" % (tuple(audio.shape), tuple(image.shape),
                                                                                  tuple(label.shape)))
        a = audio.detach().float().contiguous()
        m = image.detach().float().contiguous()
        lab = label.to(device=a.device, dtype=torch.int32).contiguous()
        B, C = a.shape
        grad = torch.empty_like(a)
        scal = torch.empty((5,), dtype=torch.float32, device=a.device)
        wsb = lib.s2i_encoder_loss_workspace_bytes(B)
        ws = _ws.get(wsb, a.device)
        check(lib.s2i_encoder_loss(ptr(a), ptr(m), ptr(lab), B, C, float(c_diff), float(c_same), int(flags), float(lambda_l1),
                                   float(lambda_distill), float(distill_T), ptr(ws), ws.numel() * 4, ptr(grad), ptr(scal),
                                   stream()), "s2i_encoder_loss")
        ctx.save_for_backward(grad)
        return scal

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g[0] if ctx.needs_input_grad[0] else None,) + (None,) * 8


def encoder_loss(audio, image, label, loss_diff=1, loss_same=1, jel=True, l1=False, lambda_l1=1, distill=False, distill_T=2,
                 lambda_distill=1):
    """LossFunc(loss_diff, loss_same, jel, l1, lambda_l1, distill, distill_T, lambda_distill)(audio, image, label) of the
    reference: {'loss', 'loss_jel', 'loss_l1', 'loss_distill', 'accu'}, all 0-d device tensors (nothing is copied to the
    host); 'loss' carries the gradient for `audio`, the image side gets none."""
    flags = (_lib.ENC_LOSS_JEL if jel else 0) | (_lib.ENC_LOSS_L1 if l1 else 0) | (_lib.ENC_LOSS_DISTILL if distill else 0)
    scal = EncoderLoss.apply(audio, image, label, loss_diff, loss_same, flags, lambda_l1 if l1 else 0.0,
                             lambda_distill if distill else 0.0, distill_T)
    parts = scal.detach()
    return {"loss": scal[0], "loss_jel": parts[1], "loss_l1": parts[2], "loss_distill": parts[3], "accu": parts[4]}


# ---- speech-encoder conv stack under autograd: train-mode BatchNorm, temporal-conv gradients, pool backward ---------------
# The reference trains all of CNNRNN (Audio_to_Image/train_audio_encoder.py:168-216); these operators are the conv stack of
# speech_encoder.py:26-52 with a graph behind it.  fp32, one GPU, frame counts that are powers of two.  Tests set
# CONV_STACK_SENTINEL to a float (NaN): every buffer a kernel must fill completely is then allocated filled with it.
CONV_STACK_SENTINEL = None
# A list here receives the stored forward tensors of every operator call, in call order: ("bn0", x, out), ("block", y raw,
# out activated) and ("pool", x, out).  conv_stack_train clears it first, so it holds the last call: the ReLU decisions are
# out > 0, the pool maxima follow from x.
CONV_STACK_LOG = None


def _cnew(shape, device):
    if CONV_STACK_SENTINEL is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    return torch.full(shape, CONV_STACK_SENTINEL, dtype=torch.float32, device=device)


def _nhwc1(x, what):
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
        raise _lib.S2IError("%s: x must be fp32 NHWC [B, 1, W, C], got %s %s" % (what, tuple(x.shape), x.dtype))
    return x.contiguous()


class TemporalConvBnRelu(torch.autograd.Function):
    """Conv2d(bias=False) + BatchNorm2d (training statistics) + ReLU of conv_layer_2d on NHWC [B, 1, W, Cin].  geom = (k,
    stride, pad) of a (1 x k) temporal convolution, or None for the first (n_mels x 1) layer, a 1x1 conv over the mel axis.
    Stored: x, the raw conv output and the activated output (the next layer's input)."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, bn_buffers, geom):
        lib = _lib_ready()
        if MATH_PLANES:
            raise _lib.S2IError("temporal_conv_bn_relu: native fp32 matrix mode only")
        x = _nhwc1(x, "temporal_conv_bn_relu")
        B, _, W, Cin = x.shape
        Cout = weight.shape[0]
        if geom is None:
            if tuple(weight.shape[1:]) != (1, Cin, 1):
                raise _lib.S2IError("temporal_conv_bn_relu: first-layer weight %s does not fit %d mel bands"
                                    % (tuple(weight.shape), Cin))
            packed = pack_weight(weight.detach().reshape(Cout, Cin), PACK_PLAIN)
            y, part, nparts = conv_raw(CONV_K1, x, None, packed, Cout, wR=packed.shape[1], ldw=packed.shape[2], stats=True)
        else:
            k, st, pd = (int(v) for v in geom)
            if tuple(weight.shape[1:]) != (Cin, 1, k):
                raise _lib.S2IError("temporal_conv_bn_relu: weight %s does not fit Cin=%d, k=%d" % (tuple(weight.shape), Cin, k))
            geom = (k, st, pd)
            packed = pack_weight(weight, PACK_PLAIN)
            y, part, nparts = conv_raw(_lib.CONV_1D, x, None, packed, Cout, wR=packed.shape[1], ldw=packed.shape[2],
                                       stats=True, conv1d=geom)
        M = y.numel() // Cout
        coef = _cnew((1, 4, Cout), x.device)
        rm, rv, nbt = bn_buffers
        check(lib.s2i_bn_finalize(ptr(part), nparts, 1, Cout, M, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), BN_MOMENTUM,
                                  BN_EPS, ptr(coef), stream()), "s2i_bn_finalize")
        out = _cnew(tuple(y.shape), x.device)
        check(lib.s2i_bn_relu_forward(ptr(y), M, Cout, ptr(coef), ptr(out), stream()), "s2i_bn_relu_forward")
        if CONV_STACK_LOG is not None:
            CONV_STACK_LOG.append(("block", y, out))
        ctx.save_for_backward(x, packed, y, out, coef)
        ctx.geom, ctx.wshape = geom, tuple(weight.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        x, packed, y, out, coef = ctx.saved_tensors
        geom = ctx.geom
        B, _, W, Cin = x.shape
        Cout = y.shape[-1]
        M = y.numel() // Cout
        dev = x.device
        dout = dout.float().contiguous()
        nparts = _num_parts(M)
        part = _cnew((2, nparts, Cout), dev)
        check(lib.s2i_bn_relu_bwd_reduce(ptr(y), ptr(out), ptr(dout), M, Cout, ptr(coef), ptr(part), nparts, stream()),
              "s2i_bn_relu_bwd_reduce")
        dgamma, dbeta, red2 = _cnew((Cout,), dev), _cnew((Cout,), dev), _cnew((2, Cout), dev)
        check(lib.s2i_bn_bwd_finalize(ptr(part), nparts, 1, Cout, M, ptr(dgamma), ptr(dbeta), 0, ptr(red2), stream()),
              "s2i_bn_bwd_finalize")
        dy = _cnew(tuple(y.shape), dev)
        check(lib.s2i_bn_relu_bwd_apply(ptr(y), ptr(out), ptr(dout), M, Cout, ptr(coef), ptr(red2), ptr(dy), stream()),
              "s2i_bn_relu_bwd_apply")
        need = ctx.needs_input_grad
        dx = dw = None
        if geom is None:
            if need[0]:
                dx, _, _ = conv_raw(CONV_K1, dy, None, packed, Cin, wmode=1, wR=packed.shape[1], ldw=packed.shape[2])
            if need[1]:
                dw = wgrad_raw(CONV_K1, x, None, dy, (Cout, Cin)).view(ctx.wshape)
        else:
            k, st, pd = geom
            if need[0]:
                dx = _cnew(tuple(x.shape), dev)
                check(lib.s2i_conv1d_dgrad(ptr(dy), ptr(packed), ptr(dx), B, W, Cin, Cout, packed.shape[1], packed.shape[2], k,
                                           st, pd, stream()), "s2i_conv1d_dgrad")
            if need[1]:
                dw = _cnew(ctx.wshape, dev)
                wsb = lib.s2i_conv1d_wgrad_workspace_bytes(B, W, Cin, Cout, k, st, pd)
                if wsb == 0:
                    check(1, "s2i_conv1d_wgrad_workspace_bytes")
                ws = _ws.get(wsb, dev)
                check(lib.s2i_conv1d_wgrad(ptr(x), ptr(dy), ptr(dw), B, W, Cin, Cout, k, st, pd, ptr(ws), ws.numel() * 4,
                                           stream()), "s2i_conv1d_wgrad")
        return dx, dw, dgamma if need[2] else None, dbeta if need[3] else None, None, None


def temporal_conv_bn_relu(x, weight, gamma, beta, bn_buffers, geom):
    """x [B, 1, W, Cin] -> relu(batchnorm_train(conv(x))) [B, 1, Wo, Cout]; bn_buffers = (running_mean, running_var,
    num_batches_tracked), updated as nn.BatchNorm2d in training mode does (momentum 0.1, unbiased variance)."""
    return TemporalConvBnRelu.apply(x, weight, gamma, beta, tuple(bn_buffers), geom)


class InputBatchNorm(torch.autograd.Function):
    """The leading nn.BatchNorm2d(1) in training mode: ONE channel over all elements of x [B, 1, T, n_mels].  The
    per-channel apply kernels run on the [n / 4][4] view of the tensor; s2i_bn1_finalize / s2i_bn1_bwd_finalize fold the
    four columns into the channel.  The statistics are s2i_bn1_stats' (double sums: x is un-normalised log-mel)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn_buffers):
        lib = _lib_ready()
        x = _nhwc1(x, "input_batchnorm")
        n = x.numel()
        if n % 4 or gamma.numel() != 1 or beta.numel() != 1:
            raise _lib.S2IError("input_batchnorm: one channel over a multiple of 4 elements (n=%d)" % n)
        dev = x.device
        R = n // 4
        nparts = _num_parts(R)
        part = _cnew((2, nparts, 4), dev)
        check(lib.s2i_bn1_stats(ptr(x), n, ptr(part), nparts, stream()), "s2i_bn1_stats")
        coef = _cnew((1, 4, 4), dev)
        rm, rv, nbt = bn_buffers
        check(lib.s2i_bn1_finalize(ptr(part), nparts, n, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), BN_MOMENTUM, BN_EPS,
                                   ptr(coef), stream()), "s2i_bn1_finalize")
        out = _cnew(tuple(x.shape), dev)
        check(lib.s2i_bn_act_forward(ptr(x), R, 1, 4, ptr(coef), ACT_NONE, None, ptr(out), stream()), "s2i_bn_act_forward")
        if CONV_STACK_LOG is not None:
            CONV_STACK_LOG.append(("bn0", x, out))
        ctx.save_for_backward(x, coef)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        x, coef = ctx.saved_tensors
        dev = x.device
        n = x.numel()
        R = n // 4
        dout = dout.float().contiguous()
        nparts = _num_parts(R)
        part = _cnew((2, nparts, 4), dev)
        check(lib.s2i_bn1_bwd_reduce(ptr(x), ptr(dout), n, ptr(coef), ptr(part), nparts, stream()), "s2i_bn1_bwd_reduce")
        dgamma, dbeta, red2 = _cnew((1,), dev), _cnew((1,), dev), _cnew((2, 4), dev)
        check(lib.s2i_bn1_bwd_finalize(ptr(part), nparts, n, ptr(dgamma), ptr(dbeta), ptr(red2), stream()),
              "s2i_bn1_bwd_finalize")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _cnew(tuple(x.shape), dev)
            check(lib.s2i_bn_act_bwd_apply(ptr(x), ptr(dout), 4, R, 1, 4, ptr(coef), ptr(red2), ACT_NONE, ptr(dx), stream()),
                  "s2i_bn_act_bwd_apply")
        return dx, dgamma if ctx.needs_input_grad[1] else None, dbeta if ctx.needs_input_grad[2] else None, None


def input_batchnorm(x, gamma, beta, bn_buffers):
    return InputBatchNorm.apply(x, gamma, beta, tuple(bn_buffers))


class MaxPoolW3S2(torch.autograd.Function):
    """nn.MaxPool2d((1, 3), (1, 2), (0, 1)) on NHWC [B, H, W, C]; the backward recomputes each window's maximum from the
    stored input (lowest position wins a tie, as torch)."""

    @staticmethod
    def forward(ctx, x):
        lib = _lib_ready()
        if x.dim() != 4 or x.dtype != torch.float32:
            raise _lib.S2IError("maxpool_w3s2: x must be fp32 NHWC, got %s" % (tuple(x.shape),))
        x = x.contiguous()
        B, H, W, C = x.shape
        out = _cnew((B, H, W // 2, C), x.device)
        check(lib.s2i_maxpool_w3s2(ptr(x), B, H, W, C, ptr(out), stream()), "s2i_maxpool_w3s2")
        if CONV_STACK_LOG is not None:
            CONV_STACK_LOG.append(("pool", x, out))
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib_ready()
        (x,) = ctx.saved_tensors
        B, H, W, C = x.shape
        dout = dout.float().contiguous()
        dx = _cnew(tuple(x.shape), x.device)
        check(lib.s2i_maxpool_w3s2_backward(ptr(x), ptr(dout), B, H, W, C, ptr(dx), stream()), "s2i_maxpool_w3s2_backward")
        return dx


def maxpool_w3s2(x):
    return MaxPoolW3S2.apply(x)


def _bn_buffers(bn):
    return bn.running_mean, bn.running_var, bn.num_batches_tracked


def conv_stack_train(conv_sequential, mel_nhwc):
    """CNNRNN.Conv (BatchNorm2d(1), conv_layer_2d blocks, MaxPool2d) in training mode on NHWC log-mel [B, 1, T, n_mels] ->
    [B, 1, T / 64, 1024], differentiable in every Conv.* parameter; running statistics and num_batches_tracked are updated in
    place through raw pointers (their torch version counters do not move)."""
    if CONV_STACK_LOG is not None:
        del CONV_STACK_LOG[:]
    mods = list(conv_sequential)
    if not isinstance(mods[0], torch.nn.BatchNorm2d) or mods[0].num_features != 1:
        raise _lib.S2IError("conv_stack_train: expected CNNRNN.Conv (leading BatchNorm2d(1))")
    h = input_batchnorm(mel_nhwc, mods[0].weight, mods[0].bias, _bn_buffers(mods[0]))
    first = True
    for m in mods[1:]:
        if isinstance(m, torch.nn.MaxPool2d):
            if (m.kernel_size, m.stride, m.padding) != ((1, 3), (1, 2), (0, 1)):
                raise _lib.S2IError("conv_stack_train: unsupported pool %s" % (m,))
            h = maxpool_w3s2(h)
        elif isinstance(m, torch.nn.Sequential):
            conv, bn = m[0], m[1]
            if conv.bias is not None or bn.momentum != BN_MOMENTUM or bn.eps != BN_EPS:
                raise _lib.S2IError("conv_stack_train: unsupported block %s" % (m,))
            geom = None if first else (conv.kernel_size[1], conv.stride[1], conv.padding[1])
            if not first and conv.kernel_size[0] != 1:
                raise _lib.S2IError("conv_stack_train: temporal convolutions are (1 x k), got %s" % (conv.kernel_size,))
            h = temporal_conv_bn_relu(h, conv.weight, bn.weight, bn.bias, _bn_buffers(bn), geom)
            first = False
        else:
            raise _lib.S2IError("conv_stack_train: unsupported module %s" % (m,))
    return h


# ---- optimiser -----------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step=0, step_dev=None, gscale=1.0):
    lib = _lib_ready()
    check(lib.s2i_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, int(step),
                            ptr(step_dev), gscale, stream()), "s2i_adam_step")


def adam_l2_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step=0, step_dev=None, gscale=1.0):
    """torch.optim.Adam(weight_decay=...) on flat fp32 buffers: adam_step with gscale * g + weight_decay * p as the gradient."""
    lib = _lib_ready()
    check(lib.s2i_adam_l2_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, int(step),
                               ptr(step_dev), gscale, stream()), "s2i_adam_l2_step")


def ema_update(avg, p, decay):
    lib = _lib_ready()
    check(lib.s2i_ema_update(ptr(avg), ptr(p), p.numel(), decay, stream()), "s2i_ema_update")


def increment(counter):
    lib = _lib_ready()
    check(lib.s2i_increment(ptr(counter), stream()), "s2i_increment")


# ---- gradient norm, clip coefficient and the non-finite guard (include/s2i_hip.h) ---------------------------------------------
GRAD_CHUNK = _lib.GRAD_CHUNK
GRAD_STATS_HEAD = _lib.GRAD_STATS_HEAD
GRAD_STATS_FIELDS = ("norm", "coef", "scale", "apply", "updates", "clipped", "skipped", "norm_sum", "norm_max", "sumsq")


def grad_chunk_table(offsets, sizes):
    """The chunks s2i_grad_sumsq cuts a flat layout into -> [(first element, length, tensor)], in block order: tensor s from
    offsets[s] on in pieces of GRAD_CHUNK, the last one shorter.  Refuses what does not describe a FlatNet layout: an empty
    tensor, an offset that is not a multiple of 4, tensors that overlap or are out of order."""
    offsets, sizes = [int(o) for o in offsets], [int(n) for n in sizes]
    if not sizes or len(offsets) != len(sizes):
        raise ValueError("grad_chunk_table: %d offsets for %d sizes" % (len(offsets), len(sizes)))
    table, end = [], 0
    for s, (o, n) in enumerate(zip(offsets, sizes)):
        if n < 1 or o % 4 or o < end:
            raise ValueError("grad_chunk_table: tensor %d (offset %d, %d elements) behind element %d: sizes must be >= 1, "
                             "offsets multiples of 4 and ascending without overlap" % (s, o, n, end))
        table += [(o + c, min(GRAD_CHUNK, n - c), s) for c in range(0, n, GRAD_CHUNK)]
        end = o + n
    return table


class GradLayout:
    """A flat layout's device-side description and the workspace of the three-launch clipped step, allocated once:
    `offsets`, `sizes` [S] and `chunk0` [S + 1] (int64), `partials` [chunks] and `stats` [GRAD_STATS_HEAD + 2 S] (fp64),
    `scale` [1] (fp32) and `apply` [1] (int32).  `total` is the length of the buffers the layout describes."""

    def __init__(self, offsets, sizes, total, device):
        table = grad_chunk_table(offsets, sizes)
        self.S, self.total, self.nchunks = len(sizes), int(total), len(table)
        if table[-1][0] + table[-1][1] > self.total:
            raise ValueError("GradLayout: the layout ends at element %d of a buffer of %d" % (table[-1][0] + table[-1][1],
                                                                                            self.total))
        chunk0 = [0]
        for n in sizes:
            chunk0.append(chunk0[-1] + -(-int(n) // GRAD_CHUNK))
        i64 = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int64, device=device)
        self.offsets, self.sizes, self.chunk0 = i64(offsets), i64(sizes), i64(chunk0)
        self.partials = torch.zeros(self.nchunks, dtype=torch.float64, device=device)
        self.stats = torch.zeros(GRAD_STATS_HEAD + 2 * self.S, dtype=torch.float64, device=device)
        self.scale = torch.zeros(1, dtype=torch.float32, device=device)
        self.apply = torch.zeros(1, dtype=torch.int32, device=device)

    def read_stats(self):
        """The stats record on the host (one synchronisation) -> dict of GRAD_STATS_FIELDS, `tensor_norms` and
        `tensor_sumsq` (lists of S)."""
        st = self.stats.cpu().tolist()
        out = dict(zip(GRAD_STATS_FIELDS, st))
        for k in ("apply", "updates", "clipped", "skipped"):
            out[k] = int(out[k])
        out["tensor_norms"] = st[GRAD_STATS_HEAD:GRAD_STATS_HEAD + self.S]
        out["tensor_sumsq"] = st[GRAD_STATS_HEAD + self.S:GRAD_STATS_HEAD + 2 * self.S]
        return out

    def reset_stats(self):
        """Zero the running aggregates (updates, clipped, skipped, norm_sum, norm_max)."""
        self.stats[4:9].zero_()


def _flat_f32(t, n, what):
    if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise _lib.S2IError("%s: expected a contiguous fp32 buffer of %d elements, got %s %s" % (what, n, tuple(t.shape), t.dtype))


def grad_sumsq(g, layout):
    """layout.partials[c] = fp64 sum of squares of chunk c of the flat gradient buffer g (s2i_grad_sumsq)."""
    lib = _lib_ready()
    _flat_f32(g, layout.total, "grad_sumsq")
    check(lib.s2i_grad_sumsq(ptr(g), g.numel(), ptr(layout.offsets), ptr(layout.sizes), ptr(layout.chunk0), layout.S,
                             layout.nchunks, ptr(layout.partials), stream()), "s2i_grad_sumsq")


def grad_clip_scale(layout, gscale, max_norm=0.0, step_dev=None):
    """Finish grad_sumsq on the device (s2i_grad_clip_scale): layout.scale[0] = float(gscale * coef) with clip_grad_norm_'s
    coef for max_norm > 0 (0: coef = 1), layout.apply[0] = the sum is finite, step_dev[0] += 1 if it is; layout.stats."""
    lib = _lib_ready()
    gscale, max_norm = float(gscale), float(max_norm)
    if not (max_norm >= 0.0) or gscale != gscale:
        raise _lib.S2IError("grad_clip_scale: max_norm must be >= 0 (0: no clipping), got %r" % max_norm)
    if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.numel() != 1):
        raise _lib.S2IError("grad_clip_scale: step_dev is one int32")
    check(lib.s2i_grad_clip_scale(ptr(layout.partials), ptr(layout.chunk0), layout.S, gscale, max_norm, ptr(step_dev),
                                  ptr(layout.scale), ptr(layout.apply), ptr(layout.stats), stream()), "s2i_grad_clip_scale")


def _dev_scalars(step_dev, scale_dev, apply_dev, what):
    for t, dt in ((step_dev, torch.int32), (scale_dev, torch.float32), (apply_dev, torch.int32)):
        if t is None or t.dtype != dt or t.numel() != 1:
            raise _lib.S2IError("%s: step_dev (int32), scale_dev (fp32) and apply_dev (int32) are one-element device tensors"
                                % what)


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, step_dev, scale_dev, apply_dev):
    """adam_step with the step count, gscale (scale_dev[0]) and the apply flag on the device; apply_dev[0] == 0 stores nothing."""
    lib = _lib_ready()
    _dev_scalars(step_dev, scale_dev, apply_dev, "adam_step_dev")
    check(lib.s2i_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, ptr(step_dev),
                                ptr(scale_dev), ptr(apply_dev), stream()), "s2i_adam_step_dev")


def adam_l2_step_dev(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_dev, scale_dev, apply_dev):
    """adam_l2_step with the step count, gscale (scale_dev[0]) and the apply flag on the device."""
    lib = _lib_ready()
    _dev_scalars(step_dev, scale_dev, apply_dev, "adam_l2_step_dev")
    check(lib.s2i_adam_l2_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                   ptr(step_dev), ptr(scale_dev), ptr(apply_dev), stream()), "s2i_adam_l2_step_dev")




# ---- evaluation output ---------------------------------------------------------------------------------------------
def images_to_uint8_hwc(img_nhwc):
    """(B,H,W,C>=3) float NHWC in [-1,1] -> (B,H,W,3) uint8: the reference's save_singleimages conversion
    (trainer.py:676-677) in one kernel, already in the HWC order a PNG encoder wants."""
    lib = _lib_ready()
    t, ld = _rows_view(img_nhwc)
    B, H, W, _ = img_nhwc.shape
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=img_nhwc.device)
    check(lib.s2i_image_to_u8(ptr(t), ld, ptr(out), B * H * W, stream()), "s2i_image_to_u8")
    return out


def image_grid_uint8(images, nrow=8, padding=2, layout="nchw"):
    """N three-channel images -> ONE (Hg, Wg, 3) uint8 device tensor: the picture the reference's
    `vutils.save_image(images, path, nrow=8, padding=2, normalize=True)` writes (trainer.py:268-295), i.e. min-max
    normalised over the whole batch, tiled `nrow` to a line with `padding` black pixels around every cell, quantised as
    `mul(255).add(0.5).clamp(0, 255)` truncated (s2i_image_grid_u8).  layout "nchw": (N, 3, H, W);
    "nhwc": (N, H, W, C >= 3), the generator's NHWC4 output, whose further channels are never read.  Any strides (a batch
    slice, a channel slice) are taken as they are; a tensor that is not fp32 (bf16 activation mode) is converted first."""
    lib = _lib_ready()
    if layout not in ("nchw", "nhwc"):
        raise ValueError("layout must be 'nchw' or 'nhwc'")
    if images.dim() != 4 or images.shape[3 if layout == "nhwc" else 1] < 3:
        raise ValueError("image_grid_uint8 takes a 4-d batch with at least three channels, got %s as %s"
                         % (tuple(images.shape), layout))
    if images.dtype != torch.float32:
        images = images.float()
    images = images.detach()
    sn, s1, s2, s3 = images.stride()
    if layout == "nhwc":
        N, H, W = images.shape[:3]
        sy, sx, sc = s1, s2, s3
    else:
        N, H, W = images.shape[0], images.shape[2], images.shape[3]
        sc, sy, sx = s1, s2, s3
    nrow, padding = int(nrow), int(padding)
    xmaps = max(1, min(nrow, N))
    ymaps = -(-N // xmaps) if N > 0 else 0
    out = torch.empty((max(ymaps * (H + padding) + padding, 0), max(xmaps * (W + padding) + padding, 0), 3),
                      dtype=torch.uint8, device=images.device)
    ws = _ws.get(lib.s2i_image_grid_workspace_bytes(), images.device)
    check(lib.s2i_image_grid_u8(ptr(images), N, H, W, sn, sy, sx, sc, nrow, padding, ptr(ws), ptr(out), stream()),
          "s2i_image_grid_u8")
    return out


# ---- data edge -----------------------------------------------------------------------------------------------------
def images_from_uint8_hwc(u8):
    """(B,H,W,3) uint8 RGB on the device -> (B,3,H,W) float in [-1,1]: the reference's per-sample
    ToTensor + Normalize(0.5, 0.5) (datasets.py:440-442) applied to the collated batch on the GPU, so the
    host->device copy carries 1 byte per sample instead of 4."""
    lib = _lib_ready()
    assert u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[-1] == 3 and u8.is_contiguous()
    B, H, W, _ = u8.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=u8.device)
    check(lib.s2i_u8_to_image(ptr(u8), ptr(out), B, H, W, stream()), "s2i_u8_to_image")
    return out


def image_batch(pool, offsets, sizes, plan, size, levels, tab1=None, tab2=None):
    """Crop, mirror, pyramid and normalise a planned batch out of a resident uint8 image pool (device_loader.py) in one
    launch: `plan` is the (n, 4) int32 device table (pool index, top, left, flip); returns `levels` float NCHW tensors
    (n, 3, size >> i, size >> i), largest first -- what `images_from_uint8_hwc` gives for the host path's uint8 batches
    (datasets.py:40-66 behind main.py:127-131), bit for bit.  `tab1` / `tab2` are `device_loader.coeff_table` of
    size -> size / 2 and size -> size / 4 on the device."""
    lib = _lib_ready()
    assert pool.dtype == torch.uint8 and pool.dim() == 1 and pool.is_contiguous()
    assert offsets.dtype == torch.int64 and sizes.dtype == torch.int32 and sizes.shape == (offsets.numel(), 2)
    assert plan.dtype == torch.int32 and plan.dim() == 2 and plan.shape[1] == 4 and plan.is_contiguous()
    assert offsets.is_contiguous() and sizes.is_contiguous()
    n = plan.shape[0]
    tabs = [None, tab1, tab2]
    for i in range(1, levels):
        want = (size >> i, 1 + (4 << (i - 1)))
        assert tabs[i] is not None and tabs[i].dtype == torch.int32 and tuple(tabs[i].shape) == want, (i, want)
        assert tabs[i].is_contiguous()
    outs = [torch.empty((n, 3, size >> i, size >> i), dtype=torch.float32, device=pool.device) for i in range(levels)]
    o = outs + [None] * (3 - len(outs))
    check(lib.s2i_image_batch(ptr(pool), pool.numel(), ptr(offsets), ptr(sizes), offsets.numel(), ptr(plan), n, size,
                              levels, ptr(tab1), ptr(tab2), ptr(o[0]), ptr(o[1]), ptr(o[2]), stream()),
          "s2i_image_batch")
    return outs


# Tests set LOGMEL_GATHER_SENTINEL to a float (NaN): the output is then allocated filled with it, so a piece the kernel
# skipped shows.
LOGMEL_GATHER_SENTINEL = None


def logmel_gather(pool, row_offsets, frames, T):
    """A batch [B, 1, T, 40] out of kept log-mel rows (speech_loader.py) in one launch: utterance b is the `frames[b]`
    rows of `pool` ([rows, 40] fp32) from row `row_offsets[b]` on, then the 0 dB fill to T -- what
    `audio.log_mel(..., layout="nhwc", target_length=T)` gives for the utterances the rows were computed from, bit for
    bit.  `row_offsets` int64 and `frames` int32 are device vectors of one length; 0 <= frames[b] <= T and the rows
    they name lie inside the pool (the caller's business: they are device values).  No autograd."""
    lib = _lib_ready()
    T = int(T)
    if pool.dtype != torch.float32 or pool.dim() != 2 or pool.shape[1] != 40 or not pool.is_contiguous():
        raise ValueError("logmel_gather: pool must be a contiguous fp32 [rows, 40] tensor, got %s %s"
                         % (pool.dtype, tuple(pool.shape)))
    if (row_offsets.dtype != torch.int64 or frames.dtype != torch.int32 or row_offsets.dim() != 1
            or frames.shape != row_offsets.shape or row_offsets.numel() < 1):
        raise ValueError("logmel_gather: row_offsets (int64) and frames (int32) must be vectors of one length >= 1")
    if not (pool.is_cuda and row_offsets.device == pool.device and frames.device == pool.device):
        raise _lib.S2IError("logmel_gather runs on the MI355X kernel: pool, row_offsets and frames must share one "
                            "device, got %s, %s, %s" % (pool.device, row_offsets.device, frames.device))
    if T < 1:
        raise ValueError("logmel_gather: T must be >= 1")
    B = row_offsets.numel()
    shape = (B, 1, T, 40)
    if LOGMEL_GATHER_SENTINEL is None:
        out = torch.empty(shape, dtype=torch.float32, device=pool.device)
    else:
        out = torch.full(shape, LOGMEL_GATHER_SENTINEL, dtype=torch.float32, device=pool.device)
    check(lib.s2i_logmel_gather(ptr(pool.detach()), ptr(row_offsets.contiguous()), ptr(frames.contiguous()), B, T,
                                ptr(out), stream()), "s2i_logmel_gather")
    return out


# ---- SpecAugment of a log-mel batch -------------------------------------------------------------------------------------
SPECAUG_MAX_MASKS, SPECAUG_MAX_FREQ_WIDTH = 8, 20


def _specaug_count_width(token, value, max_width):
    count, sep, width = value.partition("x")
    try:
        if not sep:
            raise ValueError
        count, width = int(count), int(width)
    except ValueError:
        raise ValueError("bad augmentation %r: expected COUNTxWIDTH, two integers" % token) from None
    if not 0 <= count <= SPECAUG_MAX_MASKS:
        raise ValueError("bad augmentation %r: the mask count must lie in [0, %d]" % (token, SPECAUG_MAX_MASKS))
    if width < 0 or (max_width is not None and width > max_width):
        raise ValueError("bad augmentation %r: the width must be %s" %
                         (token, ">= 0" if max_width is None else "in [0, %d]" % max_width))
    return count, width


def specaug_policy(spec):
    """'freq=2x8,time=2x40,ratio=0.2' (any order, any subset; '' = off -> None) -> (freq_masks, freq_width, time_masks,
    time_width, time_ratio) of s2i_specaug: count x maximum width per kind, at most 8 masks of a kind, frequency masks at
    most 20 bins wide; `ratio` (default 1.0, in (0, 1]) caps a time mask at that share of the utterance's frames."""
    values = {"freq": (0, 0), "time": (0, 0), "ratio": 1.0}
    seen = set()
    for token in str(spec).split(","):
        token = token.strip()
        if not token:
            continue
        key, sep, value = token.partition("=")
        key = key.strip()
        if not sep or key not in values:
            raise ValueError("unknown augmentation %r: expected a comma-separated subset of freq=NxW, time=NxW, ratio=R" % token)
        if key in seen:
            raise ValueError("augmentation %r given twice" % token)
        seen.add(key)
        if key == "ratio":
            try:
                ratio = float(value)
            except ValueError:
                raise ValueError("bad augmentation %r: expected ratio=R, a number" % token) from None
            if not 0.0 < ratio <= 1.0:      # a NaN fails both
                raise ValueError("bad augmentation %r: the ratio must lie in (0, 1]" % token)
            values[key] = ratio
        else:
            values[key] = _specaug_count_width(token, value.strip(), SPECAUG_MAX_FREQ_WIDTH if key == "freq" else None)
    if not seen:
        return None
    return values["freq"] + values["time"] + (values["ratio"],)


def specaug(mel, valid, policy, seed, step, out=None):
    """SpecAugment of a log-mel batch [B, 1, T, 40] (s2i_specaug; include/s2i_hip.h has the definitions): `policy`
    (specaug_policy's tuple, or its spec string) frequency and time masks per utterance over its first valid[b] rows, the
    masked cells set to the mean of those rows, everything else copied bit for bit.  The masks are a function of
    (seed, step, b) alone, drawn on the device by a counter-based generator: nothing random is uploaded and no generator
    state exists.  `valid`: B frame counts in [0, T], a sequence or an int32 device vector.  Returns a new tensor, or `out`
    (`out=mel` works in place).  One reduction and one apply launch; no autograd, no CPU fallback."""
    lib = _lib_ready()
    if isinstance(policy, str):
        policy = specaug_policy(policy) or (0, 0, 0, 0, 1.0)
    fm, fw, tm, tw, ratio = policy
    if not mel.is_cuda:
        raise _lib.S2IError("specaug runs on the MI355X kernel: mel is on %s" % mel.device)
    if mel.dtype != torch.float32 or mel.dim() != 4 or mel.shape[1] != 1 or mel.shape[3] != 40 or not mel.is_contiguous():
        raise ValueError("specaug: mel must be a contiguous fp32 [B, 1, T, 40] tensor, got %s %s"
                         % (mel.dtype, tuple(mel.shape)))
    B, T = mel.shape[0], mel.shape[2]
    if B < 1 or T < 1:
        raise ValueError("specaug: empty batch %s" % (tuple(mel.shape),))
    if not torch.is_tensor(valid):
        valid = [int(v) for v in valid]
        if len(valid) != B or min(valid) < 0 or max(valid) > T:
            raise ValueError("specaug: valid must hold %d frame counts in [0, %d], got %s" % (B, T, valid))
        valid = torch.tensor(valid, dtype=torch.int32, device=mel.device)
    elif valid.dtype != torch.int32 or tuple(valid.shape) != (B,) or valid.device != mel.device:
        raise ValueError("specaug: valid must be an int32 vector of %d entries on %s, got %s %s on %s"
                         % (B, mel.device, valid.dtype, tuple(valid.shape), valid.device))
    if out is None:
        out = torch.empty_like(mel)
    elif out.dtype != mel.dtype or out.shape != mel.shape or out.device != mel.device or not out.is_contiguous():
        raise ValueError("specaug: out must match mel (contiguous fp32 %s on %s)" % (tuple(mel.shape), mel.device))
    ws = _ws.get(lib.s2i_specaug_workspace_bytes(B), mel.device)
    mask64 = (1 << 64) - 1
    check(lib.s2i_specaug(ptr(mel.detach()), ptr(valid.contiguous()), B, T, ptr(out), int(fm), int(fw), int(tm), int(tw),
                          float(ratio), int(seed) & mask64, int(step) & mask64, ptr(ws), ws.numel() * 4, stream()),
          "s2i_specaug")
    return out


# ---- speed and noise augmentation of waveforms --------------------------------------------------------------------------
WAVEAUG_KEY_XOR = 0x57415645        # into key word 1: no (key, counter) block is SpecAugment's
WAVEAUG_MAX_SPEEDS = 8
WAVEAUG_MIN_FRAMES = 64             # a perturbed clip under this many frames runs at speed 1.0
WAVE_MIX_MAX_LEN = 2 ** 31 - 5
WAVE_MIX_RUN = 8192
# the device table of s2i_wave_mix, 32 bytes per clip (include/s2i_hip.h)
WAVE_MIX_ENTRY = [("g_white", "<f4"), ("g_babble", "<f4"), ("src", "<i8"), ("n_j", "<i4"), ("start", "<i4"),
                  ("uid", "<u4"), ("pad", "<i4")]
REVERB_KEY_XOR = 0x52455642         # into key word 1: no (key, counter) block is SpecAugment's or the other waveform draws'
REVERB_MAX_TAPS = 16000
REVERB_MAX_LEN = 2 ** 31 - 8225
# the device table of s2i_reverb_rir and s2i_reverb, 16 bytes per clip (include/s2i_hip.h)
REVERB_ENTRY = [("alpha", "<f4"), ("slope", "<f4"), ("taps", "<i4"), ("uid", "<u4")]
STRETCH_KEY_XOR = 0x53545243        # "STRC" into key word 1: the tempo and pitch draws share no block with any other draw
STRETCH_MAX_CHOICES = 8
STRETCH_RATE_GRID = 50              # Hz: a pitch-shifted read rate is a multiple of it, so the polyphase table has L <= 320
STRETCH_NFFT, STRETCH_HOP = 512, 128
STRETCH_MAX_LEN = 2 ** 29 - 1025
# the device table of s2i_time_stretch, 16 bytes per clip (include/s2i_hip.h)
STRETCH_ENTRY = [("rate", "<f8"), ("out_len", "<i4"), ("out_frames", "<i4")]


def _waveaug_noise(token, value):
    prob, sep, span = value.partition("@")
    lo, sep2, hi = span.partition(":")
    try:
        if not sep or not sep2:
            raise ValueError
        prob, lo, hi = float(prob), float(lo), float(hi)
    except ValueError:
        raise ValueError("bad augmentation %r: expected P@LO:HI, a probability and an SNR range in dB" % token) from None
    if not 0.0 < prob <= 1.0:       # a NaN fails both
        raise ValueError("bad augmentation %r: the probability must lie in (0, 1]" % token)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("bad augmentation %r: the SNR range needs finite LO <= HI" % token)
    return prob, lo, hi


def _waveaug_reverb(token, value):
    parts = value.split("@")
    try:
        if len(parts) != 3:
            raise ValueError
        prob = float(parts[0])
        (lo, sep, hi), (dlo, sep2, dhi) = parts[1].partition(":"), parts[2].partition(":")
        if not sep or not sep2:
            raise ValueError
        lo, hi, dlo, dhi = float(lo), float(hi), float(dlo), float(dhi)
    except ValueError:
        raise ValueError("bad augmentation %r: expected P@LO:HI@DLO:DHI, a probability, a T60 range in seconds and a range "
                         "of the direct-to-reverberant ratio in dB" % token) from None
    if not 0.0 < prob <= 1.0:       # a NaN fails both
        raise ValueError("bad augmentation %r: the probability must lie in (0, 1]" % token)
    if not 0.05 <= lo <= hi <= 1.0:
        raise ValueError("bad augmentation %r: the T60 range needs 0.05 <= LO <= HI <= 1.0 seconds" % token)
    if not -20.0 <= dlo <= dhi <= 60.0:
        raise ValueError("bad augmentation %r: the direct-to-reverberant range needs -20 <= DLO <= DHI <= 60 dB" % token)
    return prob, lo, hi, dlo, dhi


def _waveaug_speeds(token, value):
    from . import audio
    parts = value.split("/")
    if not 1 <= len(parts) <= WAVEAUG_MAX_SPEEDS:
        raise ValueError("bad augmentation %r: 1 to %d speed factors" % (token, WAVEAUG_MAX_SPEEDS))
    rates = []
    for part in parts:
        try:
            s = float(part)
        except ValueError:
            raise ValueError("bad augmentation %r: %r is not a number" % (token, part)) from None
        if not 0.5 <= s <= 2.0:
            raise ValueError("bad augmentation %r: a speed factor must lie in [0.5, 2.0]" % token)
        rate = round(audio.SAMPLE_RATE * s)
        if abs(audio.SAMPLE_RATE * s - rate) > 1e-6:
            raise ValueError("bad augmentation %r: %d x %s is not a whole sample rate" % (token, audio.SAMPLE_RATE, part))
        try:
            audio.resample_plan(rate)
        except ValueError as e:
            raise ValueError("bad augmentation %r: %s" % (token, e)) from None
        rates.append(int(rate))
    return tuple(rates)


def _waveaug_choices(token, value, what, lo, hi):
    parts = value.split("/")
    if not 1 <= len(parts) <= STRETCH_MAX_CHOICES:
        raise ValueError("bad augmentation %r: 1 to %d %s" % (token, STRETCH_MAX_CHOICES, what))
    out = []
    for part in parts:
        try:
            v = float(part)
        except ValueError:
            raise ValueError("bad augmentation %r: %r is not a number" % (token, part)) from None
        if not lo <= v <= hi:       # a NaN fails both
            raise ValueError("bad augmentation %r: %s must lie in [%g, %g]" % (token, what, lo, hi))
        out.append(v)
    return tuple(out)


def _waveaug_tempo(token, value):
    return _waveaug_choices(token, value, "tempo factors", 0.5, 2.0)


def _waveaug_pitch(token, value):
    return _waveaug_choices(token, value, "semitone values", -12.0, 12.0)


def stretch_read_rate(speed_rate, semitones):
    """The rate a clip drawn at `speed_rate` Hz and shifted by `semitones` is read at: the speed's own rate where the
    shift is 0, else 50 round(speed_rate 2^(semitones / 12) / 50) in float64 (under 6 cents off the asked pitch)."""
    if semitones == 0:
        return int(speed_rate)
    return STRETCH_RATE_GRID * int(round(speed_rate * 2.0 ** (semitones / 12.0) / STRETCH_RATE_GRID))


def waveaug_policy(spec):
    """'speed=0.9/1.0/1.1,reverb=0.3@0.2:0.6@0:15,white=0.3@5:25,babble=0.2@0:15' (any order, any subset; '' = off ->
    None) -> a dict
    {"rates": the sample rates 16000 s a clip is read at, one per speed factor (None without speed=),
     "white": (P, LO, HI) or None, "babble": (P, LO, HI) or None}
    and, only where reverb= was given, "reverb": (P, LO, HI, DLO, DHI) (read it with .get).
    speed= takes 1 to 8 factors in [0.5, 2.0], each of which makes 16000 s a whole rate `audio.resample_plan` accepts; an
    utterance draws one uniformly.  reverb=P@LO:HI@DLO:DHI convolves a clip, with probability P in (0, 1], with a room
    impulse response drawn on the device: T60 uniform in [LO, HI] seconds (0.05 <= LO <= HI <= 1.0) and the
    direct-to-reverberant ratio uniform in [DLO, DHI] dB (within [-20, 60]); it is applied after the speed and before the
    noise, whose power is then the reverberated clip's.  white= and babble= add noise or another utterance with
    probability P in (0, 1] at a signal-to-noise ratio drawn uniformly from [LO, HI] dB.  There is no gain key on purpose:
    power_to_db(ref=max) and the mean subtraction of the log-mel front end make the features invariant to a clip's
    gain.
    tempo=F/F/... (1 to 8 factors in [0.5, 2.0]) divides a clip's duration by the factor it draws and keeps its pitch;
    pitch=S/S/... (1 to 8 semitone values in [-12, 12]) multiplies the pitch by 2^(S / 12) and keeps the duration.  Both
    run the phase vocoder s2i_time_stretch before the resampler, which then reads the clip at one combined rate
    (`waveaug_plan`); the order is stretch, resample, reverb, noise.  "tempo" and "pitch" (tuples of floats) are in the dict
    only where given (read them with .get).  Every rate a (speed, pitch) pair of the spec can produce must be one
    `audio.resample_plan` accepts, and every (speed, tempo, pitch) triple's stretch tau Rs / R must lie in [0.25, 4], the
    kernel's range (at the corners of the two ranges the 50 Hz grid can round it past 4); the pitch token is named
    otherwise."""
    from . import audio
    values = {"speed": None, "white": None, "babble": None, "reverb": None, "tempo": None, "pitch": None}
    tokens = {}
    seen = set()
    for token in str(spec).split(","):
        token = token.strip()
        if not token:
            continue
        key, sep, value = token.partition("=")
        key = key.strip()
        if not sep or key not in values:
            raise ValueError("unknown augmentation %r: expected a comma-separated subset of speed=S/S/..., white=P@LO:HI, "
                             "babble=P@LO:HI, reverb=P@LO:HI@DLO:DHI, tempo=F/F/..., pitch=S/S/..." % token)
        if key in seen:
            raise ValueError("augmentation %r given twice" % token)
        seen.add(key)
        tokens[key] = token
        parse = {"speed": _waveaug_speeds, "reverb": _waveaug_reverb, "tempo": _waveaug_tempo,
                 "pitch": _waveaug_pitch}.get(key, _waveaug_noise)
        values[key] = parse(token, value.strip())
    if not seen:
        return None
    policy = {"rates": values["speed"], "white": values["white"], "babble": values["babble"]}
    for key in ("reverb", "tempo", "pitch"):
        if values[key] is not None:
            policy[key] = values[key]
    if values["pitch"] is not None:
        for speed_rate in values["speed"] or (audio.SAMPLE_RATE,):
            for semis in values["pitch"]:
                try:
                    audio.resample_plan(stretch_read_rate(speed_rate, semis))
                except ValueError as e:
                    raise ValueError("bad augmentation %r: %s semitones at %d Hz: %s"
                                     % (tokens["pitch"], semis, speed_rate, e)) from None
                # the 50 Hz grid can round the rate past the corner of the two ranges: 7225 Hz -> 7200, tempo 2 -> 4.014
                rate = stretch_read_rate(speed_rate, semis)
                for tempo in values["tempo"] or (1.0,):
                    rho = tempo * speed_rate / rate
                    if not 0.25 <= rho <= 4.0:
                        raise ValueError("bad augmentation %r: %s semitones at %d Hz and tempo %s need a time stretch by "
                                         "%.4f, outside [0.25, 4]" % (tokens["pitch"], semis, speed_rate, tempo, rho))
    return policy


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011; the rounds of include/s2i_hip.h) over numpy arrays of counters and one key:
    a uint32 array [4, ...] of output words.  Host only; nothing is launched."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def waveaug_uniforms(seed, step, uids, group):
    """float32 [4, n]: u = (r >> 8) 2^-24 of the four words of block `group` of every uid, on key
    (seed mod 2^32, (seed div 2^32) ^ WAVEAUG_KEY_XOR) and counter (step mod 2^32, step div 2^32, uid, group)."""
    import numpy as np
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    uids = np.asarray(uids, dtype=np.uint64).reshape(-1)
    r = philox4x32_10(step & 0xFFFFFFFF, step >> 32, uids, group, seed & 0xFFFFFFFF, (seed >> 32) ^ WAVEAUG_KEY_XOR)
    return (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _waveaug_index(u, n):
    """min(int(u (float)n), n - 1): one fp32 product, truncated (SpecAugment's rule), elementwise"""
    import numpy as np
    n = np.asarray(n, dtype=np.int64)
    return np.minimum((u.astype(np.float32) * n.astype(np.float32)).astype(np.int64), n - 1)


def waveaug_plan(policy, seed, step, uids, lens, pool_lens=None, pool_q=None, target_length=None):
    """The per-utterance draws of a batch, a pure function of (seed, step, uid), made on the host.

    `lens`: each clip's 16 kHz samples; `pool_lens` and `pool_q`: the length and the float64 mean square of every stored
    utterance an interferer may be (needed for babble=).  Block 0 of a uid gives u_speed, u_white (apply if < P),
    u_white_snr, u_babble (apply if < P); block 1 gives u_babble_snr, u_src and u_start; snr = LO + u (HI - LO) in
    float64.  The speed index, the interferer j and the start inside it are min(int(u (float)n), n - 1).  A clip whose
    perturbed length would have under 64 frames runs at 16000 Hz (speed 1.0), whether or not 1.0 is listed.

    Returns a dict of arrays: rate (int64, the rate the clip is read at), out_len (int64), white_snr / babble_snr
    (float64, NaN where off), g_white / g_babble (float32, 0 where off: 10^(-snr / 10), for babble divided by Q_j; 0 also
    where Q_j == 0), src and start (int64), uid (uint32).

    reverb= draws from a key of its own, (seed mod 2^32, (seed div 2^32) ^ REVERB_KEY_XOR), at counter
    (step mod 2^32, step div 2^32, uid, 0): u_on (apply if < P), u_t60, u_drr, each (r >> 8) 2^-24; T60 and DRR are
    LO + u (HI - LO) in float64.  No field above depends on it.  It adds t60 and drr (float64, NaN where off), taps (int64,
    0 where off, else 32 ceil(T60 16000 / 32), at most 16000), slope (float32, -log2(1000) / (T60 16000) rounded once) and
    alpha (float32, sqrt(10^(-DRR / 10) / E), E = sum_{k=1}^{taps-1} 2^(2 k slope) in float64 over the rounded slope, the
    geometric series summed in closed form): the tail's expected energy is 10^(-DRR / 10) of the direct path's.  Without reverb= the five fields are absent.

    tempo= and pitch= draw from a third key, (seed mod 2^32, (seed div 2^32) ^ STRETCH_KEY_XOR), at counter
    (step mod 2^32, step div 2^32, uid, 0): word 0 gives the tempo index and word 1 the pitch index, each
    min(int(u (float)n), n - 1) with u = (r >> 8) 2^-24 (a key that is absent draws tempo 1 / 0 semitones).  With Rs the
    drawn speed rate (16000 without speed=), tau the tempo and S the semitones, all in float64: the read rate is R = Rs
    where S == 0, else 50 round(Rs 2^(S / 12) / 50); the stretch is rho = tau Rs / R (no stretch where rho == 1: the clip
    is read in place); stretch_len = floor(n / rho + 0.5) and out_len = audio.resampled_length(stretch_len, R), so the
    duration is n / (tau Rs / 16000) whatever S is.  A clip whose out_len would have under 64 frames is left wholly
    unperturbed (16000 Hz, no stretch), the speed rule.  `rate` is then R and `out_len` the final length; the fields tempo,
    semitones, stretch_rate (float64) and stretch_len (int64) are added.  Without the two keys they are absent and no field
    above changes."""
    import numpy as np
    from . import audio
    uids = np.asarray(uids, dtype=np.int64).reshape(-1)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if len(uids) != len(lens) or len(uids) < 1 or uids.min() < 0 or uids.max() >= 2 ** 32:
        raise ValueError("waveaug_plan: need one 32-bit uid per clip, got %d uids for %d clips" % (len(uids), len(lens)))
    B = len(uids)
    u0 = waveaug_uniforms(seed, step, uids, 0)
    u1 = waveaug_uniforms(seed, step, uids, 1)
    rate = np.full(B, audio.SAMPLE_RATE, dtype=np.int64)
    if policy["rates"] is not None:
        rates = np.array(policy["rates"], dtype=np.int64)
        rate = rates[_waveaug_index(u0[0], np.full(B, len(rates)))]
    nf = (audio.n_frames if target_length is None else lambda n: audio.n_frames(n, target_length))
    stretch = None
    if policy.get("tempo") is not None or policy.get("pitch") is not None:
        stretch = _stretch_plan(policy, seed, step, uids, lens, rate, nf)
        rate, out_len = stretch.pop("rate"), stretch.pop("out_len")
    else:
        out_len = np.array([audio.resampled_length(n, r) for n, r in zip(lens, rate)], dtype=np.int64)
        for b in range(B):
            if rate[b] != audio.SAMPLE_RATE and nf(out_len[b]) < WAVEAUG_MIN_FRAMES:
                rate[b], out_len[b] = audio.SAMPLE_RATE, lens[b]
    plan = dict(rate=rate, out_len=out_len, uid=uids.astype(np.uint32), white_snr=np.full(B, np.nan),
                babble_snr=np.full(B, np.nan), g_white=np.zeros(B, np.float32), g_babble=np.zeros(B, np.float32),
                src=np.zeros(B, np.int64), start=np.zeros(B, np.int64))
    if policy["white"] is not None:
        p, lo, hi = policy["white"]
        on = u0[1].astype(np.float64) < p
        snr = lo + u0[2].astype(np.float64) * (hi - lo)
        plan["white_snr"] = np.where(on, snr, np.nan)
        plan["g_white"] = np.where(on, 10.0 ** (-snr / 10.0), 0.0).astype(np.float32)
    if policy["babble"] is not None:
        if pool_lens is None or pool_q is None or len(pool_lens) < 1:
            raise ValueError("waveaug_plan: babble needs a pool of stored utterances to draw interferers from")
        pool_lens = np.asarray(pool_lens, dtype=np.int64)
        pool_q = np.asarray(pool_q, dtype=np.float64)
        if len(pool_lens) >= 2 ** 24 or pool_lens.min() < 1:
            raise ValueError("waveaug_plan: a pool holds 1 to 2^24 - 1 utterances of at least one sample")
        p, lo, hi = policy["babble"]
        on = u0[3].astype(np.float64) < p
        snr = lo + u1[0].astype(np.float64) * (hi - lo)
        src = _waveaug_index(u1[1], np.full(B, len(pool_lens)))
        q = pool_q[src]
        on_q = on & (q > 0.0)
        plan["babble_snr"] = np.where(on, snr, np.nan)
        plan["g_babble"] = np.where(on_q, 10.0 ** (-snr / 10.0) / np.where(q > 0.0, q, 1.0), 0.0).astype(np.float32)
        plan["src"] = src
        plan["start"] = _waveaug_index(u1[2], pool_lens[src])
    if policy.get("reverb") is not None:
        plan.update(_reverb_plan(policy["reverb"], seed, step, uids))
    if stretch is not None:
        plan.update(stretch)
    return plan


def _stretch_plan(policy, seed, step, uids, lens, speed_rate, nf):
    """the tempo= / pitch= fields of waveaug_plan, with the rate and out_len they replace"""
    import numpy as np
    from . import audio
    tempos, pitches = policy.get("tempo") or (1.0,), policy.get("pitch") or (0.0,)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    r = philox4x32_10(step & 0xFFFFFFFF, step >> 32, np.asarray(uids, dtype=np.uint64), 0, seed & 0xFFFFFFFF,
                      (seed >> 32) ^ STRETCH_KEY_XOR)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    B = len(uids)
    tempo = np.array(tempos, dtype=np.float64)[_waveaug_index(u[0], np.full(B, len(tempos)))]
    semis = np.array(pitches, dtype=np.float64)[_waveaug_index(u[1], np.full(B, len(pitches)))]
    rate, out_len = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    rho, stretch_len = np.ones(B, dtype=np.float64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n, rs = int(lens[b]), int(speed_rate[b])
        rate[b] = stretch_read_rate(rs, float(semis[b]))
        rho[b] = float(tempo[b]) * rs / float(rate[b])
        stretch_len[b] = n if rho[b] == 1.0 else int(math.floor(n / rho[b] + 0.5))
        out_len[b] = audio.resampled_length(stretch_len[b], rate[b])
        if (rate[b] != audio.SAMPLE_RATE or rho[b] != 1.0) and nf(out_len[b]) < WAVEAUG_MIN_FRAMES:
            rate[b], out_len[b], stretch_len[b] = audio.SAMPLE_RATE, n, n
            rho[b], tempo[b], semis[b] = 1.0, 1.0, 0.0
    return dict(rate=rate, out_len=out_len, tempo=tempo, semitones=semis, stretch_rate=rho, stretch_len=stretch_len)


def stretch_table(plan):
    """The 16-byte-per-clip table of s2i_time_stretch (STRETCH_ENTRY) out of a waveaug_plan made under tempo= or pitch=:
    rate = stretch_rate and out_len = stretch_len.  out_frames = ceil((1 + n div 128) / rate) needs the clips' lengths,
    which the plan does not hold: `time_stretch_prepare` fills it in from its `lens`."""
    import numpy as np
    if "stretch_rate" not in plan:
        raise ValueError("stretch_table: the plan was made without tempo= or pitch=")
    t = np.zeros(len(plan["uid"]), dtype=STRETCH_ENTRY)
    t["rate"], t["out_len"] = plan["stretch_rate"], plan["stretch_len"]
    return t


def stretch_basis64():
    """(forward [512 samples][512 columns], inverse [512 rows][512 samples], window [512]) of s2i_time_stretch in float64,
    the periodic Hann window folded into both matrices (include/s2i_hip.h).  Forward column 32 t + 16 h + c is bin
    k = 16 t + c: w cos where h = 0, -w sin where h = 1; bin 0's h = 1 column is bin 256's cosine."""
    import numpy as np
    N = STRETCH_NFFT
    i = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / N)
    ang = lambda k: 2.0 * np.pi * ((i * k) % N) / N          # noqa: E731
    fwd, inv = np.zeros((N, N)), np.zeros((N, N))
    for k in range(N // 2):
        t, c = divmod(k, 16)
        fwd[:, 32 * t + c] = w * np.cos(ang(k))
        fwd[:, 32 * t + 16 + c] = -w * np.sin(ang(k)) if k else w * np.cos(ang(N // 2))
    for k in range(N // 2 + 1):
        inv[k] = (1.0 if k in (0, N // 2) else 2.0) * (w / N) * np.cos(ang(k))
    for k in range(1, N // 2):
        inv[N // 2 + k] = -2.0 * (w / N) * np.sin(ang(k))
    return fwd, inv, w


def pack_stretch_basis(m):
    """[512][512] -> the fragment order of include/s2i_hip.h: element (r, c of column tile nt) at
    ((r // 16 * 32 + nt) * 64 + (r % 4) * 16 + c) * 4 + (r % 16) // 4"""
    import numpy as np
    b = np.asarray(m).reshape(STRETCH_NFFT // 16, 4, 4, STRETCH_NFFT // 16, 16)     # [kg][u][g][nt][c], r = 16 kg + 4 u + g
    return np.ascontiguousarray(b.transpose(0, 3, 2, 4, 1)).reshape(-1)             # [kg][nt][g][c][u]


_STRETCH_BASIS = {}


def device_stretch_basis(device):
    """forward | inverse | window as one fp32 device tensor, rounded once from float64 and built once per device"""
    import numpy as np
    key = str(device)
    if key not in _STRETCH_BASIS:
        lib = _lib.load()
        fwd, inv, w = stretch_basis64()
        flat = np.concatenate([pack_stretch_basis(fwd), pack_stretch_basis(inv), w]).astype(np.float32)
        if flat.size != lib.s2i_stretch_basis_elems():
            raise _lib.S2IError("the stretch basis has %d floats, the library expects %d" % (flat.size, lib.s2i_stretch_basis_elems()))
        _STRETCH_BASIS[key] = torch.from_numpy(flat).to(device)
    return _STRETCH_BASIS[key]


def _reverb_plan(term, seed, step, uids):
    """the reverb fields of waveaug_plan"""
    import numpy as np
    from . import audio
    p, lo, hi, dlo, dhi = term
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    r = philox4x32_10(step & 0xFFFFFFFF, step >> 32, np.asarray(uids, dtype=np.uint64), 0, seed & 0xFFFFFFFF,
                      (seed >> 32) ^ REVERB_KEY_XOR)
    u = ((r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float64)
    B = len(uids)
    on = u[0] < p
    t60 = lo + u[1] * (hi - lo)
    drr = dlo + u[2] * (dhi - dlo)
    taps = np.minimum(32 * np.ceil(t60 * audio.SAMPLE_RATE / 32.0).astype(np.int64), REVERB_MAX_TAPS)
    slope = (-math.log2(1000.0) / (t60 * audio.SAMPLE_RATE)).astype(np.float32)
    # E = sum_{k=1}^{taps-1} q^k with q = 2^(2 slope) < 1, in closed form (float64): 16000 exponentials per clip on the host
    # would cost more than the convolution does on the device
    q = np.exp2(2.0 * slope.astype(np.float64))
    energy = q * (1.0 - q ** (taps - 1).astype(np.float64)) / (1.0 - q)
    alpha = np.where(on, np.sqrt(10.0 ** (-drr / 10.0) / energy), 0.0).astype(np.float32)
    return dict(t60=np.where(on, t60, np.nan), drr=np.where(on, drr, np.nan), taps=np.where(on, taps, 0).astype(np.int64),
                slope=np.where(on, slope, np.float32(0)).astype(np.float32), alpha=alpha)


def reverb_table(plan):
    """The 16-byte-per-clip table of s2i_reverb_rir and s2i_reverb (REVERB_ENTRY) out of a waveaug_plan made under
    reverb=."""
    import numpy as np
    if "taps" not in plan:
        raise ValueError("reverb_table: the plan was made without reverb=")
    t = np.zeros(len(plan["uid"]), dtype=REVERB_ENTRY)
    t["alpha"], t["slope"], t["taps"], t["uid"] = plan["alpha"], plan["slope"], plan["taps"], plan["uid"]
    return t


def wave_mix_table(plan, pool_offsets=None, pool_lens=None):
    """The 32-byte-per-clip table of s2i_wave_mix (WAVE_MIX_ENTRY) out of a waveaug_plan: `pool_offsets` and `pool_lens`
    give each stored utterance's first sample (in floats from the pool's start) and its length."""
    import numpy as np
    B = len(plan["uid"])
    t = np.zeros(B, dtype=WAVE_MIX_ENTRY)
    t["g_white"], t["g_babble"], t["uid"] = plan["g_white"], plan["g_babble"], plan["uid"]
    t["n_j"] = 1
    if pool_offsets is not None:
        src = plan["src"]
        t["src"], t["n_j"], t["start"] = np.asarray(pool_offsets)[src], np.asarray(pool_lens)[src], plan["start"]
    elif np.any(plan["g_babble"] != 0):
        raise ValueError("wave_mix_table: babble needs the pool's offsets and lengths")
    return t


def wave_mix_prepare(x, offsets, lens, table, pool=None):
    """The checked and uploaded arguments of one s2i_wave_mix call (include/s2i_hip.h has the definitions), for
    `wave_mix_launch`: clip b is x[offsets[b] : offsets[b] + lens[b]] of the flat fp32 device tensor `x`; `table` is a
    numpy array of WAVE_MIX_ENTRY rows (wave_mix_table), `pool` the flat fp32 device tensor the interferers are read from
    (None: no babble).  offsets, lens and table are HOST arrays: they are checked against x and pool here -- the kernel
    trusts them -- and go up in one copy.  Nothing is launched."""
    import numpy as np
    _lib_ready()
    if not x.is_cuda:
        raise _lib.S2IError("wave_mix runs on the MI355X kernel: x is on %s" % x.device)
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
        raise ValueError("wave_mix: x must be a flat contiguous fp32 tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
    table = np.ascontiguousarray(table, dtype=WAVE_MIX_ENTRY).reshape(-1)
    B = len(offsets)
    if B < 1 or len(lens) != B or len(table) != B:
        raise ValueError("wave_mix: offsets, lens and table must have one length >= 1, got %d, %d, %d"
                         % (B, len(lens), len(table)))
    if lens.min() < 0 or lens.max() > WAVE_MIX_MAX_LEN or offsets.min() < 0 or int((offsets + lens).max()) > x.numel():
        raise ValueError("wave_mix: a clip lies outside x (%d floats) or is longer than %d" % (x.numel(), WAVE_MIX_MAX_LEN))
    order = np.argsort(offsets, kind="stable")
    if np.any(offsets[order][1:] < (offsets + lens)[order][:-1]):
        raise ValueError("wave_mix: clips overlap")
    if not (np.all(np.isfinite(table["g_white"])) and np.all(np.isfinite(table["g_babble"]))
            and table["g_white"].min() >= 0 and table["g_babble"].min() >= 0):
        raise ValueError("wave_mix: gains must be finite and >= 0")
    bab = table["g_babble"] != 0
    if bab.any():
        if pool is None:
            raise ValueError("wave_mix: babble needs a pool")
        if (pool.dtype != torch.float32 or pool.dim() != 1 or not pool.is_contiguous() or pool.device != x.device
                or pool.data_ptr() == x.data_ptr()):
            raise ValueError("wave_mix: pool must be a flat contiguous fp32 tensor on %s, apart from x" % x.device)
        t = table[bab]
        if (t["n_j"].min() < 1 or t["src"].min() < 0 or int((t["src"] + t["n_j"]).max()) > pool.numel()
                or t["start"].min() < 0 or np.any(t["start"] >= t["n_j"])):
            raise ValueError("wave_mix: an interferer lies outside the pool (%d floats) or its start outside it"
                             % pool.numel())
    max_len = max(int(lens.max()), 1)
    # one upload: offsets | table | lens, each part on a 16-byte boundary
    at_table = (8 * B + 15) // 16 * 16
    at_lens = at_table + 32 * B
    image = np.zeros(at_lens + 4 * B, dtype=np.uint8)
    image[:8 * B] = offsets.view(np.uint8)
    image[at_table:at_lens] = table.view(np.uint8)
    image[at_lens:] = lens.astype(np.int32).view(np.uint8)
    image_d = torch.from_numpy(image).to(x.device)
    base = image_d.data_ptr()
    return dict(x=x, image=image_d, offsets=base, lens=base + at_lens, table=base + at_table, B=B, max_len=max_len,
                pool=pool if bab.any() else None)


def wave_mix_launch(args, seed, step):
    """s2i_wave_mix on the current stream over `wave_mix_prepare`'s arguments: the two launches and nothing else."""
    lib = _lib.load()
    x = args["x"]
    ws = _ws.get(lib.s2i_wave_mix_workspace_bytes(args["B"], args["max_len"]), x.device)
    mask64 = (1 << 64) - 1
    check(lib.s2i_wave_mix(ptr(x), args["offsets"], args["lens"], args["B"], args["max_len"], ptr(args["pool"]), args["table"],
                           int(seed) & mask64, int(step) & mask64, ptr(ws), ws.numel() * 4, stream()), "s2i_wave_mix")
    return x


def wave_mix(x, offsets, lens, table, seed, step, pool=None):
    """White noise and babble on a ragged batch of waveforms, in place: `wave_mix_prepare` (checks, one upload) then
    `wave_mix_launch` (two launches).  y_i = (x_i + a_w e_i) + a_b v_i with the noise a function of (seed, step, uid, i)
    alone.  No autograd, no CPU fallback.  Returns x."""
    return wave_mix_launch(wave_mix_prepare(x, offsets, lens, table, pool), seed, step)


def reverb(x, offsets, lens, table, seed, step, out=None):
    """Room reverberation of a ragged batch of waveforms: clip b = x[offsets[b] : offsets[b] + lens[b]] of the flat fp32
    device tensor `x` convolved with the room impulse response that row b of `table` (numpy REVERB_ENTRY rows,
    reverb_table) and (seed, step, uid) define; include/s2i_hip.h has the definitions.  The clips keep their lengths; a
    clip with taps == 0 is copied bit for bit.  offsets, lens and table are HOST arrays, checked here against x -- the
    kernels trust them -- and uploaded in one copy; then s2i_reverb_rir and s2i_reverb on the current stream.  Returns a
    new flat tensor laid out as x (`out`, where given: same shape, dtype and device, apart from x), of which only the clips
    are written.  No autograd, no CPU fallback."""
    import numpy as np
    _lib_ready()
    if not x.is_cuda:
        raise _lib.S2IError("reverb runs on the MI355X kernels: x is on %s" % x.device)
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
        raise ValueError("reverb: x must be a flat contiguous fp32 tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
    table = np.ascontiguousarray(table, dtype=REVERB_ENTRY).reshape(-1)
    B = len(offsets)
    if B < 1 or len(lens) != B or len(table) != B:
        raise ValueError("reverb: offsets, lens and table must have one length >= 1, got %d, %d, %d"
                         % (B, len(lens), len(table)))
    if lens.min() < 0 or lens.max() > REVERB_MAX_LEN or offsets.min() < 0 or int((offsets + lens).max()) > x.numel():
        raise ValueError("reverb: a clip lies outside x (%d floats) or is longer than %d" % (x.numel(), REVERB_MAX_LEN))
    order = np.argsort(offsets, kind="stable")
    if np.any(offsets[order][1:] < (offsets + lens)[order][:-1]):
        raise ValueError("reverb: clips overlap")
    taps = table["taps"].astype(np.int64)
    if taps.min() < 0 or taps.max() > REVERB_MAX_TAPS or np.any(taps % 32 != 0):
        raise ValueError("reverb: taps must be 0 or a multiple of 32 up to %d, got %s" % (REVERB_MAX_TAPS, taps.tolist()))
    if not (np.all(np.isfinite(table["alpha"])) and np.all(np.isfinite(table["slope"]))):
        raise ValueError("reverb: alpha and slope must be finite")
    if out is None:
        out = torch.empty_like(x)
    elif (out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous() or out.device != x.device
          or out.data_ptr() == x.data_ptr()):
        raise ValueError("reverb: out must be a flat contiguous fp32 tensor of x's size on %s, apart from x" % x.device)
    max_len, max_taps = max(int(lens.max()), 1), max(int(taps.max()), 32)
    # one upload: offsets | table | lens, each part on a 16-byte boundary
    at_table = (8 * B + 15) // 16 * 16
    at_lens = at_table + 16 * B
    image = np.zeros(at_lens + 4 * B, dtype=np.uint8)
    image[:8 * B] = offsets.view(np.uint8)
    image[at_table:at_lens] = table.view(np.uint8)
    image[at_lens:] = lens.astype(np.int32).view(np.uint8)
    image_d = torch.from_numpy(image).to(x.device)
    base = image_d.data_ptr()
    h = torch.empty(B * max_taps, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    mask64 = (1 << 64) - 1
    check(lib.s2i_reverb_rir(base + at_table, B, max_taps, ptr(h), int(seed) & mask64, int(step) & mask64, stream()),
          "s2i_reverb_rir")
    check(lib.s2i_reverb(ptr(x), base, base + at_lens, B, max_len, base + at_table, ptr(h), max_taps, ptr(out), stream()),
          "s2i_reverb")
    return out


def time_stretch_prepare(x, offsets, lens, table, out=None):
    """The checked and uploaded arguments of one s2i_time_stretch call, for `time_stretch_launch`: clip b is
    x[offsets[b] : offsets[b] + lens[b]] of the flat fp32 device tensor `x`; `table` is a numpy array of STRETCH_ENTRY rows
    (stretch_table) whose out_frames are filled in here from lens and rate.  offsets, lens and table are HOST arrays: they
    are checked against x here -- the kernels trust them -- and go up in one copy.  The stretched clips are laid out back
    to back, each on a 16-byte boundary, in a new flat tensor (`out`, where given: flat fp32 on x's device, apart from x,
    large enough).  Nothing is launched."""
    import numpy as np
    _lib_ready()
    if not x.is_cuda:
        raise _lib.S2IError("time_stretch runs on the MI355X kernels: x is on %s" % x.device)
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous() or x.data_ptr() % 16:
        raise ValueError("time_stretch: x must be a flat contiguous 16-byte aligned fp32 tensor, got %s %s"
                         % (x.dtype, tuple(x.shape)))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
    table = np.array(table, dtype=STRETCH_ENTRY).reshape(-1)
    B = len(offsets)
    if B < 1 or len(lens) != B or len(table) != B:
        raise ValueError("time_stretch: offsets, lens and table must have one length >= 1, got %d, %d, %d"
                         % (B, len(lens), len(table)))
    if lens.min() < 0 or lens.max() > STRETCH_MAX_LEN or offsets.min() < 0 or int((offsets + lens).max()) > x.numel():
        raise ValueError("time_stretch: a clip lies outside x (%d floats) or is longer than %d" % (x.numel(), STRETCH_MAX_LEN))
    if np.any(offsets % 4):
        raise ValueError("time_stretch: every clip must start on a 16-byte boundary")
    rate = table["rate"]
    if not np.all((rate == 1.0) | ((rate >= 0.25) & (rate <= 4.0))):       # a NaN fails both
        raise ValueError("time_stretch: a rate must be 1 or lie in [0.25, 4], got %s" % rate.tolist())
    on = (rate != 1.0) & (lens > 0)
    frames = np.where(on, 1 + lens // STRETCH_HOP, 0)
    want_len = np.where(rate == 1.0, lens, np.floor(lens / rate + 0.5)).astype(np.int64)
    if np.any(table["out_len"] != want_len):
        raise ValueError("time_stretch: out_len must be floor(n / rate + 0.5), got %s for %s" % (table["out_len"].tolist(), want_len.tolist()))
    out_frames = np.where(on, np.ceil(frames / rate), 0).astype(np.int64)
    table["out_frames"] = out_frames
    padded = (want_len + 3) // 4 * 4
    out_offsets = np.cumsum(padded) - padded
    floats = max(int(padded.sum()), 4)
    if out is None:
        out = torch.empty(floats, dtype=torch.float32, device=x.device)
    elif (out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous() or out.device != x.device
          or out.numel() < floats or out.data_ptr() % 16 or out.data_ptr() == x.data_ptr()):
        raise ValueError("time_stretch: out must be a flat contiguous 16-byte aligned fp32 tensor of at least %d floats on %s, "
                         "apart from x" % (floats, x.device))
    # one upload: offsets | out offsets | table | lens, each part on a 16-byte boundary
    at_out = (8 * B + 15) // 16 * 16
    at_table = 2 * at_out
    at_lens = at_table + 16 * B
    image = np.zeros(at_lens + 4 * B, dtype=np.uint8)
    image[:8 * B] = offsets.view(np.uint8)
    image[at_out:at_out + 8 * B] = out_offsets.astype(np.int64).view(np.uint8)
    image[at_table:at_lens] = table.view(np.uint8)
    image[at_lens:] = lens.astype(np.int32).view(np.uint8)
    image_d = torch.from_numpy(image).to(x.device)
    base = image_d.data_ptr()
    return dict(x=x, out=out, image=image_d, offsets=base, out_offsets=base + at_out, table=base + at_table,
                lens=base + at_lens, B=B, max_len=max(int(lens.max()), 1), max_out_len=int(want_len.max()),
                in_frames=int(frames.sum()), out_frames=int(out_frames.sum()), host_out_offsets=out_offsets,
                host_out_lens=want_len)


def time_stretch_launch(args):
    """s2i_time_stretch on the current stream over `time_stretch_prepare`'s arguments: the five launches, after the one
    allocation of their workspace.  Returns (out, out_offsets, out_lens), the last two int64 host arrays."""
    lib = _lib.load()
    x, out = args["x"], args["out"]
    need = lib.s2i_time_stretch_workspace_bytes(args["B"], args["in_frames"], args["out_frames"])
    if need == 0:
        raise _lib.S2IError("s2i_time_stretch_workspace_bytes: %s" % lib.s2i_last_error().decode())
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    check(lib.s2i_time_stretch(ptr(x), args["offsets"], args["lens"], args["B"], args["max_len"], args["table"],
                               ptr(device_stretch_basis(x.device)), ptr(out), args["out_offsets"], args["max_out_len"],
                               args["in_frames"], args["out_frames"], ptr(ws), ws.numel() * 4, stream()), "s2i_time_stretch")
    return out, args["host_out_offsets"], args["host_out_lens"]


def time_stretch(x, offsets, lens, table, out=None):
    """The phase-vocoder time stretch of a ragged batch of waveforms: clip b of the flat fp32 device tensor `x` comes back
    floor(n / rate + 0.5) samples long, its pitch unchanged (include/s2i_hip.h has the arithmetic); a clip whose rate is
    exactly 1 is copied bit for bit.  `time_stretch_prepare` (checks, one upload) then `time_stretch_launch` (five
    launches).  Returns (out, out_offsets, out_lens).  No autograd, no CPU fallback."""
    return time_stretch_launch(time_stretch_prepare(x, offsets, lens, table, out))


# ---- nearest-row search -------------------------------------------------------------------------------------------------
def score_rows(x, packed, n, out):
    """out[:Q * n] viewed [Q, n] = x [Q, Cp] times the first n rows of a gallery chunk packed with
    pack_weight(chunk, PACK_PLAIN): one launch of the fp32 1x1 matrix kernel, written compactly (row stride n) into the
    caller's flat fp32 buffer, which a search reuses for every chunk.  Q goes in as Q images of one pixel (_step_rows)."""
    lib = _lib_ready()
    Q, Cp = x.shape
    n = int(n)
    if (x.dtype != torch.float32 or not x.is_contiguous() or Cp % 4 or packed.dim() != 3 or packed.shape[0] != 1
            or packed.shape[1] < Cp or packed.shape[2] < n or out.dtype != torch.float32 or out.numel() < Q * n):
        raise ValueError("score_rows: x %s, packed %s, n %d and %d output floats do not fit"
                         % (tuple(x.shape), tuple(packed.shape), n, out.numel()))
    d = ConvDesc(CONV_K1, Q, 1, 1, Cp, 0, n, 0, 0, packed.shape[1], packed.shape[2], ACT_NONE, 0, n, 1, 0, 0, 0, 0,
                 TILE_ROWS, 0, 0)
    _log_exec("scores [%d,%d]x[%d,%d]" % (Q, Cp, n, Cp), Q, n, Cp, x.numel(), Cp * n, Q * n)
    wsb = lib.s2i_conv_workspace_bytes(ctypes.byref(d))
    ws = _ws.get(wsb, x.device)
    check(lib.s2i_conv_forward_cls(ctypes.byref(d), ptr(x), None, ptr(packed), None, None, ptr(out), None, ptr(ws),
                                   ws.numel() * 4, stream()), "s2i_conv_forward")
    return out[:Q * n].view(Q, n)


def topk_rows(scores, k, base=0, best=None, out=None):
    """(best_score [Q, k] fp32, best_row [Q, k] int32): for every row of `scores` ([Q, N] fp32, unit column stride, any
    row stride >= N) its k best entries, best first, as (score, base + column).  Higher scores first, equal scores by
    ascending row id, NaN ranked as -inf; slots beyond the candidates hold (-inf, -1); the scores come back bit for bit.
    `best` is a pair from an earlier call on other rows of the same queries: it is merged into, in place, and returned.
    `out` is a pair to overwrite instead of fresh tensors.  1 <= k <= 64.  No autograd."""
    k, base = int(k), int(base)
    if not torch.is_tensor(scores) or scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("topk_rows: scores must be an fp32 [Q, N] tensor")
    Q, N = scores.shape
    if Q < 1 or N < 1 or scores.stride(1) != 1 or scores.stride(0) < N:
        raise ValueError("topk_rows: scores %s with strides %s: need Q, N >= 1, unit column stride and row stride >= N"
                         % (tuple(scores.shape), tuple(scores.stride())))
    if not 1 <= k <= _lib.TOPK_MAX:
        raise ValueError("topk_rows: k %d outside 1..%d" % (k, _lib.TOPK_MAX))
    if base < 0 or base + N > 2 ** 31 - 1:
        raise ValueError("topk_rows: row ids %d .. %d leave int32" % (base, base + N - 1))
    if best is not None and out is not None:
        raise ValueError("topk_rows: give `best` (merge into) or `out` (overwrite), not both")
    if not scores.is_cuda:
        raise _lib.S2IError("topk_rows runs on the MI355X kernel: there is no CPU fallback (scores on %s)" % scores.device)
    lib = _lib_ready()
    pair = best if best is not None else out
    if pair is None:
        pair = (torch.empty((Q, k), dtype=torch.float32, device=scores.device),
                torch.empty((Q, k), dtype=torch.int32, device=scores.device))
    bs, br = pair
    if (bs.dtype != torch.float32 or br.dtype != torch.int32 or tuple(bs.shape) != (Q, k) or tuple(br.shape) != (Q, k)
            or not bs.is_contiguous() or not br.is_contiguous() or bs.device != scores.device or br.device != scores.device):
        raise ValueError("topk_rows: the result pair must be contiguous fp32 and int32 [%d, %d] tensors on %s"
                         % (Q, k, scores.device))
    check(lib.s2i_topk_rows(ptr(scores.detach()), Q, N, scores.stride(0), base, k, ptr(bs), ptr(br),
                            1 if best is not None else 0, stream()), "s2i_topk_rows")
    return bs, br


def _rank_vector(name, t, dtype, n, device):
    if (not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous()
            or t.device != device):
        raise ValueError("rank_rows: %s must be a contiguous %s vector of %d entries on %s"
                         % (name, str(dtype).replace("torch.", ""), n, device))


def rank_rows(scores, own_row, query_label, row_label, base, own_score, gt, eq, mode):
    """One [Q, N] block of scores (fp32, unit column stride, any row stride >= N; column j is gallery row base + j) folded
    into the per-query rank state (s2i_rank_rows; include/s2i_hip.h has the definitions).

    mode "gather": own_score[q] = scores[q][own_row[q] - base] for the q whose own row lies in this block; every other
                   q (own_row[q] = -1 among them) keeps its value.  query_label, row_label, gt and eq may be None.
    mode "count":  over the columns whose row_label[base + j] != query_label[q]: gt[q] += #(score > own_score[q]),
                   eq[q] += #(score == own_score[q]).  A NaN score counts in neither; a NaN own score puts every such
                   column into gt.  own_row may be None.

    own_row, query_label, gt, eq: int32 [Q]; own_score: fp32 [Q]; row_label: int32 over the whole gallery, indexed by
    global row.  Everything on the scores' device; the counters are accumulated in place (the caller zeroes them).
    Only comparisons: exact and run-to-run identical.  No autograd."""
    base = int(base)
    if mode not in ("gather", "count"):
        raise ValueError("rank_rows: mode must be 'gather' or 'count', got %r" % (mode,))
    if not torch.is_tensor(scores) or scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("rank_rows: scores must be an fp32 [Q, N] tensor")
    Q, N = scores.shape
    if Q < 1 or N < 1 or scores.stride(1) != 1 or scores.stride(0) < N:
        raise ValueError("rank_rows: scores %s with strides %s: need Q, N >= 1, unit column stride and row stride >= N"
                         % (tuple(scores.shape), tuple(scores.stride())))
    if base < 0 or base + N > 2 ** 31 - 1:
        raise ValueError("rank_rows: row ids %d .. %d leave int32" % (base, base + N - 1))
    if not scores.is_cuda:
        raise _lib.S2IError("rank_rows runs on the MI355X kernel: there is no CPU fallback (scores on %s)" % scores.device)
    dev = scores.device
    _rank_vector("own_score", own_score, torch.float32, Q, dev)
    n_labels = 0
    if mode == "gather":
        _rank_vector("own_row", own_row, torch.int32, Q, dev)
        query_label = row_label = gt = eq = None
    else:
        _rank_vector("query_label", query_label, torch.int32, Q, dev)
        _rank_vector("gt", gt, torch.int32, Q, dev)
        _rank_vector("eq", eq, torch.int32, Q, dev)
        if not torch.is_tensor(row_label) or row_label.dim() != 1:
            raise ValueError("rank_rows: row_label must be an int32 vector over the gallery's rows")
        n_labels = row_label.shape[0]
        _rank_vector("row_label", row_label, torch.int32, n_labels, dev)
        if base + N > n_labels:
            raise ValueError("rank_rows: rows %d .. %d pass the %d row labels" % (base, base + N - 1, n_labels))
        own_row = None
    lib = _lib_ready()
    check(lib.s2i_rank_rows(ptr(scores.detach()), Q, N, scores.stride(0), base, ptr(own_row), ptr(query_label),
                            ptr(row_label), n_labels, ptr(own_score), ptr(gt), ptr(eq),
                            _lib.RANK_GATHER if mode == "gather" else _lib.RANK_COUNT, stream()), "s2i_rank_rows")


# ---- kernel distance and nearest-neighbour manifolds (s2i_manifold.hip) ---------------------------------------------------
def _block(name, scores, base):
    """(Q, N, device) of one [Q, N] block of scores, checked as topk_rows and rank_rows check theirs."""
    if not torch.is_tensor(scores) or scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError("%s: scores must be an fp32 [Q, N] tensor" % name)
    Q, N = scores.shape
    if Q < 1 or N < 1 or scores.stride(1) != 1 or scores.stride(0) < N:
        raise ValueError("%s: scores %s with strides %s: need Q, N >= 1, unit column stride and row stride >= N"
                         % (name, tuple(scores.shape), tuple(scores.stride())))
    if base < 0 or base + N > 2 ** 31 - 1:
        raise ValueError("%s: row ids %d .. %d leave int32" % (name, base, base + N - 1))
    if not scores.is_cuda:
        raise _lib.S2IError("%s runs on the MI355X kernel: there is no CPU fallback (scores on %s)" % (name, scores.device))
    return Q, N, scores.device


def _block_vector(name, what, t, dtype, n, device):
    if (not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous()
            or t.device != device):
        raise ValueError("%s: %s must be a contiguous %s vector of %d entries on %s"
                         % (name, what, str(dtype).replace("torch.", ""), n, device))


def _own_base(name, own_base):
    own_base = -1 if own_base is None else int(own_base)
    if own_base < -1 or own_base > 2 ** 31 - 1:
        raise ValueError("%s: own_base must be None / -1 or a row id, got %d" % (name, own_base))
    return own_base


def polykernel_rows(scores, inv_d, sums, base=0, own_base=None):
    """sums[q] += sum_j (scores[q][j] * inv_d + 1)^3 over one [Q, N] block of scores (fp32, unit column stride, any row
    stride >= N; column j is row base + j of the other set), evaluated and added in fp64 in a fixed order
    (s2i_polykernel_rows).  own_base: query q is row own_base + q of the other set and that column is left out (the
    off-diagonal sum of a set against itself); None leaves nothing out.  sums: fp64 [Q] on the scores' device,
    accumulated in place (the caller zeroes it).  No autograd."""
    base, inv_d = int(base), float(inv_d)
    own_base = _own_base("polykernel_rows", own_base)
    if not math.isfinite(inv_d):
        raise ValueError("polykernel_rows: inv_d must be finite, got %r" % (inv_d,))
    Q, N, dev = _block("polykernel_rows", scores, base)
    _block_vector("polykernel_rows", "sums", sums, torch.float64, Q, dev)
    check(_lib_ready().s2i_polykernel_rows(ptr(scores.detach()), Q, N, scores.stride(0), base, own_base, inv_d, ptr(sums),
                                           stream()), "s2i_polykernel_rows")
    return sums


def sqdist_rows(scores, q_norm2, row_norm2, base=0, own_base=None):
    """Rewrites one [Q, N] block of scores IN PLACE to minus the squared distance, -max(0, (q_norm2[q] + row_norm2[base + j])
    - 2 scores[q][j]) in fp32 as written (s2i_sqdist_rows); a NaN stays one; the own row (base + j == own_base + q) becomes
    -inf, so topk_rows on the result gives the nearest OTHER rows.  q_norm2: fp32 [Q]; row_norm2: fp32 over the whole
    other set, indexed by global row.  Returns scores.  No autograd."""
    base = int(base)
    Q, N, dev = _block("sqdist_rows", scores, base)
    own_base = _own_base("sqdist_rows", own_base)
    _block_vector("sqdist_rows", "q_norm2", q_norm2, torch.float32, Q, dev)
    if not torch.is_tensor(row_norm2) or row_norm2.dim() != 1:
        raise ValueError("sqdist_rows: row_norm2 must be an fp32 vector over the other set's rows")
    n_rows = row_norm2.shape[0]
    _block_vector("sqdist_rows", "row_norm2", row_norm2, torch.float32, n_rows, dev)
    if base + N > n_rows:
        raise ValueError("sqdist_rows: rows %d .. %d pass the %d row norms" % (base, base + N - 1, n_rows))
    check(_lib_ready().s2i_sqdist_rows(ptr(scores.detach()), Q, N, scores.stride(0), base, own_base, ptr(q_norm2),
                                       ptr(row_norm2), n_rows, stream()), "s2i_sqdist_rows")
    return scores


def ball_rows(nd, row_bound, base=0, count=None, best=None):
    """One [Q, N] block of negated squared distances (sqdist_rows) folded into count[q] += #{j : nd[q][j] >=
    row_bound[base + j]} (int32 [Q]) and best[q] = max(best[q], max_j nd[q][j]) (fp32 [Q]); either may be None
    (s2i_ball_rows).  row_bound: fp32 over the whole other set, -radius^2 of every row's ball.  NaN entries and NaN bounds
    count nothing.  The caller zeroes count and fills best with -inf.  Only comparisons: exact.  No autograd."""
    base = int(base)
    Q, N, dev = _block("ball_rows", nd, base)
    if count is None and best is None:
        raise ValueError("ball_rows: give count, best or both")
    if count is not None:
        _block_vector("ball_rows", "count", count, torch.int32, Q, dev)
    if best is not None:
        _block_vector("ball_rows", "best", best, torch.float32, Q, dev)
    if not torch.is_tensor(row_bound) or row_bound.dim() != 1:
        raise ValueError("ball_rows: row_bound must be an fp32 vector over the other set's rows")
    n_rows = row_bound.shape[0]
    _block_vector("ball_rows", "row_bound", row_bound, torch.float32, n_rows, dev)
    if base + N > n_rows:
        raise ValueError("ball_rows: rows %d .. %d pass the %d row bounds" % (base, base + N - 1, n_rows))
    check(_lib_ready().s2i_ball_rows(ptr(nd.detach()), Q, N, nd.stride(0), base, ptr(row_bound), n_rows, ptr(count),
                                     ptr(best), stream()), "s2i_ball_rows")
    return count, best
