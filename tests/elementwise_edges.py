"""Launches of the loss, head, layout and optimiser kernels off the shapes the train step records.

tests/step_elementwise_launches.json records these entry points at one operating point: B = 24 / 72 (48 / 144), square
power-of-two maps, channel counts that are multiples of 64.  The kernels choose thread layouts (red_geom), segment counts
(border_segments, spatial_segments), row chunks (colreduce) and grid-stride trips (grid_for) from exactly those numbers.
This module restates that host geometry in plain Python, derives from it which code paths a record runs (reach), and holds
the table EDGES of the smallest shapes that run the paths the census does not.  It imports neither torch nor the library.

A record is a census record (`fn` plus the scalar arguments of elementwise_replay.ARGS and the optional pointers as
booleans) with one extra key, `why`.  tests/test_elementwise_edges_cpu.py asserts that every tag of TAGS is reached by
the table and by no census record, and checks the mirrors against the library where it exports the number;
tests/test_elementwise_edges_gpu.py replays every record against fp64.

Tags that reach() derives but that the census already reaches are listed in CENSUS_REACHED with the record that does; they
are not part of TAGS (the table's records reach them again all the same)."""
import struct

DT_F32, DT_BF16 = 0, 1          # _lib.DT_F32, _lib.DT_BF16
ACT_LRELU, ACT_TANH = 2, 3      # _lib.ACT_LRELU, _lib.ACT_TANH
F32, BF16 = DT_F32, DT_BF16
BLOCK = 256                     # every kernel here launches 256 threads


# ---- host geometry, restated -------------------------------------------------------------------------------------------
def red_geom(C):
    """csrc/s2i_elementwise.h red_geom(): Q = C / 4 channel quads, cpb = the power of two >= Q (at most 256) threads
    across quads, rpb = 256 / cpb row lanes, gy = ceil(Q / cpb) blocks across quads -> (Q, cpb, rpb, gy)."""
    Q = C // 4
    cpb = 1
    while cpb < Q and cpb < 256:
        cpb <<= 1
    return Q, cpb, 256 // cpb, (Q + cpb - 1) // cpb


def border_segments(H):
    """csrc/s2i_cvec.hip border_segments(): S = H / 4 clamped to [1, 32]."""
    return min(32, max(1, H // 4))


def spatial_segments(HW):
    """csrc/s2i_layout.hip spatial_segments(): S = HW / 64 clamped to [1, 64]."""
    return min(64, max(1, HW // 64))


def grid_for(total, block=BLOCK, cap=2048 * 4):
    """csrc/s2i_elementwise.h grid_for(): ceil(total / block) blocks clamped to [1, cap]."""
    return min(cap, max(1, (total + block - 1) // block))


def segments(n, S):
    """The [r0, r1) of each of S segments of n rows: `chunk = (n + S - 1) / S; r0 = s * chunk; r1 = min(n, r0 + chunk)` of
    border_sums_stage1 (band, y0, y1), spatial_sum_stage1 (chunk, r0, r1) and colreduce_kernel (csrc/s2i_bn.hip; one
    group: chunk, r0, r1).  An empty segment has r1 <= r0."""
    chunk = (n + S - 1) // S
    return chunk, [(s * chunk, min(n, s * chunk + chunk)) for s in range(S)]


def border_sums_workspace_bytes(B, H, W, C):
    """csrc/s2i_cvec.hip s2i_border_sums_workspace_bytes(): B * S * 9 * C floats."""
    return B * border_segments(H) * 9 * C * 4


def spatial_sum_workspace_bytes(B, HW, C):
    """csrc/s2i_layout.hip s2i_spatial_sum_workspace_bytes(): B * S * C floats."""
    return B * spatial_segments(HW) * C * 4


def trips(total):
    """Grid-stride trips of the busiest thread of a grid_for(total) launch."""
    return -(-total // (grid_for(total) * BLOCK))


# ---- what a record reaches ---------------------------------------------------------------------------------------------
def _geom_tags(fam, C):
    Q, cpb, rpb, gy = red_geom(C)
    out = set()
    if Q != cpb * gy:
        out.add(fam + ":quad lanes idle (Q is no power of two)")
    if gy > 1:
        out.add(fam + ":gy > 1")
    return out


def _segment_tags(fam, n, S):
    chunk, segs = segments(n, S)
    live = [(a, b) for a, b in segs if b > a]
    out = set()
    if len(live) < S:
        out.add(fam + ":empty segment")
    if live[-1][1] - live[-1][0] < chunk:
        out.add(fam + ":short last segment")
    return out


def _stride_tags(fam, total):
    """Elementwise launches over `total` items: a partly filled last block, one block that is not full, a second trip."""
    out = set()
    if total < BLOCK:
        out.add(fam + ":less than one block")
    elif total % BLOCK:
        out.add(fam + ":tail block")
    if trips(total) > 1:
        out.add(fam + ":second grid-stride trip")
    return out


def _one_block_tags(fam, total):
    """One-block reductions whose threads stride by 256 over `total` items."""
    out = set()
    if total < BLOCK:
        out.add(fam + ":fewer items than threads")
    if total > BLOCK:
        out.add(fam + ":more than one stride")
    return out


def reach(rec):
    """The set of tags (code paths and operand forms off the census) the launch `rec` runs, derived from the mirrors."""
    fn, t = rec["fn"], set()
    if fn == "s2i_tap_sums_dt":
        H, W, C = rec["H"], rec["W"], rec["C"]
        S = border_segments(H)
        rpb = red_geom(C)[2]
        t |= _geom_tags("tap_sums", C) | _segment_tags("tap_sums", H, S)
        if S == 1:
            t.add("tap_sums:S = 1")
        if H < W:
            t.add("tap_sums:H < W")
        if H > W:
            t.add("tap_sums:H > W")
        if W < rpb:
            t.add("tap_sums:W < rpb")
        if W > rpb and W % rpb:
            t.add("tap_sums:W > rpb with a tail")
    elif fn == "s2i_spatial_sum_dt":
        HW, C = rec["HW"], rec["C"]
        S = spatial_segments(HW)
        t |= _geom_tags("spatial_sum", C) | _segment_tags("spatial_sum", HW, S)
        t.add("spatial_sum:S = %d" % S)
        if rec["ld"] > C:
            t.add("spatial_sum:ld > C")
        if segments(HW, S)[0] < red_geom(C)[2]:
            t.add("spatial_sum:fewer rows than row lanes")
    elif fn == "s2i_colstats":
        M, C, nparts = rec["M"], rec["C"], rec["nparts"]
        t |= _geom_tags("colstats", C) | _segment_tags("colstats", M, nparts)
        if nparts > 1:
            t.add("colstats:nparts > 1")
        if rec["ldy"] > C:
            t.add("colstats:ldy > C")
    elif fn == "s2i_cvec_bias_table":
        Cc, N = rec["Cc"], rec["N"]
        if Cc % 4:
            t.add("cvec_table:Cc %% 4 = %d" % (Cc % 4))
        if Cc < 4:
            t.add("cvec_table:Cc < 4")
        if N < rec["Op"]:
            t.add("cvec_table:N < Op")
        if N > BLOCK:
            t.add("cvec_table:N > 256")
        if rec["B"] == 1:
            t.add("cvec_table:B = 1")
    elif fn == "s2i_cvec_grads":
        Cc, N = rec["Cc"], rec["N"]
        if rec["dc"]:
            if Cc % 64:
                t.add("cvec_grads:last 64-channel block partly live")
            if N < 16:
                t.add("cvec_grads:idle lanes (N < 16)")
            if N % 16:
                t.add("cvec_grads:N % 16 != 0")
            if not rec["dw"]:
                t.add("cvec_grads:dc alone")
        if rec["dw"]:
            if rec["O"] < N:
                t.add("cvec_grads:O < N")
            if rec["I_total"] > Cc:
                t.add("cvec_grads:I_total > Cc")
            t.add("cvec_grads:dw accumulated" if rec["accumulate"] else "cvec_grads:dw assigned")
            if not rec["dc"]:
                t.add("cvec_grads:dw alone")
    elif fn == "s2i_logit_forward":
        n = 16 * rec["C"]
        if n < BLOCK:
            t.add("logit_forward:n < 256")
        if n % BLOCK:
            t.add("logit_forward:n % 256 != 0")
        if not rec["bias"]:
            t.add("logit_forward:NULL bias")
    elif fn == "s2i_logit_backward":
        B, n = rec["B"], 16 * rec["C"]
        if B % 8:
            t.add("logit_backward:B % 8 != 0")
        if B > BLOCK:
            t.add("logit_backward:B > 256")
        if n % BLOCK:
            t.add("logit_backward:dead threads")
            if B > BLOCK:
                t.add("logit_backward:dead threads under the second barrier pair")
        if rec["dx"] and rec["acc_dx"]:
            t.add("logit_backward:acc_dx")
        if not rec["dx"]:
            t.add("logit_backward:NULL dx")
        if rec["dx"] and not rec["dw"] and not rec["dbias"]:
            t.add("logit_backward:dx alone")
        if rec["dw"] and not rec["acc_dw"]:
            t.add("logit_backward:dw assigned")
    elif fn in ("s2i_bce_forward", "s2i_bce_backward"):
        fam = fn[4:]
        B, tg = rec["B"], rec["target"]
        t |= _one_block_tags(fam, B) if fn == "s2i_bce_forward" else _stride_tags(fam, B)
        if B < 4:
            t.add(fam + ":B < 4")
        if 0 < tg < 1:
            t.add(fam + ":0 < target < 1")
        if tg == 0:
            t.add(fam + ":target = 0")
        if rec["weight"] != 1:
            t.add(fam + ":weight != 1")
        if rec.get("accumulate"):
            t.add(fam + ":accumulate")
    elif fn in ("s2i_bce_multi_forward", "s2i_bce_multi_backward"):
        fam = fn[4:]
        G, H, B = rec["G"], rec["H"], rec["B"]
        t |= _one_block_tags(fam, G * H * B) if fn.endswith("forward") else _stride_tags(fam, G * H * B)
        if H in (1, 4):
            t.add(fam + ":H = %d" % H)
        if G == 1:
            t.add(fam + ":G = 1")
    elif fn == "s2i_cal_loss":
        t |= _one_block_tags("cal_loss", rec["B"] ** 2)
        if rec["B"] ** 2 > BLOCK and rec["B"] ** 2 % BLOCK:
            t.add("cal_loss:more than one stride with a tail")
        if not rec["dscores"]:
            t.add("cal_loss:NULL dS")
        if rec["accumulate"]:
            t.add("cal_loss:accumulate")
    elif fn in ("s2i_kl_forward", "s2i_kl_backward"):
        fam = fn[4:]
        n = rec["B"] * rec["E"]
        t |= _one_block_tags(fam, n) if fn.endswith("forward") else _stride_tags(fam, n)
        if rec["ldmu"] != rec["ldlv"]:
            t.add(fam + ":ldmu != ldlv")
        if rec["ldmu"] == rec["E"]:
            t.add(fam + ":ldmu = E")
    elif fn in ("s2i_reparam_forward", "s2i_reparam_backward"):
        fam = fn[4:]
        t |= _stride_tags(fam, rec["B"] * rec["E"])
        if fn.endswith("backward"):
            if not rec["dc"]:
                t.add(fam + ":NULL dc")
            if rec["dmu"] and rec["dlogvar"]:
                t.add(fam + ":direct gradients present")
    elif fn in ("s2i_glu_forward", "s2i_glu_backward"):
        t |= _stride_tags(fn[4:], rec["M"] * (rec["C"] // 2))
    elif fn == "s2i_act_backward_dt":
        fam = "act_backward"
        t |= _stride_tags(fam, rec["M"] * (rec["C"] // 4))
        if rec["lddout"] > rec["C"]:
            t.add(fam + ":lddout > C")
        if rec["dtype"] == DT_BF16 and rec["act"] == ACT_TANH:
            t.add(fam + ":tanh in bf16")
    elif fn == "s2i_nchw_to_nhwc_dt":
        fam = "nchw_to_nhwc"
        B, C, H, W, Cp = (rec[k] for k in ("B", "C", "H", "W", "Cp"))
        fast = rec["dtype"] == DT_F32 and C == 3 and Cp == 4          # s2i_nchw_to_nhwc(): nchw3_to_nhwc4_kernel
        if fast and H * W == 1:
            t.add(fam + ":fast path at one pixel")
        if C == 3 and not fast:
            t.add(fam + ":C = 3 off the fast path")
        if Cp > C and not fast:
            t.add(fam + ":generic kernel pads")
        if H != W:
            t.add(fam + ":H != W")
        t |= _stride_tags(fam, B * H * W * (1 if fast else Cp)) - {fam + ":second grid-stride trip"}
    elif fn == "s2i_nhwc_to_nchw_dt":
        fam = "nhwc_to_nchw"
        if rec["lds"] - rec["C"] > 1:
            t.add(fam + ":more than one pad column")
        if rec["lds"] > rec["C"] and rec["dtype"] == DT_BF16:
            t.add(fam + ":lds > C in bf16")
        if rec["H"] != rec["W"]:
            t.add(fam + ":H != W")
    elif fn in ("s2i_axpby", "s2i_scale_dev", "s2i_ema_update"):
        fam = fn[4:]
        t |= _stride_tags(fam, rec["n"])
        if fn == "s2i_axpby" and rec["b"] == 0:
            t.add("axpby:b = 0")
    elif fn == "s2i_cast":
        t |= _stride_tags("cast", rec["n"] // 4)
    return t


# ---- the table -------------------------------------------------------------------------------------------------------
def _f32(v):
    """A float argument as the kernel receives it, which is how the census records one."""
    return struct.unpack("f", struct.pack("f", v))[0]


def _tap(B, H, W, C, dt, why):
    return dict(fn="s2i_tap_sums_dt", dtype=dt, B=B, H=H, W=W, C=C, dy=True, tapsum=True, why=why)


def _spatial(B, HW, C, ld, dt, why):
    return dict(fn="s2i_spatial_sum_dt", dtype=dt, B=B, HW=HW, C=C, ld=ld, src=True, dst=True, why=why)


def _colstats(M, C, ldy, nparts, why):
    return dict(fn="s2i_colstats", M=M, C=C, ldy=ldy, nparts=nparts, y=True, part=True, why=why)


def _table(B, Cc, Ip, Op, N, why):
    return dict(fn="s2i_cvec_bias_table", B=B, Cc=Cc, Ip=Ip, Op=Op, N=N, cvec=True, packed=True, table=True, why=why)


def _grads(B, Cc, Ip, Op, N, O, It, acc, dc, dw, why):
    return dict(fn="s2i_cvec_grads", B=B, Cc=Cc, Ip=Ip, Op=Op, N=N, O=O, I_total=It, accumulate=acc, dc=dc, dw=dw, cvec=True,
                packed=True, tapsum=True, why=why)


def _lfwd(B, C, bias, why):
    return dict(fn="s2i_logit_forward", B=B, C=C, bias=bias, x=True, w=True, prob=True, why=why)


def _lbwd(B, C, dx, acc_dx, dw, dbias, acc_dw, why):
    return dict(fn="s2i_logit_backward", B=B, C=C, dx=dx, acc_dx=acc_dx, dw=dw, dbias=dbias, acc_dw=acc_dw, x=True, w=True,
                prob=True, dprob=True, why=why)


def _bce(B, target, weight, acc, why):
    return [dict(fn="s2i_bce_forward", B=B, target=_f32(target), weight=_f32(weight), accumulate=acc, prob=True, loss=True,
                 why=why),
            dict(fn="s2i_bce_backward", B=B, target=_f32(target), weight=_f32(weight), prob=True, gout=True, dprob=True,
                 why=why)]


def _bce_multi(G, H, B, why):
    return [dict(fn="s2i_bce_multi_forward", G=G, H=H, B=B, probs=True, target=True, weight=True, loss=True, why=why),
            dict(fn="s2i_bce_multi_backward", G=G, H=H, B=B, probs=True, target=True, weight=True, gout=True, dprobs=True,
                 why=why)]


def _cal(B, D, acc, dS, why):
    return dict(fn="s2i_cal_loss", B=B, D=D, accumulate=acc, dscores=dS, scores=True, labels=True, loss=True, why=why)


def _kl(B, E, ldmu, ldlv, why):
    return [dict(fn="s2i_kl_forward", B=B, E=E, ldmu=ldmu, ldlv=ldlv, mu=True, logvar=True, kl=True, why=why),
            dict(fn="s2i_kl_backward", B=B, E=E, ldmu=ldmu, ldlv=ldlv, mu=True, logvar=True, gout=True, dmu=True,
                 dlogvar=True, why=why)]


def _reparam(B, E, dc, direct, why):
    return [dict(fn="s2i_reparam_forward", B=B, E=E, h=True, eps=True, c=True, why=why),
            dict(fn="s2i_reparam_backward", B=B, E=E, h=True, eps=True, dc=dc, dmu=direct, dlogvar=direct, dh=True,
                 why=why)]


def _glu(M, C, why):
    return [dict(fn="s2i_glu_forward", M=M, C=C, x=True, out=True, why=why),
            dict(fn="s2i_glu_backward", M=M, C=C, x=True, dout=True, dx=True, why=why)]


def _act(dt, M, C, ldd, act, why):
    return dict(fn="s2i_act_backward_dt", dtype=dt, M=M, C=C, lddout=ldd, act=act, out=True, dout=True, dy=True, why=why)


def _to_nhwc(dt, B, C, H, W, Cp, why):
    return dict(fn="s2i_nchw_to_nhwc_dt", dtype=dt, B=B, C=C, H=H, W=W, Cp=Cp, src=True, dst=True, why=why)


def _to_nchw(dt, B, C, H, W, lds, why):
    return dict(fn="s2i_nhwc_to_nchw_dt", dtype=dt, B=B, C=C, H=H, W=W, lds=lds, src=True, dst=True, why=why)


def _flat(n):
    why = {1: "one element", 255: "one block, one thread idle", 257: "a tail block of one element",
           2097153: "one element past 8192 blocks of 256: the second grid-stride trip"}[n]
    return [dict(fn="s2i_axpby", n=n, a=_f32(0.5), b=0.0, x=True, y=True, why=why + "; b = 0 over a NaN-filled y"),
            dict(fn="s2i_axpby", n=n, a=_f32(-1.5), b=_f32(0.25), x=True, y=True, why=why + "; b != 0"),
            dict(fn="s2i_scale_dev", n=n, a=True, x=True, y=True, why=why),
            dict(fn="s2i_ema_update", n=n, decay=_f32(0.75), avg=True, p=True, why=why)]


def _cast(n, why):
    return [dict(fn="s2i_cast", n=n, src_dtype=s, dst_dtype=d, src=True, dst=True, why=why)
            for s, d in ((DT_F32, DT_BF16), (DT_BF16, DT_F32))]


def _flatten(items):
    out = []
    for it in items:
        out.extend(it if isinstance(it, list) else [it])
    return out


T, F = True, False
EDGES = _flatten([
    _tap(3, 2, 2, 4, F32, "S = 1 with both rows border rows; one quad, 254 row lanes idle"),
    _tap(2, 3, 7, 12, F32, "S = 1, H < W, Q = 3 under cpb = 4"),
    _tap(2, 9, 5, 132, BF16, "S = 2 with a short last band (5 + 4 rows), H > W, Q = 33 under cpb = 64, W = 5 over rpb = 4"),
    _tap(1, 34, 6, 64, F32, "S = 8, band 5: band 6 has 4 rows and band 7 none, and must still write zeros"),
    _tap(1, 130, 3, 8, BF16, "S = 32, band 5: bands 26..31 are empty"),
    _tap(1, 4, 4, 1028, F32, "Q = 257: two blocks across quads, the second with one live quad lane"),
    _tap(2, 7, 34, 36, BF16, "H < W with W = 34 = 2 * rpb + 2: a tail of the column loop"),
    _spatial(2, 1, 4, 4, F32, "one row, one quad"),
    _spatial(3, 63, 12, 20, BF16, "S = 1 just below the first split, ld > C, Q = 3 under cpb = 4"),
    _spatial(2, 130, 132, 132, F32, "S = 2 in whole chunks of 65 rows, Q = 33 under cpb = 64"),
    _spatial(2, 200, 64, 640, BF16, "S = 3, chunk 67: the last segment has 66 rows"),
    _spatial(1, 4097, 8, 8, F32, "S = 64, chunk 65: the last segment has 2 rows"),
    _spatial(1, 70, 1028, 1028, F32, "Q = 257: two blocks across quads"),
    _colstats(1037, 48, 64, 16, "chunk 65: the last chunk has 62 rows; ldy > C; Q = 12 under cpb = 16"),
    _colstats(5, 4, 4, 8, "more parts than rows: parts 5..7 are empty and must be written as zeros"),
    _colstats(517, 132, 132, 3, "chunk 173: the last chunk has 171 rows; Q = 33 under cpb = 64"),
    _colstats(33, 1028, 1028, 2, "Q = 257: two blocks across quads; chunk 17 + 16"),
    _table(1, 1, 8, 8, 3, "one channel: only the scalar tail of the channel loop; N < Op; B = 1"),
    _table(5, 3, 8, 12, 5, "Cc = 3: the scalar tail alone, three times"),
    _table(2, 5, 16, 264, 260, "Cc = 5: one unrolled trip and a tail of one; N = 260: the second trip of the n loop"),
    _table(3, 130, 160, 64, 64, "Cc = 130: a tail of two after 32 unrolled trips"),
    _grads(1, 70, 96, 8, 4, 3, 80, 0, T, T, "Cc = 70: six live channels in the second block; N = 4: three lanes idle; O < N"),
    _grads(5, 5, 8, 24, 20, 20, 5, 1, T, T, "N = 20: lane 0 makes two trips, lanes 1..3 one; I_total = Cc"),
    _grads(2, 130, 160, 36, 36, 36, 140, 0, T, F, "dc alone, three channel blocks, N = 36"),
    _grads(3, 64, 64, 64, 64, 64, 64, 1, F, T, "dw alone, accumulated"),
    _lfwd(1, 4, T, "n = 64: three quarters of the block idle"),
    _lfwd(23, 24, F, "n = 384 = 256 + 128; no bias"),
    _lfwd(5, 40, T, "n = 640 = 2 * 256 + 128"),
    _lbwd(1, 4, T, 0, T, T, 0, "one image, one quarter-filled block, everything assigned"),
    _lbwd(7, 24, T, 1, T, T, 1, "B = 7: a tail of 7 in the 8-row walk; dx accumulated; the second block half dead"),
    _lbwd(23, 512, T, 0, T, T, 1, "the ragged production batch at the production width: 2 * 8 + 7 rows"),
    _lbwd(257, 24, T, 0, T, T, 0, "B = 257: a second trip of one image, dead threads under its barrier pair"),
    _lbwd(300, 40, F, 0, T, T, 1, "B = 300 with dx NULL: dw and dbias alone over two trips"),
    _lbwd(300, 4, T, 1, F, F, 0, "B = 300 with dx alone, accumulated"),
    _bce(1, 1, 1, 0, "one probability"),
    _bce(3, 0, 0.5, 1, "B < 4, target 0, weight 0.5, accumulated"),
    _bce(23, 1, 1, 1, "the ragged production batch, accumulated"),
    _bce(257, 0.3, 2, 0, "one item past a stride; a target strictly between 0 and 1"),
    _bce(600, 0, 1, 1, "three strides, the last of 88"),
    _bce_multi(1, 1, 1, "one term of one probability"),
    _bce_multi(1, 4, 5, "four heads, one stacked batch"),
    _bce_multi(3, 2, 23, "the ragged production batch"),
    _bce_multi(2, 3, 130, "780 items: four strides, the last of 12"),
    _cal(2, 1, 0, T, "two samples of one class: one same-label pair each way"),
    _cal(5, 8192, 1, T, "25 items, accumulated"),
    _cal(17, 64, 0, T, "289 items: one stride and a tail of 33"),
    _cal(23, 8192, 1, F, "the ragged production batch, no dS, accumulated"),
    _cal(40, 16, 0, T, "1600 items: seven strides, the last of 64"),
    _kl(1, 1, 1, 1, "one element"),
    _kl(3, 5, 5, 5, "15 elements in contiguous rows"),
    _kl(23, 128, 256, 256, "the ragged production batch"),
    _kl(7, 100, 228, 100, "mu out of a wider row, logvar contiguous"),
    _reparam(1, 1, T, F, "one element"),
    _reparam(5, 100, F, T, "dc NULL: the direct gradients alone"),
    _reparam(23, 128, T, T, "the ragged production batch with both direct gradients"),
    _glu(1, 2, "one element"),
    _glu(5, 6, "15 elements"),
    _glu(23, 512, "the ragged production batch"),
    _glu(4099, 1026, "4099 * 513 = 2102787 items: 5635 past 8192 blocks of 256"),
] + [_act(dt, M, C, ldd, act, why) for act in (ACT_LRELU, ACT_TANH) for dt in (F32, BF16)
     for M, C, ldd, why in ((1, 4, 4, "one quad"), (23, 12, 20, "69 quads, lddout > C"))] + [
    _act(F32, 2097155, 4, 4, ACT_TANH, "three quads past 8192 blocks of 256 (tanh, as the image head)"),
    _act(BF16, 2097155, 4, 4, ACT_LRELU, "three quads past 8192 blocks of 256"),
    _to_nhwc(F32, 1, 3, 1, 1, 4, "the 3 -> 4 fast path at a single pixel"),
    _to_nhwc(F32, 2, 3, 5, 7, 8, "C = 3 with Cp = 8: the generic kernel writes five zero channels"),
    _to_nhwc(BF16, 2, 3, 5, 7, 4, "C = 3, Cp = 4 in bf16: the generic kernel, one zero channel"),
    _to_nhwc(F32, 3, 5, 3, 2, 8, "H > W, three zero channels"),
    _to_nhwc(BF16, 2, 36, 3, 5, 40, "H < W, four zero channels in bf16"),
    _to_nhwc(F32, 1, 1, 1, 1, 1, "one element"),
    _to_nchw(F32, 2, 3, 5, 7, 4, "the image form off the square"),
    _to_nchw(BF16, 2, 5, 3, 2, 8, "three unread columns in bf16"),
    _to_nchw(F32, 1, 7, 1, 9, 12, "one row of pixels, five unread columns"),
    _to_nchw(BF16, 3, 36, 2, 2, 36, "lds = C in bf16"),
] + [_flat(n) for n in (1, 255, 257, 2097153)] + [_cast(4, "one thread"), _cast(1028, "257 quads: a tail block of one")])
del T, F

# derived by reach() but run by the step itself, with the census record that does (fp32_b24 unless stated): not claimed
CENSUS_REACHED = {
    "spatial_sum:S = 1": "HW = 16",
    "spatial_sum:ld > C": "ld = 640 over C = 128",
    "cvec_grads:I_total > Cc": "I_total = 160 over Cc = 128",
    "cvec_grads:dw accumulated": "every cvec_grads launch of the step accumulates",
    "logit_backward:dx alone": "the generator's pass through the discriminator heads, B = 24",
    "cal_loss:more than one stride": "B = 24: 576 items",
    "cal_loss:more than one stride with a tail": "B = 24: 576 = 2 * 256 + 64",
    "kl_forward:more than one stride": "B E = 3072",
    "act_backward:second grid-stride trip": "M = 1179648, C = 64: 18874368 quads",
    "ema_update:second grid-stride trip": "n = 21239696",
    "ema_update:tail block": "n = 21239696 = 82967 * 256 + 144",
    "bce_multi_backward:less than one block": "G H B = 144",
    "bce_multi_backward:tail block": "bf16_b48: G H B = 288 = 256 + 32",
    "bce_multi_forward:fewer items than threads": "G H B = 144",
    "bce_multi_forward:more than one stride": "bf16_b48: G H B = 288",
    "bce_forward:fewer items than threads": "B = 24",
    "bce_backward:less than one block": "B = 24",
}


def all_reached(records):
    out = set()
    for r in records:
        out |= reach(r)
    return out


# the code paths and operand forms the table claims: each reached by a record of EDGES and by no census record
TAGS = (
    "act_backward:lddout > C", "act_backward:less than one block", "act_backward:tail block",
    "act_backward:tanh in bf16", "axpby:b = 0", "axpby:less than one block", "axpby:second grid-stride trip",
    "axpby:tail block", "bce_backward:0 < target < 1", "bce_backward:B < 4", "bce_backward:tail block",
    "bce_backward:target = 0", "bce_backward:weight != 1", "bce_forward:0 < target < 1", "bce_forward:B < 4",
    "bce_forward:accumulate", "bce_forward:more than one stride", "bce_forward:target = 0", "bce_forward:weight != 1",
    "bce_multi_backward:G = 1", "bce_multi_backward:H = 1", "bce_multi_backward:H = 4", "bce_multi_forward:G = 1",
    "bce_multi_forward:H = 1", "bce_multi_forward:H = 4", "cal_loss:NULL dS", "cal_loss:accumulate",
    "cal_loss:fewer items than threads", "cast:less than one block", "cast:tail block", "colstats:empty segment",
    "colstats:gy > 1", "colstats:ldy > C", "colstats:nparts > 1", "colstats:quad lanes idle (Q is no power of two)",
    "colstats:short last segment", "cvec_grads:N % 16 != 0", "cvec_grads:O < N", "cvec_grads:dc alone",
    "cvec_grads:dw alone", "cvec_grads:dw assigned", "cvec_grads:idle lanes (N < 16)",
    "cvec_grads:last 64-channel block partly live", "cvec_table:B = 1", "cvec_table:Cc % 4 = 1",
    "cvec_table:Cc % 4 = 2", "cvec_table:Cc % 4 = 3", "cvec_table:Cc < 4", "cvec_table:N < Op", "cvec_table:N > 256",
    "ema_update:less than one block", "glu_backward:less than one block", "glu_backward:second grid-stride trip",
    "glu_backward:tail block", "glu_forward:less than one block", "glu_forward:second grid-stride trip",
    "glu_forward:tail block", "kl_backward:ldmu != ldlv", "kl_backward:ldmu = E", "kl_backward:less than one block",
    "kl_backward:tail block", "kl_forward:fewer items than threads", "kl_forward:ldmu != ldlv", "kl_forward:ldmu = E",
    "logit_backward:B % 8 != 0", "logit_backward:B > 256", "logit_backward:NULL dx", "logit_backward:acc_dx",
    "logit_backward:dead threads", "logit_backward:dead threads under the second barrier pair",
    "logit_backward:dw assigned", "logit_forward:NULL bias", "logit_forward:n % 256 != 0", "logit_forward:n < 256",
    "nchw_to_nhwc:C = 3 off the fast path", "nchw_to_nhwc:H != W", "nchw_to_nhwc:fast path at one pixel",
    "nchw_to_nhwc:generic kernel pads", "nchw_to_nhwc:less than one block", "nchw_to_nhwc:tail block",
    "nhwc_to_nchw:H != W", "nhwc_to_nchw:lds > C in bf16", "nhwc_to_nchw:more than one pad column",
    "reparam_backward:NULL dc", "reparam_backward:direct gradients present", "reparam_backward:less than one block",
    "reparam_backward:tail block", "reparam_forward:less than one block", "reparam_forward:tail block",
    "scale_dev:less than one block", "scale_dev:second grid-stride trip", "scale_dev:tail block", "spatial_sum:S = 2",
    "spatial_sum:S = 3", "spatial_sum:S = 64", "spatial_sum:fewer rows than row lanes", "spatial_sum:gy > 1",
    "spatial_sum:quad lanes idle (Q is no power of two)", "spatial_sum:short last segment", "tap_sums:H < W",
    "tap_sums:H > W", "tap_sums:S = 1", "tap_sums:W < rpb", "tap_sums:W > rpb with a tail", "tap_sums:empty segment",
    "tap_sums:gy > 1", "tap_sums:quad lanes idle (Q is no power of two)", "tap_sums:short last segment",
)


def record_id(i, rec):
    keys = [k for k in ("dtype", "B", "G", "H", "W", "HW", "M", "C", "Cc", "N", "E", "D", "n", "act") if k in rec]
    return "%03d-%s-%s" % (i, rec["fn"][4:], "-".join("%s%s" % (k, rec[k]) for k in keys))
