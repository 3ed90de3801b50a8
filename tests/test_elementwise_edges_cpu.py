"""What tests/elementwise_edges.py claims, derived on the host, and the fp64 reference off the shapes it was written at.

  * schema: every record of the table is a census record (the scalar arguments of elementwise_replay.ARGS) plus `why`.
  * reach: every tag of E.TAGS is reached by a record of the table and by no record of either mode of
    tests/step_elementwise_launches.json; reach() derives nothing that is neither claimed nor listed in E.CENSUS_REACHED.
    The issue that asked for the table also named a few paths the census does reach (the second grid-stride trip of fp32
    act_backward and of ema_update, `ld > C` of spatial_sum, `dx` alone of logit_backward, more than one stride of
    cal_loss and kl_forward): those are in E.CENSUS_REACHED, with the census record that reaches them, and not in E.TAGS.
  * mirrors: border_segments / spatial_segments through the library's workspace queries (no device needed), the
    segment arithmetic on the examples the table was built around.
  * reference: elementwise_ref.py was checked at the step's shapes (tests/test_elementwise_ref.py); here tap_sums and the
    broadcast-channel functions run at H != W and Cc % 4 != 0 against F.conv2d and its autograd, the row sums against
    plain loops over the segments of the table's records (empty ones included), cal_loss on its two inactive branches
    and logit_backward / bce at B = 300 and at probabilities of exactly 0 and 1 against torch autograd."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import elementwise_edges as E  # noqa: E402
import elementwise_ref as R  # noqa: E402
import elementwise_replay as ER  # noqa: E402
import launch_harness as LH  # noqa: E402
from speech_to_image_translation_without_text_amd import _lib  # noqa: E402

CENSUS_FILE = os.path.join(HERE, "step_elementwise_launches.json")
IDS = [E.record_id(i, r) for i, r in enumerate(E.EDGES)]


def _census():
    census = LH.load_census(CENSUS_FILE)
    assert set(census) == set(LH.STEP_MODES)
    return census


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- schema and reach ------------------------------------------------------------------------------------------------
def test_constants_are_the_library_s():
    assert (E.DT_F32, E.DT_BF16, E.ACT_LRELU, E.ACT_TANH) == (_lib.DT_F32, _lib.DT_BF16, _lib.ACT_LRELU, _lib.ACT_TANH)


def test_records_use_the_census_schema():
    scalars = {}
    for recs in _census().values():
        for r in recs:
            scalars.setdefault(r["fn"], set()).update(k for k, v in r.items() if k != "fn" and not isinstance(v, bool))
    assert len(set(IDS)) == len(IDS) and len({LH.canon(r) for r in E.EDGES}) == len(E.EDGES)
    for rec in E.EDGES:
        names = set(ER.ARGS[rec["fn"]].split()) - set(ER.NOT_RECORDED)
        assert set(rec) - {"fn", "why"} == names, (rec, names)
        assert rec["fn"] in ER.REPLAY
        for k in scalars[rec["fn"]]:
            assert not isinstance(rec[k], bool) or rec["fn"] == "s2i_scale_dev", (rec, k)
        assert rec["why"] and "\n" not in rec["why"]
        for k, v in rec.items():        # a float argument is recorded as the fp32 value the kernel receives
            assert not isinstance(v, float) or v == ctypes.c_float(v).value, (rec, k)


@pytest.mark.parametrize("tag", E.TAGS)
def test_tag_is_reached_by_the_table(tag):
    assert any(tag in E.reach(r) for r in E.EDGES), tag


def test_reach_derives_nothing_unclaimed():
    derived = E.all_reached(E.EDGES)
    assert derived - set(E.TAGS) <= set(E.CENSUS_REACHED), sorted(derived - set(E.TAGS) - set(E.CENSUS_REACHED))
    assert not set(E.TAGS) & set(E.CENSUS_REACHED)
    assert len(set(E.TAGS)) == len(E.TAGS)


def test_step_census_reaches_no_tag():
    """The gap as a test: no launch of either workload runs any of the paths the table claims; and what CENSUS_REACHED says
    the step does run, it runs."""
    seen = set()
    for mode, recs in _census().items():
        for r in recs:
            got = E.reach(r)
            assert not got & set(E.TAGS), "%s: %s reaches %s" % (mode, LH.canon(r), sorted(got & set(E.TAGS)))
            seen |= got
    assert seen == set(E.CENSUS_REACHED), sorted(seen ^ set(E.CENSUS_REACHED))


# ---- the mirrors -------------------------------------------------------------------------------------------------------
def test_segment_mirrors_agree_with_the_library():
    lib = _lib.load()
    for H in list(range(2, 300)) + [1024]:
        assert lib.s2i_border_sums_workspace_bytes(3, H, 5, 8) == E.border_sums_workspace_bytes(3, H, 5, 8), H
    for HW in list(range(1, 600)) + [4095, 4096, 4097, 4159, 4160, 65536]:
        assert lib.s2i_spatial_sum_workspace_bytes(3, HW, 8) == E.spatial_sum_workspace_bytes(3, HW, 8), HW
    for recs in list(_census().values()) + [E.EDGES]:
        for r in recs:
            if r["fn"] == "s2i_tap_sums_dt":
                a = (r["B"], r["H"], r["W"], r["C"])
                assert lib.s2i_border_sums_workspace_bytes(*a) == E.border_sums_workspace_bytes(*a), a
            if r["fn"] == "s2i_spatial_sum_dt":
                a = (r["B"], r["HW"], r["C"])
                assert lib.s2i_spatial_sum_workspace_bytes(*a) == E.spatial_sum_workspace_bytes(*a), a


def test_mirrors_on_the_shapes_the_table_is_built_around():
    assert E.border_segments(34) == 8 and E.segments(34, 8) == (5, [(5 * s, min(34, 5 * s + 5)) for s in range(8)])
    assert E.segments(34, 8)[1][6] == (30, 34) and E.segments(34, 8)[1][7] == (35, 34)      # 4 rows, then none
    assert E.border_segments(130) == 32
    assert [s for s, (a, b) in enumerate(E.segments(130, 32)[1]) if b <= a] == list(range(26, 32))
    assert [E.border_segments(h) for h in (2, 3, 7, 8, 64, 128, 129, 4096)] == [1, 1, 1, 2, 16, 32, 32, 32]
    assert [E.spatial_segments(n) for n in (1, 16, 63, 127, 128, 130, 200, 4097, 9999)] == [1, 1, 1, 1, 2, 2, 3, 64, 64]
    assert E.segments(4097, 64)[1][-1] == (4095, 4097) and E.segments(200, 3)[1][-1] == (134, 200)
    assert E.red_geom(4) == (1, 1, 256, 1) and E.red_geom(12) == (3, 4, 64, 1) and E.red_geom(132) == (33, 64, 4, 1)
    assert E.red_geom(128) == (32, 32, 8, 1) and E.red_geom(1024) == (256, 256, 1, 1) and E.red_geom(1028) == (257, 256, 1, 2)
    assert E.grid_for(1) == 1 and E.grid_for(256 * 8192) == 8192 and E.grid_for(256 * 8192 + 1) == 8192
    assert E.trips(256 * 8192) == 1 and E.trips(256 * 8192 + 1) == 2 and E.trips(4099 * 513) == 2
    assert E.segments(1037, 16)[0] == 65 and E.segments(1037, 16)[1][-1] == (975, 1037)
    assert [b - a for a, b in E.segments(5, 8)[1]] == [1, 1, 1, 1, 1, 0, -1, -2]


# ---- the fp64 reference off the square shapes ----------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _tap_loop(dy):
    """tapsum[b][3 ky + kx][c]: dy summed over the output pixels (y, x) whose tap reads input pixel (y + ky - 1, x + kx - 1)
    inside the map."""
    B, H, W, C = dy.shape
    out = torch.zeros(B, 9, C, dtype=dy.dtype)
    for ky in range(3):
        for kx in range(3):
            for y in range(H):
                for x in range(W):
                    if 0 <= y + ky - 1 < H and 0 <= x + kx - 1 < W:
                        out[:, 3 * ky + kx] += dy[:, y, x]
    return out


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 7, 4), (2, 9, 5, 8), (1, 2, 2, 4), (1, 34, 6, 4), (2, 7, 34, 4), (1, 2, 5, 4)])
def test_tap_sums_off_the_square(B, H, W, C):
    dy = _randn(_gen(H * 100 + W), B, H, W, C)
    _close(R.tap_sums(dy), _tap_loop(dy))
    # the weight gradient of a depthwise 3 x 3, pad 1 convolution of an all-ones map, image by image
    for b in range(B):
        w = torch.zeros(C, 1, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(torch.ones(1, C, H, W, dtype=torch.float64), w, padding=1, groups=C)
        y.backward(dy[b:b + 1].permute(0, 3, 1, 2))
        _close(R.tap_sums(dy)[b], w.grad.reshape(C, 9).t())
    if H != W:
        assert float((R.tap_sums(dy) - R.tap_sums(dy.reshape(B, W, H, C))).abs().max()) > 1e-3      # the mutant is one


def _tap_sums_in_kernel_order(dy):
    """border_sums_stage1 / stage2 (csrc/s2i_cvec.hip) restated in fp32 numpy, sum by sum in the kernel's order: a lane adds
    its pixels of a band one after another, lane 0 adds the other lanes' sums, stage 2 adds the bands and forms
    total - row - column + corner.  dy: float32 [B][H][W][C] -> [B][9][C]."""
    import numpy as np
    B, H, W, C = dy.shape
    S, rpb = E.border_segments(H), E.red_geom(C)[2]
    tot = np.zeros((9, B, C), np.float32)
    for y0, y1 in E.segments(H, S)[1]:
        band = np.zeros((9, B, C), np.float32)
        for rl in range(min(rpb, W)):
            a = np.zeros((9, B, C), np.float32)
            for y in range(y0, y1):
                for x in range(rl, W, rpb):
                    on = (True, y == 0, y == H - 1, x == 0, x == W - 1, y == 0 and x == 0, y == 0 and x == W - 1,
                          y == H - 1 and x == 0, y == H - 1 and x == W - 1)
                    for k in range(9):
                        if on[k]:
                            a[k] += dy[:, y, x]
            band = a if rl == 0 else band + a
        tot += band
    out = np.zeros((B, 9, C), np.float32)
    for ky in range(3):
        for kx in range(3):
            er, ec = (1, 0, 2)[ky], (3, 0, 4)[kx]
            r = tot[0].copy()
            if er:
                r -= tot[er]
            if ec:
                r -= tot[ec]
            if er and ec:
                r += tot[5 + (2 if er == 2 else 0) + (1 if ec == 4 else 0)]
            out[:, 3 * ky + kx] = r
    return out


@pytest.mark.parametrize("B,H,W,C,measured", [(3, 2, 2, 4, 7.5e-8), (2, 3, 7, 12, 8.2e-8), (1, 34, 6, 64, 4.3e-8),
                                             (1, 4, 4, 1028, 1.6e-7)])
def test_tap_sums_bound_is_explained_by_rounding(B, H, W, C, measured):
    """GAMMA["tap_sums"] was 3e-8 of the image's total |dy|, measured on 64 x 64 maps; these records of the table measured
    `measured` on one MI355X.  The kernel's own summation order in fp32 on the host gives the same size of error, so it is
    rounding: below the new constant, above the old one, within a factor of two of what the GPU gave (the worst of four
    draws: a maximum over a few hundred elements moves by tens of percent from draw to draw)."""
    ratio = 0.0
    for seed in range(4):
        dy = torch.randn(B, H, W, C, generator=_gen(seed))
        got = torch.from_numpy(_tap_sums_in_kernel_order(dy.numpy())).double()
        dd = dy.double()
        ratio = max(ratio, float(((got - R.tap_sums(dd)).abs() / dd.abs().sum((1, 2)).unsqueeze(1)).max()))
    print("tap_sums %dx%dx%dx%d in fp32 on the host: %.3e (GPU %.1e)" % (B, H, W, C, ratio, measured))
    assert 3e-8 < ratio <= ER.GAMMA["tap_sums"] and measured / 2 <= ratio <= measured * 2


def _border_class(i, n):
    return 0 if i == 0 else (2 if i == n - 1 else 1)


@pytest.mark.parametrize("B,Cc,N,H,W", [(2, 5, 4, 4, 7), (1, 1, 3, 7, 3), (3, 130, 8, 3, 5), (2, 3, 4, 5, 4)])
def test_cvec_functions_against_conv2d_of_a_constant_map(B, Cc, N, H, W):
    g = _gen(Cc * 10 + H)
    Ip, Op = Cc + 3, N + 4
    c = _randn(g, B, Cc).requires_grad_(True)
    w = _randn(g, N, Cc, 3, 3).requires_grad_(True)
    packed = _randn(g, 9, Ip, Op)                                   # rows >= Cc and columns >= N are not the layer's
    packed[:, :Cc, :N] = w.detach().reshape(N, Cc, 9).permute(2, 1, 0)
    _close(R.packed_to_oihw(packed, Cc, N), w.detach(), 0.0)
    y = F.conv2d(c.view(B, Cc, 1, 1).expand(B, Cc, H, W), w, padding=1)
    table = R.cvec_bias_table(c.detach(), packed, Cc, N)
    for i in range(H):
        for j in range(W):
            _close(table[:, 3 * _border_class(i, H) + _border_class(j, W)], y.detach()[:, :, i, j])
    dy = _randn(g, B, H, W, N)
    y.backward(dy.permute(0, 3, 1, 2))
    tapsum = R.tap_sums(dy)
    _close(R.cvec_dc(packed, tapsum, Cc, N), c.grad, 1e-11)
    _close(R.cvec_dw(c.detach(), tapsum, N), w.grad, 1e-11)
    _close(R.cvec_dw(c.detach(), tapsum, N - 1), w.grad[:N - 1], 1e-11)        # O < N: the first O output channels


def _segment_loop(v, S):
    """[n][C] -> [S][C] over E.segments(n, S), empty ones as zeros."""
    out = torch.zeros(S, v.shape[1], dtype=v.dtype)
    for s, (a, b) in enumerate(E.segments(v.shape[0], S)[1]):
        for r in range(a, b):
            out[s] += v[r]
    return out


def test_row_sums_against_loops_at_the_table_s_chunkings():
    g = _gen(7)
    seen = set()
    for rec in E.EDGES:
        if rec["fn"] == "s2i_colstats":
            y = _randn(g, rec["M"], rec["C"])
            part = R.colstats(y, rec["nparts"])
            _close(part[0], _segment_loop(y, rec["nparts"]))
            _close(part[1], _segment_loop(y * y, rec["nparts"]))
            seen |= E.reach(rec)
        if rec["fn"] == "s2i_spatial_sum_dt":
            B, HW, C, ld = rec["B"], rec["HW"], rec["C"], rec["ld"]
            src = _randn(g, B * HW, ld)
            want = torch.stack([_segment_loop(src[b * HW:(b + 1) * HW, :C], E.spatial_segments(HW)).sum(0) for b in range(B)])
            _close(R.spatial_sum(src, B, C), want)
    assert {"colstats:empty segment", "colstats:short last segment"} <= seen
    # chunk_sums with groups: every group is split on its own
    for G, Rg, ppg in ((2, 5, 8), (3, 517, 8), (2, 1037, 16), (1, 33, 2)):
        v = _randn(g, G, Rg, 4)
        _close(R.chunk_sums(v, ppg), torch.cat([_segment_loop(v[k], ppg) for k in range(G)]))


def _cal_torch(S, labels, D):
    """The class-aware loss as a torch expression: relu(mean S - mean of S over same-class off-diagonal pairs) / D, and
    the gradient the kernel hands out (d loss / d S plus its transpose)."""
    B = S.shape[0]
    S = S.clone().requires_grad_(True)
    same = (labels.view(-1, 1) == labels.view(1, -1)) & ~torch.eye(B, dtype=torch.bool)
    if int(same.sum()) == 0:
        return torch.zeros((), dtype=S.dtype), torch.zeros_like(S)
    loss = torch.relu(S.mean() - S[same].mean()) / D
    loss.backward()
    return loss.detach(), S.grad + S.grad.t()


def test_cal_loss_inactive_branches():
    g = _gen(11)
    # no same-label pair
    for B in (5, 17):
        S, labels = _randn(g, B, B), torch.arange(B, dtype=torch.int32)
        loss, dS = R.cal_loss(S, labels, 64)
        assert float(loss) == 0 and not dS.any()
        tl, tg = _cal_torch(S, labels, 64)
        assert float(tl) == 0 and not tg.any()
    # diff < 0: the same-label pairs score 4, everything else 0
    for B in (5, 17):
        labels = (torch.arange(B) % 2).to(torch.int32)
        same = (labels.view(-1, 1) == labels.view(1, -1)) & ~torch.eye(B, dtype=torch.bool)
        S = 4.0 * same.double()
        loss, dS = R.cal_loss(S, labels, 64)
        tl, tg = _cal_torch(S, labels, 64)
        assert float(S.mean() - S[same].mean()) < 0
        assert float(loss) == 0 and not dS.any() and float(tl) == 0 and not tg.any()
    # and the active branch, for the expression itself
    X = _randn(g, 17, 64)
    S, labels = X @ X.t(), (torch.arange(17) % 4).to(torch.int32)
    loss, dS = R.cal_loss(S, labels, 64)
    tl, tg = _cal_torch(S, labels, 64)
    assert float(loss) > 0
    _close(loss, tl)
    _close(dS, tg)


def test_logit_backward_against_autograd_at_b_300():
    g = _gen(13)
    B, C = 300, 4
    x = _randn(g, B, 4, 4, C).requires_grad_(True)
    w = (0.05 * _randn(g, 1, C, 4, 4)).requires_grad_(True)
    b = _randn(g, 1).requires_grad_(True)
    prob = torch.sigmoid(torch.einsum("bhwc,chw->b", x, w[0]) + b[0])
    _close(R.logit_forward(x.detach(), w.detach(), b.detach()), prob.detach())
    dprob = _randn(g, B)
    prob.backward(dprob)
    dl, dx, dw, db = R.logit_backward(x.detach(), w.detach(), prob.detach(), dprob)
    _close(dx, x.grad)
    _close(dw, w.grad)
    _close(db, b.grad)
    # what the mutant of the GPU suite leaves out is visible
    assert float((R.logit_backward(x.detach()[:256], w.detach(), prob.detach()[:256], dprob[:256])[2] - dw).abs().max()) > 1e-4


@pytest.mark.parametrize("B,target,weight", [(300, 0.0, 1.0), (300, 1.0, 0.5), (300, 0.3, 2.0), (3, 0.0, 0.5), (1, 1.0, 1.0)])
def test_bce_against_torch_at_exact_0_and_1(B, target, weight):
    """torch's BCELoss is the definition: log clamped at -100, the gradient's denominator at 1e-12."""
    g = _gen(B)
    p = 0.02 + 0.96 * torch.rand(B, generator=g, dtype=torch.float64)
    p[0] = 0.0
    p[-1] = 1.0 if B > 1 else 0.0
    p.requires_grad_(True)
    loss = weight * F.binary_cross_entropy(p, torch.full_like(p, target))
    gout = 0.7
    (gout * loss).backward()
    _close(R.bce_forward(p.detach(), target, weight), loss.detach())
    assert torch.isfinite(p.grad).all()
    # torch clamps the denominator at the fp32 constant 1e-12f = 1e-12 (1 - 4e-9), elementwise_ref at the double: where
    # the clamp acts (p = 0 or 1) the two differ by 4e-9 of the element, far below what an fp32 kernel resolves
    got = R.bce_backward(p.detach(), target, weight, gout)
    assert bool(((got - p.grad).abs() <= 1e-8 * p.grad.abs() + 1e-14).all())


def test_bce_multi_against_torch_above_one_stride():
    g = _gen(17)
    G, H, B = 2, 3, 130
    probs = [(0.02 + 0.96 * torch.rand(G * B, generator=g, dtype=torch.float64)) for _ in range(H)]
    for p in probs:
        p[1], p[2] = 0.0, 1.0
        p.requires_grad_(True)
    target = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0, 1.0], dtype=torch.float64)
    weight = 0.5 + 0.37 * torch.arange(G * H, dtype=torch.float64)
    loss = sum(weight[k * H + h] * F.binary_cross_entropy(probs[h][k * B:(k + 1) * B], target[k * H + h].expand(B))
               for k in range(G) for h in range(H))
    (0.7 * loss).backward()
    det = [p.detach() for p in probs]
    _close(R.bce_multi_forward(det, target, weight, G, B), loss.detach())
    for got, p in zip(R.bce_multi_backward(det, target, weight, G, B, 0.7), probs):
        assert bool(((got - p.grad).abs() <= 1e-8 * p.grad.abs() + 1e-14).all())      # 1e-12f, as above
