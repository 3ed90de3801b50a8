"""Host side of KID and precision / recall / density / coverage (no GPU here): the float64 references of tests/
manifold_ref.py against hand computation, the conditions the GPU suite's inputs are chosen to meet, the three
s2i_manifold.hip symbols with their refusals, the refusal of CPU tensors, and the command line's three flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import manifold_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_ARGS = ["--netG", "netG_1.pth", "--inception", "i.pth", "--data_dir", "d"]


# ---- the references --------------------------------------------------------------------------------------------------------
def test_kid_ref_against_a_double_loop():
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((5, 6)), rng.standard_normal((4, 6)) + 0.5
    D = 6

    def k(a, b):
        return (float(np.dot(a, b)) / D + 1.0) ** 3

    sxx = sum(k(x[i], x[j]) for i in range(5) for j in range(5) if i != j)
    syy = sum(k(y[i], y[j]) for i in range(4) for j in range(4) if i != j)
    sxy = sum(k(x[i], y[j]) for i in range(5) for j in range(4))
    want = sxx / (5 * 4) + syy / (4 * 3) - 2.0 * sxy / (5 * 4)
    got = M.kid_ref(x, y)
    assert abs(got - want) <= 1e-13 * (abs(sxx) / 20 + abs(syy) / 12 + 2 * abs(sxy) / 20), (got, want)
    assert abs(M.kid_ref(x, x[::-1].copy())) > 0           # the same set twice: -2/(m) of the diagonal's mean, not 0
    assert M.kid_ref(x, y) == M.kid_ref(x, y) and M.kid_ref(y, x) == pytest.approx(got, rel=1e-12)


def test_prdc_ref_on_hand_cases():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((12, 3))
    same = M.prdc_ref(a, a.copy(), nearest_k=2)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0
    # a fake on a real row lies in that row's ball and in the balls of the rows that count it among their 2 nearest
    assert same["density"] >= 0.5 and (same["fake_count"] >= 1).all() and (same["fake_near"] == 0).all()
    far = M.prdc_ref(a, a + 100.0, nearest_k=2)
    assert far["precision"] == far["recall"] == far["density"] == far["coverage"] == 0.0
    assert not far["fake_undecided"].any() and not far["real_undecided"].any()
    # five points on a line, by hand: real 0 1 2 3 10, fake 0.4 2.5 20; k = 1
    real = np.array([[0.0], [1.0], [2.0], [3.0], [10.0]])
    fake = np.array([[0.4], [2.5], [20.0]])
    r = M.prdc_ref(real, fake, nearest_k=1)
    assert np.array_equal(r["r2_real"], [1.0, 1.0, 1.0, 1.0, 49.0])        # each to its nearest other real row
    np.testing.assert_allclose(r["r2_fake"], [2.1 ** 2, 2.1 ** 2, 17.5 ** 2], rtol=1e-14)
    assert np.array_equal(r["fake_count"], [2, 2, 0])                      # 0.4: balls of 0, 1; 2.5: of 2, 3 (10's ends at 3)
    assert r["precision"] == 2 / 3 and r["density"] == 4 / 3
    # the balls of 0.4 and 2.5 have radius 2.1, that of 20 reaches down to 2.5
    assert np.array_equal(r["real_count"], [1, 2, 2, 2, 1])
    assert r["recall"] == 1.0
    assert np.array_equal(r["real_covered"], [True, True, True, True, False]) and r["coverage"] == 4 / 5
    # the surface of a ball is inside: a fake at distance exactly r
    edge = M.prdc_ref(np.array([[0.0], [1.0], [5.0]]), np.array([[2.0], [2.5], [9.0]]), nearest_k=1)
    assert edge["fake_count"][0] == 2 and edge["real_covered"][1]          # |2 - 1| = r(1) = 1, and |2 - 5| < r(5) = 4
    assert edge["fake_undecided"][0] and edge["real_undecided"][1]         # and that is what a band of 0 already flags


def test_kernel_restatements():
    s = np.array([[1.0, -2.0, 3.0, 0.5]], np.float32)
    tot, mag = M.polykernel_rows_ref(s, 0.5, base=10, own_base=12)          # query 0 is row 12: column 2 is left out
    assert tot[0] == 1.5 ** 3 + 0.0 + 1.25 ** 3 and mag[0] == tot[0]
    nd = M.sqdist_rows_ref(np.array([[1.0, 5.0, np.nan, 2.0]], np.float32), [2.0], [9, 9, 1.0, 3.0, 1.0, 4.0], base=2,
                           own_base=5)
    assert np.array_equal(nd[0, :2], np.float32([-1.0, -0.0])) and np.signbit(nd[0, 1])      # 5 - 10 clamps to 0
    assert np.isnan(nd[0, 2]) and nd[0, 3] == -np.inf                      # the NaN stays, row 5 is the query itself
    cnt, best = M.ball_rows_ref(np.array([[-1.0, np.nan, -3.0, -0.5]], np.float32), [7, -2.0, -9.0, np.nan, -0.5], base=1,
                                count=[4], best=[-0.75])
    assert cnt[0] == 4 + 2 and best[0] == np.float32(-0.5)                 # -1 >= -2 and -0.5 >= -0.5; NaNs count nothing


# ---- the conditions the GPU suite's inputs meet ------------------------------------------------------------------------------
def test_integer_rows_are_exact_in_fp32_and_tie():
    real, fake = M.integer_rows()
    s = M.INTEGER_SHAPES
    assert real.shape == (s["real"], s["D"]) and fake.shape == (s["fake"], s["D"])
    both = np.concatenate([real, fake]).astype(np.float64)
    assert np.array_equal(both, np.round(both)) and np.abs(both).max() == 3
    top = (both * both).sum(1).max()
    print("integer rows: max |x|^2 %d" % top)
    assert 4 * top < 2 ** 24                    # |a|^2 + |b|^2 + 2 |a.b| <= 4 max|x|^2: every intermediate is exact
    assert s["real"] % s["chunk_rows"] and s["fake"] % s["chunk_rows"] and s["fake"] % s["query_block"] == 0
    for k in (1, 5):
        r = M.prdc_ref(real, fake, k)
        assert r["fake_band_pairs"] > 0 and r["real_band_pairs"] > 0      # band 0: pairs exactly on a surface
        assert (r["fake_near"] == 0).sum() >= 3
        assert 0 < r["precision"] < 1 or 0 < r["recall"] < 1, r


@pytest.mark.parametrize("seed", M.REAL_SEEDS)
def test_real_valued_rows_leave_few_queries_undecided_and_a_kid_above_its_bound(seed):
    real, fake = M.real_valued_rows(seed)
    s = M.REAL_SHAPES
    assert real.shape == (s["real"], s["D"]) and fake.shape == (s["fake"], s["D"]) and real.dtype == np.float32
    kid, bound = M.kid_ref(fake, real), M.kid_fp32_bound(fake, real)
    band = M.prdc_band(real, fake)
    r = M.prdc_ref(real, fake, 5, band)
    nf, nr = int(r["fake_undecided"].sum()), int(r["real_undecided"].sum())
    print("seed %d: kid %.4g, fp32 bound %.3g, band %.3g, undecided %d / %d fake (%d pairs), %d / %d real (%d pairs)"
          % (seed, kid, bound, band, nf, s["fake"], r["fake_band_pairs"], nr, s["real"], r["real_band_pairs"]))
    assert kid > 10 * bound                                   # the KID test discriminates
    assert nf <= 0.02 * s["fake"] and nr <= 0.02 * s["real"]
    # every undecided query has one pair in the band, so its count moves by one at the most
    assert r["fake_band_pairs"] == nf and r["real_band_pairs"] == nr
    assert 0 < r["precision"] < 1 and 0 < r["recall"] < 1 and r["density"] > 0


# ---- symbols, refusals, wrappers -------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from speech_to_image_translation_without_text_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    assert re.search(r"\bint s2i_polykernel_rows\(const float\* scores, int Q, int N, int lds, int base, int own_base, "
                     r"double inv_d, double\* sum,\s+void\* stream\);", header)
    assert re.search(r"\bint s2i_sqdist_rows\(float\* scores, int Q, int N, int lds, int base, int own_base, "
                     r"const float\* q_norm2,\s+const float\* row_norm2, int n_rows, void\* stream\);", header)
    assert re.search(r"\bint s2i_ball_rows\(const float\* nd, int Q, int N, int lds, int base, const float\* row_bound, "
                     r"int n_rows, int\* count,\s+float\* best, void\* stream\);", header)
    lib = _lib.load()
    for name in ("s2i_polykernel_rows", "s2i_sqdist_rows", "s2i_ball_rows"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
    for name in ("polykernel_rows", "sqdist_rows", "ball_rows"):
        assert callable(getattr(ops, name))
    makefile = open(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "csrc", "Makefile")).read()
    assert "s2i_manifold.hip" in makefile


def test_bad_arguments_are_refused_before_any_device_is_touched():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    f = (ctypes.c_double * 8)()
    fa = ctypes.addressof(f)                                         # host memory: never dereferenced

    def refused(call, prefix, word):
        assert call() != 0
        msg = lib.s2i_last_error().decode()
        assert msg.startswith(prefix + ":") and word in msg, msg

    def poly(word, scores=fa, Q=1, N=4, lds=4, base=0, own=-1, inv_d=0.5, out=fa):
        refused(lambda: lib.s2i_polykernel_rows(scores, Q, N, lds, base, own, inv_d, out, None), "polykernel_rows", word)

    def sqd(word, scores=fa, Q=1, N=4, lds=4, base=0, own=-1, qn=fa, rn=fa, n_rows=8):
        refused(lambda: lib.s2i_sqdist_rows(scores, Q, N, lds, base, own, qn, rn, n_rows, None), "sqdist_rows", word)

    def ball(word, nd=fa, Q=1, N=4, lds=4, base=0, bound=fa, n_rows=8, count=fa, best=fa):
        refused(lambda: lib.s2i_ball_rows(nd, Q, N, lds, base, bound, n_rows, count, best, None), "ball_rows", word)

    for fn in (poly, sqd, ball):
        fn("positive", Q=0)
        fn("positive", N=0)
        fn("stride", lds=3)
        fn("leave int", base=-1)
        fn("leave int", base=2 ** 31 - 3)
    poly("null", scores=None)
    poly("null", out=None)
    poly("own_base", own=-2)
    poly("finite", inv_d=float("inf"))
    poly("finite", inv_d=float("nan"))
    poly("aligned", scores=fa + 2)
    poly("aligned", out=fa + 4)
    sqd("null", scores=None)
    sqd("null", qn=None)
    sqd("null", rn=None)
    sqd("own_base", own=-2)
    sqd("row norms", base=5)                                         # 5 + 4 > 8 norms
    sqd("aligned", rn=fa + 2)
    ball("null", nd=None)
    ball("null", bound=None)
    ball("null", count=None, best=None)
    ball("row bounds", base=5)
    ball("aligned", count=fa + 2)


def test_wrappers_validate_and_there_is_no_cpu_fallback():
    import torch
    from speech_to_image_translation_without_text_amd import _lib, gan_metrics as GM, ops, retrieval
    x = torch.zeros(2, 8)
    f32, f64, i32, wide = torch.zeros(2), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), torch.zeros(8)
    calls = ((ops.polykernel_rows, dict(scores=x, inv_d=0.5, sums=f64)),
             (ops.sqdist_rows, dict(scores=x, q_norm2=f32, row_norm2=wide)),
             (ops.ball_rows, dict(nd=x, row_bound=wide, count=i32, best=f32)))
    for fn, good in calls:
        first = "nd" if fn is ops.ball_rows else "scores"
        for change in ({first: torch.zeros(8)}, {first: x.double()}, {first: x.t()}, dict(base=-1), dict(base=2 ** 31 - 8)):
            with pytest.raises(ValueError):
                fn(**dict(good, **change))
        with pytest.raises(_lib.S2IError, match="no CPU fallback"):
            fn(**good)                                               # CPU tensors
    with pytest.raises(ValueError):
        ops.polykernel_rows(x, float("nan"), f64)
    with pytest.raises(ValueError):
        ops.polykernel_rows(x, 0.5, f64, own_base=-2)
    for fn in (GM.kid, GM.prdc):
        with pytest.raises(_lib.S2IError, match="no CPU fallback"):
            fn(torch.zeros(8, 4), torch.zeros(9, 4))
        with pytest.raises(ValueError):
            fn(torch.zeros(8, 4).double(), torch.zeros(9, 4))
    with pytest.raises(_lib.S2IError, match="no CPU fallback"):
        retrieval.pack_device_rows(torch.zeros(8, 4))
    doc = " ".join(GM.kid.__doc__.split())
    assert "same expectation" in doc and "lower variance" in doc and "no seed" in doc


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_command_line_flags_default_off_and_turn_keep_rows_on():
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    args = GM.parse_args(BASE_ARGS)
    assert (args.kid, args.prdc, args.nearest_k, args.keep_rows) == (False, False, 5, False)
    args = GM.parse_args(BASE_ARGS + ["--kid"])
    assert (args.kid, args.prdc, args.keep_rows) == (True, False, True)
    args = GM.parse_args(BASE_ARGS + ["--prdc"])
    assert (args.kid, args.prdc, args.nearest_k, args.keep_rows) == (False, True, 5, True)
    args = GM.parse_args(BASE_ARGS + ["--nearest_k", "3"])
    assert (args.prdc, args.nearest_k, args.keep_rows) == (True, 3, True)
    args = GM.parse_args(BASE_ARGS + ["--kid", "--prdc", "--nearest_k", "64"])
    assert (args.kid, args.prdc, args.nearest_k) == (True, True, 64)
    for bad in ("0", "65"):
        with pytest.raises(SystemExit):
            GM.parse_args(BASE_ARGS + ["--nearest_k", bad])


@pytest.mark.parametrize("flags", [["--kid"], ["--prdc"], ["--nearest_k", "3"]])
def test_command_line_refuses_the_flags_with_real_statistics_that_exist(flags, tmp_path, capsys):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    stats = tmp_path / "real.npz"
    args = GM.parse_args(BASE_ARGS + flags + ["--real_stats", str(stats)])          # not there yet: it will be written
    assert args.real_stats_mode == "write" and args.keep_rows
    GM.save_stats(str(stats), np.zeros(4), np.eye(4), 9)
    assert GM.parse_args(BASE_ARGS + ["--real_stats", str(stats)]).real_stats_mode == "read"
    with pytest.raises(SystemExit):
        GM.parse_args(BASE_ARGS + flags + ["--real_stats", str(stats)])
    assert "no real rows" in capsys.readouterr().err
