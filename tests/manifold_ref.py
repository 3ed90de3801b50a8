"""Plain-numpy references of the kernel inception distance and the k-nearest-neighbour manifold metrics (gan_metrics.kid,
gan_metrics.prdc; csrc/s2i_manifold.hip): float64 brute force for the metrics, an fp32 restatement of the one kernel that
computes in fp32, the error bounds the GPU tests hold the kernels to, and the seeded inputs both suites share."""
import numpy as np

F32_EPS = 2.0 ** -24          # unit roundoff of fp32
F64_ULP = 2.0 ** -52


# ---- KID ---------------------------------------------------------------------------------------------------------------
def poly_kernel(a, b):
    """k[i][j] = (a_i . b_j / D + 1)^3 in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a @ b.T / a.shape[1] + 1.0) ** 3


def kid_ref(x, y):
    """The unbiased MMD^2 estimator over the full samples, float64 (gan_metrics.kid)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m, n = x.shape[0], y.shape[0]
    kxx, kyy, kxy = poly_kernel(x, x), poly_kernel(y, y), poly_kernel(x, y)
    np.fill_diagonal(kxx, 0.0)
    np.fill_diagonal(kyy, 0.0)
    return kxx.sum() / (m * (m - 1.0)) + kyy.sum() / (n * (n - 1.0)) - 2.0 * kxy.sum() / (float(m) * n)


def kid_sum_bound(x, y):
    """What reordering the fp64 sums can change in kid_ref when every kernel value is exact: each of the three sums over
    P terms moves by at most P 2^-52 sum|k|, then divided as the estimator divides it."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m, n = x.shape[0], y.shape[0]
    out = 0.0
    for a, b, scale in ((x, x, 1.0 / (m * (m - 1.0))), (y, y, 1.0 / (n * (n - 1.0))), (x, y, 2.0 / (float(m) * n))):
        k = np.abs(poly_kernel(a, b))
        out += scale * k.size * F64_ULP * k.sum()
    return out


def kid_fp32_bound(x, y):
    """Worst case of the fp32 scores behind KID: T_xx + T_yy + 2 T_xy with
    T_ab = max over pairs of 3 (|a.b| / D + 1)^2 (D + 2) 2^-24 |a| |b| / D: a D-term fp32 dot product is off by at most
    (D + 2) 2^-24 |a| |b| (the products, the sums, the store), the kernel's slope in the score is 3 t^2 / D, and a mean of
    values each off by at most T is off by at most T."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    D = x.shape[1]

    def T(a, b):
        na, nb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
        s = np.abs(a @ b.T)
        return float((3.0 * (s / D + 1.0) ** 2 * (D + 2) * F32_EPS * np.outer(na, nb) / D).max())

    return T(x, x) + T(y, y) + 2.0 * T(x, y)


# ---- the kernels ---------------------------------------------------------------------------------------------------------
def own_columns(Q, N, base, own_base):
    """[Q] the column of every query that is its own row, -1 where none lies in the block."""
    if own_base is None or own_base < 0:
        return np.full(Q, -1, np.int64)
    c = own_base + np.arange(Q, dtype=np.int64) - base
    return np.where((c >= 0) & (c < N), c, -1)


def polykernel_rows_ref(scores, inv_d, base=0, own_base=None):
    """(sum [Q], sum of |k| [Q]) of s2i_polykernel_rows in float64: the same operations on every entry, numpy's order of
    summation."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    t = s * np.float64(inv_d) + 1.0
    k = t * t * t
    own = own_columns(s.shape[0], s.shape[1], base, own_base)
    rows = np.nonzero(own >= 0)[0]
    k[rows, own[rows]] = 0.0
    return k.sum(axis=1), np.abs(k).sum(axis=1)


def sqdist_rows_ref(scores, q_norm2, row_norm2, base=0, own_base=None):
    """s2i_sqdist_rows restated in fp32, operation by operation: -max(0, (qn + rn) - 2 s), NaN kept, the own row -inf."""
    s = np.asarray(scores, np.float32)
    Q, N = s.shape
    qn = np.asarray(q_norm2, np.float32).reshape(Q, 1)
    rn = np.asarray(row_norm2, np.float32)[base:base + N].reshape(1, N)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (qn + rn) - np.float32(2.0) * s
        nd = -np.maximum(np.float32(0.0), d)            # np.maximum hands a NaN on
    assert nd.dtype == np.float32
    own = own_columns(Q, N, base, own_base)
    rows = np.nonzero(own >= 0)[0]
    nd[rows, own[rows]] = -np.inf
    return nd


def ball_rows_ref(nd, row_bound, base=0, count=None, best=None):
    """(count, best) of s2i_ball_rows from the given starting values (zeros and -inf by default)."""
    nd = np.asarray(nd, np.float32)
    Q, N = nd.shape
    b = np.asarray(row_bound, np.float32)[base:base + N]
    count = np.zeros(Q, np.int32) if count is None else np.asarray(count, np.int32).copy()
    best = np.full(Q, -np.inf, np.float32) if best is None else np.asarray(best, np.float32).copy()
    with np.errstate(invalid="ignore"):
        count += (nd >= b[None, :]).sum(axis=1).astype(np.int32)       # a NaN on either side compares false
        top = np.where(np.isnan(nd), -np.inf, nd).max(axis=1).astype(np.float32)
        best = np.where(top > best, top, best).astype(np.float32)
    return count, best


# ---- precision, recall, density, coverage ---------------------------------------------------------------------------------
def sqdist64(a, b):
    """[len(a), len(b)] squared distances in float64 from the differences themselves (no cancellation)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    for i in range(a.shape[0]):
        diff = b - a[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def radii2(d2_self, k):
    """[n] squared distance from every row to its k-th nearest OTHER row."""
    d = d2_self.copy()
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, k - 1]


def prdc_ref(real, fake, nearest_k=5, band=0.0):
    """Brute-force float64 precision / recall / density / coverage with a ball's surface inside it (gan_metrics.prdc), the
    per-query quantities behind them, and which queries an error of `band` in a squared distance or radius could change:

    fake_count [M]  real balls that hold each fake row      real_count [N]  fake balls that hold each real row
    fake_near  [M]  squared distance to the nearest real    real_near  [N]  squared distance to the nearest fake row
    real_covered [N]  real_near <= r_real^2
    fake_undecided [M]  some real i has |d^2(fake, real_i) - r_real_i^2| <= band
    real_undecided [N]  some fake j has |d^2(real, fake_j) - r_fake_j^2| <= band, or |real_near - r_real^2| <= band
    fake_band_pairs, real_band_pairs  the number of such pairs in all (the coverage comparison counts as one)."""
    k = int(nearest_k)
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    N, M = real.shape[0], fake.shape[0]
    assert N > k and M > k
    r2_real, r2_fake = radii2(sqdist64(real, real), k), radii2(sqdist64(fake, fake), k)
    d_fr = sqdist64(fake, real)                              # [M, N]
    d_rf = d_fr.T                                            # [N, M]
    fake_count = (d_fr <= r2_real[None, :]).sum(axis=1)
    real_count = (d_rf <= r2_fake[None, :]).sum(axis=1)
    fake_near, real_near = d_fr.min(axis=1), d_rf.min(axis=1)
    covered = real_near <= r2_real
    f_band = np.abs(d_fr - r2_real[None, :]) <= band
    r_band = np.abs(d_rf - r2_fake[None, :]) <= band
    c_band = np.abs(real_near - r2_real) <= band
    return dict(precision=float((fake_count > 0).sum()) / M, recall=float((real_count > 0).sum()) / N,
                density=float(fake_count.sum()) / (float(k) * M), coverage=float(covered.sum()) / N,
                fake_count=fake_count, real_count=real_count, fake_near=fake_near, real_near=real_near,
                real_covered=covered, r2_real=r2_real, r2_fake=r2_fake,
                fake_undecided=f_band.any(axis=1), real_undecided=r_band.any(axis=1) | c_band,
                fake_band_pairs=int(f_band.sum()), real_band_pairs=int(r_band.sum() + c_band.sum()))


def prdc_band(real, fake):
    """How far a squared distance of the GPU pipeline can be from the float64 one: |a|^2 + |b|^2 - 2 a.b in fp32 with
    each term below 2 max|x|^2 and D-term sums, 2 (D + 4) 2^-24 2 max|x|^2 with room for the stored norms and the two
    additions."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    D = real.shape[1]
    top = max((real * real).sum(1).max(), (fake * fake).sum(1).max())
    return 2.0 * (D + 4) * F32_EPS * 2.0 * top


# ---- the inputs -------------------------------------------------------------------------------------------------------------
INTEGER_SHAPES = dict(D=2048, real=130, fake=150, chunk_rows=64, query_block=50)
REAL_SHAPES = dict(D=64, real=257, fake=391, chunk_rows=128, query_block=100)
REAL_SEEDS = (0, 1)
WIDE_SHAPES = dict(D=2048, real=257, fake=391, chunk_rows=128, query_block=100, seed=0)


def integer_rows(seed=0):
    """(real [130, 2048], fake [150, 2048]) fp32 with integer entries in [-3, 3]: every product and squared norm is an
    integer below 2^24, so the fp32 scores and distances are exact and the GPU must equal float64 brute force.  A few rows
    are copies (within and across the sets): distances of exactly 0 and exact ties."""
    rng = np.random.default_rng(seed)
    s = INTEGER_SHAPES
    real = rng.integers(-3, 4, size=(s["real"], s["D"])).astype(np.float32)
    fake = rng.integers(-3, 4, size=(s["fake"], s["D"])).astype(np.float32)
    real[70] = real[3]                     # a duplicate inside the real set, in another chunk and query block
    fake[149] = fake[10]
    fake[64] = real[129]                   # fakes that sit on real rows
    fake[65] = real[129]
    fake[0] = real[0]
    return real, fake


def real_valued_rows(seed, D=REAL_SHAPES["D"], n_real=REAL_SHAPES["real"], n_fake=REAL_SHAPES["fake"]):
    """(real, fake) fp32: real standard normal, fake 0.9 x normal shifted by +0.3 along coordinate 0, one generator."""
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((n_real, D))
    fake = 0.9 * rng.standard_normal((n_fake, D))
    fake[:, 0] += 0.3
    return real.astype(np.float32), fake.astype(np.float32)
