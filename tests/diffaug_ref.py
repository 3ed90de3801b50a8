"""numpy reference of the differentiable-augmentation operator (include/s2i_hip.h, s2i_diffaug_forward / _backward), its
mutants, and the fixed inputs that the CPU and GPU suites share.

Forward and adjoint are fp64; the integer draws are float32 exactly as the header states them (one float32 multiply,
truncation), so they give the kernel's integers bit for bit.  The float32 uniforms themselves enter the fp64 arithmetic
unrounded: b = u_b - 0.5, s = 2 u_s, k = u_c + 0.5 in fp64.

A mutant is the reference with one deliberate mistake, selected by name: both suites assert that the comparison in use
tells every mutant from the reference."""
import numpy as np

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
POLICIES = tuple(range(8))
ONE_BELOW = np.float32(0.99999994)      # the largest float32 below 1

MUTANTS = (
    "translation_sign",              # out[r][q] = z[r - ty][q - tx]
    "cutout_row_shift",              # the cutout window one row lower
    "contrast_mean_without_b",       # contrast about m where m + b belongs
    "channel_mean_over_4",           # the pixel's channel mean as sum / 4
    "adjoint_without_mean",          # g_y = k g_z: the (1 - k) mean term dropped
    "cutout_before_translation",     # the window cut from z, then moved with it
)

# the bounds of the GPU suite (tests/test_diffaug_gpu.py) for policies with COLOR: absolute on the forward of inputs in
# [-1, 1]; times max |dy| on the backward
FWD_TOL = 1e-5
BWD_TOL = 1e-5


def geometry(H):
    """(S, n_t, c, n_c) of an H x H image."""
    S = int(H * 0.125 + 0.5)
    c = int(H * 0.5 + 0.5)
    return S, 2 * S + 1, c, H + 1 - (c % 2)


def draw(u, n):
    """min(int(u * n), n - 1) with the product one float32 multiply."""
    prod = np.asarray(u, dtype=np.float32) * np.float32(n)
    assert prod.dtype == np.float32
    return np.minimum(prod.astype(np.int64), n - 1)


def draws(table, policy, H):
    """Per image: tx, ty (0 without TRANSLATION) and the clipped cutout window r0, r1, q0, q1 (empty without CUTOUT)."""
    table = np.asarray(table, dtype=np.float32)
    N = table.shape[0]
    S, n_t, c, n_c = geometry(H)
    tx = ty = np.zeros(N, dtype=np.int64)
    r0 = r1 = q0 = q1 = np.zeros(N, dtype=np.int64)
    if policy & TRANSLATION:
        tx, ty = draw(table[:, 3], n_t) - S, draw(table[:, 4], n_t) - S
    if policy & CUTOUT:
        ox, oy = draw(table[:, 5], n_c), draw(table[:, 6], n_c)
        r0, r1 = np.maximum(oy - c // 2, 0), np.minimum(oy - c // 2 + c, H)
        q0, q1 = np.maximum(ox - c // 2, 0), np.minimum(ox - c // 2 + c, H)
    return dict(tx=tx, ty=ty, r0=r0, r1=r1, q0=q0, q1=q1)


def colour_factors(table, policy):
    t = np.asarray(table, dtype=np.float32).astype(np.float64)
    N = t.shape[0]
    if not policy & COLOR:
        return np.zeros(N), np.ones(N), np.ones(N)
    return t[:, 0] - 0.5, 2.0 * t[:, 1], t[:, 2] + 0.5


def live_mask(d, n, H, mutant=None):
    """[H][H] bool over OUTPUT pixels of image n: the source lies inside the image and the cutout spares the pixel."""
    tx, ty = int(d["tx"][n]), int(d["ty"][n])
    if mutant == "translation_sign":
        tx, ty = -tx, -ty
    r0, r1, q0, q1 = (int(d[k][n]) for k in ("r0", "r1", "q0", "q1"))
    if mutant == "cutout_row_shift" and r1 > r0:
        r0, r1 = min(r0 + 1, H), min(r1 + 1, H)
    r, q = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    inside = (r + ty >= 0) & (r + ty < H) & (q + tx >= 0) & (q + tx < H)
    cut = (r >= r0) & (r < r1) & (q >= q0) & (q < q1)
    if mutant == "cutout_before_translation":       # the window sits in z's coordinates and moves with the image
        rs, qs = r + ty, q + tx
        cut = (rs >= r0) & (rs < r1) & (qs >= q0) & (qs < q1)
    return inside & ~cut, tx, ty


def forward(x, table, policy, mutant=None):
    """x [N][3][H][H] -> y [N][H][H][4] float64."""
    x = np.asarray(x, dtype=np.float64)
    N, C, H, W = x.shape
    assert C == 3 and H == W and H % 2 == 0
    d = draws(table, policy, H)
    b, s, k = colour_factors(table, policy)
    out = np.zeros((N, H, W, 4))
    r, q = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    for n in range(N):
        z = x[n]
        if policy & COLOR:
            m = z.mean()
            p = z.sum(0) / (4.0 if mutant == "channel_mean_over_4" else 3.0)
            y = ((z + b[n]) - (p + b[n])) * s[n] + (p + b[n])
            mb = m if mutant == "contrast_mean_without_b" else m + b[n]
            z = (y - mb) * k[n] + mb
        live, tx, ty = live_mask(d, n, H, mutant)
        rs, qs = np.clip(r + ty, 0, H - 1), np.clip(q + tx, 0, H - 1)
        moved = z[:, rs, qs]                                      # [3][H][H]
        out[n, :, :, :3] = np.where(live[None], moved, 0.0).transpose(1, 2, 0)
    return out


def adjoint(dy, table, policy, mutant=None):
    """dy [N][H][H][>= 3] (the first three channels count) -> dx [N][3][H][H] float64: the transpose of forward's linear
    part."""
    dy = np.asarray(dy, dtype=np.float64)[..., :3]
    N, H, W, _ = dy.shape
    d = draws(table, policy, H)
    b, s, k = colour_factors(table, policy)
    out = np.zeros((N, 3, H, W))
    r, q = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    for n in range(N):
        live, tx, ty = live_mask(d, n, H, mutant)
        g = np.where(live[..., None], dy[n], 0.0)                 # over output pixels
        # g_z[r][q] = g[r - ty][q - tx] where that output pixel exists
        rd, qd = r - ty, q - tx
        ok = (rd >= 0) & (rd < H) & (qd >= 0) & (qd < H)
        gz = np.where(ok[..., None], g[np.clip(rd, 0, H - 1), np.clip(qd, 0, H - 1)], 0.0).transpose(2, 0, 1)   # [3][H][H]
        if policy & COLOR:
            mean = 0.0 if mutant == "adjoint_without_mean" else gz.mean()
            gy = k[n] * gz + (1.0 - k[n]) * mean
            pm = gy.sum(0) / (4.0 if mutant == "channel_mean_over_4" else 3.0)
            gz = s[n] * gy + (1.0 - s[n]) * pm
        out[n] = gz
    return out


# ---- the inputs both suites use -------------------------------------------------------------------------------------------
SHAPES = ((3, 8), (5, 64), (2, 256))       # (N, H)


def make_table(N, H, seed):
    """[N][8] float32 uniforms in [0, 1).  Hand-set rows: row 0 the largest positive shifts and the cutout at offset 0; row 1
    the largest negative shifts and the cutout at offset n_c - 1; row 2 (where there is one) tx = ty = 0.  The colour
    uniforms of every row are random."""
    rng = np.random.RandomState(seed)
    t = rng.random_sample((N, 8)).astype(np.float32)
    t = np.minimum(t, ONE_BELOW)
    t[0, 3:7] = (ONE_BELOW, ONE_BELOW, 0.0, 0.0)
    if N > 1:
        t[1, 3:7] = (0.0, 0.0, ONE_BELOW, ONE_BELOW)
    if N > 2:
        t[2, 3:5] = 0.5
    return t


def make_case(N, H):
    """x in [-1, 1], the table, and a gradient with a mean far from zero (0.5: the adjoint's image-mean term then carries
    weight), all float32."""
    rng = np.random.RandomState(1000 + H)
    x = (rng.random_sample((N, 3, H, H)) * 2.0 - 1.0).astype(np.float32)
    dy = (rng.random_sample((N, H, H, 4)) * 2.0 - 0.5).astype(np.float32)
    return x, make_table(N, H, 2000 + H), dy


# ---- the comparisons both suites use --------------------------------------------------------------------------------------
def max_err(out, ref):
    return float(np.max(np.abs(np.asarray(out, dtype=np.float64) - np.asarray(ref, dtype=np.float64))))


def within(out, ref, tol):
    """The comparison of policies with COLOR: every element within tol of the fp64 reference."""
    return max_err(out, ref) <= tol


def same_bits(out, ref):
    """The comparison of policies without COLOR: out (float32) holds the reference's values bit for bit, zeros as +0."""
    a = np.ascontiguousarray(np.asarray(out, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).astype(np.float32))
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
