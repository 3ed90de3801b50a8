"""numpy float32 restatement of s2i_image_grid_u8 (include/s2i_hip.h): the picture torchvision's
`save_image(images, nrow=8, padding=2, normalize=True)` writes, every operation on np.float32 and rounded on its own.

    lo, hi = min, max over the whole batch (three channels);  d = max(hi - lo, 1e-5)
    v = (x - lo) / d;  q = v * 255;  q = q + 0.5;  clamp to [0, 255];  truncate to uint8
    image k at row (k // xmaps) * (H + padding) + padding, column (k % xmaps) * (W + padding) + padding of a zero canvas,
    xmaps = min(nrow, N), ymaps = ceil(N / xmaps)
"""
import numpy as np

F = np.float32


def grid_shape(N, H, W, nrow=8, padding=2):
    """(rows, columns, xmaps, ymaps) of the grid of N images of H x W pixels."""
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, xmaps, ymaps


def as_nchw3(images, layout):
    """(N, 3, H, W) float32 view of an NCHW batch or of the first three channels of an NHWC one (any strides)."""
    x = np.asarray(images)
    assert x.dtype == np.float32 and x.ndim == 4, (x.dtype, x.shape)
    if layout == "nhwc":
        x = x[..., :3].transpose(0, 3, 1, 2)
    else:
        assert layout == "nchw", layout
        x = x[:, :3]
    assert x.shape[1] == 3, x.shape
    return x


def quantise(x, lo, hi):
    """uint8 of float32 values x for the batch extrema lo, hi: five float32 operations, then the truncation."""
    lo, hi = F(lo), F(hi)
    d = np.maximum(F(hi - lo), F(1e-5))
    v = (x - lo) / d
    q = v * F(255.0)
    q = q + F(0.5)
    q = np.minimum(np.maximum(q, F(0.0)), F(255.0))
    assert v.dtype == np.float32 and q.dtype == np.float32 and d.dtype == np.float32
    return q.astype(np.uint8)


def image_grid_u8(images, nrow=8, padding=2, layout="nchw"):
    """(Hg, Wg, 3) uint8 grid of a float32 batch, NCHW or NHWC (channels beyond the third are not read)."""
    x = as_nchw3(images, layout)
    N, _, H, W = x.shape
    Hg, Wg, xmaps, _ = grid_shape(N, H, W, nrow, padding)
    u8 = quantise(x, x.min(), x.max())
    out = np.zeros((Hg, Wg, 3), np.uint8)
    for k in range(N):
        r = (k // xmaps) * (H + padding) + padding
        c = (k % xmaps) * (W + padding) + padding
        out[r:r + H, c:c + W] = u8[k].transpose(1, 2, 0)
    return out
