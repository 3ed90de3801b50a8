"""The float32 restatement of the snapshot grid (grid_ref.py) against hand-worked cases, against torchvision where it is
installed, and the embedding line of the interpolation strip (speech_to_image.interpolation_embeddings).  No GPU."""
import numpy as np
import pytest
import torch

import grid_ref as G


@pytest.mark.parametrize("N,nrow,xmaps,ymaps", [(1, 8, 1, 1), (5, 8, 5, 1), (8, 8, 8, 1), (11, 8, 8, 2), (23, 10, 10, 3)])
def test_grid_shape_formula(N, nrow, xmaps, ymaps):
    H, W, pad = 6, 10, 2
    Hg, Wg, xm, ym = G.grid_shape(N, H, W, nrow, pad)
    assert (xm, ym) == (xmaps, ymaps)
    assert (Hg, Wg) == (ymaps * (H + pad) + pad, xmaps * (W + pad) + pad)
    x = np.random.default_rng(N).standard_normal((N, 3, H, W)).astype(np.float32)
    assert G.image_grid_u8(x, nrow, pad).shape == (Hg, Wg, 3)


def test_two_images_by_hand():
    """lo = -1, hi = 1, d = 2: -1 -> 0;  -0.5 -> 0.25 * 255 + 0.5 = 64.25 -> 64;  0 -> 127.5 + 0.5 -> 128;
    0.5 -> 191.25 + 0.5 = 191.75 -> 191;  1 -> 255.5, clamped -> 255.  padding 1: a 4 x 7 canvas."""
    img0 = [[[-1, -0.5], [0, 0.5]], [[1, 1], [1, 1]], [[0, 0], [-1, -1]]]
    img1 = [[[0.5, 0.5], [0.5, 0.5]], [[-1, 0], [0, 1]], [[-0.5, -0.5], [1, 1]]]
    x = np.array([img0, img1], np.float32)
    z = (0, 0, 0)
    want = np.array([
        [z, z, z, z, z, z, z],
        [z, (0, 255, 128), (64, 255, 128), z, (191, 0, 64), (191, 128, 64), z],
        [z, (128, 255, 0), (191, 255, 0), z, (191, 128, 255), (191, 255, 255), z],
        [z, z, z, z, z, z, z]], np.uint8)
    np.testing.assert_array_equal(G.image_grid_u8(x, nrow=8, padding=1), want)
    # the same pixels as NHWC4 storage whose fourth channel holds NaN
    nhwc = np.full((2, 2, 2, 4), np.nan, np.float32)
    nhwc[..., :3] = x.transpose(0, 2, 3, 1)
    np.testing.assert_array_equal(G.image_grid_u8(nhwc, nrow=8, padding=1, layout="nhwc"), want)
    # nrow = 1: one image under the other
    col = G.image_grid_u8(x, nrow=1, padding=1)
    assert col.shape == (7, 4, 3)
    np.testing.assert_array_equal(col[1:3, 1:3], want[1:3, 1:3])
    np.testing.assert_array_equal(col[4:6, 1:3], want[1:3, 4:6])


def test_one_pair_for_the_whole_batch():
    """The extrema are taken over the batch, not per image: an image spanning [0, 1] beside one spanning [0, 4]."""
    x = np.zeros((2, 3, 1, 2), np.float32)
    x[0, :, 0, 1] = 1.0
    x[1, :, 0, 1] = 4.0
    g = G.image_grid_u8(x, nrow=8, padding=0)
    assert g.shape == (1, 4, 3)
    assert g[0, :, 0].tolist() == [0, 64, 0, 255]       # 0.25 * 255 + 0.5 = 64.25


def test_constant_batch_is_black():
    x = np.full((3, 3, 4, 5), 0.37, np.float32)
    assert not G.image_grid_u8(x).any()


def test_blank_cells_and_padding_are_zero():
    N, H, W, nrow, pad = 11, 4, 6, 8, 2
    x = (np.random.default_rng(0).random((N, 3, H, W)) + 1.0).astype(np.float32)
    x[0, 0, 0, 0] = 0.0                                      # every other value lies above lo: its byte is >= 1
    g = G.image_grid_u8(x, nrow, pad)
    inside = np.zeros(g.shape[:2], bool)
    for k in range(N):
        r, c = (k // nrow) * (H + pad) + pad, (k % nrow) * (W + pad) + pad
        inside[r:r + H, c:c + W] = True
    assert not g[~inside].any()
    assert (g[inside].reshape(-1) > 0).sum() == N * 3 * H * W - 1
    # the five missing cells of the second row
    assert not g[H + 2 * pad:, 3 * (W + pad):].any()


def test_against_torchvision():
    tv = pytest.importorskip("torchvision.utils")
    rng = np.random.default_rng(5)
    for N, H, W, nrow, pad in ((1, 4, 4, 8, 2), (5, 6, 10, 8, 2), (11, 16, 16, 8, 2), (23, 8, 8, 10, 0)):
        x = (rng.standard_normal((N, 3, H, W)) * 1.5).astype(np.float32)
        grid = tv.make_grid(torch.from_numpy(x), nrow=nrow, padding=pad, normalize=True)
        want = grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
        np.testing.assert_array_equal(G.image_grid_u8(x, nrow, pad), want)


def test_interpolation_embeddings():
    from speech_to_image_translation_without_text_amd.speech_to_image import interpolation_embeddings
    a, b = torch.tensor([4.0, 8.0, -2.0]), torch.tensor([0.0, -4.0, 2.0])
    rows = interpolation_embeddings(a, b, 4)
    assert rows.shape == (5, 3)
    assert rows.tolist() == [[0, -4, 2], [1, -1, 1], [2, 2, 0], [3, 5, -1], [4, 8, -2]]
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(1024, generator=g), torch.randn(1, 1024, generator=g)
    for steps in (1, 3, 10):
        rows = interpolation_embeddings(a, b, steps)
        assert rows.shape == (steps + 1, 1024) and rows.dtype == torch.float32
        assert torch.equal(rows[0], b[0]) and torch.equal(rows[-1], a)
        i = steps // 2 + 1 if steps > 1 else 1
        alpha = torch.tensor(float(i)) / steps
        assert torch.equal(rows[i], a * alpha + b[0] * (1 - alpha))
    with pytest.raises(ValueError):
        interpolation_embeddings(a, b, 0)
