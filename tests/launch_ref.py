"""Plain fp64 restatement of the convolution launches of the train step (tests/test_step_launches_gpu.py).

A launch of ops.conv_any / conv_raw / wgrad_any / wgrad_raw is identified by its raw arguments (kind, wmode, flip, swap,
fold); the fixed tables of ops (_KIND for the forward, _DGRAD for the input gradient, ops._wgrad for the weight gradient)
map them back to the layer operation they compute:

  fwd    y  = conv(x, W)             of a k1 / k3s1 / k4s2 / up layer (up = nearest x2, then 3x3 pad 1)
  dgrad  dx = d conv(x, W) / dx . dy
  wgrad  dW = d conv(x, W) / dW . dy
  matmul y  = x . P or x . P^T        K1 launches whose second operand is a plain matrix (the class-aware loss)

Everything here is NCHW / OIHW float64 and uses only stock torch tensor ops (conv2d, conv_transpose2d, unfold, einsum);
tests/test_launch_ref.py checks it against autograd through stock torch modules."""
import torch
import torch.nn.functional as F

from speech_to_image_translation_without_text_amd import ops
from speech_to_image_translation_without_text_amd._lib import ACT_LRELU, ACT_NONE, ACT_TANH, CONV_K4S2

LAYERS = ("k1", "k3s1", "k4s2", "up")


def layer_op(rec):
    """(operation, layer) of a census record (see tests/step_launches.json)."""
    if rec["fn"] in ("conv_any", "conv_raw"):
        if rec["w"]["oihw"] is None:
            return "matmul", "k1"
        if rec["wmode"] == 0:
            return "fwd", {v: k for k, v in ops._KIND.items()}[rec["kind"]]
        return "dgrad", {v: k for k, v in ops._DGRAD.items()}[(rec["kind"], rec["flip"])]
    if rec["swap"]:
        # ops._wgrad: the up layer's gradient gathers dy by the k4s2 pattern against the layer input
        assert rec["kind"] == CONV_K4S2 and rec["fold"] == 1, rec
        return "wgrad", "up"
    assert rec["fold"] == 0, rec
    return "wgrad", {v: k for k, v in ops._KIND.items()}[rec["kind"]]


def pack_mode(op, layer):
    return ops.PACK_UPFOLD if (layer == "up" and op in ("fwd", "dgrad")) else ops.PACK_PLAIN


def _w4(w):
    return w.view(w.shape[0], w.shape[1], 1, 1) if w.dim() == 2 else w


def _up(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def fwd(layer, x, w):
    """x (B, I, H, W), w (O, I, kh, kw) or (O, I) -> (B, O, Ho, Wo)."""
    w = _w4(w)
    if layer == "k1":
        return torch.einsum("bihw,oi->bohw", x, w[:, :, 0, 0])
    if layer == "k3s1":
        return F.conv2d(x, w, padding=1)
    if layer == "k4s2":
        return F.conv2d(x, w, stride=2, padding=1)
    return F.conv2d(_up(x), w, padding=1)


def dgrad(layer, dy, w):
    """dy (B, O, Ho, Wo) -> dx (B, I, H, W)."""
    w = _w4(w)
    if layer == "k1":
        return torch.einsum("bohw,oi->bihw", dy, w[:, :, 0, 0])
    if layer == "k3s1":
        return F.conv_transpose2d(dy, w, padding=1)
    if layer == "k4s2":
        return F.conv_transpose2d(dy, w, stride=2, padding=1)
    z = F.conv_transpose2d(dy, w, padding=1)          # gradient w.r.t. the upsampled map
    B, I, H2, W2 = z.shape
    return z.view(B, I, H2 // 2, 2, W2 // 2, 2).sum((3, 5))


def wgrad(layer, x, dy, kh):
    """x (B, I, H, W), dy (B, O, Ho, Wo) -> dW (O, I, kh, kh)."""
    B, O = dy.shape[:2]
    I = x.shape[1]
    if layer == "k1":
        return torch.einsum("bohw,bihw->oi", dy, x).view(O, I, 1, 1)
    if layer == "k3s1":
        cols = F.unfold(x, 3, padding=1)
    elif layer == "k4s2":
        cols = F.unfold(x, 4, padding=1, stride=2)
    else:
        cols = F.unfold(_up(x), 3, padding=1)
    return torch.einsum("bol,bkl->ok", dy.flatten(2), cols).view(O, I, kh, kh)


def border_class(Ho, Wo, device=None):
    """cls = 3 * (top | middle | bottom) + (left | middle | right) of each output pixel (include/s2i_hip.h,
    s2i_cvec_bias_table): (Ho, Wo) int64."""
    def band(n):
        b = torch.ones(n, dtype=torch.long, device=device)
        b[0] = 0
        b[-1] = 2
        return b
    return 3 * band(Ho).view(Ho, 1) + band(Wo).view(1, Wo)


def add_class_bias(y, table):
    """y (B, N, Ho, Wo) + table[b, cls(oy, ox), n]; table (B, 9, N)."""
    B, N, Ho, Wo = y.shape
    cls = border_class(Ho, Wo, y.device).view(-1)
    return y + table[:, cls, :].permute(0, 2, 1).reshape(B, N, Ho, Wo)


def act(y, a):
    if a == ACT_NONE:
        return y
    if a == ACT_LRELU:
        return F.leaky_relu(y, 0.2)
    if a == ACT_TANH:
        return torch.tanh(y)
    raise ValueError("activation %d" % a)


def group_stats(y, groups):
    """Per-group column sums and sums of squares of y (B, N, Ho, Wo): (2, groups, N).  The groups are equal, consecutive
    runs of images (the stacked real / wrong / fake batches)."""
    B, N = y.shape[:2]
    g = max(groups, 1)
    yg = y.reshape(g, B // g, N, -1)
    return torch.stack((yg.sum((1, 3)), (yg * yg).sum((1, 3))))


def pad_channels(y, N):
    """(B, C, ...) -> (B, N, ...) with zero channels appended (or the first N kept)."""
    if y.shape[1] >= N:
        return y[:, :N]
    return torch.cat((y, y.new_zeros((y.shape[0], N - y.shape[1]) + tuple(y.shape[2:]))), 1)
