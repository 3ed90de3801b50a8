"""Inception-v3 scorer on the MI355X kernels: the network behind the reference's INCEPTION_V3
(StackGAN_v2/model.py:17-109), i.e. torchvision's `Inception3` in eval mode with `transform_input=False`, preceded by the
reference's input stage and followed by its softmax.

What runs:
  * the weights come from a LOCAL torchvision-layout state_dict (e.g. inception_v3_google-1a9a5a14.pth); nothing is
    downloaded and torchvision is not needed;
  * every BasicConv2d (bias-free conv, BatchNorm(eps=0.001), ReLU) is ONE s2i_conv2d_forward launch: the BatchNorm is
    folded into the weights and a per-channel bias, the ReLU is the epilogue;
  * the branches of an Inception block write their channel slices of the block's output directly (no torch.cat);
  * input stage (x*0.5+0.5, ImageNet mean / std, bilinear resize to 299, NHWC), pools and softmax are one kernel each;
  * the fc (2048 -> 1000) is a 1x1 s2i_conv2d_forward over the pool3 rows.
fp32 throughout.  Images are processed in chunks of at most MAX_BATCH so every tensor stays inside 32-bit offsets.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import POOL_AVG3S1, POOL_GLOBAL, POOL_MAX3S2, check, ptr, stream

BN_EPS = 1e-3
SIZE = 299
MAX_BATCH = 48
POOL3, CLASSES = 2048, 1000


def _geom(k, s=1, p=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (p, p) if isinstance(p, int) else p
    return kh, kw, s, s, ph, pw


def architecture(aux_logits=True):
    """Ordered {BasicConv2d name: (cin, cout, kh, kw, sh, sw, ph, pw)} of torchvision's Inception3, plus 'fc'
    (2048 -> 1000 with bias) and, with aux_logits, the AuxLogits head (its fc under 'AuxLogits.fc')."""
    L = collections.OrderedDict()

    def bc(name, cin, cout, k, s=1, p=0):
        L[name] = (cin, cout) + _geom(k, s, p)

    bc("Conv2d_1a_3x3", 3, 32, 3, 2)
    bc("Conv2d_2a_3x3", 32, 32, 3)
    bc("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    bc("Conv2d_3b_1x1", 64, 80, 1)
    bc("Conv2d_4a_3x3", 80, 192, 3)
    for name, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        bc(name + ".branch1x1", cin, 64, 1)
        bc(name + ".branch5x5_1", cin, 48, 1)
        bc(name + ".branch5x5_2", 48, 64, 5, 1, 2)
        bc(name + ".branch3x3dbl_1", cin, 64, 1)
        bc(name + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        bc(name + ".branch3x3dbl_3", 96, 96, 3, 1, 1)
        bc(name + ".branch_pool", cin, pf, 1)
    bc("Mixed_6a.branch3x3", 288, 384, 3, 2)
    bc("Mixed_6a.branch3x3dbl_1", 288, 64, 1)
    bc("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    bc("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        bc(name + ".branch1x1", 768, 192, 1)
        bc(name + ".branch7x7_1", 768, c7, 1)
        bc(name + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        bc(name + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        bc(name + ".branch7x7dbl_1", 768, c7, 1)
        bc(name + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        bc(name + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        bc(name + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        bc(name + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        bc(name + ".branch_pool", 768, 192, 1)
    if aux_logits:
        bc("AuxLogits.conv0", 768, 128, 1)
        bc("AuxLogits.conv1", 128, 768, 5)
    bc("Mixed_7a.branch3x3_1", 768, 192, 1)
    bc("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    bc("Mixed_7a.branch7x7x3_1", 768, 192, 1)
    bc("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    bc("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    bc("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        bc(name + ".branch1x1", cin, 320, 1)
        bc(name + ".branch3x3_1", cin, 384, 1)
        bc(name + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        bc(name + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        bc(name + ".branch3x3dbl_1", cin, 448, 1)
        bc(name + ".branch3x3dbl_2", 448, 384, 3, 1, 1)
        bc(name + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        bc(name + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        bc(name + ".branch_pool", cin, 192, 1)
    return L


def state_dict_shapes(aux_logits=True, num_batches_tracked=True):
    """{key: shape} of torchvision's Inception3 state_dict (aux_logits=True is what the pretrained file holds)."""
    S = collections.OrderedDict()
    for name, (cin, cout, kh, kw, *_rest) in architecture(aux_logits).items():
        S[name + ".conv.weight"] = (cout, cin, kh, kw)
        for b in ("weight", "bias", "running_mean", "running_var"):
            S["%s.bn.%s" % (name, b)] = (cout,)
        if num_batches_tracked:
            S[name + ".bn.num_batches_tracked"] = ()
    if aux_logits:
        S["AuxLogits.fc.weight"] = (CLASSES, 768)
        S["AuxLogits.fc.bias"] = (CLASSES,)
    S["fc.weight"] = (CLASSES, POOL3)
    S["fc.bias"] = (CLASSES,)
    return S


def parameter_count(aux_logits=True):
    """Learnable parameters (BatchNorm running statistics excluded), torchvision's published figure for aux_logits=True."""
    n = 0
    for k, shp in state_dict_shapes(aux_logits, False).items():
        if "running_" in k:
            continue
        c = 1
        for s in shp:
            c *= s
        n += c
    return n


def check_state_dict(sd):
    """Raise ValueError unless `sd` holds every key of the eval network with its shape.  AuxLogits.* keys are ignored
    (the eval forward never uses them); num_batches_tracked is optional; any other key is an error."""
    want = state_dict_shapes(aux_logits=False, num_batches_tracked=False)
    missing = [k for k in want if k not in sd]
    if missing:
        raise ValueError("Inception-v3 weights lack %d keys, e.g. %s" % (len(missing), missing[:4]))
    bad = ["%s: %s, expected %s" % (k, tuple(sd[k].shape), s) for k, s in want.items() if tuple(sd[k].shape) != s]
    if bad:
        raise ValueError("Inception-v3 weights of the wrong shape: %s" % "; ".join(bad[:4]))
    extra = [k for k in sd if k not in want and not k.startswith("AuxLogits.") and not k.endswith(".num_batches_tracked")]
    if extra:
        raise ValueError("unexpected keys in the Inception-v3 weights: %s" % extra[:4])


def fold(sd):
    """{name: (w OIHW, bias)} float64 with every eval BatchNorm folded into its convolution, plus 'fc'."""
    out = collections.OrderedDict()
    for name in architecture(aux_logits=False):
        w = sd[name + ".conv.weight"].double()
        g, b = sd[name + ".bn.weight"].double(), sd[name + ".bn.bias"].double()
        m, v = sd[name + ".bn.running_mean"].double(), sd[name + ".bn.running_var"].double()
        s = g / torch.sqrt(v + BN_EPS)
        out[name] = (w * s[:, None, None, None], b - m * s)
    out["fc"] = (sd["fc.weight"].double()[:, :, None, None], sd["fc.bias"].double())
    return out


def pack_weight(w, cin_pad=None):
    """OIHW -> the packed layout of s2i_conv2d_forward: P[(ky*kw + kx)*C + c][Np] (Np = O rounded up to 4)."""
    O, I, KH, KW = w.shape
    C = cin_pad or I
    Np = (O + 3) // 4 * 4
    P = torch.zeros(KH, KW, C, Np, dtype=torch.float32, device=w.device)
    P[:, :, :I, :O] = w.permute(2, 3, 1, 0).float()
    return P.reshape(KH * KW * C, Np).contiguous()


class InceptionNet:
    """The folded, packed network on one device.  `run(images, softmax_out, pool3_out)` is the whole scorer."""

    def __init__(self, state_dict, device):
        check_state_dict(state_dict)
        self.device = torch.device(device)
        self.arch = architecture(aux_logits=False)
        self.layers = {}
        for name, (w, b) in fold(state_dict).items():
            cin_pad = 4 if name == "Conv2d_1a_3x3" else None       # the image is NHWC4
            self.layers[name] = (pack_weight(w.to(self.device), cin_pad), b.float().to(self.device).contiguous())
        self._descs = {}

    # -- launches -----------------------------------------------------------------------------------------------------
    def conv(self, name, x, B, H, W, y=None, coff=0, relu=True, ldx=None):
        """BasicConv2d `name` on the NHWC tensor x (B, H, W, ldx) -> y (B, Ho, Wo, ldy) at channel offset coff."""
        ldx = ldx or x.shape[-1]
        if name == "fc":
            cin, cout, kh, kw, sh, sw, ph, pw = POOL3, CLASSES, 1, 1, 1, 1, 0, 0
        else:
            cin, cout, kh, kw, sh, sw, ph, pw = self.arch[name]
        if name == "Conv2d_1a_3x3":
            cin = 4
        Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        if y is None:
            y = torch.empty(B, Ho, Wo, cout, device=self.device)
        key = (name, B, H, W, ldx, y.shape[-1], coff, relu)
        d = self._descs.get(key)
        if d is None:
            d = _lib.Conv2dDesc(B, H, W, cin, ldx, cout, kh, kw, sh, sw, ph, pw, Ho, Wo, y.shape[-1], coff,
                                int(relu), 0)
            self._descs[key] = d
        w, b = self.layers[name]
        check(_lib.load().s2i_conv2d_forward(ctypes.byref(d), ptr(x), ptr(w), ptr(b), ptr(y), stream()),
              "s2i_conv2d_forward(%s)" % name)
        return y, Ho, Wo

    def pool(self, mode, x, B, H, W, C, y=None, coff=0):
        if mode == POOL_MAX3S2:
            Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        elif mode == POOL_AVG3S1:
            Ho, Wo = H, W
        else:
            Ho, Wo = 1, 1
        if y is None:
            y = torch.empty(B, Ho, Wo, C, device=self.device)
        check(_lib.load().s2i_pool2d(mode, ptr(x), B, H, W, C, x.shape[-1], ptr(y), y.shape[-1], coff, stream()),
              "s2i_pool2d")
        return y, Ho, Wo

    # -- blocks of torchvision's Inception3 -----------------------------------------------------------------------------
    def _block_a(self, n, x, B, H, W, pf):
        out = torch.empty(B, H, W, 224 + pf, device=self.device)
        self.conv(n + ".branch1x1", x, B, H, W, out, 0)
        t, _, _ = self.conv(n + ".branch5x5_1", x, B, H, W)
        self.conv(n + ".branch5x5_2", t, B, H, W, out, 64)
        t, _, _ = self.conv(n + ".branch3x3dbl_1", x, B, H, W)
        t, _, _ = self.conv(n + ".branch3x3dbl_2", t, B, H, W)
        self.conv(n + ".branch3x3dbl_3", t, B, H, W, out, 128)
        p, _, _ = self.pool(POOL_AVG3S1, x, B, H, W, x.shape[-1])
        self.conv(n + ".branch_pool", p, B, H, W, out, 224)
        return out

    def _block_b(self, n, x, B, H, W):
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = torch.empty(B, Ho, Wo, 384 + 96 + x.shape[-1], device=self.device)
        self.conv(n + ".branch3x3", x, B, H, W, out, 0)
        t, _, _ = self.conv(n + ".branch3x3dbl_1", x, B, H, W)
        t, _, _ = self.conv(n + ".branch3x3dbl_2", t, B, H, W)
        self.conv(n + ".branch3x3dbl_3", t, B, H, W, out, 384)
        self.pool(POOL_MAX3S2, x, B, H, W, x.shape[-1], out, 480)
        return out, Ho, Wo

    def _block_c(self, n, x, B, H, W):
        out = torch.empty(B, H, W, 768, device=self.device)
        self.conv(n + ".branch1x1", x, B, H, W, out, 0)
        t, _, _ = self.conv(n + ".branch7x7_1", x, B, H, W)
        t, _, _ = self.conv(n + ".branch7x7_2", t, B, H, W)
        self.conv(n + ".branch7x7_3", t, B, H, W, out, 192)
        t, _, _ = self.conv(n + ".branch7x7dbl_1", x, B, H, W)
        for i in (2, 3, 4):
            t, _, _ = self.conv(n + ".branch7x7dbl_%d" % i, t, B, H, W)
        self.conv(n + ".branch7x7dbl_5", t, B, H, W, out, 384)
        p, _, _ = self.pool(POOL_AVG3S1, x, B, H, W, 768)
        self.conv(n + ".branch_pool", p, B, H, W, out, 576)
        return out

    def _block_d(self, n, x, B, H, W):
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = torch.empty(B, Ho, Wo, 320 + 192 + x.shape[-1], device=self.device)
        t, _, _ = self.conv(n + ".branch3x3_1", x, B, H, W)
        self.conv(n + ".branch3x3_2", t, B, H, W, out, 0)
        t, _, _ = self.conv(n + ".branch7x7x3_1", x, B, H, W)
        t, _, _ = self.conv(n + ".branch7x7x3_2", t, B, H, W)
        t, _, _ = self.conv(n + ".branch7x7x3_3", t, B, H, W)
        self.conv(n + ".branch7x7x3_4", t, B, H, W, out, 320)
        self.pool(POOL_MAX3S2, x, B, H, W, x.shape[-1], out, 512)
        return out, Ho, Wo

    def _block_e(self, n, x, B, H, W):
        out = torch.empty(B, H, W, 2048, device=self.device)
        self.conv(n + ".branch1x1", x, B, H, W, out, 0)
        t, _, _ = self.conv(n + ".branch3x3_1", x, B, H, W)
        self.conv(n + ".branch3x3_2a", t, B, H, W, out, 320)
        self.conv(n + ".branch3x3_2b", t, B, H, W, out, 704)
        t, _, _ = self.conv(n + ".branch3x3dbl_1", x, B, H, W)
        t, _, _ = self.conv(n + ".branch3x3dbl_2", t, B, H, W)
        self.conv(n + ".branch3x3dbl_3a", t, B, H, W, out, 1088)
        self.conv(n + ".branch3x3dbl_3b", t, B, H, W, out, 1472)
        p, _, _ = self.pool(POOL_AVG3S1, x, B, H, W, x.shape[-1])
        self.conv(n + ".branch_pool", p, B, H, W, out, 1856)
        return out

    def features(self, x, B, pool3):
        """MY_Inception3.forward (model.py:19-77, eval) on the prepared NHWC4 299 x 299 batch: pool3 (B, 2048) rows are
        written into `pool3` (row stride pool3.stride(0)); returns the (B, 1000) logits."""
        H = W = SIZE
        x, H, W = self.conv("Conv2d_1a_3x3", x, B, H, W)
        x, H, W = self.conv("Conv2d_2a_3x3", x, B, H, W)
        x, H, W = self.conv("Conv2d_2b_3x3", x, B, H, W)
        x, H, W = self.pool(POOL_MAX3S2, x, B, H, W, 64)
        x, H, W = self.conv("Conv2d_3b_1x1", x, B, H, W)
        x, H, W = self.conv("Conv2d_4a_3x3", x, B, H, W)
        x, H, W = self.pool(POOL_MAX3S2, x, B, H, W, 192)
        for n, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
            x = self._block_a(n, x, B, H, W, pf)
        x, H, W = self._block_b("Mixed_6a", x, B, H, W)
        for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self._block_c(n, x, B, H, W)
        x, H, W = self._block_d("Mixed_7a", x, B, H, W)
        for n in ("Mixed_7b", "Mixed_7c"):
            x = self._block_e(n, x, B, H, W)
        check(_lib.load().s2i_pool2d(POOL_GLOBAL, ptr(x), B, H, W, POOL3, x.shape[-1], ptr(pool3), pool3.stride(0), 0,
                                     stream()), "s2i_pool2d")
        logits, _, _ = self.conv("fc", pool3, B, 1, 1, relu=False, ldx=pool3.stride(0))
        return logits.reshape(B, CLASSES)

    def prep(self, img, y):
        """One image tensor (B, 3, h, w) fp32, any strides (an NCHW view of NHWC4 storage or plain NCHW) -> y NHWC4."""
        if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
            raise ValueError("INCEPTION_V3 takes (B, 3, H, W) float32 images, got %s %s" % (tuple(img.shape), img.dtype))
        sb, sc, sh, sw = img.stride()
        check(_lib.load().s2i_inception_prep(ptr(img), img.shape[0], img.shape[2], img.shape[3], sb, sc, sh, sw, ptr(y),
                                             SIZE, 4, stream()), "s2i_inception_prep")

    def run(self, images, softmax_out, pool3_out):
        """Score the concatenation of `images` (a list of (B_i, 3, h, w) tensors) into softmax_out (sum B_i, 1000) and
        pool3_out (sum B_i, 2048), both fp32 row-major on the device (any row-contiguous slices)."""
        segs, total = [], 0
        for t in images:
            segs.append((t, total))
            total += t.shape[0]
        for o, cols in ((softmax_out, CLASSES), (pool3_out, POOL3)):
            if (o.dim() != 2 or tuple(o.shape) != (total, cols) or o.stride(1) != 1 or o.dtype != torch.float32
                    or o.device != self.device):
                raise ValueError("outputs must be (%d, %d) fp32 rows on %s" % (total, cols, self.device))
        lib = _lib.load()
        for c0 in range(0, total, MAX_BATCH):
            c1 = min(total, c0 + MAX_BATCH)
            B = c1 - c0
            x = torch.empty(B, SIZE, SIZE, 4, device=self.device)
            for t, s0 in segs:
                lo, hi = max(c0, s0), min(c1, s0 + t.shape[0])
                if lo < hi:
                    self.prep(t[lo - s0:hi - s0], x[lo - c0:hi - c0])
            logits = self.features(x, B, pool3_out[c0:c1])
            check(lib.s2i_softmax_rows(ptr(logits), B, CLASSES, CLASSES, ptr(softmax_out[c0:c1]), softmax_out.stride(0),
                                       stream()), "s2i_softmax_rows")
        return softmax_out, pool3_out
