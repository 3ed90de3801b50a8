"""BVLC GoogLeNet image features on the MI355X kernels: the 10-view pool5/7x7_s1 features of
Audio_to_Image/prepare_image_feature.py:86-118 (Caffe's deploy network, its Transformer and the ten crops), without Caffe.

What runs:
  * the weights come from a LOCAL `bvlc_googlenet.caffemodel`, read here by a small protobuf wire-format reader (no
    generated caffe_pb2, no google.protobuf); an in-memory {layer: (w, b)} dict works as well;
  * the input stage (bilinear resize to 227, RGB -> BGR, mean, ten 224 x 224 views) is one kernel over a ragged batch of
    uint8 HWC images (s2i_googlenet_prep);
  * every convolution is ONE s2i_conv2d_forward launch with bias and ReLU in the epilogue; the branches of an inception
    block write their channel slices of the block's output directly (no torch.cat);
  * pool1 + norm1 and norm2 + pool2 are one launch each (s2i_lrn_maxpool3), the other max pools are s2i_maxpool3 and
    pool5/7x7_s1 is s2i_pool2d(S2I_POOL_GLOBAL) on the 7 x 7 map.
fp32 throughout.  Images run in chunks of at most MAX_BATCH (10 views each) so every tensor stays inside the 32-bit
offsets of s2i_conv2d_forward.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LRN_THEN_POOL, POOL_GLOBAL, POOL_THEN_LRN, check, ptr, stream
from .inception import pack_weight

FEATURE_LAYER = "pool5/7x7_s1"
FEATURES = 1024
VIEWS = 10
VIEW = 224
SIZE = 227
MAX_BATCH = 48
# ilsvrc_2012_mean.npy averaged over H and W (prepare_image_feature.py:101), BGR
MEAN_BGR = (104.00698793, 116.66876762, 122.67891434)
LRN_SIZE, LRN_ALPHA, LRN_BETA, LRN_K = 5, 1e-4, 0.75, 1.0

# s2i_conv2d_forward addresses every tensor with 32-bit byte offsets below this bound (conv2d_validate, s2i_conv2d.hip);
# the largest tensor of a chunk is conv1/7x7_s2's output, (10 B, 112, 112, 64) fp32
CONV2D_BYTE_LIMIT = 0x7FFF0000
assert MAX_BATCH * VIEWS * 112 * 112 * 64 * 4 < CONV2D_BYTE_LIMIT

# inception blocks: (name, 1x1, 3x3 reduce, 3x3, 5x5 reduce, 5x5, pool_proj)
BLOCKS = (
    ("inception_3a", 64, 96, 128, 16, 32, 32),
    ("inception_3b", 128, 128, 192, 32, 96, 64),
    ("inception_4a", 192, 96, 208, 16, 48, 64),
    ("inception_4b", 160, 112, 224, 24, 64, 64),
    ("inception_4c", 128, 128, 256, 24, 64, 64),
    ("inception_4d", 112, 144, 288, 32, 64, 64),
    ("inception_4e", 256, 160, 320, 32, 128, 128),
    ("inception_5a", 256, 160, 320, 32, 128, 128),
    ("inception_5b", 384, 192, 384, 48, 128, 128),
)
# a stride-2 max pool follows these blocks
POOL_AFTER = {"inception_3b": "pool3/3x3_s2", "inception_4e": "pool4/3x3_s2"}


def block_width(block):
    _, n1, _, n3, _, n5, npp = block
    return n1 + n3 + n5 + npp


def architecture():
    """Ordered {Caffe conv layer name: (cin, cout, k, stride, pad)} of the deploy network up to pool5/7x7_s1."""
    L = collections.OrderedDict()
    L["conv1/7x7_s2"] = (3, 64, 7, 2, 3)
    L["conv2/3x3_reduce"] = (64, 64, 1, 1, 0)
    L["conv2/3x3"] = (64, 192, 3, 1, 1)
    cin = 192
    for blk in BLOCKS:
        n, n1, r3, n3, r5, n5, npp = blk
        L[n + "/1x1"] = (cin, n1, 1, 1, 0)
        L[n + "/3x3_reduce"] = (cin, r3, 1, 1, 0)
        L[n + "/3x3"] = (r3, n3, 3, 1, 1)
        L[n + "/5x5_reduce"] = (cin, r5, 1, 1, 0)
        L[n + "/5x5"] = (r5, n5, 5, 1, 2)
        L[n + "/pool_proj"] = (cin, npp, 1, 1, 0)
        cin = block_width(blk)
    return L


def ceil_pool(n, k=3, s=2):
    """Caffe's (and F.max_pool2d(ceil_mode=True)'s) output extent of an unpadded k x k, stride-s pool."""
    return -(-(n - k) // s) + 1


def map_sizes(size=VIEW):
    """Spatial extent after conv1, pool1, pool2, pool3, pool4 and pool5."""
    h = (size + 2 * 3 - 7) // 2 + 1
    out = [h]
    for _ in range(4):
        h = ceil_pool(h)
        out.append(h)
    out.append(1)
    return out


def weight_shapes():
    """{layer: [(O, I, k, k), (O,)]} the feature network needs."""
    return collections.OrderedDict((n, [(o, i, k, k), (o,)]) for n, (i, o, k, _s, _p) in architecture().items())


def parameter_count():
    return sum(int(np.prod(w)) + b[0] for w, b in weight_shapes().values())


def layer_extent(name, size=VIEW):
    """Output extent of convolution `name`."""
    sizes = map_sizes(size)
    if name == "conv1/7x7_s2":
        return sizes[0]
    if name.startswith("conv2"):
        return sizes[1]
    return sizes[{"3": 2, "4": 3, "5": 4}[name[len("inception_")]]]


def flops_per_view(size=VIEW):
    """Multiply-adds x 2 of the convolutions for one view (pools and LRN excluded)."""
    total = 0
    for n, (i, o, k, _s, _p) in architecture().items():
        hw = layer_extent(n, size)
        total += 2 * hw * hw * o * i * k * k
    return total


# ---- caffemodel reader (protobuf wire format) -------------------------------------------------------------------------
class CaffemodelError(ValueError):
    pass


def _varint(buf, pos, end):
    result, shift = 0, 0
    while True:
        if pos >= end:
            raise CaffemodelError("truncated caffemodel: varint runs past the end of its message")
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, pos
        shift += 7
        if shift > 63:
            raise CaffemodelError("corrupt caffemodel: varint longer than 10 bytes")


def _fields(buf, pos, end):
    """Yield (field number, wire type, value) of one message: value is an int (varint / fixed), or a (start, stop) byte
    range for length-delimited fields.  Groups are skipped."""
    while pos < end:
        key, pos = _varint(buf, pos, end)
        fn, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos, end)
        elif wt == 1:
            if pos + 8 > end:
                raise CaffemodelError("truncated caffemodel: fixed64 field %d" % fn)
            v, pos = (pos, pos + 8), pos + 8
        elif wt == 2:
            n, pos = _varint(buf, pos, end)
            if pos + n > end:
                raise CaffemodelError("truncated caffemodel: field %d claims %d bytes, %d remain" % (fn, n, end - pos))
            v, pos = (pos, pos + n), pos + n
        elif wt == 5:
            if pos + 4 > end:
                raise CaffemodelError("truncated caffemodel: fixed32 field %d" % fn)
            v, pos = (pos, pos + 4), pos + 4
        elif wt == 3:
            depth = 1
            while depth:
                if pos >= end:
                    raise CaffemodelError("truncated caffemodel: unterminated group %d" % fn)
                k2, pos = _varint(buf, pos, end)
                w2 = k2 & 7
                if w2 == 3:
                    depth += 1
                elif w2 == 4:
                    depth -= 1
                elif w2 == 0:
                    _, pos = _varint(buf, pos, end)
                elif w2 == 1:
                    pos += 8
                elif w2 == 5:
                    pos += 4
                elif w2 == 2:
                    n, pos = _varint(buf, pos, end)
                    pos += n
                else:
                    raise CaffemodelError("corrupt caffemodel: wire type %d" % w2)
            continue
        else:
            raise CaffemodelError("corrupt caffemodel: wire type %d at byte %d" % (wt, pos))
        yield fn, wt, v
    if pos != end:
        raise CaffemodelError("truncated caffemodel: a field runs past the end of its message")


def _blob(buf, start, end):
    """BlobProto -> float32 ndarray.  data = 5 (packed or not), double_data = 8; shape = 7 (BlobShape.dim = 1) or the
    legacy num / channels / height / width = 1..4."""
    data, ddata, dims, legacy = [], [], None, {}
    for fn, wt, v in _fields(buf, start, end):
        if fn == 5:
            if wt == 2:
                if (v[1] - v[0]) % 4:
                    raise CaffemodelError("corrupt caffemodel: packed float data of %d bytes" % (v[1] - v[0]))
                data.append(np.frombuffer(buf[v[0]:v[1]], dtype="<f4"))
            elif wt == 5:
                data.append(np.frombuffer(buf[v[0]:v[1]], dtype="<f4"))
        elif fn == 8:
            if wt == 2:
                ddata.append(np.frombuffer(buf[v[0]:v[1]], dtype="<f8"))
            elif wt == 1:
                ddata.append(np.frombuffer(buf[v[0]:v[1]], dtype="<f8"))
        elif fn == 7 and wt == 2:
            dims = []
            for f2, w2, d in _fields(buf, v[0], v[1]):
                if f2 != 1:
                    continue
                if w2 == 0:
                    dims.append(d)
                elif w2 == 2:
                    p = d[0]
                    while p < d[1]:
                        x, p = _varint(buf, p, d[1])
                        dims.append(x)
        elif fn in (1, 2, 3, 4) and wt == 0:
            legacy[fn] = v
    arr = np.concatenate(data) if data else (np.concatenate(ddata) if ddata else np.zeros(0, np.float64))
    if dims is None:
        dims = [legacy.get(i, 1 if legacy else 0) for i in (1, 2, 3, 4)] if legacy else [arr.size]
    shape = tuple(int(d) for d in dims)
    if int(np.prod(shape)) != arr.size:
        raise CaffemodelError("corrupt caffemodel: blob of shape %s holds %d values" % (shape, arr.size))
    return arr.astype(np.float32).reshape(shape)


def _is_head(name):
    return name.startswith("loss1/") or name.startswith("loss2/") or name == "loss3/classifier"


def parse_caffemodel(data):
    """NetParameter bytes -> {layer name: [blob ndarray, ...]} of every layer with blobs except the heads loss1/*,
    loss2/* and loss3/classifier.  Reads `layer` (100, LayerParameter: name 1, blobs 7) and the legacy V1 `layers`
    (2, V1LayerParameter: name 4, blobs 6); every other field is skipped."""
    buf = memoryview(data)
    out = collections.OrderedDict()
    for fn, wt, v in _fields(buf, 0, len(buf)):
        if wt != 2 or fn not in (100, 2):
            continue
        name_f, blob_f = (1, 7) if fn == 100 else (4, 6)
        name, blobs = None, []
        for f2, w2, d in _fields(buf, v[0], v[1]):
            if w2 != 2:
                continue
            if f2 == name_f:
                name = bytes(buf[d[0]:d[1]]).decode("utf-8")
            elif f2 == blob_f:
                blobs.append(_blob(buf, d[0], d[1]))
        if not blobs or name is None or _is_head(name):
            continue
        if name in out:
            raise CaffemodelError("caffemodel holds layer %r twice" % name)
        out[name] = blobs
    return out


def load_caffemodel(path):
    """`bvlc_googlenet.caffemodel` -> {layer name: [weight (O, I, kh, kw), bias, ...]} (see parse_caffemodel)."""
    with open(path, "rb") as f:
        return parse_caffemodel(f.read())


def check_weights(weights):
    """Normalise {layer: [w, b]} (ndarrays or tensors; a bias may be (O,) or the legacy (1, 1, 1, O)) to
    {layer: (w float32 (O, I, k, k), b float32 (O,))}.  Raises ValueError naming every missing layer, wrong shape or
    unexpected layer."""
    want = weight_shapes()
    missing = [n for n in want if n not in weights]
    extra = [n for n in weights if n not in want and not _is_head(n)]
    bad, out = [], collections.OrderedDict()
    for n, (ws, bs) in want.items():
        if n not in weights:
            continue
        blobs = list(weights[n])
        if len(blobs) != 2:
            bad.append("%s: %d blobs, expected weight and bias" % (n, len(blobs)))
            continue
        w, b = (np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32) for t in blobs)
        if b.ndim == 4 and b.shape[:3] == (1, 1, 1):
            b = b.reshape(-1)
        if w.shape != ws:
            bad.append("%s weight: %s, expected %s" % (n, w.shape, ws))
        if b.shape != bs:
            bad.append("%s bias: %s, expected %s" % (n, b.shape, bs))
        out[n] = (w, b)
    errs = []
    if missing:
        errs.append("missing %d layers: %s" % (len(missing), ", ".join(missing)))
    if bad:
        errs.append("wrong shapes: %s" % "; ".join(bad))
    if extra:
        errs.append("unexpected layers: %s" % ", ".join(extra))
    if errs:
        raise ValueError("GoogLeNet weights: " + " | ".join(errs))
    return out


# ---- host decoding ---------------------------------------------------------------------------------------------------
def as_rgb(img):
    """uint8 (H, W), (H, W, 1), (H, W, 3) or (H, W, 4) -> contiguous uint8 (H, W, 3): grayscale tiled, alpha dropped
    (PIL's convert("RGB"), as caffe.io.load_image(color=True) does)."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError("images must be uint8, got %s" % a.dtype)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("images must be (H, W), (H, W, 1|3|4), got %s" % (a.shape,))
    if a.shape[2] == 1:
        a = np.repeat(a, 3, axis=2)
    elif a.shape[2] == 4:
        a = a[:, :, :3]
    return np.ascontiguousarray(a)


def read_image(path):
    """PIL decode -> uint8 RGB HWC."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def mean_from_file(path):
    """An `.npy` mean image (3, H, W), BGR -> the per-channel mean the reference uses (.mean(1).mean(1))."""
    m = np.load(path, allow_pickle=False)
    if m.ndim != 3 or m.shape[0] != 3:
        raise ValueError("mean file %s: expected shape (3, H, W), got %s" % (path, m.shape))
    return tuple(float(v) for v in m.astype(np.float64).mean(1).mean(1))


# ---- the network -------------------------------------------------------------------------------------------------------
class GoogLeNetFeatures:
    """The packed network on one device.  `self(images)` -> (B, 10, 1024) float32 CPU tensor of pool5/7x7_s1 features,
    the five crops first, then the five crops of the up-down flipped image (prepare_image_feature.py:88-98)."""

    def __init__(self, weights, device, mean_bgr=MEAN_BGR):
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = load_caffemodel(weights)
        self.device = torch.device(device)
        self.arch = architecture()
        self.mean_bgr = tuple(float(v) for v in mean_bgr)
        self.layers = {}
        for name, (w, b) in check_weights(weights).items():
            w = torch.from_numpy(w).to(self.device)
            self.layers[name] = (pack_weight(w, 4 if name == "conv1/7x7_s2" else None),
                                 torch.from_numpy(b).to(self.device).contiguous())
        self._descs = {}

    # -- launches -----------------------------------------------------------------------------------------------------
    def conv(self, name, x, B, H, W, y=None, coff=0):
        cin, cout, k, s, p = self.arch[name]
        if name == "conv1/7x7_s2":
            cin = 4
        Ho = Wo = (H + 2 * p - k) // s + 1
        if y is None:
            y = torch.empty(B, Ho, Wo, cout, device=self.device)
        key = (name, B, H, x.shape[-1], y.shape[-1], coff)
        d = self._descs.get(key)
        if d is None:
            d = _lib.Conv2dDesc(B, H, W, cin, x.shape[-1], cout, k, k, s, s, p, p, Ho, Wo, y.shape[-1], coff, 1, 0)
            self._descs[key] = d
        w, b = self.layers[name]
        check(_lib.load().s2i_conv2d_forward(ctypes.byref(d), ptr(x), ptr(w), ptr(b), ptr(y), stream()),
              "s2i_conv2d_forward(%s)" % name)
        return y, Ho

    def maxpool(self, x, B, H, stride, pad, y=None, coff=0):
        C = x.shape[-1]
        Ho = H if stride == 1 else ceil_pool(H)
        if y is None:
            y = torch.empty(B, Ho, Ho, C, device=self.device)
        check(_lib.load().s2i_maxpool3(ptr(x), B, H, H, C, C, stride, pad, ptr(y), y.shape[-1], coff, stream()),
              "s2i_maxpool3")
        return y, Ho

    def lrn_pool(self, order, x, B, H):
        C = x.shape[-1]
        Ho = ceil_pool(H)
        y = torch.empty(B, Ho, Ho, C, device=self.device)
        check(_lib.load().s2i_lrn_maxpool3(order, ptr(x), B, H, H, C, C, ptr(y), C, 0, LRN_SIZE, LRN_ALPHA, LRN_BETA,
                                           LRN_K, stream()), "s2i_lrn_maxpool3")
        return y, Ho

    def _inception(self, blk, x, B, H):
        n, n1, _r3, n3, _r5, n5, _npp = blk
        out = torch.empty(B, H, H, block_width(blk), device=self.device)
        self.conv(n + "/1x1", x, B, H, H, out, 0)
        t, _ = self.conv(n + "/3x3_reduce", x, B, H, H)
        self.conv(n + "/3x3", t, B, H, H, out, n1)
        t, _ = self.conv(n + "/5x5_reduce", x, B, H, H)
        self.conv(n + "/5x5", t, B, H, H, out, n1 + n3)
        p, _ = self.maxpool(x, B, H, 1, 1)
        self.conv(n + "/pool_proj", p, B, H, H, out, n1 + n3 + n5)
        return out

    def features(self, x, V, out):
        """The deploy network on the prepared (V, 224, 224, 4) views: pool5/7x7_s1 rows into `out` (V, 1024)."""
        x, H = self.conv("conv1/7x7_s2", x, V, VIEW, VIEW)
        x, H = self.lrn_pool(POOL_THEN_LRN, x, V, H)
        x, H = self.conv("conv2/3x3_reduce", x, V, H, H)
        x, H = self.conv("conv2/3x3", x, V, H, H)
        x, H = self.lrn_pool(LRN_THEN_POOL, x, V, H)
        for blk in BLOCKS:
            x = self._inception(blk, x, V, H)
            if blk[0] in POOL_AFTER:
                x, H = self.maxpool(x, V, H, 2, 0)
        check(_lib.load().s2i_pool2d(POOL_GLOBAL, ptr(x), V, H, H, FEATURES, FEATURES, ptr(out), out.stride(0), 0,
                                     stream()), "s2i_pool2d")
        return out

    def prep(self, images, y):
        """uint8 RGB HWC arrays -> the (10 B, 224, 224, 4) views in y."""
        flat = np.concatenate([im.reshape(-1) for im in images])
        sizes = np.array([im.size for im in images], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        hw = np.array([im.shape[:2] for im in images], dtype=np.int32)
        dev = self.device
        img = torch.from_numpy(flat).to(dev)
        offs_d = torch.from_numpy(offs).to(dev)
        hs = torch.from_numpy(np.ascontiguousarray(hw[:, 0])).to(dev)
        ws = torch.from_numpy(np.ascontiguousarray(hw[:, 1])).to(dev)
        b, g, r = self.mean_bgr
        check(_lib.load().s2i_googlenet_prep(ptr(img), flat.size, ptr(offs_d), ptr(hs), ptr(ws), len(images), b, g, r,
                                             ptr(y), stream()), "s2i_googlenet_prep")
        return img, offs_d, hs, ws      # kept alive by the caller until the stream has read them

    def __call__(self, images, batch_size=MAX_BATCH):
        if not 1 <= batch_size <= MAX_BATCH:
            raise ValueError("batch_size must be in 1..%d" % MAX_BATCH)
        images = [as_rgb(im) for im in images]
        out = torch.empty(len(images), VIEWS, FEATURES)
        for s in range(0, len(images), batch_size):
            chunk = images[s:s + batch_size]
            V = VIEWS * len(chunk)
            x = torch.empty(V, VIEW, VIEW, 4, device=self.device)
            keep = self.prep(chunk, x)
            f = torch.empty(V, FEATURES, device=self.device)
            self.features(x, V, f)
            out[s:s + len(chunk)] = f.reshape(len(chunk), VIEWS, FEATURES).cpu()
            del keep
        return out

    def rows(self, u8, per_view=False):
        """Images that are already on the device: a contiguous uint8 (B, H, W, 3) RGB tensor on self.device -> fp32
        (B, 1024) on the device, the mean of each image's ten views (s2i_time_mean over T = 10: ten fp32 additions in view
        order, then one division), which is what `Gallery(views="mean")` stores for a real image up to that rounding.
        per_view=True: the (B, 10, 1024) views themselves, the values `self(images)` returns for the same pixels.  The
        images run in chunks of at most MAX_BATCH, as in `self(images)`; no pixel or feature is copied to the host."""
        if (not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or u8.shape[0] < 1
                or u8.shape[1] < 1 or u8.shape[2] < 1 or not u8.is_contiguous()):
            raise ValueError("GoogLeNetFeatures.rows takes a contiguous uint8 (B >= 1, H, W, 3) tensor, got %s %s"
                             % (getattr(u8, "dtype", type(u8)), tuple(getattr(u8, "shape", ()))))
        if u8.device != self.device:
            raise _lib.S2IError("GoogLeNetFeatures.rows: the images are on %s, the network on %s: there is no CPU "
                                "fallback and no implicit copy" % (u8.device, self.device))
        B, H, W, _ = u8.shape
        lib = _lib.load()
        b, g, r = self.mean_bgr
        with torch.cuda.device(self.device):
            views = torch.empty(B, VIEWS, FEATURES, device=self.device)
            n = min(B, MAX_BATCH)
            offs = torch.arange(n, dtype=torch.int64, device=self.device) * (H * W * 3)
            hs = torch.full((n,), H, dtype=torch.int32, device=self.device)
            ws = torch.full((n,), W, dtype=torch.int32, device=self.device)
            for s in range(0, B, MAX_BATCH):
                part = u8[s:s + MAX_BATCH]
                nb = part.shape[0]
                x = torch.empty(VIEWS * nb, VIEW, VIEW, 4, device=self.device)
                check(lib.s2i_googlenet_prep(ptr(part), part.numel(), ptr(offs), ptr(hs), ptr(ws), nb, b, g, r, ptr(x),
                                             stream()), "s2i_googlenet_prep")
                self.features(x, VIEWS * nb, views[s:s + nb].view(VIEWS * nb, FEATURES))
            if per_view:
                return views
            out = torch.empty(B, FEATURES, device=self.device)
            check(lib.s2i_time_mean(ptr(views), B, VIEWS, FEATURES, ptr(out), stream()), "s2i_time_mean")
            return out


def flops_per_image():
    return VIEWS * flops_per_view()
