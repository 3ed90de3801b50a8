"""Train-step harness with the surface of the reference's StackGAN_v2/trainer.py, on the MI355X kernels.

Same names and meaning as the reference where a caller can see them:
  weights_init (:65-75), load_params / copy_G_params (:78-85), KL_loss (:54-58),
  class_aware_loss (:298-311), load_network (:162-233), define_optimizers (:236-252),
  save_model (:255-265), condGANTrainer(output_dir, data_loader, imsize, my_dataset_flag,
  local_rank, distributed) with prepare_data / train_Dnet / train_Gnet / train (:318-638).

What is built differently (MI355X-first):
  * every network's parameters, gradients and Adam moments live in ONE flat fp32 buffer each, so the
    optimiser is a single fused kernel per network (Adam, plus the EMA of G), and data-parallel
    training is one RCCL all-reduce per network over xGMI instead of DDP's bucket stream;
  * the three D updates are independent, so D_i's all-reduce overlaps D_{i+1}'s forward/backward;
  * the G update does not compute (and never reduces) the discriminators' weight gradients the
    reference's backward produces and then discards (trainer.py:385 zeroes them);
  * per-replica BatchNorm statistics and per-replica class-aware loss, as in the reference's DDP.
The reference's quality metrics are opt-in (TRAIN.INCEPTION_WEIGHTS or enable_inception): the Inception-v3 pass over
each step's fake and real 256 px images runs on the gfx950 kernels (inception.py) into device buffers, and every snapshot
with >= 500 collected batches reports the Inception score, NLPP and FID (trainer.py:563-565, 603-629).  Every snapshot
also writes the reference's image grids (trainer.py:268-295, 589-601): Image/real_samples.png and
Image/count_<count>_fake_samples<i>.png, from the EMA generator on a noise batch fixed for the run, composed on the device
(ops.image_grid_uint8); TRAIN.VIS_COUNT = 0 turns them off.  The TensorBoard calls of the reference loop are not reproduced.
Beyond the reference: TRAIN.STATE_EVERY writes Model/state.pt, the full training state, at epoch boundaries, and TRAIN.STATE
continues from one bit for bit (save_state / load_state, train_state.py); both are off by default.
"""
import json
import os
import time
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import S2IError
from .miscc.config import cfg
from .miscc.utils import mkdir_p
from .model import D_NET64, D_NET128, D_NET256, D_NET512, D_NET1024, G_NET, INCEPTION_V3  # noqa: F401


# ---- shared functions --------------------------------------------------------------------------------
def compute_mean_covariance(img):
    """Per-image channel mean (B,C,1,1) and C x C covariance over pixels (trainer.py:34-51).  Dormant in every
    BASELINE config (COLOR_LOSS = 0): plain torch ops on 3-channel images, no kernel of its own."""
    batch_size, channel_num, height, width = img.shape
    num_pixels = height * width
    mu = img.mean(2, keepdim=True).mean(3, keepdim=True)
    img_hat = (img - mu.expand_as(img)).view(batch_size, channel_num, num_pixels)
    covariance = torch.bmm(img_hat, img_hat.transpose(1, 2)) / num_pixels
    return mu, covariance


def KL_loss(mu, logvar):
    return ops.KLLoss.apply(mu, logvar)


# ---- GAN quality metrics (trainer.py:88-159), host float64 -------------------------------------------------------------
def compute_inception_score(predictions, num_splits=1):
    """exp(E_x KL(p(y|x) || p(y))) per split of the softmax rows; (mean, std) over the splits."""
    predictions = np.asarray(predictions, dtype=np.float64)
    scores = []
    for i in range(num_splits):
        istart = i * predictions.shape[0] // num_splits
        iend = (i + 1) * predictions.shape[0] // num_splits
        part = predictions[istart:iend, :]
        kl = part * (np.log(part) - np.log(np.expand_dims(np.mean(part, 0), 0)))
        kl = np.mean(np.sum(kl, 1))
        scores.append(np.exp(kl))
    return np.mean(scores), np.std(scores)


def _trace_sqrtm_product(s1, s2):
    """trace(sqrtm(s1 @ s2)) for symmetric positive semi-definite s1, s2: s1 @ s2 is similar to
    sqrt(s1) @ s2 @ sqrt(s1), which is symmetric PSD, so the trace is the sum of the square roots of its eigenvalues
    (rounding-negative ones count as 0, as the real part of scipy's sqrtm does)."""
    l, u = np.linalg.eigh(s1)
    r = (u * np.sqrt(np.clip(l, 0.0, None))) @ u.T
    m = r @ s2 @ r
    ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    return float(np.sum(np.sqrt(np.clip(ev, 0.0, None))))


def compute_frethet_distance(predictions_g, predictions_r, eps=1e-6):
    """Frechet distance between Gaussians fitted to two sets of pool3 rows (the reference's spelling and return value:
    (distance, [{'mu', 'sigma'} x 2]), where the reference stores mu_g in both entries)."""
    predictions_g = np.asarray(predictions_g, dtype=np.float64)
    predictions_r = np.asarray(predictions_r, dtype=np.float64)
    mu1, sigma1 = np.atleast_1d(np.mean(predictions_g, axis=0)), np.atleast_2d(np.cov(predictions_g, rowvar=False))
    mu2, sigma2 = np.atleast_1d(np.mean(predictions_r, axis=0)), np.atleast_2d(np.cov(predictions_r, rowvar=False))
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    data = [{'mu': mu1, 'sigma': sigma1}, {'mu': mu1, 'sigma': sigma2}]
    return _frechet_from_moments(mu1, sigma1, mu2, sigma2, eps), data


def _frechet_from_moments(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """||mu1 - mu2||^2 + tr(sigma1) + tr(sigma2) - 2 tr(sqrtm(sigma1 sigma2)), retried with eps on the diagonals when the
    product is singular (trainer.py:125-144)."""
    diff = mu1 - mu2
    tr_covmean = _trace_sqrtm_product(sigma1, sigma2)
    if not np.isfinite(tr_covmean):
        print('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        tr_covmean = _trace_sqrtm_product(sigma1 + offset, sigma2 + offset)
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


def negative_log_posterior_probability(predictions, num_splits=1):
    """-log max_y p(y|x), averaged per split; (mean, std) over the splits."""
    predictions = np.asarray(predictions, dtype=np.float64)
    scores = []
    for i in range(num_splits):
        istart = i * predictions.shape[0] // num_splits
        iend = (i + 1) * predictions.shape[0] // num_splits
        part = predictions[istart:iend, :]
        scores.append(np.mean(-1. * np.log(np.max(part, 1))))
    return np.mean(scores), np.std(scores)


def weights_init(m):
    """Conv*/Linear: orthogonal(gain 1); BatchNorm*: weight ~ N(1, 0.02), bias 0 (trainer.py:65-75)."""
    classname = m.__class__.__name__
    if classname.find('Conv') != -1:
        nn.init.orthogonal_(m.weight.data, 1.0)
    elif classname.find('BatchNorm') != -1:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)
    elif classname.find('Linear') != -1:
        nn.init.orthogonal_(m.weight.data, 1.0)
        if m.bias is not None:
            m.bias.data.fill_(0.0)


def load_params(model, new_param):
    for p, new_p in zip(model.parameters(), new_param):
        p.data.copy_(new_p)
    ops.refresh_packed(model.parameters())


def copy_G_params(model):
    return deepcopy(list(p.data for p in model.parameters()))


def class_labels_to_device(class_labels, device):
    if torch.is_tensor(class_labels):
        return class_labels.to(device=device, dtype=torch.int32).contiguous()
    return torch.tensor([int(v) for v in class_labels], dtype=torch.int32, device=device)


def class_aware_loss(x_activates, class_labels):
    """x_activates (B, D); class_labels: sequence / tensor of B class ids (trainer.py:298-311)."""
    return ops.ClassAwareLoss.apply(x_activates, class_labels_to_device(class_labels, x_activates.device))


def _unwrap(net):
    return net.module if hasattr(net, 'module') else net


def save_singleimages(images_u8, filenames, save_dir, split_dir, sentenceID, imsize, sample_idx=0):
    """images_u8: (B,H,W,3) uint8 on the host.  Same file naming as the reference (trainer.py:664-679)."""
    from PIL import Image
    for i in range(images_u8.shape[0]):
        s_tmp = '%s/single_samples/%s/%s' % (save_dir, split_dir, filenames[i])
        folder = s_tmp[:s_tmp.rfind('/')]
        if not os.path.isdir(folder):
            mkdir_p(folder)
        Image.fromarray(images_u8[i]).save('%s_%d_sentence%d_%d.png' % (s_tmp, imsize, sentenceID, sample_idx))


class _Replica(nn.Module):
    """Stand-in for the reference's DataParallel / DDP wrapper: same `module.`-prefixed state_dict
    keys (trainer.py:167-171, 192-196, 255-265) and a `device_ids` attribute, no comm of its own —
    gradients are reduced per network by FlatNet below."""

    def __init__(self, module, device_ids):
        super().__init__()
        self.module = module
        self.device_ids = list(device_ids)

    def forward(self, *a, **k):
        return self.module(*a, **k)


def load_network(gpus, distributed):
    """Build G and the per-scale Ds, initialise, wrap, optionally resume (trainer.py:162-233).
    The reference also builds INCEPTION_V3 here (a network download); the returned slot is None."""
    dev = torch.device('cuda', gpus[0]) if cfg.CUDA else torch.device('cpu')
    netG = G_NET()
    netG.apply(weights_init)
    netG = _Replica(netG.to(dev), gpus)
    classes = (D_NET64, D_NET128, D_NET256, D_NET512, D_NET1024)
    netsD = []
    for i in range(min(cfg.TREE.BRANCH_NUM, len(classes))):
        d = classes[i]()
        d.apply(weights_init)
        netsD.append(_Replica(d.to(dev), gpus))
    count = 0
    if cfg.TRAIN.NET_G != '':
        state_dict = torch.load(cfg.TRAIN.NET_G, map_location='cpu', weights_only=True)
        netG.load_state_dict(state_dict)
        istart = cfg.TRAIN.NET_G.rfind('_') + 1
        iend = cfg.TRAIN.NET_G.rfind('.')
        count = int(cfg.TRAIN.NET_G[istart:iend]) + 1
    if cfg.TRAIN.NET_D != '':
        for i in range(len(netsD)):
            state_dict = torch.load('%s%d.pth' % (cfg.TRAIN.NET_D, i), map_location='cpu', weights_only=True)
            netsD[i].load_state_dict(state_dict)
    return netG, netsD, len(netsD), None, count


# ---- flat parameter storage + fused optimiser -------------------------------------------------------------
class FlatNet:
    """All parameters of one network re-homed into a flat buffer (views keep nn.Module semantics);
    gradients accumulate into a second flat buffer; Adam moments in two more.  `params` re-homes that subset of the
    network's parameters instead of all of them; a `weight_decay` other than 0 makes the step torch.optim.Adam's L2 form
    (ops.adam_l2_step: the speech encoder's optimiser, encoder_train.py)."""

    def __init__(self, net, lr, betas=(0.5, 0.999), eps=1e-8, with_ema=False, weight_decay=0.0, params=None):
        self.net = net
        self.params = [p for p in (net.parameters() if params is None else params)]
        self.weight_decay = float(weight_decay)
        dev = self.params[0].device
        self.sizes = [p.numel() for p in self.params]
        self.offsets, off = [], 0
        for n in self.sizes:
            self.offsets.append(off)
            off += (n + 3) & ~3  # keep every tensor 16-byte aligned inside the flat buffer
        self.total = off
        self.p = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.g = torch.zeros_like(self.p)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        for p, o, n in zip(self.params, self.offsets, self.sizes):
            self.p[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.p[o:o + n].view_as(p)
            p.grad = self.g[o:o + n].view_as(p)
        self.avg = self.p.clone() if with_ema else None
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_count = 0
        self.clip, self.skipped_before = None, 0     # ops.GradLayout of the guarded step, built at its first use
        ops.refresh_packed(self.params)

    def zero_grad(self):
        self.g.zero_()
        for p, o, n in zip(self.params, self.offsets, self.sizes):
            if p.grad is None or p.grad.data_ptr() != self.g.data_ptr() + 4 * o:
                p.grad = self.g[o:o + n].view_as(p)

    def set_requires_grad(self, flag):
        for p in self.params:
            p.requires_grad_(flag)

    def adam(self, gscale=1.0, max_norm=None, guard=False):
        """One optimiser step on gscale * g.  With `max_norm` (> 0) or `guard` it is the three-launch guarded step
        (_adam_guarded); without them, the default and all the GAN trainer uses, s2i_increment and one Adam launch."""
        if max_norm or guard:
            return self._adam_guarded(gscale, float(max_norm or 0.0))
        ops.increment(self.step_dev)
        self.step_count += 1
        if self.weight_decay:
            ops.adam_l2_step(self.p, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps,
                             self.weight_decay, step_dev=self.step_dev, gscale=gscale)
        else:
            ops.adam_step(self.p, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps,
                          step_dev=self.step_dev, gscale=gscale)
        ops.refresh_packed(self.params)

    def _adam_guarded(self, gscale, max_norm):
        """ops.grad_sumsq over the flat gradient buffer, ops.grad_clip_scale (the norm of gscale * g, clip_grad_norm_'s
        coefficient for max_norm > 0, the skip decision and the step counter's increment, all on the device) and the Adam
        launch that reads them.  A gradient whose sum of squares is not finite is skipped whether or not max_norm is set: p,
        m, v and the step counter stay as they were.  Nothing is read back here, so `step_count` lags until sync_step_count()."""
        if self.clip is None:
            self.clip = ops.GradLayout(self.offsets, self.sizes, self.total, self.p.device)
        c = self.clip
        ops.grad_sumsq(self.g, c)
        ops.grad_clip_scale(c, gscale, max_norm, self.step_dev)
        if self.weight_decay:
            ops.adam_l2_step_dev(self.p, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps,
                                 self.weight_decay, self.step_dev, c.scale, c.apply)
        else:
            ops.adam_step_dev(self.p, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps,
                              self.step_dev, c.scale, c.apply)
        ops.refresh_packed(self.params)

    def sync_step_count(self):
        """`step_count` as the device counts it: behind guarded steps the number of applied updates (one synchronisation;
        without a guarded step the host count is already right and nothing is read)."""
        if self.clip is not None:
            self.step_count = int(self.step_dev)
        return self.step_count

    def grad_stats(self, reset=False):
        """The guarded steps' record on the host (one synchronisation): the last step's `norm` (of the gradient the
        optimiser used, gscale included), `coef`, `scale` and `apply`; since the last reset `updates` (applied), `clipped`
        (coef < 1), `skipped`, `norm_mean` and `norm_max` over the applied ones; `skipped_total` since construction or
        load_state_dict; `tensor_norms`, the last step's norm per parameter name.  None before the first guarded step."""
        if self.clip is None:
            return None
        st = self.clip.read_stats()
        names = {id(p): n for n, p in self.net.named_parameters()} if self.net is not None else {}
        norms, sumsq = st.pop("tensor_norms"), st.pop("tensor_sumsq")
        st["tensor_norms"] = {names.get(id(p), "param%d" % k): norms[k] for k, p in enumerate(self.params)}
        st["tensor_sumsq"] = sumsq
        st["norm_mean"] = st["norm_sum"] / st["updates"] if st["updates"] else 0.0
        st["skipped_total"] = self.skipped_before + st["skipped"]
        if reset:
            self.skipped_before += st["skipped"]
            self.clip.reset_stats()
        return st

    def ema(self, decay=0.999):
        ops.ema_update(self.avg, self.p, decay)

    def avg_params(self):
        return [self.avg[o:o + n].view_as(p) for p, o, n in zip(self.params, self.offsets, self.sizes)]

    def state_dict(self):
        """Clones of the parameters, both Adam moments and the EMA copy (if kept), the step count and learning rate, and
        the layout (`sizes`, `offsets`) that load_state_dict checks.  The gradient buffer is not state: every update
        zeroes it first."""
        self.sync_step_count()
        sd = {"p": self.p.detach().clone(), "m": self.m.clone(), "v": self.v.clone(), "step_count": int(self.step_count),
              "lr": float(self.lr), "sizes": list(self.sizes), "offsets": list(self.offsets)}
        if self.avg is not None:
            sd["avg"] = self.avg.clone()
        return sd

    def load_state_dict(self, sd):
        """Copy a state_dict() into the existing buffers in place: the flat buffers and every parameter view keep their
        addresses, which a recorded plan or graph and avg_params() hold.  The device-side step counter follows, and every
        packed, bf16 or split-plane copy of the old weights is re-derived."""
        sizes = [int(n) for n in sd["sizes"]]
        if sizes != self.sizes:
            names = {id(p): n for n, p in self.net.named_parameters()} if self.net is not None else {}
            for k in range(max(len(sizes), len(self.sizes))):
                have = self.sizes[k] if k < len(self.sizes) else None
                got = sizes[k] if k < len(sizes) else None
                if have != got:
                    name = names.get(id(self.params[k]), "") if k < len(self.params) else ""
                    raise ValueError("FlatNet.load_state_dict: tensor %d%s has %s elements here and %s in the state "
                                     "(%d tensors here, %d there)" % (k, " (%s)" % name if name else "", have, got,
                                                                      len(self.sizes), len(sizes)))
        if ("avg" in sd) != (self.avg is not None):
            raise ValueError("FlatNet.load_state_dict: the state %s an EMA copy and this network %s"
                             % (("has", "keeps none") if "avg" in sd else ("has no", "keeps one")))
        pairs = [(self.p, sd["p"]), (self.m, sd["m"]), (self.v, sd["v"])] + ([(self.avg, sd["avg"])] if "avg" in sd else [])
        for dst, src in pairs:
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError("FlatNet.load_state_dict: a buffer of %s %s for one of %s %s"
                                 % (tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype))
        with torch.no_grad():
            for dst, src in pairs:
                dst.copy_(src)
        self.step_count = int(sd["step_count"])
        self.step_dev.fill_(self.step_count)
        self.lr = float(sd["lr"])
        ops.refresh_packed(self.params)
        ops.invalidate_derived(self.params)


class _LegacyOptimizer:
    """`optimizer.step()` / `.zero_grad()` facade over FlatNet for callers written against
    torch.optim (define_optimizers' return values)."""

    def __init__(self, flat):
        self.flat = flat

    def step(self):
        # torch's own `net.zero_grad()` (set_to_none) detaches the parameters' .grad views from the flat gradient
        # buffer; stepping then would apply stale zeros.  Refuse instead of silently not training.
        f = self.flat
        for p, o in zip(f.params, f.offsets):
            if p.grad is None or p.grad.data_ptr() != f.g.data_ptr() + 4 * o:
                raise RuntimeError("optimizer.step(): a parameter's .grad no longer aliases the flat gradient buffer "
                                   "(was net.zero_grad(set_to_none=True) called?); use optimizer.zero_grad()")
        self.flat.adam()

    def zero_grad(self):
        self.flat.zero_grad()


def define_optimizers(netG, netsD):
    """Adam(lr from cfg, betas (0.5, 0.999)) per network (trainer.py:236-252), fused and flat."""
    flatsD = [FlatNet(_unwrap(d), cfg.TRAIN.DISCRIMINATOR_LR) for d in netsD]
    flatG = FlatNet(_unwrap(netG), cfg.TRAIN.GENERATOR_LR, with_ema=True)
    return _LegacyOptimizer(flatG), [_LegacyOptimizer(f) for f in flatsD]


def save_model(netG, avg_param_G, netsD, epoch, model_dir):
    """Model/netG_<count>.pth holds the EMA weights, Model/netD<i>.pth the live ones; keys carry the
    wrapper's `module.` prefix (trainer.py:255-265).  Tensors are cloned so the flat buffers behind
    the parameter views are not serialised whole."""
    load_params(netG, avg_param_G)
    torch.save({k: v.clone() for k, v in netG.state_dict().items()}, '%s/netG_%d.pth' % (model_dir, epoch))
    for i, netD in enumerate(netsD):
        torch.save({k: v.clone() for k, v in netD.state_dict().items()}, '%s/netD%d.pth' % (model_dir, i))
    print('Save G/Ds models.')


# ---- the trainer -----------------------------------------------------------------------------------------------
_D_STREAMS = {}   # (device, number of discriminators, priorities) -> per-discriminator HIP streams, shared process-wide


class condGANTrainer(object):
    d_overlap_min = 1 << 20     # smallest tail (elements) of a discriminator's flat gradient worth a second all-reduce

    def __init__(self, output_dir, data_loader, imsize, my_dataset_flag, local_rank=0, distributed=False):
        self.my_dataset_flag = my_dataset_flag
        if output_dir is not None:
            if not cfg.TRAIN.FLAG:
                output_dir += "_eval"
            self.model_dir = os.path.join(output_dir, 'Model')
            self.image_dir = os.path.join(output_dir, 'Image')
            self.log_dir = os.path.join(output_dir, 'Log')
            for d in (self.model_dir, self.image_dir, self.log_dir):
                mkdir_p(d)
        self.gpus = [local_rank]
        self.batch_size = cfg.TRAIN.BATCH_SIZE
        self.max_epoch = cfg.TRAIN.MAX_EPOCH
        self.snapshot_interval = cfg.TRAIN.SNAPSHOT_INTERVAL
        self.data_loader = data_loader
        self.num_batches = len(data_loader) if data_loader is not None else 0
        self.distributed = distributed
        self.world = torch.distributed.get_world_size() if distributed else 1
        self._pending = []
        self.stack_d_passes = True
        # independent discriminator passes on separate HIP streams (S2I_D_STREAMS=0 turns it off)
        self.d_streams = os.environ.get("S2I_D_STREAMS", "1") == "1" and torch.cuda.is_available()
        self._side_streams = None
        # hipGraph replay of the single-GPU step (S2I_GRAPH=1 or enable_graph()): the step has no host synchronisation and
        # a device-side Adam counter, so after a few eager warm-up steps it is captured once and replayed
        self._graph = None
        self._labels_dev = None
        self._g_pass = []
        self._aug = None      # (uniforms (num_Ds, 4, B, 8), policy mask) of the current step while TRAIN.DIFFAUG is set
        if os.environ.get("S2I_GRAPH", "0") == "1":
            self.enable_graph()
        # Inception-v3 scoring (off by default): per step, (softmax, pool3) device rows of [fake; real]
        self.inception_model = None
        self.inception_min_batches = 500      # trainer.py:605: metrics once this many batches are collected
        self._inception_rows = []
        if cfg.TRAIN.INCEPTION_WEIGHTS:
            self.enable_inception(cfg.TRAIN.INCEPTION_WEIGHTS)
        # snapshot grids: z and the conditioning-augmentation noise of the whole run (drawn by train() / on first use)
        self.fixed_noise = self.fixed_eps = None

    def _make_d_streams(self):
        """One stream per discriminator, all at the default priority.  (Round 2 gave the largest discriminator's stream the
        high HIP priority for 0.3 ms per step.  Round 3 found what that costs: while a high-priority queue holds PENDING
        packets -- the next step's discriminator work waiting on an event -- every other queue's kernels run slower, so a
        host that runs more than one step ahead made the step 20 % slower: 38.7 vs 31.6 ms, all of it in the generator's
        single-stream pieces (tools/replay_pieces.py, profiles/r03_replay_and_stream_priority.md section 3).  That, not
        branch serialisation, was also why hipGraph replay looked slow: with the priority removed the Python step, the launch
        plan and hipGraphLaunch take the same time (section 4 there).)  The streams are shared by every trainer of the process."""
        key = (torch.cuda.current_device(), self.num_Ds)
        if key not in _D_STREAMS:
            _D_STREAMS[key] = [torch.cuda.Stream() for i in range(self.num_Ds)]
        return _D_STREAMS[key]

    # -- set-up -------------------------------------------------------------------------------------------
    def build(self, netG=None, netsD=None, start_count=0):
        """Networks + flat optimisers.  `train()` calls this; benches and tests may pass their own nets."""
        if netG is None:
            netG, netsD, _, _, start_count = load_network(self.gpus, self.distributed)
        self.netG, self.netsD, self.num_Ds = netG, netsD, len(netsD)
        self.optimizerG, self.optimizersD = define_optimizers(self.netG, self.netsD)
        self.flatG = self.optimizerG.flat
        self.flatsD = [o.flat for o in self.optimizersD]
        if self.distributed:
            for f in [self.flatG] + self.flatsD:  # identical start on every rank (DDP's initial broadcast)
                torch.distributed.broadcast(f.p, 0)
                if f.avg is not None:
                    f.avg.copy_(f.p)
                ops.refresh_packed(f.params)
                # DDP(broadcast_buffers=True) (trainer.py:167, 192): a resumed rank-0 checkpoint propagates its
                # BatchNorm running statistics too
                for buf in f.net.buffers():
                    torch.distributed.broadcast(buf, 0)
            self.rank = torch.distributed.get_rank()
            self._install_g_overlap()
            self._install_d_overlap()
        self.avg_param_G = self.flatG.avg_params()
        return start_count

    def prepare_data(self, data):
        if self.my_dataset_flag:
            imgs, w_imgs, t_embedding = data["real_image"], data["wrong_image"], data["real_embedding"]
            class_labels = data.get("class_label", data.get("text"))
        else:
            imgs, w_imgs, t_embedding, _, class_labels = data
        dev = torch.device('cuda', self.gpus[0])
        vembedding = t_embedding.float().to(dev, non_blocking=True).requires_grad_()
        def to_dev(t):
            t = t.to(dev, non_blocking=True)
            # datasets built with device_normalize=True hand over uint8 HWC batches: ToTensor + Normalize on the GPU
            return ops.images_from_uint8_hwc(t.contiguous()) if t.dtype == torch.uint8 else t
        real_vimgs = [to_dev(imgs[i]) for i in range(self.num_Ds)]
        wrong_vimgs = [to_dev(w_imgs[i]) for i in range(self.num_Ds)]
        return imgs, real_vimgs, wrong_vimgs, vembedding, class_labels

    # -- communication ------------------------------------------------------------------------------------------
    def _reduce_async(self, flat, lo=0, hi=None):
        if not self.distributed:
            return None
        g = flat.g if (lo == 0 and hi is None) else flat.g[lo:hi]
        return torch.distributed.all_reduce(g, op=torch.distributed.ReduceOp.SUM, async_op=True)

    def _install_g_overlap(self):
        """G's gradient all-reduce in two contiguous chunks: everything behind INIT_STAGE_G.upsample1 in parameter
        order (upsample2..4, the image heads, stages 2 and 3: their backward is complete when the gradient of
        upsample1's output exists) is reduced while upsample1 / fc / ca_net -- 80 % of G's parameters, last in the
        backward -- are still computing; the head chunk follows the backward.  Same sums as one all-reduce."""
        g = _unwrap(self.netG)
        h1 = getattr(g, 'h_net1', None)
        self._g_split, self._g_tail_work = None, None
        if h1 is None or os.environ.get("S2I_G_OVERLAP", "1") != "1":
            return
        ids = {id(p): k for k, p in enumerate(self.flatG.params)}
        first_tail = ids.get(id(h1.upsample2[1].weight))
        if first_tail is None:
            return
        self._g_split = self.flatG.offsets[first_tail]

        def hook(grad):
            if self._g_hook_armed:
                self._g_hook_armed = False
                self._g_tail_work = self._reduce_async(self.flatG, self._g_split, None)
            return None
        h1.after_up1_hook = hook
        self._g_hook_armed = False

    def _install_d_overlap(self):
        """The same for the discriminators: the parameters behind img_code_s16 in parameter order (tower, jointConv, logit
        heads: 68 of D_NET256's 71 M parameters) have their gradients first in the backward; their all-reduce starts from a
        hook on img_code_s16's output and runs under the backward of the four image-side convolutions, which is most of a
        discriminator's backward time.  Same sums as one all-reduce (`S2I_D_OVERLAP=0`: one all-reduce after the backward)."""
        n = len(self.netsD)
        self._d_split, self._d_tail_work = [None] * n, [None] * n
        self._d_hook_armed, self._d_fires, self._d_expected = [False] * n, [0] * n, [1] * n
        if os.environ.get("S2I_D_OVERLAP", "1") != "1":
            return
        for idx, netD in enumerate(self.netsD):
            d = _unwrap(netD)
            flat = self.flatsD[idx]
            head = {id(p) for p in d.img_code_s16.parameters()}
            k = 0
            while k < len(flat.params) and id(flat.params[k]) in head:
                k += 1
            if k == 0 or k >= len(flat.params):
                continue
            split = flat.offsets[k]
            if flat.g.numel() - split < self.d_overlap_min:
                continue                                   # a tail below 4 MB is not worth a second collective
            self._d_split[idx] = split

            def hook(grad, idx=idx):
                if self._d_hook_armed[idx]:
                    self._d_fires[idx] += 1
                    if self._d_fires[idx] == self._d_expected[idx]:   # un-stacked passes: the last of the three
                        self._d_hook_armed[idx] = False
                        self._d_tail_work[idx] = self._reduce_async(self.flatsD[idx], self._d_split[idx], None)
                return None
            d.after_s16_hook = hook

    # -- differentiable augmentation of the discriminators' inputs (TRAIN.DIFFAUG) ----------------
    def draw_aug(self, B, device):
        """The step's uniforms while TRAIN.DIFFAUG names a policy, else None (and nothing is drawn): (num_Ds, 4, B, 8) from
        the device generator; [d, 0 / 1 / 2] are the tables of discriminator d's real / wrong / fake pass in train_Dnet and
        [d, 3] the table of its pass of the generator update."""
        if not ops.diffaug_policy(cfg.TRAIN.DIFFAUG):
            return None
        return torch.rand(self.num_Ds, 4, B, 8, device=device)

    def _set_aug(self, aug, B):
        policy = ops.diffaug_policy(cfg.TRAIN.DIFFAUG)
        if aug is None:
            if policy:
                raise ValueError("TRAIN.DIFFAUG = %r: train_step needs the step's uniforms (draw_aug)" % cfg.TRAIN.DIFFAUG)
            self._aug = None
            return
        if not policy:
            raise ValueError("train_step was given augmentation uniforms but TRAIN.DIFFAUG is empty")
        if tuple(aug.shape) != (self.num_Ds, 4, B, 8) or aug.dtype != torch.float32:
            raise ValueError("augmentation uniforms must be fp32 %s, got %s %s"
                             % ((self.num_Ds, 4, B, 8), aug.dtype, tuple(aug.shape)))
        self._aug = (aug.detach().contiguous(), policy)

    def _aug_of(self, idx, slot, slots=1):
        """(table, policy) of discriminator idx: the rows of `slots` consecutive passes from `slot` on, or None."""
        if self._aug is None:
            return None
        table, policy = self._aug
        return table[idx, slot:slot + slots].reshape(-1, 8), policy

    # -- D update (trainer.py:375-427) ----------------------------------------------------------------------------
    def _d_logits(self, idx):
        """Conditional/unconditional probabilities of the real, wrong and fake batches.  When the batch is a
        multiple of 8 (so that every layer's rows split into whole 128-row tiles per batch) the three passes run
        as ONE stacked forward with per-batch BatchNorm statistics; otherwise as the reference's three calls."""
        netD = self.netsD[idx]
        mu = self.mu.detach()
        B = mu.shape[0]
        stacked = self.stack_d_passes and B % 8 == 0
        if getattr(self, '_d_expected', None) is not None:
            self._d_expected[idx] = 1 if stacked else 3     # backward firings of the img_code_s16 hook
        if stacked:
            x = torch.cat((self.real_imgs[idx], self.wrong_imgs[idx], self.fake_imgs[idx].detach()), 0)
            logits, _ = _unwrap(netD)(x, mu.repeat(3, 1), groups=3, need_features=False, aug=self._aug_of(idx, 0, 3))
            self._stacked_logits = logits
            return [[l[g * B:(g + 1) * B] for l in logits] for g in range(3)]
        self._stacked_logits = None
        return [netD(self.real_imgs[idx], mu, aug=self._aug_of(idx, 0))[0],
                netD(self.wrong_imgs[idx], mu, aug=self._aug_of(idx, 1))[0],
                netD(self.fake_imgs[idx].detach(), mu, aug=self._aug_of(idx, 2))[0]]

    def _d_loss(self, idx):
        u = cfg.TRAIN.COEFF.UNCOND_LOSS
        real_logits, wrong_logits, fake_logits = self._d_logits(idx)
        if self._stacked_logits is not None and len(self._stacked_logits) == 2 and u > 0:
            # the six BCE terms of trainer.py:394-409 on the stacked (real | wrong | fake) heads, one launch:
            # cond targets 1/0/0, uncond targets 1/1/0 (wrong pairs count as real for the uncond head, :401)
            dev = self._stacked_logits[0].device
            key = (str(dev), float(u))
            if getattr(self, '_bce_consts', (None,))[0] != key:
                self._bce_consts = (key, torch.tensor([1., 1., 0., 1., 0., 0.], device=dev),
                                    torch.tensor([1., u, 1., u, 1., u], device=dev))
            return ops.BCEMulti.apply(self._bce_consts[1], self._bce_consts[2], 3, *self._stacked_logits)
        errD_real = ops.BCELoss.apply(real_logits[0], 1.0, 1.0)
        errD_wrong = ops.BCELoss.apply(wrong_logits[0], 0.0, 1.0)
        errD_fake = ops.BCELoss.apply(fake_logits[0], 0.0, 1.0)
        if len(real_logits) > 1 and u > 0:
            errD_real = errD_real + ops.BCELoss.apply(real_logits[1], 1.0, u)
            errD_wrong = errD_wrong + ops.BCELoss.apply(wrong_logits[1], 1.0, u)  # uncond target real (:401)
            errD_fake = errD_fake + ops.BCELoss.apply(fake_logits[1], 0.0, u)
            return errD_real + errD_wrong + errD_fake
        return errD_real + 0.5 * (errD_wrong + errD_fake)

    def train_Dnet(self, idx, count, defer_step=False):
        flat = self.flatsD[idx]
        flat.zero_grad()
        split = getattr(self, '_d_split', [None] * self.num_Ds)[idx] if self.distributed else None
        if split is not None:
            self._d_tail_work[idx], self._d_fires[idx] = None, 0
            self._d_hook_armed[idx] = True
        errD = self._d_loss(idx)
        errD.backward()
        if split is not None:
            self._d_hook_armed[idx] = False
        if split is not None and self._d_tail_work[idx] is not None:
            works = [self._reduce_async(flat, 0, split), self._d_tail_work[idx]]   # head chunk: img_code_s16
            self._d_tail_work[idx] = None
        else:
            works = [self._reduce_async(flat)]
        if defer_step:
            self._pending.append((flat, works))
        else:
            for work in works:
                if work is not None:
                    work.wait()
            flat.adam(1.0 / self.world)
        return errD

    def _flush_d_steps(self):
        for flat, works in self._pending:
            for work in works:
                if work is not None:
                    work.wait()
            flat.adam(1.0 / self.world)
        self._pending = []

    # -- G update (trainer.py:429-489) ------------------------------------------------------------------------------
    def _g_pass_of_d(self, i):
        """Discriminator i's part of the G update, forward AND backward, on the current stream: the adversarial (and
        class-aware) loss of the fake image of scale i, and its gradients w.r.t. that image and mu.  The images and mu enter
        as detached leaves, so this piece of the backward belongs to this discriminator's stream alone; the generator's
        backward (`_g_backward`) continues from the two gradients.  Same chain rule as one backward over the summed loss
        (trainer.py:437-446, 487)."""
        u = cfg.TRAIN.COEFF.UNCOND_LOSS
        flat = self.flatsD[i]
        flat.set_requires_grad(False)   # D's weight gradients would be discarded (trainer.py:385)
        try:
            fake = self.fake_imgs[i].detach().requires_grad_(True)
            mu = self.mu.detach().requires_grad_(True)
            outputs, x_active = self.netsD[i](fake, mu, aug=self._aug_of(i, 3))
            errG = ops.BCELoss.apply(outputs[0], 1.0, 1.0)
            if len(outputs) > 1 and u > 0:
                errG = errG + ops.BCELoss.apply(outputs[1], 1.0, u)
            if cfg.TRAIN.COEFF.CAL_LOSS > 0:
                if self._labels_dev is None:
                    self._labels_dev = class_labels_to_device(self.class_labels, x_active.device)
                errG = errG + ops.ClassAwareLoss.apply(x_active, self._labels_dev).reshape(())
            g_fake, g_mu = torch.autograd.grad(errG, [fake, mu], allow_unused=True)
        finally:
            flat.set_requires_grad(True)
        self._g_pass[i] = (errG.detach(), g_fake, g_mu)

    def _g_backward(self):
        """The generator's own part of the G update on the current stream (after every `_g_pass_of_d`): KL term, the
        backward from the image gradients, all-reduce, Adam."""
        self.flatG.zero_grad()
        errG_total = 0
        roots, grads = [], []
        g_mu_total = None
        for i in range(self.num_Ds):
            errG, g_fake, g_mu = self._g_pass[i]
            errG_total = errG_total + errG
            roots.append(self.fake_imgs[i])
            grads.append(g_fake)
            if g_mu is not None:
                g_mu_total = g_mu if g_mu_total is None else g_mu_total + g_mu
        self._g_pass = [None] * self.num_Ds
        extra = 0
        if cfg.TRAIN.COEFF.COLOR_LOSS > 0:
            # colour-consistency between neighbouring scales (trainer.py:455-478); dormant by default
            coef = cfg.TRAIN.COEFF.COLOR_LOSS
            for hi, lo in ((-1, -2), (-2, -3)):
                if self.num_Ds >= -lo:
                    mu1, cov1 = compute_mean_covariance(self.fake_imgs[hi])
                    mu2, cov2 = compute_mean_covariance(self.fake_imgs[lo].detach())
                    extra = extra + coef * nn.functional.mse_loss(mu1, mu2) + coef * 5 * nn.functional.mse_loss(cov1, cov2)
        kl_loss = KL_loss(self.mu, self.logvar) * cfg.TRAIN.COEFF.KL
        own = kl_loss + extra
        errG_total = errG_total + own.detach()
        if g_mu_total is not None:
            roots.append(self.mu)
            grads.append(g_mu_total)
        roots.append(own)
        grads.append(torch.ones_like(own))
        split = getattr(self, '_g_split', None) if self.distributed else None
        self._g_tail_work = None
        self._g_hook_armed = split is not None
        torch.autograd.backward(roots, grads)
        self._g_hook_armed = False
        if self.distributed and self._g_tail_work is not None:
            work = self._reduce_async(self.flatG, 0, split)   # head chunk: ca_net, fc, upsample1
            work.wait()
            self._g_tail_work.wait()
            self._g_tail_work = None
        else:
            work = self._reduce_async(self.flatG)
            if work is not None:
                work.wait()
        self.flatG.adam(1.0 / self.world)
        return kl_loss.detach(), errG_total

    def train_Gnet(self, count):
        """One generator update: every discriminator's pass on its own HIP stream (forward, losses, backward to the fake
        image), then the generator's backward and Adam on the current stream."""
        self._labels_dev = None
        self._g_pass = [None] * self.num_Ds
        main = torch.cuda.current_stream() if self.d_streams else None
        if self.d_streams and self._side_streams is None:
            self._side_streams = self._make_d_streams()
        for i in range(self.num_Ds):
            if self.d_streams:
                self._side_streams[i].wait_stream(main)  # fake images / mu; D_i's own update is already in order
                with torch.cuda.stream(self._side_streams[i]):
                    self._g_pass_of_d(i)
            else:
                self._g_pass_of_d(i)
        if self.d_streams:
            for i in range(self.num_Ds):
                main.wait_stream(self._side_streams[i])
        return self._g_backward()

    # -- one iteration (trainer.py:536-572), Inception forwards excluded --------------------------------------------
    def enable_graph(self, warmup=3, executor="plan"):
        """Replay the single-GPU step from a recording after `warmup` eager steps.  The step is cut where its HIP streams
        fork and join, and every piece is captured as a graph of ONE stream: the generator forward (main stream), per
        discriminator its update followed by its pass of the G update (that discriminator's stream), the generator's
        backward + Adam + EMA (main stream).  The pieces are launched like kernels -- stream waits between them -- so the
        three discriminator streams stay concurrent.  executor="plan" (default): the captured graphs are only the RECORDING;
        their kernel nodes are re-issued as plain launches from one C call per piece (s2i_plan_replay, include/s2i_hip.h):
        hipGraphLaunch itself is slower than the Python step it replaces on ROCm 7.2.
        executor="graph": hipGraphLaunch of each piece.  Single process only: an RCCL all-reduce inside a recording is
        not exercised here.  Not with TRAIN.DIFFAUG: a recording would replay the uniforms it was captured with, so this
        raises S2IError while a policy is set, and so does a step that is given uniforms after enable_graph()."""
        if ops.diffaug_policy(cfg.TRAIN.DIFFAUG):
            raise S2IError("enable_graph: TRAIN.DIFFAUG = %r draws new uniforms every step, which a recorded step "
                                    "would not see; run the eager step" % cfg.TRAIN.DIFFAUG)
        # warm-up and capture run on one private stream: autograd's AccumulateGrad nodes remember the stream they were
        # created on, and one that lives on the (non-capturing) default stream invalidates the capture
        if executor not in ("plan", "graph"):
            raise ValueError("executor must be 'plan' or 'graph'")
        self._graph = dict(warmup=warmup, seen=0, graphs=None, stream=torch.cuda.Stream(), executor=executor)

    def _graph_signature(self, real_imgs, wrong_imgs, txt_embedding, noise, eps):
        ts = list(real_imgs) + list(wrong_imgs) + [txt_embedding, noise] + ([eps] if eps is not None else [])
        return tuple((tuple(t.shape), t.dtype) for t in ts) + (ops.ACT_BF16, ops.MATH_PLANES, bool(txt_embedding.requires_grad))

    def _capture(self, real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps):
        st = self._graph
        dev = noise.device
        static = dict(real=[t.detach().clone() for t in real_imgs], wrong=[t.detach().clone() for t in wrong_imgs],
                      emb=txt_embedding.detach().clone().requires_grad_(txt_embedding.requires_grad),
                      noise=noise.detach().clone(), eps=None if eps is None else eps.detach().clone(),
                      labels=class_labels_to_device(class_labels, dev).clone())
        # no autograd graph of an earlier iteration may survive into the capture (it would keep its AccumulateGrad nodes)
        self.fake_imgs = self.mu = self.logvar = self._stacked_logits = None
        self.real_imgs = self.wrong_imgs = self.txt_embedding = None
        import gc
        gc.collect()
        torch.cuda.synchronize()
        ops.pin_graph_resources()      # workspaces and pack tables referenced by the graphs are never freed from here on
        main = st['stream']
        if self._side_streams is None:
            self._side_streams = self._make_d_streams()
        n = self.num_Ds
        # one memory pool per stream: pieces that replay concurrently must not share freed blocks
        pools = [torch.cuda.graph_pool_handle() for _ in range(n + 1)]
        keep = st['executor'] == "plan"       # the plan reads the captured graph's nodes: keep the hipGraph_t
        graphs = dict(fwd=torch.cuda.CUDAGraph(keep_graph=keep), d=[torch.cuda.CUDAGraph(keep_graph=keep) for _ in range(n)],
                      g=torch.cuda.CUDAGraph(keep_graph=keep))
        errs = [None] * n
        with ops.param_grad_mode(True):
            with torch.cuda.graph(graphs['fwd'], pool=pools[n], stream=main):
                self._begin_step(static['real'], static['wrong'], static['emb'], static['labels'])
                self.fake_imgs, self.mu, self.logvar = _unwrap(self.netG)(static['noise'], static['emb'], static['eps'])
            for i in reversed(range(n)):
                with torch.cuda.graph(graphs['d'][i], pool=pools[i], stream=self._side_streams[i]):
                    errs[i] = self.train_Dnet(i, 0).detach()
                    self._g_pass_of_d(i)
            with torch.cuda.graph(graphs['g'], pool=pools[n], stream=main):
                kl_loss, errG_total = self._g_backward()
                self.flatG.ema(0.999)
                errD_total = 0
                for e in reversed(errs):        # the eager step's order: largest discriminator first
                    errD_total = errD_total + e
                outs = [o.detach().reshape(()) for o in (errD_total, errG_total, kl_loss)]
        for f in [self.flatG] + self.flatsD:
            f.step_count -= 1          # FlatNet.adam counted a step the capture did not execute; the replay below counts it
        plans = None
        if keep:
            import ctypes
            from . import _lib
            lib = _lib.load()

            def make_plan(g):
                handle, counts = ctypes.c_void_p(), (ctypes.c_int * 3)()
                _lib.check(lib.s2i_plan_create(g.raw_cuda_graph(), ctypes.byref(handle), counts), "s2i_plan_create")
                return handle, tuple(counts)
            plans = dict(fwd=make_plan(graphs['fwd']), d=[make_plan(g) for g in graphs['d']], g=make_plan(graphs['g']))
            st['launches'] = (plans['fwd'][1][0] + sum(p[1][0] for p in plans['d']) + plans['g'][1][0])
        st.update(graphs=graphs, plans=plans, static=static, outs=outs, pools=pools,
                  sig=self._graph_signature(real_imgs, wrong_imgs, txt_embedding, noise, eps))
        # the capture itself did not execute anything: replay once so that this call IS a step
        return self._replay(real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps, fresh=True)

    def _replay(self, real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps, fresh=False):
        st = self._graph
        s = st['static']

        def put(dst, src):
            if dst.data_ptr() != src.data_ptr():
                with torch.no_grad():
                    dst.copy_(src.detach(), non_blocking=True)
        if not fresh:
            for d, r in zip(s['real'], real_imgs):
                put(d, r)
            for d, r in zip(s['wrong'], wrong_imgs):
                put(d, r)
            put(s['emb'], txt_embedding)
            put(s['noise'], noise)
            if eps is not None:
                put(s['eps'], eps)
            put(s['labels'], class_labels_to_device(class_labels, noise.device))
        main = torch.cuda.current_stream()
        if st['plans'] is not None:
            from . import _lib
            lib, pl = _lib.load(), st['plans']
            _lib.check(lib.s2i_plan_replay(pl['fwd'][0], main.cuda_stream), "s2i_plan_replay")
            for i in reversed(range(self.num_Ds)):    # largest first, as the eager step enqueues them
                side = self._side_streams[i]
                side.wait_stream(main)
                _lib.check(lib.s2i_plan_replay(pl['d'][i][0], side.cuda_stream), "s2i_plan_replay")
            for i in range(self.num_Ds):
                main.wait_stream(self._side_streams[i])
            _lib.check(lib.s2i_plan_replay(pl['g'][0], main.cuda_stream), "s2i_plan_replay")
        else:
            g = st['graphs']
            g['fwd'].replay()
            for i in reversed(range(self.num_Ds)):
                side = self._side_streams[i]
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    g['d'][i].replay()
            for i in range(self.num_Ds):
                main.wait_stream(self._side_streams[i])
            g['g'].replay()
        for f in [self.flatG] + self.flatsD:
            f.step_count += 1
        if txt_embedding.requires_grad and s['emb'].grad is not None:
            txt_embedding.grad = s['emb'].grad.clone()     # the static gradient buffer is overwritten by the next replay
        return tuple(st['outs'])

    # -- GAN quality metrics (trainer.py:217-232, 563-565, 603-629) ------------------------------------------------------
    def enable_inception(self, weights):
        """Score every step's fake_imgs[-1] and real_imgs[-1] with Inception-v3 (`weights`: a local torchvision-layout
        state_dict file, a loaded dict, or an INCEPTION_V3).  The pass runs after the step on the same stream, as one
        stacked batch, into device buffers: no host synchronisation until a snapshot scores them.  With data parallelism
        only rank 0 runs it, so the metrics describe rank 0's shard of the data."""
        self.inception_model = weights if isinstance(weights, INCEPTION_V3) else INCEPTION_V3(weights)
        self._inception_rows = []

    def _inception_pass(self, real):
        if self.distributed and torch.distributed.get_rank() != 0:
            return
        fake = self.fake_imgs[-1].detach()
        real = real.detach()
        imgs = [t if t.dtype == torch.float32 else t.float() for t in (fake, real)]
        rows = fake.shape[0] + real.shape[0]
        soft = torch.empty(rows, 1000, device=fake.device)
        pool3 = torch.empty(rows, 2048, device=fake.device)
        self.inception_model.net(fake.device).run(imgs, soft, pool3)
        self._inception_rows.append((fake.shape[0], soft, pool3))

    def inception_arrays(self):
        """The collected rows on the host as float64: (predictions_g, predictions_r, activate_g, activate_r)."""
        pg, pr, ag, ar = [], [], [], []
        for b, soft, pool3 in self._inception_rows:
            soft, pool3 = soft.cpu().double().numpy(), pool3.cpu().double().numpy()
            pg.append(soft[:b]), pr.append(soft[b:]), ag.append(pool3[:b]), ar.append(pool3[b:])
        cat = np.concatenate
        return cat(pg, 0), cat(pr, 0), cat(ag, 0), cat(ar, 0)

    def score_inception(self, count):
        """At a snapshot: with >= inception_min_batches collected batches, IS (10 splits), NLPP (10 splits) and FID of fake
        vs real pool3; printed, appended as one JSON line to <output_dir>/Log/metrics.jsonl, and the buffers cleared.
        Returns the record, or None when nothing was scored."""
        if self.inception_model is None or len(self._inception_rows) < self.inception_min_batches:
            return None
        n = len(self._inception_rows)
        predictions_g, _, activate_g, activate_r = self.inception_arrays()
        self._inception_rows = []
        mean, std = compute_inception_score(predictions_g, 10)
        mean_nlpp, std_nlpp = negative_log_posterior_probability(predictions_g, 10)
        fid, _ = compute_frethet_distance(activate_g, activate_r)
        rec = dict(count=int(count), batches=n, images=int(predictions_g.shape[0]), inception_mean=float(mean),
                   inception_std=float(std), nlpp_mean=float(mean_nlpp), nlpp_std=float(std_nlpp), fid=float(fid))
        print('[%d] Inception score %.4f +- %.4f  NLPP %.4f +- %.4f  FID %.4f (%d images)'
              % (count, mean, std, mean_nlpp, std_nlpp, fid, rec['images']))
        if getattr(self, 'log_dir', None):
            with open(os.path.join(self.log_dir, 'metrics.jsonl'), 'a') as f:
                f.write(json.dumps(rec) + '\n')
        return rec

    def train_step(self, real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps=None, aug=None):
        """`aug`: the step's augmentation uniforms (draw_aug) while TRAIN.DIFFAUG is set, None otherwise."""
        self._set_aug(aug, noise.shape[0])
        if self._aug is not None and self._graph is not None:
            raise S2IError("TRAIN.DIFFAUG cannot run under enable_graph(): a recorded step would replay stale uniforms")
        out = self._dispatch_step(real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps)
        if self.inception_model is not None:
            self._inception_pass(real_imgs[-1])
        return out

    def _dispatch_step(self, real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps=None):
        st = self._graph
        if st is not None and not self.distributed and torch.cuda.is_available() and self.d_streams:
            if st['graphs'] is not None:
                if st['sig'] == self._graph_signature(real_imgs, wrong_imgs, txt_embedding, noise, eps):
                    return self._replay(real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps)
                # another batch shape (ragged last batch of an epoch): an eager step.  The replays bypassed the host-side
                # bookkeeping of the derived weight copies (bf16 / split planes, keyed by plan layout, and another batch
                # plans other layouts): drop them all, they are re-derived from the current masters on first use.
                for f in [self.flatG] + self.flatsD:
                    ops.invalidate_derived(f.params)
            elif st['seen'] >= st['warmup']:
                return self._capture(real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps)
            else:
                st['seen'] += 1
                gs, cur = st['stream'], torch.cuda.current_stream()
                gs.wait_stream(cur)
                with torch.cuda.stream(gs), ops.param_grad_mode(True):
                    out = self._train_step(real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps)
                cur.wait_stream(gs)
                return out
        # kernels accumulate into the flat gradient buffers (zeroed per update); the switch is scoped to the step, so
        # a later stock-optimiser use of the modules in this process gets autograd-returned gradients again.
        with ops.param_grad_mode(True):
            return self._train_step(real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps)

    def _begin_step(self, real_imgs, wrong_imgs, txt_embedding, class_labels):
        self.real_imgs, self.wrong_imgs = real_imgs, wrong_imgs
        self.txt_embedding, self.class_labels = txt_embedding, class_labels
        # class labels on the device once per step, on the main stream, before the discriminator streams fork
        self._labels_dev = (class_labels_to_device(class_labels, txt_embedding.device)
                            if cfg.TRAIN.COEFF.CAL_LOSS > 0 else None)
        self._g_pass = [None] * self.num_Ds

    def _train_step(self, real_imgs, wrong_imgs, txt_embedding, class_labels, noise, eps=None):
        self._begin_step(real_imgs, wrong_imgs, txt_embedding, class_labels)
        self.fake_imgs, self.mu, self.logvar = _unwrap(self.netG)(noise, txt_embedding, eps)
        errD_total = 0
        if self.d_streams and self.num_Ds >= 2:
            # the D updates are independent: each runs on its own HIP stream (zero, stacked forward, backward,
            # all-reduce, Adam, re-pack), so the many short kernels of one fill the idle CUs of the others.  The
            # same stream then carries that discriminator's pass of the G update (forward, losses, backward to the fake
            # image), which can start as soon as D_i is updated, while a larger discriminator is still in its own update.
            main = torch.cuda.current_stream()
            if self._side_streams is None:
                self._side_streams = self._make_d_streams()
            errs = []
            for i in reversed(range(self.num_Ds)):  # largest first: it is the critical path
                st = self._side_streams[i]
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    errs.append(self.train_Dnet(i, 0))
            for i in range(self.num_Ds):
                with torch.cuda.stream(self._side_streams[i]):
                    self._g_pass_of_d(i)
            for i in range(self.num_Ds):
                main.wait_stream(self._side_streams[i])
        else:
            # largest first, so that its gradient all-reduce (285 MB for D_NET256) hides behind the smaller
            # discriminators' forward/backward
            errs = [self.train_Dnet(i, 0, defer_step=True) for i in reversed(range(self.num_Ds))]
            self._flush_d_steps()
            for i in range(self.num_Ds):
                self._g_pass_of_d(i)
        kl_loss, errG_total = self._g_backward()
        self.flatG.ema(0.999)
        for e in errs:
            errD_total = errD_total + e
        return errD_total, errG_total, kl_loss

    # -- snapshot image grids (trainer.py:268-295, 511-512, 589-601) ------------------------------------------------------
    def draw_fixed_noise(self, device):
        """fixed_noise (batch_size, Z_DIM) and fixed_eps (batch_size, EMBEDDING_DIM) of the snapshot grids, from a private
        CPU generator seeded with torch.initial_seed(): neither the global CPU generator nor the device's is advanced, so
        a seeded run draws the same training noise, and ends in the same weights, with the snapshots on or off.  (The
        reference fixes z only, from the global generator, and lets CA_NET draw a fresh eps per snapshot.)"""
        g = torch.Generator().manual_seed(torch.initial_seed())
        self.fixed_noise = torch.randn(self.batch_size, cfg.GAN.Z_DIM, generator=g).to(device)
        self.fixed_eps = torch.randn(self.batch_size, cfg.GAN.EMBEDDING_DIM, generator=g).to(device)

    @torch.no_grad()
    def snapshot_images(self, count, real_imgs, txt_embedding):
        """The reference's snapshot pictures: G with the EMA weights, in training mode as the reference runs it (BatchNorm on
        batch statistics), on fixed_noise[:B], the current batch's embeddings and fixed_eps[:B]; then one grid
        (ops.image_grid_uint8, nrow 8, padding 2) of the first min(VIS_COUNT, B) real images of the last scale and one per
        scale of the fake ones.  Returns the uint8 (Hg, Wg, 3) device grids, real grid first; rank 0 also writes them as
        <image_dir>/real_samples.png (overwritten every time) and count_%09d_fake_samples%d.png.  Every rank runs the
        forward pass.  Runs eagerly on the current stream, after the step's side streams have joined: train() calls it
        outside the recorded step, so a plan or graph executor never holds it.
        Deviations: the live weights come back afterwards (as in save()), and so do G's BatchNorm buffers (running_mean,
        running_var, num_batches_tracked) -- the reference lets the snapshot forward move them; here a snapshot leaves
        the training state untouched, so checkpoints do not depend on VIS_COUNT.  self.fake_imgs keeps the snapshot's
        images (NHWC4) as in the reference, except under a captured step, whose self.fake_imgs are the recording's static
        outputs and stay."""
        netG = _unwrap(self.netG)
        B = txt_embedding.shape[0]
        if self.fixed_noise is None:
            self.draw_fixed_noise(txt_embedding.device)
        live = self.flatG.p.clone()
        buffers = [(b, b.clone()) for b in netG.buffers()]
        was_training = netG.training
        load_params(self.netG, self.avg_param_G)
        netG.train()
        try:
            fake_imgs, _, _ = netG(self.fixed_noise[:B], txt_embedding.detach(), self.fixed_eps[:B], True)
        finally:
            netG.train(was_training)
            for b, kept in buffers:
                b.copy_(kept)
            self.flatG.p.copy_(live)
            ops.refresh_packed(self.flatG.params)
        if self._graph is None or self._graph.get('graphs') is None:
            self.fake_imgs = fake_imgs
        num = min(int(cfg.TRAIN.VIS_COUNT), B)
        grids = [ops.image_grid_uint8(real_imgs[-1][:num], nrow=8, padding=2, layout="nchw")]
        grids += [ops.image_grid_uint8(f[:num], nrow=8, padding=2, layout="nhwc") for f in fake_imgs]
        rank0 = not self.distributed or torch.distributed.get_rank() == 0
        if rank0 and getattr(self, 'image_dir', None):
            from PIL import Image
            names = ['real_samples.png'] + ['count_%09d_fake_samples%d.png' % (count, i) for i in range(len(fake_imgs))]
            for name, grid in zip(names, grids):
                Image.fromarray(grid.cpu().numpy()).save(os.path.join(self.image_dir, name))
        return grids

    def train(self):
        start_count = self.build()
        dev = torch.device('cuda', self.gpus[0])
        nz = cfg.GAN.Z_DIM
        noise = torch.empty(self.batch_size, nz, device=dev)
        if cfg.TRAIN.STATE:
            start_epoch, count = self.load_state(cfg.TRAIN.STATE)    # before any recording of the step
        else:
            self.draw_fixed_noise(dev)
            count = start_count
            start_epoch = start_count // max(self.num_batches, 1)
        state_every = int(cfg.TRAIN.STATE_EVERY)
        errD_total = errG_total = kl_loss = None
        for epoch in range(start_epoch, self.max_epoch):
            start_t = time.time()
            for step, data in enumerate(self.data_loader, 0):
                _, real, wrong, emb, labels = self.prepare_data(data)
                noise.normal_(0, 1)
                aug = self.draw_aug(emb.shape[0], dev)      # after the noise; nothing is drawn while TRAIN.DIFFAUG is empty
                errD_total, errG_total, kl_loss = self.train_step(real, wrong, emb, labels, noise[:emb.shape[0]], aug=aug)
                if step == 0 and self.gpus[0] == 0:
                    print('[%d/%d][%d/%d] Loss_D: %.2f Loss_G: %.2f'
                          % (epoch, self.max_epoch, step, self.num_batches, errD_total.item(), errG_total.item()))
                count += 1
                if count % cfg.TRAIN.SNAPSHOT_INTERVAL == 0:
                    self.save(count)
                    if cfg.TRAIN.VIS_COUNT > 0:
                        self.snapshot_images(count, real, emb)
                    self.score_inception(count)
            if errD_total is not None and self.gpus[0] == 0:
                print('[%d/%d][%d] Loss_D: %.2f Loss_G: %.2f Loss_KL: %.2f Time: %.2fs'
                      % (epoch, self.max_epoch, self.num_batches, errD_total.item(), errG_total.item(),
                         kl_loss.item(), time.time() - start_t))
            if state_every > 0 and ((epoch + 1) % state_every == 0 or epoch + 1 == self.max_epoch):
                self.save_state(os.path.join(self.model_dir, 'state.pt'), epoch + 1, count)
        self.save(count)

    def save(self, count):
        """The reference overwrites G's live weights with the EMA copy when it saves and never restores
        them (trainer.py:256, 590-601); the live weights are kept here.  With data-parallel ranks only
        rank 0 writes (the reference lets every rank write the same file names: a race on a shared filesystem); its
        BatchNorm buffers are the ones kept, as DDP's broadcast_buffers would leave them.
        A second deviation lives in snapshot_images: the reference's snapshot forward moves G's BatchNorm running
        statistics (trainer.py:595-597), so its later checkpoints depend on how often it drew pictures; here the buffers
        are restored after that forward and a checkpoint is the same with TRAIN.VIS_COUNT = 0 or not."""
        if self.distributed and torch.distributed.get_rank() != 0:
            return
        live = self.flatG.p.clone()
        save_model(self.netG, self.avg_param_G, self.netsD, count, self.model_dir)
        self.flatG.p.copy_(live)
        ops.refresh_packed(self.flatG.params)

    # -- full training state: an exact resume at an epoch boundary (train_state.py) ------------------
    def save_state(self, path, epoch, count):
        """Everything the next epoch depends on, in one file that rank 0 replaces atomically: the FlatNet state of G and of
        every D (live weights, both Adam moments, G's EMA copy, step counts, learning rates), every BatchNorm buffer, the
        snapshot grids' fixed_noise / fixed_eps, `epoch` (finished epochs) and `count`, every rank's generator states
        (gathered: every rank must call this), and world size, batch size and math mode, which load_state checks.
        Not saved: the Inception rows collected since the last metrics record (a resumed run's next record covers the
        batches since the resume) and a recorded plan or graph (the resumed run records its own)."""
        from . import train_state
        dev = torch.device('cuda', self.gpus[0])
        rng = train_state.gather(train_state.capture_rng(dev), self.distributed)
        if self.distributed and torch.distributed.get_rank() != 0:
            return
        nets = [self.netG] + list(self.netsD)
        state = {"format": train_state.FORMAT, "kind": "condGANTrainer", "epoch": int(epoch), "count": int(count),
                 "world": int(self.world), "batch_size": int(self.batch_size), "act_bf16": bool(ops.ACT_BF16),
                 "math_planes": int(ops.MATH_PLANES),
                 "flats": [train_state.to_cpu(f.state_dict()) for f in [self.flatG] + self.flatsD],
                 "buffers": [{k: b.detach().cpu() for k, b in _unwrap(n).named_buffers()} for n in nets],
                 "fixed_noise": None if self.fixed_noise is None else self.fixed_noise.cpu(),
                 "fixed_eps": None if self.fixed_eps is None else self.fixed_eps.cpu(), "rng": rng}
        train_state.atomic_save(state, path)

    def load_state(self, path):
        """Inverse of save_state, into the networks build() made -> (epoch, count).  The flat buffers are written in place,
        so it may follow build() at any time before the step is recorded; train() calls it there when TRAIN.STATE is set.
        Refused: a state of another world size (the per-rank generator states do not map), batch size, math mode or
        network layout.  With data parallelism every rank reads the file; rank r restores generator state r, and every
        rank gets rank 0's BatchNorm buffers, as a checkpoint keeps them (the others' never reach an output)."""
        from . import train_state
        state = train_state.load(path)
        if state.get("kind") != "condGANTrainer":
            raise ValueError("%s is not a condGANTrainer state (kind %r)" % (path, state.get("kind")))
        rank = torch.distributed.get_rank() if self.distributed else 0
        rng = train_state.rank_entry(state["rng"], rank, self.world, path)
        if int(state["world"]) != self.world:
            raise ValueError("%s was written by %d rank(s) and cannot be resumed by %d" % (path, state["world"], self.world))
        if int(state["batch_size"]) != self.batch_size:
            raise ValueError("%s was written at batch size %d; this run has %d" % (path, state["batch_size"], self.batch_size))
        mode, here = (bool(state["act_bf16"]), int(state["math_planes"])), (bool(ops.ACT_BF16), int(ops.MATH_PLANES))
        if mode != here:
            raise ValueError("%s was written with (ACT_BF16, MATH_PLANES) = %s; this run has %s" % (path, mode, here))
        flats, nets = [self.flatG] + self.flatsD, [self.netG] + list(self.netsD)
        if len(state["flats"]) != len(flats):
            raise ValueError("%s holds %d networks; this run has %d" % (path, len(state["flats"]), len(flats)))
        for k, (f, sd) in enumerate(zip(flats, state["flats"])):       # every layout first: nothing is half loaded
            if [int(n) for n in sd["sizes"]] != f.sizes or ("avg" in sd) != (f.avg is not None):
                raise ValueError("%s: network %d has another parameter layout than this run's" % (path, k))
        for f, sd in zip(flats, state["flats"]):
            f.load_state_dict(sd)
        with torch.no_grad():
            for n, saved in zip(nets, state["buffers"]):
                mine = dict(_unwrap(n).named_buffers())
                if set(mine) != set(saved):
                    raise ValueError("%s: buffers %s do not match this network's" % (path, sorted(set(mine) ^ set(saved))))
                for k, b in mine.items():
                    b.copy_(saved[k])
        dev = self.flatG.p.device
        self.fixed_noise = None if state["fixed_noise"] is None else state["fixed_noise"].to(dev)
        self.fixed_eps = None if state["fixed_eps"] is None else state["fixed_eps"].to(dev)
        train_state.restore_rng(rng, dev)      # last: nothing above may draw after it
        return int(state["epoch"]), int(state["count"])

    # -- evaluation (trainer.py:664-679, 681-825): the PNGs, and with TRAIN.INCEPTION_WEIGHTS set the IS / FID / NLPP that
    # the reference computes only after its early return (gan_metrics.GeneratorScorer)
    def save_singleimages(self, images_u8, filenames, save_dir, split_dir, sentenceID, imsize, sample_idx=0):
        save_singleimages(images_u8, filenames, save_dir, split_dir, sentenceID, imsize, sample_idx)

    @torch.no_grad()
    def evaluate(self, split_dir):
        """G in eval mode over every embedding of every test item -> PNGs under <NET_G dir>/iteration<N>/.
        BatchNorm uses the running statistics (no batch barrier); the [-1,1] -> uint8 HWC conversion is one
        kernel on the NHWC output.  Returns the reference's placeholder metrics (trainer.py:803), or, with an Inception
        model (TRAIN.INCEPTION_WEIGHTS), prints the reference's IS / FID / NLPP line over every fake image against each
        batch's last-branch real images (scored once per batch) and returns [{'mu', 'sigma'} fake, {'mu', 'sigma'} real];
        the noise draws and the PNGs are the same either way."""
        if cfg.TRAIN.NET_G == '':
            print('Error: the path for morels is not found!')
            return None
        if split_dir == 'test':
            split_dir = 'valid'
        dev = torch.device('cuda', self.gpus[0])
        netG = G_NET()
        netG.apply(weights_init)
        netG = _Replica(netG.to(dev), self.gpus)
        netG.load_state_dict(torch.load(cfg.TRAIN.NET_G, map_location='cpu', weights_only=True))
        s_tmp = cfg.TRAIN.NET_G
        iteration = int(s_tmp[s_tmp.rfind('_') + 1:s_tmp.rfind('.')])
        save_dir = '%s/iteration%d' % (s_tmp[:s_tmp.rfind('/')], iteration)
        netG.eval()
        nz = cfg.GAN.Z_DIM
        imsize = cfg.TREE.BASE_SIZE * (2 ** (cfg.TREE.BRANCH_NUM - 1))
        scorer = None
        if self.inception_model is not None:
            from . import gan_metrics
            n_items = len(getattr(self.data_loader, 'dataset', ())) or self.batch_size * len(self.data_loader)
            scorer = gan_metrics.GeneratorScorer(self.inception_model, 10 * n_items, dev)   # ten sentences per item
        for data in self.data_loader:
            imgs, t_embeddings, filenames = data
            t_embeddings = t_embeddings.float().to(dev)
            batch_size = t_embeddings.shape[0]
            noise = torch.empty(batch_size, nz, device=dev)
            if scorer is not None:
                real = imgs[-1].to(dev)
                scorer.add_real(ops.images_from_uint8_hwc(real) if real.dtype == torch.uint8 else real.float())
            for i in range(t_embeddings.size(1)):
                noise.normal_(0, 1)
                fake_imgs, _, _ = netG.module(noise, t_embeddings[:, i, :].contiguous(), None, True)
                if scorer is not None:
                    scorer.add_fake(gan_metrics.nhwc4_as_nchw(fake_imgs[-1]))
                u8 = ops.images_to_uint8_hwc(fake_imgs[-1]).cpu().numpy()
                self.save_singleimages(u8, filenames, save_dir, split_dir, i, imsize, 0)
        if scorer is None:
            return [{'mu': 0, 'sigma': 0}, {'mu': 0, 'sigma': 0}]
        res = scorer.result(10)
        print("total, IS mean:{}, FID mean:{}, NLPP mean:{}".format(res['is_mean'], res['fid'], res['nlpp_mean']))
        (mu_g, sigma_g, _), (mu_r, sigma_r, _) = res['fake_stats'], res['real_stats']
        return [{'mu': mu_g, 'sigma': sigma_g}, {'mu': mu_r, 'sigma': sigma_r}]
