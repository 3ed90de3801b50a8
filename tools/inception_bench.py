"""Inception-v3 scorer timing (GPU box only): the stacked pass over 2B = 48 images of 256 px, every convolution of it
alone grouped by layer class (TFLOP/s against the 157.3 TFLOP/s fp32 matrix peak of the MI355X), and the cfg/birds_3stages.yml
train step with and without the pass.  Seeded random weights in torchvision layout (the timing does not depend on them).

Usage:  python tools/inception_bench.py [--batch 24] [--reps 10]
"""
import argparse
import collections
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_to_image_translation_without_text_amd import _lib, inception as I, model, trainer as T  # noqa: E402
from speech_to_image_translation_without_text_amd.miscc.config import cfg, cfg_from_file  # noqa: E402

PEAK_TF = 157.3


def seeded_state_dict(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in I.state_dict_shapes(aux_logits=False, num_batches_tracked=False).items():
        if k.endswith("running_var") or k.endswith("bn.weight"):
            sd[k] = torch.rand(shp, generator=g) + 0.5
        elif k.endswith("weight"):
            fan = 1
            for s in shp[1:]:
                fan *= s
            sd[k] = torch.randn(shp, generator=g) * (2.0 / fan) ** 0.5
        else:
            sd[k] = torch.randn(shp, generator=g) * 0.1
    return sd


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_class(name, g):
    cin, cout, kh, kw, sh, sw, ph, pw = g
    if name.startswith("Conv2d_"):
        return "stem"
    if name == "fc":
        return "fc"
    if sh == 2:
        return "3x3 s2"
    if kh == kw:
        return "%dx%d" % (kh, kw)
    return "1x%d / %dx1" % (max(kh, kw), max(kh, kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24, help="images per side: the pass scores 2 x batch")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.require_device()
    B = args.batch
    incep = model.INCEPTION_V3(weights=seeded_state_dict())
    net = incep.net(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    fake = torch.rand(B, 3, 256, 256, device=dev, generator=gen) * 2 - 1
    real = torch.rand(B, 3, 256, 256, device=dev, generator=gen) * 2 - 1
    soft, pool3 = torch.empty(2 * B, 1000, device=dev), torch.empty(2 * B, 2048, device=dev)
    pass_ms = timed(lambda: net.run([fake, real], soft, pool3), args.reps)

    # every launch of one pass, timed alone at its own descriptor
    records = []
    orig = net.conv

    def rec(name, x, Bx, H, W, y=None, coff=0, relu=True, ldx=None):
        out = orig(name, x, Bx, H, W, y, coff, relu, ldx)
        records.append((name, x, Bx, H, W, out[0], coff, relu, ldx))
        return out
    net.conv = rec
    net.run([fake, real], soft, pool3)
    net.conv = orig
    torch.cuda.synchronize()
    arch = dict(I.architecture(aux_logits=False), fc=(2048, 1000, 1, 1, 1, 1, 0, 0))
    classes = collections.OrderedDict()
    conv_ms, flops_all = 0.0, 0.0
    for name, x, Bx, H, W, y, coff, relu, ldx in records:
        ms = timed(lambda: orig(name, x, Bx, H, W, y, coff, relu, ldx), args.reps)
        g = arch[name]
        Ho, Wo = (H + 2 * g[6] - g[2]) // g[4] + 1, (W + 2 * g[7] - g[3]) // g[5] + 1
        fl = 2.0 * Bx * Ho * Wo * g[1] * g[0] * g[2] * g[3]
        c = classes.setdefault(layer_class(name, g), [0, 0.0, 0.0])
        c[0] += 1
        c[1] += ms
        c[2] += fl
        conv_ms += ms
        flops_all += fl
    print("pass over %d images (256 px -> 299): %.3f ms, %.1f GFLOP in convolutions, %.1f TFLOP/s over the pass"
          % (2 * B, pass_ms, flops_all / 1e9, flops_all / pass_ms / 1e9))
    print("sum of the convolutions alone: %.3f ms (%.1f TFLOP/s, %.0f%% of %.1f)"
          % (conv_ms, flops_all / conv_ms / 1e9, 100 * flops_all / conv_ms / 1e9 / PEAK_TF, PEAK_TF))
    print("%-12s %5s %9s %9s %8s" % ("class", "convs", "ms", "GFLOP", "TFLOP/s"))
    for k, (n, ms, fl) in sorted(classes.items(), key=lambda kv: -kv[1][1]):
        print("%-12s %5d %9.3f %9.1f %8.1f" % (k, n, ms, fl / 1e9, fl / ms / 1e9))

    # the train step without and with the pass
    cfg_from_file(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "cfg", "birds_3stages.yml"))
    cfg.TRAIN.BATCH_SIZE = B
    torch.manual_seed(0)
    netG = model.G_NET()
    netG.apply(T.weights_init)
    netsD = [c() for c in (model.D_NET64, model.D_NET128, model.D_NET256)]
    for d in netsD:
        d.apply(T.weights_init)
    netG.to(dev)
    for d in netsD:
        d.to(dev)
    tr = T.condGANTrainer(None, None, 256, False)
    tr.build(netG, netsD)
    reals = [torch.rand(B, 3, 64 << i, 64 << i, device=dev, generator=gen) * 2 - 1 for i in range(3)]
    wrong = [torch.rand(B, 3, 64 << i, 64 << i, device=dev, generator=gen) * 2 - 1 for i in range(3)]
    emb = torch.randn(B, 1024, device=dev, generator=gen)
    labels = (torch.arange(B, device=dev) % 3).to(torch.int32)
    noise = torch.randn(B, 100, device=dev, generator=gen)
    eps = torch.randn(B, 128, device=dev, generator=gen)

    def step():
        tr.train_step(reals, wrong, emb, labels, noise, eps)
    step_ms = timed(step, args.steps)
    tr.enable_inception(incep)
    step_incep_ms = timed(step, args.steps)
    tr._inception_rows = []
    print("train step (B = %d, eager): %.3f ms without the pass, %.3f ms with it (+%.3f ms)"
          % (B, step_ms, step_incep_ms, step_incep_ms - step_ms))
    print(json.dumps(dict(images=2 * B, pass_ms=round(pass_ms, 3), conv_gflop=round(flops_all / 1e9, 2),
                          conv_alone_ms=round(conv_ms, 3), step_ms=round(step_ms, 3),
                          step_with_pass_ms=round(step_incep_ms, 3),
                          classes={k: dict(convs=n, ms=round(ms, 3), tflops=round(fl / ms / 1e9, 1))
                                   for k, (n, ms, fl) in classes.items()})))


if __name__ == "__main__":
    main()
