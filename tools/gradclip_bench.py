"""Times the gradient-norm pass of the fused optimiser and the training step with and without it, with HIP events: median
of --iters after --warmup.

  * s2i_grad_sumsq + s2i_grad_clip_scale alone on the head's flat layout (RNN.*, 8 tensors) and on the whole bidirectional
    encoder's, in microseconds and in GB/s of the gradient buffer read once;
  * the three-launch guarded optimiser step (FlatNet.adam with max_norm) next to s2i_increment + one Adam launch;
  * one EncoderTrainer.step at B = 64, T = 2048 with fused_adam alone, with clip_grad and with accum = 2.

--package_root DIR imports the package from another checkout (the parent commit, built): only the fused_adam step is timed
there, which is the figure the options-off step is compared with.  Writes profiles/gradclip_bench.json (or --out) and
prints it.  No thresholds: nobody has measured these numbers before.

    python tools/gradclip_bench.py [--iters 20] [--warmup 5] [--batch 64] [--package_root DIR] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--package_root", type=str, default=ROOT)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "gradclip_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, args.package_root)
    from speech_to_image_translation_without_text_amd import _lib, ops
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    from speech_to_image_translation_without_text_amd.trainer import FlatNet
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(1234)
    net = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).eval()
    here = os.path.abspath(args.package_root) == ROOT
    result = {"device": torch.cuda.get_device_name(dev), "iters": args.iters, "warmup": args.warmup, "T": 2048,
              "B": args.batch, "this_checkout": here}
    if here:
        for name, pick in (("head", lambda m: list(m.RNN.parameters())), ("encoder", lambda m: list(m.parameters()))):
            model = copy.deepcopy(net).to(dev)
            flat = FlatNet(model, 1e-3, betas=(0.9, 0.999), weight_decay=1e-5, params=pick(model))
            flat.g.normal_(0.0, 1e-2)
            flat.adam(1.0, max_norm=1.0)                    # builds the layout
            c = flat.clip

            def norm_pass():
                ops.grad_sumsq(flat.g, c)
                ops.grad_clip_scale(c, 1.0, 1.0, None)

            nbytes = 4.0 * sum(flat.sizes)
            r = {"tensors": len(flat.sizes), "elements": sum(flat.sizes), "chunks": c.nchunks}
            r["sumsq_clip_scale"] = timed(norm_pass, args.iters, args.warmup)
            r["sumsq_clip_scale_gbs"] = nbytes / r["sumsq_clip_scale"]["median_ms"] / 1e6
            r["sumsq_alone"] = timed(lambda: ops.grad_sumsq(flat.g, c), args.iters, args.warmup)
            r["sumsq_alone_gbs"] = nbytes / r["sumsq_alone"]["median_ms"] / 1e6
            r["guarded_adam"] = timed(lambda: flat.adam(1.0, max_norm=1.0), args.iters, args.warmup)
            r["increment_adam"] = timed(lambda: flat.adam(1.0), args.iters, args.warmup)
            result[name] = r
            del flat, model
    g = torch.Generator().manual_seed(1)
    B = args.batch
    mel = (-80.0 * torch.rand(B, 1, 2048, 40, generator=g)).to(dev)
    lens = sorted(torch.randint(10, 33, (B,), generator=g).tolist(), reverse=True)
    image = torch.randn(B, 1024, generator=g).to(dev)
    label = torch.randint(0, 20, (B,), generator=g).to(dev)
    variants = [("step_fused_adam", dict(fused_adam=True))]
    if here:
        variants += [("step_clip_grad", dict(clip_grad=1.0)), ("step_clip_grad_accum2", dict(clip_grad=1.0, accum=2))]
    for name, kw in variants:
        trainer = EncoderTrainer(copy.deepcopy(net).to(dev), jel=True, **kw)
        result[name] = timed(lambda: trainer.step(mel, lens, image, label), args.iters, args.warmup)
        del trainer
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
