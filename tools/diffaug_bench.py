"""What TRAIN.DIFFAUG costs: ms_per_step of the fp32 train step at the cfg/birds_3stages.yml shapes with the policy empty and
with 'color,translation,cutout', from one process, one trainer and alternating blocks of steps, beside the byte estimate
of the extra traffic timed at the bandwidth the existing layout kernel (nchw3_to_nhwc4_kernel) reaches on the same images.

  python tools/diffaug_bench.py [--batch 24] [--steps 20] [--rounds 3] [--policy color,translation,cutout]

Prints one JSON line.  The policy-off figure is the step every other benchmark measures; on minus off is the feature."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="alternating off / on blocks")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--policy", default="color,translation,cutout")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from bench import synthetic_batch
    from speech_to_image_translation_without_text_amd import model, ops, trainer as T
    from speech_to_image_translation_without_text_amd.miscc.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(ROOT, "speech_to_image_translation_without_text_amd", "cfg", "birds_3stages.yml"))
    B = cfg.TRAIN.BATCH_SIZE = args.batch
    policy = ops.diffaug_policy(args.policy)
    torch.manual_seed(0)
    netG = model.G_NET()
    netG.apply(T.weights_init)
    netsD = []
    for cls in (model.D_NET64, model.D_NET128, model.D_NET256):
        d = cls()
        d.apply(T.weights_init)
        netsD.append(d.to(dev))
    tr = T.condGANTrainer(None, None, 256, False)
    tr.build(netG.to(dev), netsD)
    batch, gen = synthetic_batch(B, dev, 1)
    noise = torch.empty(B, cfg.GAN.Z_DIM, device=dev)
    eps = torch.empty(B, cfg.GAN.EMBEDDING_DIM, device=dev)

    def block(spec, steps):
        cfg.TRAIN.DIFFAUG = spec
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            noise.normal_(generator=gen)
            eps.normal_(generator=gen)
            aug = tr.draw_aug(B, dev)
            out = tr.train_step(batch["real"], batch["wrong"], batch["emb"].detach().requires_grad_(True), batch["labels"],
                                noise, eps, aug=aug)
        torch.cuda.synchronize()
        losses = [float(v) for v in out]
        if not all(abs(v) < 1e6 for v in losses):
            raise RuntimeError("non-finite losses: %s" % losses)
        return (time.perf_counter() - t0) / steps * 1e3

    for spec in ("", args.policy):
        block(spec, args.warmup)
    off, on = [], []
    for _ in range(args.rounds):
        off.append(block("", args.steps))
        on.append(block(args.policy, args.steps))
    cfg.TRAIN.DIFFAUG = ""

    # the operators alone, on the stacked (real | wrong | fake) batch of each scale
    sizes = (64, 128, 256)
    imgs = {s: torch.rand(3 * B, 3, s, s, device=dev) * 2 - 1 for s in sizes}
    tables = {s: torch.rand(3 * B, 8, device=dev) for s in sizes}
    grads = {s: torch.randn(B, s, s, 4, device=dev) for s in sizes}
    plain_ms = {s: event_ms(lambda s=s: ops.ToNHWC.apply(imgs[s], 4)) for s in sizes}
    fused_ms = {s: event_ms(lambda s=s: ops.DiffAugToNHWC.apply(imgs[s], tables[s], policy)) for s in sizes}

    def backward_of(fn, s):
        x = imgs[s][:B].clone().requires_grad_(True)
        y = fn(x)
        return lambda: torch.autograd.grad(y, x, grads[s], retain_graph=True)
    plain_bwd_ms = {s: event_ms(backward_of(lambda x: ops.ToNHWC.apply(x, 4), s)) for s in sizes}
    fused_bwd_ms = {s: event_ms(backward_of(lambda x, s=s: ops.DiffAugToNHWC.apply(x, tables[s][:B], policy), s)) for s in sizes}
    layout_bytes = sum(3 * B * s * s * (12 + 16) for s in sizes)              # NCHW fp32 read, NHWC4 fp32 written
    layout_gbs = layout_bytes / (sum(plain_ms.values()) * 1e-3) / 1e9
    # the extra traffic of the colour stage: the forward reduction reads the raw images of all four passes per
    # discriminator (3 B stacked + B in the generator update), the backward reduction the NHWC4 gradient of the one pass
    # that has a backward
    extra_bytes = sum(4 * B * 3 * s * s * 4 + B * s * s * 16 for s in sizes) if policy & 1 else 0
    est_ms = extra_bytes / (layout_gbs * 1e9) * 1e3
    ms_off, ms_on = min(off), min(on)
    line = {
        "metric": "fp32 train step at cfg/birds_3stages.yml shapes, TRAIN.DIFFAUG off / on, same process",
        "batch": B, "policy": args.policy, "steps_per_block": args.steps,
        "ms_per_step": {"off": round(ms_off, 3), "on": round(ms_on, 3)},
        "ms_per_step_blocks": {"off": [round(v, 3) for v in off], "on": [round(v, 3) for v in on]},
        "on_minus_off_ms": round(ms_on - ms_off, 3), "on_over_off": round(ms_on / ms_off, 4),
        "extra_bytes_per_step": extra_bytes, "layout_kernel_gbs": round(layout_gbs, 1),
        "estimate_ms": round(est_ms, 4), "on_minus_off_over_estimate": round((ms_on - ms_off) / est_ms, 2) if est_ms else None,
        "operator_ms_3B": {str(s): {"to_nhwc": round(plain_ms[s], 4), "diffaug_to_nhwc": round(fused_ms[s], 4)} for s in sizes},
        "operator_backward_ms_B": {str(s): {"to_nhwc": round(plain_bwd_ms[s], 4), "diffaug_to_nhwc": round(fused_bwd_ms[s], 4)}
                                   for s in sizes},
        "note": "ms_per_step is the fastest block of each setting (blocks alternate off / on); operator_* times include the "
                "host's enqueue and torch's autograd dispatch",
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
