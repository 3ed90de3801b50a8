"""Spoken sentences -> images: WAV files through the speech encoder into a trained StackGAN-v2 generator.

    python -m speech_to_image_translation_without_text_amd.speech_to_image --model encoder.pt --netG netG_600.pth \\
        --out_dir out --bidirectional a.wav b.wav

Each 16 kHz PCM16 WAV becomes its log-mel (audio.log_mel), its 1024-d sentence embedding (CNNRNN.forward_nhwc, one
utterance per sequence: cap_len = n_frames // 64, so a clip needs at least 64 frames, about 0.65 s), and then G's
last-stage image, written as `<out_dir>/<wav name>.png`.  G runs in .eval() mode as trainer.evaluate runs it; z and the
conditioning-augmentation noise are drawn, in that order, from a CPU generator seeded with --seed, so a run is
reproducible.  --cfg takes the training YAML (G's widths and branch count).  --resample takes WAVs of any rate from 4 to
192 kHz, PCM or float, 1 to 8 channels, and converts them to 16 kHz mono on the GPU first (audio.to_16k).

    ... --interpolate 10 a.wav b.wav

takes exactly two WAVs and writes the reference's interpolation strip (StackGAN_v2/interpolation.py:54-88): STEPS + 1
embeddings on the line between the two utterances, row i = a * (i / STEPS) + b * (1 - i / STEPS) (so image 0 is b's and
the last one a's), through G as one batch with ONE z and ONE eps shared by every row, as `<out_dir>/interp_<i>.png` and
side by side, min-max normalised over the strip, as `<out_dir>/interp_grid.png` (ops.image_grid_uint8).
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from . import audio, ops
from .extract_audio_feature import MIN_FRAMES, load_encoder, read_wavs
from .miscc.config import cfg, cfg_from_file


def embed(model, waves):
    """(N, 1024) sentence embeddings of the waveforms on the encoder's device."""
    dev = next(model.parameters()).device
    logspec, nf = audio.log_mel(waves, layout="nhwc", device=dev)
    short = [i for i, n in enumerate(nf) if n < MIN_FRAMES]
    if short:
        raise ValueError("utterances %s are shorter than %d frames" % (short, MIN_FRAMES))
    cap = nf // MIN_FRAMES
    order = np.argsort(-cap, kind="stable")
    sent = model.forward_nhwc(logspec.index_select(0, torch.from_numpy(order).to(dev)), cap[order].tolist())[1]
    out = torch.empty_like(sent)
    out[torch.from_numpy(order).to(dev)] = sent
    return out


def draw_noise(n, seed):
    """(z (n, Z_DIM), eps (n, EMBEDDING_DIM)) from a CPU generator seeded with `seed`, z first."""
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn(n, cfg.GAN.Z_DIM, generator=g)
    eps = torch.randn(n, cfg.GAN.EMBEDDING_DIM, generator=g)
    return z, eps


def load_generator(path, device):
    from .model import G_NET
    from .trainer import weights_init
    netG = G_NET()
    netG.apply(weights_init)
    state = torch.load(path, map_location="cpu", weights_only=True)
    if next(iter(state)).startswith("module."):
        state = {k[len("module."):]: v for k, v in state.items()}
    netG.load_state_dict(state)
    return netG.to(device).eval()


def interpolation_embeddings(emb_a, emb_b, steps):
    """(steps + 1, D) rows emb_a * (i / steps) + emb_b * (1 - i / steps), the reference's order
    (interpolation.py:69-71): row 0 is emb_b, the last row emb_a."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("interpolation needs at least one step, got %d" % steps)
    a, b = emb_a.reshape(1, -1), emb_b.reshape(1, -1)
    alpha = (torch.arange(steps + 1, dtype=a.dtype, device=a.device) / steps).reshape(-1, 1)
    return a * alpha + b * (1 - alpha)


@torch.no_grad()
def interpolate(netG, emb_a, emb_b, steps, seed):
    """G's last-stage NHWC4 images (steps + 1, H, W, 4) of interpolation_embeddings(emb_a, emb_b, steps), one batch, with
    the single (z, eps) draw of `seed` repeated for every row (interpolation.py:74, 87: one noise for the strip)."""
    emb = interpolation_embeddings(emb_a, emb_b, steps).contiguous()
    dev = emb.device
    z, eps = draw_noise(1, seed)
    n = emb.shape[0]
    fake_imgs, _, _ = netG(z.repeat(n, 1).to(dev), emb, eps.repeat(n, 1).to(dev), True)
    return fake_imgs[-1]


@torch.no_grad()
def generate(netG, emb, seed):
    """uint8 (N, H, W, 3) images of the last stage of G for embeddings `emb` (N, 1024)."""
    dev = emb.device
    z, eps = draw_noise(emb.shape[0], seed)
    fake_imgs, _, _ = netG(z.to(dev), emb.contiguous(), eps.to(dev), True)
    return ops.images_to_uint8_hwc(fake_imgs[-1]).cpu().numpy()


def get_parser():
    p = argparse.ArgumentParser(description="speech to image")
    p.add_argument("wavs", nargs="+", help="16 kHz PCM16 WAV files (any rate and PCM / float format with --resample)")
    p.add_argument("--model", required=True, help="CNNRNN checkpoint")
    p.add_argument("--netG", required=True, help="generator state_dict (netG_<N>.pth)")
    p.add_argument("--out_dir", required=True)
    p.add_argument("--cfg", default=None, help="training YAML of the generator")
    p.add_argument("--bidirectional", action="store_true", default=False)
    p.add_argument("--rnn_layers", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--interpolate", type=int, default=None, metavar="STEPS",
                   help="two WAVs: write the STEPS + 1 images between them (interp_<i>.png, interp_grid.png)")
    p.add_argument("--resample", action="store_true", default=False,
                   help="accept WAVs of any rate (4-192 kHz), PCM 8/16/24/32-bit or float 32/64-bit, 1-8 channels: "
                        "decoded, mixed down and resampled to 16 kHz on the GPU (audio.to_16k)")
    return p


def main(argv=None):
    p = get_parser()
    args = p.parse_args(argv)
    if args.interpolate is not None:
        if len(args.wavs) != 2:
            p.error("--interpolate takes exactly two WAV files, got %d" % len(args.wavs))
        if args.interpolate < 1:
            p.error("--interpolate needs STEPS >= 1")
    if args.cfg:
        cfg_from_file(args.cfg)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = load_encoder(args.model, args.bidirectional, args.rnn_layers, dev)
    emb = embed(model, read_wavs(args.wavs, resample=args.resample))
    netG = load_generator(args.netG, dev)
    os.makedirs(args.out_dir, exist_ok=True)
    if args.interpolate is not None:
        imgs = interpolate(netG, emb[0], emb[1], args.interpolate, args.seed)
        singles = ops.images_to_uint8_hwc(imgs).cpu().numpy()
        strip = ops.image_grid_uint8(imgs, nrow=imgs.shape[0], padding=2, layout="nhwc").cpu().numpy()
        outs = [(os.path.join(args.out_dir, "interp_%d.png" % i), img) for i, img in enumerate(singles)]
        outs.append((os.path.join(args.out_dir, "interp_grid.png"), strip))
        for out, img in outs:
            Image.fromarray(img).save(out)
            print(out)
        return
    images = generate(netG, emb, args.seed)
    for path, img in zip(args.wavs, images):
        out = os.path.join(args.out_dir, os.path.splitext(os.path.basename(path))[0] + ".png")
        Image.fromarray(img).save(out)
        print(out)


if __name__ == "__main__":
    main()
