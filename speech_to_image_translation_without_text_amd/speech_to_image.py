"""Spoken sentences -> images: WAV files through the speech encoder into a trained StackGAN-v2 generator.

    python -m speech_to_image_translation_without_text_amd.speech_to_image --model encoder.pt --netG netG_600.pth \\
        --out_dir out --bidirectional a.wav b.wav

Each 16 kHz PCM16 WAV becomes its log-mel (audio.log_mel), its 1024-d sentence embedding (CNNRNN.forward_nhwc, one
utterance per sequence: cap_len = n_frames // 64, so a clip needs at least 64 frames, about 0.65 s), and then G's
last-stage image, written as `<out_dir>/<wav name>.png`.  G runs in .eval() mode as trainer.evaluate runs it; z and the
conditioning-augmentation noise are drawn, in that order, from a CPU generator seeded with --seed, so a run is
reproducible.  --cfg takes the training YAML (G's widths and branch count).
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


@torch.no_grad()
def generate(netG, emb, seed):
    """uint8 (N, H, W, 3) images of the last stage of G for embeddings `emb` (N, 1024)."""
    dev = emb.device
    z, eps = draw_noise(emb.shape[0], seed)
    fake_imgs, _, _ = netG(z.to(dev), emb.contiguous(), eps.to(dev), True)
    return ops.images_to_uint8_hwc(fake_imgs[-1]).cpu().numpy()


def main(argv=None):
    p = argparse.ArgumentParser(description="speech to image")
    p.add_argument("wavs", nargs="+", help="16 kHz PCM16 WAV files")
    p.add_argument("--model", required=True, help="CNNRNN checkpoint")
    p.add_argument("--netG", required=True, help="generator state_dict (netG_<N>.pth)")
    p.add_argument("--out_dir", required=True)
    p.add_argument("--cfg", default=None, help="training YAML of the generator")
    p.add_argument("--bidirectional", action="store_true", default=False)
    p.add_argument("--rnn_layers", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    if args.cfg:
        cfg_from_file(args.cfg)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = load_encoder(args.model, args.bidirectional, args.rnn_layers, dev)
    emb = embed(model, read_wavs(args.wavs))
    images = generate(load_generator(args.netG, dev), emb, args.seed)
    os.makedirs(args.out_dir, exist_ok=True)
    for path, img in zip(args.wavs, images):
        out = os.path.join(args.out_dir, os.path.splitext(os.path.basename(path))[0] + ".png")
        Image.fromarray(img).save(out)
        print(out)


if __name__ == "__main__":
    main()
