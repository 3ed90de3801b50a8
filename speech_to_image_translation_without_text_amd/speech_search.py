"""Spoken sentences -> the images of a collection they describe: WAV files through the speech encoder, ranked against
the GoogLeNet features of a split on the GPU.

    python -m speech_to_image_translation_without_text_amd.speech_search --model encoder.pt --bidirectional \\
        --image data/birds/test/image_features_googlenet_caffe.pickle --dataset birds --data_dir data/birds --split test \\
        --topk 10 [--views all] [--cosine] [--resample] [--out hits.jsonl] a.wav b.wav

Each WAV becomes its 1024-d sentence embedding exactly as speech_to_image makes it (read_wavs -> speech_to_image.embed:
16 kHz PCM16, or anything audio.read_audio accepts with --resample; a clip under 64 frames is refused), and the
embeddings go through retrieval.Gallery.search.  The gallery is the image-feature pickle of the split (N items x 10
views x 1024): one row per image, the mean of its views (default), or with --views all one row per view.  Scores are dot
products, as the encoder's loss and retrieval.eval_class score, or cosines with --cosine.  Image paths come from the
split JSON (extract_image_feature.split_items), so the pickle must hold exactly as many items as the JSON.

One JSON line per WAV is printed (and written to --out):

    {"wav": "a.wav", "hits": [{"rank": 1, "image": "<path>", "view": null, "score": 12.5}, ...]}

--topk is clipped to the number of gallery rows and may be at most 64.
"""
import argparse
import json
import os

import torch

from . import datasets
from .extract_audio_feature import load_encoder, read_wavs
from .extract_image_feature import split_items
from .retrieval import GALLERY_CHUNK_ROWS, Gallery
from .speech_to_image import embed


def load_gallery(image_pickle, data_dir, split, dataset, device, views="mean", cosine=False,
                 chunk_rows=GALLERY_CHUNK_ROWS):
    """(Gallery, image paths) of one split; the pickle and the split JSON must agree on the number of items."""
    paths, _ = split_items(data_dir, split, dataset)
    features = datasets.load_embedding_pickle(image_pickle)
    if len(features) != len(paths):
        raise ValueError("%s holds %d items but %s lists %d images"
                         % (image_pickle, len(features), os.path.join(data_dir, "%s.json" % split), len(paths)))
    return Gallery(features, device, views=views, cosine=cosine, chunk_rows=chunk_rows), paths


def hit_lines(wavs, paths, scores, items, views):
    """The JSON-ready records of a search result (host values)."""
    scores, items = scores.cpu().tolist(), items.cpu().tolist()
    views = views.cpu().tolist() if views is not None else None
    lines = []
    for i, wav in enumerate(wavs):
        hits = [{"rank": r + 1, "image": paths[items[i][r]], "view": views[i][r] if views is not None else None,
                 "score": scores[i][r]} for r in range(len(items[i]))]
        lines.append({"wav": wav, "hits": hits})
    return lines


def get_parser():
    p = argparse.ArgumentParser(description="search an image gallery by speech")
    p.add_argument("wavs", nargs="+", help="16 kHz PCM16 WAV files (any rate and PCM / float format with --resample)")
    p.add_argument("--model", required=True, help="CNNRNN checkpoint")
    p.add_argument("--image", required=True, help="image feature pickle of the split (N x (10, 1024))")
    p.add_argument("--dataset", choices=["birds", "flowers"], default="birds")
    p.add_argument("--data_dir", required=True, help="directory with <split>.json (the image paths)")
    p.add_argument("--split", default="test")
    p.add_argument("--bidirectional", action="store_true", default=False)
    p.add_argument("--rnn_layers", type=int, default=1)
    p.add_argument("--topk", type=int, default=10, help="hits per WAV (clipped to the gallery; at most 64)")
    p.add_argument("--views", choices=["mean", "all"], default="mean",
                   help="mean: one row per image, the mean of its views; all: one row per view")
    p.add_argument("--cosine", action="store_true", default=False, help="cosine similarity instead of the dot product")
    p.add_argument("--chunk_rows", type=int, default=GALLERY_CHUNK_ROWS, help="gallery rows scored per launch")
    p.add_argument("--resample", action="store_true", default=False,
                   help="accept WAVs of any rate (4-192 kHz), PCM 8/16/24/32-bit or float 32/64-bit, 1-8 channels: "
                        "decoded, mixed down and resampled to 16 kHz on the GPU (audio.to_16k)")
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    return p


def main(argv=None):
    p = get_parser()
    args = p.parse_args(argv)
    if args.topk < 1:
        p.error("--topk must be >= 1")
    dev = torch.device("cuda", torch.cuda.current_device())
    gallery, paths = load_gallery(args.image, args.data_dir, args.split, args.dataset, dev, args.views, args.cosine,
                                  args.chunk_rows)
    model = load_encoder(args.model, args.bidirectional, args.rnn_layers, dev)
    with torch.no_grad():
        emb = embed(model, read_wavs(args.wavs, resample=args.resample))
    lines = hit_lines(args.wavs, paths, *gallery.search(emb, args.topk))
    text = [json.dumps(line) for line in lines]
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(t + "\n" for t in text))
    for t in text:
        print(t)
    return lines


if __name__ == "__main__":
    main()
