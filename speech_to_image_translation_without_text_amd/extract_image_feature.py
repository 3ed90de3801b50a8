"""Images -> the 10-view GoogLeNet pool5 feature pickles the speech encoder is trained and scored against
(Audio_to_Image/prepare_image_feature.py:121-160), on the gfx950 kernels instead of Caffe.

    python -m speech_to_image_translation_without_text_amd.extract_image_feature \\
        --weights bvlc_googlenet.caffemodel --dataset birds --data_dir data/birds [--splits train,test] \\
        [--mean_file ilsvrc_2012_mean.npy] [--batch_size 48]

For each split it reads `<data_dir>/<split>.json` and finds each item's image at
  * birds:   `image_base_path/images/<item["image"]>`  (prepare_image_feature.py:135)
  * flowers: `image_base_path/<item["img"]>`           (:157)
(a relative `image_base_path` is taken relative to the working directory, as the reference does) and writes ONE
`pickle.dump` of a list of (10, 1024) float32 arrays, one per item in JSON order:
  * birds:   the JSON's `image_feature_path` if it has one, else `<data_dir>/<split>/image_features_googlenet_caffe.pickle`
  * flowers: `<data_dir>/<split>_image_feature_caffe.pickle`.
Images are decoded with PIL (convert("RGB")) on up to MAX_READERS threads while the GPU runs the previous chunk.
"""
import argparse
import json
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import googlenet

MAX_READERS = 16


def split_items(data_dir, split, dataset):
    """(image paths, output pickle path) of one split."""
    with open(os.path.join(data_dir, "%s.json" % split)) as f:
        meta = json.load(f)
    base = meta["image_base_path"]
    if dataset == "birds":
        paths = [os.path.join(base, "images", d["image"]) for d in meta["data"]]
        out = meta.get("image_feature_path") or os.path.join(data_dir, split, "image_features_googlenet_caffe.pickle")
    elif dataset == "flowers":
        paths = [os.path.join(base, d["img"]) for d in meta["data"]]
        out = os.path.join(data_dir, "%s_image_feature_caffe.pickle" % split)
    else:
        raise ValueError("unknown dataset %r (birds or flowers)" % dataset)
    return paths, out


def extract_paths(net, paths, batch_size=googlenet.MAX_BATCH, workers=MAX_READERS):
    """(N, 10, 1024) float32 features of the image files, decoding chunk i + 1 while chunk i runs."""
    out = np.empty((len(paths), googlenet.VIEWS, googlenet.FEATURES), dtype=np.float32)
    chunks = [paths[s:s + batch_size] for s in range(0, len(paths), batch_size)]
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_READERS, workers))) as pool, \
            ThreadPoolExecutor(max_workers=1) as ahead:
        def decode(chunk):
            return list(pool.map(googlenet.read_image, chunk))
        pending = ahead.submit(decode, chunks[0]) if chunks else None
        s = 0
        for i in range(len(chunks)):
            images = pending.result()
            pending = ahead.submit(decode, chunks[i + 1]) if i + 1 < len(chunks) else None
            out[s:s + len(images)] = net(images, batch_size).numpy()
            s += len(images)
    return out


def write_feature_pickle(feats, path):
    """The reference's format: one pickle.dump of a list of (10, 1024) float32 arrays."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump([np.ascontiguousarray(a) for a in feats], f)


def extract_split(net, data_dir, split, dataset, batch_size=googlenet.MAX_BATCH):
    paths, out = split_items(data_dir, split, dataset)
    if not paths:
        raise ValueError("%s split of %s has no items" % (split, data_dir))
    feats = extract_paths(net, paths, batch_size)
    write_feature_pickle(feats, out)
    return feats, out


def get_parser():
    p = argparse.ArgumentParser(description="extract_image_feature")
    p.add_argument("--weights", required=True, help="bvlc_googlenet.caffemodel")
    p.add_argument("--dataset", choices=["birds", "flowers"], default="birds")
    p.add_argument("--data_dir", type=str, default=None, help="directory with <split>.json (default ./data/<dataset>)")
    p.add_argument("--splits", type=str, default="train,test")
    p.add_argument("--mean_file", type=str, default="", help=".npy mean image (3, H, W), BGR; averaged over H and W")
    p.add_argument("--batch_size", type=int, default=googlenet.MAX_BATCH,
                   help="images per GPU chunk (1..%d)" % googlenet.MAX_BATCH)
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not 1 <= args.batch_size <= googlenet.MAX_BATCH:
        raise SystemExit("--batch_size must be in 1..%d" % googlenet.MAX_BATCH)
    data_dir = args.data_dir or os.path.join(".", "data", args.dataset)
    mean = googlenet.mean_from_file(args.mean_file) if args.mean_file else googlenet.MEAN_BGR
    dev = torch.device("cuda", torch.cuda.current_device())
    net = googlenet.GoogLeNetFeatures(args.weights, dev, mean)
    for split in args.splits.split(","):
        feats, out = extract_split(net, data_dir, split, args.dataset, args.batch_size)
        print("%s: %d images -> %s" % (split, len(feats), out))


if __name__ == "__main__":
    main()
