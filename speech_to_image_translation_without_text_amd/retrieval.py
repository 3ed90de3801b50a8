"""Speech-to-image retrieval score of a speech encoder: the class-centre accuracy and AP@50 of the reference's
EvalClass.eval_class and eval_audio_feature (Audio_to_Image/train_audio_encoder.py:219-244, 364-382), on the host in
float64 (the sizes are a few thousand rows of 1024).

    python -m speech_to_image_translation_without_text_amd.retrieval --audio data/birds/test/audio_features_0.pickle \\
        --image data/birds/test/image_features_googlenet_caffe.pickle --data_dir data/birds --split test [--seed 0]

prints and writes (``--out``, default ``<audio pickle dir>/retrieval_<split>.json``) one JSON line with ``accu`` and
``ap50`` in percent.
"""
import argparse
import json
import os
import pickle
import random

import numpy as np

from . import datasets

TOPK = 50


def eval_class(query, target, labels, topk=TOPK):
    """(accuracy %, AP@topk %): the class centres are the means of the query rows of each class; target row i scores
    target_i . centre_c; accuracy is that of the argmax class; for each class the top-k targets by its score are drawn
    and those of that class counted, over all drawn (train_audio_encoder.py:219-244)."""
    query = np.asarray(query, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    lab = lab.reshape(-1)
    if query.ndim != 2 or target.shape != query.shape or lab.shape[0] != query.shape[0]:
        raise ValueError("query %s, target %s and %d labels must agree" % (query.shape, target.shape, lab.shape[0]))
    ncls = int(lab.max()) + 1
    centres = np.stack([query[lab == c].mean(axis=0) for c in range(ncls)])
    scores = target @ centres.T
    accu = float((scores.argmax(axis=1) == lab).mean())
    k = min(topk, scores.shape[0])
    hits = 0
    for c in range(ncls):
        top = np.argsort(scores[:, c])[-k:]
        hits += int((lab[top] == c).sum())
    return accu * 100.0, hits / float(ncls * k) * 100.0


def labels_from_json(path):
    """The class of every item of a split JSON: the integer before the first '.' of its `class`."""
    with open(path) as f:
        meta = json.load(f)
    return [int(str(item["class"]).split(".")[0]) for item in meta["data"]]


def labels_from_filenames(path):
    """The reference's label source: a pickled list of `filenames` such as '001.Black_footed_Albatross/...'."""
    with open(path, "rb") as f:
        names = pickle.load(f)
    return [int(str(n).split(".")[0]) for n in names]


def draw_views(audio, image, seed):
    """One of the 10 rows per item, as eval_audio_feature draws them after random.seed(seed): every audio draw first,
    then every image draw."""
    rng = random.Random(seed)
    n = len(audio)
    a_idx = [rng.randint(0, 9) for _ in range(n)]
    i_idx = [rng.randint(0, 9) for _ in range(n)]
    a = np.stack([np.asarray(audio[i])[j] for i, j in enumerate(a_idx)])
    b = np.stack([np.asarray(image[i])[j] for i, j in enumerate(i_idx)])
    return a, b


def eval_features(audio, image, labels, seed=0, topk=TOPK):
    if not len(audio) == len(image) == len(labels):
        raise ValueError("%d audio items, %d image items and %d labels" % (len(audio), len(image), len(labels)))
    a, b = draw_views(audio, image, seed)
    return eval_class(a, b, labels, topk)


def eval_feature_files(audio_pickle, image_pickle, labels, seed=0, topk=TOPK):
    """eval_audio_feature (train_audio_encoder.py:364-382) on the two pickles (read with the restricted unpickler)."""
    return eval_features(datasets.load_embedding_pickle(audio_pickle), datasets.load_embedding_pickle(image_pickle),
                         labels, seed, topk)


def get_parser():
    p = argparse.ArgumentParser(description="speech-to-image retrieval accuracy and AP@50")
    p.add_argument("--audio", required=True, help="audio_features_<switch>.pickle (N, 10, D)")
    p.add_argument("--image", required=True, help="image feature pickle (N x (10, D))")
    p.add_argument("--data_dir", default=None, help="directory with <split>.json (labels from each item's class)")
    p.add_argument("--split", default="test")
    p.add_argument("--filenames", default=None, help="filenames.pickle to take the labels from instead")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--topk", type=int, default=TOPK)
    p.add_argument("--out", default=None, help="JSON output (default <audio dir>/retrieval_<split>.json)")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.filenames:
        labels = labels_from_filenames(args.filenames)
    elif args.data_dir:
        labels = labels_from_json(os.path.join(args.data_dir, "%s.json" % args.split))
    else:
        raise SystemExit("give --data_dir (split JSON) or --filenames for the labels")
    accu, ap = eval_feature_files(args.audio, args.image, labels, args.seed, args.topk)
    line = json.dumps({"split": args.split, "items": len(labels), "seed": args.seed, "accu": accu, "ap50": ap})
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(args.audio)), "retrieval_%s.json" % args.split)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
    return accu, ap


if __name__ == "__main__":
    main()
