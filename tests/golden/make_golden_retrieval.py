"""Generate tests/golden/retrieval.npz from the REFERENCE's retrieval score (runs only in the build container).

The reference's Audio_to_Image/train_audio_encoder.py is imported with in-memory stand-ins for the absent h5py,
tensorboardX, librosa and torchvision (none of them is on the scoring path) and scipy.signal's old window names, and
its EvalClass.eval_class (train_audio_encoder.py:219-244) and eval_audio_feature (:364-382, after random.seed(s)) run on seeded float64 arrays.
Only the seeds, shapes and results are stored: the tests regenerate the arrays with the functions below.

Usage:  python tests/golden/make_golden_retrieval.py            (writes next to this file)
"""
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/Audio_to_Image"

# eval_class cases: (seed, classes, rows per class: "equal" k or "unequal", dim, topk)
CLASS_CASES = [
    (1, 10, 8, 64, 50),          # N = 80 > topk
    (2, 7, "unequal", 32, 50),   # unequal class sizes, N < topk
    (3, 200, 3, 128, 50),        # 200 classes (CUB's test split has 50, the whole set 200)
    (4, 5, "unequal", 16, 5),    # small topk
]
# eval_audio_feature cases: (seed of the arrays, seed of the draws, classes, items, dim)
FILE_CASES = [(11, 0, 12, 90, 48), (12, 1234, 30, 200, 64)]


def class_arrays(seed, classes, per, dim):
    """query (N, dim), target (N, dim), labels (N,) with class-correlated rows and CUB-style labels 1..classes."""
    rng = np.random.default_rng(seed)
    counts = [per] * classes if per != "unequal" else list(rng.integers(1, 9, classes))
    labels = np.concatenate([np.full(c, k + 1) for k, c in enumerate(counts)])
    rng.shuffle(labels)
    centre = rng.standard_normal((classes + 1, dim))
    query = centre[labels] + 1.5 * rng.standard_normal((labels.size, dim))
    target = centre[labels] + 1.5 * rng.standard_normal((labels.size, dim))
    return query, target, labels


def file_arrays(seed, classes, items, dim):
    """audio (items, 10, dim), image list of (10, dim), filenames 'NNN.Class/img_i'."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(1, classes + 1, items)
    centre = rng.standard_normal((classes + 1, dim))
    audio = centre[labels][:, None, :] + 4.0 * rng.standard_normal((items, 10, dim))
    image = [centre[l][None, :] + 4.0 * rng.standard_normal((10, dim)) for l in labels]
    names = ["%03d.Class_%d/img_%d" % (l, l, i) for i, l in enumerate(labels)]
    return audio, image, names


def import_reference():
    for name in ("h5py", "librosa", "torchvision"):
        sys.modules.setdefault(name, types.ModuleType(name))
    tbx = types.ModuleType("tensorboardX")

    class SummaryWriter(object):
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, name):
            return lambda *a, **k: None
    tbx.SummaryWriter = SummaryWriter
    sys.modules.setdefault("tensorboardX", tbx)
    import scipy.signal
    import scipy.signal.windows as win
    for name in ("hamming", "hann", "blackman", "bartlett"):   # moved to scipy.signal.windows in newer scipy
        if not hasattr(scipy.signal, name):
            setattr(scipy.signal, name, getattr(win, name))
    sys.path.insert(0, REF)
    import train_audio_encoder as rt
    return rt


def main():
    rt = import_reference()
    out = {}
    for seed, classes, per, dim, topk in CLASS_CASES:
        q, t, lab = class_arrays(seed, classes, per, dim)
        accu, ap = rt.EvalClass().eval_class(q, t, list(lab), topk)
        out["class_%d" % seed] = np.array([accu, ap], dtype=np.float64)
    for seed, draw, classes, items, dim in FILE_CASES:
        audio, image, names = file_arrays(seed, classes, items, dim)
        with tempfile.TemporaryDirectory() as d:
            paths = []
            for k, obj in (("a", audio), ("i", image), ("f", names)):
                p = os.path.join(d, k + ".pickle")
                with open(p, "wb") as f:
                    pickle.dump(obj, f)
                paths.append(p)
            random.seed(draw)
            accu, ap = rt.eval_audio_feature(*paths)
        out["file_%d" % seed] = np.array([accu, ap], dtype=np.float64)
    np.savez(os.path.join(HERE, "retrieval.npz"), **out)
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    main()
