"""Generate tests/golden/inception_metrics.npz from the REFERENCE's metric functions (runs only in the build container).

The reference's StackGAN_v2/trainer.py is imported with the stand-ins of make_golden.py (torchvision, tensorboardX,
easydict) and its compute_inception_score, negative_log_posterior_probability (trainer.py:88-100, 147-159) and
compute_frethet_distance (:103-144, scipy's sqrtm) run on seeded float64 arrays.  Only the seeds, shapes and results are
stored: the tests regenerate the arrays with `arrays()` below.

Usage:  python tests/golden/make_golden_inception_metrics.py            (writes next to this file)
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# softmax-like rows: (seed, rows, classes, splits)
SOFTMAX_CASES = [(11, 600, 1000, 10), (12, 257, 200, 10), (13, 40, 1000, 1)]
# pool3-like features: (seed, rows_g, rows_r, dim) -- fewer and more rows than the 2048 feature dimensions
FID_CASES = [(21, 1000, 1200, 2048), (22, 3000, 2500, 2048), (23, 300, 400, 64)]


def softmax_rows(seed, rows, classes):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((rows, classes)) * 3.0
    e = np.exp(logits - logits.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def features(seed, rows_g, rows_r, dim):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    g = np.maximum(rng.standard_normal((rows_g, dim)) @ mix + 0.3, 0.0)
    r = np.maximum(rng.standard_normal((rows_r, dim)) @ mix * 1.2 + 0.2, 0.0)
    return g, r


def main():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    _, _, rt = mg.import_reference()
    out = {}
    for seed, rows, classes, splits in SOFTMAX_CASES:
        p = softmax_rows(seed, rows, classes)
        out["is_%d" % seed] = np.array(rt.compute_inception_score(p, splits), dtype=np.float64)
        out["nlpp_%d" % seed] = np.array(rt.negative_log_posterior_probability(p, splits), dtype=np.float64)
    for seed, rg, rr, dim in FID_CASES:
        g, r = features(seed, rg, rr, dim)
        fid, _ = rt.compute_frethet_distance(g, r)
        out["fid_%d" % seed] = np.array(float(np.real(fid)), dtype=np.float64)
    np.savez(os.path.join(HERE, "inception_metrics.npz"), **out)
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    main()
