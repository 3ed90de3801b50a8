"""CPU suite of the test-split scorer (gan_metrics.py): the Frechet distance from fitted Gaussians against the reference's
own FIDs (tests/golden/inception_metrics.npz), the moments .npz round trip and its refusals, the command line, and the
argument checks of s2i_moments_accumulate (host code, no GPU)."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import GOLDEN

_spec = importlib.util.spec_from_file_location("make_golden_inception_metrics",
                                               os.path.join(GOLDEN, "make_golden_inception_metrics.py"))
mgm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mgm)


def gaussian(rows):
    return rows.mean(0), np.cov(rows, rowvar=False), rows.shape[0]


def test_frechet_distance_reproduces_the_reference_fids():
    from speech_to_image_translation_without_text_amd import gan_metrics as GM, trainer as T
    gold = np.load(os.path.join(GOLDEN, "inception_metrics.npz"))
    for seed, rg, rr, dim in mgm.FID_CASES:
        g, r = mgm.features(seed, rg, rr, dim)
        (mu1, s1, _), (mu2, s2, _) = gaussian(g), gaussian(r)
        fid = GM.frechet_distance(mu1, s1, mu2, s2)
        np.testing.assert_allclose(fid, gold["fid_%d" % seed], rtol=1e-6)
        assert fid == float(T.compute_frethet_distance(g, r)[0])      # same rows: the same number


def test_frechet_distance_refuses_mismatched_dimensions():
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    with pytest.raises(ValueError):
        GM.frechet_distance(np.zeros(4), np.eye(4), np.zeros(5), np.eye(5))
    with pytest.raises(ValueError):
        GM.frechet_distance(np.zeros(4), np.eye(4), np.zeros(4), np.eye(3))


def test_stats_npz_round_trip_and_refusals(tmp_path):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    rng = np.random.default_rng(0)
    mu, sigma, n = gaussian(rng.standard_normal((50, 6)))
    p = str(tmp_path / "s.npz")
    GM.save_stats(p, mu, sigma, n)
    mu2, sigma2, n2 = GM.FeatureMoments.load(p, D=6)
    assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2) and n2 == n
    with pytest.raises(ValueError, match="expected 8"):
        GM.load_stats(p, D=8)
    GM.save_stats(p, mu, sigma, 1)
    with pytest.raises(ValueError, match="need >= 2"):
        GM.load_stats(p)
    np.savez(p, mu=mu, sigma=sigma[:5, :5], n=np.int64(n))
    with pytest.raises(ValueError):
        GM.load_stats(p)
    np.savez(p, mu=mu, sigma=sigma)
    with pytest.raises(ValueError, match="lacks"):
        GM.load_stats(p)
    np.savez(p, mu=np.array([{"a": 1}], dtype=object), sigma=sigma, n=np.int64(n))
    with pytest.raises(ValueError):                                  # pickled objects are never loaded
        GM.load_stats(p)


def test_feature_moments_refuse_fewer_than_two_rows():
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    m = GM.FeatureMoments(8, "cpu")
    with pytest.raises(ValueError, match="at least 2"):
        m.mean_cov()


def test_command_line_and_real_stats_read_versus_write(tmp_path):
    from speech_to_image_translation_without_text_amd import gan_metrics as GM
    base = ["--netG", "out/Model/netG_600.pth", "--inception", "i.pth", "--data_dir", "data/birds"]
    a = GM.parse_args(base)
    assert (a.seed, a.max_items, a.save_images, a.real_stats, a.real_stats_mode, a.out) == (0, None, False, None, None,
                                                                                             "metrics.json")
    stats = tmp_path / "real.npz"
    a = GM.parse_args(base + ["--real_stats", str(stats), "--seed", "3", "--max_items", "5", "--save_images",
                              "--out", str(tmp_path / "m.json"), "--cfg", "c.yml"])
    assert (a.seed, a.max_items, a.save_images, a.cfg, a.real_stats_mode) == (3, 5, True, "c.yml", "write")
    stats.write_bytes(b"")
    assert GM.parse_args(base + ["--real_stats", str(stats)]).real_stats_mode == "read"
    for bad in (["--max_items", "0"], ["--seed", "x"]):
        with pytest.raises(SystemExit):
            GM.parse_args(base + bad)
    with pytest.raises(SystemExit):
        GM.parse_args(base[2:])                                      # --netG is required
    assert GM._image_dir("out/Model/netG_600.pth") == os.path.abspath("out/Model") + "/iteration600"


def test_moments_argument_errors_without_a_gpu():
    from speech_to_image_translation_without_text_amd import _lib
    lib = _lib.load()
    assert "s2i_moments_accumulate" in _lib.EXPORTED_SYMBOLS
    for args, word in (((1, 1, 64, 64, 1, 1, None), b"null rows"), ((1, 1, 0, 64, 1, 1, None), b"D 0"),
                       ((1, 1, 65537, 65537, 1, 1, None), b"D 65537"), ((1, 1, 100, 64, 1, 1, None), b"row stride"),
                       ((1, -1, 64, 64, 1, 1, None), b"rows -1"), ((1, 1, 64, 64, None, 1, None), b"null pointer")):
        x, rows, D, ldx, cs, g, st = args
        assert lib.s2i_moments_accumulate(None if word == b"null rows" else x, rows, D, ldx, cs, g, st) != 0
        assert word in lib.s2i_last_error(), lib.s2i_last_error()
    assert lib.s2i_moments_accumulate(None, 0, 64, 64, 1, 1, None) == 0   # no rows: nothing to launch
