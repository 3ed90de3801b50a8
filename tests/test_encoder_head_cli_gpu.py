"""train_encoder_head end to end on a synthetic <split>.json tree: a few generated WAVs and a random image-feature pickle
in a temp directory; one short epoch; the checkpoints it writes are accepted by extract_audio_feature and retrieval."""
import json
import os
import wave

import numpy as np
import pytest
import torch

from encoder_ref import build_encoder

pytestmark = pytest.mark.gpu


def _write_wav(path, seconds, seed):
    rng = np.random.RandomState(seed)
    n = int(16000 * seconds)
    t = np.arange(n) / 16000.0
    sig = 0.3 * np.sin(2 * np.pi * (200 + 40 * seed) * t) + 0.05 * rng.randn(n)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def _make_split(root, split, items, seed):
    from speech_to_image_translation_without_text_amd import datasets
    rng = np.random.RandomState(seed)
    data = []
    for i in range(items):
        names = []
        for u in range(10):
            name = "%s/item%d/utt%d.wav" % (split, i, u)
            _write_wav(os.path.join(root, "audio", name), 1.0 + 0.25 * ((i + u) % 4), seed * 1000 + i * 10 + u)
            names.append(name)
        data.append({"audio": names, "class": "%03d.Some_bird" % (1 + i % 2)})
    feat = os.path.join(root, split, "image_features.pickle")
    datasets.save_embedding_pickle(rng.randn(items, 10, 1024).astype(np.float32), feat)
    with open(os.path.join(root, "%s.json" % split), "w") as f:
        json.dump({"audio_base_path": os.path.join(root, "audio"), "image_feature_path": feat, "data": data}, f)


def test_cli_runs_an_epoch_and_writes_usable_checkpoints(gpu, tmp_path):
    from speech_to_image_translation_without_text_amd import extract_audio_feature, retrieval, train_encoder_head
    root = str(tmp_path)
    _make_split(root, "train", 4, 1)
    _make_split(root, "test", 2, 2)
    start = os.path.join(root, "start.pt")
    torch.save({"state_dict": build_encoder().state_dict()}, start)
    out_dir = os.path.join(root, "out")
    best = train_encoder_head.main(["--model", start, "--dataset", "birds", "--data_dir", root, "--output_dir", out_dir,
                                    "--epoch", "1", "--batch_size", "3", "--bidirectional", "--jel_flag", "--l1_flag",
                                    "--distill_flag", "--seed", "0"])
    assert 0.0 <= best <= 100.0
    for name in ("epoch_1.pth", "latest.pth", "best.pth"):
        assert os.path.exists(os.path.join(out_dir, name)), name
    before = build_encoder().state_dict()
    after = torch.load(os.path.join(out_dir, "best.pth"), map_location="cpu", weights_only=True)
    assert after["meta"] == {"epoch": 1}
    changed = [k for k in before if not torch.equal(before[k], after["state_dict"][k])]
    assert changed and all(k.startswith("RNN.") for k in changed), changed
    # the checkpoint feeds the feature extraction and the retrieval score
    extract_audio_feature.main(["--model", os.path.join(out_dir, "best.pth"), "--dataset", "birds", "--bidirectional",
                                "--data_dir", root, "--splits", "test"])
    accu, ap = retrieval.main(["--audio", os.path.join(root, "test", "audio_features_0.pickle"),
                               "--image", os.path.join(root, "test", "image_features.pickle"), "--data_dir", root])
    assert 0.0 <= accu <= 100.0 and 0.0 <= ap <= 100.0
