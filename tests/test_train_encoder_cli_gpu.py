"""train_encoder end to end on a synthetic <split>.json tree (the tree of tests/test_encoder_head_cli_gpu.py): one short
epoch from the seeded initialisation and one from a checkpoint; the checkpoints are accepted by
extract_audio_feature.load_encoder, carry the reference's key set and differ from the start in the conv stack."""
import os

import pytest
import torch

from encoder_ref import build_encoder
from test_encoder_head_cli_gpu import _make_split

pytestmark = pytest.mark.gpu


def _run(root, out_dir, extra):
    from speech_to_image_translation_without_text_amd import train_encoder
    best = train_encoder.main(["--dataset", "birds", "--data_dir", root, "--output_dir", out_dir, "--epoch", "1",
                               "--batch_size", "4", "--bidirectional", "--jel_flag", "--l1_flag"] + extra)
    assert 0.0 <= best <= 100.0
    for name in ("epoch_1.pth", "latest.pth", "best.pth"):
        assert os.path.exists(os.path.join(out_dir, name)), name
    return torch.load(os.path.join(out_dir, "latest.pth"), map_location="cpu", weights_only=True)


def _check(ckpt, start, gpu, path):
    from speech_to_image_translation_without_text_amd import extract_audio_feature
    assert ckpt["meta"] == {"epoch": 1}
    after = ckpt["state_dict"]
    assert list(after) == list(start)                       # the reference's key set, in its order
    changed = [k for k in start if not torch.equal(start[k], after[k])]
    assert any(k.startswith("Conv.") and k.endswith(".0.weight") for k in changed), changed
    assert any(k.startswith("RNN.") for k in changed) and any(k.endswith("running_var") for k in changed)
    assert all(bool(torch.isfinite(v.float()).all()) for v in after.values())
    model = extract_audio_feature.load_encoder(path, True, 1, gpu)
    loaded = model.state_dict()
    assert all(torch.equal(loaded[k].cpu(), after[k]) for k in after)


def test_cli_trains_from_the_seeded_initialisation(gpu, tmp_path):
    from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN
    root = str(tmp_path)
    _make_split(root, "train", 4, 1)
    _make_split(root, "test", 2, 2)
    out_dir = os.path.join(root, "out")
    ckpt = _run(root, out_dir, ["--seed", "3"])
    torch.manual_seed(3)
    start = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).state_dict()
    _check(ckpt, start, gpu, os.path.join(out_dir, "latest.pth"))


def test_cli_trains_from_a_checkpoint(gpu, tmp_path):
    root = str(tmp_path)
    _make_split(root, "train", 4, 1)
    _make_split(root, "test", 2, 2)
    start_path = os.path.join(root, "start.pt")
    start = build_encoder().state_dict()
    torch.save({"state_dict": start}, start_path)
    out_dir = os.path.join(root, "out")
    ckpt = _run(root, out_dir, ["--model", start_path])
    _check(ckpt, start, gpu, os.path.join(out_dir, "latest.pth"))
