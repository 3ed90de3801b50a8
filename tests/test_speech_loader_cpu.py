"""Host side of the resident speech feeder: `speech_loader.plan_draw` makes the random draws of `SplitData.draw`, the pool
layout, the numpy reference's power to tell itself from wrong gathers, and the new symbol's declaration and binding.
No GPU."""
import os
import random
import re

import numpy as np
import pytest

from speech_loader_ref import MUTANTS, gather_ref, kernel_cases, make_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ten utterances per item, three of them 0.3 s long: 1 + 4800 // 160 = 31 frames, under the 64 a draw asks for
ITEM = [1.0, 0.3, 1.2, 0.7, 0.3, 1.5, 0.9, 0.3, 1.1, 0.8]
SPEC = [ITEM[k:] + ITEM[:k] for k in range(6)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from speech_to_image_translation_without_text_amd import audio, speech_loader, train_encoder_head
    root = str(tmp_path_factory.mktemp("speech_tree"))
    paths = make_tree(root, "train", SPEC, seed=3)
    split = train_encoder_head.SplitData(root, "train", "birds")
    frames = speech_loader.scan_frames(split, workers=4)
    waves = [[audio.read_wav(p) for p in item] for item in paths]
    return split, frames, waves


def _utterance_of(wave, waves_of_item):
    """the number of the utterance `SplitData.draw` returned, by the waveform's length and first samples"""
    hits = [u for u, w in enumerate(waves_of_item) if len(w) == len(wave) and np.array_equal(w[:64], wave[:64])]
    assert len(hits) == 1, hits
    return hits[0]


class _CountingRandom:
    """the `random` module's randint, counted"""
    calls = 0

    def randint(self, a, b):
        self.calls += 1
        return random.randint(a, b)


def _view_of(image, views):
    hits = [v for v in range(len(views)) if np.array_equal(views[v], image)]
    assert len(hits) == 1, hits
    return hits[0]


def test_scan_frames_counts_what_n_frames_counts(tree):
    from speech_to_image_translation_without_text_amd import audio
    split, frames, waves = tree
    assert len(frames) == len(split)
    for f, item in zip(frames, waves):
        assert f.dtype == np.int64 and f.tolist() == [audio.n_frames(len(w)) for w in item]
    assert sorted(frames[0].tolist())[:3] == [31, 31, 31] and sorted(frames[0].tolist())[3] >= 64


@pytest.mark.parametrize("shuffle", [False, True])
def test_plan_draw_makes_the_draws_of_split_data(tree, shuffle):
    from speech_to_image_translation_without_text_amd import speech_loader
    split, frames, waves = tree
    rng = _CountingRandom()
    for seed in range(8):
        random.seed(seed)
        order = list(range(len(split)))
        if shuffle:
            random.shuffle(order)
        host = []
        for i in order:
            image, wave, label = split.draw(i)
            host.append((i, _view_of(image, split.image[i]), _utterance_of(wave, waves[i]), label))
        host_state = random.getstate()

        random.seed(seed)
        order2 = list(range(len(split)))
        if shuffle:
            random.shuffle(order2)
        assert order2 == order
        planned = []
        for i in order2:
            view, u = speech_loader.plan_draw(frames[i], len(split.image[i]), rng, i)
            planned.append((i, view, u, split.labels[i]))
        assert planned == host
        assert random.getstate() == host_state
        assert all(frames[i][u] >= 64 for i, _, u, _ in planned)
    assert rng.calls > 8 * 2 * len(split)          # some draws met a short utterance and drew again


def test_an_item_of_short_utterances_is_refused_with_split_datas_message(tmp_path):
    from speech_to_image_translation_without_text_amd import speech_loader, train_encoder_head
    root = str(tmp_path)
    make_tree(root, "train", [[1.0, 0.3], [0.3, 0.2, 0.39]], seed=5)
    split = train_encoder_head.SplitData(root, "train", "birds")
    frames = speech_loader.scan_frames(split, workers=2)
    random.seed(0)
    with pytest.raises(ValueError) as host:
        split.draw(1)
    host_state = random.getstate()
    random.seed(0)
    with pytest.raises(ValueError) as planned:
        speech_loader.plan_draw(frames[1], len(split.image[1]), random, 1)
    assert str(planned.value) == str(host.value) and "item 1" in str(host.value)
    assert random.getstate() == host_state


def test_pool_layout_is_cumulative_over_the_stored_utterances(tree):
    from speech_to_image_translation_without_text_amd import speech_loader
    _, frames, _ = tree
    offsets, rows = speech_loader.pool_layout(frames)
    flat = np.concatenate(frames)
    assert offsets.dtype == np.int64 and offsets.shape == flat.shape
    expect, at = [], 0
    for f in flat:
        expect.append(at if f >= 64 else -1)
        at += f if f >= 64 else 0
    assert offsets.tolist() == expect
    assert (offsets[flat < 64] == -1).all() and (flat < 64).sum() == 3 * len(frames)
    last = np.nonzero(offsets >= 0)[0][-1]
    assert offsets[last] + flat[last] == rows == at
    # frames are capped at the target length before they are laid out
    capped, rows2 = speech_loader.pool_layout([np.minimum(f, 80) for f in frames])
    assert rows2 == int(np.minimum(flat, 80)[flat >= 64].sum()) and capped.dtype == np.int64


def test_gather_ref_rejects_its_mutants():
    differs = {m.__name__: [] for m in MUTANTS}
    for name, pool, offsets, frames, T in kernel_cases():
        ref = gather_ref(pool, offsets, frames, T)
        assert ref.shape == (len(offsets), 1, T, 40) and ref.dtype == np.float32
        for m in MUTANTS:
            out = m(pool, offsets, frames, T)
            assert out.shape == ref.shape
            if not np.array_equal(out, ref):
                differs[m.__name__].append(name)
    every = [c[0] for c in kernel_cases()]
    assert differs["mutant_pads_with_next_rows"] == every[1:]        # T = 1, one row: nothing is padded
    assert differs["mutant_drops_last_row"] == every
    assert differs["mutant_offsets_in_floats"] == every


def test_symbol_is_declared_and_bound():
    from speech_to_image_translation_without_text_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    decl = re.search(r"int s2i_logmel_gather\(([^)]*)\)", header)
    assert decl and [a.strip() for a in decl.group(1).replace("\n", " ").split(",")] == [
        "const float* pool", "const long long* row_offsets", "const int* frames", "int B", "int T", "float* out",
        "void* stream"]
    assert "s2i_logmel_gather" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.s2i_version() == 7
    # refused before anything touches a device
    assert lib.s2i_logmel_gather(None, None, None, 1, 1, None, None) != 0 and b"null" in lib.s2i_last_error()
