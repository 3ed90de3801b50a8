"""References for the resident speech feeder (speech_loader.py, s2i_logmel_gather): the gather in numpy, three wrong
versions of it that a test must be able to tell from it, the kernel's test inputs, and a writer of synthetic
<split>.json trees with WAVs of chosen lengths."""
import json
import os
import wave

import numpy as np

N_MELS = 40


def gather_ref(pool, row_offsets, frames, T):
    """out [B, 1, T, 40]: out[b, 0, t] = pool[row_offsets[b] + t] for t < frames[b], 0.0 for frames[b] <= t < T."""
    pool = np.asarray(pool, dtype=np.float32)
    out = np.zeros((len(row_offsets), 1, int(T), pool.shape[1]), dtype=np.float32)
    for b, (o, f) in enumerate(zip(row_offsets, frames)):
        o, f = int(o), int(f)
        assert 0 <= f <= T and 0 <= o and o + f <= len(pool), (b, o, f)
        out[b, 0, :f] = pool[o:o + f]
    return out


def mutant_pads_with_next_rows(pool, row_offsets, frames, T):
    """wrong: the rows past frames[b] come from the pool (the following utterance's) instead of being 0"""
    pool = np.asarray(pool, dtype=np.float32)
    rows = np.minimum(np.asarray(row_offsets, dtype=np.int64)[:, None] + np.arange(T)[None, :], len(pool) - 1)
    return pool[rows][:, None]


def mutant_drops_last_row(pool, row_offsets, frames, T):
    """wrong: frames[b] - 1 rows are copied"""
    return gather_ref(pool, row_offsets, [max(int(f) - 1, 0) for f in frames], T)


def mutant_offsets_in_floats(pool, row_offsets, frames, T):
    """wrong: row_offsets[b] is taken as an index of floats, not of rows"""
    flat = np.asarray(pool, dtype=np.float32).reshape(-1)
    out = np.zeros((len(row_offsets), 1, int(T), N_MELS), dtype=np.float32)
    for b, (o, f) in enumerate(zip(row_offsets, frames)):
        o, f = int(o), int(f)
        out[b, 0, :f] = flat[o:o + f * N_MELS].reshape(f, N_MELS)
    return out


MUTANTS = (mutant_pads_with_next_rows, mutant_drops_last_row, mutant_offsets_in_floats)


def coded_pool(rows, first=0):
    """[rows, 40] with value (first + row) * 64 + m at (row, m): exact in fp32 below 2^18 rows, and a wrong row or a wrong
    column shows"""
    return ((first + np.arange(rows, dtype=np.int64))[:, None] * 64 + np.arange(N_MELS)[None, :]).astype(np.float32)


def kernel_cases():
    """(name, pool, row_offsets int64, frames int32, T) of every small launch the kernel is tested at."""
    def case(name, rows, offsets, frames, T):
        return name, coded_pool(rows), np.array(offsets, dtype=np.int64), np.array(frames, dtype=np.int32), T
    return [
        case("one_row", 4, [2], [1], 1),
        # empty, one row, one short of full, full
        case("edges_of_T70", 140, [0, 0, 1, 70], [0, 1, 69, 70], 70),
        # stored: 2048 rows at 0, 2047 at 2048, 1000 at 4095, 65 at 5095; the batch takes them out of order, and the last
        # utterance twice (once cut to 64 rows)
        case("production_T", 5160, [5095, 2048, 0, 4095, 5095], [64, 2047, 2048, 1000, 65], 2048),
        # every padded region lies over the following utterance's rows
        case("padding_over_neighbours", 170, [0, 10, 43], [10, 33, 63], 64),
    ]


def write_wav(path, seconds, seed, channels=1):
    """A seeded tone in noise as 16 kHz PCM16; every (seed, channels) gives other samples."""
    rng = np.random.RandomState(seed)
    n = int(round(16000 * seconds))
    t = np.arange(n) / 16000.0
    sig = 0.3 * np.sin(2 * np.pi * (200 + 7 * (seed % 97)) * t)[:, None] + 0.05 * rng.randn(n, channels)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def make_tree(root, split, spec, seed=0, views=10):
    """Write `<root>/<split>.json`, its image-feature pickle and its WAVs.  `spec` has one list per item; an entry is the
    clip's length in seconds, or (seconds, channels).  Item i is of class 1 + i % 2.  Returns the utterances' paths, per
    item."""
    from speech_to_image_translation_without_text_amd import datasets
    rng = np.random.RandomState(seed)
    data, paths = [], []
    for i, clips in enumerate(spec):
        names = []
        for u, clip in enumerate(clips):
            seconds, channels = clip if isinstance(clip, tuple) else (clip, 1)
            name = "%s/item%d/utt%d.wav" % (split, i, u)
            write_wav(os.path.join(root, "audio", name), seconds, seed * 100003 + i * 101 + u, channels)
            names.append(name)
        data.append({"audio": names, "class": "%03d.Some_bird" % (1 + i % 2)})
        paths.append([os.path.join(root, "audio", n) for n in names])
    feat = os.path.join(root, split, "image_features.pickle")
    os.makedirs(os.path.dirname(feat), exist_ok=True)
    datasets.save_embedding_pickle(rng.randn(len(spec), views, 1024).astype(np.float32), feat)
    with open(os.path.join(root, "%s.json" % split), "w") as f:
        json.dump({"audio_base_path": os.path.join(root, "audio"), "image_feature_path": feat, "data": data}, f)
    return paths
