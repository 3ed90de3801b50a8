"""The encoder's training utterances resident in device memory as log-mel rows; a batch is one gather launch.

The host path (train_encoder_head.SplitData.batches) repeats for every batch and every epoch: open and parse B WAV files,
copy B ragged arrays to the device, run the three log-mel kernels.  An utterance's log-mel depends on that utterance alone
(its own mean, its own maximum), so `ResidentSpeechSet` computes it once per utterance with `audio.log_mel`, keeps the
first min(n_frames, T) rows of every utterance a draw can return -- those with at least 64 frames -- back to back in one
fp32 [rows, 40] pool on the device, and makes a batch with `ops.logmel_gather`: two small index uploads and one launch
that copies the rows and writes the 0 dB fill of Audio_to_Image/utils.py:329-340.  `plan_draw` makes the random draws of
`SplitData.draw` with its calls in its order, so under the same seed of Python's `random` both feeders choose the same
views and utterances and every tensor of a batch is bit-identical (tests/test_speech_loader_cpu.py,
tests/test_speech_loader_gpu.py).

The host path stays the default; nothing here changes it.  A frame costs 160 bytes and an utterance at most
T * 160 = 327 680 bytes at T = 2048.
"""
import os
import random
import wave
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import audio
from .extract_audio_feature import MIN_FRAMES
from .train_encoder_head import MAX_DRAWS

MAX_READ_THREADS = 16
ROW_BYTES = 4 * audio.N_MELS


def _threads(workers):
    return max(1, min(int(workers), MAX_READ_THREADS))


def _resolve(device):
    """`device` with "cuda" spelled out as the current device"""
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def plan_draw(frames_of_item, n_views, rng=random, item=0):
    """The random draws of `SplitData.draw(item)`, with its calls in its order: `randint` for the image view, then
    `randint` for the utterance, again while the drawn one has fewer than 64 frames, MAX_DRAWS times at the most.
    `frames_of_item` holds the frame count of each of the item's utterances.  Returns (view, utterance)."""
    view = rng.randint(0, n_views - 1)
    n = len(frames_of_item)
    for _ in range(MAX_DRAWS):
        u = rng.randint(0, n - 1)
        if frames_of_item[u] >= MIN_FRAMES:
            return view, u
    raise ValueError("item %d: no utterance with at least %d frames in %d draws" % (item, MIN_FRAMES, MAX_DRAWS))


def _samples(path):
    """Samples per channel of a WAV from its header; a file `wave` cannot open goes to `audio.read_wav` for its message."""
    try:
        with wave.open(str(path), "rb") as f:
            return f.getnframes()
    except (wave.Error, EOFError):
        return len(audio.read_wav(path))


def utterance_paths(split):
    """Per item the paths of its utterances, in the JSON's order."""
    return [[os.path.join(split.audio_base, n) for n in item[split.key]] for item in split.items]


def _samples_16k(path):
    """Samples the file has at 16 kHz, by the integer rule, from its header (any format `audio.probe_audio` accepts)"""
    info = audio.probe_audio(path)
    return audio.resampled_length(info.frames, info.rate)


def scan_frames(split, workers=MAX_READ_THREADS, target_length=audio.TARGET_LENGTH, resample=False):
    """Per item an int64 array of `audio.n_frames` of each utterance, capped at `target_length`, from the WAV headers;
    with `resample`, of each utterance's length at 16 kHz."""
    paths = utterance_paths(split)
    with ThreadPoolExecutor(max_workers=_threads(workers)) as ex:
        flat = list(ex.map(_samples_16k if resample else _samples, [p for item in paths for p in item]))
    out, k = [], 0
    for item in paths:
        out.append(np.array([audio.n_frames(n, target_length) for n in flat[k:k + len(item)]], dtype=np.int64))
        k += len(item)
    return out


def pool_layout(frames):
    """Where each utterance's rows start: (row_offsets, rows).  `row_offsets` is int64 over all utterances in the JSON's
    order, cumulative over the stored ones (at least 64 frames) and -1 for the others; `rows` is the pool's row count."""
    flat = np.concatenate(frames).astype(np.int64) if len(frames) else np.zeros(0, np.int64)
    kept = np.where(flat >= MIN_FRAMES, flat, 0)
    ends = np.cumsum(kept)
    return np.where(flat >= MIN_FRAMES, ends - kept, -1).astype(np.int64), int(ends[-1]) if len(ends) else 0


class ResidentSpeechSet:
    """Every utterance of `split` (a train_encoder_head.SplitData) with at least 64 frames as its first
    min(n_frames, target_length) log-mel rows, in one fp32 [rows, 40] tensor on `device`.

    frames        per item an int64 array: each utterance's frame count (kept for the short ones too: the draw needs it)
    row_offsets   int64 over all utterances in the JSON's order: first pool row, -1 where nothing is stored
    first         int64 per item: the number of its first utterance in that order
    pool, nbytes  the device tensor and its size in bytes

    The image features and labels stay on the host, as in SplitData.  `workers` (at most 16) threads read the files,
    `chunk` utterances at a time go through `audio.log_mel`, and only one chunk of waveforms is held on the host."""

    def __init__(self, split, device, workers=16, chunk=256, target_length=audio.TARGET_LENGTH, resample=False):
        from . import _lib
        self.split = split
        self.resample = bool(resample)     # files of any accepted rate and format, through audio.to_16k
        self.device = torch.device(device)
        self.T = int(target_length)
        if self.T < MIN_FRAMES:
            raise ValueError("ResidentSpeechSet: target_length %d is under the %d frames a draw asks for" % (self.T, MIN_FRAMES))
        if int(chunk) < 1:
            raise ValueError("ResidentSpeechSet: chunk must be >= 1")
        if self.device.type != "cuda":
            raise _lib.S2IError("the log-mel pool is made and read by the MI355X kernels: there is no CPU fallback (device %s)"
                                % self.device)
        self.frames = scan_frames(split, workers, self.T, self.resample)
        self.row_offsets, rows = pool_layout(self.frames)
        counts = np.array([len(f) for f in self.frames], dtype=np.int64)
        self.first = np.cumsum(counts) - counts
        self.pool = torch.empty((rows, audio.N_MELS), dtype=torch.float32, device=self.device)
        self.nbytes = rows * ROW_BYTES
        self._fill(int(chunk), _threads(workers))

    def _fill(self, chunk, threads):
        """Read every utterance once, `chunk` at a time; the stored ones of a chunk go through log_mel together and
        their kept rows, which are consecutive in the pool, land there as one masked copy."""
        paths = [p for item in utterance_paths(self.split) for p in item]
        flat = np.concatenate(self.frames) if self.frames else np.zeros(0, np.int64)
        steps = torch.arange(self.T, device=self.device)
        with ThreadPoolExecutor(max_workers=threads) as ex:
            for s in range(0, len(paths), chunk):
                if self.resample:
                    waves = audio.to_16k(list(ex.map(audio.read_audio, paths[s:s + chunk])), self.device)
                else:
                    waves = list(ex.map(audio.read_wav, paths[s:s + chunk]))
                for k, w in enumerate(waves, s):
                    if audio.n_frames(len(w), self.T) != flat[k]:
                        raise ValueError("%s holds %d samples, its header promised %d frames" % (paths[k], len(w), flat[k]))
                ids = [k for k in range(s, s + len(waves)) if self.row_offsets[k] >= 0]
                if not ids:
                    continue
                mel, nf = audio.log_mel([waves[k - s] for k in ids], target_length=self.T, layout="nhwc",
                                        device=self.device)
                del waves
                keep = steps[None, :] < torch.from_numpy(nf).to(self.device)[:, None]
                lo = int(self.row_offsets[ids[0]])
                hi = int(self.row_offsets[ids[-1]] + flat[ids[-1]])
                self.pool[lo:hi] = mel.view(len(ids), self.T, audio.N_MELS)[keep]

    def __len__(self):
        return len(self.split)

    def draw(self, index):
        """(image view (1024,), utterance number, label) of `SplitData.draw(index)` under the same `random` state; no
        file is opened."""
        views = self.split.image[index]
        view, u = plan_draw(self.frames[index], len(views), random, index)
        return views[view], u, self.split.labels[index]

    def mel(self, utterances):
        """[B, 1, T, 40] log-mel of a list of (item, utterance number) pairs, and their frame counts (int64 ndarray)."""
        from . import _lib, ops
        flat = np.array([self.first[i] + u for i, u in utterances], dtype=np.int64)
        frames = np.array([self.frames[i][u] for i, u in utterances], dtype=np.int64)
        offsets = self.row_offsets[flat]
        if len(flat) == 0 or int(offsets.min()) < 0:
            raise _lib.S2IError("ResidentSpeechSet.mel: %s" % ("no utterances" if len(flat) == 0 else
                                "utterance %r has under %d frames and is not stored"
                                % (utterances[int(np.argmin(offsets))], MIN_FRAMES)))
        # two small pinned copies; the caching host allocator keeps the blocks until the copies have run
        off_d = torch.from_numpy(offsets).pin_memory().to(self.device, non_blocking=True)
        frm_d = torch.from_numpy(frames.astype(np.int32)).pin_memory().to(self.device, non_blocking=True)
        return ops.logmel_gather(self.pool, off_d, frm_d, self.T), frames

    def batches(self, batch_size, device, shuffle, order=None):
        """The batches of `SplitData.batches`: (mel_nhwc [B, 1, T, 40], cap_lens, image_feature [B, 1024], label [B]),
        with its `random` calls in its order.  `order`, where given, is the list of items to go through (a rank's share of
        an epoch, train_encoder_head.shard_order; the pool itself is whole on every rank) and `shuffle` is not looked at."""
        from . import _lib
        if _resolve(device) != _resolve(self.device):
            raise _lib.S2IError("the log-mel pool is on %s, batches were asked for on %s: there is no CPU fallback and no "
                                "copy between devices" % (self.device, device))
        if order is None:
            order = list(range(len(self)))
            if shuffle:
                random.shuffle(order)
        for s in range(0, len(order), batch_size):
            items = order[s:s + batch_size]
            drawn = [self.draw(i) for i in items]
            mel, frames = self.mel([(i, u) for i, (_, u, _) in zip(items, drawn)])
            image = torch.from_numpy(np.stack([v for v, _, _ in drawn])).float()
            yield mel, (frames // MIN_FRAMES).tolist(), image, torch.tensor([c for _, _, c in drawn], dtype=torch.int64)
