"""The encoder's training utterances resident in device memory as 16 kHz waveforms, so that waveform-domain augmentation
can run on them: tempo and pitch through the phase vocoder s2i_time_stretch, speed (and the pitch's rate) through the
resampler, room reverberation through s2i_reverb and additive noise / babble through s2i_wave_mix, in that order.

`ResidentSpeechSet` (speech_loader.py) keeps finished log-mel rows, to which no waveform operation can be applied.
`ResidentWaveSet` keeps the fp32 samples of every utterance a draw can return -- those with at least 64 frames -- back to
back in one flat device buffer, each clip on a 16-byte boundary, so that `s2i_pcm_resample` reads a clip in place
(raw = the pool, format S2I_PCM_F32, byte offset = the clip's start).  A batch is: one resample launch per distinct speed
(speed 1.0 is the kernel's bypass L = M = 1, which then is the gather; where a clip drew a tempo or a pitch, the five
stretch launches come first and the resampler reads their buffer instead of the pool), the two reverberation launches where a clip drew
a room, the mix launches where a noise term is on, and the three log-mel launches.  fp32 is the stored type because it reproduces the host path bit for bit, stereo mixdown and the
resampled files of `resample=True` included: with augmentation off a batch equals `SplitData.batches` and
`ResidentSpeechSet.batches` under the same `random` seed (tests/test_waveaug_gpu.py).

The draws of `SplitData.draw` are repeated with its `random` calls in its order (speech_loader.plan_draw); the
augmentation's own draws come from a counter-based generator keyed by (seed, step, batch position) and touch neither
`random` nor torch's generators (ops.waveaug_plan).
"""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import audio
from .extract_audio_feature import MIN_FRAMES
from .speech_loader import _resolve, _samples, _samples_16k, _threads, plan_draw, utterance_paths

PAD_FLOATS = 4      # every stored clip and every clip of a batch starts on a 16-byte boundary


def _pad(n):
    return (np.asarray(n, dtype=np.int64) + PAD_FLOATS - 1) // PAD_FLOATS * PAD_FLOATS


class WaveAug:
    """What `ResidentWaveSet.batches(aug=...)` takes: a policy (ops.waveaug_policy's dict, or its spec string) and the
    seed of its draws."""

    def __init__(self, policy, seed):
        from . import ops
        self.policy = ops.waveaug_policy(policy) if isinstance(policy, str) else policy
        if self.policy is None:
            raise ValueError("WaveAug: an empty policy; pass aug=None instead")
        self.seed = int(seed)


def pool_layout(samples, target_length=audio.TARGET_LENGTH):
    """(offsets, floats): where each utterance's samples start, in floats, int64 over all utterances in the JSON's order,
    -1 for those under 64 frames (not stored); every start is a multiple of 4 floats.  `floats` is the pool's size."""
    samples = np.asarray(samples, dtype=np.int64)
    stored = np.array([audio.n_frames(n, target_length) >= MIN_FRAMES for n in samples], dtype=bool)
    kept = np.where(stored, _pad(samples), 0)
    ends = np.cumsum(kept)
    return np.where(stored, ends - kept, -1).astype(np.int64), int(ends[-1]) if len(ends) else 0


def render(pool, in_offsets, in_lens, rate, out_lens):
    """The clips pool[in_offsets[b] : + in_lens[b]] (starts in floats, multiples of 4), each read as if recorded at rate[b]
    Hz and converted to 16 kHz, into a new flat fp32 buffer on the pool's device: (flat, out_offsets), every clip on a
    16-byte boundary.  One s2i_pcm_resample launch per distinct rate, the pool read in place as S2I_PCM_F32; 16000 is the
    kernel's bypass, a copy.  One upload carries every launch's byte offsets | out offsets | frames | out lens | tiles."""
    from . import _lib
    lib = _lib.load()
    dev = pool.device
    in_offsets, in_lens = np.asarray(in_offsets, dtype=np.int64), np.asarray(in_lens, dtype=np.int64)
    rate, out_lens = np.asarray(rate, dtype=np.int64), np.asarray(out_lens, dtype=np.int64)
    padded = _pad(out_lens)
    out_offsets = np.cumsum(padded) - padded
    flat = torch.empty(max(int(padded.sum()), PAD_FLOATS), dtype=torch.float32, device=dev)
    parts, where, at = [], [], 0
    for r in sorted(set(rate[out_lens > 0].tolist())):
        ids = np.flatnonzero((rate == r) & (out_lens > 0))
        tiles = audio.resample_tiles(out_lens[ids])
        group = [(in_offsets[ids] * 4).astype(np.int64), out_offsets[ids].astype(np.int64), in_lens[ids].astype(np.int32),
                 out_lens[ids].astype(np.int32), tiles.reshape(-1)]
        pos = []
        for a in group:
            pos.append(at)
            at += audio._pad16(a.nbytes)
        parts += group
        where.append((r, len(ids), len(tiles), pos))
    image = np.zeros(max(at, 16), dtype=np.uint8)
    for a, p in zip(parts, [p for _, _, _, pos in where for p in pos]):
        image[p:p + a.nbytes] = np.ascontiguousarray(a).view(np.uint8)
    image_d = torch.from_numpy(image).to(dev)
    base = image_d.data_ptr()
    for r, n, ntiles, (boff, ooff, frm, olen, til) in where:
        L, M, W, _ = audio.resample_plan(r)
        _lib.check(lib.s2i_pcm_resample(_lib.ptr(pool), base + boff, base + frm, n, _lib.PCM_F32, 1, L, M, W,
                                        _lib.ptr(audio.device_resample_table(dev, r)), base + til, ntiles, _lib.ptr(flat),
                                        base + ooff, base + olen, _lib.stream()), "s2i_pcm_resample")
    return flat, out_offsets


def _stretch(pool, offsets, lens, plan):
    """(buffer, offsets, lens) the resampler reads: the pool's clips themselves, or -- where a clip of the batch drew a
    tempo or a pitch that needs the phase vocoder -- the whole batch written by s2i_time_stretch into a new flat buffer,
    the clips with rate 1 copied bit for bit"""
    from . import ops
    if plan is None or "stretch_rate" not in plan or not np.any(plan["stretch_rate"] != 1.0):
        return pool, offsets, lens
    return ops.time_stretch(pool, offsets, lens, ops.stretch_table(plan))


def _reverberate(flat, offsets, plan, aug, step):
    """`flat` under the plan's room impulse responses (a new buffer), or `flat` itself where no clip drew one"""
    from . import ops
    if plan is None or "taps" not in plan or not np.any(plan["taps"] > 0):
        return flat
    return ops.reverb(flat, offsets, plan["out_len"], ops.reverb_table(plan), aug.seed, step)


def perturb(waves, aug, device, step=0, uids=None):
    """The waveforms (16 kHz mono: numpy arrays or device tensors) under `aug`, without a pool of other utterances: tempo,
    pitch, speed, reverberation and white noise; babble= is refused.  Clip k draws with uid uids[k] (default: k).  Returns fp32 device tensors, views of
    one flat buffer, which `audio.log_mel` takes unchanged."""
    from . import _lib, ops
    if aug.policy["babble"] is not None:
        raise ValueError("babble= draws its interferers from a pool of training utterances (wave_loader.ResidentWaveSet), "
                         "which an extraction does not have: use tempo=, pitch=, speed=, reverb= and white= here")
    _lib.load()
    _lib.require_device()
    dev = torch.device(device)
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    padded = _pad(lens)
    offsets = np.cumsum(padded) - padded
    with torch.cuda.device(dev):
        if all(isinstance(w, np.ndarray) for w in waves):
            host = np.zeros(max(int(padded.sum()), PAD_FLOATS), dtype=np.float32)
            for o, w in zip(offsets, waves):
                host[o:o + len(w)] = w
            pool = torch.from_numpy(host).to(dev)
        else:
            pool = torch.zeros(max(int(padded.sum()), PAD_FLOATS), dtype=torch.float32, device=dev)
            for o, w in zip(offsets, waves):
                pool[o:o + len(w)] = torch.as_tensor(w).to(device=dev, dtype=torch.float32)
        plan = ops.waveaug_plan(aug.policy, aug.seed, step, np.arange(len(waves)) if uids is None else uids, lens)
        flat, out_offsets = render(*_stretch(pool, offsets, lens, plan), plan["rate"], plan["out_len"])
        flat = _reverberate(flat, out_offsets, plan, aug, step)
        if np.any(plan["g_white"] != 0):
            ops.wave_mix(flat, out_offsets, plan["out_len"], ops.wave_mix_table(plan), aug.seed, step)
    return [flat[int(o):int(o + n)] for o, n in zip(out_offsets, plan["out_len"])]


class ResidentWaveSet:
    """Every utterance of `split` (a train_encoder_head.SplitData) with at least 64 frames as its 16 kHz mono fp32
    samples in one flat tensor on `device`.

    samples       int64 over all utterances in the JSON's order: 16 kHz samples (kept for the short ones too)
    frames        per item an int64 array of frame counts, capped at target_length (the draw needs them)
    offsets       int64 over all utterances: first float in the pool, -1 where nothing is stored
    first         int64 per item: the number of its first utterance in that order
    stored        the numbers of the stored utterances; stored_offsets / stored_lens / stored_q: their starts, lengths
                  and mean squares Q (float64, accumulated on the host), what a babble draw indexes
    pool, nbytes  the device tensor and its size in bytes
    message       utterances, samples, bytes and seconds of the pool, for the caller to print

    `max_bytes` (None: no limit) refuses a pool above it before anything is allocated."""

    def __init__(self, split, device, workers=16, chunk=256, target_length=audio.TARGET_LENGTH, resample=False,
                 max_bytes=None):
        from . import _lib
        self.split = split
        self.resample = bool(resample)
        self.device = torch.device(device)
        self.T = int(target_length)
        if self.T < MIN_FRAMES:
            raise ValueError("ResidentWaveSet: target_length %d is under the %d frames a draw asks for" % (self.T, MIN_FRAMES))
        if int(chunk) < 1:
            raise ValueError("ResidentWaveSet: chunk must be >= 1")
        if self.device.type != "cuda":
            raise _lib.S2IError("the waveform pool is made and read by the MI355X kernels: there is no CPU fallback "
                                "(device %s)" % self.device)
        paths = utterance_paths(split)
        self.paths = [p for item in paths for p in item]
        with ThreadPoolExecutor(max_workers=_threads(workers)) as ex:
            self.samples = np.array(list(ex.map(_samples_16k if self.resample else _samples, self.paths)), dtype=np.int64)
        counts = np.array([len(item) for item in paths], dtype=np.int64)
        self.first = np.cumsum(counts) - counts
        flat_frames = np.array([audio.n_frames(n, self.T) for n in self.samples], dtype=np.int64)
        self.frames = [flat_frames[f:f + c] for f, c in zip(self.first, counts)]
        self.offsets, floats = pool_layout(self.samples, self.T)
        self.stored = np.flatnonzero(self.offsets >= 0)
        self.stored_offsets = self.offsets[self.stored]
        self.stored_lens = self.samples[self.stored]
        self.stored_q = np.zeros(len(self.stored), dtype=np.float64)
        self.nbytes = 4 * floats
        total = int(self.stored_lens.sum())
        self.message = ("%d utterances, %d samples, %d bytes, %.1f seconds of 16 kHz fp32 audio"
                        % (len(self.stored), total, self.nbytes, total / float(audio.SAMPLE_RATE)))
        if max_bytes is not None and self.nbytes > int(max_bytes):
            raise ValueError("ResidentWaveSet: the waveform pool needs %s, over max_bytes = %d: raise the limit or train "
                             "without waveform augmentation" % (self.message, int(max_bytes)))
        self.pool = torch.zeros(max(floats, PAD_FLOATS), dtype=torch.float32, device=self.device)
        self._fill(int(chunk), _threads(workers))

    def _fill(self, chunk, threads):
        """Read every utterance once, `chunk` at a time; the stored ones of a chunk are consecutive in the pool and go
        up as one copy, after their mean squares were taken in float64."""
        rank = np.full(len(self.paths), -1, dtype=np.int64)
        rank[self.stored] = np.arange(len(self.stored))
        with ThreadPoolExecutor(max_workers=threads) as ex:
            for s in range(0, len(self.paths), chunk):
                names = self.paths[s:s + chunk]
                if self.resample:
                    waves = [w.cpu().numpy() for w in audio.to_16k(list(ex.map(audio.read_audio, names)), self.device)]
                else:
                    waves = list(ex.map(audio.read_wav, names))
                for k, w in enumerate(waves, s):
                    if len(w) != self.samples[k]:
                        raise ValueError("%s holds %d samples, its header promised %d" % (self.paths[k], len(w), self.samples[k]))
                ids = [k for k in range(s, s + len(waves)) if self.offsets[k] >= 0]
                if not ids:
                    continue
                lo = int(self.offsets[ids[0]])
                hi = int(self.offsets[ids[-1]] + _pad(self.samples[ids[-1]]))
                host = np.zeros(hi - lo, dtype=np.float32)
                for k in ids:
                    w = np.asarray(waves[k - s], dtype=np.float32)
                    host[self.offsets[k] - lo:self.offsets[k] - lo + len(w)] = w
                    self.stored_q[rank[k]] = np.mean(w.astype(np.float64) ** 2) if len(w) else 0.0
                self.pool[lo:hi] = torch.from_numpy(host).to(self.device)

    def __len__(self):
        return len(self.split)

    def draw(self, index):
        """(image view (1024,), utterance number, label) of `SplitData.draw(index)` under the same `random` state; no
        file is opened."""
        views = self.split.image[index]
        view, u = plan_draw(self.frames[index], len(views), random, index)
        return views[view], u, self.split.labels[index]

    def waves(self, utterances, aug=None, step=0, uids=None):
        """The (item, utterance number) pairs as one flat fp32 device buffer of 16 kHz clips, perturbed under `aug` (a
        WaveAug; None: copied bit for bit): (flat, offsets int64 in floats, lens int64, plan or None).  `uids`: the id of
        each clip in the draws, its position in the list by default."""
        from . import _lib, ops
        lib = _lib.load()
        flat_ids = np.array([self.first[i] + u for i, u in utterances], dtype=np.int64)
        if len(flat_ids) == 0 or int(self.offsets[flat_ids].min()) < 0:
            raise _lib.S2IError("ResidentWaveSet.waves: %s" % ("no utterances" if len(flat_ids) == 0 else
                                "utterance %r has under %d frames and is not stored"
                                % (utterances[int(np.argmin(self.offsets[flat_ids]))], MIN_FRAMES)))
        B = len(flat_ids)
        lens_in = self.samples[flat_ids]
        plan = None
        rate = np.full(B, audio.SAMPLE_RATE, dtype=np.int64)
        out_lens = lens_in.copy()
        if aug is not None:
            uids = np.arange(B) if uids is None else np.asarray(uids)
            plan = ops.waveaug_plan(aug.policy, aug.seed, step, uids, lens_in, self.stored_lens, self.stored_q, self.T)
            rate, out_lens = plan["rate"], plan["out_len"]
        with torch.cuda.device(self.device):
            flat, out_offsets = render(*_stretch(self.pool, self.offsets[flat_ids], lens_in, plan), rate, out_lens)
            flat = _reverberate(flat, out_offsets, plan, aug, step)
            if plan is not None and (np.any(plan["g_white"] != 0) or np.any(plan["g_babble"] != 0)):
                table = ops.wave_mix_table(plan, self.stored_offsets, self.stored_lens)
                ops.wave_mix(flat, out_offsets, out_lens, table, aug.seed, step, pool=self.pool)
        return flat, out_offsets, out_lens, plan

    def mel(self, utterances, aug=None, step=0, uids=None):
        """[B, 1, T, 40] log-mel of a list of (item, utterance number) pairs and their frame counts (int64 ndarray), of
        the clips as stored or, under `aug`, perturbed: `audio.log_mel`'s three launches on the flat batch in place."""
        flat, offsets, lens, _ = self.waves(utterances, aug, step, uids)
        B, dev = len(lens), self.device
        with torch.cuda.device(dev):
            out = torch.empty((B, 1, self.T, audio.N_MELS), dtype=torch.float32, device=dev)
            audio.launch(audio.prepare_flat(flat, offsets, lens, self.T, dev), out, "nhwc")
        nf = 1 + lens // audio.HOP
        return out, np.minimum(nf, self.T).astype(np.int64)

    def batches(self, batch_size, device, shuffle, order=None, aug=None, step=None):
        """The batches of `SplitData.batches`: (mel_nhwc [B, 1, T, 40], cap_lens, image_feature [B, 1024], label [B]),
        with its `random` calls in its order.  `order`, where given, is the list of items to go through and `shuffle` is
        not looked at.  `aug` (a WaveAug) perturbs every utterance; `step` is then a callable that returns the counter of
        the draws when a batch is made (a trainer's `steps`, the value before the step's increment) and the clip's id is
        its position in the batch.  The frame counts and cap_lens are the perturbed clips'."""
        from . import _lib
        if _resolve(device) != _resolve(self.device):
            raise _lib.S2IError("the waveform pool is on %s, batches were asked for on %s: there is no CPU fallback and no "
                                "copy between devices" % (self.device, device))
        if aug is not None and not callable(step):
            raise ValueError("ResidentWaveSet.batches: aug needs step, a callable that returns the draw counter")
        for items, drawn in self.plan_batches(batch_size, shuffle, order):
            mel, frames = self.mel([(i, u) for i, (_, u, _) in zip(items, drawn)], aug, int(step()) if aug is not None else 0)
            image = torch.from_numpy(np.stack([v for v, _, _ in drawn])).float()
            yield mel, (frames // MIN_FRAMES).tolist(), image, torch.tensor([c for _, _, c in drawn], dtype=torch.int64)

    def plan_batches(self, batch_size, shuffle, order=None):
        """(items, their draws) batch by batch: every `random` call of an epoch of `SplitData.batches`, in its order, and
        nothing else (host only)."""
        if order is None:
            order = list(range(len(self)))
            if shuffle:
                random.shuffle(order)
        for s in range(0, len(order), batch_size):
            items = order[s:s + batch_size]
            yield items, [self.draw(i) for i in items]
