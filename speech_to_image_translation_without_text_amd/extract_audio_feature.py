"""WAV files -> `audio_features_<switch>.pickle` / `audio_features_lens_<switch>.pickle`, the sentence embeddings that
datasets.py trains and evaluates on (Audio_to_Image/extract_audio_feature.py:25-96).

    python -m speech_to_image_translation_without_text_amd.extract_audio_feature --model encoder.pt \\
        --audio_switch 0 --dataset birds --bidirectional --data_dir data/birds

For each split (train, test) it reads `<data_dir>/<split>.json`, takes `audio_base_path` + each item's `audio` (birds) or
`wav` (flowers) list, and writes `<data_dir>/<split>/audio_features_<switch>.pickle` (N/10, 10, 1024) float32 and
`audio_features_lens_<switch>.pickle` (N/10, 10) int64 (the n_frames of each file).  A relative `audio_base_path` is
taken relative to the working directory, as the reference does.  The files are 16 kHz PCM16; --resample takes any rate
from 4 to 192 kHz, PCM or float, 1 to 8 channels, as librosa.load(path, 16000) does for the reference (audio.to_16k).

The reference processes files in chunks of 10, in file order: it sorts a chunk by n_frames (descending), replaces the
shortest item's data and length by the second-shortest's when it has fewer than 64 frames, encodes with
cap_lens = n_frames // 64 and restores the order.  The encoder treats every item on its own, so here the chunk rule is
applied to the lengths first (`chunk_sources`) and any number of files runs as one GPU batch: log-mel (audio.log_mel,
NHWC) straight into CNNRNN.forward_nhwc.

--waveaug 'speed=1.1,white=1@20:20' --waveaug_seed S writes the embeddings of perturbed audio instead (ops.waveaug_policy,
wave_loader.perturb): every file at a drawn speed, tempo (tempo=F/F/..., duration only) and pitch (pitch=S/S/...
semitones, pitch only; `retrieval` over such files measures the sensitivity to a shifted voice), in a drawn room (reverb=P@LO:HI@DLO:DHI, T60 in seconds and the
direct-to-reverberant ratio in dB) and under white noise at a drawn signal-to-noise ratio, the draws a
function of (S, 0, the file's running number in its split) alone, so a run repeats bit for bit.  The `retrieval` CLI over
such files measures how accuracy, AP@50 and recall@k fall with noise or tempo.  babble= needs a pool of training
utterances and is refused here.  Without the flag nothing changes.
"""
import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import audio, datasets
from .speech_encoder import CNNRNN

CHUNK = 10
MIN_FRAMES = 64
MAX_READERS = 16


def chunk_sources(frames, chunk=CHUNK):
    """For each item, the item whose log-mel and length it is encoded with under the reference's chunk rule (itself,
    unless it is the shortest of its chunk of `chunk` with fewer than 64 frames: then the chunk's second-shortest).
    Ties keep file order (a stable descending sort)."""
    frames = np.asarray(frames)
    src = np.arange(len(frames))
    for s in range(0, len(frames), chunk):
        idx = np.arange(s, min(s + chunk, len(frames)))
        order = idx[np.argsort(-frames[idx], kind="stable")]
        if frames[order[-1]] < MIN_FRAMES:
            if len(order) < 2:
                raise ValueError("item %d has %d frames (< %d) and no chunk neighbour to stand in for it"
                                 % (order[-1], frames[order[-1]], MIN_FRAMES))
            src[order[-1]] = order[-2]
    return src


def load_encoder(path, bidirectional=False, rnn_layers=1, device=None):
    """CNNRNN(40, 1024, 1024, 1024) from a checkpoint (Audio_to_Image/trainer.py:18-54): {'state_dict': ...} or a bare
    state_dict, a `module.` prefix stripped, loaded strictly, in .eval() mode."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ckpt, dict) and "state_dict" in ckpt and isinstance(ckpt["state_dict"], dict):
        state = ckpt["state_dict"]
    elif isinstance(ckpt, dict) and ckpt and all(torch.is_tensor(v) for v in ckpt.values()):
        state = ckpt
    else:
        raise RuntimeError("No state_dict found in checkpoint file %s" % path)
    if next(iter(state)).startswith("module."):
        state = {k[len("module."):]: v for k, v in state.items()}
    model = CNNRNN(40, embedding_dim=1024, nhidden=1024, nsent=1024, bidirectional=bidirectional,
                   rnn_layers=rnn_layers)
    model.load_state_dict(state, strict=True)
    model.eval()
    return model.to(device) if device is not None else model


def read_wavs(paths, workers=MAX_READERS, resample=False):
    """The files as 16 kHz mono float32 waveforms.  `resample` takes any rate and sample format `audio.read_audio`
    accepts and converts on the current GPU (`audio.to_16k`: device tensors); without it, `audio.read_wav`'s arrays."""
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_READERS, workers, len(paths)))) as pool:
        if resample:
            return audio.to_16k(list(pool.map(audio.read_audio, paths)))
        return list(pool.map(audio.read_wav, paths))


def encode_waveforms(model, waves, batch_size=240, chunk=CHUNK, aug=None):
    """Sentence embeddings (N, D) float32 and n_frames (N,) int64 of the waveforms, equal to the reference's
    chunk-of-10 processing for any batch_size.  `aug` (a wave_loader.WaveAug; None: off) perturbs each waveform first,
    waveform k drawing with step 0 and uid k: the perturbed lengths, which the chunk rule needs before anything runs,
    come from the host-side plan, and the perturbed audio of one batch at a time is on the device."""
    if aug is not None:
        from . import ops
        from .wave_loader import perturb
        plan = ops.waveaug_plan(aug.policy, aug.seed, 0, np.arange(len(waves)), [len(w) for w in waves])
        frames = np.array([audio.n_frames(n) for n in plan["out_len"]], dtype=np.int64)
    else:
        frames = np.array([audio.n_frames(len(w)) for w in waves], dtype=np.int64)
    src = chunk_sources(frames, chunk)
    dev = next(model.parameters()).device
    feats = None
    for s in range(0, len(waves), batch_size):
        items = np.arange(s, min(s + batch_size, len(waves)))
        need = np.unique(src[items])
        clips = [waves[i] for i in need]
        if aug is not None:
            clips = perturb(clips, aug, dev, step=0, uids=need)
        logspec, nf = audio.log_mel(clips, layout="nhwc", device=dev)
        pos = np.searchsorted(need, src[items])
        cap = nf[pos] // MIN_FRAMES
        order = np.argsort(-cap, kind="stable")                  # the encoder takes cap_lens sorted descending
        x = logspec.index_select(0, torch.from_numpy(pos[order]).to(dev))
        sent = model.forward_nhwc(x, cap[order].tolist())[1]
        out = torch.empty_like(sent)
        out[torch.from_numpy(order).to(dev)] = sent
        out = out.cpu().numpy()
        if feats is None:
            feats = np.empty((len(waves), out.shape[1]), dtype=np.float32)
        feats[items] = out
    return feats, frames


def split_files(data_dir, split, dataset):
    with open(os.path.join(data_dir, "%s.json" % split)) as f:
        meta = json.load(f)
    key = "audio" if dataset == "birds" else "wav"
    return [os.path.join(meta["audio_base_path"], name) for d in meta["data"] for name in d[key]]


def extract_split(model, data_dir, split, dataset, audio_switch, batch_size=240, resample=False, aug=None):
    """`aug` (a wave_loader.WaveAug; None: off) perturbs every file first, inside the encode loop."""
    files = split_files(data_dir, split, dataset)
    if not files or len(files) % CHUNK:
        raise ValueError("%s split has %d files: need a positive multiple of %d" % (split, len(files), CHUNK))
    feats, frames = encode_waveforms(model, read_wavs(files, resample=resample), batch_size, aug=aug)
    out_dir = os.path.join(data_dir, split)
    datasets.save_embedding_pickle(feats.reshape(-1, CHUNK, feats.shape[1]),
                                   os.path.join(out_dir, "audio_features_%s.pickle" % audio_switch))
    datasets.save_embedding_pickle(frames.reshape(-1, CHUNK),
                                   os.path.join(out_dir, "audio_features_lens_%s.pickle" % audio_switch))
    return feats, frames


def get_parser():
    p = argparse.ArgumentParser(description="extract_audio_feature")
    p.add_argument("--model", type=str, default="./Audio_to_Image/model/model_best.pt",
                   help="CNNRNN checkpoint ({'state_dict': ...} or a bare state_dict)")
    p.add_argument("--audio_switch", type=str, default="0", help="audio switch to be extracted")
    p.add_argument("--dataset", choices=["birds", "flowers"], default="birds")
    p.add_argument("--bidirectional", action="store_true", default=False)
    p.add_argument("--rnn_layers", type=int, default=1)
    p.add_argument("--data_dir", type=str, default=None, help="directory with <split>.json (default ./data/<dataset>)")
    p.add_argument("--batch_size", type=int, default=240, help="utterances per GPU batch (any size)")
    p.add_argument("--splits", type=str, default="train,test")
    p.add_argument("--resample", action="store_true", default=False,
                   help="accept WAVs of any rate (4-192 kHz), PCM 8/16/24/32-bit or float 32/64-bit, 1-8 channels: "
                        "decoded, mixed down and resampled to 16 kHz on the GPU (audio.to_16k)")
    p.add_argument("--waveaug", type=str, default="",
                   help="write the embeddings of perturbed audio, e.g. 'speed=1.1,reverb=1@0.3:0.3@5:5,white=1@20:20' "
                        "(ops.waveaug_policy; speed=, tempo=F/F/..., pitch=S/S/... in semitones, "
                        "reverb=P@T60LO:T60HI@DRRLO:DRRHI and white= are taken; "
                        "babble= is refused: it needs a pool of training utterances); default '': off")
    p.add_argument("--waveaug_seed", type=int, default=0, help="seed of --waveaug's draws")
    return p


def make_aug(spec, seed):
    """The WaveAug of --waveaug (None for ''), refused with the reason where the spec is bad or asks for babble."""
    from . import ops
    try:
        if ops.waveaug_policy(spec) is None:
            return None
    except ValueError as e:
        raise SystemExit("--waveaug: %s" % e)
    from .wave_loader import WaveAug
    aug = WaveAug(spec, seed)
    if aug.policy["babble"] is not None:
        raise SystemExit("--waveaug: babble= draws its interferers from a pool of training utterances, which an extraction "
                         "does not have: use speed=, tempo=, pitch=, reverb= and white= here")
    return aug


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    aug = make_aug(args.waveaug, args.waveaug_seed)
    data_dir = args.data_dir or os.path.join(".", "data", args.dataset)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = load_encoder(args.model, args.bidirectional, args.rnn_layers, dev)
    for split in args.splits.split(","):
        feats, _ = extract_split(model, data_dir, split, args.dataset, args.audio_switch, args.batch_size, args.resample, aug)
        print("%s: %d utterances -> %s" % (split, len(feats), os.path.join(data_dir, split)))


if __name__ == "__main__":
    main()
