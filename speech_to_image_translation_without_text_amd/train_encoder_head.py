"""Fine-tune the LSTM head of a speech-encoder checkpoint on WAV recordings, conv stack frozen (the recurrent part of
Audio_to_Image/train_audio_encoder.py).

    python -m speech_to_image_translation_without_text_amd.train_encoder_head --model encoder.pt --dataset birds \\
        --data_dir data/birds --output_dir output/encoder_head --epoch 100 --batch_size 64 --bidirectional --jel_flag

`<data_dir>/train.json` and `test.json` are the files extract_audio_feature reads: `audio_base_path`,
`image_feature_path` (a pickle of N x (views, 1024) image features) and per item an `audio` (birds) / `wav` (flowers) list
and a `class`.  Per item and epoch one random utterance with at least 64 frames and one random image view are drawn with
`random`, as BirdDataset.__getitem__ does.  Every --eval_every epochs (and after the last) the test split is scored with
retrieval.eval_class and `epoch_<n>.pth`, `latest.pth` and, on a new best test accuracy, `best.pth` are written in the
reference's checkpoint layout, which extract_audio_feature --model reads.  --resident reads every WAV once and keeps both
splits' log-mel rows in device memory (speech_loader.ResidentSpeechSet): the same batches, one launch each.  --resample
takes WAVs of any rate from 4 to 192 kHz, PCM or float, 1 to 8 channels, converted to 16 kHz mono on the GPU per batch
(audio.to_16k), also under --resident; without it the files are 16 kHz PCM16 as before.

--fused_adam keeps the trained parameters in one flat buffer and steps them with one fused Adam launch
(encoder_train.py).  --resume PATH loads a checkpoint this CLI wrote and continues at its `meta.epoch` + 1 with the learning
rate StepLR has reached by then; the Adam moments start afresh unless the checkpoint carries them (the reference's layout
has an `optimizer` field for them; `epoch_<n>.pth`, `latest.pth` and `best.pth` leave it out).  It stands in for --model, and
`best.pth` becomes the best of the resumed run alone unless the checkpoint records the accuracy it was saved at.
--state_every N writes the checkpoint that carries both: every N-th epoch and after the last, rank 0 atomically replaces
`<output_dir>/state.pth` with `meta` {epoch, best_accu}, `state_dict`, `optimizer` (always a torch.optim.Adam.state_dict()
over the trained parameters, also under --fused_adam) and `rng`, the state of every rank's `random` (train_state.py).
--resume state.pth restores all of it -- moments, step counts, the learning rate, `best` and each rank's draws -- so the
epochs that follow are, bit for bit, those of a run that was never stopped.  The state is taken behind an epoch's
scheduled evaluation (--eval_every) and in front of the closing evaluation of a run's last epoch, which a longer run would
not have made: neither that evaluation's draws nor its accuracy enter the state.  A state written by another number of
ranks is refused.
--distributed trains data-parallel, one process per GPU, as the reference's run_audio_encoder.sh does under
torch.distributed.launch:

    python -m torch.distributed.run --nproc-per-node 8 -m speech_to_image_translation_without_text_amd.train_encoder_head \
        --distributed --model encoder.pt ...

RANK, WORLD_SIZE and LOCAL_RANK come from the launcher; --dist_backend (default nccl, i.e. RCCL) names the process group.
Every rank loads the same model; an epoch's item order is drawn from random.Random(seed + epoch), alike on every rank, and
rank r takes every world-th item of it from the r-th on (`shard_order`: DistributedSampler's padding and stride), so all
ranks run ceil(N / world / batch_size) steps.  The global `random`, which draws views and utterances, is seeded seed + rank.
Rank 0 alone prints, evaluates and writes checkpoints while the others wait at a barrier.  --resident keeps the WHOLE pool
on every rank.
--specaug 'freq=2x8,time=2x40,ratio=0.2' masks every training batch on the GPU (SpecAugment: count x maximum width of the
frequency and time masks, masked cells set to the utterance's mean; encoder_train.py, ops.specaug).  The masks come from a
counter-based generator keyed by --seed (plus the rank under --distributed) and counted by the trainer's step counter:
they take nothing from `random`, so the batches drawn are the same with and without the option, and a --state_every state
continues the mask sequence exactly.  A plain --resume epoch_N.pth restarts the counter at 0.  Evaluation and the
checkpoints never see a mask.  Default '': off.
--waveaug 'speed=0.9/1.0/1.1,white=0.3@5:25,babble=0.2@0:15' perturbs every training utterance as a waveform, in front of
the log-mel front end (wave_loader.py, ops.waveaug_policy): a speed factor drawn from the list, white noise and another
training utterance (babble) each with its probability at a signal-to-noise ratio drawn from LO:HI dB.
reverb=P@LO:HI@DLO:DHI adds a room between the speed and the noise: with probability P the clip is convolved on the GPU
with an impulse response of T60 drawn from LO:HI seconds at a direct-to-reverberant ratio drawn from DLO:DHI dB.
tempo=F/F/... and pitch=S/S/... vary the speaker: a drawn tempo factor in [0.5, 2] divides the duration at an unchanged
pitch, a drawn number of semitones in [-12, 12] moves the pitch at an unchanged duration; both run a phase vocoder on the
GPU (s2i_time_stretch) in front of the resampler, so the order is stretch, resample, reverb, noise.  It keeps the
training split's 16 kHz samples in device memory (wave_loader.ResidentWaveSet; --waveaug_max_bytes refuses a pool above
it) whether or not --resident is given; the test split stays as it is and is never perturbed.  The draws come from a
counter-based generator keyed by --waveaug_seed (default --seed; the rank is added to either under --distributed) and counted by the
trainer's step counter, with the batch position as the utterance's id: they take nothing from `random`, and a
--state_every state continues the sequence exactly.  A plain --resume epoch_N.pth restarts the counter at 0.  With
--specaug the waveform is perturbed first and the masks go over its log-mel.  Default '': off, and then nothing of it is
imported, drawn, launched or allocated.
--clip_grad F clips the global gradient norm to F, --skip_nonfinite skips (and counts) an optimiser step whose gradient
holds a NaN or an inf, --accum N sums the gradients of N batches per optimiser step (an epoch's last, incomplete group is
stepped at the epoch's end); each implies --fused_adam, and all of it runs inside the fused optimiser with nothing read
back per step (encoder_train.py).  With --clip_grad or --skip_nonfinite the epoch line gains
`gnorm mean/max A/B, clipped k/n, skipped s` (one read per epoch: the norm of the gradient the optimiser used over the n
applied steps, how many of them were clipped, how many steps were skipped), and state.pth's `meta` carries `steps`,
`updates` and `skipped`.  Defaults 0, 1 and off: every line and file is then what it was.
"""
import argparse
import json
import os
import random
import shutil
import time

import numpy as np
import torch

from . import audio, datasets, ops
from .encoder_train import HeadTrainer
from .extract_audio_feature import MIN_FRAMES, load_encoder

MAX_DRAWS = 64


class SplitData:
    """One split: the JSON's items, the image-feature pickle and the class labels (0-based)."""

    def __init__(self, data_dir, split, dataset, resample=False):
        self.resample = bool(resample)     # any WAV audio.read_audio accepts, converted by audio.to_16k per batch
        with open(os.path.join(data_dir, "%s.json" % split)) as f:
            meta = json.load(f)
        self.audio_base = meta["audio_base_path"]
        self.items = meta["data"]
        self.key = "audio" if dataset == "birds" else "wav"
        self.image = datasets.load_embedding_pickle(meta["image_feature_path"])
        if len(self.image) != len(self.items):
            raise ValueError("%s: %d items but %d image-feature rows" % (split, len(self.items), len(self.image)))
        self.labels = [int(str(d["class"]).split(".")[0]) - 1 for d in self.items]

    def __len__(self):
        return len(self.items)

    def draw(self, index):
        """(image view (1024,), waveform, label): a random view and a random utterance of at least 64 frames.  With
        `resample` the waveform is the file's `audio.read_audio` pair, its 16 kHz length taken from the header."""
        views = self.image[index]
        image = views[random.randint(0, len(views) - 1)]
        names = self.items[index][self.key]
        for _ in range(MAX_DRAWS):
            if self.resample:
                clip = audio.read_audio(os.path.join(self.audio_base, names[random.randint(0, len(names) - 1)]))
                if audio.n_frames(audio.resampled_length(clip[0].frames, clip[0].rate)) >= MIN_FRAMES:
                    return image, clip, self.labels[index]
                continue
            wave = audio.read_wav(os.path.join(self.audio_base, names[random.randint(0, len(names) - 1)]))
            if audio.n_frames(len(wave)) >= MIN_FRAMES:
                return image, wave, self.labels[index]
        raise ValueError("item %d: no utterance with at least %d frames in %d draws" % (index, MIN_FRAMES, MAX_DRAWS))

    def batches(self, batch_size, device, shuffle, order=None):
        """Batches of (mel_nhwc [B, 1, 2048, 40], cap_lens, image_feature [B, 1024], label [B]).  `order`, where given, is
        the list of items to go through (a rank's share of an epoch, shard_order) and `shuffle` is not looked at."""
        if order is None:
            order = list(range(len(self)))
            if shuffle:
                random.shuffle(order)
        for s in range(0, len(order), batch_size):
            drawn = [self.draw(i) for i in order[s:s + batch_size]]
            waves = [w for _, w, _ in drawn]
            if self.resample:
                waves = audio.to_16k(waves, device)
            mel, frames = audio.log_mel(waves, layout="nhwc", device=device)
            image = torch.from_numpy(np.stack([v for v, _, _ in drawn])).float()
            yield mel, (frames // MIN_FRAMES).tolist(), image, torch.tensor([c for _, _, c in drawn], dtype=torch.int64)


def shard_order(order, rank, world):
    """Rank `rank`'s share of an epoch's item order among `world` ranks, by torch's DistributedSampler rules: the order is
    padded with its own head (repeated if need be) to a multiple of `world`, and the rank takes every world-th entry from
    its own number on.  Every share has ceil(len(order) / world) entries."""
    order = list(order)
    if not 0 <= rank < world:
        raise ValueError("shard_order: rank %d of %d" % (rank, world))
    total = -(-len(order) // world) * world
    padded = order
    while order and len(padded) < total:
        padded = padded + order[:total - len(padded)]
    return padded[rank::world]


class _Parser(argparse.ArgumentParser):
    """--model is required (where the CLI requires it) unless --resume names the checkpoint to load."""
    model_required = False

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if self.model_required and not ns.model and not ns.resume:
            self.error("the following arguments are required: --model (or --resume)")
        return ns


def get_parser(description="fine-tune the speech encoder's LSTM head (conv stack frozen); single GPU, or one process per "
               "GPU with --distributed", model_required=True,
               output_dir="./output/Audio_to_Image/encoder_head", seed=None):
    """The flags of this CLI; train_encoder builds its own from the same list (--model optional, a default seed)."""
    p = _Parser(description=description)
    p.model_required = model_required
    p.add_argument("--model", type=str, default="", help="CNNRNN checkpoint to start from")
    p.add_argument("--dataset", choices=["birds", "flowers"], default="birds")
    p.add_argument("--data_dir", type=str, default=None, help="directory with train.json / test.json (default ./data/<dataset>)")
    p.add_argument("--output_dir", type=str, default=output_dir)
    p.add_argument("--epoch", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--bidirectional", action="store_true", default=False)
    p.add_argument("--learning_rate", type=float, default=1e-3)
    p.add_argument("--lr_scheduler_step_size", type=int, default=30)
    p.add_argument("--lr_scheduler_gamma", type=float, default=0.2)
    p.add_argument("--eval_every", type=int, default=5)
    p.add_argument("--loss_diff", type=float, default=1)
    p.add_argument("--loss_same", type=float, default=1)
    p.add_argument("--jel_flag", action="store_true", default=False)
    p.add_argument("--l1_flag", action="store_true", default=False)
    p.add_argument("--distill_flag", action="store_true", default=False)
    p.add_argument("--lambda_l1", type=float, default=1.0)
    p.add_argument("--lambda_distill", type=float, default=1.0)
    p.add_argument("--distill_T", type=float, default=2.0)
    p.add_argument("--seed", type=int, default=seed, help="seed of `random` (utterance / view draws, batch order)")
    p.add_argument("--resident", action="store_true", default=False,
                   help="keep both splits' log-mel rows in device memory (speech_loader.ResidentSpeechSet)")
    p.add_argument("--resample", action="store_true", default=False,
                   help="accept WAVs of any rate (4-192 kHz), PCM 8/16/24/32-bit or float 32/64-bit, 1-8 channels: "
                        "decoded, mixed down and resampled to 16 kHz on the GPU (audio.to_16k)")
    p.add_argument("--resident_workers", type=int, default=16, help="threads that read the WAV files for --resident")
    p.add_argument("--fused_adam", action="store_true", default=False,
                   help="flat parameter storage and one fused Adam launch per step (encoder_train.py)")
    p.add_argument("--distributed", action="store_true", default=False,
                   help="data-parallel training, one process per GPU (start under torch.distributed.run); implies --fused_adam")
    p.add_argument("--dist_backend", type=str, default="nccl", help="torch.distributed backend of --distributed")
    p.add_argument("--resume", type=str, default="",
                   help="checkpoint of this CLI to continue from, at its epoch + 1 (it stands in for --model; best.pth is "
                        "the best of the resumed run alone unless the file is a --state_every state.pth, which is "
                        "continued exactly)")
    p.add_argument("--state_every", type=int, default=0,
                   help="every this many epochs and after the last, replace <output_dir>/state.pth with the full training "
                        "state (weights, Adam moments, learning rate, best accuracy, every rank's `random`); 0 = never")
    p.add_argument("--specaug", type=str, default="",
                   help="SpecAugment of every training batch on the GPU, e.g. 'freq=2x8,time=2x40,ratio=0.2': count x maximum "
                        "width of the frequency and time masks, `ratio` the largest share of an utterance one time mask "
                        "may take (ops.specaug_policy); default '': off")
    p.add_argument("--waveaug", type=str, default="",
                   help="speed, tempo, pitch, reverberation and noise augmentation of every training utterance's waveform on the "
                        "GPU, e.g. 'speed=0.9/1.0/1.1,reverb=0.3@0.2:0.6@0:15,white=0.3@5:25,babble=0.2@0:15': speed factors, "
                        "reverb=P@T60LO:T60HI@DRRLO:DRRHI in seconds and dB, white= and babble=P@SNRLO:SNRHI in dB, "
                        "tempo=F/F/... factors in [0.5, 2] (duration only) and pitch=S/S/... semitones in [-12, 12] (pitch only) "
                        "(ops.waveaug_policy); keeps the training split's samples in device memory; default '': off")
    p.add_argument("--waveaug_seed", type=int, default=None,
                   help="seed of --waveaug's draws (default: --seed); under --distributed the rank is added to it, whether "
                        "it was given or defaulted, so that the ranks draw independently")
    p.add_argument("--waveaug_max_bytes", type=int, default=None,
                   help="refuse a waveform pool above this many bytes (default: no limit)")
    p.add_argument("--clip_grad", type=float, default=0.0,
                   help="clip the global gradient norm to this value inside the fused optimiser (clip_grad_norm_'s rule, on "
                        "the device); 0 = off; implies --fused_adam")
    p.add_argument("--accum", type=int, default=1,
                   help="accumulate the gradients of this many batches per optimiser step; implies --fused_adam")
    p.add_argument("--skip_nonfinite", action="store_true", default=False,
                   help="skip an optimiser step whose gradient holds a NaN or an inf (parameters, moments and the Adam step "
                        "stay as they were) and count it; implies --fused_adam")
    return p


def check_args(args):
    if args.batch_size < 1 or args.epoch < 1 or args.eval_every < 1:
        raise SystemExit("--batch_size, --epoch and --eval_every must be >= 1")
    if args.state_every < 0:
        raise SystemExit("--state_every must be >= 0")
    if not getattr(args, "clip_grad", 0.0) >= 0.0:
        raise SystemExit("--clip_grad must be >= 0 (0 = off)")
    if getattr(args, "accum", 1) < 1:
        raise SystemExit("--accum must be >= 1")
    try:
        ops.specaug_policy(getattr(args, "specaug", ""))
    except ValueError as e:
        raise SystemExit("--specaug: %s" % e)
    try:
        ops.waveaug_policy(getattr(args, "waveaug", ""))
    except ValueError as e:
        raise SystemExit("--waveaug: %s" % e)


def trainer_kwargs(args):
    """HeadTrainer's keywords.  The mask generator's seed is --seed, plus the rank under --distributed (once the process
    group exists), as seed_draws seeds `random`: the ranks mask independently."""
    specaug_seed = args.seed or 0
    if args.distributed and torch.distributed.is_available() and torch.distributed.is_initialized():
        specaug_seed += torch.distributed.get_rank()
    clip_grad, accum, skip = getattr(args, "clip_grad", 0.0), getattr(args, "accum", 1), getattr(args, "skip_nonfinite", False)
    return dict(lr=args.learning_rate, weight_decay=1e-5, step_size=args.lr_scheduler_step_size,
                gamma=args.lr_scheduler_gamma, loss_diff=args.loss_diff, loss_same=args.loss_same, jel=args.jel_flag,
                l1=args.l1_flag, lambda_l1=args.lambda_l1, distill=args.distill_flag, distill_T=args.distill_T,
                lambda_distill=args.lambda_distill,
                fused_adam=bool(args.fused_adam or clip_grad > 0 or accum > 1 or skip), distributed=args.distributed,
                specaug=getattr(args, "specaug", ""), specaug_seed=specaug_seed, clip_grad=clip_grad, accum=accum,
                skip_nonfinite=skip)


def make_resident(split, name, dev, workers, say=print, resample=False):
    """`split` behind a speech_loader.ResidentSpeechSet, with one line about the pool."""
    from .speech_loader import ResidentSpeechSet
    t0 = time.perf_counter()
    resident = ResidentSpeechSet(split, dev, workers=workers, resample=resample)
    torch.cuda.synchronize(dev)
    say("resident %s: %d utterances, %d rows, %d bytes, %.2f s" % (name, len(resident.row_offsets), resident.pool.shape[0],
                                                                  resident.nbytes, time.perf_counter() - t0))
    return resident


def make_wave_resident(split, dev, args, rank, say=print):
    """(the training split behind a wave_loader.ResidentWaveSet, with one line about the pool; the WaveAug of --waveaug).
    The seed is --waveaug_seed, or --seed where it is not given; under --distributed the rank is added to either."""
    from .wave_loader import ResidentWaveSet, WaveAug
    seed = (args.waveaug_seed if args.waveaug_seed is not None else (args.seed or 0)) + (rank if args.distributed else 0)
    aug = WaveAug(args.waveaug, seed)
    t0 = time.perf_counter()
    try:
        resident = ResidentWaveSet(split, dev, workers=args.resident_workers, resample=args.resample,
                                   max_bytes=args.waveaug_max_bytes)
    except ValueError as e:
        raise SystemExit("--waveaug: %s" % e)
    torch.cuda.synchronize(dev)
    say("resident train waveforms: %s, %.2f s" % (resident.message, time.perf_counter() - t0))
    return resident, aug


def init_device(args):
    """The device of this process.  Under --distributed: LOCAL_RANK's GPU and the process group (RANK and WORLD_SIZE from
    the launcher's environment), set up before any other GPU work."""
    if not args.distributed:
        return torch.device("cuda", torch.cuda.current_device())
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if args.dist_backend == "nccl":
        torch.distributed.init_process_group("nccl", device_id=dev)
    else:
        torch.distributed.init_process_group(args.dist_backend)
    return dev


def seed_draws(args):
    """Seed the global `random` (views, utterances, and the batch order of a single-process run): --seed, plus the rank
    under --distributed, so that the ranks draw independently."""
    seed = args.seed
    if args.distributed:
        seed = (seed or 0) + torch.distributed.get_rank()
    if seed is not None:
        random.seed(seed)


def resume_epoch(path):
    """`meta.epoch` of a checkpoint written by `run`."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or "meta" not in ckpt or "epoch" not in ckpt["meta"]:
        raise SystemExit("--resume %s: the checkpoint carries no meta.epoch" % path)
    return int(ckpt["meta"]["epoch"])


def write_state(trainer, path, epoch, best, distributed):
    """`path` replaced atomically by the full state behind `epoch` finished epochs (module docstring).  Every rank calls
    it: the `random` states are gathered; rank 0 writes."""
    from . import train_state
    rng = train_state.gather(random.getstate(), distributed)
    if distributed and torch.distributed.get_rank() != 0:
        return
    st = trainer.state_dict()
    meta = {"epoch": int(epoch), "best_accu": float(best)}
    if "updates" in st:     # --clip_grad, --accum, --skip_nonfinite: step() calls, optimiser steps and skipped ones part ways
        meta.update(steps=st["steps"], updates=st["updates"], skipped=st["skipped"])
    train_state.atomic_save({"format": train_state.FORMAT, "meta": meta,
                             "state_dict": st["state_dict"], "optimizer": st["optimizer"], "rng": rng}, path)


def resume_state(trainer, ckpt, path, rank, world):
    """Continue from a checkpoint with an `optimizer` field -> (first epoch, best accuracy so far).  The learning rate is
    the one the optimizer state records and the step count its parameters'; a file without `rng` or `best_accu` (the
    reference's own save_checkpoint writes neither) keeps this run's seeding and starts `best` anew."""
    from . import train_state
    if "format" in ckpt:
        train_state.check_format(ckpt, path)
    rng = train_state.rank_entry(ckpt["rng"], rank, world, path) if "rng" in ckpt else None     # refused before any change
    opt, meta = ckpt["optimizer"], ckpt.get("meta", {})
    steps = max([int(e["step"]) for e in opt["state"].values()] or [0])
    epoch = int(meta.get("epoch", 0))
    state = {"state_dict": ckpt["state_dict"], "epoch": epoch, "steps": int(meta.get("steps", steps)),
             "lr": opt["param_groups"][0]["lr"], "optimizer": opt}
    if "updates" in meta:
        state.update(updates=int(meta["updates"]), skipped=int(meta.get("skipped", 0)))
    trainer.load_state_dict(state)
    if rng is not None:
        random.setstate(train_state.as_tuple(rng))
    return epoch + 1, float(meta.get("best_accu", -1.0))


def train_and_close(make_trainer, args):
    """main() of both CLIs behind the parser: device (and process group), model and trainer, `run`, and the process
    group's end."""
    dev = init_device(args)
    try:
        return run(make_trainer(dev), args, dev)
    finally:
        if args.distributed:
            torch.distributed.destroy_process_group()


def run(trainer, args, dev):
    """The epoch loop, evaluation and checkpoints shared with train_encoder -> best test accuracy.  The number of
    optimiser steps taken is left in `trainer.steps` and, under --distributed, printed by every rank."""
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if args.distributed else (0, 1)
    say = print if rank == 0 else (lambda *a, **k: None)
    data_dir = args.data_dir or os.path.join(".", "data", args.dataset)
    # the test split is rank 0's alone: the other ranks never evaluate, and with --resident would fill a pool they never read
    names = ("train", "test") if rank == 0 else ("train",)
    splits = [SplitData(data_dir, name, args.dataset, resample=args.resample) for name in names]
    waveaug = ops.waveaug_policy(getattr(args, "waveaug", "")) is not None
    feed = {}           # what train.batches takes beyond SplitData's arguments
    if waveaug:         # the training split as waveforms; the other one as --resident says
        wave_train, aug = make_wave_resident(splits[0], dev, args, rank, say)
        feed = dict(aug=aug, step=lambda: trainer.steps)
    if args.resident:
        splits = [s if waveaug and name == "train" else make_resident(s, name, dev, args.resident_workers, say, args.resample)
                  for s, name in zip(splits, names)]
    if waveaug:
        splits[0] = wave_train
    train, test = splits[0], (splits[1] if rank == 0 else None)
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)
    first = 1
    best = -1.0        # of THIS run: a resumed run does not know the accuracy behind an earlier best.pth and replaces it
    if args.resume:
        ckpt = torch.load(args.resume, map_location="cpu", weights_only=True)
        if isinstance(ckpt, dict) and "optimizer" in ckpt:
            first, best = resume_state(trainer, ckpt, args.resume, rank, world)     # ... unless the state records it
        else:
            first = resume_epoch(args.resume) + 1
            trainer.skip_epochs(first - 1)
        del ckpt

    def evaluate(epoch, best):
        if rank == 0:
            accu, ap50 = trainer.evaluate(test.batches(args.batch_size, dev, shuffle=False))
            path = os.path.join(args.output_dir, "epoch_%d.pth" % epoch)
            trainer.save(path, epoch)
            shutil.copyfile(path, os.path.join(args.output_dir, "latest.pth"))
            if accu > best:
                best = accu
                shutil.copyfile(path, os.path.join(args.output_dir, "best.pth"))
            print(json.dumps({"epoch": epoch, "test_accu": accu, "test_ap50": ap50, "best_accu": best}))
        if args.distributed:
            torch.distributed.barrier()
        return best
    for epoch in range(first, args.epoch + 1):
        total, seen = None, 0
        order = None
        if args.distributed:
            order = list(range(len(train)))
            random.Random((args.seed or 0) + epoch).shuffle(order)       # alike on every rank
            order = shard_order(order, rank, world)
        for mel, cap_lens, image, label in train.batches(args.batch_size, dev, shuffle=True, order=order, **feed):
            loss = trainer.step(mel, cap_lens, image, label)
            part = torch.stack([loss["loss"], loss["accu"]]) * len(cap_lens)       # stays on the device until the epoch ends
            total = part if total is None else total + part
            seen += len(cap_lens)
        trainer.end_epoch()
        mean_loss, mean_accu = (total / seen).tolist()
        line = "epoch %d: loss %.4f, batch accu %.2f" % (epoch, mean_loss, mean_accu)
        gs = trainer.grad_stats(reset=True) if hasattr(trainer, "grad_stats") else None      # one read per epoch
        if gs is not None:
            line += ", gnorm mean/max %.4g/%.4g, clipped %d/%d, skipped %d" % (gs["norm_mean"], gs["norm_max"], gs["clipped"],
                                                                              gs["updates"], gs["skipped"])
        say(line)
        scheduled, last = epoch % args.eval_every == 0, epoch == args.epoch
        if scheduled:
            best = evaluate(epoch, best)
        if args.state_every > 0 and (epoch % args.state_every == 0 or last):
            write_state(trainer, os.path.join(args.output_dir, "state.pth"), epoch, best, args.distributed)
        if last and not scheduled:
            best = evaluate(epoch, best)        # the closing evaluation: behind the state, which a longer run continues
    if args.distributed:
        print("rank %d of %d: %d steps" % (rank, world, trainer.steps), flush=True)
    return best


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)

    def make_trainer(dev):
        seed_draws(args)
        model = load_encoder(args.resume or args.model, args.bidirectional, 1, dev)
        return HeadTrainer(model, **trainer_kwargs(args))
    return train_and_close(make_trainer, args)


if __name__ == "__main__":
    main()
