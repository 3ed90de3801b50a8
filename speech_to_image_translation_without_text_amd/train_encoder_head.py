"""Fine-tune the LSTM head of a speech-encoder checkpoint on WAV recordings, conv stack frozen (the recurrent part of
Audio_to_Image/train_audio_encoder.py).  Single GPU.

    python -m speech_to_image_translation_without_text_amd.train_encoder_head --model encoder.pt --dataset birds \\
        --data_dir data/birds --output_dir output/encoder_head --epoch 100 --batch_size 64 --bidirectional --jel_flag

`<data_dir>/train.json` and `test.json` are the files extract_audio_feature reads: `audio_base_path`,
`image_feature_path` (a pickle of N x (views, 1024) image features) and per item an `audio` (birds) / `wav` (flowers) list
and a `class`.  Per item and epoch one random utterance with at least 64 frames and one random image view are drawn with
`random`, as BirdDataset.__getitem__ does.  Every --eval_every epochs (and after the last) the test split is scored with
retrieval.eval_class and `epoch_<n>.pth`, `latest.pth` and, on a new best test accuracy, `best.pth` are written in the
reference's checkpoint layout, which extract_audio_feature --model reads.  --resident reads every WAV once and keeps both
splits' log-mel rows in device memory (speech_loader.ResidentSpeechSet): the same batches, one launch each.
"""
import argparse
import json
import os
import random
import shutil
import time

import numpy as np
import torch

from . import audio, datasets
from .encoder_train import HeadTrainer
from .extract_audio_feature import MIN_FRAMES, load_encoder

MAX_DRAWS = 64


class SplitData:
    """One split: the JSON's items, the image-feature pickle and the class labels (0-based)."""

    def __init__(self, data_dir, split, dataset):
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
        """(image view (1024,), waveform, label): a random view and a random utterance of at least 64 frames."""
        views = self.image[index]
        image = views[random.randint(0, len(views) - 1)]
        names = self.items[index][self.key]
        for _ in range(MAX_DRAWS):
            wave = audio.read_wav(os.path.join(self.audio_base, names[random.randint(0, len(names) - 1)]))
            if audio.n_frames(len(wave)) >= MIN_FRAMES:
                return image, wave, self.labels[index]
        raise ValueError("item %d: no utterance with at least %d frames in %d draws" % (index, MIN_FRAMES, MAX_DRAWS))

    def batches(self, batch_size, device, shuffle):
        """Batches of (mel_nhwc [B, 1, 2048, 40], cap_lens, image_feature [B, 1024], label [B])."""
        order = list(range(len(self)))
        if shuffle:
            random.shuffle(order)
        for s in range(0, len(order), batch_size):
            drawn = [self.draw(i) for i in order[s:s + batch_size]]
            mel, frames = audio.log_mel([w for _, w, _ in drawn], layout="nhwc", device=device)
            image = torch.from_numpy(np.stack([v for v, _, _ in drawn])).float()
            yield mel, (frames // MIN_FRAMES).tolist(), image, torch.tensor([c for _, _, c in drawn], dtype=torch.int64)


def get_parser(description="fine-tune the speech encoder's LSTM head (conv stack frozen); single GPU", model_required=True,
               output_dir="./output/Audio_to_Image/encoder_head", seed=None):
    """The flags of this CLI; train_encoder builds its own from the same list (--model optional, a default seed)."""
    p = argparse.ArgumentParser(description=description)
    p.add_argument("--model", type=str, required=model_required, default="" if not model_required else None,
                   help="CNNRNN checkpoint to start from")
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
    p.add_argument("--resident_workers", type=int, default=16, help="threads that read the WAV files for --resident")
    return p


def check_args(args):
    if args.batch_size < 1 or args.epoch < 1 or args.eval_every < 1:
        raise SystemExit("--batch_size, --epoch and --eval_every must be >= 1")


def trainer_kwargs(args):
    return dict(lr=args.learning_rate, weight_decay=1e-5, step_size=args.lr_scheduler_step_size,
                gamma=args.lr_scheduler_gamma, loss_diff=args.loss_diff, loss_same=args.loss_same, jel=args.jel_flag,
                l1=args.l1_flag, lambda_l1=args.lambda_l1, distill=args.distill_flag, distill_T=args.distill_T,
                lambda_distill=args.lambda_distill)


def make_resident(split, name, dev, workers):
    """`split` behind a speech_loader.ResidentSpeechSet, with one line about the pool."""
    from .speech_loader import ResidentSpeechSet
    t0 = time.perf_counter()
    resident = ResidentSpeechSet(split, dev, workers=workers)
    torch.cuda.synchronize(dev)
    print("resident %s: %d utterances, %d rows, %d bytes, %.2f s" % (name, len(resident.row_offsets), resident.pool.shape[0],
                                                                    resident.nbytes, time.perf_counter() - t0))
    return resident


def run(trainer, args, dev):
    """The epoch loop, evaluation and checkpoints shared with train_encoder -> best test accuracy."""
    data_dir = args.data_dir or os.path.join(".", "data", args.dataset)
    train, test = SplitData(data_dir, "train", args.dataset), SplitData(data_dir, "test", args.dataset)
    if args.resident:
        train, test = (make_resident(s, name, dev, args.resident_workers) for s, name in ((train, "train"), (test, "test")))
    os.makedirs(args.output_dir, exist_ok=True)
    best = -1.0
    for epoch in range(1, args.epoch + 1):
        total, seen = None, 0
        for mel, cap_lens, image, label in train.batches(args.batch_size, dev, shuffle=True):
            loss = trainer.step(mel, cap_lens, image, label)
            part = torch.stack([loss["loss"], loss["accu"]]) * len(cap_lens)       # stays on the device until the epoch ends
            total = part if total is None else total + part
            seen += len(cap_lens)
        trainer.end_epoch()
        mean_loss, mean_accu = (total / seen).tolist()
        print("epoch %d: loss %.4f, batch accu %.2f" % (epoch, mean_loss, mean_accu))
        if epoch % args.eval_every == 0 or epoch == args.epoch:
            accu, ap50 = trainer.evaluate(test.batches(args.batch_size, dev, shuffle=False))
            path = os.path.join(args.output_dir, "epoch_%d.pth" % epoch)
            trainer.save(path, epoch)
            shutil.copyfile(path, os.path.join(args.output_dir, "latest.pth"))
            if accu > best:
                best = accu
                shutil.copyfile(path, os.path.join(args.output_dir, "best.pth"))
            print(json.dumps({"epoch": epoch, "test_accu": accu, "test_ap50": ap50, "best_accu": best}))
    return best


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)
    if args.seed is not None:
        random.seed(args.seed)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = load_encoder(args.model, args.bidirectional, 1, dev)
    return run(HeadTrainer(model, **trainer_kwargs(args)), args, dev)


if __name__ == "__main__":
    main()
