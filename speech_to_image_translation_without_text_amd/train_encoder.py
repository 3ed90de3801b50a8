"""Train the whole speech encoder (conv stack and LSTM head) on WAV recordings, from the reference's seeded initialisation
or from a checkpoint (Audio_to_Image/train_audio_encoder.py).  fp32, one LSTM layer; one GPU, or data-parallel over
several with --distributed.

    python -m speech_to_image_translation_without_text_amd.train_encoder --dataset birds --data_dir data/birds \\
        --output_dir output/encoder --epoch 100 --batch_size 64 --bidirectional --jel_flag

The flags, the data handling (`<data_dir>/train.json`, `test.json`, one random utterance and image view per item and
epoch), the per-epoch and evaluation lines and the checkpoints (`epoch_<n>.pth`, `latest.pth`, `best.pth`, read by
extract_audio_feature --model) are train_encoder_head's.  --model is optional: without it the encoder is
CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=...) built under torch.manual_seed(--seed), which is how the
reference initialises it.  --seed (default 1234) also seeds `random` (utterance / view draws, batch order).
--fused_adam, --resume, --state_every and --distributed are train_encoder_head's too (its docstring has the details): the reference's
own way to run this training, run_audio_encoder.sh, is data-parallel, and here that is

    python -m torch.distributed.run --nproc-per-node 8 -m speech_to_image_translation_without_text_amd.train_encoder \
        --distributed --dataset birds --data_dir data/birds --output_dir output/encoder --epoch 1000 --bidirectional --jel_flag

Every rank builds the same seeded model (or loads the same checkpoint) and rank 0's parameters and BatchNorm buffers are
broadcast; --resident keeps the whole pool on every rank.  --specaug and --waveaug (speed, tempo, pitch, reverberation, white noise
and babble on the training waveforms, wave_loader.py) are train_encoder_head's as well.
Not built: bf16, more than one LSTM layer (and so nn.LSTM's dropout).
"""
import torch

from .encoder_train import EncoderTrainer
from .extract_audio_feature import load_encoder
from .speech_encoder import CNNRNN
from .train_encoder_head import (SplitData, check_args, get_parser as _head_parser, run, seed_draws,  # noqa: F401
                                 train_and_close, trainer_kwargs)

DEFAULT_SEED = 1234


def get_parser():
    return _head_parser(description="train the speech encoder (conv stack + LSTM head); single GPU, or one process per GPU "
                        "with --distributed", model_required=False,
                        output_dir="./output/Audio_to_Image/encoder", seed=DEFAULT_SEED)


def build_model(args):
    """The reference's initialisation: the constructor's own RNG draws under torch.manual_seed(seed)."""
    torch.manual_seed(args.seed)
    return CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=args.bidirectional).eval()


def main(argv=None):
    args = get_parser().parse_args(argv)
    check_args(args)

    def make_trainer(dev):
        seed_draws(args)
        start = args.resume or args.model
        model = load_encoder(start, args.bidirectional, 1, dev) if start else build_model(args).to(dev)
        return EncoderTrainer(model, **trainer_kwargs(args))
    return train_and_close(make_trainer, args)


if __name__ == "__main__":
    main()
