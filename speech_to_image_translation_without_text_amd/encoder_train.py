"""Training the speech encoder on the MI355X kernels (the reference's Audio_to_Image/train_audio_encoder.py:168-216,
308-361, 460-480): HeadTrainer fine-tunes the recurrent head with the conv stack frozen, EncoderTrainer trains all of it.

HeadTrainer: the conv stack of a CNNRNN runs frozen, exactly as inference runs it (eval-mode BatchNorm folded into the
convolutions); its output [B, 1, L, 1024] is the seam.  Behind it, ops.lstm_sentence (LSTM forward that stores its gates, backward
through time) and ops.encoder_loss (joint-embedding loss + L1 + distillation) give the gradients of `RNN.*`, which
torch.optim.Adam (L2 weight decay, as the reference) and StepLR update: 6.3 M parameters, plumbing.  The model stays in
.eval() mode throughout: CNNRNN.forward keeps refusing training mode, and with one LSTM layer nn.LSTM's dropout is a
no-op, so train and eval agree.

EncoderTrainer: the same step with ops.conv_stack_train in front (train-mode BatchNorm, temporal-conv and pool gradients),
which consumes the gradient ops.lstm_sentence returns for the seam; Adam then updates Conv.* and RNN.*.  Train-mode
BatchNorm is a property of this entry point: the module flag stays .eval() and CNNRNN.forward keeps refusing training
mode.  fp32, one LSTM layer, frame counts that are powers of two; bf16, more LSTM layers and dropout are not built.

Both trainers take `fused_adam=True`: the trained parameters are re-homed into one flat fp32 buffer (trainer.FlatNet, as
the GAN networks), their .grad views alias a second one, and the optimiser is s2i_increment + ONE s2i_adam_l2_step launch
(torch.optim.Adam's L2 form, `gscale g + weight_decay p`) instead of torch.optim.Adam over 34 tensors (the head: 8); StepLR's rule is
applied to the host-side learning rate in end_epoch.  `distributed=True` (implies fused_adam) is the data-parallel step of
the reference's DistributedDataParallel run: the flat parameters and the BatchNorm buffers are broadcast from rank 0 at
construction, every step sums the whole flat gradient buffer over the ranks in one torch.distributed.all_reduce between
backward and the optimiser launch, and 1 / world_size is folded into that launch.  The loss and the train-mode BatchNorm
statistics stay per rank, as under DDP; rank 0's running statistics are the ones a checkpoint keeps.

state_dict() / load_state_dict() carry the whole training state (weights, Adam moments and step counts in torch.optim.Adam's
own state_dict form for either optimiser, the epoch and the learning rate): a fresh trainer that loads it continues bit for bit.

`specaug='freq=2x8,time=2x40,ratio=0.2'` (ops.specaug_policy; default '': off, and then no draw, launch or allocation is
added) masks every training batch in front of features(): SpecAugment's frequency and time masks over the
64 * cap_lens[b] frames the LSTM consumes, masked cells set to the utterance's mean (ops.specaug).  The masks of a step
are a function of (specaug_seed, steps, b) alone, `steps` being the counter before the step's increment, so there is no
generator state: `steps` is already in state_dict(), and a trainer that loads a state continues the mask sequence exactly.
A checkpoint without training state (save(); the CLIs' plain --resume epoch_N.pth) restarts the counter at 0, so its
masks repeat the run's first ones: that path carries no Adam moments either and was never exact.  step_features, embed,
evaluate and save never see a mask.

`clip_grad=F` (> 0), `accum=N` (> 1) and `skip_nonfinite=True` are off by default, and then no launch, allocation or bit
of the step changes; any of them implies fused_adam.  With clip_grad or skip_nonfinite the optimiser step is
FlatNet._adam_guarded: one fixed-order fp64 reduction over the flat gradient buffer (ops.grad_sumsq), one small launch that
keeps the norm, torch.nn.utils.clip_grad_norm_'s coefficient and the decision to apply on the device and counts the Adam step
(ops.grad_clip_scale), and the Adam launch that reads them: no host round trip, bit-reproducible.  The norm is that of the
gradient the optimiser uses, behind 1 / (world * accum).  A gradient whose sum of squares is not finite (a NaN or an inf
anywhere in it) is skipped on that path, with or without clip_grad: parameters, moments and the Adam step stay bit for bit as
they were, weight decay included, and the skip is counted; skip_nonfinite selects the path without clipping.
grad_stats() reads the record.  `accum=N`: the flat gradient buffer is zeroed before the first micro-batch of a group only
and autograd adds the others into it; the all-reduce and the optimiser step follow the N-th, scaled by 1 / (world * N);
end_epoch flushes an incomplete group of k by 1 / (world * k), so no gradient is pending at an epoch boundary.  `steps`
keeps counting step() calls (the augmentations' counter), `updates` counts optimiser steps, BatchNorm's running statistics
move with every micro-batch as under torch.  Accumulation is not a larger batch: the joint-embedding loss takes its
negatives from the micro-batch, so N micro-batches of B give the mean of N losses over B, not one loss over N * B, and
train-mode BatchNorm normalises each micro-batch by its own statistics.
"""
import copy
import warnings

import numpy as np
import torch

from . import _lib, ops, retrieval


class HeadTrainer:
    def __init__(self, model, lr=1e-3, weight_decay=1e-5, step_size=30, gamma=0.2, loss_diff=1, loss_same=1, jel=True,
                 l1=False, lambda_l1=1, distill=False, distill_T=2, lambda_distill=1, fused_adam=False, distributed=False,
                 specaug='', specaug_seed=0, clip_grad=0.0, accum=1, skip_nonfinite=False):
        if model.rnn_layers != 1:
            raise _lib.S2IError("HeadTrainer supports rnn_layers=1 (the reference's default)")
        self.clip_grad, self.accum, self.skip_nonfinite = float(clip_grad), int(accum), bool(skip_nonfinite)
        if not self.clip_grad >= 0.0 or self.accum < 1:
            raise ValueError("clip_grad must be >= 0 (0: off) and accum >= 1, got %r and %r" % (clip_grad, accum))
        self.guarded = self.clip_grad > 0.0 or self.skip_nonfinite      # the optimiser step is FlatNet's three-launch one
        self.model = model.eval()
        self.distributed = bool(distributed)
        self.world = torch.distributed.get_world_size() if self.distributed else 1
        self.step_size, self.gamma, self.epoch, self.steps = int(step_size), gamma, 0, 0
        self.updates, self.pending = 0, 0       # optimiser steps (skipped ones included); micro-batches in the open group
        self.specaug, self.specaug_seed = ops.specaug_policy(specaug), int(specaug_seed)      # None: off
        self.flat = self.optimizer = self.scheduler = None
        if fused_adam or self.distributed or self.guarded or self.accum > 1:
            from .trainer import FlatNet
            self.flat = FlatNet(model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay,
                                params=self._trained())
            if self.distributed:        # identical start on every rank (DDP's initial broadcast)
                torch.distributed.broadcast(self.flat.p, 0)
                for buf in model.buffers():
                    torch.distributed.broadcast(buf, 0)
            self._stale()
        else:
            self.optimizer = torch.optim.Adam(self._trained(), lr=lr, weight_decay=weight_decay)
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=step_size, gamma=gamma)
        self.params = ops.lstm_params(model.RNN)       # after the re-homing: the flat buffer's views
        self.loss_args = dict(loss_diff=loss_diff, loss_same=loss_same, jel=jel, l1=l1, lambda_l1=lambda_l1, distill=distill,
                              distill_T=distill_T, lambda_distill=lambda_distill)

    def _trained(self):
        return list(self.model.RNN.parameters())

    def _stale(self):
        # the kernels write running_mean / running_var / num_batches_tracked and, with fused_adam, the parameters through
        # raw pointers, which leaves the version counters CNNRNN._prepare keys its folded weights by unchanged: drop the cache
        self.model._prepared = None

    @property
    def lr(self):
        return self.flat.lr if self.flat is not None else self.optimizer.param_groups[0]["lr"]

    @property
    def device(self):
        return self.params[0].device

    @torch.no_grad()
    def features(self, mel_nhwc):
        """The frozen conv stack on NHWC log-mel [B, 1, T, 40] (audio.log_mel(..., layout="nhwc")) -> [B, 1, T/64, 1024]."""
        _lib.load()
        _lib.require_device()
        n_mels = self.model.Conv[1][0].kernel_size[0]
        if mel_nhwc.dim() != 4 or mel_nhwc.shape[1] != 1 or mel_nhwc.shape[3] != n_mels:
            raise _lib.S2IError("HeadTrainer.features: expected [B, 1, T, %d], got %s" % (n_mels, tuple(mel_nhwc.shape)))
        return self.model._conv_features(mel_nhwc.contiguous())

    @staticmethod
    def _sorted(cap_lens, *tensors):
        """Descending by length, as batch_process sorts a batch (sort_torch_data; ties keep their order)."""
        lens = torch.as_tensor(cap_lens).cpu()
        lens, order = torch.sort(lens, dim=0, descending=True, stable=True)
        return lens.tolist(), [t.index_select(0, order.to(t.device)) for t in tensors]

    def step_features(self, feat, cap_lens, image_feature, label):
        """One optimiser step from conv features [B, 1, L, E]: what step() does behind features()."""
        if self.model.training:
            self.model.eval()
        dev = self.device
        lens, (feat, image_feature, label) = self._sorted(cap_lens, feat, image_feature.to(dev).float(), label.to(dev))
        _, sent = ops.lstm_sentence(feat, lens, *self.params)
        loss = ops.encoder_loss(sent, image_feature, label, **self.loss_args)
        if self.flat is None:
            self.optimizer.zero_grad(set_to_none=True)
            loss["loss"].backward()
            self.optimizer.step()
            self.updates += 1
        else:
            if self.pending == 0:
                self.flat.zero_grad()       # one memset; never set_to_none, which would detach the views
            loss["loss"].backward()         # a group's further micro-batches are added into the flat buffer by autograd
            self.pending += 1
            if self.pending >= self.accum:
                self._update()
        self.steps += 1
        return {k: v.detach() for k, v in loss.items()}

    def _update(self):
        """The optimiser step on the `pending` micro-batches summed in the flat gradient buffer, scaled by
        1 / (world * pending).  Under `distributed` the norm is taken behind the all-reduce, on a buffer every rank holds
        alike: all ranks clip by the same coefficient and skip together, a non-finite value on one rank reaching all of them
        through the sum."""
        if self.distributed:            # on the current stream, behind the backward's launches
            torch.distributed.all_reduce(self.flat.g, op=torch.distributed.ReduceOp.SUM)
        if self.guarded:
            self.flat.adam(1.0 / (self.world * self.pending), max_norm=self.clip_grad, guard=True)
        else:
            self.flat.adam(1.0 / (self.world * self.pending))
        self.pending = 0
        self.updates += 1
        self._stale()

    def grad_stats(self, reset=False):
        """FlatNet.grad_stats of the guarded step (clip_grad or skip_nonfinite; one synchronisation), else None."""
        return self.flat.grad_stats(reset) if self.guarded else None

    def step(self, mel_nhwc, cap_lens, image_feature, label):
        """Sort by length, conv features, lstm_sentence, the loss, backward, Adam.  Returns the loss dict (device tensors:
        loss, loss_jel, loss_l1, loss_distill, accu).  With a `specaug` policy the batch is masked first (ops.specaug, into a
        new tensor: the caller's batch is left alone) over each utterance's 64 * cap_lens[b] frames, the ones the LSTM
        consumes, with the step counter as the generator's counter."""
        if self.specaug is not None:
            mel_nhwc = ops.specaug(mel_nhwc.detach().float().contiguous(), [64 * int(n) for n in cap_lens], self.specaug,
                                   self.specaug_seed, self.steps)
        return self.step_features(self.features(mel_nhwc), cap_lens, image_feature, label)

    def end_epoch(self):
        """StepLR: the learning rate is multiplied by gamma every step_size epochs.  An incomplete accumulation group of k
        micro-batches is flushed first, as an optimiser step scaled by 1 / (world * k) at the epoch's learning rate."""
        if self.pending:
            self._update()
        self.epoch += 1
        if self.flat is None:
            self.scheduler.step()
        elif self.epoch % self.step_size == 0:
            self.flat.lr *= self.gamma

    def skip_epochs(self, n):
        """Advance the schedule over n finished epochs (a resumed run; the Adam moments start afresh unless the checkpoint
        carries them: load_state_dict)."""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)    # StepLR stepped before the first optimiser step
            for _ in range(int(n)):
                self.end_epoch()

    @torch.no_grad()
    def embed(self, mel_nhwc, cap_lens):
        """Sentence embeddings [B, D*H] in the caller's order (the inference path)."""
        lens, (x,) = self._sorted(cap_lens, mel_nhwc)
        order = torch.sort(torch.as_tensor(cap_lens).cpu(), dim=0, descending=True, stable=True)[1].to(x.device)
        sent = self.model.forward_nhwc(x, lens)[1]
        out = torch.empty_like(sent)
        out[order] = sent
        return out

    def evaluate(self, loader):
        """(accuracy %, AP@50 %) of retrieval.eval_class over batches of (mel_nhwc, cap_lens, image_feature, label)."""
        audio, image, labels = [], [], []
        for mel, cap_lens, image_feature, label in loader:
            audio.append(self.embed(mel.to(self.device), cap_lens).cpu().numpy())
            image.append(torch.as_tensor(image_feature).float().cpu().numpy())
            labels.append(torch.as_tensor(label).cpu().numpy())
        return retrieval.eval_class(np.concatenate(audio), np.concatenate(image), np.concatenate(labels))

    def state_dict(self):
        """The whole training state on the CPU: the model's state_dict, `epoch` (finished epochs), `steps`, the current
        `lr`, and `optimizer`, which is always a torch.optim.Adam.state_dict() over the trained parameters in _trained()
        order -- torch's own, or with fused_adam the flat moments and step count in that form
        (train_state.flat_to_adam_state) -- so a state written by either kind of trainer loads into the other, and into the
        reference's resume_model.  With clip_grad, accum or skip_nonfinite on, `updates` counts the optimiser steps and `skipped` those of them the non-finite guard
        dropped; the Adam `step` in `optimizer` is the number of applied updates, updates - skipped.  A state is taken between
        accumulation groups (end_epoch closes an open one); with micro-batches pending it is refused."""
        from . import train_state
        if self.pending:
            raise ValueError("state_dict: %d micro-batches of an accumulation group are pending; call end_epoch() first"
                             % self.pending)
        skipped = 0
        if self.flat is None:
            opt = train_state.to_cpu(self.optimizer.state_dict())
        else:
            f = self.flat
            if self.guarded:        # before the first guarded step there is no record yet: the count a loaded state brought
                skipped = f.grad_stats()["skipped_total"] if f.clip is not None else f.skipped_before
            opt = train_state.flat_to_adam_state(f.m.cpu(), f.v.cpu(), f.sync_step_count(), [tuple(p.shape) for p in f.params],
                                                 f.offsets, f.lr, f.betas, f.eps, f.weight_decay)
        state = {"state_dict": {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                 "epoch": int(self.epoch), "steps": int(self.steps), "lr": float(self.lr), "optimizer": opt}
        if self.guarded or self.accum > 1:      # with the options off the state has the keys it always had
            state.update(updates=int(self.updates), skipped=int(skipped))
        return state

    def load_state_dict(self, state):
        """Inverse of state_dict(), in place: with fused_adam the parameters stay views of the flat buffer.  The learning
        rate is the state's own, not StepLR's rule replayed."""
        from . import train_state
        self.model.load_state_dict(state["state_dict"])
        self.epoch, self.steps = int(state["epoch"]), int(state["steps"])
        self.updates, self.pending = int(state.get("updates", self.steps)), 0
        lr = float(state["lr"])
        if self.flat is None:
            # a copy: torch keeps the `step` tensors it is handed and increments them in place
            self.optimizer.load_state_dict(copy.deepcopy(state["optimizer"]))
            for group, base in zip(self.optimizer.param_groups, self.scheduler.base_lrs):
                group["lr"] = lr
                group.setdefault("initial_lr", base)
            sch = self.scheduler
            sch.last_epoch, sch._step_count, sch._last_lr = self.epoch, self.epoch + 1, [lr] * len(self.optimizer.param_groups)
        else:
            f = self.flat
            m, v, step = train_state.adam_state_to_flat(state["optimizer"], f.sizes, f.offsets, f.total)
            with torch.no_grad():
                f.m.copy_(m)
                f.v.copy_(v)
            f.step_count = step
            f.step_dev.fill_(step)
            f.skipped_before = int(state.get("skipped", 0))
            if f.clip is not None:
                f.clip.reset_stats()
            f.lr = lr
            ops.refresh_packed(f.params)
            ops.invalidate_derived(f.params)
        self._stale()

    def save(self, path, epoch):
        """The reference's checkpoint layout (Audio_to_Image/trainer.py save_checkpoint), read by
        extract_audio_feature.load_encoder."""
        state = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        torch.save({"meta": {"epoch": int(epoch)}, "state_dict": state}, path)


class EncoderTrainer(HeadTrainer):
    """HeadTrainer's interface, training every parameter: `features` is ops.conv_stack_train with gradients enabled, the
    optimiser is the reference's Adam(model.parameters(), lr, weight_decay=1e-5) with StepLR.  embed / evaluate run the
    inference path, which folds the running statistics training has produced."""

    def _trained(self):
        return list(self.model.parameters())

    def features(self, mel_nhwc):
        """The conv stack in training mode on NHWC log-mel [B, 1, T, 40] -> [B, 1, T/64, 1024], with a graph behind it;
        updates the running statistics."""
        _lib.load()
        _lib.require_device()
        n_mels = self.model.Conv[1][0].kernel_size[0]
        if mel_nhwc.dim() != 4 or mel_nhwc.shape[1] != 1 or mel_nhwc.shape[3] != n_mels:
            raise _lib.S2IError("EncoderTrainer.features: expected [B, 1, T, %d], got %s" % (n_mels, tuple(mel_nhwc.shape)))
        T = mel_nhwc.shape[2]
        if T < 64 or T & (T - 1):
            raise _lib.S2IError("EncoderTrainer.features: the frame count must be a power of two >= 64, got %d" % T)
        self._stale()
        with torch.enable_grad():
            return ops.conv_stack_train(self.model.Conv, mel_nhwc.detach().float().contiguous())

    def step_features(self, feat, cap_lens, image_feature, label):
        try:
            return super().step_features(feat, cap_lens, image_feature, label)
        finally:
            self._stale()
