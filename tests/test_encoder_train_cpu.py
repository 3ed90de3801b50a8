"""CPU side of the speech-encoder head training: the fp64 restatement (tests/encoder_train_ref.py) against the oracle,
against autograd through nn.LSTM on packed sequences and against a literal transcription of the reference's loss; the new
ABI symbols; HeadTrainer's host-side behaviour (no kernel runs here)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import encoder_train_ref as R
from encoder_ref import small_encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("s2i_lstm_train_step", "s2i_lstm_train_cell", "s2i_lstm_bwd_step", "s2i_lstm_bwd_cell", "s2i_lstm_bias_grad",
               "s2i_encoder_loss_workspace_bytes", "s2i_encoder_loss")


def _lstm(E, H, D, params):
    rnn = nn.LSTM(E, H, num_layers=1, batch_first=True, bidirectional=D == 2).double()
    names = [n + s for s in ["", "_reverse"][:D] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    with torch.no_grad():
        for n, p in zip(names, params):
            getattr(rnn, n).copy_(p)
    return rnn, names


@pytest.mark.parametrize("case", [(3, 8, 32, 8, 2), (4, 8, 32, 16, 1)])
def test_restated_head_equals_the_oracle(case):
    from oracle import speech_encoder_oracle as orc
    B, L, E, H, D = case
    lens = R.case_lens(B, L)
    x, params, _, _ = R.head_case(B, L, E, H, D, lens)
    _, names = _lstm(E, H, D, params)
    p = {"RNN." + n: v for n, v in zip(names, params)}
    torch.set_default_dtype(torch.float64)
    try:
        out_o = orc.lstm_packed(p, x, lens, H, D == 2)
    finally:
        torch.set_default_dtype(torch.float32)
    out, sent, _, _ = R.lstm_head(x, lens, params)
    assert R.rel_err(out, out_o) < 1e-12 and R.rel_err(sent, out_o.mean(-2)) < 1e-12


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", [(3, 8, 32, 8, 2), (5, 8, 32, 16, 1)])
def test_restated_head_gradients_equal_autograd_through_nn_lstm(case, pattern):
    B, L, E, H, D = case
    lens = R.case_lens(B, L)
    x, params, g_out, g_sent = R.head_case(B, L, E, H, D, lens)
    ref = R.head_run(x, lens, params, g_out, g_sent, pattern)
    rnn, names = _lstm(E, H, D, params)
    xr = x.clone().requires_grad_(True)
    packed = pack_padded_sequence(xr, torch.tensor(lens), batch_first=True)
    out, (hn, cn) = rnn(packed)
    out = pad_packed_sequence(out, batch_first=True, total_length=L)[0]
    sent = out.mean(1)
    obj = ((out * g_out).sum() if pattern in ("out", "both") else 0) + ((sent * g_sent).sum() if pattern != "out" else 0)
    grads = torch.autograd.grad(obj, [xr] + [getattr(rnn, n) for n in names])
    assert R.rel_err(ref["out"], out) < 1e-12 and R.rel_err(ref["sent"], sent) < 1e-12
    assert R.rel_err(ref["hn"], hn) < 1e-12 and R.rel_err(ref["cn"], cn) < 1e-12
    assert R.rel_err(ref["dx"], grads[0]) < 1e-11
    for a, b in zip(ref["dparams"], grads[1:]):
        assert R.rel_err(a, b) < 1e-11


def _reference_loss(source, target, label, loss_diff, loss_same, jel=True, l1=False, lambda_l1=1, distill=False, distill_T=2,
                    lambda_distill=1):
    """JointEmbeddingLoss and LossFunc.__call__ transcribed (jel.py:17-43, train_audio_encoder.py:327-361)."""
    fea_txt, fea_img = source, target
    if jel:
        batchsize = fea_img.size(0)
        num_class = fea_txt.size(0)
        score = torch.mm(fea_img, fea_txt.transpose(0, 1))
        score_abs = score - score.diag()
        selected_idx_diff = (label.unsqueeze(0).repeat([batchsize, 1]) != label.unsqueeze(1))
        selected_idx_same = (label.unsqueeze(0).repeat([batchsize, 1]) == label.unsqueeze(1))
        ld = score_abs[selected_idx_diff] + 1
        ls = score_abs[selected_idx_same]
        loss = (loss_diff * ld[ld > 0].sum() + loss_same * ls[ls > 0].sum())
        _, max_idx = score.max(dim=1)
        acc_batch = (max_idx == torch.LongTensor(range(score.shape[1]))).sum().item()
        acc_batch = 100 * (acc_batch / batchsize)
        vj = loss / (batchsize * num_class)
    else:
        vj, acc_batch = torch.zeros(()).double(), 0
    v1 = torch.nn.L1Loss()(source / torch.norm(source), target / torch.norm(target)) if l1 else torch.zeros(()).double()
    if distill:
        s_, t_ = F.log_softmax(source, dim=1), F.softmax(target.div(distill_T), dim=1)
        vd = F.kl_div(s_, t_, reduction="mean")
    else:
        vd = torch.zeros(()).double()
    return {"loss": vj + v1 * lambda_l1 + vd * lambda_distill, "loss_jel": vj, "loss_l1": v1, "loss_distill": vd,
            "accu": acc_batch}


@pytest.mark.parametrize("flags", list(R.LOSS_FLAGS))
@pytest.mark.parametrize("B,C", [(5, 32), (37, 64)])
def test_restated_loss_equals_the_reference_arithmetic(B, C, flags):
    audio, image, label = R.loss_case(B, C)
    _, _, score, score_abs, same = R.jel_loss(audio, image, label, 1, 1)
    off = ~torch.eye(B, dtype=torch.bool)
    assert bool((same & off).any()), "labels must repeat"
    assert bool((torch.where(same, score_abs, score_abs + 1)[off].abs() > 1e-6).all())
    top2 = score.topk(2, dim=1)[0]
    assert bool((top2[:, 0] - top2[:, 1] > 1e-6).all())
    kw = R.LOSS_FLAGS[flags]
    got, grad = R.loss_run(audio, image, label, **kw)
    a = audio.clone().requires_grad_(True)
    ref = _reference_loss(a, image, label, kw.get("loss_diff", 1), kw.get("loss_same", 1),
                          **{k: v for k, v in kw.items() if k not in ("loss_diff", "loss_same")})
    (rgrad,) = torch.autograd.grad(ref["loss"], [a])
    for k in ("loss", "loss_jel", "loss_l1", "loss_distill"):
        assert R.rel_err(got[k], ref[k]) < 1e-12, k
    assert float(got["accu"]) == float(ref["accu"])
    assert R.rel_err(grad, rgrad) < 1e-11


def test_restated_loss_with_every_flag_off_is_zero():
    audio, image, label = R.loss_case(5, 32)
    got, grad = R.loss_run(audio, image, label, jel=False)
    assert all(float(v) == 0.0 for v in got.values()) and float(grad.abs().sum()) == 0.0


def test_mutants_differ_from_the_restatement():
    case = (3, 8, 32, 8, 2)
    lens = R.case_lens(3, 8)
    x, params, g_out, g_sent = R.head_case(*case, lens)
    ref = R.head_run(x, lens, params, g_out, g_sent, "both")
    for mutant, key in (("reset", "hn"), ("mean_len", "sent"), ("rev_L", "out")):
        assert R.rel_err(R.head_run(x, lens, params, g_out, g_sent, "both", mutant)[key], ref[key]) > 1e-2, mutant
    audio, image, label = R.loss_case(37, 64)
    for mutant, kw in (("diag_row", dict(jel=True)), ("l1_row", dict(jel=False, l1=True))):
        assert R.rel_err(R.loss_run(audio, image, label, mutant=mutant, **kw)[1], R.loss_run(audio, image, label, **kw)[1]) > 1e-2


def test_new_abi_symbols_are_declared_bound_and_exported():
    from speech_to_image_translation_without_text_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2i_hip.h")).read()
    declared = set(re.findall(r"\b(s2i_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    # argument checks run before anything touches a device
    assert lib.s2i_lstm_bwd_step(None, None, None, None, None, None, None, 4, 8, 512, 2, 0, 1, None, None, None) != 0
    assert lib.s2i_encoder_loss(None, None, None, 4, 8, 1.0, 1.0, 1, 1.0, 1.0, 2.0, None, 0, None, None, None) != 0
    assert lib.s2i_encoder_loss_workspace_bytes(64) == (2 * 64 * 64 + 9 * 64 + 2) * 4


def test_ops_surface():
    from speech_to_image_translation_without_text_amd import _lib, ops
    assert issubclass(ops.LstmSentence, torch.autograd.Function) and issubclass(ops.EncoderLoss, torch.autograd.Function)
    assert callable(ops.lstm_sentence) and callable(ops.encoder_loss)
    with pytest.raises(_lib.S2IError):
        ops.lstm_params(nn.LSTM(8, 8, num_layers=2, batch_first=True))


def test_head_trainer_optimises_exactly_the_rnn_parameters():
    from speech_to_image_translation_without_text_amd import _lib, encoder_train
    net = small_encoder(True, 64)
    tr = encoder_train.HeadTrainer(net)
    opt = [id(p) for g in tr.optimizer.param_groups for p in g["params"]]
    assert sorted(opt) == sorted(id(p) for p in net.RNN.parameters()) and len(opt) == 8
    assert not (set(opt) & {id(p) for p in net.Conv.parameters()})
    g0 = tr.optimizer.param_groups[0]
    assert isinstance(tr.optimizer, torch.optim.Adam) and g0["lr"] == 1e-3 and g0["weight_decay"] == 1e-5
    assert isinstance(tr.scheduler, torch.optim.lr_scheduler.StepLR) and tr.scheduler.step_size == 30
    assert not net.training
    net2 = small_encoder(False, 64)
    net2.rnn_layers = 2
    with pytest.raises(_lib.S2IError):
        encoder_train.HeadTrainer(net2)


def test_saved_checkpoint_loads_through_load_encoder(tmp_path):
    from speech_to_image_translation_without_text_amd import encoder_train
    from speech_to_image_translation_without_text_amd.extract_audio_feature import load_encoder
    from encoder_ref import build_encoder
    net = build_encoder()
    path = str(tmp_path / "epoch_3.pth")
    encoder_train.HeadTrainer(net).save(path, 3)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["meta"] == {"epoch": 3} and set(ckpt) == {"meta", "state_dict"}
    back = load_encoder(path, bidirectional=True)
    assert not back.training
    for (k, a), (k2, b) in zip(net.state_dict().items(), back.state_dict().items()):
        assert k == k2 and torch.equal(a, b)


def test_cli_help_says_single_gpu():
    from speech_to_image_translation_without_text_amd import train_encoder_head
    text = train_encoder_head.get_parser().format_help()
    assert "single GPU" in text
    for opt in ("--model", "--dataset", "--data_dir", "--output_dir", "--epoch", "--batch_size", "--bidirectional", "--jel_flag",
                "--l1_flag", "--distill_flag", "--loss_diff", "--loss_same", "--lambda_l1", "--lambda_distill", "--distill_T",
                "--learning_rate", "--lr_scheduler_step_size", "--lr_scheduler_gamma", "--eval_every"):
        assert opt in text, opt
