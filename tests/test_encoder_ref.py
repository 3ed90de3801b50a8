"""tests/encoder_ref.py (the fp64 restatement the encoder's GPU launches are held to) against the fp32 oracle, on the
CPU: folding the BatchNorms as CNNRNN._prepare() does and composing the per-launch functions reproduces
oracle/speech_encoder_oracle.forward, which tests/golden/encoder.npz pins to the reference's own outputs.

Bound.  The oracle is stock fp32 torch: nine convolutions of up to K = 2560 terms each, then 32 recurrent steps.  Its
rounding reaches the outputs as a few 1e-6 of their magnitude (measured, see the printed figures: words 6e-7 / 1.0e-6, sent
3e-7 / 5e-7 on the two cases); the fp64 side contributes nothing at that scale.  ORACLE_TOL = 2e-5 of (|ref| + rms) leaves
room for another BLAS / thread count and is 50 times below the 1e-3 the end-to-end tests use."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import encoder_ref as E  # noqa: E402
from helpers import GOLDEN  # noqa: E402

ORACLE_TOL = 2e-5


def _ratio(got, ref):
    """max |got - ref| / (|ref| + rms(ref)): element-wise relative error with the tensor's own scale as the floor."""
    ref = ref.double()
    return float(((got.double() - ref).abs() / (ref.abs() + ref.pow(2).mean().sqrt())).max())


def _against_oracle(net, x, lens, hd, bidirectional, what):
    from oracle import speech_encoder_oracle as orc
    with torch.no_grad():
        words_o, sent_o = orc.forward({k: v.clone() for k, v in net.state_dict().items()}, x, lens, hd, bidirectional)
        nhwc = x.double().transpose(1, 2).unsqueeze(1).contiguous()            # (B, 40, T) -> [B, 1, T, 40]
        words, sent = E.encode(E.fold(net), nhwc, lens)
    assert words.dtype == torch.float64 and words.shape == words_o.shape and sent.shape == sent_o.shape
    rw, rs = _ratio(words_o, words), _ratio(sent_o, sent)
    print("%s: oracle vs fp64 composition: words %.2e, sent %.2e (bound %.1e)" % (what, rw, rs, ORACLE_TOL))
    assert rw <= ORACLE_TOL and rs <= ORACLE_TOL, (what, rw, rs)
    for b in range(x.shape[0]):
        assert float(words[b, :, int(lens[b]):].abs().max() if int(lens[b]) < words.shape[2] else 0.0) == 0.0
    return words, sent


def test_composition_reproduces_the_oracle_on_the_golden_inputs():
    gold = np.load(os.path.join(GOLDEN, "encoder.npz"), allow_pickle=False)
    x, lens = E.mge.make_inputs()
    words, sent = _against_oracle(E.build_encoder(), x, lens, 512, True, "golden B=3 bidirectional")
    # and with it the reference's own outputs, at the tolerance the oracle is pinned with
    assert torch.allclose(words.float(), torch.from_numpy(gold["words"]), rtol=1e-3, atol=1e-5)
    assert torch.allclose(sent.float(), torch.from_numpy(gold["sent"]), rtol=1e-3, atol=1e-6)


def test_composition_reproduces_the_oracle_unidirectional():
    """The CLIs' default: one direction, Hd = 1024; ragged lengths including 1 and the full 8 steps."""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(4, 40, 512, generator=g) * 20 - 40
    _against_oracle(E.small_encoder(False, 1024), x, torch.tensor([8, 5, 2, 1]), 1024, False, "B=4 unidirectional")


def test_single_pieces_against_stock_modules():
    """Each launch function against the stock torch module it restates, in fp64 (1e-12)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 32, 8, generator=g, dtype=torch.float64)
    for k, st, pd in ((3, 1, 1), (17, 2, 8), (13, 2, 6), (9, 2, 4), (5, 2, 2)):
        w = torch.randn(6, 8, k, generator=g, dtype=torch.float64)
        b = torch.randn(6, generator=g, dtype=torch.float64)
        ref = torch.relu(torch.nn.functional.conv1d(x[:, 0].transpose(1, 2), w, b, stride=st, padding=pd))
        got = E.conv1d(x, w, b, k, st, pd)
        assert got.shape == (2, 1, ref.shape[2], 6)
        assert torch.allclose(got[:, 0].transpose(1, 2), ref, rtol=1e-12, atol=1e-12), (k, st, pd)
    xn = -1.0 - torch.rand(1, 1, 8, 4, generator=g, dtype=torch.float64)       # all negative: zero padding would win
    assert torch.equal(E.maxpool_w3s2(xn)[0, 0, 0], xn[0, 0, :2].max(0)[0])
    assert torch.equal(E.maxpool_w3s2(xn)[0, 0, 3], xn[0, 0, 5:8].max(0)[0])
    # the recurrence against nn.LSTM on packed sequences, both directions
    Hd, In, L = 8, 5, 6
    rnn = torch.nn.LSTM(In, Hd, batch_first=True, bidirectional=True).double()
    feat = torch.randn(3, L, In, generator=g, dtype=torch.float64)
    lens = [6, 3, 1]
    with torch.no_grad():
        packed = torch.nn.utils.rnn.pack_padded_sequence(feat, lens, batch_first=True)
        ref, _ = torch.nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], batch_first=True, total_length=L)
        w_ih = torch.cat((rnn.weight_ih_l0, rnn.weight_ih_l0_reverse), 0)
        b = torch.cat((rnn.bias_ih_l0 + rnn.bias_hh_l0, rnn.bias_ih_l0_reverse + rnn.bias_hh_l0_reverse), 0)
        got = E.lstm_sequence(E.k1(feat, w_ih, b), lens, [rnn.weight_hh_l0, rnn.weight_hh_l0_reverse], Hd)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(E.time_mean(got), got.sum(1) / L, rtol=1e-14, atol=0)
    assert [E.time_index(s, 3, False) for s in range(4)] == [0, 1, 2, None]
    assert [E.time_index(s, 3, True) for s in range(4)] == [2, 1, 0, None]
