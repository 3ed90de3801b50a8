"""SpecAugment on the MI355X: s2i_specaug against the numpy restatement (tests/specaug_ref.py), and the trainers' option.

Bounds.  Cells outside the reference's masks equal x bit for bit.  The masked cells of an utterance hold one value within
(d + 2) 2^-24 mean|x_b| of the float64 mean, d = specaug_ref.depth(T) being the depth of the summation the header states
(22 at T = 128, 21 at T = 2048): d roundings of a same-sign sum (the inputs lie in [-80, 0]), one of the division, one
unit for the higher-order terms.  Derived, not measured; the measured deviation is printed beside it.  Measured on one
MI355X: at most 1.14 units of 2^-24 mean|x_b| over cases A - E (bound 23 or 24 units) and 1.21 over the checked utterances
of the B = 65 540 batch (T = 2, bound 20 units)."""
import copy

import numpy as np
import pytest
import torch

import encoder_conv_train_ref as ER
import specaug_ref as R

pytestmark = pytest.mark.gpu


def run_case(gpu, name, out_of_place=True):
    from speech_to_image_translation_without_text_amd import ops
    c = R.CASES[name]
    x = R.case_input(name)
    mel = torch.from_numpy(x).to(gpu).view(c["B"], 1, c["T"], 40)
    if out_of_place:
        y = ops.specaug(mel, c["valid"], c["policy"], c["seed"], c["step"])
        assert y.data_ptr() != mel.data_ptr() and torch.equal(mel.cpu(), torch.from_numpy(x).view_as(mel)), "x is left alone"
    else:
        y = ops.specaug(mel, c["valid"], c["policy"], c["seed"], c["step"], out=mel)
        assert y is mel
    return c, x, y.cpu().numpy().reshape(x.shape)


def check_against_reference(x, y, valid, policy, seed, step, what, utterances=None):
    """Unmasked cells bit-equal, masked cells one value per utterance inside the derived bound -> worst deviation in
    units of 2^-24 mean|x_b|."""
    B, T, _ = x.shape
    worst = 0.0
    for b in (range(B) if utterances is None else utterances):
        n = int(valid[b])
        mask = R.mask_array(policy, seed, step, b, n, T)
        assert np.array_equal(y[b][~mask].view(np.uint32), x[b][~mask].view(np.uint32)), "%s: utterance %d outside its masks" % (what, b)
        if not mask.any():
            continue
        values = np.unique(y[b][mask])
        assert values.size == 1, "%s: utterance %d holds %d masked values" % (what, b, values.size)
        rows = x[b, :n].astype(np.float64)
        mean, mean_abs = rows.mean(), np.abs(rows).mean()
        dev = abs(float(values[0]) - mean)
        bound = R.mean_bound(T, mean_abs)
        print("%s utterance %d: |m - mean| = %.3e = %.2f units, bound %.3e = %d units"
              % (what, b, dev, dev / (2.0 ** -24 * mean_abs), bound, R.depth(T) + 2))
        assert dev <= bound, "%s: utterance %d mean off by %.3e > %.3e" % (what, b, dev, bound)
        worst = max(worst, dev / (2.0 ** -24 * mean_abs))
    return worst


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_kernel_matches_the_reference(gpu, name):
    c, x, y = run_case(gpu, name)
    check_against_reference(x, y, c["valid"], c["policy"], c["seed"], c["step"], "case " + name)
    changed = (y != x).reshape(c["B"], -1).any(axis=1)
    for b, n in enumerate(c["valid"]):
        assert bool(changed[b]) == (n >= 64), "case %s: utterance %d (valid %d)" % (name, b, n)     # non-vacuous, and valid = 0 copies
    if name == "D":     # W = 0: frequency masks alone, so every changed row changes the same bins
        for b, n in enumerate(c["valid"]):
            rows = (y[b] != x[b])
            assert rows[:n].any() and np.array_equal(rows[:n], np.broadcast_to(rows[0], (n, 40))) and not rows[n:].any()


@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_in_place_equals_out_of_place(gpu, name):
    _, _, y = run_case(gpu, name)
    _, _, z = run_case(gpu, name, out_of_place=False)
    assert np.array_equal(y.view(np.uint32), z.view(np.uint32))
    _, _, again = run_case(gpu, name)                        # two calls with equal arguments: equal bits
    assert np.array_equal(y.view(np.uint32), again.view(np.uint32))


def test_no_masks_copies_bit_for_bit(gpu):
    from speech_to_image_translation_without_text_amd import ops
    x = torch.from_numpy(R.case_input("B")).to(gpu).view(5, 1, 128, 40)
    x.view(-1)[:4] = torch.tensor([float("nan"), float("inf"), -0.0, 1e-42], device=gpu)      # bits, not values
    for policy in ((0, 0, 0, 0, 1.0), (0, 8, 0, 20, 0.2), ""):
        y = ops.specaug(x, R.CASES["B"]["valid"], policy, 1, 2)
        assert y.data_ptr() != x.data_ptr() and torch.equal(y.view(torch.int32), x.view(torch.int32))
        keep = x.clone()
        assert ops.specaug(x, R.CASES["B"]["valid"], policy, 1, 2, out=x) is x and torch.equal(x.view(torch.int32), keep.view(torch.int32))
    # zero-width masks mask nothing either
    y = ops.specaug(x, R.CASES["B"]["valid"], (8, 0, 8, 0, 1.0), 1, 2)
    assert torch.equal(y.view(torch.int32), x.view(torch.int32))


def test_masks_depend_on_seed_step_and_b_alone(gpu):
    """Utterance b of case B's batch of five, and the same utterance in row b of a batch whose other rows hold other data
    with other lengths: the same mask set and the same bits."""
    from speech_to_image_translation_without_text_amd import ops
    c, x, y = run_case(gpu, "B")
    other = np.random.RandomState(77).uniform(-80.0, 0.0, size=x.shape).astype(np.float32)
    for b in range(c["B"]):
        x2, valid2 = other.copy(), [128, 128, 0, 64, 128]
        x2[b], valid2[b] = x[b], c["valid"][b]
        y2 = ops.specaug(torch.from_numpy(x2).to(gpu).view(5, 1, 128, 40), valid2, c["policy"], c["seed"], c["step"])
        y2 = y2.cpu().numpy().reshape(x.shape)
        ref = R.mask_array(c["policy"], c["seed"], c["step"], b, c["valid"][b], c["T"])
        assert np.array_equal(y2[b] != x2[b], ref) and np.array_equal(y[b] != x[b], ref), "utterance %d: mask set" % b
        assert np.array_equal(y2[b].view(np.uint32), y[b].view(np.uint32)), "utterance %d: values" % b
        # another step, or another row, draws other masks
        y3 = ops.specaug(torch.from_numpy(x2).to(gpu).view(5, 1, 128, 40), valid2, c["policy"], c["seed"], c["step"] + 1)
        if c["valid"][b]:
            assert not np.array_equal(y3.cpu().numpy().reshape(x.shape)[b] != x2[b], ref)


def test_more_utterances_than_one_grid_dimension_holds(gpu):
    """B = 65 540 > 65 535: the blocks walk the batch in strides; the utterances of the second stride and the first few are
    checked against the reference, every other one for an untouched tail."""
    from speech_to_image_translation_without_text_amd import ops
    B, T, policy, seed, step = 65540, 2, (1, 8, 1, 2, 1.0), 5, 9
    rng = np.random.RandomState(3)
    x = rng.uniform(-80.0, 0.0, size=(B, T, 40)).astype(np.float32)
    valid = rng.randint(0, 3, size=B).astype(np.int32)
    valid[[0, 65535, 65539]] = 2
    y = ops.specaug(torch.from_numpy(x).to(gpu).view(B, 1, T, 40), torch.from_numpy(valid).to(gpu), policy, seed, step)
    y = y.cpu().numpy().reshape(x.shape)
    check_against_reference(x, y, valid, policy, seed, step, "B = 65540", utterances=[0, 1, 2, 3, 65534] + list(range(65535, B)))
    tail = np.arange(T)[None, :] >= valid[:, None]
    assert np.array_equal(y[tail].view(np.uint32), x[tail].view(np.uint32))
    assert (y != x).reshape(B, -1).any(axis=1).sum() > B // 4


def test_element_indices_past_2_to_the_31(gpu):
    """B T 40 > 2^31 elements: the last utterances lie past the 32-bit range.  All but the last two have valid = 0."""
    from speech_to_image_translation_without_text_amd import ops
    B, T, policy, seed, step = 26220, 2048, (2, 8, 2, 40, 0.2), 31, 4
    assert (B - 2) * T * 40 > 2 ** 31
    g = torch.Generator(device=gpu).manual_seed(1)
    x = torch.empty((B, 1, T, 40), dtype=torch.float32, device=gpu).uniform_(-80.0, 0.0, generator=g)
    valid = torch.zeros(B, dtype=torch.int32)
    valid[-2:] = torch.tensor([1984, 2048], dtype=torch.int32)
    y = ops.specaug(x, valid.to(gpu), policy, seed, step)
    assert torch.equal(y[:B - 2], x[:B - 2])
    last_x, last_y = x[B - 2:].cpu().numpy().reshape(2, T, 40), y[B - 2:].cpu().numpy().reshape(2, T, 40)
    del x, y
    for i, b in enumerate((B - 2, B - 1)):
        n = int(valid[b])
        mask = R.mask_array(policy, seed, step, b, n, T)
        assert mask.any() and np.array_equal(last_y[i] != last_x[i], mask)
        mean = last_x[i, :n].astype(np.float64).mean()
        assert np.unique(last_y[i][mask]).size == 1 and abs(float(last_y[i][mask][0]) - mean) <= R.mean_bound(T, abs(mean))


def test_bad_arguments_raise_before_a_launch(gpu):
    from speech_to_image_translation_without_text_amd import _lib, ops
    x = torch.zeros((3, 1, 128, 40), device=gpu)
    policy = R.POLICY_A
    with pytest.raises(_lib.S2IError, match="cpu"):
        ops.specaug(x.cpu(), [128] * 3, policy, 0, 0)                       # a CPU tensor
    with pytest.raises(ValueError, match="40"):
        ops.specaug(torch.zeros((3, 1, 128, 41), device=gpu), [128] * 3, policy, 0, 0)      # the wrong last dimension
    with pytest.raises(ValueError, match="valid"):
        ops.specaug(x, [128] * 4, policy, 0, 0)                             # valid longer than B
    with pytest.raises(ValueError, match="valid"):
        ops.specaug(x, torch.full((4,), 128, dtype=torch.int32, device=gpu), policy, 0, 0)
    with pytest.raises(ValueError, match="valid"):
        ops.specaug(x, [128, 129, 0], policy, 0, 0)                         # past T
    with pytest.raises(ValueError, match="valid"):
        ops.specaug(x, torch.full((3,), 128, dtype=torch.int64, device=gpu), policy, 0, 0)
    with pytest.raises(ValueError, match="fp32"):
        ops.specaug(x.double(), [128] * 3, policy, 0, 0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.specaug(torch.zeros((3, 1, 40, 128), device=gpu).transpose(2, 3), [128] * 3, policy, 0, 0)
    with pytest.raises(ValueError, match="out"):
        ops.specaug(x, [128] * 3, policy, 0, 0, out=torch.zeros((2, 1, 128, 40), device=gpu))
    with pytest.raises(_lib.S2IError, match="mask counts"):
        ops.specaug(x, [128] * 3, (9, 8, 0, 0, 1.0), 0, 0)                  # the library's own refusal
    assert not x.any()


# ---- the trainers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    return ER.stack_net(bidirectional=True, nhidden=512)


@pytest.fixture(scope="module")
def batch(gpu):
    mel, lens, image, label = R.trainer_batch()
    return mel.to(gpu), lens, image, label


def make(net, gpu, kind="encoder", **kw):
    from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer, HeadTrainer
    cls = {"head": HeadTrainer, "encoder": EncoderTrainer}[kind]
    return cls(copy.deepcopy(net).to(gpu), **ER.TRAINER_LOSS, **kw)


def same_parameters(a, b):
    sa, sb = a.model.state_dict(), b.model.state_dict()
    return [k for k in sa if not torch.equal(sa[k], sb[k])]


@pytest.mark.parametrize("kind", ["head", "encoder"])
def test_trainer_with_specaug_equals_stepping_on_ops_specaug_by_hand(gpu, net, batch, kind):
    from speech_to_image_translation_without_text_amd import ops
    t = R.TRAINER
    mel, lens, image, label = batch
    keep = mel.clone()
    auto = make(net, gpu, kind, specaug=t["spec"], specaug_seed=t["seed"])
    hand = make(net, gpu, kind)
    plain = make(net, gpu, kind)
    policy = ops.specaug_policy(t["spec"])
    for step in range(2):
        la = auto.step(mel, lens, image, label)
        masked = ops.specaug(mel, [64 * n for n in lens], policy, t["seed"], hand.steps)
        assert not torch.equal(masked, mel)
        lh = hand.step(masked, lens, image, label)
        lp = plain.step(mel, lens, image, label)
        for k in la:
            assert torch.equal(la[k], lh[k]), "step %d: %s" % (step, k)
        assert not torch.equal(la["loss"], lp["loss"]), "the masks change the loss"
    assert auto.steps == hand.steps == 2 and torch.equal(mel, keep), "the caller's batch is left alone"
    assert same_parameters(auto, hand) == []
    assert same_parameters(auto, plain) != []


@pytest.mark.parametrize("fused", [False, True], ids=["torch_adam", "fused_adam"])
def test_specaug_resumes_bit_for_bit_through_the_public_state(gpu, net, batch, fused):
    t = R.TRAINER
    kw = dict(specaug=t["spec"], specaug_seed=t["seed"], fused_adam=fused)
    a = make(net, gpu, **kw)
    for _ in range(4):
        a.step(*batch)
    b = make(net, gpu, **kw)
    for _ in range(2):
        b.step(*batch)
    state = b.state_dict()
    assert set(state) == {"state_dict", "epoch", "steps", "lr", "optimizer"} and state["steps"] == 2
    c = make(net, gpu, **kw)
    c.load_state_dict(state)
    for _ in range(2):
        c.step(*batch)
    assert c.steps == 4 and same_parameters(a, c) == []
    # the comparison can fail: a counter that restarts at 0 repeats the first masks and ends elsewhere
    d = make(net, gpu, **kw)
    d.load_state_dict(state)
    d.steps = 0
    for _ in range(2):
        d.step(*batch)
    assert same_parameters(a, d) != []


def test_embed_never_sees_a_mask_and_off_is_todays_step(gpu, net, batch):
    t = R.TRAINER
    mel, lens, image, label = batch
    on, off, today = make(net, gpu, specaug=t["spec"], specaug_seed=t["seed"]), make(net, gpu, specaug=""), make(net, gpu)
    assert off.specaug is None and today.specaug is None and on.specaug == (2, 8, 2, 20, 0.2)
    assert torch.equal(on.embed(mel, lens), today.embed(mel, lens))
    lo, lt = off.step(mel, lens, image, label), today.step(mel, lens, image, label)
    assert all(torch.equal(lo[k], lt[k]) for k in lt) and same_parameters(off, today) == []
    on.step(mel, lens, image, label)
    assert same_parameters(on, today) != []
    with pytest.raises(ValueError, match="pitch"):
        make(net, gpu, specaug="pitch=1x2")
