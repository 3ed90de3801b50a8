"""Plain-torch restatement of the speech encoder's trainable head and its loss (tests/test_encoder_train_*.py).

The LSTM with the packed-sequence rule written out step by step (not nn.LSTM, so that mutants can be made from it), the mean
over all L steps, and the three loss terms of the reference's LossFunc (Audio_to_Image/train_audio_encoder.py:308-361,
jel.py:17-43).  Any dtype, any device; gradients come from autograd.  `mutant` names one deliberate mistake:
  "reset"    the state of a finished sequence is reset instead of carried (shows in h_n, c_n only)
  "mean_len" the mean over time divides by len[b] instead of L
  "rev_L"    the reverse direction starts at L-1 instead of len-1
  "diag_row" score_abs subtracts the diagonal entry of the row instead of the column
  "l1_row"   the L1 term normalises each row instead of the whole tensor
"""
import torch
import torch.nn.functional as F


def lstm_head(x, lens, params, mutant=None):
    """x [B, L, E]; lens B ints; params = weight_ih (4H, E), weight_hh (4H, H), bias_ih, bias_hh per direction (the second
    direction runs reversed) -> out [B, L, D*H] (zero at t >= len), sent [B, D*H], h_n and c_n [D, B, H]."""
    B, L, _ = x.shape
    D = len(params) // 4
    lens = [int(v) for v in lens]
    lens_t = torch.tensor(lens, device=x.device)
    bidx = torch.arange(B, device=x.device)
    outs, hn, cn = [], [], []
    for d in range(D):
        w_ih, w_hh, b_ih, b_hh = params[4 * d:4 * d + 4]
        H = w_hh.shape[1]
        h = x.new_zeros((B, H))
        c = x.new_zeros((B, H))
        out = x.new_zeros((B, L, H))
        start = lens_t - 1 if mutant != "rev_L" else torch.full_like(lens_t, L - 1)
        steps = max(lens) if not (d == 1 and mutant == "rev_L") else L
        for step in range(steps):
            t = (start - step) if d == 1 else torch.full_like(lens_t, step)
            live = ((t >= 0) & (step < L)) if (d == 1 and mutant == "rev_L") else (step < lens_t)
            tc = t.clamp(0, L - 1)
            z = x[bidx, tc] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            i, f, g, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
            c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h2 = torch.sigmoid(o) * torch.tanh(c2)
            m = live.unsqueeze(1)
            keep_h, keep_c = (torch.zeros_like(h), torch.zeros_like(c)) if mutant == "reset" else (h, c)
            h = torch.where(m, h2, keep_h)
            c = torch.where(m, c2, keep_c)
            valid = live & (tc < lens_t)                   # outputs exist at valid positions only
            out = out.index_put((bidx[valid], tc[valid]), h2[valid])
        outs.append(out)
        hn.append(h)
        cn.append(c)
    out = torch.cat(outs, 2)
    if mutant == "mean_len":
        sent = out.sum(1) / lens_t.to(out.dtype).unsqueeze(1)
    else:
        sent = out.mean(1)
    return out, sent, torch.stack(hn), torch.stack(cn)


def jel_loss(audio, image, label, c_diff, c_same, mutant=None):
    B = audio.shape[0]
    score = image @ audio.t()
    diag = score.diag()
    score_abs = score - (diag.unsqueeze(1) if mutant == "diag_row" else diag.unsqueeze(0))
    same = label.unsqueeze(0) == label.unsqueeze(1)
    ld = torch.where(~same, score_abs + 1, torch.zeros_like(score_abs))
    ls = torch.where(same, score_abs, torch.zeros_like(score_abs))
    loss = (c_diff * ld[ld > 0].sum() + c_same * ls[ls > 0].sum()) / (B * B)
    hits = (score.argmax(1) == torch.arange(B, device=score.device)).sum()
    return loss, 100.0 * hits.to(audio.dtype) / B, score, score_abs, same


def encoder_loss(audio, image, label, loss_diff=1, loss_same=1, jel=True, l1=False, lambda_l1=1, distill=False, distill_T=2,
                 lambda_distill=1, mutant=None):
    """-> dict(loss, loss_jel, loss_l1, loss_distill, accu); the image side is a constant."""
    image = image.detach()
    zero = audio.new_zeros(())
    vj, accu, v1, vd = zero, zero, zero, zero
    if jel:
        vj, accu = jel_loss(audio, image, label, loss_diff, loss_same, mutant)[:2]
    if l1:
        if mutant == "l1_row":
            v1 = (audio / audio.norm(dim=1, keepdim=True) - image / image.norm(dim=1, keepdim=True)).abs().mean()
        else:
            v1 = (audio / audio.norm() - image / image.norm()).abs().mean()
    if distill:
        q = F.softmax(image / distill_T, 1)
        vd = (q * (torch.log(q) - F.log_softmax(audio, 1))).sum() / audio.numel()
    return {"loss": vj + lambda_l1 * v1 + lambda_distill * vd, "loss_jel": vj, "loss_l1": v1, "loss_distill": vd, "accu": accu}


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def head_case(B, L, E, H, D, lens, seed=0, dtype=torch.float64):
    """x [B, L, E] (padded positions hold data too, as the conv stack produces it), nn.LSTM-style parameters and fixed
    cotangents for out and sent."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = 1.0 / H ** 0.5
    x = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    params = []
    for _ in range(D):
        params += [(torch.rand(4 * H, E, generator=g, dtype=torch.float64) * 2 - 1) * k,
                   (torch.rand(4 * H, H, generator=g, dtype=torch.float64) * 2 - 1) * k,
                   (torch.rand(4 * H, generator=g, dtype=torch.float64) * 2 - 1) * k,
                   (torch.rand(4 * H, generator=g, dtype=torch.float64) * 2 - 1) * k]
    g_out = torch.randn(B, L, D * H, generator=g, dtype=torch.float64)
    g_sent = torch.randn(B, D * H, generator=g, dtype=torch.float64)
    cast = lambda t: t.to(dtype)
    return cast(x), [cast(p) for p in params], cast(g_out), cast(g_sent)


def head_run(x, lens, params, g_out, g_sent, pattern, mutant=None):
    """Forward and gradients for one cotangent pattern ("sent", "out" or "both") -> dict of detached tensors."""
    x = x.detach().clone().requires_grad_(True)
    params = [p.detach().clone().requires_grad_(True) for p in params]
    out, sent, hn, cn = lstm_head(x, lens, params, mutant)
    obj = 0
    if pattern in ("out", "both"):
        obj = obj + (out * g_out).sum()
    if pattern in ("sent", "both"):
        obj = obj + (sent * g_sent).sum()
    grads = torch.autograd.grad(obj, [x] + params)
    return dict(out=out.detach(), sent=sent.detach(), hn=hn.detach(), cn=cn.detach(), dx=grads[0], dparams=list(grads[1:]))


def loss_case(B, C, seed=0, dtype=torch.float64, margin=1e-6):
    """audio, image [B, C] and labels that repeat, drawn until no score_abs or score_abs + 1 lies within `margin` of zero
    (off the diagonal, where score_abs is exactly zero) and no row of score has a tied maximum."""
    for attempt in range(100):
        g = torch.Generator().manual_seed(7000 + 100 * seed + attempt)
        audio = torch.randn(B, C, generator=g, dtype=torch.float64) * (1.5 / C ** 0.5)
        image = torch.randn(B, C, generator=g, dtype=torch.float64) * (1.5 / C ** 0.5) + 0.5 * audio
        label = torch.randint(0, max(2, B // 3), (B,), generator=g)
        if loss_case_ok(audio, image, label, margin):
            return audio.to(dtype), image.to(dtype), label
    raise RuntimeError("no admissible loss inputs for B=%d C=%d" % (B, C))


def loss_case_ok(audio, image, label, margin=1e-6):
    _, _, score, score_abs, same = jel_loss(audio.double(), image.double(), label, 1, 1)
    off = ~torch.eye(len(label), dtype=torch.bool)
    hinge = torch.where(same, score_abs, score_abs + 1)
    top2 = score.topk(2, dim=1)[0]
    repeats = bool((same & off).any())
    return bool((hinge[off].abs() > margin).all()) and bool(((top2[:, 0] - top2[:, 1]) > margin).all()) and repeats


def loss_run(audio, image, label, mutant=None, **flags):
    audio = audio.detach().clone().requires_grad_(True)
    res = encoder_loss(audio, image, label, mutant=mutant, **flags)
    grad = torch.zeros_like(audio)
    if res["loss"].requires_grad:
        grad = torch.autograd.grad(res["loss"], [audio])[0]
    return {k: v.detach() for k, v in res.items()}, grad


def rel_err(got, ref):
    """max|got - ref| / max|ref| (the tolerance metric of the encoder-training tests)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    den = float(ref.abs().max())
    return float((got - ref).abs().max()) / (den if den > 0 else 1.0)


# ---- the cases of the GPU tests and the fp32 yardstick of their tolerances ---------------------------------------------------
def case_lens(B, L, seed=0):
    """B lengths sorted descending that include L (twice: two equal values) and 1."""
    if B == 3:
        return [L, L, 1]
    g = torch.Generator().manual_seed(50 + seed)
    mid = torch.randint(1, L + 1, (B - 3,), generator=g).tolist()
    return sorted([L, L, 1] + mid, reverse=True)


HEAD_CASES = [(3, 8, 32, 8, 2), (3, 8, 32, 64, 1), (33, 8, 32, 64, 2), (4, 8, 64, 1024, 1)]
PRODUCTION = (64, 32, 1024, 512, 2)
PATTERNS = ("sent", "out", "both")
LOSS_SHAPES = [(5, 32), (64, 1024), (37, 1024)]
LOSS_FLAGS = {
    "jel": dict(jel=True),
    "l1": dict(jel=False, l1=True),
    "distill": dict(jel=False, distill=True),
    "all": dict(jel=True, l1=True, distill=True),
    "weights": dict(jel=True, l1=True, distill=True, loss_diff=0.7, loss_same=1.6, lambda_l1=2.5, lambda_distill=0.4,
                    distill_T=3.0),
}


def production_lens():
    g = torch.Generator().manual_seed(77)
    return sorted(torch.randint(10, 33, (PRODUCTION[0],), generator=g).tolist(), reverse=True)


def train_case(B=8, L=8, E=1024, H=32, D=2, seed=4):
    """Three batches of synthetic conv features, image features, labels and lengths for the HeadTrainer tests."""
    g = torch.Generator().manual_seed(300 + seed)
    batches = []
    for _ in range(3):
        feat = torch.randn(B, L, E, generator=g, dtype=torch.float64).abs() * 0.5       # conv features are post-ReLU
        image = torch.randn(B, D * H, generator=g, dtype=torch.float64)
        label = torch.randint(0, 3, (B,), generator=g)
        lens = sorted(torch.randint(1, L + 1, (B,), generator=g).tolist(), reverse=True)
        batches.append((feat, lens, image, label))
    return batches


def train_steps(params, batches, dtype, lr=1e-3, weight_decay=1e-5, **loss_args):
    """Three optimiser steps of the restated head with torch.optim.Adam on the CPU -> (losses, updated parameters)."""
    params = [p.detach().clone().to(dtype).requires_grad_(True) for p in params]
    opt = torch.optim.Adam(params, lr=lr, weight_decay=weight_decay)
    losses = []
    for feat, lens, image, label in batches:
        _, sent, _, _ = lstm_head(feat.to(dtype), lens, params)
        res = encoder_loss(sent, image.to(dtype), label, **loss_args)
        opt.zero_grad()
        res["loss"].backward()
        opt.step()
        losses.append(res["loss"].detach())
    return torch.stack(losses), [p.detach() for p in params]


# ---- edge cases of the fused step kernels, the two-kernel path and the loss (tests/test_encoder_head_edges_*.py) -----------------
def fused_path(B, Hd):
    """The rule ops.LstmSentence takes the one-launch step kernels by."""
    return B <= 32 and Hd % 8 == 0 and Hd <= 512


def edge_lens(pattern, B, L, seed=0):
    """B lengths in [1, L]: "std" = case_lens (sorted descending, L twice); "full" = all L; "ones" = all 1; "unsorted" =
    seeded draws with slot 0 set to 1 and the last slot set to L; "short" = seeded, unsorted, nothing above L - 2, the
    longest not in slot 0."""
    if pattern == "std":
        return case_lens(B, L, seed)
    if pattern == "full":
        return [L] * B
    if pattern == "ones":
        return [1] * B
    g = torch.Generator().manual_seed(90 + seed)
    if pattern == "unsorted":
        lens = torch.randint(1, L + 1, (B,), generator=g).tolist()
        lens[0], lens[-1] = 1, L
        return lens
    if pattern == "short":
        if L < 4 or B < 3:
            raise ValueError("short lens need L >= 4 and B >= 3")
        lens = torch.randint(1, L - 1, (B,), generator=g).tolist()
        lens[0], lens[B // 2], lens[-1] = max(1, (L - 2) // 2), L - 2, 1
        return lens
    raise ValueError("unknown lens pattern %r" % (pattern,))


# ((B, L, E, Hd, D), lens pattern, the path ops.LstmSentence takes at its defaults)
EDGE_HEAD_CASES = [
    ((32, 6, 32, 512, 2), "std", "fused"),          # production Hd, all 32 slots, both kernels above 64 KB of LDS
    ((31, 6, 32, 512, 1), "unsorted", "fused"),     # one empty slot, one direction, the longest sequence last
    ((32, 6, 32, 512, 2), "full", "fused"),         # no padded column anywhere
    ((5, 6, 32, 408, 1), "std", "fused"),           # backward LDS 65 920 bytes: just over 64 KB
    ((5, 6, 32, 400, 2), "std", "fused"),           # 64 640 bytes: just under
    ((17, 5, 32, 256, 2), "unsorted", "fused"),     # forward LDS 66 560 bytes: just over, odd B
    ((6, 8, 32, 64, 2), "short", "fused"),          # max(lens) < L
    ((1, 4, 32, 8, 1), "full", "fused"),            # B = 1, one block per direction
    ((32, 1, 32, 8, 2), "ones", "fused"),           # L = 1: the first backward launch is the only one
    ((9, 7, 32, 8, 2), "ones", "fused"),            # one step, six padded columns per sequence
    ((4, 6, 32, 12, 2), "std", "two-kernel"),       # Hd % 8 != 0; the bias gradient sees N = 96
    ((3, 6, 32, 520, 1), "std", "two-kernel"),      # the first Hd the fused limit refuses
    ((33, 8, 32, 16, 2), "short", "two-kernel"),    # B = 33 with max(lens) < L
    ((33, 6, 32, 512, 2), "unsorted", "two-kernel"),  # production Hd through the other path
]
EDGE_MUTANT_CASES = [EDGE_HEAD_CASES[6], EDGE_HEAD_CASES[12]]


def edge_case_id(entry):
    return "B%d_L%d_E%d_H%d_D%d" % entry[0] + "_" + entry[1]


def fwd_step_lds_bytes(Hd):
    """Dynamic LDS of the fused forward step: h [32][Hd + 4] and the W_hh slice [32][Hd + 4], fp32."""
    return 2 * 32 * (Hd + 4) * 4


def bwd_step_lds_bytes(Hd):
    """Dynamic LDS of the fused backward step: a dG chunk [32][Hd + 4] and the transposed W_hh slice [8][Hd + 4], fp32."""
    return 40 * (Hd + 4) * 4


EDGE_LOSS_SHAPES = [(257, 40), (300, 4), (37, 1000), (5, 63), (2, 8)]
HOT_LOSS_FLAGS = {
    "T2": dict(jel=False, distill=True, distill_T=2),
    "T3": dict(jel=False, distill=True, distill_T=3, lambda_distill=0.4),
}


def label_case(kind):
    """loss_case(12, 96) with its labels replaced: "one_class" = all zero (every pair is a same-class pair), "distinct" =
    arange(12) (none is)."""
    audio, image, _ = loss_case(12, 96)
    label = torch.zeros(12, dtype=torch.long) if kind == "one_class" else torch.arange(12)
    return audio, image, label


def hinge_margin(audio, image, label):
    """(smallest |hinge argument| off the diagonal, smallest gap between a score row's two largest entries)."""
    _, _, score, score_abs, same = jel_loss(audio.double(), image.double(), label, 1, 1)
    off = ~torch.eye(len(label), dtype=torch.bool)
    hinge = torch.where(same, score_abs, score_abs + 1)
    top2 = score.topk(2, dim=1)[0]
    return float(hinge[off].abs().min()), float((top2[:, 0] - top2[:, 1]).min())


def single_row_case(C=40, seed=0):
    """B = 1: one embedding pair, one label."""
    g = torch.Generator().manual_seed(7900 + seed)
    audio = torch.randn(1, C, generator=g, dtype=torch.float64) * (1.5 / C ** 0.5)
    image = torch.randn(1, C, generator=g, dtype=torch.float64) * (1.5 / C ** 0.5) + 0.5 * audio
    return audio, image, torch.zeros(1, dtype=torch.long)


def hot_loss_case(B=37, C=1000, seed=0):
    """Logits near 100 (audio) and 200 (image): exp of either overflows fp32 unless the row maximum is subtracted first.
    Both are rounded to fp32, so that the fp64 reference and an fp32 kernel start from the same numbers."""
    g = torch.Generator().manual_seed(7950 + seed)
    audio = (100 + 3 * torch.randn(B, C, generator=g, dtype=torch.float64)).float().double()
    image = (200 + 6 * torch.randn(B, C, generator=g, dtype=torch.float64)).float().double()
    label = torch.randint(0, B // 3, (B,), generator=g)
    return audio, image, label


def hits(accu, B):
    """The hit count behind an accuracy in percent (100 * hits / B rounds differently in fp32 and fp64)."""
    return int(round(float(accu) * B / 100))
