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
