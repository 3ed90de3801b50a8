"""Plain fp64 restatement of the non-matrix launches of the train step (tests/test_step_elementwise_gpu.py).

One function per entry point of include/s2i_hip.h that tests/step_elementwise_launches.json records.  The functions take
float64 tensors in the kernels' layouts and use only stock torch tensor ops:

  rows       y [M][C] NHWC rows; the M rows are G consecutive BatchNorm groups of M / G rows each
  part       [2][nparts][C] partial column sums; group g owns parts [g * ppg, (g + 1) * ppg), ppg = nparts / G, and part p
             of a group covers its rows [p * chunk, (p + 1) * chunk), chunk = ceil(rows per group / ppg)
  coef       [G][4][C] = mean | invstd | scale | shift of each group (s2i_bn_finalize)
  red2       [G][2][C] = mean dz | mean dz * xhat of each group (s2i_bn_bwd_finalize)
  tapsum     [B][9][C], tap t = 3 * ky + kx of a 3 x 3, pad 1 convolution
  table      [B][9][N], border class 3 * (top | middle | bottom) + (left | middle | right)

tests/test_elementwise_ref.py checks these against stock torch modules and autograd."""
import torch
import torch.nn.functional as F

from speech_to_image_translation_without_text_amd._lib import ACT_GLU, ACT_LRELU, ACT_NONE, ACT_TANH

SLOPE = 0.2
LOG_CLAMP = -100.0
BCE_EPS = 1e-12


# ---- BatchNorm -------------------------------------------------------------------------------------------------------
def group_part_sums(part, G):
    """[2][nparts][C] -> [2][G][C]."""
    two, nparts, C = part.shape
    return part.reshape(two, G, nparts // G, C).sum(2)


def bn_finalize(part, G, count, gamma, beta, rm=None, rv=None, nbt=None, momentum=0.1, eps=1e-5, biased_running=False):
    """-> (coef [G][4][C], running_mean, running_var, num_batches_tracked): nn.BatchNorm in training mode applied to G
    stacked batches one after another.  biased_running: the wrong restatement that feeds the biased var to running_var."""
    s = group_part_sums(part, G)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    coef = torch.stack((mean, invstd, scale, shift), 1)
    if rm is not None:
        rm, rv = rm.clone(), rv.clone()
        unb = var if (biased_running or count <= 1) else var * count / (count - 1)
        for g in range(G):
            rm = (1 - momentum) * rm + momentum * mean[g]
            rv = (1 - momentum) * rv + momentum * unb[g]
    if nbt is not None:
        nbt = nbt + G
    return coef, rm, rv, nbt


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=1e-5):
    """-> coef [1][4][C] of nn.BatchNorm in eval mode: mean = running_mean, invstd = 1 / sqrt(running_var + eps),
    scale = gamma * invstd, shift = beta - mean * scale (one group: every row of the launch)."""
    invstd = 1.0 / torch.sqrt(running_var + eps)
    scale = gamma * invstd
    return torch.stack((running_mean, invstd, scale, beta - running_mean * scale)).unsqueeze(0)


def bn_bwd_finalize(part, G, count, dgamma=None, dbeta=None, accumulate=False):
    """-> (red2 [G][2][C], dgamma, dbeta): means per group and totals over the groups, added to the given values when
    accumulating."""
    s = group_part_sums(part, G)
    red2 = (s / count).permute(1, 0, 2).contiguous()
    tot = s.sum(1)
    dg = tot[1] + (dgamma if (accumulate and dgamma is not None) else 0)
    db = tot[0] + (dbeta if (accumulate and dbeta is not None) else 0)
    return red2, dg, db


def _rows(t, G):
    return t.reshape(G, t.shape[0] // G, t.shape[-1])


def pre_act(y, coef, G):
    """z = scale * y + shift per group: [G][Rg][C]."""
    return _rows(y, G) * coef[:, 2:3, :] + coef[:, 3:4, :]


def act_forward(z, act):
    if act == ACT_GLU:
        h = z.shape[-1] // 2
        return z[..., :h] * torch.sigmoid(z[..., h:])
    if act == ACT_LRELU:
        return torch.where(z > 0, z, SLOPE * z)
    if act == ACT_NONE:
        return z
    raise ValueError("activation %d" % act)


def bn_act_forward(y, G, coef, act, residual=None):
    """out = act(scale * y + shift) (+ residual): [M][C or C/2]."""
    o = act_forward(pre_act(y, coef, G), act).reshape(y.shape[0], -1)
    return o if residual is None else o + residual


def act_dz(z, d, act):
    """Gradient w.r.t. z = scale * y + shift given d = gradient w.r.t. act(z) (first Cout columns of dout)."""
    if act == ACT_GLU:
        h = z.shape[-1] // 2
        a, s = z[..., :h], torch.sigmoid(z[..., h:])
        return torch.cat((d * s, d * a * s * (1 - s)), -1)
    if act == ACT_LRELU:
        return torch.where(z > 0, d, SLOPE * d)
    if act == ACT_NONE:
        return d
    raise ValueError("activation %d" % act)


def xhat(y, coef, G):
    return (_rows(y, G) - coef[:, 0:1, :]) * coef[:, 1:2, :]


def dz_of(y, dout, G, coef, act):
    """[G][Rg][C] gradient w.r.t. z from dout [M][>= Cout] (a channel slice of a wider row when ldd > Cout)."""
    C = y.shape[-1]
    cout = C // 2 if act == ACT_GLU else C
    return act_dz(pre_act(y, coef, G), _rows(dout[:, :cout], G), act)


def chunk_sums(v, nparts_per_group):
    """v [G][Rg][C] -> [G * ppg][C]: sums over each group's row chunks (colreduce_kernel's split)."""
    G, Rg, C = v.shape
    ppg = nparts_per_group
    chunk = -(-Rg // ppg)
    if ppg * chunk > Rg:      # the last chunks are short or empty
        v = torch.cat((v, v.new_zeros((G, ppg * chunk - Rg, C))), 1)
    return v.reshape(G, ppg, chunk, C).sum(2).reshape(G * ppg, C)


def bn_act_bwd_reduce(y, dout, G, coef, act, nparts):
    """part [2][nparts][C] of (dz, dz * xhat)."""
    dz = dz_of(y, dout, G, coef, act)
    return torch.stack((chunk_sums(dz, nparts // G), chunk_sums(dz * xhat(y, coef, G), nparts // G)))


def bn_act_bwd_apply(y, dout, G, coef, red2, act):
    """dy = scale * (dz - mean dz - xhat * mean dz xhat): [M][C]."""
    dz = dz_of(y, dout, G, coef, act)
    dy = coef[:, 2:3, :] * (dz - red2[:, 0:1, :] - xhat(y, coef, G) * red2[:, 1:2, :])
    return dy.reshape(y.shape)


def act_backward(out, dout, act):
    """dy = dout * act'(.) from the forward OUTPUT of LeakyReLU or tanh."""
    if act == ACT_LRELU:
        return torch.where(out > 0, dout, SLOPE * dout)
    if act == ACT_TANH:
        return dout * (1 - out * out)
    raise ValueError("activation %d" % act)


# ---- sums over rows, taps and broadcast channels -----------------------------------------------------------------------
def colstats(y, nparts):
    """y [M][C] -> part [2][nparts][C] of (y, y^2) over nparts row chunks."""
    v = y.unsqueeze(0)
    return torch.stack((chunk_sums(v, nparts), chunk_sums(v * v, nparts)))


def spatial_sum(src, B, C):
    """src [B * HW][ld] -> [B][C]: per-image sums of the first C columns."""
    return src[:, :C].reshape(B, -1, C).sum(1)


def _tap_rows(n, k):
    """Output rows (or columns) on which tap k of a 3-wide, pad 1 window reads in bounds."""
    return slice(1 if k == 0 else 0, n - 1 if k == 2 else n)


def tap_sums(dy, swap_top_bottom=False):
    """dy [B][H][W][C] -> tapsum [B][9][C]: sum of dy over the pixels where tap (ky, kx) reads in bounds."""
    B, H, W, C = dy.shape
    out = []
    for ky in range(3):
        kr = 2 - ky if (swap_top_bottom and ky != 1) else ky
        for kx in range(3):
            out.append(dy[:, _tap_rows(H, kr), _tap_rows(W, kx)].sum((1, 2)))
    return torch.stack(out, 1)


def packed_to_oihw(packed, Cc, N):
    """P[9][Ip][Op] rows [0, Cc), columns [0, N) -> W [N][Cc][3][3]."""
    return packed[:, :Cc, :N].permute(2, 1, 0).reshape(N, Cc, 3, 3)


def cvec_bias_table(cvec, packed, Cc, N, swap_top_bottom=False):
    """table [B][9][N]: the 3 x 3, pad 1 convolution of a spatially constant map c over a 3 x 3 grid, whose pixel (i, j)
    is the representative of border class 3 i + j."""
    B = cvec.shape[0]
    w = packed_to_oihw(packed, Cc, N)
    t = F.conv2d(cvec.view(B, Cc, 1, 1).expand(B, Cc, 3, 3), w, padding=1)
    if swap_top_bottom:
        t = t.flip(2)
    return t.reshape(B, N, 9).permute(0, 2, 1)


def cvec_dc(packed, tapsum, Cc, N):
    """dc [B][Cc] = sum_{t, n} P[t][cc][n] tapsum[b][t][n]."""
    return torch.einsum("tcn,btn->bc", packed[:, :Cc, :N], tapsum[:, :, :N])


def cvec_dw(cvec, tapsum, O):
    """dW[:, :Cc] [O][Cc][3][3] = sum_b c[b][cc] tapsum[b][t][o]."""
    B, Cc = cvec.shape
    return torch.einsum("bc,bto->oct", cvec, tapsum[:, :, :O]).reshape(O, Cc, 3, 3)


# ---- CA_NET, heads and losses ------------------------------------------------------------------------------------------
def glu(x):
    h = x.shape[1] // 2
    return x[:, :h] * torch.sigmoid(x[:, h:])


def glu_backward(x, dout):
    h = x.shape[1] // 2
    a, s = x[:, :h], torch.sigmoid(x[:, h:])
    return torch.cat((dout * s, dout * a * s * (1 - s)), 1)


def reparam_forward(h, eps):
    E = eps.shape[1]
    return eps * torch.exp(0.5 * h[:, E:]) + h[:, :E]


def reparam_backward(h, eps, dc):
    E = eps.shape[1]
    return torch.cat((dc, dc * eps * 0.5 * torch.exp(0.5 * h[:, E:])), 1)


def kl_forward(mu, lv):
    return -0.5 * torch.mean(1 + lv - mu * mu - torch.exp(lv))


def kl_backward(mu, lv, gout):
    g = gout * -0.5 / mu.numel()
    return g * (-2 * mu), g * (1 - torch.exp(lv))


def logit_forward(x, w, bias):
    """x [B][4][4][C] NHWC, w [1][C][4][4] -> sigmoid(<x_b, w> + bias) [B]."""
    z = torch.einsum("bhwc,chw->b", x, w[0])
    return torch.sigmoid(z + (0 if bias is None else bias[0]))


def logit_backward(x, w, prob, dprob):
    """-> (dlogit [B], dx [B][4][4][C], dw [1][C][4][4], dbias [1])."""
    dl = dprob * prob * (1 - prob)
    dx = dl.view(-1, 1, 1, 1) * w[0].permute(1, 2, 0).unsqueeze(0)
    dw = torch.einsum("b,bhwc->chw", dl, x).unsqueeze(0)
    return dl, dx, dw, dl.sum().view(1)


def bce_terms(p, t):
    """Elementwise nn.BCELoss terms with torch's log clamp at -100."""
    lp = torch.log(p).clamp_min(LOG_CLAMP)
    lq = torch.log(1 - p).clamp_min(LOG_CLAMP)
    return -(t * lp + (1 - t) * lq)


def bce_grad(p, t):
    """d BCE / d p of one term, as torch computes it: (p - t) / max((1 - p) p, 1e-12)."""
    return (p - t) / ((1 - p) * p).clamp_min(BCE_EPS)


def bce_forward(prob, target, weight):
    return weight * bce_terms(prob, target).mean()


def bce_backward(prob, target, weight, gout):
    return weight * gout * bce_grad(prob, target) / prob.numel()


def bce_multi_forward(probs, target, weight, G, B):
    """probs: H tensors of G * B rows; term (g, h) has target[g * H + h], weight[g * H + h]."""
    H = len(probs)
    loss = 0
    for g in range(G):
        for h in range(H):
            loss = loss + weight[g * H + h] * bce_terms(probs[h][g * B:(g + 1) * B], target[g * H + h]).mean()
    return loss


def bce_multi_backward(probs, target, weight, G, B, gout):
    H = len(probs)
    out = []
    for h in range(H):
        parts = [weight[g * H + h] * gout * bce_grad(probs[h][g * B:(g + 1) * B], target[g * H + h]) / B
                 for g in range(G)]
        out.append(torch.cat(parts))
    return out


def cal_loss(S, labels, D, count_diagonal=False):
    """-> (loss, dS): max(0, mean(S) - mean(S over same-class off-diagonal pairs)) / D and its gradient, symmetrised
    (d loss / d S + its transpose, so that dX = dS X)."""
    B = S.shape[0]
    same = labels.view(-1, 1) == labels.view(1, -1)
    if not count_diagonal:
        same = same & ~torch.eye(B, dtype=torch.bool, device=S.device)
    n = int(same.sum())
    if n == 0:
        return S.new_zeros(()), torch.zeros_like(S)
    diff = S.mean() - S[same].sum() / n
    if diff <= 0:
        return S.new_zeros(()), torch.zeros_like(S)
    dS = 2 * (1.0 / (B * B) - same.to(S.dtype) / n) / D
    return diff / D, dS


# ---- optimiser and elementwise helpers ---------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, gscale=1.0):
    """torch.optim.Adam (no weight decay, no amsgrad) at 1-based step `step` on the gradient g * gscale."""
    gg = g * gscale
    m = beta1 * m + (1 - beta1) * gg
    v = beta2 * v + (1 - beta2) * gg * gg
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    p = p - (lr / bc1) * m / (torch.sqrt(v) / bc2 ** 0.5 + eps)
    return p, m, v


def ema_update(avg, p, decay):
    return decay * avg + (1 - decay) * p


def axpby(y, x, a, b):
    return a * x + (b * y if b != 0 else 0)


def scale_dev(x, a):
    return x * a


# ---- layouts and casts -------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, Cp):
    """(B, C, H, W) -> (B, H, W, Cp) with zero pad channels."""
    y = x.permute(0, 2, 3, 1)
    return torch.cat((y, y.new_zeros(y.shape[:3] + (Cp - x.shape[1],))), 3)


def nhwc_to_nchw(src, B, C, H, W):
    """src [B * H * W][lds] -> (B, C, H, W)."""
    return src[:, :C].reshape(B, H, W, C).permute(0, 3, 1, 2)


def cast(x, dtype):
    return x.to(dtype)


# entry points of the census and the restatement each one has here
RESTATES = {
    "s2i_bn_finalize": bn_finalize,
    "s2i_bn_bwd_finalize": bn_bwd_finalize,
    "s2i_bn_act_forward_dt": bn_act_forward,
    "s2i_bn_act_bwd_reduce_dt": bn_act_bwd_reduce,
    "s2i_bn_act_bwd_apply_dt": bn_act_bwd_apply,
    "s2i_act_backward_dt": act_backward,
    "s2i_colstats": colstats,
    "s2i_axpby": axpby,
    "s2i_spatial_sum_dt": spatial_sum,
    "s2i_tap_sums_dt": tap_sums,
    "s2i_cvec_bias_table": cvec_bias_table,
    "s2i_cvec_grads": cvec_dw,
    "s2i_glu_forward": glu,
    "s2i_glu_backward": glu_backward,
    "s2i_reparam_forward": reparam_forward,
    "s2i_reparam_backward": reparam_backward,
    "s2i_kl_forward": kl_forward,
    "s2i_kl_backward": kl_backward,
    "s2i_logit_forward": logit_forward,
    "s2i_logit_backward": logit_backward,
    "s2i_bce_forward": bce_forward,
    "s2i_bce_backward": bce_backward,
    "s2i_bce_multi_forward": bce_multi_forward,
    "s2i_bce_multi_backward": bce_multi_backward,
    "s2i_cal_loss": cal_loss,
    "s2i_scale_dev": scale_dev,
    "s2i_adam_step": adam_step,
    "s2i_ema_update": ema_update,
    "s2i_increment": lambda c: c + 1,
    "s2i_nchw_to_nhwc_dt": nchw_to_nhwc,
    "s2i_nhwc_to_nchw_dt": nhwc_to_nchw,
    "s2i_cast": cast,
}
