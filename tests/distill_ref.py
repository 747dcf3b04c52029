"""The distillation loss of csrc/distill_rules.inc.h, restated twice in float64 and once more in float32.

Per row with target t != pad: student logits x, teacher rows z_m, weights w_m, rule, temperature tau, hard weight alpha,
label smoothing eps --

    hard = (1 - eps) (lse(x) - x[t]) + eps (lse(x) - mean_v x[v])
    y    = ensemble_ref.combine_np(z, w, rule)          (M == 1: y = z_0)
    q    = softmax(y / tau),  p = softmax(x / tau)
    soft = tau^2 sum_v q[v] (log q[v] - log p[v])       (0 where q[v] == 0)
    loss = alpha hard + (1 - alpha) soft
    dlogits[v] = alpha (softmax(x)[v] - (1 - eps) [v == t] - eps / V) + (1 - alpha) tau (p[v] - q[v])

a pad row is exactly zero everywhere and its teacher values are never looked at.

``distill_np`` is the closed form on numpy float64 arrays.  ``distill_torch`` is the autograd form --
F.cross_entropy(label_smoothing) + tau^2 F.kl_div(log_softmax(x / tau), softmax(y / tau)) and ``backward`` -- in float64
(y from combine_np) or in float32 (y by the same formulas on float32 tensors: the "same formulas in float32 on the CPU"
of the tolerance rule).  The two float64 forms agree to 1e-12 (test_distill_host.py), which pins the closed-form gradient.

``floors`` gives the rounding floors of the tolerance rule err <= 4 err_fp32cpu + floor, derived the way
test_small_entries_vs_float64.py section 2 derives CE's (2^-22 on a gradient in [-1, 1], 2^-21 x the magnitudes of the
terms that enter a sum):

  dlogits   2^-22 (alpha + (1 - alpha) tau): the hard term alpha (softmax - onehot - eps / V) lies in [-alpha, alpha], the
            soft term (1 - alpha) tau (p - q) in [-(1 - alpha) tau, (1 - alpha) tau]; CE's floor scaled by the two ranges.
  hard      per kept row 2^-21 (|lse(x)| + |mean_v x[v]| + |x[t]|): CE's floor, the same three terms.
  soft      per kept row 2^-21 tau^2 sum_v q[v] (|y[v]| / tau + |lse(y / tau)| + |x[v]| / tau + |lse(x / tau)|): the row's
            soft loss is tau^2 sum_v q[v] ((y[v] / tau - lse(y / tau)) - (x[v] / tau - lse(x / tau))), so these four are
            the terms that enter it, each weighted by q[v] as the sum weights it -- CE's |x[t]| and |lse| with the one-hot
            weight replaced by q.
  loss sum  alpha x (hard floor) + (1 - alpha) x (soft floor), summed over the kept rows.
"""
import numpy as np
import torch
import torch.nn.functional as F

from ensemble_ref import combine_np, normalised


def f32(v):
    """The value a C float argument carries, as a Python double."""
    return float(np.float32(v))


def _lse(a):
    top = a.max(axis=-1, keepdims=True)
    return top + np.log(np.exp(a - top).sum(axis=-1, keepdims=True))


def teacher_rows_np(z, weights, rule, keep=None):
    """z (M, rows, V), finite at the kept rows -> y (rows, V) float64; pad rows are 0 and their z is not read."""
    z = np.asarray(z, dtype=np.float64)
    M, rows, V = z.shape
    keep = np.ones(rows, dtype=bool) if keep is None else np.asarray(keep)
    y = np.zeros((rows, V))
    for r in np.nonzero(keep)[0]:
        y[r] = z[0, r] if M == 1 else combine_np(z[:, r], weights, rule)
    return y


def distill_np(x, z, weights, rule, tgt, pad, tau, alpha, eps):
    """-> dict(hard (rows), soft (rows), loss (rows), d (rows, V), keep (rows) bool, y (rows, V)), float64."""
    x = np.asarray(x, dtype=np.float64)
    tgt = np.asarray(tgt)
    rows, V = x.shape
    tau, alpha, eps = f32(tau), f32(alpha), f32(eps)
    keep = tgt != pad
    tg = np.clip(tgt, 0, V - 1)
    y = teacher_rows_np(z, weights, rule, keep)
    lse = _lse(x)
    x_t = x[np.arange(rows), tg]
    hard = (1 - eps) * (lse[:, 0] - x_t) + eps * (lse[:, 0] - x.mean(axis=1))
    lq = y / tau - _lse(y / tau)
    lp = x / tau - _lse(x / tau)
    q, p = np.exp(lq), np.exp(lp)
    soft = tau * tau * np.where(q > 0, q * (lq - lp), 0.0).sum(axis=1)
    onehot = np.zeros((rows, V))
    onehot[np.arange(rows), tg] = 1.0
    d = alpha * (np.exp(x - lse) - (1 - eps) * onehot - eps / V) + (1 - alpha) * tau * (p - q)
    hard, soft = np.where(keep, hard, 0.0), np.where(keep, soft, 0.0)
    d = np.where(keep[:, None], d, 0.0)
    return dict(hard=hard, soft=soft, loss=alpha * hard + (1 - alpha) * soft, d=d, keep=keep, y=y)


def _teacher_rows_f32(z, weights, rule):
    """combine_np's formulas on float32 tensors; z (M, rows, V) finite."""
    M = z.shape[0]
    if M == 1:
        return z[0]
    w = torch.from_numpy(normalised(weights, M)).to(torch.float32)
    lp = torch.log_softmax(z, dim=-1)
    if rule == "logprob":
        return (w[:, None, None] * lp).sum(dim=0)
    return torch.logsumexp(torch.log(w)[:, None, None] + lp, dim=0)


def loss_terms_torch(xg, y_kept, tgt, pad, tau, eps):
    """The autograd form on tensors: xg (rows, V) (differentiable), y_kept the teacher's rows AT THE KEPT ROWS, tgt (rows)
    int64 -> per-row hard (rows) and soft (rows, 0 at pad rows)."""
    keep = tgt != pad
    hard = F.cross_entropy(xg, tgt, ignore_index=pad, reduction="none", label_smoothing=eps)
    soft = torch.zeros(xg.shape[0], dtype=xg.dtype)
    if keep.any():
        kl = F.kl_div(torch.log_softmax(xg[keep] / tau, dim=-1), torch.softmax(y_kept / tau, dim=-1), reduction="none")
        soft = soft.index_put((torch.nonzero(keep)[:, 0],), (tau * tau) * kl.sum(dim=-1))
    return hard, soft


def distill_torch(x, z, weights, rule, tgt, pad, tau, alpha, eps, dtype=torch.float64):
    """The autograd form in ``dtype``.  -> dict(hard (rows), soft (rows), d (rows, V)) as float64 numpy arrays holding
    the ``dtype`` values; the gradient is that of sum_rows (alpha hard + (1 - alpha) soft)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    z = np.asarray(z)
    tgt_np = np.asarray(tgt)
    tau, alpha, eps = f32(tau), f32(alpha), f32(eps)
    keep_np = tgt_np != pad
    xg = x.clone().requires_grad_(True)
    if dtype == torch.float64:
        y = torch.from_numpy(teacher_rows_np(z, weights, rule, keep_np))[torch.from_numpy(keep_np)]
    else:
        y = _teacher_rows_f32(torch.as_tensor(z[:, keep_np]).to(dtype), weights, rule)
    hard, soft = loss_terms_torch(xg, y, torch.as_tensor(tgt_np).long(), pad, tau, eps)
    (alpha * hard.sum() + (1 - alpha) * soft.sum()).backward()
    return dict(hard=hard.detach().double().numpy(), soft=soft.detach().double().numpy(),
                d=xg.grad.double().numpy())


def simulate_training(student_sd, student_cfg, teacher_logits, images, formulas, pad, tau, alpha, eps, steps, lr,
                      weight_decay=1e-4, clip=5.0):
    """TrainStep.step with a one-member teacher, ``steps`` times on one batch, in float64 on the CPU with the oracle's
    forward, clip and Adam: the mean (over non-pad tokens) of the distillation loss, its gradient by autograd.
    ``teacher_logits`` (B, T, V) float64.  -> (soft loss per token before every step, student logits before the first
    step, student logits after the last)."""
    import img2latex_oracle as O
    sd = {k: torch.from_numpy(np.asarray(v)).double().clone() for k, v in student_sd.items()}
    images, formulas = torch.as_tensor(images).double(), torch.as_tensor(formulas).long()
    tgt = formulas[:, 1:].reshape(-1)
    keep = tgt != pad
    y = torch.as_tensor(teacher_logits).double().reshape(tgt.numel(), -1)[keep]
    state, softs, first = {}, [], None
    for _ in range(steps + 1):
        params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        logits = O.seq2seq_forward(params, student_cfg, images, formulas)
        if first is None:
            first = logits.detach().clone()
        hard, soft = loss_terms_torch(logits.reshape(tgt.numel(), -1), y, tgt, pad, tau, eps)
        softs.append(float(soft.sum().detach() / keep.sum()))
        if len(softs) == steps + 1:
            return softs, first, logits.detach()
        loss = (alpha * hard.sum() + (1 - alpha) * soft.sum()) / keep.sum()
        gl = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
        grads = {k: (torch.zeros_like(sd[k]) if g is None else g.detach().clone()) for k, g in zip(params.keys(), gl)}
        O.clip_grad_norm(grads, clip)
        with torch.no_grad():
            O.adam_step(sd, grads, state, lr, weight_decay)


def floors(x, y, tgt, pad, tau, alpha, eps):
    """-> (dlogits floor (a number), hard floor (rows), soft floor (rows)); pad rows have floor 0.  ``y`` is distill_np's."""
    x = np.asarray(x, dtype=np.float64)
    tgt = np.asarray(tgt)
    rows, V = x.shape
    tau, alpha = f32(tau), f32(alpha)
    keep = tgt != pad
    x_t = x[np.arange(rows), np.clip(tgt, 0, V - 1)]
    hard = 2.0 ** -21 * (np.abs(_lse(x)[:, 0]) + np.abs(x.mean(axis=1)) + np.abs(x_t))
    lse_y, lse_x = _lse(y / tau), _lse(x / tau)
    q = np.exp(y / tau - lse_y)
    mag = (q * (np.abs(y) / tau + np.abs(lse_y) + np.abs(x) / tau + np.abs(lse_x))).sum(axis=1)
    soft = 2.0 ** -21 * tau * tau * mag
    return 2.0 ** -22 * (alpha + (1 - alpha) * tau), np.where(keep, hard, 0.0), np.where(keep, soft, 0.0)
