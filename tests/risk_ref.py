"""The rules of csrc/risk_rules.inc.h (minimum-risk fine-tuning) restated in Python / float64, and the weighted loss.

One image: a gold row ``formulas (T + 1)`` = [START, tokens ..., END, PAD ...] and ``N`` draws of ``T`` ids, -1 behind END.

    cut        draw: ids before the first END, all T without one; gold: formulas[1:] before the first END or PAD
    d          Levenshtein distance of the two cuts (the textbook table, Python ints)
    reward     1 - d / max(len_draw, len_gold), 1.0 when both are empty (Python floats are IEEE doubles)
    advantage  r[n] - (sum over m != n of r[m], in index order) / (N - 1)
    coef       gold: alpha as the C float carries it; draw: (1 - alpha) A[n] in double
    rows       gold row as it stands; [START, draw through its END, PAD ...]

Values stored as fp32 are the doubles rounded once (``np.float32``).  ``weighted_ce_np`` is the closed form of

    L_sum = sum over token rows of coef[seq] keep CE_smooth[seq](x, target)

and its gradient on numpy float64 arrays; ``weighted_ce_torch`` the autograd form (F.cross_entropy per sequence) in float64
or float32.  ``floors`` scales distill_ref's hard-term floors (2^-22 on a gradient in [-1, 1], 2^-21 x the magnitudes of
the terms that enter a row's loss) by |coef|.
"""
import numpy as np
import torch
import torch.nn.functional as F

from distill_ref import _lse, f32


def levenshtein_table(a, b):
    """The textbook table, one Python int at a time (the check of ``levenshtein`` below)."""
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        diag, row[0] = row[0], i
        for j in range(1, len(b) + 1):
            up = row[j]
            row[j] = min(diag + (a[i - 1] != b[j - 1]), up + 1, row[j - 1] + 1)
            diag = up
    return row[len(b)]


def levenshtein(a, b):
    """The same table a row at a time on int64 arrays: new[j] = min(t[j], new[j - 1] + 1) with t the minimum over the
    cell above and the diagonal is min over k <= j of (t[k] - k) + j, a running minimum.  Exact."""
    a, b = np.asarray(list(a), dtype=np.int64), np.asarray(list(b), dtype=np.int64)
    at = np.arange(len(b) + 1, dtype=np.int64)
    row = at.copy()
    for i in range(1, len(a) + 1):
        t = np.empty_like(row)
        t[0] = i
        t[1:] = np.minimum(row[:-1] + (b != a[i - 1]), row[1:] + 1)
        row = np.minimum.accumulate(t - at) + at
    return int(row[len(b)])


def cut_draw(draw, end):
    draw = [int(t) for t in draw]
    return draw[:draw.index(end)] if end in draw else draw


def cut_gold(formula, end, pad):
    out = []
    for t in (int(v) for v in formula[1:]):
        if t == end or t == pad:
            break
        out.append(t)
    return out


def risk_rows(formulas, draws, start, end, pad, alpha, smoothing):
    """formulas (B, T + 1), draws (B, N, T) ints -> dict of numpy arrays as i2l_risk_rows writes them: rows
    (B (N + 1), T + 1) int32, coef / smooth float32 and part int32 (B (N + 1)), dist / len int32 and reward / advantage
    float32 (B, N) -- plus "reward64" / "advantage64" / "coef64", the doubles before the one rounding."""
    formulas, draws = np.asarray(formulas), np.asarray(draws)
    B, N, T = draws.shape
    assert formulas.shape == (B, T + 1)
    alpha, smoothing = f32(alpha), f32(smoothing)
    rows = np.zeros((B * (N + 1), T + 1), dtype=np.int32)
    coef64 = np.zeros(B * (N + 1))
    smooth = np.zeros(B * (N + 1), dtype=np.float32)
    part = np.zeros(B * (N + 1), dtype=np.int32)
    dist, ln = np.zeros((B, N), dtype=np.int32), np.zeros((B, N), dtype=np.int32)
    reward64, adv64 = np.zeros((B, N)), np.zeros((B, N))
    for b in range(B):
        s0 = b * (N + 1)
        gold = cut_gold(formulas[b], end, pad)
        rows[s0] = formulas[b]
        coef64[s0], smooth[s0], part[s0] = alpha, smoothing, 0
        for n in range(N):
            seq = cut_draw(draws[b, n], end)
            d = levenshtein(seq, gold)
            longest = max(len(seq), len(gold))
            dist[b, n], ln[b, n] = d, len(seq)
            reward64[b, n] = 1.0 if longest == 0 else 1.0 - d / longest
            body = seq + ([end] if len(seq) < T else [])
            rows[s0 + 1 + n] = [start] + body + [pad] * (T - len(body))
            part[s0 + 1 + n] = 1
        for n in range(N):
            others = 0.0
            for m in range(N):
                if m != n:
                    others += reward64[b, m]
            adv64[b, n] = reward64[b, n] - others / (N - 1)
            coef64[s0 + 1 + n] = (1.0 - alpha) * adv64[b, n]
    return dict(rows=rows, coef=coef64.astype(np.float32), smooth=smooth, part=part, dist=dist, len=ln,
                reward=reward64.astype(np.float32), advantage=adv64.astype(np.float32), reward64=reward64,
                advantage64=adv64, coef64=coef64)


def weighted_ce_np(x, tgt, steps, pad, coef, smooth, part):
    """x (seqs * steps, V), tgt (seqs * steps), per-sequence coef / smooth (as fp32 values) / part -> dict of float64:
    loss (rows, unweighted, 0 at pad), d (rows, V), keep (rows) bool, out = [sum coef loss, count], parts (4)."""
    x = np.asarray(x, dtype=np.float64)
    tgt = np.asarray(tgt)
    rows, V = x.shape
    seq = np.arange(rows) // steps
    c = np.asarray(coef, dtype=np.float32).astype(np.float64)[seq]
    eps = np.asarray(smooth, dtype=np.float32).astype(np.float64)[seq]
    gold = np.asarray(part)[seq] == 0
    keep = tgt != pad
    tg = np.clip(tgt, 0, V - 1)
    lse = _lse(x)[:, 0]
    loss = (1 - eps) * (lse - x[np.arange(rows), tg]) + eps * (lse - x.mean(axis=1))
    onehot = np.zeros((rows, V))
    onehot[np.arange(rows), tg] = 1.0
    d = c[:, None] * (np.exp(x - lse[:, None]) - (1 - eps)[:, None] * onehot - (eps / V)[:, None])
    loss = np.where(keep, loss, 0.0)
    d = np.where(keep[:, None], d, 0.0)
    parts = np.array([loss[gold].sum(), float((keep & gold).sum()), loss[~gold].sum(), float((keep & ~gold).sum())])
    return dict(loss=loss, d=d, keep=keep, coef=c, out=np.array([(c * loss).sum(), float(keep.sum())]), parts=parts)


def weighted_ce_torch(x, tgt, steps, pad, coef, smooth, dtype=torch.float64):
    """The autograd form in ``dtype``: per sequence F.cross_entropy(ignore_index, label_smoothing, reduction="none"), the
    gradient of sum_rows coef loss.  -> dict(loss (rows), d (rows, V), total) as float64 numpy holding the ``dtype``
    values."""
    xg = torch.as_tensor(np.asarray(x)).to(dtype).clone().requires_grad_(True)
    t = torch.as_tensor(np.asarray(tgt)).long()
    seqs = xg.shape[0] // steps
    losses, total = [], 0
    for s in range(seqs):
        sl = slice(s * steps, (s + 1) * steps)
        row = F.cross_entropy(xg[sl], t[sl], ignore_index=pad, reduction="none", label_smoothing=f32(smooth[s]))
        losses.append(row)
        total = total + torch.tensor(f32(coef[s]), dtype=dtype) * row.sum()
    total.backward()
    return dict(loss=torch.cat(losses).detach().double().numpy(), d=xg.grad.double().numpy(), total=float(total.detach()))


def floors(x, tgt, pad, c):
    """-> (dlogits floor per row (rows), loss floor per row (rows)): distill_ref.floors' hard-term floors x |coef|; ``c``
    the per-ROW coefficients (weighted_ce_np's "coef")."""
    x = np.asarray(x, dtype=np.float64)
    tgt = np.asarray(tgt)
    rows, V = x.shape
    keep = tgt != pad
    x_t = x[np.arange(rows), np.clip(tgt, 0, V - 1)]
    hard = 2.0 ** -21 * (np.abs(_lse(x)[:, 0]) + np.abs(x.mean(axis=1)) + np.abs(x_t))
    return 2.0 ** -22 * np.abs(c), np.where(keep, hard, 0.0) * np.abs(c)
