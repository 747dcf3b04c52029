"""Shared helpers for the parity tests: fixtures -> (cfg, state_dict, inputs)."""
import json
import os

import numpy as np
import torch

from conftest import record
from img2latex_amd import synth
from img2latex_amd.model import Seq2SeqModel

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
START, END, PAD = synth.START, synth.END, synth.PAD
SMALL = ["tiny_l1", "tiny_l2_attn", "odd_dims", "odd_hidden"]   # odd_hidden: V 777, E 36, H 320, L 3
WIDE = ["ref_test_64x800", "shipped_128x800"]      # the reference's own shapes (tests/test_encoder.py:11-42, configs/config.yaml:30-50)
BIG = ["primary", "secondary"] + WIDE + ["wide_vocab"]   # fixtures that hold samples instead of whole tensors, T = 24
ALL = SMALL + BIG


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(d["cfg_json"]))
    sd_kw = json.loads(str(d["sd_kw_json"]))
    if "end_clock" in sd_kw and sd_kw["end_clock"] is not None:
        sd_kw["end_clock"] = tuple(sd_kw["end_clock"])
    return d, cfg, sd_kw


_SD_CACHE = {}


def np_state_dict(name):
    if name not in _SD_CACHE:
        _, cfg, sd_kw = load(name)
        _SD_CACHE[name] = synth.make_state_dict(cfg, **sd_kw)
    return _SD_CACHE[name]


def torch_state_dict(name, device="cpu"):
    return {k: torch.from_numpy(v.copy()).to(device) for k, v in np_state_dict(name).items()}


def images(cfg, batch=4, seed=1234, device="cpu"):
    return torch.from_numpy(synth.make_images(batch, cfg, seed=seed)).to(device)


# ---------------------------------------------------------------------------------------------------------------
# GPU parity checks shared by test_hip_parity.py and test_pipeline_headline.py
# ---------------------------------------------------------------------------------------------------------------
DEV = "cuda"


def close(a, b, tol, what=None, absolute=False):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = 1.0 if absolute else max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    if what:
        record(what + (" [abs]" if absolute else " [rel to max(1,|ref|)]"), err / scale)
    assert err <= tol * scale, f"{what}: max err {err} > {tol} * {scale}"


_MODELS = {}


def model_for(name, sd_kw=None, cfg=None):
    key = (name, repr(sd_kw))
    if key not in _MODELS:
        if cfg is None:
            _, cfg, kw = load(name)
            sd_kw = kw if sd_kw is None else sd_kw
        m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(cfg, **sd_kw).items()})
        _MODELS[key] = (m.to(DEV).eval(), cfg)
    return _MODELS[key]


def _margin_guard(got, ref_ids, margins, tol):
    """ids must agree with the reference up to the first step whose reference top1-top2
    margin is below tol (a fp32 near-tie, after which sequences legitimately diverge)."""
    diverged = 0
    for b in range(ref_ids.shape[0]):
        ne = np.nonzero(got[b] != ref_ids[b, 1:1 + got.shape[1]])[0]
        if ne.size:
            t = int(ne[0])
            assert margins[b, t] < tol, f"row {b} step {t}: ids differ at margin {margins[b, t]}"
            diverged += 1
    return diverged


def uniform01(seed, row, step):
    """Python twin of decode.hip::uniform01 (splitmix64 finaliser of (seed, row, step), 24 bits)."""
    M = (1 << 64) - 1
    z = (seed + (((row << 32) | step) * 0x9E3779B97F4A7C15)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z = z ^ (z >> 31)
    return np.float32(z >> 40) * np.float32(1.0 / 16777216.0)


def check_sampling(decoder, enc, oracle_step, top_k, top_p, temp, seed, steps=6, what=None):
    """predictor.py:295-331 through i2l_sample_decode: the masked / renormalised distribution equals the one rebuilt
    from ``oracle_step(tok (B,1) int64 on the host, hidden) -> (logits (B,1,V), hidden)`` replayed along the HIP-sampled
    tokens; every draw is the inverse-CDF of that distribution at the kernel's documented uniform (draws within 1e-5
    of a CDF step are not judged); same seed -> same ids."""
    from img2latex_amd import _lib
    rows = enc.shape[0]
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=enc.device)
    ids, probs = decoder.sample_steps(enc, steps, tok0, temp, top_k, top_p, seed, stop=_lib.STOP_NONE, want_probs=True)
    ids2, _ = decoder.sample_steps(enc, steps, tok0, temp, top_k, top_p, seed, stop=_lib.STOP_NONE)
    ids3, _ = decoder.sample_steps(enc, steps, tok0, temp, top_k, top_p, seed + 1, stop=_lib.STOP_NONE)
    assert torch.equal(ids, ids2)
    ids_h, probs_h = ids.cpu().numpy(), probs.cpu().numpy()
    tok = torch.full((rows, 1), START, dtype=torch.long)
    hidden = None
    for t in range(steps):
        with torch.no_grad():
            out, hidden = oracle_step(tok, hidden)
        p = torch.softmax(out.squeeze(1) / temp, dim=-1)
        if top_k > 0:
            kth = torch.topk(p, min(top_k, p.size(-1)), dim=-1).values[:, -1, None]
            p = torch.where(p < kth, torch.zeros_like(p), p)
            p = p / p.sum(-1, keepdim=True)
        if top_p > 0:
            sp, si = torch.sort(p, descending=True, stable=True)
            cum = torch.cumsum(sp, -1)
            rm = cum > top_p
            rm[:, 1:] = rm[:, :-1].clone()
            rm[:, 0] = False
            p = torch.where(rm.scatter(-1, si, rm), torch.zeros_like(p), p)
            p = p / p.sum(-1, keepdim=True)
        want = p.cpu().numpy()
        close(probs_h[:, t, :], want, 1e-5, what)
        for b in range(rows):
            pr = probs_h[b, t].astype(np.float32)
            assert pr[ids_h[b, t]] > 0
            u = uniform01(seed, b, t)
            cdf = np.cumsum(pr.astype(np.float64))
            j = int(np.searchsorted(cdf, float(u) * cdf[-1], side="right"))
            lo = cdf[j - 1] if j > 0 else 0.0
            if min(abs(float(u) * cdf[-1] - lo), abs(cdf[min(j, len(cdf) - 1)] - float(u) * cdf[-1])) > 1e-5:
                assert j == ids_h[b, t], (b, t, j, ids_h[b, t])
        tok = torch.from_numpy(ids_h[:, t:t + 1].astype(np.int64))
    if top_k != 1:
        assert not torch.equal(ids, ids3)        # a different seed draws different tokens
    else:
        assert torch.equal(ids, ids3)            # top-1 sampling is greedy


def padded_to_lists(arr, lens):
    return [list(map(int, arr[j, :lens[j]])) for j in range(len(lens))]


def sample(t, n=4096):
    f = t.detach().reshape(-1).cpu()
    step = max(1, f.numel() // n)
    return f[::step][:n].numpy()


# ---------------------------------------------------------------------------------------------------------------
# Discrete decisions of the conv blocks (pooling arg max, ReLU gate).  The conv gradients are discontinuous in them,
# and a near-tie (two window values, or a pre-activation and zero, closer than fp32 rounding resolves) is decided
# differently by different correct fp32 evaluations -- ATen's included.  The training tests therefore (1) read the
# choices the HIP forward made, (2) require that they differ from a float64 evaluation only at such near-ties, and
# (3) compare the HIP gradients element by element with the float64 gradient of the SAME choices
# (oracle.conv_block_decided), where the remaining difference is smooth rounding only.
# ---------------------------------------------------------------------------------------------------------------
def hip_decisions(model, x_dev):
    """Per conv block (argmax map, ReLU gate) of the HIP training forward (deterministic: same maps as inside a step)."""
    am = []
    with torch.no_grad():
        ys = model.encoder.conv_blocks(x_dev, am)
    return [(a.cpu().long(), (y > 0).cpu()) for a, y in zip(am, ys)]


def check_decisions(sd, cfg, x, decisions, tol=2e-6):
    """Against float64 (each block evaluated on the float64 output of the blocks before it UNDER the given decisions):
    a decision may differ only where the gap is below `tol` * sum |x||w| of the window -- what an fp32 dot product
    of that length cannot resolve.  Returns (number of windows deciding differently, number of windows)."""
    import torch.nn.functional as F
    import img2latex_oracle as O
    inp = x.double()
    n_off = n_all = 0
    for i, (am, gate) in enumerate(decisions):
        w = sd[f"encoder.cnn_layers.{3 * i}.weight"].double()
        b = sd[f"encoder.cnn_layers.{3 * i}.bias"].double()
        win = O.pool_windows(F.conv2d(inp, w, None, padding=1))
        mag = O.pool_windows(F.conv2d(inp.abs(), w.abs(), None, padding=1)).amax(-1) + b.abs()[None, :, None, None]
        top2 = win.topk(2, dim=-1).values
        gap = top2[..., 0] - top2[..., 1]
        pre = top2[..., 0] + b[None, :, None, None]
        wrong_gate = gate != (pre > 0)
        wrong_am = (am != win.argmax(-1)) & gate & (pre > 0) & (gap > 0)       # the arg max matters where the ReLU passes
        if wrong_am.any():
            # the chosen value, not just the runner-up, must be within tol of the maximum
            chosen = win.gather(-1, am.unsqueeze(-1)).squeeze(-1)
            worst = float(((top2[..., 0] - chosen)[wrong_am] / mag[wrong_am]).max())
            assert worst <= tol, f"block {i}: arg max differs from float64 at a gap of {worst:.2e} of sum|x||w|"
        if wrong_gate.any():
            worst = float((pre[wrong_gate].abs() / mag[wrong_gate]).max())
            assert worst <= tol, f"block {i}: ReLU gate differs from float64 at |pre| = {worst:.2e} of sum|x||w|"
        tie = (gap == 0) & gate & (pre > 0)
        assert bool((am[tie] == win.argmax(-1)[tie]).all()), f"block {i}: an exact tie must take the first index"
        n_off += int(wrong_am.sum()) + int(wrong_gate.sum())
        n_all += am.numel()
        inp = O.conv_block_decided(inp, w, b, am, gate)
    return n_off, n_all


# Operands that break a split-bf16 product scheme which only LOOKS fp32-grade on randn data (test_hip_parity.py,
# test_train_primitives.py)
ADVERSARIAL = ["cancellation", "range_2^+-60", "tiny_2^-100", "huge_2^+100"]


def _adversarial(kind, x, w, chan_dim_x, chan_dim_w, g):
    """Rewrites (x, w) along their reduction (input-channel / K) axis; returns the operands."""
    n = x.shape[chan_dim_x]
    if kind == "cancellation":          # consecutive reduction slots cancel to ~2^-12 of their size
        xe, xo = x.narrow(chan_dim_x, 0, n // 2 * 2).unfold(chan_dim_x, 2, 2).unbind(-1)
        we, wo = w.narrow(chan_dim_w, 0, n // 2 * 2).unfold(chan_dim_w, 2, 2).unbind(-1)
        xo.copy_(-xe * (1.0 + 2.0 ** -12))
        wo.copy_(we)
        x, w = x * 64.0, w * 64.0
    elif kind == "range_2^+-60":        # slot c scaled by 2^e_c in x and 2^-e_c in w: products stay O(1)
        e = torch.randint(-60, 61, (n,), generator=g).double()
        shape_x = [1] * x.dim(); shape_x[chan_dim_x] = n
        shape_w = [1] * w.dim(); shape_w[chan_dim_w] = n
        x = (x.double() * (2.0 ** e).reshape(shape_x)).float()
        w = (w.double() * (2.0 ** -e).reshape(shape_w)).float()
    elif kind == "tiny_2^-100":         # low split pieces at 2^-116: still normal bf16 numbers
        x = x * 2.0 ** -100
    elif kind == "huge_2^+100":
        x, w = x * 2.0 ** 100, w * 2.0 ** -20
    return x.contiguous(), w.contiguous()


def adam_first_step_allowance(g_a, g_b, p0, coef_a=1.0, coef_b=1.0, coef_unc=0.0, lr=1e-3, wd=1e-4, eps=1e-8, base=3e-6):
    """How far one parameter may move between two runs of the FIRST Adam step whose gradients are g_a and g_b and whose
    clip coefficients are coef_a and coef_b (each known to a relative `coef_unc`: the total norm is a sum over 11.6 M
    terms that torch accumulates in fp32 and the HIP kernel in double):
        p -= lr * f(x),  x = coef * g + wd * p0,  f(x) = x / (|x| + eps),  |f(a) - f(b)| <= min(2, |a - b| / (min(|a|, |b|) + eps)).
    An element whose |x| is at the level of x's own rounding error -- a tiny gradient, or a clipped gradient that happens
    to cancel the weight-decay term -- moves by up to lr either way."""
    xa, xb = coef_a * g_a + wd * p0, coef_b * g_b + wd * p0
    slack = coef_unc * torch.maximum((coef_a * g_a).abs(), (coef_b * g_b).abs())
    dx = (xa - xb).abs() + slack
    lo = torch.clamp(torch.minimum(xa.abs(), xb.abs()) - slack, min=0.0)
    return base + lr * torch.clamp(dx / (lo + eps), max=2.0)
