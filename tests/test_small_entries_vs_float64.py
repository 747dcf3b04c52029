"""Five small entry points -- i2l_grad_clip_adam_step (csrc/train_opt.hip), i2l_ce_label_smooth_fwd_bwd
(csrc/train_decoder.hip), i2l_attention_context_fwd (csrc/attention.hip), i2l_compact_ids (csrc/metrics.hip) and
i2l_resize_bilinear_f32 (csrc/preprocess.hip) -- each called on its own through the C ABI at the seams of its kernels
(grid-stride passes, 64-lane and 256-thread strides, alignment, LDS limit, refusals) and compared with a plain float64
CPU computation of the same operation: torch.optim.Adam + clip_grad_norm_, F.cross_entropy with autograd, the
reference's Attention.forward, ten lines of Python, ATen's bilinear formula.

One tolerance rule for every floating check: the same formulas are also evaluated in float32 on the CPU, and

    err_hip <= 4 * err_fp32cpu + floor

where `floor` is the rounding floor derived at each entry (stated in its section).  Errors that come through a quantity
a whole row shares (a row's log-sum-exp, the attention scores) take the row's / the case's maximum fp32 error, local
ones are judged element by element.  Both errors are record()ed in units of the floor for every case family.  Outputs
start as NaN or a sentinel and carry a sentinel head and tail that must survive the call."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record
from img2latex_amd import _lib

gpu = pytest.mark.gpu
DEV = "cuda"
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3
TAIL = 64
F32, F64 = torch.float32, torch.float64


def f32(x):
    """The value a C float argument carries, as a Python double."""
    return float(np.float32(x))


class Buf:
    """`host` (flattened) on the device at element offset `off`, between sentinel elements that must survive."""

    def __init__(self, host, off=0):
        host = host.reshape(-1)
        self.n, self.off, self.dtype = host.numel(), off, host.dtype
        self.sent = -1536.0 if host.dtype.is_floating_point else -77777
        self.buf = torch.full((off + self.n + TAIL,), self.sent, dtype=host.dtype, device=DEV)
        self.buf[off:off + self.n] = host.to(DEV)

    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def get(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        edge = torch.cat([host[:self.off], host[self.off + self.n:]])
        assert torch.equal(edge, torch.full_like(edge, self.sent)), "a write outside the buffer"
        return host[self.off:self.off + self.n].clone()


def nans(*shape):
    return torch.full(shape, float("nan"))


def judge(name, err_hip, err_cpu, floor, what=None, share=None):
    """err_hip <= 4 * err_fp32cpu + floor (tensors or numbers, broadcast); both recorded in units of the floor.
    share = "row" / "all": the fp32 error allowed is the largest of the element's row / of the whole case."""
    err_hip, err_cpu, floor = (torch.as_tensor(t, dtype=F64) for t in (err_hip, err_cpu, floor))
    floor = floor + 1e-300
    record(f"small entries {name} err_hip [floors]", float((err_hip / floor).max()))
    record(f"small entries {name} err_fp32cpu [floors]", float((err_cpu / floor).max()))
    if share is not None:
        err_cpu = err_cpu.amax(-1, keepdim=True) if share == "row" else err_cpu.max()
    assert torch.isfinite(err_hip).all(), (name, what)
    over = err_hip - (4 * err_cpu + floor)
    assert float(over.max()) <= 0, (name, what, float((err_hip / floor).max()), float((err_cpu / floor).max()))


# ---------------------------------------------------------------------------------------------------------------
# 1. i2l_grad_clip_adam_step
#    Floor: 2^-23 |p| + 2^-21 |update| on the parameter (one rounding of p, eight of the update's chain
#    g*gs + wd*p -> m, v -> sqrt -> / -> + eps -> / -> * step), 2^-22 of their magnitude on m and v, 2^-22 relative on
#    the norm and the clip coefficient.  Parameters are mostly 1e-3..1e-2 with lr = 1e-2, so that the update, not the
#    rounding of p, is what the parameter check sees; a quarter of them are 0.1..1.  A gradient element keeps its sign
#    from step to step, so that m never cancels, and |coef g / count + wd p| >= 1e-3 (asserted): away from the
#    x / (|x| + eps) discontinuity that helpers.adam_first_step_allowance is about.
# ---------------------------------------------------------------------------------------------------------------
HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)


def adam_restated(p, g, m, v, count, max_norm, hp, t, dtype):
    """clip_grad_norm_ + torch.optim.Adam's single-tensor step (coupled L2) in `dtype`, on the values the ABI receives:
    hyperparameters at their fp32 values, the bias corrections Python doubles, 1 / count folded into the gradient.
    Returns p', m', v', the update p - p', the gradient fed to the moments, total norm and clip coefficient."""
    lr, b1, b2, eps, wd, max_norm = (f32(x) for x in (hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], max_norm))
    p, g, m, v = (x.to(dtype) for x in (p, g, m, v))
    g = g / (1.0 if count is None else max(float(count), 1.0))
    total = torch.linalg.vector_norm(g)
    coef = torch.ones((), dtype=dtype)
    if max_norm > 0:
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        g = g * coef
    if wd != 0:
        g = g.add(p, alpha=wd)
    m = m.lerp(g, 1 - b1)
    v = (v * b2).addcmul(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = (v.sqrt() / bc2 ** 0.5).add(eps)
    upd = (lr / bc1) * (m / denom)
    return p - upd, m, v, upd, g, float(total), float(coef)


def torch_adam64(p, g, m, v, count, max_norm, hp, t, python_double_betas=False):
    """The real thing on float64 tensors: clip_grad_norm_ and torch.optim.Adam with the moments of step t - 1."""
    conv = (lambda x: x) if python_double_betas else f32
    w = torch.nn.Parameter(p.double().clone())
    w.grad = g.double() / (1.0 if count is None else max(float(count), 1.0))
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([w], f32(max_norm))
    opt = torch.optim.Adam([w], lr=f32(hp["lr"]), betas=(conv(hp["b1"]), conv(hp["b2"])), eps=f32(hp["eps"]),
                           weight_decay=f32(hp["wd"]), foreach=False)
    opt.state[w] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    opt.step()
    return w.detach(), opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"]


def adam_state(n, seed, moments):
    """p, the per-element gradient sign, m, v (zero, or m of the gradient's sign and v > 0) and the generator."""
    gen = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    psign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    small = torch.rand(n, generator=gen) < 0.75
    u = torch.rand(n, generator=gen)
    p = psign * torch.where(small, 1e-3 + 9e-3 * u, 0.1 + 0.9 * u)
    if moments:
        m = sign * (0.05 + 0.45 * torch.rand(n, generator=gen))
        v = (0.05 + 0.65 * torch.rand(n, generator=gen)) ** 2
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, sign, m, v, gen


def adam_grad(sign, gen, scale=1.0):
    """|g| / scale in [0.05, 1): after a clip coefficient of 0.5 still >= 0.025 > wd |p| + 1e-3."""
    return sign * (0.05 + 0.95 * torch.rand(sign.numel(), generator=gen)) * scale


def adam_ws():
    nbytes = _lib.lib().i2l_optimizer_workspace_bytes()
    return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)


def adam_skipped(ws):
    """The skipped-call counter: the first word of the workspace's last 256 bytes (csrc/train_opt.hip)."""
    torch.cuda.synchronize()
    return int(ws[ws.numel() - 256:ws.numel() - 252].cpu().view(torch.int32)[0])


def adam_call(p, g, m, v, count, max_norm, hp, step, off=0, ws=None):
    """One call on fresh device buffers; returns p', m', v', stats (host) and the workspace."""
    n = p.numel()
    P, G, M, V = (Buf(x.float(), off) for x in (p, g, m, v))
    S = Buf(nans(4))
    C = None if count is None else Buf(torch.tensor([float(count)]))
    ws = adam_ws() if ws is None else ws
    rc = _lib.lib().i2l_grad_clip_adam_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, None if C is None else C.ptr(),
                                            max_norm, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step,
                                            ws.data_ptr(), ws.numel(), S.ptr(), _lib.stream_ptr())
    assert rc == OK, rc
    assert torch.equal(G.get().view(torch.int32), g.float().view(torch.int32)), "the gradient is an input"
    return P.get(), M.get(), V.get(), S.get(), ws


def adam_check(family, p, g, m, v, count, max_norm, hp, step, t=None, off=0, ws=None, what=None, norm64=None,
               cpu=True):
    """One call against the float64 restatement under the 4x rule; `t` is the applied-step number when it differs
    from `step`; cpu=False: the floors alone (gradients whose squares overflow the fp32 CPU norm).  Returns the
    device results."""
    t = step if t is None else t
    got_p, got_m, got_v, stats, ws = adam_call(p, g, m, v, count, max_norm, hp, step, off, ws)
    p64, m64, v64, upd64, g64, tot64, coef64 = adam_restated(p, g, m, v, count, max_norm, hp, t, F64)
    p32, m32, v32, upd32, _, tot32, coef32 = adam_restated(p, g, m, v, count, max_norm, hp, t, F32)
    if not cpu:
        p32, m32, v32, upd32, tot32, coef32 = p64, m64, v64, upd64, tot64, coef64
    if hp["eps"] <= 1e-6:                               # the inputs keep the fp32 reference itself well-conditioned
        assert float(g64.abs().min()) >= 1e-3, what
        assert float(((upd32.double() - upd64).abs() / upd64.abs()).max()) <= 1e-6, what
    judge(f"adam {family} p", (got_p.double() - p64).abs(), (p32.double() - p64).abs(),
          2.0 ** -23 * p64.abs() + 2.0 ** -21 * upd64.abs(), what)
    judge(f"adam {family} m", (got_m.double() - m64).abs(), (m32.double() - m64).abs(), 2.0 ** -22 * m64.abs(), what)
    judge(f"adam {family} v", (got_v.double() - v64).abs(), (v32.double() - v64).abs(), 2.0 ** -22 * v64.abs(), what)
    if norm64 is not None:                              # a norm known in closed form
        assert abs(tot64 - norm64) <= 1e-13 * norm64, what
        tot64 = norm64
    judge(f"adam {family} total norm", abs(float(stats[0]) - tot64), abs(tot32 - tot64), 2.0 ** -22 * tot64, what)
    judge(f"adam {family} clip coefficient", abs(float(stats[1]) - coef64), abs(coef32 - coef64), 2.0 ** -22 * coef64, what)
    if max_norm <= 0 or f32(max_norm) > 1.001 * tot64:
        assert float(stats[1]) == 1.0, what
    inv = 1.0 if count is None else 1.0 / max(float(count), 1.0)
    assert abs(float(stats[2]) - inv) <= 2.0 ** -23 * inv, what
    assert float(stats[3]) == 0.0, what
    return got_p, got_m, got_v, stats, ws


ADAM_SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 262144, 262145, 262147, 1048581]


@gpu
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_sizes_vs_float64(n):
    """One to several grid-stride passes of both kernels and tails that are no multiple of 4 (1024 x 256 elements are
    one pass of the norm's partial sums, 4096 x 256 one of the update), third step on non-zero moments, clipped.
    The gradients are +-2^-k, so the norm is known in closed form: sqrt(sum 4^-k)."""
    p, sign, m, v, gen = adam_state(n, 1000 + n, moments=True)
    k = torch.randint(0, 5, (n,), generator=gen)
    g = sign * torch.pow(2.0, -k.float())
    norm = math.sqrt(sum(int((k == j).sum()) * 4 ** (4 - j) for j in range(5)) / 256.0)
    adam_check("sizes", p, g, m, v, None, 0.5 * norm, HP, 3, what=n, norm64=norm)


@gpu
@pytest.mark.parametrize("n", [257, 262147])
def test_adam_unaligned_equals_aligned(n):
    """Every buffer one float off a 16-byte boundary (the norm then reads element by element): the same bits as the
    aligned call on the same numbers, which in turn meets the float64 bounds."""
    p, sign, m, v, gen = adam_state(n, 2000 + n, moments=True)
    g = adam_grad(sign, gen, scale=3.0)
    max_norm = 0.5 * float(torch.linalg.vector_norm(g.double())) / 3.0
    assert Buf(p, 1).ptr() % 16 == 4 and Buf(p).ptr() % 16 == 0
    a = adam_check("alignment", p, g, m, v, 3.0, max_norm, HP, 2, what=n)
    b = adam_call(p, g, m, v, 3.0, max_norm, HP, 2, off=1)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y), n


@gpu
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_adam_modes_vs_float64(betas, eps):
    """count NULL / 0 (clamped to 1) / 137, no clip / coefficient exactly 1 / coefficient < 1, weight decay 0 / 1e-2,
    at n = 1023 on the third step with non-zero moments."""
    n = 1023
    p, sign, m, v, gen = adam_state(n, 31, moments=True)
    for count in (None, 0.0, 137.0):
        g = adam_grad(sign, gen, scale=count or 1.0)
        norm = float(torch.linalg.vector_norm(g.double())) / max(count or 1.0, 1.0)
        for max_norm in (0.0, -1.0, 2.0 * norm, 0.5 * norm):
            for wd in (0.0, 1e-2):
                hp = dict(HP, b1=betas[0], b2=betas[1], eps=eps, wd=wd)
                adam_check("modes", p, g, m, v, count, max_norm, hp, 3, what=(count, max_norm, wd))


@gpu
def test_adam_five_steps_vs_float64_and_torch_optim():
    """step = 1..5 from zero moments with a fresh gradient each; every step's reference starts from the device's own
    p, m, v of before the step, so nothing compounds.  The restatement the other tests use is torch.optim.Adam +
    clip_grad_norm_ themselves (1e-13).  Recorded only: the distance to torch.optim.Adam called with the Python-double
    betas 0.9 / 0.999 instead of their fp32 values, which the ABI cannot carry."""
    n = 4099
    p, sign, m, v, gen = adam_state(n, 41, moments=False)
    ws = adam_ws()
    for step in range(1, 6):
        g = adam_grad(sign, gen, scale=137.0)
        ref = adam_restated(p, g, m, v, 137.0, 20.0, HP, step, F64)
        real = torch_adam64(p, g, m, v, 137.0, 20.0, HP, step)
        for a, b in zip(ref[:3], real):
            assert float(((a - b).abs() / (b.abs() + 1e-2)).max()) <= 1e-13, step
        new = adam_check("steps", p, g, m, v, 137.0, 20.0, HP, step, ws=ws, what=step)
        dbl = torch_adam64(p, g, m, v, 137.0, 20.0, HP, step, python_double_betas=True)[0]
        upd = p.double() - dbl
        record("small entries adam update vs torch.optim.Adam(python-double betas) [relative]",
               float((((p.double() - new[0].double()) - upd).abs() / upd.abs())[p.abs() < 0.05].max()))
        p, m, v = new[:3]
    assert adam_skipped(ws) == 0


@gpu
def test_adam_step_1000_vs_float64():
    """Far into training: random non-negative v, bias corrections 1 - 0.9^1000 = 1 and 1 - 0.999^1000 = 0.632."""
    p, sign, m, v, gen = adam_state(4099, 43, moments=True)
    for eps in (1e-8, 1e-3):
        adam_check("step 1000", p, adam_grad(sign, gen), m, v, None, 0.0, dict(HP, eps=eps), 1000, what=eps)


@gpu
def test_adam_skip_bookkeeping():
    """good, NaN gradient, a gradient whose norm overflows fp32, good: the two bad calls leave p, m, v bit-identical
    and set stats[3]; the last call uses the bias correction of applied step 2; the workspace counter reads 2.  A large
    but finite norm (1000 elements of 1e30) is an ordinary clipped step."""
    n = 1000
    p, sign, m, v, gen = adam_state(n, 47, moments=False)
    ws = adam_ws()
    p, m, v, _, _ = adam_check("skip", p, adam_grad(sign, gen), m, v, None, 5.0, HP, 1, ws=ws, what="first")
    bad_nan = adam_grad(sign, gen)
    bad_nan[n // 2] = float("nan")
    bad_inf = adam_grad(sign, gen)
    bad_inf[:4] = 3e38
    for i, g in enumerate((bad_nan, bad_inf)):
        got_p, got_m, got_v, stats, _ = adam_call(p, g, m, v, None, 5.0, HP, 2 + i, ws=ws)
        assert torch.equal(got_p, p) and torch.equal(got_m, m) and torch.equal(got_v, v), i
        assert float(stats[3]) == 1.0 and float(stats[1]) == 0.0, (i, stats)
        assert not math.isfinite(float(stats[0])), (i, stats)
        assert adam_skipped(ws) == 1 + i
    adam_check("skip", p, adam_grad(sign, gen), m, v, None, 5.0, HP, 4, t=2, ws=ws, what="after two skipped calls")
    assert adam_skipped(ws) == 2
    big = sign * 1e30
    got = adam_check("skip", p, big, m, v, None, 1.0, HP, 5, t=3, ws=ws, what="1e30 x 1000", cpu=False)
    assert float(got[3][3]) == 0.0 and adam_skipped(ws) == 2
    assert abs(float(got[3][0]) - 1e30 * math.sqrt(1000)) <= 1e-6 * 1e30 * math.sqrt(1000)


@gpu
def test_adam_is_deterministic():
    n = 262147
    p, sign, m, v, gen = adam_state(n, 53, moments=True)
    g = adam_grad(sign, gen)
    a = adam_call(p, g, m, v, 137.0, 0.05, HP, 7)
    b = adam_call(p, g, m, v, 137.0, 0.05, HP, 7)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)


@gpu
def test_adam_refusals():
    """n == 0, step < 1, a NULL pointer, a missing or short workspace: an error code and no launch -- every buffer
    keeps its bits."""
    L = _lib.lib()
    n = 300
    p, sign, m, v, gen = adam_state(n, 59, moments=True)
    g = adam_grad(sign, gen)
    bufs = [Buf(x) for x in (p, g, m, v)]
    S = Buf(nans(4))
    ws = adam_ws()
    hp = (1.0, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"])

    def call(ptrs, n_, step, wsp, wsn, sp):
        return L.i2l_grad_clip_adam_step(*ptrs, n_, None, *hp, step, wsp, wsn, sp, _lib.stream_ptr())

    ptrs = [b.ptr() for b in bufs]
    assert call(ptrs, 0, 1, ws.data_ptr(), ws.numel(), S.ptr()) == ERR_ARG
    assert call(ptrs, n, 0, ws.data_ptr(), ws.numel(), S.ptr()) == ERR_ARG
    assert call(ptrs, n, -3, ws.data_ptr(), ws.numel(), S.ptr()) == ERR_ARG
    for i in range(4):
        assert call(ptrs[:i] + [None] + ptrs[i + 1:], n, 1, ws.data_ptr(), ws.numel(), S.ptr()) == ERR_ARG, i
    assert call(ptrs, n, 1, ws.data_ptr(), ws.numel(), None) == ERR_ARG
    assert call(ptrs, n, 1, None, ws.numel(), S.ptr()) == ERR_WORKSPACE
    assert call(ptrs, n, 1, ws.data_ptr(), ws.numel() - 1, S.ptr()) == ERR_WORKSPACE
    assert call(ptrs, n, 1, ws.data_ptr(), 0, S.ptr()) == ERR_WORKSPACE
    for b, x in zip(bufs, (p, g, m, v)):
        assert torch.equal(b.get(), x)
    assert torch.isnan(S.get()).all() and int(ws.cpu().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------
# 2. i2l_ce_label_smooth_fwd_bwd
#    Floor: 2^-22 absolute on dlogits (values in [-1, 1]); 2^-21 x sum over kept rows of (|lse| + |mean logit| + |x_t|)
#    on the loss sum.  A row's gradient shares the row's max and sum, so dlogits take the ROW's largest fp32 error.
# ---------------------------------------------------------------------------------------------------------------
def ce_call(logits, tgt, pad, eps, want_d=True):
    L = _lib.lib()
    rows, V = logits.shape
    X, T = Buf(logits), Buf(tgt.to(torch.int32))
    D = Buf(nans(rows, V)) if want_d else None
    out = Buf(nans(2))
    nbytes = L.i2l_ce_workspace_bytes(rows)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    rc = L.i2l_ce_label_smooth_fwd_bwd(X.ptr(), T.ptr(), rows, V, pad, eps, ws.data_ptr(), nbytes,
                                       D.ptr() if want_d else None, out.ptr(), _lib.stream_ptr())
    assert rc == OK, rc
    return out.get(), (D.get().reshape(rows, V) if want_d else None)


def ce_ref(logits, tgt, pad, eps, dtype):
    x = logits.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(x, tgt.long(), ignore_index=pad, reduction="sum", label_smoothing=f32(eps))
    loss.backward()
    return float(loss.detach()), x.grad


def ce_check(family, logits, tgt, pad, eps, what):
    rows, V = logits.shape
    out, d = ce_call(logits, tgt, pad, eps)
    out_null, _ = ce_call(logits, tgt, pad, eps, want_d=False)
    assert torch.equal(out, out_null), what                             # the same two floats without dlogits
    keep = tgt != pad
    assert float(out[1]) == float(keep.sum()), what                     # an exact integer
    assert torch.isfinite(out).all() and torch.isfinite(d).all(), what
    assert torch.equal(d[~keep], torch.zeros_like(d[~keep])), what      # +0 or -0: exactly zero
    if not keep.any():
        assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and not d.any(), what
    loss64, d64 = ce_ref(logits, tgt, pad, eps, F64)
    loss32, d32 = ce_ref(logits, tgt, pad, eps, F32)
    judge(f"ce {family} dlogits", (d.double() - d64).abs(), (d32.double() - d64).abs(), 2.0 ** -22, what, share="row")
    x64 = logits.double()
    lse = torch.logsumexp(x64, 1)
    x_t = x64.gather(1, tgt.long().clamp(0, V - 1)[:, None])[:, 0]
    mag = ((lse.abs() + x64.mean(1).abs() + x_t.abs()) * keep).sum()
    judge(f"ce {family} loss sum", abs(float(out[0]) - loss64), abs(loss32 - loss64), 2.0 ** -21 * float(mag), what)
    sums = d.double().sum(1)[keep]                                      # softmax sums to 1, the target terms to 1
    if sums.numel():
        record(f"small entries ce {family} |sum_v dlogits| [V x 2^-23]", float(sums.abs().max()) / (V * 2.0 ** -23))
        assert float(sums.abs().max()) <= V * 2.0 ** -23, what


CE_V = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 5000]
CE_SHAPES = [(7, V) for V in CE_V] + [(r, V) for V in (65, 513) for r in (1, 257, 1000)]


def ce_targets(rows, V, pad, gen):
    """Random targets in [0, V) with every fifth row (from row 1) the pad id."""
    tgt = torch.randint(0, V, (rows,), generator=gen)
    tgt[1::5] = pad
    return tgt


@gpu
@pytest.mark.parametrize("rows,V", CE_SHAPES)
def test_ce_shapes_vs_float64(rows, V):
    """V around the 64-lane and 256-thread strides, rows around the 256-thread stride of the ordered sum; smoothing 0,
    0.1 and 0.5; pad id 0, 3 and -100 (outside [0, V): only targets of -100 are ignored)."""
    gen = torch.Generator().manual_seed(rows * 10007 + V)
    logits = torch.randn(rows, V, generator=gen) * 3
    for pad in (0, 3, -100):
        tgt = ce_targets(rows, V, pad, gen)
        for eps in (0.0, 0.1, 0.5):
            ce_check("shapes", logits, tgt, pad, eps, (rows, V, pad, eps))


@gpu
@pytest.mark.parametrize("V", [65, 513])
def test_ce_row_mix(V):
    """An all-PAD batch gives exactly (0, 0) and zero gradients; a batch with exactly one kept row."""
    rows = 260
    gen = torch.Generator().manual_seed(V)
    logits = torch.randn(rows, V, generator=gen) * 3
    for pad in (0, 3, -100):
        tgt = torch.full((rows,), pad)
        ce_check("row mix", logits, tgt, pad, 0.1, (V, pad, "all pad"))
        tgt[257] = 7
        ce_check("row mix", logits, tgt, pad, 0.1, (V, pad, "one kept"))


@gpu
@pytest.mark.parametrize("V", [2, 65, 513, 5000])
def test_ce_extreme_logits(V):
    """Rows scaled by 30, one logit of +1e4 among zeros (at and off the target), a row of all -1e4, rows of equal
    values: finite, within the float64 bounds, and a kept row's gradient sums to zero within V x 2^-23."""
    gen = torch.Generator().manual_seed(77 + V)
    logits = torch.randn(12, V, generator=gen) * 90          # 3 x 30
    tgt = torch.randint(0, V, (12,), generator=gen)
    tgt[5] = 0
    logits[6], logits[7] = 0.0, 0.0
    logits[6, V - 1], logits[7, V // 2] = 1e4, 1e4
    tgt[6], tgt[7] = V - 1, 0
    logits[8], logits[9], logits[10] = -1e4, 0.0, 88.5
    for pad in (0, -100):
        for eps in (0.0, 0.1):
            ce_check("extreme", logits, tgt, pad, eps, (V, pad, eps))


@gpu
@pytest.mark.parametrize("V", [65, 513])
def test_ce_minus_inf_logits(V):
    """-inf logits (a masked vocabulary).  Smoothing 0 has no smoothing term, as in torch: with -inf in non-target
    columns only, the loss sum and the gradient are finite and within the float64 bounds (the floor without the mean
    logit, which the loss then does not contain); with -inf at a kept target the sum is +inf.  Smoothing 0.1: +inf."""
    gen = torch.Generator().manual_seed(31 + V)
    rows = 9
    logits = torch.randn(rows, V, generator=gen) * 3
    tgt = torch.randint(4, V - 1, (rows,), generator=gen)
    tgt[tgt == V // 2 - 20] = 5
    tgt[1::5] = 0
    logits[:, 1], logits[::2, V // 2 - 20], logits[3, V - 1] = -math.inf, -math.inf, -math.inf
    logits[1, 2:] = -math.inf                                           # a pad row, all but one logit masked
    out, d = ce_call(logits, tgt, 0, 0.0)
    keep = tgt != 0
    loss64, d64 = ce_ref(logits, tgt, 0, 0.0, F64)
    loss32, d32 = ce_ref(logits, tgt, 0, 0.0, F32)
    assert math.isfinite(loss64) and float(out[1]) == float(keep.sum())
    assert torch.isfinite(out).all() and torch.isfinite(d).all()
    judge("ce -inf dlogits", (d.double() - d64).abs(), (d32.double() - d64).abs(), 2.0 ** -22, V, share="row")
    x64 = logits.double()
    mag = ((torch.logsumexp(x64, 1).abs() + x64.gather(1, tgt[:, None])[:, 0].abs()) * keep).sum()
    judge("ce -inf loss sum", abs(float(out[0]) - loss64), abs(loss32 - loss64), 2.0 ** -21 * float(mag), V)
    assert ce_ref(logits, tgt, 0, 0.1, F64)[0] == math.inf and float(ce_call(logits, tgt, 0, 0.1)[0][0]) == math.inf
    logits[4, tgt[4]] = -math.inf                                       # -inf at a kept target
    assert ce_ref(logits, tgt, 0, 0.0, F64)[0] == math.inf and float(ce_call(logits, tgt, 0, 0.0)[0][0]) == math.inf


@gpu
def test_ce_refusals():
    L = _lib.lib()
    rows, V = 9, 33
    X, T = Buf(torch.zeros(rows, V)), Buf(torch.ones(rows, dtype=torch.int32))
    D, out = Buf(nans(rows, V)), Buf(nans(2))
    nbytes = L.i2l_ce_workspace_bytes(rows)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def call(x, t, r, v, wsp, wsn, o):
        return L.i2l_ce_label_smooth_fwd_bwd(x, t, r, v, 0, 0.1, wsp, wsn, D.ptr(), o, _lib.stream_ptr())

    good = (X.ptr(), T.ptr(), rows, V, ws.data_ptr(), nbytes, out.ptr())
    for i, bad in ((0, None), (1, None), (6, None), (2, 0), (2, -1), (3, 0), (3, -5)):
        assert call(*(good[:i] + (bad,) + good[i + 1:])) == ERR_ARG, (i, bad)
    assert call(*(good[:4] + (None,) + good[5:])) == ERR_WORKSPACE
    assert call(*(good[:5] + (nbytes - 1,) + good[6:])) == ERR_WORKSPACE
    assert L.i2l_ce_workspace_bytes(0) == 0 and L.i2l_ce_workspace_bytes(-1) == 0
    assert torch.isnan(D.get()).all() and torch.isnan(out.get()).all() and int(ws.cpu().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------
# 3. i2l_attention_context_fwd
#    Floor: 2^-21 x sum_s |weight_s| |enc[s, e]| for the weighted sum itself.  What comes through the scores (a long
#    fp32 dot product, tanh, softmax) moves a whole row of the context at once: it takes 4x the case's largest fp32
#    CPU error.
# ---------------------------------------------------------------------------------------------------------------
def attention_ref(hidden, enc, w_attn, b_attn, v, dtype):
    """Attention.forward of the reference (decoder.py:312-343): context (B, E) and the weights (B, S)."""
    hidden, enc, w_attn, b_attn, v = (t.to(dtype) for t in (hidden, enc, w_attn, b_attn, v))
    S = enc.shape[1]
    cat = torch.cat((hidden[:, None, :].repeat(1, S, 1), enc), dim=2)
    energy = torch.tanh(F.linear(cat, w_attn, b_attn))
    attention = F.linear(energy, v[None, :]).squeeze(2)
    weights = F.softmax(attention, dim=1)
    return torch.bmm(weights.unsqueeze(1), enc).squeeze(1), weights


def attention_operands(B, S, H, E, seed):
    gen = torch.Generator().manual_seed(seed)
    hidden = torch.rand(B, H, generator=gen) * 2 - 1
    enc = torch.randn(B, S, E, generator=gen)
    w_attn = torch.randn(H, H + E, generator=gen) / math.sqrt(H + E)
    b_attn = torch.randn(H, generator=gen) * 0.1
    v = torch.randn(H, generator=gen) / math.sqrt(H)
    return hidden, enc, w_attn, b_attn, v


def attention_call(hidden, enc, w_attn, b_attn, v, expect=OK):
    B, S, E = enc.shape
    H = hidden.shape[1]
    bufs = [Buf(t) for t in (hidden, enc, w_attn, b_attn, v)]
    ctx = Buf(nans(B, E))
    rc = _lib.lib().i2l_attention_context_fwd(*[b.ptr() for b in bufs], ctx.ptr(), B, S, H, E, _lib.stream_ptr())
    assert rc == expect, (rc, B, S, H, E)
    got = ctx.get().reshape(B, E)
    for b, t in zip(bufs, (hidden, enc, w_attn, b_attn, v)):
        assert torch.equal(b.get(), t.reshape(-1))
    return got


def attention_check(family, ops, what):
    hidden, enc = ops[0], ops[1]
    got = attention_call(*ops)
    assert torch.isfinite(got).all(), what
    if enc.shape[1] == 1:                                   # the decoder's case: the context IS the encoder vector
        assert torch.equal(got, enc[:, 0]), what
    c64, w64 = attention_ref(*ops, F64)
    c32, _ = attention_ref(*ops, F32)
    floor = 2.0 ** -21 * torch.einsum("bs,bse->be", w64.abs(), enc.double().abs())
    judge(f"attention {family}", (got.double() - c64).abs(), (c32.double() - c64).abs(), floor, what, share="all")
    return got, c64


ATTN_STRIDES = [(2, 5, H, 37) for H in (1, 63, 64, 65, 255, 256, 257, 512, 1000)] + \
               [(2, 5, 64, E) for E in (1, 37, 255, 256, 257, 512, 600)]
ATTN_LENGTHS = [(3, S, 96, 48) for S in (1, 2, 64, 65, 300)]


@gpu
@pytest.mark.parametrize("B,S,H,E", ATTN_STRIDES + ATTN_LENGTHS + [(5, 9, 512, 512), (4, 1, 512, 512), (2, 1, 257, 600)])
def test_attention_shapes_vs_float64(B, S, H, E):
    """H and E on both sides of the 64-lane and 256-thread strides (the hidden half, the score and the context loops
    each stride by 256), source lengths around 64, the shipped decoder's 512 x 512, and S = 1 at the widths past the
    strides: there the context must equal enc bit for bit, whatever the weights."""
    attention_check("shapes", attention_operands(B, S, H, E, 7 * H + E + S), (B, S, H, E))


@gpu
def test_attention_saturation():
    """v x 50: a nearly one-hot softmax; w_attn x 20: tanh saturates; v = 0: all scores equal, the context is the
    plain mean of enc over s."""
    B, S, H, E = 3, 9, 96, 48
    hidden, enc, w_attn, b_attn, v = attention_operands(B, S, H, E, 5)
    attention_check("saturation", (hidden, enc, w_attn, b_attn, v * 50), "v x 50")
    attention_check("saturation", (hidden, enc, w_attn * 20, b_attn, v), "w_attn x 20")
    attention_check("saturation", (hidden, enc, w_attn * 20, b_attn, v * 50), "both")
    got, _ = attention_check("saturation", (hidden, enc, w_attn, b_attn, v * 0), "v = 0")
    mean = enc.double().mean(1)
    assert float(((got.double() - mean).abs() - 2.0 ** -21 * enc.double().abs().mean(1)).max()) <= 0


@gpu
def test_attention_lds_bound():
    """The largest source length the entry accepts at H = 64 -- (H + S + 4) * 4 bytes == 64 KiB, S = 16316 -- runs and
    agrees with float64; S = 16317 is refused as unsupported and leaves `context` alone."""
    B, H, E = 1, 64, 4
    attention_check("LDS bound", attention_operands(B, 16316, H, E, 11), "S = 16316")
    ops = attention_operands(B, 16317, H, E, 11)
    got = attention_call(*ops, expect=ERR_UNSUPPORTED)
    assert torch.isnan(got).all()


@gpu
def test_attention_refusals():
    L = _lib.lib()
    B, S, H, E = 2, 3, 8, 5
    ops = attention_operands(B, S, H, E, 3)
    bufs = [Buf(t) for t in ops]
    ctx = Buf(nans(B, E))
    good = tuple(b.ptr() for b in bufs) + (ctx.ptr(), B, S, H, E)
    for i in range(6):
        assert L.i2l_attention_context_fwd(*(good[:i] + (None,) + good[i + 1:]), _lib.stream_ptr()) == ERR_ARG, i
    for i in range(6, 10):
        for bad in (0, -1):
            assert L.i2l_attention_context_fwd(*(good[:i] + (bad,) + good[i + 1:]), _lib.stream_ptr()) == ERR_ARG, i
    assert torch.isnan(ctx.get()).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. i2l_compact_ids -- integer work, exact
# ---------------------------------------------------------------------------------------------------------------
def compact_rule(row, end_id, drop):
    """The header's rule: keep, in order, the ids before the first stop (id == end_id, or id < 0) that are not dropped."""
    out = []
    for t in row:
        if t == end_id or t < 0:
            break
        if t not in drop:
            out.append(t)
    return out


def test_compact_rule_is_the_host_decode_path():
    """The rule above against the host path: the predictor's cut before the first END or negative filler followed by
    the tokenizer's decode(skip_special_tokens=True), on 400 random rows.  TokenTable.decode is called; the cut is a
    COPY of the two lines of Predictor.predict_batch_ids (that method needs a model), so a change there is not seen
    here."""
    from img2latex_amd.training.predictor import DEFAULT_SPECIAL_TOKENS, TokenTable
    vocab = {t: i for i, t in enumerate(list(DEFAULT_SPECIAL_TOKENS.values()) + [f"t{i}" for i in range(4, 40)])}
    table = TokenTable(vocab)
    end = table.end_token_id
    drop = {vocab[t] for t in DEFAULT_SPECIAL_TOKENS.values()}
    rng = np.random.default_rng(5)
    a = rng.integers(0, 40, size=(400, 70))
    a[rng.random(a.shape) < 0.02] = end
    a[rng.random(a.shape) < 0.01] = -1
    a[:40, :] = np.where(a[:40, :] == end, 7, np.abs(a[:40, :]))         # rows without any stop
    a[40:60, 0] = end
    stop = (a == end) | (a < 0)                                          # copied from Predictor.predict_batch_ids
    lens = np.where(stop.any(axis=1), stop.argmax(axis=1), a.shape[1]).tolist()
    for row, n in zip(a.tolist(), lens):
        want = table.decode(row[:n])
        assert " ".join(table.id_to_token[i] for i in compact_rule(row, end, drop)) == want
    assert min(lens) == 0 and max(lens) == 70


DROP8 = [0, 1, 2, 3, 5, 8, 13, 21]
#                 n_drop, drop ids, end id
COMPACT_CONFIGS = [(0, None, 2), (1, [0], 2), (8, DROP8, 2), (8, DROP8, -1), (1, [0], -1)]


def compact_rows(rows, width, end_id, drop, seed):
    """Rows whose first stop sits at column 0, 62, 63, 64, 65, width - 1 or nowhere, as END, -1 or -3, with a second
    stop behind it in every other row; rows of dropped ids only; dropped ids on both sides of column 64."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 40, size=(rows, width)).astype(np.int32)
    if end_id >= 0:
        a[a == end_id] = 30
    stops = [c for c in (0, 62, 63, 64, 65, width - 1) if c < width] + [None]
    kinds = [end_id, -1, -3] if end_id >= 0 else [-1, -3]
    for r in range(rows):
        i = r + width + seed
        col, kind = stops[i % len(stops)], kinds[(i // len(stops)) % len(kinds)]
        recipe = (i // (len(stops) * len(kinds))) % 4
        if recipe == 1 and drop:
            a[r, :] = np.asarray(drop, dtype=np.int32)[rng.integers(0, len(drop), size=width)]
            if end_id >= 0:
                a[r][a[r] == end_id] = drop[0]
        elif recipe == 2 and drop:
            a[r, max(0, min(width, 64) - 3):min(width, 67)] = drop[-1] if drop[-1] != end_id else drop[0]
        if col is not None:
            a[r, col] = kind
            if r % 2 and col + 2 < width:
                a[r, col + 2] = kinds[(i + 1) % len(kinds)]
    return a


@gpu
@pytest.mark.parametrize("width", [1, 63, 64, 65, 128, 129, 200])
def test_compact_ids_exact(width):
    """rows 1..257 (a ragged last workgroup), stride = width + 7 with END and negative junk behind `width`,
    out_stride = width + 5 pre-filled with a sentinel; drop lists of 0 (NULL), 1 and 8 ids, one of them END itself;
    end_id = -1, where only a negative id stops a row."""
    L = _lib.lib()
    stride, out_stride = width + 7, width + 5
    for rows in (1, 3, 4, 5, 257):
        for n_drop, drop, end_id in COMPACT_CONFIGS:
            a = compact_rows(rows, width, end_id, drop or [], rows + 3 * n_drop)
            full = np.empty((rows, stride), dtype=np.int32)
            full[:, :width] = a
            full[:, width:] = np.asarray([max(end_id, 2), -1, 7, -3, 2, 0, 1], dtype=np.int32)
            ids = Buf(torch.from_numpy(full))
            drops = Buf(torch.tensor(drop, dtype=torch.int32)) if drop else None
            out = Buf(torch.full((rows, out_stride), -5555, dtype=torch.int32))
            out_len = Buf(torch.full((rows,), -5555, dtype=torch.int32))
            rc = L.i2l_compact_ids(ids.ptr(), rows, width, stride, end_id, drops.ptr() if drops else None, n_drop,
                                   out.ptr(), out_stride, out_len.ptr(), _lib.stream_ptr())
            assert rc == OK, rc
            got, lens = out.get().reshape(rows, out_stride).numpy(), out_len.get().numpy()
            assert torch.equal(ids.get().reshape(rows, stride), torch.from_numpy(full))
            for r in range(rows):
                want = compact_rule(a[r].tolist(), end_id, set(drop or []))
                what = (width, rows, n_drop, end_id, r)
                assert int(lens[r]) == len(want), what
                assert got[r, :len(want)].tolist() == want, what
                assert (got[r, len(want):] == -5555).all(), what          # nothing behind the kept ids, none >= width


@gpu
def test_compact_ids_refusals():
    L = _lib.lib()
    rows, width = 3, 10
    ids = Buf(torch.zeros(rows, width, dtype=torch.int32))
    drops = Buf(torch.arange(9, dtype=torch.int32))
    out = Buf(torch.full((rows, width), -5555, dtype=torch.int32))
    out_len = Buf(torch.full((rows,), -5555, dtype=torch.int32))
    #       ids, rows, width, stride, end, drop, n_drop, out, out_stride, out_len
    good = (ids.ptr(), rows, width, width, 2, drops.ptr(), 8, out.ptr(), width, out_len.ptr())
    for i, bad in ((6, 9), (6, -1), (5, None), (3, width - 1), (8, width - 1), (1, 0), (1, -2), (2, 0), (0, None),
                   (7, None), (9, None)):
        assert L.i2l_compact_ids(*(good[:i] + (bad,) + good[i + 1:]), _lib.stream_ptr()) == ERR_ARG, (i, bad)
    assert (out.get() == -5555).all() and (out_len.get() == -5555).all()


# ---------------------------------------------------------------------------------------------------------------
# 5. i2l_resize_bilinear_f32
#    (a) the documented formula: scale and source coordinates in fp32 exactly as ATen computes them, the blend in
#        float64.  Floor 8 x 2^-24 x max |the four neighbours| (1 - l, four products, three sums).
#    (b) F.interpolate(mode="bilinear", align_corners=False) in fp32 on the CPU: 1e-6 x max |src|, the header's number;
#        it is also the fp32 CPU evaluation of the 4x rule.
# ---------------------------------------------------------------------------------------------------------------
#                  planes, (in_h, in_w), (out_h, out_w)
BILINEAR_SHAPES = [(p, i, o) for p in (1, 3) for i, o in [
    ((5, 7), (5, 7)), ((1, 1), (5, 7)), ((3, 3), (7, 7)), ((7, 5), (3, 2)), ((64, 800), (64, 800)),
    ((37, 211), (64, 800)), ((128, 1600), (64, 800)), ((2, 2), (1, 1)), ((5, 9), (1, 1))]] + \
    [(40, (16, 32), (128, 256))]                            # 40 x 128 x 256 outputs > 4096 x 256: the grid stride


def bilinear_src(planes, size):
    gen = torch.Generator().manual_seed(planes * 131 + size[0] * 17 + size[1])
    return torch.rand(planes, size[0], size[1], generator=gen) * 2 - 1


def bilinear_restated(src, out_size):
    """float64 blend at ATen's fp32 coordinates: scale = (float)in / out, src = max(0, scale * (dst + 0.5) - 0.5) with
    the product and the subtraction rounded once -- the fused multiply-add ATen's kernels are compiled to (its
    vectorised CPU build and its GPU build; test_bilinear_restatement_is_atens holds this to the CPU build).
    Returns the result and max |the four neighbours| per output."""
    def axis(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        dst = np.arange(n_out, dtype=np.float32) + np.float32(0.5)
        assert scale.dtype == np.float32 and dst.dtype == np.float32
        f = np.maximum((np.float64(scale) * dst.astype(np.float64) - 0.5).astype(np.float32), np.float32(0.0))   # exact in double
        i0 = np.minimum(f.astype(np.int64), n_in - 1)
        lam = (f - i0.astype(np.float32)).astype(np.float64)
        return i0, np.minimum(i0 + 1, n_in - 1), lam
    s = src.double().numpy()
    y0, y1, ly = axis(s.shape[1], out_size[0])
    x0, x1, lx = axis(s.shape[2], out_size[1])
    ly = ly[None, :, None]
    lx = lx[None, None, :]
    n = [s[:, ya][:, :, xa] for ya in (y0, y1) for xa in (x0, x1)]
    top = (1 - lx) * n[0] + lx * n[1]
    bot = (1 - lx) * n[2] + lx * n[3]
    return torch.from_numpy((1 - ly) * top + ly * bot), torch.from_numpy(np.max(np.abs(np.stack(n)), axis=0))


def aten_bilinear(src, out_size):
    return F.interpolate(src[None], size=out_size, mode="bilinear", align_corners=False)[0]


@pytest.mark.parametrize("planes,in_size,out_size", BILINEAR_SHAPES)
def test_bilinear_restatement_is_atens(planes, in_size, out_size):
    """Without a GPU: the float64 restatement and ATen's fp32 result agree within 1e-6 x max |src| on every shape.
    This rests on the ATen CPU kernel in use contracting scale * (dst + 0.5) - 0.5 into one fused multiply-add, as its
    AVX2 and AVX512 builds do.  Where ATen dispatches to a build without FMA (ATEN_CPU_CAPABILITY=default, or a CPU
    without it), ATen's own coordinate moves by an ulp at some columns -- 1e-5 x max |src| at (37, 211) -> (64, 800) --
    and this test fails with neither the restatement nor the kernel at fault."""
    src = bilinear_src(planes, in_size)
    a, _ = bilinear_restated(src, out_size)
    b = aten_bilinear(src, out_size)
    assert a.shape == b.shape
    assert float((a - b.double()).abs().max()) <= 1e-6 * float(src.abs().max())


@gpu
@pytest.mark.parametrize("planes,in_size,out_size", BILINEAR_SHAPES)
def test_bilinear_vs_float64_and_aten(planes, in_size, out_size):
    """Identity (a bit-exact copy), a constant, up- and down-scaling in one or both directions, to a single pixel, and
    more outputs than one grid pass: against the float64 blend (4x rule) and against ATen's fp32 result (1e-6)."""
    src = bilinear_src(planes, in_size)
    X, Y = Buf(src), Buf(nans(planes, *out_size))
    rc = _lib.lib().i2l_resize_bilinear_f32(X.ptr(), Y.ptr(), planes, *in_size, *out_size, _lib.stream_ptr())
    assert rc == OK, rc
    got = Y.get().reshape(planes, *out_size)
    assert torch.equal(X.get().reshape(src.shape), src)
    if in_size == out_size:
        assert torch.equal(got, src)                                    # a bit-exact copy
    a, mag = bilinear_restated(src, out_size)
    b = aten_bilinear(src, out_size)
    judge("bilinear", (got.double() - a).abs(), (b.double() - a).abs(), 8 * 2.0 ** -24 * mag, (planes, in_size, out_size))
    vs_aten = float((got - b).abs().max()) / float(src.abs().max())
    record("small entries bilinear vs ATen fp32 [err / max|src|]", vs_aten)
    assert vs_aten <= 1e-6


@gpu
def test_bilinear_refusals():
    L = _lib.lib()
    X, Y = Buf(torch.zeros(2, 3, 4)), Buf(nans(2, 5, 6))
    good = (X.ptr(), Y.ptr(), 2, 3, 4, 5, 6)
    for i in range(2):
        assert L.i2l_resize_bilinear_f32(*(good[:i] + (None,) + good[i + 1:]), _lib.stream_ptr()) == ERR_ARG
    for i in range(2, 7):
        for bad in (0, -1):
            assert L.i2l_resize_bilinear_f32(*(good[:i] + (bad,) + good[i + 1:]), _lib.stream_ptr()) == ERR_ARG, (i, bad)
    assert torch.isnan(Y.get()).all()
