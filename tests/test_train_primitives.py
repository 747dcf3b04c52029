"""The ResNet training primitives (csrc/resnet_train.hip), the bf16 inference pools (csrc/resnet.hip) and the linear
layer's backward (csrc/gemm.hip), each called on its own through the C ABI at odd and edge shapes and compared with a
plain float64 CPU computation of the same operation.

Every bound scales with the operands: a GEMM-shaped result may miss its float64 value by 2^-20 of the sum of the
magnitudes of its products (the class of an fp32 fmaf chain), a pool or a gather must be exact, and a BatchNorm
quantity is judged against the float64 statistics of the same fp32 z.  Outputs start as NaN (or as known integers
where the kernel adds to them) and carry a sentinel tail that must survive the call.  The worst measured ratio of every
family is record()ed into parity_errors.json."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import record
from helpers import _adversarial
from img2latex_amd import _lib

DEV = "cuda"
ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3
TAIL = 64
SENTINEL = -1536.0                       # exact in fp32 and bf16


class Out:
    """A device output of `shape` followed by TAIL sentinel elements; `init` (a CPU tensor) or `fill` is the content."""

    def __init__(self, shape, fill=float("nan"), dtype=torch.float32, init=None):
        self.shape, self.n, self.dtype = tuple(shape), math.prod(shape), dtype
        self.buf = torch.full((self.n + TAIL,), SENTINEL, dtype=dtype, device=DEV)
        if init is not None:
            self.buf[:self.n] = init.reshape(-1).to(dtype).to(DEV)
        else:
            self.buf[:self.n] = fill

    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert torch.equal(host[self.n:], torch.full((TAIL,), SENTINEL, dtype=self.dtype)), "a write past the end"
        return host[:self.n].reshape(self.shape)


def _dev(t):
    return t.contiguous().to(DEV)


def _ws(nbytes):
    """A workspace of exactly `nbytes` (0xFF bytes: NaN as fp32, so nothing may rely on its content)."""
    return torch.full((max(nbytes, 16),), 255, dtype=torch.uint8, device=DEV)


def _ratio(got, want, mag):
    return float(((got.double() - want).abs() / (mag + 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------
# 0. Output-size formulas: a window larger than the padded input has no output (host-side size queries, no GPU)
# ---------------------------------------------------------------------------------------------------------------
def test_windows_larger_than_the_padded_input_are_refused():
    """Ho = (H + 2 pad - kh) / stride + 1 truncates toward zero in C: with kh = H + 2 pad + 1 and stride >= 2 it gives
    Ho = 1 where torch's floor gives 0 and refuses the geometry.  Both size queries must return 0 there, and the exact
    size where the window just fits (Ho = 1)."""
    L = _lib.lib()
    B, H, W, Cin, Cout = 2, 2, 3, 3, 8
    for stride in (1, 2, 3):
        for pad in (0, 1):
            for kh, kw in ((H + 2 * pad + 1, 1), (1, W + 2 * pad + 1), (H + 2 * pad + 1, W + 2 * pad + 1)):
                for bdx in (0, 1):
                    assert L.i2l_conv_f32_workspace_bytes(1, B, H, W, Cin, Cout, kh, kw, stride, pad, bdx) == 0, (kh, kw, stride, pad)
                    assert L.i2l_conv_f32_workspace_bytes(2, B, H, W, Cin, Cout, kh, kw, stride, pad, bdx) == 0, (kh, kw, stride, pad)
                for flags in (0, _lib.FLAG_RESNET_IM2COL_STEM):
                    assert L.i2l_conv_bf16_workspace_bytes(B, H, W, Cin, Cout, kh, kw, stride, pad, flags) == 0, (kh, kw, stride, pad)
            # the window fits exactly: one output row / column
            kh, kw = H + 2 * pad, W + 2 * pad
            Wo = (W + 2 * pad - 1) // stride + 1                      # with kw = 1
            for kwx, wo in ((kw, 1), (1, Wo)):
                M, Kc = B * 1 * wo, Cin * kh * kwx
                col = (M * Kc * 4 + 255) // 256 * 256
                fwd = L.i2l_conv_f32_workspace_bytes(1, B, H, W, Cin, Cout, kh, kwx, stride, pad, 0)
                bwd = L.i2l_conv_f32_workspace_bytes(1, B, H, W, Cin, Cout, kh, kwx, stride, pad, 1)
                assert fwd >= col + 256 and bwd - fwd == col, (kh, kwx, stride, pad, fwd, bwd)
                kp = (Kc + 7) // 8 * 8                                # Cin = 3: the im2col image of the bf16 path
                assert L.i2l_conv_bf16_workspace_bytes(B, H, W, Cin, Cout, kh, kwx, stride, pad, 0) == \
                    (M * kp * 2 + 255) // 256 * 256, (kh, kwx, stride, pad)


# ---------------------------------------------------------------------------------------------------------------
# 1. i2l_conv_f32_fwd / i2l_conv_f32_bwd
# ---------------------------------------------------------------------------------------------------------------
#        B   H    W    Cin   Cout k  s  p  layout
CONV_CASES = [
    (2, 25, 125, 64, 128, 3, 2, 1, "nhwc"),      # odd inputs of the stride-2 layers of a 100x500 trunk
    (2, 13, 63, 256, 512, 1, 2, 0, "nhwc"),
    (2, 7, 32, 512, 512, 3, 2, 1, "nhwc"),
    (3, 5, 9, 72, 40, 1, 1, 0, "nhwc"),          # direct: the column image is x
    (1, 1, 1, 512, 2048, 1, 1, 0, "nhwc"),       # direct, M = 1
    (2, 4, 4, 5, 7, 3, 1, 1, "nhwc"),            # Kc = 45: the fp32 kernel
    (1, 2, 3, 8, 8, 3, 2, 1, "nhwc"),            # split kernel, tiny M
    (2, 3, 5, 2048, 512, 1, 1, 0, "nhwc"),       # long K
    (4, 16, 100, 64, 64, 3, 1, 1, "nhwc"),       # large M: split-K slabs in dw
    (2, 9, 11, 3, 64, 7, 2, 3, "nchw"),          # the stem, Kc = 147
    (1, 64, 800, 3, 64, 7, 2, 3, "nchw"),
]


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _conv_operands(case, g, adversarial=None):
    B, H, W, Cin, Cout, k, s, p, layout = case
    Ho, Wo = _out_hw(H, W, k, s, p)
    x = torch.randn(B, Cin, H, W, generator=g)                              # NCHW
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    if adversarial:
        x, w = _adversarial(adversarial, x, w, 1, 1, g)
    dz = torch.randn(B, Cout, Ho, Wo, generator=g)
    return x, w, dz


def _conv_truth(case, x, w, dz):
    """float64 z, dx, dw and their magnitudes (the same operations on |operands|), NHWC / (Cout,Cin,k,k)."""
    _, _, _, _, _, k, s, p, _ = case
    xd, wd, dzd = x.double(), w.double(), dz.double()
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    z = nhwc(F.conv2d(xd, wd, stride=s, padding=p))
    zm = nhwc(F.conv2d(xd.abs(), wd.abs(), stride=s, padding=p))
    dx = nhwc(torch.nn.grad.conv2d_input(xd.shape, wd, dzd, stride=s, padding=p))
    dxm = nhwc(torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dzd.abs(), stride=s, padding=p))
    dw = torch.nn.grad.conv2d_weight(xd, wd.shape, dzd, stride=s, padding=p)
    dwm = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dzd.abs(), stride=s, padding=p)
    return z, zm, dx, dxm, dw, dwm


def _conv_args(case):
    B, H, W, Cin, Cout, k, s, p, layout = case
    return (1 if layout == "nhwc" else 2), (B, H, W, Cin, Cout, k, k, s, p)


def _conv_fwd(L, x_dev, kind, w_dev, geo, flags, ws=None, bdx=0):
    B, H, W, Cin, Cout, kh, kw, s, p = geo
    Ho, Wo = _out_hw(H, W, kh, s, p)
    nb = L.i2l_conv_f32_workspace_bytes(kind, *geo, bdx)
    assert nb > 0
    ws = _ws(nb) if ws is None else ws
    z = Out((B, Ho, Wo, Cout))
    assert L.i2l_conv_f32_fwd(x_dev.data_ptr(), kind, w_dev.data_ptr(), z.ptr(), *geo, ws.data_ptr(), nb, flags,
                              _lib.stream_ptr()) == 0
    return z.get(), ws


def _conv_bwd(L, x_dev, kind, w_dev, dz_dev, geo, flags, want_dx, want_dw, ws=None):
    B, H, W, Cin, Cout, kh, kw, s, p = geo
    nb = L.i2l_conv_f32_workspace_bytes(kind, *geo, 1 if want_dx else 0)
    assert nb > 0
    ws = _ws(nb) if ws is None else ws
    dx = Out((B, H, W, Cin)) if want_dx else None
    dw = Out((Cout, Cin, kh, kw)) if want_dw else None
    assert L.i2l_conv_f32_bwd(x_dev.data_ptr(), kind, w_dev.data_ptr(), dz_dev.data_ptr(), dx.ptr() if dx else None,
                              dw.ptr() if dw else None, *geo, ws.data_ptr(), nb, flags, _lib.stream_ptr()) == 0
    return (dx.get() if dx else None), (dw.get() if dw else None)


def _check_conv_case(case, g, worst, adversarial=None):
    L = _lib.lib()
    x, w, dz = _conv_operands(case, g, adversarial)
    z64, zm, dx64, dxm, dw64, dwm = _conv_truth(case, x, w, dz)
    kind, geo = _conv_args(case)
    x_dev = _dev(x.permute(0, 2, 3, 1) if kind == 1 else x)
    w_dev, dz_dev = _dev(w), _dev(dz.permute(0, 2, 3, 1))
    tag = adversarial or "randn"
    for flags in (0, _lib.FLAG_EXACT_FP32):
        z, _ = _conv_fwd(L, x_dev, kind, w_dev, geo, flags)
        r = _ratio(z, z64, zm)
        worst[("fwd", tag, flags)] = max(worst.get(("fwd", tag, flags), 0.0), r)
        assert r <= 2.0 ** -20, (case, flags, "z", r)
        modes = [(False, True)] if kind == 2 else [(False, True), (True, False), (True, True)]
        for want_dx, want_dw in modes:
            dx, dw = _conv_bwd(L, x_dev, kind, w_dev, dz_dev, geo, flags, want_dx, want_dw)
            if dx is not None:
                r = _ratio(dx, dx64, dxm)
                worst[("dx", tag, flags)] = max(worst.get(("dx", tag, flags), 0.0), r)
                assert r <= 2.0 ** -20, (case, flags, want_dw, "dx", r)
            if dw is not None:
                r = _ratio(dw, dw64, dwm)
                worst[("dw", tag, flags)] = max(worst.get(("dw", tag, flags), 0.0), r)
                assert r <= 2.0 ** -20, (case, flags, want_dx, "dw", r)


@pytest.mark.gpu
def test_conv_f32_odd_shapes_vs_float64():
    """z, dx and dw of every case, split-bf16 and exact-fp32 kernels, dw only / dx only / both, within
    2^-20 of the float64 value of the same operation on the absolute operands."""
    g = torch.Generator().manual_seed(101)
    worst = {}
    for case in CONV_CASES:
        _check_conv_case(case, g, worst)
    # 2^+-60 dynamic range inside one reduction (x and w scaled inversely per input channel)
    _check_conv_case((2, 9, 11, 64, 96, 3, 2, 1, "nhwc"), g, worst, adversarial="range_2^+-60")
    for (what, tag, flags), v in worst.items():
        record(f"train prims conv_f32 {what} {tag} flags={flags} [err / float64 magnitude]", v)


@pytest.mark.gpu
def test_conv_f32_col_ready_and_gradient_holes():
    """(a) dw (and dx) of a backward call that reuses the forward call's column image (FLAG_CONV_COL_READY) are
    bit-identical to a call on a fresh workspace; (b) a 1x1 / stride 2 conv on odd H, W reads no pixel of an odd row or
    column, and its dx there is exactly 0."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(102)
    for case in [c for c in CONV_CASES if not (c[5] == 1 and c[6] == 1 and c[8] == "nhwc")]:
        x, w, dz = _conv_operands(case, g)
        kind, geo = _conv_args(case)
        x_dev = _dev(x.permute(0, 2, 3, 1) if kind == 1 else x)
        w_dev, dz_dev = _dev(w), _dev(dz.permute(0, 2, 3, 1))
        want_dx = kind == 1
        for flags in (0, _lib.FLAG_EXACT_FP32):
            _, ws = _conv_fwd(L, x_dev, kind, w_dev, geo, flags, bdx=1 if want_dx else 0)
            dx_r, dw_r = _conv_bwd(L, x_dev, kind, w_dev, dz_dev, geo, flags | _lib.FLAG_CONV_COL_READY, want_dx, True, ws=ws)
            dx_f, dw_f = _conv_bwd(L, x_dev, kind, w_dev, dz_dev, geo, flags, want_dx, True)
            assert torch.equal(dw_r, dw_f), (case, flags)
            if want_dx:
                assert torch.equal(dx_r, dx_f), (case, flags)
    for case in [(2, 13, 63, 256, 512, 1, 2, 0, "nhwc"), (1, 5, 7, 8, 16, 1, 2, 0, "nhwc")]:
        x, w, dz = _conv_operands(case, g)
        _, geo = _conv_args(case)
        for flags in (0, _lib.FLAG_EXACT_FP32):
            dx, _ = _conv_bwd(L, _dev(x.permute(0, 2, 3, 1)), 1, _dev(w), _dev(dz.permute(0, 2, 3, 1)), geo, flags, True, False)
            assert not torch.isnan(dx).any()
            assert (dx[:, 1::2] == 0).all() and (dx[:, :, 1::2] == 0).all(), (case, flags)
            assert (dx[:, ::2, ::2] != 0).any()


@pytest.mark.gpu
def test_conv_f32_refusals():
    L = _lib.lib()
    B, H, W, Cin, Cout, k, s, p = 1, 5, 6, 8, 8, 3, 2, 1
    geo = (B, H, W, Cin, Cout, k, k, s, p)
    x, w, z, dx, dw = (torch.zeros(n, device=DEV) for n in (B * H * W * Cin, Cout * Cin * 9, 4096, B * H * W * Cin, Cout * Cin * 9))
    st = _lib.stream_ptr()
    nb = L.i2l_conv_f32_workspace_bytes(1, *geo, 1)
    ws = _ws(nb)
    for kind in (0, 3):
        assert L.i2l_conv_f32_workspace_bytes(kind, *geo, 1) == 0
        assert L.i2l_conv_f32_fwd(x.data_ptr(), kind, w.data_ptr(), z.data_ptr(), *geo, ws.data_ptr(), nb, 0, st) == ERR_ARG
        assert L.i2l_conv_f32_bwd(x.data_ptr(), kind, w.data_ptr(), z.data_ptr(), dx.data_ptr(), dw.data_ptr(), *geo,
                                  ws.data_ptr(), nb, 0, st) == ERR_ARG
    assert L.i2l_im2col_f32(x.data_ptr(), 3, B, H, W, Cin, k, k, s, p, z.data_ptr(), st) == ERR_ARG
    nb2 = L.i2l_conv_f32_workspace_bytes(2, *geo, 1)
    assert L.i2l_conv_f32_bwd(x.data_ptr(), 2, w.data_ptr(), z.data_ptr(), dx.data_ptr(), None, *geo, ws.data_ptr(), nb2, 0,
                              st) == ERR_UNSUPPORTED
    for bdx in (0, 1):
        short = L.i2l_conv_f32_workspace_bytes(1, *geo, bdx) - 1
        if bdx == 0:
            assert L.i2l_conv_f32_fwd(x.data_ptr(), 1, w.data_ptr(), z.data_ptr(), *geo, ws.data_ptr(), short, 0, st) == ERR_WORKSPACE
            assert L.i2l_conv_f32_bwd(x.data_ptr(), 1, w.data_ptr(), z.data_ptr(), None, dw.data_ptr(), *geo, ws.data_ptr(),
                                      short, 0, st) == ERR_WORKSPACE
        else:
            assert L.i2l_conv_f32_bwd(x.data_ptr(), 1, w.data_ptr(), z.data_ptr(), dx.data_ptr(), dw.data_ptr(), *geo,
                                      ws.data_ptr(), short, 0, st) == ERR_WORKSPACE
    # windows larger than the padded input: refused before any launch (see the host-side test above)
    packed = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for stride in (1, 2, 3):
        for pad in (0, 1):
            kh = H + 2 * pad + 1
            bad = (B, H, W, Cin, Cout, kh, 1, stride, pad)
            assert L.i2l_conv_f32_fwd(x.data_ptr(), 1, w.data_ptr(), z.data_ptr(), *bad, ws.data_ptr(), nb, 0, st) == ERR_ARG
            assert L.i2l_conv_f32_bwd(x.data_ptr(), 1, w.data_ptr(), z.data_ptr(), dx.data_ptr(), dw.data_ptr(), *bad,
                                      ws.data_ptr(), nb, 0, st) == ERR_ARG
            assert L.i2l_im2col_f32(x.data_ptr(), 1, B, H, W, Cin, kh, 1, stride, pad, z.data_ptr(), st) == ERR_ARG
            assert L.i2l_col2im_f32(z.data_ptr(), B, H, W, Cin, kh, 1, stride, pad, dx.data_ptr(), 0, st) == ERR_ARG
            assert L.i2l_conv_bn_act_bf16_fwd(x.data_ptr(), 0, packed.data_ptr(), None, z.data_ptr(), B, H, W, Cin, Cout, kh,
                                              1, stride, pad, 1, ws.data_ptr(), nb, 0, st) == ERR_ARG
    torch.cuda.synchronize()
    assert (z == 0).all() and (dx == 0).all() and (dw == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. i2l_bn_train_fwd_f32 / i2l_bn_train_bwd_f32
# ---------------------------------------------------------------------------------------------------------------
#          M       C     residual relu running momentum
BN_CASES = [
    (1, 64, True, True, True, 0.1),
    (2, 24, False, True, True, 1.0 / 3.0),
    (127, 8, True, False, False, 0.1),
    (128, 2048, False, False, True, 0.1),
    (129, 24, True, True, True, 1.0 / 3.0),
    (385, 4096, True, True, True, 0.1),
    (2500, 64, False, True, False, 0.1),
    (102400, 64, True, True, True, 1.0 / 3.0),
]


def _bn_z(M, C, g):
    """fp32 z (M, C): per-channel spreads 2^-4 .. 2^4 and means up to 10^4 spreads; channel 1 has an outlier in row 0
    (the shift of the one-pass variance), channel 3 a large mean AND a row-0 outlier."""
    spread = 2.0 ** (torch.rand(C, generator=g, dtype=torch.float64) * 8 - 4)
    mean = torch.randn(C, generator=g, dtype=torch.float64) * spread * 3
    mean[::4] = spread[::4] * 1e4 * torch.sign(torch.randn(len(mean[::4]), generator=g, dtype=torch.float64))
    z = mean + spread * torch.randn(M, C, generator=g, dtype=torch.float64)
    if M > 1:
        z[0, 1] = mean[1] + 1e3 * spread[1]
        z[0, 3] = mean[3] - 3e3 * spread[3]
    return z.float()


def _bn_forward(L, z_dev, res_dev, gamma_dev, beta_dev, rm, rv, momentum, eps, relu, M, C):
    y, sm, si = Out((M, C)), Out((C,)), Out((C,))
    nb = L.i2l_bn_train_workspace_bytes(M, C)
    ws = _ws(nb)
    assert L.i2l_bn_train_fwd_f32(z_dev.data_ptr(), None if res_dev is None else res_dev.data_ptr(), gamma_dev.data_ptr(),
                                  beta_dev.data_ptr(), rm.ptr() if rm else None, rv.ptr() if rv else None, momentum, eps,
                                  1 if relu else 0, y.ptr(), sm.ptr(), si.ptr(), M, C, ws.data_ptr(), nb,
                                  _lib.stream_ptr()) == 0
    return y.get(), sm.get(), si.get()


@pytest.mark.gpu
def test_bn_train_forward_vs_float64():
    """Batch mean, biased variance (recovered from invstd), y and the running statistics (momentum, UNBIASED
    variance) against float64 statistics of the same fp32 z.  M = 1 is the kernel's own definition (torch refuses it
    in training): variance 0, running variance updated with 0."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(201)
    eps = 1e-5
    worst = {}
    for (M, C, use_res, relu, running, momentum) in BN_CASES:
        z = _bn_z(M, C, g)
        gamma = (torch.rand(C, generator=g) + 0.25) * torch.sign(torch.randn(C, generator=g))
        beta = torch.randn(C, generator=g)
        res = torch.randn(M, C, generator=g) if use_res else None
        rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        rm, rv = (Out((C,), init=rm0), Out((C,), init=rv0)) if running else (None, None)
        y, mean, invstd = _bn_forward(L, _dev(z), None if res is None else _dev(res), _dev(gamma), _dev(beta), rm, rv,
                                      momentum, eps, relu, M, C)
        zd = z.double()
        mu = zd.mean(0)
        var = zd.var(0, unbiased=False)
        sig = var.sqrt()
        r_mean = _ratio(mean, mu, mu.abs() + sig)
        assert r_mean <= 2.0 ** -21, (M, C, "mean", r_mean)
        var_k = 1.0 / invstd.double() ** 2 - eps
        r_var = _ratio(var_k, var, var + eps)
        assert r_var <= 2.0 ** -20, (M, C, "var", r_var)
        inv64 = 1.0 / (var + eps).sqrt()
        pre = gamma.double() * (zd - mu) * inv64 + beta.double()
        if res is not None:
            pre = pre + res.double()
        want = pre.relu() if relu else pre
        mag = gamma.double().abs() * inv64 * (zd.abs() + mu.abs()) + beta.double().abs()
        if res is not None:
            mag = mag + res.double().abs()
        r_y = _ratio(y, want, mag)
        assert r_y <= 2.0 ** -20, (M, C, "y", r_y)
        if M == 1:                                   # variance exactly 0: invstd = 1 / sqrt(eps)
            assert torch.equal(invstd, torch.full((C,), 1.0 / math.sqrt(float(torch.tensor(eps))), dtype=torch.float64).float())
            assert (y == (beta + (res[0] if res is not None else 0)).clamp(min=0 if relu else -math.inf)).all()
        r_run = 0.0
        if running:
            unbiased = var * M / (M - 1) if M > 1 else var
            for got, old, new in ((rm.get(), rm0.double(), mu), (rv.get(), rv0.double(), unbiased)):
                want_r = (1 - momentum) * old + momentum * new
                r_run = max(r_run, _ratio(got, want_r, (1 - momentum) * old.abs() + momentum * new.abs()))
            assert r_run <= 2.0 ** -20, (M, C, "running", r_run)
        for k, v in (("mean [/(|mu|+sigma)]", r_mean), ("var [/(var+eps)]", r_var), ("y", r_y), ("running stats", r_run)):
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        record(f"train prims bn_train_fwd {k}", v)


@pytest.mark.gpu
def test_bn_train_backward_vs_float64():
    """dz, dgamma, dbeta and dres from the kernel's own saved mean / invstd (promoted to float64): dz within
    2^-16 |gamma| invstd (|g| + mean|g| + |xhat| mean|g xhat|), dgamma / dbeta within 2^-16 of sum|g xhat| / sum|g|,
    dres exactly g (or old + g); dgamma, dbeta and dres may each be NULL without changing dz."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(202)
    eps = 1e-5
    worst = {}
    for (M, C, use_res, relu, running, momentum) in BN_CASES:
        z = _bn_z(M, C, g)
        gamma = (torch.rand(C, generator=g) + 0.25) * torch.sign(torch.randn(C, generator=g))
        beta = torch.randn(C, generator=g) * 0.5
        z_dev, gamma_dev = _dev(z), _dev(gamma)
        y, mean, invstd = _bn_forward(L, z_dev, None, gamma_dev, _dev(beta), None, None, momentum, eps, relu, M, C)
        dy = torch.randn(M, C, generator=g)
        gm = dy.double() * (y > 0) if relu else dy.double()
        mu, inv = mean.double(), invstd.double()
        xh = (z.double() - mu) * inv
        mg, mgx = gm.mean(0), (gm * xh).mean(0)
        gam = gamma.double()
        dz64 = gam * inv * (gm - mg - xh * mgx)
        dz_mag = gam.abs() * inv * (gm.abs() + gm.abs().mean(0) + xh.abs() * (gm * xh).abs().mean(0))
        old = torch.randint(-8, 9, (M, C), generator=g).float()
        y_dev, dy_dev, mean_dev, inv_dev = _dev(y), _dev(dy), _dev(mean), _dev(invstd)
        nb = L.i2l_bn_train_workspace_bytes(M, C)
        dz_ref = None
        for has_dg, has_db, has_dres, acc in ((True, True, True, 0), (True, True, True, 1), (False, True, False, 0),
                                              (True, False, True, 1), (False, False, False, 0)):
            dz, dgam, dbet = Out((M, C)), Out((C,)) if has_dg else None, Out((C,)) if has_db else None
            dres = Out((M, C), init=old) if acc else (Out((M, C)) if has_dres else None)
            ws = _ws(nb)
            assert L.i2l_bn_train_bwd_f32(dy_dev.data_ptr(), y_dev.data_ptr() if relu else None, z_dev.data_ptr(),
                                          gamma_dev.data_ptr(), mean_dev.data_ptr(), inv_dev.data_ptr(), dz.ptr(),
                                          dgam.ptr() if dgam else None, dbet.ptr() if dbet else None,
                                          dres.ptr() if dres else None, acc, M, C, ws.data_ptr(), nb, _lib.stream_ptr()) == 0
            got = dz.get()
            if dz_ref is None:
                dz_ref = got
                r = _ratio(got, dz64, dz_mag)
                worst["dz"] = max(worst.get("dz", 0.0), r)
                assert r <= 2.0 ** -16, (M, C, "dz", r)
            else:
                assert torch.equal(got, dz_ref), (M, C, has_dg, has_db, has_dres, acc)
            if dgam is not None:
                r = _ratio(dgam.get(), (gm * xh).sum(0), (gm * xh).abs().sum(0))
                worst["dgamma"] = max(worst.get("dgamma", 0.0), r)
                assert r <= 2.0 ** -16, (M, C, "dgamma", r)
            if dbet is not None:
                r = _ratio(dbet.get(), gm.sum(0), gm.abs().sum(0))
                worst["dbeta"] = max(worst.get("dbeta", 0.0), r)
                assert r <= 2.0 ** -16, (M, C, "dbeta", r)
            if dres is not None:
                g32 = gm.float()
                assert torch.equal(dres.get(), old + g32 if acc else g32), (M, C, "dres", acc)
    for k, v in worst.items():
        record(f"train prims bn_train_bwd {k} [err / magnitude]", v)


@pytest.mark.gpu
def test_bn_train_refusals():
    L = _lib.lib()
    M, C = 16, 12
    t = torch.zeros(M * 16, device=DEV)
    p = t.data_ptr()
    ws = _ws(1 << 16)
    st = _lib.stream_ptr()
    assert L.i2l_bn_train_fwd_f32(p, None, p, p, None, None, 0.1, 1e-5, 1, p, p, p, M, C, ws.data_ptr(), 1 << 16, st) == ERR_UNSUPPORTED
    assert L.i2l_bn_train_bwd_f32(p, p, p, p, p, p, p, p, p, p, 0, M, C, ws.data_ptr(), 1 << 16, st) == ERR_UNSUPPORTED
    C = 16
    for rm, rv in ((p, None), (None, p)):
        assert L.i2l_bn_train_fwd_f32(p, None, p, p, rm, rv, 0.1, 1e-5, 1, p, p, p, M, C, ws.data_ptr(), 1 << 16, st) == ERR_ARG
    torch.cuda.synchronize()
    assert (t == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. Pools
# ---------------------------------------------------------------------------------------------------------------
POOL_HW = [1, 2, 3, 5, 8, 13]


def _pool_input(B, H, W, C, g):
    """NHWC fp32 quantised to a few values (ties inside windows), ReLU zeros and some -inf entries."""
    x = torch.randint(-3, 4, (B, H, W, C), generator=g).float().relu()
    x[torch.rand(B, H, W, C, generator=g) < 0.1] = -math.inf
    return x


@pytest.mark.gpu
def test_maxpool_f32_forward_and_backward_exact():
    """Forward equals CPU max_pool2d(3, 2, 1) exactly; backward (integer dy: sums exact in any order) equals CPU ATen's
    backward, where the FIRST maximum of a window in row-major order takes the gradient."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(301)
    st = _lib.stream_ptr()
    combos = [(1, 4), (3, 12), (1, 64), (3, 4), (1, 12), (3, 64)]
    n = 0
    for H in POOL_HW:
        for W in POOL_HW:
            B, C = combos[n % len(combos)]
            n += 1
            x = _pool_input(B, H, W, C, g)
            xc = x.permute(0, 3, 1, 2).contiguous()
            want = F.max_pool2d(xc, 3, 2, 1).permute(0, 2, 3, 1)
            Ho, Wo = want.shape[1:3]
            y = Out((B, Ho, Wo, C))
            assert L.i2l_maxpool3x3s2_f32_fwd(_dev(x).data_ptr(), y.ptr(), B, H, W, C, st) == 0
            assert torch.equal(y.get(), want), (B, H, W, C)
            for Cb in (C, 3):
                xb = x if Cb == C else _pool_input(B, H, W, Cb, g)
                xcb = xb.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
                yb = F.max_pool2d(xcb, 3, 2, 1)
                dy = torch.randint(-64, 65, yb.shape, generator=g).float()
                yb.backward(dy)
                want_dx = xcb.grad.permute(0, 2, 3, 1)
                dx = Out((B, H, W, Cb))
                assert L.i2l_maxpool3x3s2_f32_bwd(_dev(xb).data_ptr(), _dev(dy.permute(0, 2, 3, 1)).data_ptr(), dx.ptr(),
                                                  B, H, W, Cb, st) == 0
                assert torch.equal(dx.get(), want_dx), (B, H, W, Cb)
    x = torch.zeros(1, 4, 4, 3, device=DEV)
    y = torch.zeros(64, device=DEV)
    assert L.i2l_maxpool3x3s2_f32_fwd(x.data_ptr(), y.data_ptr(), 1, 4, 4, 3, st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == 0).all()


@pytest.mark.gpu
def test_maxpool_bf16_forward_exact():
    L = _lib.lib()
    g = torch.Generator().manual_seed(302)
    st = _lib.stream_ptr()
    for H in POOL_HW:
        for W in POOL_HW:
            for B, C in ((1, 8), (3, 64)):
                x = (_pool_input(B, H, W, C, g) + torch.randn(B, H, W, C, generator=g) * 0.01).to(torch.bfloat16)
                want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(torch.bfloat16)
                y = Out(tuple(want.shape), dtype=torch.bfloat16)
                assert L.i2l_maxpool3x3s2_bf16_fwd(_dev(x).data_ptr(), y.ptr(), B, H, W, C, st) == 0
                assert torch.equal(y.get(), want), (B, H, W, C)
    x = torch.zeros(1, 4, 4, 12, dtype=torch.bfloat16, device=DEV)
    y = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    assert L.i2l_maxpool3x3s2_bf16_fwd(x.data_ptr(), y.data_ptr(), 1, 4, 4, 12, st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == 0).all()


AVG_HW = [(1, 1), (1, 3), (5, 10), (14, 16), (20, 20)]          # HW = 1, 3, 50, 224, 400


@pytest.mark.gpu
def test_global_avgpool_vs_float64():
    """fp32 pool (C % 4 == 0) and bf16 pool (vectorised C % 8 == 0, scalar otherwise) within HW 2^-24 mean|x| of the
    float64 mean; the fp32 backward is exactly dfeat * fp32(1 / HW) at every position."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(303)
    st = _lib.stream_ptr()
    worst = {}
    for H, W in AVG_HW:
        HW = H * W
        for kind, C in (("f32", 4), ("f32", 64), ("bf16", 8), ("bf16", 64), ("bf16", 3), ("bf16", 12)):
            B = 3
            x = torch.randn(B, H, W, C, generator=g) + 0.5
            if kind == "bf16":
                x = x.to(torch.bfloat16)
            xd = x.double().reshape(B, HW, C)
            want, mag = xd.mean(1), xd.abs().mean(1)
            y = Out((B, C))
            fn = L.i2l_global_avgpool_f32_fwd if kind == "f32" else L.i2l_global_avgpool_bf16_fwd
            assert fn(_dev(x).data_ptr(), y.ptr(), B, H, W, C, st) == 0
            r = _ratio(y.get(), want, HW * mag)
            key = f"{kind} {'scalar' if kind == 'bf16' and C % 8 else 'vector'}"
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 2.0 ** -24, (kind, B, H, W, C, r)
        for C in (3, 64):
            dfeat = torch.randn(2, C, generator=g)
            dx = Out((2, H, W, C))
            assert L.i2l_global_avgpool_bwd_f32(_dev(dfeat).data_ptr(), dx.ptr(), 2, H, W, C, st) == 0
            inv = torch.tensor(1.0, dtype=torch.float32) / HW
            assert torch.equal(dx.get(), (dfeat * inv)[:, None, None, :].expand(2, H, W, C)), (H, W, C)
    x = torch.zeros(1, 2, 2, 3, device=DEV)
    y = torch.zeros(64, device=DEV)
    assert L.i2l_global_avgpool_f32_fwd(x.data_ptr(), y.data_ptr(), 1, 2, 2, 3, st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == 0).all()
    for k, v in worst.items():
        record(f"train prims global avgpool {k} [err / (HW 2^-24 mean|x|)]", v * 2.0 ** 24)


# ---------------------------------------------------------------------------------------------------------------
# 4. i2l_im2col_f32 / i2l_col2im_f32
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_im2col_and_col2im_exact():
    """im2col equals unfold in the weight tensor's (ci, ky, kx) column order for NHWC bf16, NHWC fp32 and NCHW fp32
    input; col2im of an integer-valued column gradient equals fold, overwriting (accumulate 0) or adding to integer
    content (accumulate 1)."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(401)
    st = _lib.stream_ptr()
    for (B, H, W, Cin, _, k, s, p, layout) in CONV_CASES:
        Ho, Wo = _out_hw(H, W, k, s, p)
        M, Kc = B * Ho * Wo, Cin * k * k
        x = torch.randn(B, Cin, H, W, generator=g)
        for kind in ((0, 1) if layout == "nhwc" else (2,)):
            xs = x.to(torch.bfloat16).float() if kind == 0 else x
            want = F.unfold(xs, k, padding=p, stride=s).transpose(1, 2).reshape(M, Kc)
            src = x.permute(0, 2, 3, 1).to(torch.bfloat16) if kind == 0 else (x.permute(0, 2, 3, 1) if kind == 1 else x)
            col = Out((M, Kc))
            assert L.i2l_im2col_f32(_dev(src).data_ptr(), kind, B, H, W, Cin, k, k, s, p, col.ptr(), st) == 0
            assert torch.equal(col.get(), want), (B, H, W, Cin, k, s, p, kind)
        dcol = torch.randint(-8, 9, (M, Kc), generator=g).float()
        folded = F.fold(dcol.reshape(B, Ho * Wo, Kc).transpose(1, 2), (H, W), k, padding=p, stride=s).permute(0, 2, 3, 1)
        old = torch.randint(-100, 101, (B, H, W, Cin), generator=g).float()
        for acc in (0, 1):
            dx = Out((B, H, W, Cin), init=old) if acc else Out((B, H, W, Cin))
            assert L.i2l_col2im_f32(_dev(dcol).data_ptr(), B, H, W, Cin, k, k, s, p, dx.ptr(), acc, st) == 0
            assert torch.equal(dx.get(), old + folded if acc else folded), (B, H, W, Cin, k, s, p, acc)


# ---------------------------------------------------------------------------------------------------------------
# 5. i2l_linear_bias_act_bwd at odd shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_linear_bwd_odd_shapes_vs_float64():
    """dx and dw within 2^-20 of the float64 sums of |operand| products, db within 2^-20 of sum |g|, with ReLU on and
    off, dx or db NULL, both kernels.  With ReLU the gradient at y == 0 is 10^6: a gate that passed any of it fails."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(501)
    st = _lib.stream_ptr()
    worst = {}
    for (M, K, N) in [(1, 7, 3), (5, 33, 70), (67, 130, 65), (4, 4096, 33), (256, 1024, 96), (130, 2056, 70),
                      (256, 40960, 256), (3, 8192, 200)]:
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g)
        y = torch.relu(x @ w.t() + b)
        y[:, ::5] = 0.0                                  # exact zeros in every row, also for the relu = 0 calls
        dy = torch.randn(M, N, generator=g)
        x_dev, w_dev, y_dev = _dev(x), _dev(w), _dev(y)
        nb = L.i2l_linear_bwd_workspace_bytes(M, K, N)
        for relu in (0, 1):
            dyr = torch.where(y > 0, dy, torch.full_like(dy, 1e6)) if relu else dy
            gm = dyr.double() * (y > 0) if relu else dyr.double()
            dx64, dxm = gm @ w.double(), gm.abs() @ w.double().abs()
            dw64, dwm = gm.t() @ x.double(), gm.abs().t() @ x.double().abs()
            db64, dbm = gm.sum(0), gm.abs().sum(0)
            dy_dev = _dev(dyr)
            for flags in (0, _lib.FLAG_EXACT_FP32):
                for want_dx, want_db in ((True, True), (False, True), (True, False)):
                    dx = Out((M, K)) if want_dx else None
                    dw = Out((N, K))
                    db = Out((N,)) if want_db else None
                    ws = _ws(nb)
                    assert L.i2l_linear_bias_act_bwd(x_dev.data_ptr(), w_dev.data_ptr(), y_dev.data_ptr(), dy_dev.data_ptr(),
                                                     dx.ptr() if dx else None, dw.ptr(), db.ptr() if db else None, M, K, N,
                                                     relu, ws.data_ptr(), nb, flags, None, st) == 0
                    for name, out, want, mag in (("dx", dx, dx64, dxm), ("dw", dw, dw64, dwm), ("db", db, db64, dbm)):
                        if out is None:
                            continue
                        r = _ratio(out.get(), want, mag)
                        worst[(name, flags)] = max(worst.get((name, flags), 0.0), r)
                        assert r <= 2.0 ** -20, (M, K, N, relu, flags, want_dx, want_db, name, r)
    for (name, flags), v in worst.items():
        record(f"train prims linear_bwd {name} flags={flags} [err / float64 magnitude]", v)
    # The magnitude bound above does not see a lost product of the six-product split scheme (zero-mean operands: 0.05 to
    # 0.4 of the bound, tests/test_linear_fwd_vs_float64.py).  Selection operands do: every dx and dw element is ONE
    # product, exact in fp32, so both kernels must return the float64 value bit for bit.  dx sums over n and dw over m,
    # so the one-hot operand holds one value per COLUMN k (w and x), or per row and column (dy).  A: dy dense randn
    # (a lost a1 b0 / a2 b0 shows), w and x one-hot +-2^e.  B: dy one-hot, w and x dense (a0 b1 / a0 b2).  C: every value
    # +-2^e (1 + 2^-9), w and x one-hot: the product's 2^-18 bit is the a1 b1 term.  M = 70: dw's reduction runs on the
    # split kernel's M/N-contiguous instantiation; M = 5: on the fp32 kernel.  dx (reduction N = 72) is split in both.
    def pow2(*shape):
        e = torch.randint(-6, 7, shape, generator=g).double()
        return ((torch.randint(0, 2, shape, generator=g).double() * 2 - 1) * 2.0 ** e).float()

    def one_per_column(rows, K, val):
        m = torch.zeros(rows, K)
        m[(7 * torch.arange(K)) % rows, torch.arange(K)] = val
        return m

    for (M, K, N) in [(70, 130, 72), (5, 33, 72)]:
        assert M <= N and math.gcd(7, N) == 1            # dy's one-hot rows sit in distinct columns
        nb = L.i2l_linear_bwd_workspace_bytes(M, K, N)
        for fam in "ABC":
            if fam == "A":
                dy, w, x = torch.randn(M, N, generator=g), one_per_column(N, K, pow2(K)), one_per_column(M, K, pow2(K))
            elif fam == "B":
                dy = torch.zeros(M, N)
                dy[torch.arange(M), (7 * torch.arange(M)) % N] = pow2(M)
                w, x = torch.randn(N, K, generator=g), torch.randn(M, K, generator=g)
            else:
                c = 1 + 2.0 ** -9
                dy = (pow2(M, N).double() * c).float()
                w, x = one_per_column(N, K, (pow2(K).double() * c).float()), one_per_column(M, K, (pow2(K).double() * c).float())
            dx64, dw64 = dy.double() @ w.double(), dy.double().t() @ x.double()
            assert torch.equal(dx64.float().double(), dx64) and torch.equal(dw64.float().double(), dw64)
            assert float(dx64.abs().max()) > 0 and float(dw64.abs().max()) > 0
            x_dev, w_dev, dy_dev = _dev(x), _dev(w), _dev(dy)
            for flags in (0, _lib.FLAG_EXACT_FP32):
                dx, dw, ws = Out((M, K)), Out((N, K)), _ws(nb)
                assert L.i2l_linear_bias_act_bwd(x_dev.data_ptr(), w_dev.data_ptr(), None, dy_dev.data_ptr(), dx.ptr(),
                                                 dw.ptr(), None, M, K, N, 0, ws.data_ptr(), nb, flags, None, st) == 0
                assert torch.equal(dx.get(), dx64.float()), ("selection", fam, M, K, N, flags, "dx")
                assert torch.equal(dw.get(), dw64.float()), ("selection", fam, M, K, N, flags, "dw")
