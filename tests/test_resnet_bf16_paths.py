"""The bf16 ResNet trunk's conv kernels (csrc/resnet.hip, resnet_patch.inc.h, resnet_join.inc.h) through the C ABI only --
i2l_conv_bn_act_bf16_fwd and i2l_bottleneck_join_bf16_fwd -- on every dispatch path, against float64.

A. Interval model.  Everything in float64 from exactly the operands the kernel sees (x and w rounded to bf16 to nearest
even, the BatchNorm inputs as fp32):
    scale = gamma / sqrt(var + eps),  bias = beta - mean * scale,  u = scale * conv64(x, w) + bias
    delta = 2^-21 * (|scale| * conv64(|x|, |w|) + |beta| + |mean * scale|)
(the project's class bound for an fp32 chain, test_bf16x3_adversarial_operands; it also absorbs the fp32 rounding of scale
and bias and a fused or unfused multiply-add in the epilogue),
    lo = rne_bf16(u - delta),  hi = rne_bf16(u + delta)        rne_bf16: float64 -> 8 significant bits in ONE rounding
    f(t) = relu(t) without a residual (ReLU before the single rounding)
    f(t) = bf16_rne(relu(fp32(t) + fp32(r))) with one (the kernels round the scaled tile, then add in fp32)
and the assertion is f(lo) <= got <= f(hi) for every element: bit-equality wherever f(lo) == f(hi), which an unmarked
test holds to at least 95 % of the elements of every case.

B. Exact model.  Integer x and w ([-4, 4] from K = 576, [-16, 16] below) and a BatchNorm that folds exactly (var 3, eps 1,
mean 0, gamma in {1, 2, 4}, integer beta): every partial sum is an integer below 2^24 whatever the summation order, so the
output must equal f(rne_bf16(u)) on every path, relu 0 and 1.  Unmarked tests hold every case to 2 * max(mag) < 2^24 and
to at least 1 % of its non-zero outputs sitting exactly on a bf16 midpoint (ties to even).

C. Part 0 RESTATES the entry's dispatch in Python (stem, im2col fallbacks, direct / implicit, short_k, the tile width and
its balance rule, ring_depth, patch_plan and its key, the flags); an unmarked test maps every (case, flags) pair below to a
kernel instance and asserts that together they reach every instance some shape can select.  IT MUST BE EDITED TOGETHER WITH
resnet.hip AND resnet_patch.inc.h: a changed threshold there silently moves a case to another kernel otherwise.

D. The join: y by model A with the residual, z by model A applied to the y the kernel returned; model B on both.

Outputs start as NaN, workspaces are exactly the size the query returns; the worst (got - f(rne(u))) / ulp of every kernel
family is record()ed into parity_errors.json."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import record
from img2latex_amd import _lib
from test_hip_parity import BF16_CONV_CASES

NO_RING, IM2COL_STEM = _lib.FLAG_RESNET_NO_RING, _lib.FLAG_RESNET_IM2COL_STEM
WIDE, NO_PATCH = _lib.FLAG_RESNET_WIDE_TILES, _lib.FLAG_RESNET_NO_PATCH
DEPTH, SHAPE = _lib.flag_resnet_ring_depth, _lib.flag_resnet_patch_shape
DEV = "cuda"
DELTA = 2.0 ** -21


# ---------------------------------------------------------------------------------------------------------------
# 0. The dispatch of i2l_conv_bn_act_bf16_fwd, restated.  A case is (B, H, W, Cin, Cout, k, stride, pad, residual, nchw fp32)
# ---------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def out_hw(case):
    _, H, W, _, _, k, s, pd, _, _ = case
    return (H + 2 * pd - k) // s + 1, (W + 2 * pd - k) // s + 1


PATCH_SHAPES = [(1, 4, 5, 1), (1, 4, 3, 1), (2, 2, 2, 2), (2, 2, 5, 1), (2, 2, 4, 1)]       # (wm, wn, mtw, ntw)
# launch_patch's switch: (shape index, nlpt, nsw)
PATCH_INSTANCES = [(0, 4, 6), (0, 8, 4), (1, 4, 6), (1, 8, 4), (2, 4, 6), (2, 8, 4), (3, 4, 6), (3, 8, 4), (3, 12, 4),
                   (4, 8, 4), (4, 12, 4)]


def patch_shape_plan(i, W):
    """The (R, nlpt, nsw) patch_plan computes for shape i at width W, or None where it skips the shape."""
    wm, wn, mtw, ntw = PATCH_SHAPES[i]
    PT, BN = 32 * wm * mtw, 32 * wn * ntw
    if W > PT:
        return None
    R = PT // W
    need = ((R + 2) * (W + 2) * 64 + 64 + 4095) // 4096
    nlpt = 4 if need <= 4 else 8 if need <= 8 else 12 if need <= 12 else 0
    if not nlpt or (nlpt == 12 and BN != 64) or (nlpt == 4 and mtw == 4):
        return None
    nsw = 6 if 6 * BN * 64 + 2 * nlpt * 4096 <= 80 * 1024 else 4
    return R, nlpt, nsw


def patch_plan(M, H, W, Cin, Cout, force, n_cu=256):
    """resnet_patch.inc.h patch_plan: (shape index, R, nlpt, nsw) or None."""
    if H < 1 or W < 1 or Cin % 32 or Cout % 64 or M * Cin > 0x7fffffff or M * Cout > 0x7fffffff:
        return None
    if force == 0 and Cin > 128:
        return None
    G = M // W
    best, best_cost, best_tiles = None, 0, 0
    for i, (wm, wn, mtw, ntw) in enumerate(PATCH_SHAPES):
        if force > 0 and i != force - 1:
            continue
        BN = 32 * wn * ntw
        p = patch_shape_plan(i, W)
        if Cout % BN or p is None:
            continue
        R, nlpt, nsw = p
        tiles = cdiv(G, R) * (Cout // BN)
        cost = cdiv(tiles, n_cu) * mtw * ntw
        if best is None or cost < best_cost or (cost == best_cost and tiles > best_tiles):
            best, best_cost, best_tiles = (i, R, nlpt, nsw), cost, tiles
    return best


def _b(v):
    return "true" if v else "false"


def ring_name(ntw, depth, conv, res):
    bk, ns = {2: (64, 2), 3: (64, 3), 4: (64, 4), 5: (32, 4)}[depth]
    return f"gemm_bf16_ring_kernel<{ntw},{bk},{ns},{_b(conv)},{_b(res)}>"


def patch_name(i, nlpt, nsw, res):
    wm, wn, mtw, ntw = PATCH_SHAPES[i]
    return f"conv3x3_patch_bf16_kernel<{wm},{wn},{mtw},{ntw},{nlpt},{nsw},{_b(res)}>"


def conv_path(case, flags):
    """The kernel (with the im2col kernel before it, if any) that i2l_conv_bn_act_bf16_fwd launches; facts in a dict."""
    B, H, W, Cin, Cout, k, s, pd, res, nchw = case
    Ho, Wo = out_hw(case)
    M, Kp = B * Ho * Wo, cdiv(k * k * Cin, 8) * 8
    assert (nchw or Cin % 8 == 0) and Cout % 8 == 0, "the entry refuses these"
    stem = Cin == 3 and Cout == 64 and k == 7 and s == 2 and pd == 3
    if nchw and not res and not flags & IM2COL_STEM and stem:
        return "stem_conv7_kernel", {}
    direct = not nchw and k == 1 and s == 1 and pd == 0
    implicit = not nchw and not direct and Cin % 64 == 0
    pre = ""
    if not direct and not implicit:
        if nchw:
            stem_lds = Cin * k * (31 * s + k) * 4
            pre = "im2col_stem_kernel+" if stem_lds <= 48 * 1024 and Ho <= 65535 and B <= 65535 else "im2col_nchw_f32_kernel+"
        else:
            pre = "im2col_nhwc_bf16_kernel+"
    forced = (flags >> 8) & 0xF
    short_k = direct and Kp <= 256 and not forced and cdiv(M, 128) * cdiv(Cout, 64) >= 1024
    gn = 64 if (Cout <= 64 or short_k) else 128
    if gn == 128 and Cout % 128 == 0 and not flags & WIDE:
        t128 = cdiv(M, 128) * (Cout // 128)
        if (2 * t128 + 255) // 256 < ((t128 + 255) // 256) * 2:
            gn = 64
    facts = {"M": M, "Kp": Kp, "gn": gn, "short_k": short_k}
    if implicit and k == 3 and s == 1 and pd == 1 and not flags & (NO_RING | NO_PATCH):
        pp = patch_plan(M, H, W, Cin, Cout, (flags >> 20) & 0xF)
        if pp is not None:
            i, R, nlpt, nsw = pp
            assert (i, nlpt, nsw) in PATCH_INSTANCES, "launch_patch would answer I2L_ERR_UNSUPPORTED"
            G = M // W
            facts.update(R=R, ragged=G % R != 0, straddle=H < R and B > 1)
            return patch_name(i, nlpt, nsw, res), facts
    if not flags & NO_RING and (direct or implicit) and Kp % 64 == 0:
        total = cdiv(Cout, gn) * cdiv(M, 128)
        depth = forced if 2 <= forced <= 5 else (4 if total <= 256 and Kp // 64 >= 4 else 2)
        facts.update(tiles=total, depth=depth)
        if short_k:
            return ("gemm_bf16_ring_kernel<1,64,1,false,%s,4>" if Kp == 64 else "gemm_bf16_ring_kernel<1,64,2,false,%s,3>") % _b(res), facts
        return ring_name(gn // 64, depth, implicit, res), facts
    return f"{pre}gemm_bf16_kernel<{gn // 64}>", facts


def family(name):
    """Kernel family of an instance name: the key of the recorded worst errors."""
    if name.startswith("gemm_bf16_ring_kernel"):
        return "short_k" if name.count(",") == 5 else "ring"         # the short_k instances carry an occupancy argument
    for key, fam in (("stem_conv7", "stem"), ("im2col", "im2col + single-buffered GEMM"), ("gemm_bf16_kernel", "single-buffered GEMM"),
                     ("patch", "patch")):
        if key in name:
            return fam
    raise AssertionError(name)


# ---------------------------------------------------------------------------------------------------------------
# 1. Cases.  name -> (case, flags of every variant)
# ---------------------------------------------------------------------------------------------------------------
def parity_variants(case):
    """The variant list of test_bf16_conv_bn_act_vs_torch."""
    _, _, _, _, _, k, s, pd, _, _ = case
    v = [0, NO_RING, DEPTH(2), DEPTH(3), DEPTH(4), DEPTH(5), IM2COL_STEM, WIDE]
    if k == 3 and s == 1 and pd == 1:
        v += [SHAPE(n) for n in range(1, 6)] + [NO_PATCH]
    return v


RING_DEPTHS = [DEPTH(2), DEPTH(3), DEPTH(4), DEPTH(5)]
NEW_CASES = [
    # short_k, Kp = 64: 256 row tiles (the last one ragged) x 4 column tiles = 1024; a forced depth switches short_k off
    ((1, 163, 201, 64, 256, 1, 1, 0, 0, 0), [0, DEPTH(3)]), ((1, 163, 201, 64, 256, 1, 1, 0, 1, 0), [0, DEPTH(3)]),
    # short_k, Kp = 128 and 256: 128 row tiles (ragged) x 8 column tiles
    ((1, 100, 163, 128, 512, 1, 1, 0, 0, 0), [0]), ((1, 100, 163, 128, 512, 1, 1, 0, 1, 0), [0]),
    ((1, 100, 163, 256, 512, 1, 1, 0, 0, 0), [0]), ((1, 100, 163, 256, 512, 1, 1, 0, 1, 0), [0]),
    # ring, 128-column tiles that the balance rule cannot narrow (Cout % 128 != 0, ragged N): direct and strided, no residual
    ((2, 5, 5, 128, 72, 1, 1, 0, 0, 0), RING_DEPTHS), ((2, 6, 6, 64, 136, 3, 2, 1, 0, 0), RING_DEPTHS),
    # ring, 64-column tiles: direct with a residual, strided 1x1 with a residual
    ((3, 5, 7, 128, 64, 1, 1, 0, 1, 0), RING_DEPTHS), ((2, 9, 7, 64, 64, 1, 2, 0, 1, 0), RING_DEPTHS),
    # im2col fallbacks with both tile widths of the single-buffered GEMM: fp32 images whose window is over 48 KB of LDS
    # (72 * 3 * 65 floats), fp32 images through the LDS window, NHWC with Cin % 64 != 0
    ((1, 7, 9, 72, 64, 3, 2, 1, 0, 1), [0]), ((1, 7, 9, 72, 72, 3, 2, 1, 1, 1), [0]),
    ((2, 9, 11, 3, 72, 3, 1, 1, 1, 1), [0]), ((2, 9, 9, 32, 72, 3, 1, 1, 0, 0), [0]),
    # single-buffered GEMM, 128-column tiles, straight from NHWC (Kp % 64 != 0)
    ((2, 5, 5, 40, 72, 1, 1, 0, 1, 0), [0]),
]
# patch: one (B, H, W, Cin, Cout) per (shape, nlpt, nsw) that some width selects, forced, with and without a residual
PATCH_NEW = [
    (0, (3, 3, 12, 64, 128)),      # shape 0, nlpt 4, ring 6: R = 13 rows of 12 > H = 3 (tiles straddle images), 9 rows % 13 != 0
    (0, (2, 3, 50, 64, 128)),      # shape 0, nlpt 8, ring 4: R = 3
    (1, (1, 3, 81, 64, 128)),      # shape 1, nlpt 4, ring 6: R = 1
    (1, (2, 3, 90, 64, 128)),      # shape 1, nlpt 8, ring 4: R = 1
    (1, (5, 1, 10, 64, 128)),      # shape 1, nlpt 4: R = 9, images of one row
    (2, (3, 3, 12, 64, 128)),      # shape 2, nlpt 4, ring 6: R = 10
    (2, (1, 5, 100, 64, 128)),     # shape 2, nlpt 8, ring 4: R = 1
    (3, (1, 3, 200, 64, 64)),      # shape 3, nlpt 12, ring 4: R = 1
    (3, (3, 7, 10, 64, 64)),       # shape 3, nlpt 8, ring 4: R = 32 > all 21 rows
    (4, (3, 5, 10, 64, 64)),       # shape 4, nlpt 8, ring 4: R = 25 > H
    (4, (1, 3, 200, 64, 64)),      # shape 4, nlpt 12, ring 4: R = 1
    (4, (2, 5, 100, 64, 64)),      # shape 4, nlpt 8: R = 2, 10 rows of 100
]
for _i, (_B, _H, _W, _ci, _co) in PATCH_NEW:
    for _res in (0, 1):
        NEW_CASES.append(((_B, _H, _W, _ci, _co, 3, 1, 1, _res, 0), [SHAPE(_i + 1)]))


def _name(case):
    return "x".join(str(v) for v in case)


CASES = {_name(c): (c, parity_variants(c)) for c in BF16_CONV_CASES}
for _c, _v in NEW_CASES:                                 # a shape listed twice runs the variants of both entries
    _have = CASES.setdefault(_name(_c), (_c, []))[1]
    _have += [f for f in _v if f not in _have]
NAMES = list(CASES)
JOIN_CASES = [(64, (3, 5, 20)), (128, (2, 16, 80)), (64, (1, 1, 1)), (128, (5, 7, 37))]     # test_bottleneck_join_equals_two_launches


# ---------------------------------------------------------------------------------------------------------------
# 2. The two float64 models
# ---------------------------------------------------------------------------------------------------------------
def rne_bf16(t):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), still as float64: one rounding, not through fp32."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)       # torch.round: half to even


def bf16_ulp(t):
    """Spacing of bf16 at the bf16 value t (t != 0)."""
    _, e = torch.frexp(t.double())
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def to_bf(t):
    return t.to(torch.bfloat16)


class Model:
    """u and its magnitude for one conv + BatchNorm, in float64, NCHW.  x64 / w64 hold bf16 values; r is bf16 NCHW or None."""

    def __init__(self, x64, w64, gamma, beta, mean, var, eps, stride, pad, r):
        scale = gamma.double() / torch.sqrt(var.double() + float(torch.tensor(eps, dtype=torch.float32)))
        bias = beta.double() - mean.double() * scale
        sh = (1, -1, 1, 1)
        conv = F.conv2d(x64, w64, stride=stride, padding=pad)
        self.conv_mag = F.conv2d(x64.abs(), w64.abs(), stride=stride, padding=pad)
        self.u = conv * scale.reshape(sh) + bias.reshape(sh)
        self.mag = self.conv_mag * scale.abs().reshape(sh) + (beta.double().abs() + (mean.double() * scale).abs()).reshape(sh)
        self.r = None if r is None else r.float()

    def f(self, t64, relu):
        t = t64.float()                                  # a bf16 value: exact
        if self.r is None:
            return to_bf(torch.relu(t) if relu else t)
        v = t + self.r                                   # fp32 add of two bf16 values
        return to_bf(torch.relu(v) if relu else v)

    def interval(self, relu, factor=DELTA):
        d = factor * self.mag
        return self.f(rne_bf16(self.u - d), relu), self.f(rne_bf16(self.u + d), relu)

    def center(self, relu):
        return self.f(rne_bf16(self.u), relu)


class Operands:
    pass


def _gen(case, exact):
    B, H, W, Cin, Cout, k, s, pd, res, nchw = case
    Ho, Wo = out_hw(case)
    g = torch.Generator().manual_seed(sum(case) + (7919 if exact else 0))
    o = Operands()
    if exact:
        n = 4 if k * k * Cin >= 576 else 16
        o.w = torch.randint(-n, n + 1, (Cout, Cin, k, k), generator=g).float()
        o.x = torch.randint(-n, n + 1, (B, Cin, H, W), generator=g).float()
        o.gamma = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (Cout,), generator=g)]
        o.beta = torch.randint(-3, 4, (Cout,), generator=g).float()
        o.mean, o.var, o.eps = torch.zeros(Cout), torch.full((Cout,), 3.0), 1.0
        o.r = to_bf(torch.randint(-64, 65, (B, Cout, Ho, Wo), generator=g).float()) if res else None
    else:                                                # the operands of test_bf16_conv_bn_act_vs_torch
        o.w = torch.randn(Cout, Cin, k, k, generator=g) * (Cin * k * k) ** -0.5
        o.gamma, o.beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
        o.mean, o.var, o.eps = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5, 1e-5
        o.x = torch.randn(B, Cin, H, W, generator=g)
        o.r = to_bf(torch.randn(B, Cout, Ho, Wo, generator=g)) if res else None
    # x: the fp32 images as they are (the stem and the im2col kernels round them to nearest even), else bf16
    o.x = o.x if nchw else to_bf(o.x)
    o.model = Model(to_bf(o.x).double(), to_bf(o.w).double(), o.gamma, o.beta, o.mean, o.var, o.eps, s, pd, o.r)
    return o


@functools.lru_cache(maxsize=None)
def interval_case(name):
    """Operands and (f(lo), f(hi), f(rne(u))) of a case on randn operands, relu = 1.  Read-only, shared by the tests."""
    o = _gen(CASES[name][0], exact=False)
    o.lo, o.hi = o.model.interval(1)
    o.mid = o.model.center(1)
    o.t = to_bf(rne_bf16(o.model.u).float())
    o.model = None                                       # the float64 planes of the big cases are not kept
    return o


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """Integer operands; want[relu] = f(rne(u)); the share of exact ties and the largest magnitude."""
    o = _gen(CASES[name][0], exact=True)
    m = o.model
    o.want = {relu: m.center(relu) for relu in (0, 1)}
    o.max_mag = float(torch.maximum(m.mag, m.conv_mag).max())
    o.tie_share = _tie_share(m.u)
    o.model = None
    return o


def _tie_share(u):
    """Share of the non-zero u that sit exactly half way between two bf16 values."""
    nz = u != 0
    b = rne_bf16(u)
    tie = ((u - b).abs() * 2 == bf16_ulp(torch.where(nz, u, torch.ones_like(u)))) & nz
    # u in [2^(e-1), 2^e): frexp's exponent of u is the binade's, also when rne(u) rounds up to 2^e
    return float(tie.sum()) / max(1, int(nz.sum()))


# ---------------------------------------------------------------------------------------------------------------
# 3. Host tests
# ---------------------------------------------------------------------------------------------------------------
def test_rne_bf16_is_one_rounding_to_even():
    one, ulp = 1.0, 2.0 ** -7
    t = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -30, -(one + ulp / 2), 0.0, 255.5, 256.0 + 1.0,
                      one + ulp / 2 - 2.0 ** -40], dtype=torch.float64)
    want = torch.tensor([one, one + 2 * ulp, one + ulp, -one, 0.0, 256.0, 256.0, one], dtype=torch.float64)
    assert torch.equal(rne_bf16(t), want)
    # through fp32 the last one rounds twice: 1 + 2^-8 - 2^-40 -> (fp32) 1 + 2^-8 -> (bf16, tie to even) 1.0 is still right,
    # but 1 + 2^-8 + 2^-40 -> 1 + 2^-8 -> 1.0 is wrong
    v = torch.tensor([one + ulp / 2 + 2.0 ** -40], dtype=torch.float64)
    assert float(rne_bf16(v)) == one + ulp and float(v.float().to(torch.bfloat16)) == one
    # agrees with torch's fp32 -> bf16 on fp32 inputs
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    assert torch.equal(rne_bf16(x.double()).float(), x.to(torch.bfloat16).float())
    assert float(bf16_ulp(torch.tensor(1.0))) == ulp and float(bf16_ulp(torch.tensor(255.0))) == 1.0


def reachable_patch_instances():
    """(shape, nlpt, nsw) that patch_plan computes for some width 1..PT of the shape."""
    out = set()
    for i, (wm, _, mtw, _) in enumerate(PATCH_SHAPES):
        for W in range(1, 32 * wm * mtw + 1):
            p = patch_shape_plan(i, W)
            if p is not None:
                out.add((i, p[1], p[2]))
    return out


# instantiated in launch_patch's switch, selected by no width (the trunk's path table): shape 3 = 320 pixels needs
# (R + 2)(W + 2) <= 255 with R = 320 // W for nlpt 4
UNREACHABLE_PATCH = {(3, 4, 6)}


def test_every_kernel_instance_is_reached():
    reached = {}
    for name, (case, variants) in CASES.items():
        for flags in variants:
            reached.setdefault(conv_path(case, flags)[0], (name, flags))
    want = {"stem_conv7_kernel"}
    want |= {f"{pre}+gemm_bf16_kernel<{n}>" for pre in ("im2col_stem_kernel", "im2col_nchw_f32_kernel", "im2col_nhwc_bf16_kernel")
             for n in (1, 2)}
    want |= {"gemm_bf16_kernel<1>", "gemm_bf16_kernel<2>"}
    want |= {ring_name(ntw, d, conv, res) for ntw in (1, 2) for d in (2, 3, 4, 5) for conv in (0, 1) for res in (0, 1)}
    want |= {f"gemm_bf16_ring_kernel<1,64,{ns},false,{_b(res)},{occ}>" for ns, occ in ((1, 4), (2, 3)) for res in (0, 1)}
    reachable = reachable_patch_instances()
    assert reachable <= set(PATCH_INSTANCES), "patch_plan computes a combination that launch_patch does not instantiate"
    assert set(PATCH_INSTANCES) - reachable == UNREACHABLE_PATCH
    want |= {patch_name(i, nl, ns, res) for (i, nl, ns) in reachable for res in (0, 1)}
    assert len(want) == 1 + 6 + 2 + 32 + 4 + 2 * len(reachable)
    missing = sorted(want - set(reached))
    assert not missing, missing
    assert set(reached) <= want, sorted(set(reached) - want)      # the restatement names nothing that does not exist
    # both join widths are the two n2 of JOIN_CASES
    assert {n2 for n2, _ in JOIN_CASES} == {64, 128}


def test_dispatch_thresholds():
    """The edges of the restated rules, at the shapes the GPU cases sit on."""
    sk64 = (1, 163, 201, 64, 256, 1, 1, 0, 0, 0)
    name, facts = conv_path(sk64, 0)
    assert name == "gemm_bf16_ring_kernel<1,64,1,false,false,4>" and facts["M"] == 32763 and facts["M"] % 128 and facts["tiles"] == 1024
    assert conv_path(sk64, DEPTH(3))[0] == ring_name(2, 3, 0, 0)                      # a forced depth switches short_k off
    name, facts = conv_path((1, 160, 204, 64, 256, 1, 1, 0, 0, 0), 0)               # 1020 tiles: the ordinary path
    assert facts["M"] == 32640 and not facts["short_k"] and name == ring_name(2, 2, 0, 0)
    for cin in (128, 256):
        name, facts = conv_path((1, 100, 163, cin, 512, 1, 1, 0, 1, 0), 0)
        assert name == "gemm_bf16_ring_kernel<1,64,2,false,true,3>" and facts["M"] == 16300 and facts["tiles"] == 1024
    assert not conv_path((1, 100, 163, 320, 512, 1, 1, 0, 1, 0), 0)[1]["short_k"]    # Kp > 256
    # the balance rule: 320 tiles of 128 x 128 -> 64 columns; 4 stages from 4 K tiles at no more than one tile per CU
    assert conv_path((16, 16, 80, 64, 256, 1, 1, 0, 0, 0), 0)[1]["gn"] == 64 and conv_path((16, 16, 80, 64, 256, 1, 1, 0, 0, 0), WIDE)[1]["gn"] == 128
    assert conv_path((1, 4, 5, 2048, 512, 1, 1, 0, 0, 0), 0)[1]["depth"] == 4 and conv_path((2, 7, 9, 192, 64, 1, 1, 0, 0, 0), 0)[1]["depth"] == 2
    # patch: tiles that straddle images, a grid that is no multiple of the tile, the widths of the issue's examples
    facts = [conv_path(c, v[0])[1] for c, v in NEW_CASES if c[5] == 3 and v[0] >> 20]
    assert any(f["straddle"] for f in facts) and any(f["ragged"] for f in facts) and any(f["R"] == 1 for f in facts)
    assert patch_shape_plan(1, 81) == (1, 4, 6) and patch_shape_plan(4, 10)[1] == 8 and patch_shape_plan(4, 200)[1] == 12
    assert patch_plan(100, 10, 10, 256, 128, 0) is None and patch_plan(100, 10, 10, 256, 128, 3) is not None   # Cin > 128 only forced


@pytest.mark.parametrize("name", NAMES)
def test_interval_is_bit_exact_on_95_percent(name):
    o = interval_case(name)
    amb = float((o.lo.float() != o.hi.float()).float().mean())
    assert bool((o.lo.float() <= o.mid.float()).all() and (o.mid.float() <= o.hi.float()).all())
    assert amb <= 0.05, amb


@pytest.mark.parametrize("name", NAMES)
def test_exact_case_is_exact_and_has_ties(name):
    o = exact_case(name)
    assert 2 * o.max_mag < 2 ** 24, o.max_mag
    assert o.tie_share >= 0.01, o.tie_share


def test_truncating_store_fails_the_interval():
    """What the interval is for: a store that truncates instead of rounding (restated on the CPU from an fp32 conv) leaves it on
    a large share of the elements, with and without a residual; the fp32 conv rounded to nearest even stays inside."""
    trunc = lambda t: (t.view(torch.int32) & ~0xFFFF).view(torch.float32)
    for name in ("2x9x13x64x64x3x1x1x0x0", "3x8x10x64x256x1x1x0x1x0"):
        case = CASES[name][0]
        o = interval_case(name)
        _, _, _, _, _, _, s, pd, res, _ = case
        scale = o.gamma / torch.sqrt(o.var + 1e-5)
        v = F.conv2d(o.x.float(), to_bf(o.w).float(), stride=s, padding=pd) * scale[None, :, None, None] \
            + (o.beta - o.mean * scale)[None, :, None, None]
        lo, hi = o.lo.float(), o.hi.float()
        good = torch.relu(to_bf(v).float() + o.r.float()).to(torch.bfloat16).float() if res else torch.relu(to_bf(v).float())
        bad = trunc(torch.relu(trunc(v) + o.r.float())) if res else torch.relu(trunc(v))
        assert bool(((good >= lo) & (good <= hi)).all())
        assert float(((bad < lo) | (bad > hi)).float().mean()) > 0.15


# ---------------------------------------------------------------------------------------------------------------
# 4. GPU tests
# ---------------------------------------------------------------------------------------------------------------
def _dv(t):
    return t.contiguous().to(DEV)


def _pack(L, w, gamma, beta, mean, var, eps):
    cout, cin, k, _ = w.shape
    nb = L.i2l_conv_bf16_packed_bytes(cout, cin, k, k)
    buf = torch.empty(nb, dtype=torch.uint8, device=DEV)
    t = [_dv(v) for v in (w, gamma, beta, mean, var)]
    _lib.check(L.i2l_conv_bn_bf16_pack(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), eps,
                                       buf.data_ptr(), nb, cout, cin, k, k, _lib.stream_ptr()), "pack")
    return buf


class Launch:
    """The device side of one case: operands uploaded once, one call per (flags, relu)."""

    def __init__(self, case, o):
        self.case, self.L = case, _lib.lib()
        B, H, W, Cin, Cout, k, s, pd, res, nchw = case
        self.packed = _pack(self.L, o.w, o.gamma, o.beta, o.mean, o.var, o.eps)
        self.x = _dv(o.x) if nchw else _dv(o.x.permute(0, 2, 3, 1))
        assert self.x.dtype == (torch.float32 if nchw else torch.bfloat16)
        self.r = _dv(o.r.permute(0, 2, 3, 1)) if res else None
        Ho, Wo = out_hw(case)
        self.y = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=DEV)

    def __call__(self, flags, relu):
        B, H, W, Cin, Cout, k, s, pd, res, nchw = self.case
        self.y.fill_(float("nan"))
        wsb = self.L.i2l_conv_bf16_workspace_bytes(B, H, W, Cin, Cout, k, k, s, pd, flags)
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.check(self.L.i2l_conv_bn_act_bf16_fwd(self.x.data_ptr(), nchw, self.packed.data_ptr(), _lib.ptr(self.r), self.y.data_ptr(),
                                                   B, H, W, Cin, Cout, k, k, s, pd, relu, ws.data_ptr(), wsb, flags,
                                                   _lib.stream_ptr()), "conv_bn_act_bf16_fwd")
        return self.y.cpu().permute(0, 3, 1, 2)          # NCHW view, bf16


def _in_interval(got, lo, hi, mid, t, what, fam):
    """f(lo) <= got <= f(hi) everywhere; records the worst distance from f(rne(u)) in bf16 ulps -- of rne(u) = t or of f(t),
    whichever is larger (with a residual the sum may cancel far below the tile's own rounding unit)."""
    g, lo, hi, mid = got.float(), lo.float(), hi.float(), mid.float()
    assert bool(torch.isfinite(g).all()), what
    ref = torch.maximum(mid.abs(), t.float().abs())
    nz = ref != 0
    if bool(nz.any()):
        record(f"resnet bf16 {fam}: worst |got - f(rne_bf16(u))| / ulp (interval model)",
               float(((g - mid)[nz].double().abs() / bf16_ulp(ref[nz])).max()))
    out = (g < lo) | (g > hi)
    if bool(out.any()):
        i = tuple(int(v) for v in out.nonzero()[0])
        raise AssertionError(f"{what}: {int(out.sum())} of {out.numel()} outside the interval; first at {i}: got {float(g[i])}, "
                             f"interval [{float(lo[i])}, {float(hi[i])}]")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_conv_interval_vs_float64(name):
    case, variants = CASES[name]
    o = interval_case(name)
    run = Launch(case, o)
    for flags in variants:
        path = conv_path(case, flags)[0]
        _in_interval(run(flags, 1), o.lo, o.hi, o.mid, o.t, (name, hex(flags), path), family(path))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_conv_exact_on_integers(name):
    case, variants = CASES[name]
    o = exact_case(name)
    run = Launch(case, o)
    for flags in variants:
        path = conv_path(case, flags)[0]
        for relu in (0, 1):
            got, want = run(flags, relu).float(), o.want[relu].float()
            bad = got != want                            # NaN compares unequal: an unwritten cell fails
            if bool(bad.any()):
                i = tuple(int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"{name} flags {hex(flags)} relu {relu} {path}: {int(bad.sum())} of {bad.numel()} differ; "
                                     f"first at {i}: got {float(got[i])}, want {float(want[i])}")


def _join_operands(n2, shape, exact):
    B, H, W = shape
    g = torch.Generator().manual_seed(500 + n2 + B * H * W + (7919 if exact else 0))
    o = Operands()
    o.convs = []
    for cout, cin in ((256, 64), (n2, 256)):
        c = Operands()
        if exact:
            n = 16 if cin == 64 else 4               # the rule of _gen: [-16, 16] at K = 64
            c.w = torch.randint(-n, n + 1, (cout, cin, 1, 1), generator=g).float()
            c.gamma = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (cout,), generator=g)]
            c.beta = torch.randint(-3, 4, (cout,), generator=g).float()
            c.mean, c.var, c.eps = torch.zeros(cout), torch.full((cout,), 3.0), 1.0
        else:
            c.w = torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5
            c.gamma, c.beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
            c.mean, c.var, c.eps = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5, 1e-5
        o.convs.append(c)
    if exact:
        o.o2 = to_bf(torch.randint(-16, 17, (B, 64, H, W), generator=g).float())
        o.ident = to_bf(torch.randint(-64, 65, (B, 256, H, W), generator=g).float())
    else:
        o.o2 = to_bf(torch.randn(B, 64, H, W, generator=g) * 0.7)
        o.ident = to_bf(torch.randn(B, 256, H, W, generator=g))
    c = o.convs[0]
    o.model_y = Model(o.o2.double(), to_bf(c.w).double(), c.gamma, c.beta, c.mean, c.var, c.eps, 1, 0, o.ident)
    return o


def _model_z(o, y):
    c = o.convs[1]
    return Model(y.double(), to_bf(c.w).double(), c.gamma, c.beta, c.mean, c.var, c.eps, 1, 0, None)


@pytest.mark.parametrize("n2,shape", JOIN_CASES)
def test_join_exact_case_is_exact_and_has_ties(n2, shape):
    """y by its model; z from the y the model expects (on the GPU: from the y the kernel returned, which must equal it)."""
    o = _join_operands(n2, shape, exact=True)
    y = o.model_y.center(1)
    mz = _model_z(o, y)
    for m in (o.model_y, mz):
        assert 2 * float(torch.maximum(m.mag, m.conv_mag).max()) < 2 ** 24
    # the 1 x 1 x 1 case has 256 + n2 outputs: too few for a share, the three others carry it
    if shape != (1, 1, 1):
        assert _tie_share(o.model_y.u) >= 0.01 and _tie_share(mz.u) >= 0.01


def _run_join(o, n2, shape):
    B, H, W = shape
    L = _lib.lib()
    p3, p1 = (_pack(L, c.w, c.gamma, c.beta, c.mean, c.var, c.eps) for c in o.convs)
    o2, ident = _dv(o.o2.permute(0, 2, 3, 1)), _dv(o.ident.permute(0, 2, 3, 1))
    y = torch.full((B, H, W, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
    z = torch.full((B, H, W, n2), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.check(L.i2l_bottleneck_join_bf16_fwd(o2.data_ptr(), p3.data_ptr(), ident.data_ptr(), y.data_ptr(), p1.data_ptr(), z.data_ptr(),
                                              B * H * W, 64, 256, n2, _lib.stream_ptr()), "join")
    return y.cpu().permute(0, 3, 1, 2), z.cpu().permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("n2,shape", JOIN_CASES)
def test_join_vs_float64(n2, shape):
    o = _join_operands(n2, shape, exact=False)
    y, z = _run_join(o, n2, shape)
    lo, hi = o.model_y.interval(1)
    assert float((lo != hi).float().mean()) <= 0.05
    _in_interval(y, lo, hi, o.model_y.center(1), rne_bf16(o.model_y.u), ("join y", n2, shape), "join")
    mz = _model_z(o, y)                                  # z from the y the kernel returned
    lo, hi = mz.interval(1)
    assert float((lo != hi).float().mean()) <= 0.05
    _in_interval(z, lo, hi, mz.center(1), rne_bf16(mz.u), ("join z", n2, shape), "join")


@pytest.mark.gpu
@pytest.mark.parametrize("n2,shape", JOIN_CASES)
def test_join_exact_on_integers(n2, shape):
    o = _join_operands(n2, shape, exact=True)
    y, z = _run_join(o, n2, shape)
    assert torch.equal(y.float(), o.model_y.center(1).float())
    assert torch.equal(z.float(), _model_z(o, y).center(1).float())


@pytest.mark.gpu
def test_fp32_images_never_overrun_the_workspace():
    """The size query has no x_is_nchw_f32 argument and answers 256 bytes for Cin % 64 == 0 (it sizes the gathering path, which
    takes NHWC bf16 only); fp32 images go through the column image, so the call must refuse that workspace rather than write
    B*Ho*Wo*Kp bf16 into it -- and compute the same result as any other path from a workspace that holds the image."""
    case = (1, 6, 7, 64, 64, 3, 1, 1, 0, 1)
    B, H, W, Cin, Cout, k, s, pd, _, _ = case
    L = _lib.lib()
    o = _gen(case, exact=True)
    run = Launch(case, o)
    assert L.i2l_conv_bf16_workspace_bytes(B, H, W, Cin, Cout, k, k, s, pd, 0) == 256
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    args = (run.x.data_ptr(), 1, run.packed.data_ptr(), None, run.y.data_ptr(), B, H, W, Cin, Cout, k, k, s, pd, 1, ws.data_ptr())
    assert L.i2l_conv_bn_act_bf16_fwd(*args, 256, 0, _lib.stream_ptr()) == -3
    need = (B * H * W * 9 * Cin * 2 + 255) // 256 * 256
    assert need <= ws.numel()
    assert L.i2l_conv_bn_act_bf16_fwd(*args, need - 256, 0, _lib.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert int(ws.max()) == 0                            # nothing was written
    run.y.fill_(float("nan"))
    _lib.check(L.i2l_conv_bn_act_bf16_fwd(*args, need, 0, _lib.stream_ptr()), "conv_bn_act_bf16_fwd")
    assert torch.equal(run.y.cpu().permute(0, 3, 1, 2).float(), o.model.center(1).float())
