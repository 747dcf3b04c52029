"""The CNN encoder's conv block (csrc/conv.hip, csrc/conv_bf16x3.hip, the conv branches of csrc/gemm.hip) through the C ABI
only -- i2l_conv3x3_relu_pool2_fwd and i2l_conv3x3_relu_pool2_bwd -- on every dispatch path, against a float64 restatement.

Backward.  The entry takes y, argmax and dy as INPUTS, so the test makes them up (argmax uniform in 0..3, y randn with a
few +0.0 / -0.0 / positive-subnormal cells, dy randn): the backward is then a linear function of (x, w, dy) and its
float64 value has no near-tie problem:
    g = dy * (y > 0);  dyp[:, :, e>>1 : 2Hp : 2, e&1 : 2Wp : 2] = g * (argmax == e)  for e in 0..3, zeros elsewhere
    dx = conv2d_input(dyp, w);  dw = conv2d_weight(x, dyp);  db = dyp.sum((0, 2, 3))
Bounds (taken from the project, not tuned on the kernels): dx 2^-21 of the same operation on the absolute operands (the bound
test_bf16x3_adversarial_operands holds the same conv kernels to), dw 2^-20 (test_train_primitives' bound for GEMM-shaped
results), db 2^-23 of sum |dyp| on the plane_sum path (a double accumulation rounded once) and 2^-20 from the first-block
kernel (fp32 partials).  Where every contribution is zero the result must be exactly 0.0.

Forward.  |err| <= 2^-21 * (sum |x||w| + |b|) against float64 and never worse than 4x the fp32 CPU oracle's error
+ 2^-22 of the magnitude (the rule of test_bf16x3_adversarial_operands), with and without argmax_out; the arg max and the
ReLU gate by the rule of helpers.check_decisions (they may differ from float64 only within 2e-6 of the window's
magnitude, exact ties take the first index).

Part 0 of this file RESTATES the dispatch arithmetic of conv.hip, conv_bf16x3.hip and gemm.hip in Python (pick_wx, the
tile walks, the first-block kernel's LDS budget, the split-bf16 GEMM's applicability, the backward's branch order) and an
unmarked test asserts that the case lists below reach every path it names.  IT MUST BE EDITED TOGETHER WITH THOSE THREE
FILES: a changed threshold there silently moves a case to another kernel otherwise.

Outputs start as NaN and carry a sentinel tail, workspaces are exactly the size the query returns and filled with 0xFF
(test_train_primitives' Out / _ws); the worst ratio of every family is record()ed into parity_errors.json."""
import math

import pytest
import torch
import torch.nn.functional as F

import img2latex_oracle as O
from conftest import record
from helpers import _adversarial
from img2latex_amd import _lib
from test_train_primitives import Out, _dev, _ratio, _ws

EXACT, NO_SPARSE = _lib.FLAG_EXACT_FP32, _lib.FLAG_CONV_NO_SPARSE_WGRAD


# ---------------------------------------------------------------------------------------------------------------
# 0. The dispatch arithmetic of conv.hip / conv_bf16x3.hip / gemm.hip, restated (pointers 16-byte aligned, as every
#    tensor and workspace of this file is)
# ---------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def pick_wx(rows, cols):
    """conv.hip pick_wx / i2l_conv_bf16x3_run: workgroup tile (4/wx*4) x (wx*16), fewest covered positions, ties 8x32."""
    best, best_cover = 2, -1
    for wx in (2, 1, 4):
        tr, tc = (4 // wx) * 4, wx * 16
        cover = cdiv(rows, tr) * tr * cdiv(cols, tc) * tc
        if best_cover < 0 or cover < best_cover:
            best, best_cover = wx, cover
    return best


def split_walk(B, H, W, Cout):
    """i2l_conv_bf16x3_run: (wx, tiles per image, items_per_wg, does a walk of > 1 tile straddle two images)."""
    rows, cols = 2 * (H // 2), 2 * (W // 2)
    wx = pick_wx(rows, cols)
    tpi = cdiv(cols, wx * 16) * cdiv(rows, (4 // wx) * 4)
    n_items, co_blocks = tpi * B, cdiv(Cout, 64)
    ipw = (n_items * co_blocks + 511) // 512
    if n_items * co_blocks <= 768:
        ipw = 1
    ipw = max(ipw, 1)
    straddle = ipw > 1 and any((k * ipw) // tpi != (min((k + 1) * ipw, n_items) - 1) // tpi
                               for k in range(cdiv(n_items, ipw)))
    return wx, tpi, ipw, straddle


def smallk_parts(B, H, W, Cout):
    """i2l_conv_smallk_run: (column tiles of a band, parts, tiles per part)."""
    tiles_x, bands = cdiv(2 * (W // 2), 32), cdiv(2 * (H // 2), 8)
    parts = 1
    while parts < tiles_x and (Cout // 32) * bands * B * parts < 1536:
        parts += 1
    tpp = cdiv(tiles_x, parts)
    return tiles_x, cdiv(tiles_x, tpp), tpp


def wgrad_first_lds(Cin, W, Cout):
    """conv.hip wgrad_first_lds: LDS bytes of conv_wgrad_first_kernel, 0 = not its business / over 80 KB."""
    if Cin < 1 or Cin > 3 or Cout % 32 != 0 or W < 2:
        return 0
    gs_, no = (W // 2) | 1, Cin * 9 + 1
    b = (Cin * 4 * (W + 2) + max(32 * gs_, 8 * 32 * no)) * 4 + 32 * gs_
    return b if b <= 80 * 1024 else 0


def gemm_split_ok(K, nz, lda, bsa, pooled=False, conv_h=0, conv_w=0):
    """gemm.hip bf16x3_applicable for the conv weight gradients (A K-contiguous; W gathered when conv_h > 0, else the
    K-contiguous column image with ldw = K)."""
    if K < 64 or (nz > 1 and (K % 32 != 0 or nz * K > 0x7fffffff)):
        return False
    if pooled:
        if not (conv_h > 0 and conv_w % 8 == 0 and conv_h % 2 == 0 and lda % 4 == 0 and bsa % 4 == 0):
            return False
    elif lda % 4 != 0 or K % 8 != 0:
        return False
    if conv_h > 0:
        return K == conv_h * conv_w
    return K % 8 == 0


def split_gemm_slabs(M, N, KT):
    """gemm.hip plan_bf16x3: K slabs of the split-bf16 GEMM."""
    tiles = cdiv(M, 64 * (1 if M <= 64 else 2)) * cdiv(N, 64)
    s = (512 if M * N >= 65536 else 768) // tiles
    s = max(1, min(s, KT // 256))
    kc = cdiv(cdiv(KT, s), 32) * 32
    return cdiv(KT, kc)


def _reduce_name(M, N, S):
    if S == 1:
        return "one_slab"
    return "reduce_lanes" if M * N <= 131072 and S >= 32 else "reduce_plain"


def fwd_path(case, flags, want_am):
    """(kernel family, path names) of i2l_conv3x3_relu_pool2_fwd."""
    B, Cin, H, W, Cout = case
    am = "argmax" if want_am else "no_argmax"
    odd = ":odd_hw" if H % 2 and W % 2 else ""
    if not flags & EXACT and 1 <= Cin <= 3 and Cout % 32 == 0:
        tiles_x, parts, tpp = smallk_parts(B, H, W, Cout)
        if parts > 1 and tpp > 1 and tiles_x % tpp != 0:
            kind = "parts_short_last"
        elif parts == 1 and tiles_x > 1:
            kind = "single_part"
        else:
            kind = "one_tile_parts"
        return "smallk", {f"fwd:smallk<{Cin}>:{kind}:{am}"}
    if not flags & EXACT and Cin % 16 == 0 and Cout % 64 == 0:
        wx, tpi, ipw, straddle = split_walk(B, H, W, Cout)
        names = {f"fwd:split:wx{wx}:{am}"}
        if ipw > 1 and straddle and tpi % 2 == 1:
            names.add(f"fwd:split:multi_tile_walk:{am}")
        return "split", names
    if Cout % 32 == 0:
        ci_blk, ntl = (4 if Cin <= 4 else 8), (2 if Cout % 64 == 0 else 1)
        wx = pick_wx(2 * (H // 2), 2 * (W // 2))
        return "mfma", {f"fwd:mfma<{ci_blk},{ntl}>:{am}", f"fwd:mfma:wx{wx}"}
    return "direct", {f"fwd:direct{odd}:{am}"}


def bwd_path(case, flags, want_dx):
    """({"dx": family, "dw": family, "db": family}, path names) of i2l_conv3x3_relu_pool2_bwd, in its branch order."""
    B, Cin, H, W, Cout = case
    Hp, Wp, HW = H // 2, W // 2, H * W
    exact, split = bool(flags & EXACT), not flags & EXACT
    names, fam = set(), {}
    first_ok = wgrad_first_lds(Cin, W, Cout) != 0
    first = first_ok and not want_dx and not flags & NO_SPARSE
    fused = (not want_dx and H % 2 == 0 and W % 2 == 0 and split and
             gemm_split_ok(HW, B, Hp * Wp, Cout * Hp * Wp, pooled=True, conv_h=H, conv_w=W))
    if not fused and not first:
        names.add("unpool:vec4" if W % 4 == 0 else "unpool:scalar")
        if H % 2 and W % 2:
            names.add("unpool:odd_hw")
    if 1 <= Cin <= 3 and Cout % 32 == 0 and not want_dx:
        if flags & NO_SPARSE:
            names.add("dw:first:disabled_by_flag")
        elif not first_ok:
            names.add(f"dw:first<{Cin}>:lds_refused")
    if first:
        fast = W % 8 == 0 and W <= 512
        names.add(f"dw:first<{Cin}>:{'fast' if fast else 'slow'}")
        names.add("db:first")
        fam["dw"], fam["db"] = "first", "first"
        return fam, names
    names.add("db:plane_sum")
    fam["db"] = "plane_sum"
    if fused:
        names.add("dw:fused_unpool:" + _reduce_name(Cout, Cin * 9, split_gemm_slabs(Cout, Cin * 9, B * HW)))
        fam["dw"] = "fused_unpool"
    elif split and gemm_split_ok(HW, B, HW, Cout * HW, conv_h=H, conv_w=W):
        names.add("dw:implicit:" + _reduce_name(Cout, Cin * 9, split_gemm_slabs(Cout, Cin * 9, B * HW)))
        fam["dw"] = "implicit"
    else:
        # im2col_t + i2l_gemm per chunk of 32 images.  Each chunk GEMM asks bf16x3_applicable again, with its own
        # number of images: a chunk of several images is refused whenever the implicit GEMM was (gemm_kernel, fp32
        # MFMA), but a last chunk of ONE image needs no H*W % 32 == 0 and can run gemm_bf16x3_kernel with `accumulate`
        chunks = [min(32, B - b0) for b0 in range(0, B, 32)]
        on_split = [split and gemm_split_ok(HW, nb, HW, Cout * HW) for nb in chunks]
        assert not on_split[0] and not any(ok for ok, nb in zip(on_split, chunks) if nb > 1)
        why = "exact_flag" if exact else ("hw_not_32" if HW % 32 else "other")
        names.add("dw:chunked:" + ("accumulate:" if B > 32 else "one_chunk:") + why)
        if on_split[-1]:
            names.add("dw:chunked:accumulate:split_last_chunk")
        fam["dw"] = "chunked"
    if want_dx:
        # run_conv(pool = false, dyp, w): Cout -> Cin channels at full resolution
        even = H % 2 == 0 and W % 2 == 0
        if split and even and Cout % 16 == 0 and (Cin % 64 == 0 or Cin == 32):
            # conv3x3_bf16x3_kernel<WX, true, false, 1>: 32 output channels per workgroup, which are all of a 32-channel
            # block's input ("whole") or one half of a packed 64-channel filter block ("halves")
            wx, blocks = pick_wx(H, W), ("whole" if Cin == 32 else "halves")
            names.add(f"dx:split:wx{wx}:{blocks}")
            fam["dx"] = f"split wx{wx} {blocks}"
        elif Cin % 32 == 0:
            why = "exact_flag" if exact else ("odd_hw" if not even else ("cout_not_16" if Cout % 16 else "other"))
            names.add("dx:mfma_plain:" + why)
            fam["dx"] = "mfma"
        else:
            names.add("dx:direct" + (":odd_hw" if H % 2 and W % 2 else ""))
            fam["dx"] = "direct"
    return fam, names


# ---- the case lists --------------------------------------------------------------------------------------------
#             B  Cin  H    W   Cout
BWD_CASES = [
    (2, 32, 14, 16, 64),       # dx split (32 channels) on 16x16; dw implicit / fused un-pool in one slab
    (2, 64, 4, 64, 64),        # dx split (64 channels, two half blocks) on 4x64; two K slabs: the plain reduction
    (2, 32, 12, 20, 64),       # dx split (32 channels) on 8x32; H*W = 240: chunked fallback, one chunk
    (2, 32, 4, 64, 64),        # dx split (32 channels) on 4x64
    (2, 64, 12, 20, 64),       # dx split (64 channels, two half blocks) on 8x32
    (8, 32, 16, 64, 64),       # 32 K slabs: splitk_reduce_lanes_kernel (implicit and fused un-pool)
    (3, 64, 16, 80, 128),      # block 3 of the primary config: dx split (two half blocks) on 16x16, 128-row GEMM tiles, 15 slabs
    (33, 16, 6, 10, 64),       # B > 32 and H*W % 32 != 0: the second chunk accumulates; dx direct on even H, W
    (33, 32, 4, 16, 64),       # implicit GEMM; chunked + accumulate under the exact flag only
    (33, 32, 12, 20, 64),      # H*W = 240: 32 images on the fp32 GEMM, the 33rd alone on the split GEMM with `accumulate`
    (2, 32, 7, 9, 64),         # odd H and W: scalar un-pool, plain-mode MFMA dx
    (2, 32, 8, 8, 24),         # forward Cout % 16 != 0 with forward Cin % 32 == 0: plain-mode MFMA dx on even H, W
    (2, 5, 7, 9, 9),           # direct dx on odd H and W
    (3, 16, 10, 14, 64),       # W % 4 != 0 on even H, W
    # the first block (Cin <= 3, Cout % 32 == 0): the sparse kernel without dx, the GEMMs with NO_SPARSE / with dx
    (2, 1, 6, 16, 32), (2, 2, 6, 24, 32), (2, 3, 7, 40, 64),       # fast staging (W % 8 == 0, W <= 512)
    (2, 1, 5, 34, 32), (2, 2, 4, 34, 32), (2, 3, 6, 34, 32), (2, 3, 7, 9, 32),   # slow staging
    (2, 3, 2, 800, 32), (2, 2, 4, 800, 32),    # over the LDS budget: the GEMMs
    (2, 1, 2, 800, 32),                        # fits (slow staging: W > 512)
]


def _bwd_runs(case):
    flag_list = [0, EXACT]
    if 1 <= case[1] <= 3 and case[4] % 32 == 0:
        flag_list.append(NO_SPARSE)
    return [(fl, dx) for fl in flag_list for dx in (False, True)]


BWD_ADVERSARIAL_CASE = (6, 32, 8, 32, 64)      # split dx, implicit / fused-unpool dw (H*W = 256)
# positive-subnormal gate: scalar and vec4 un-pool, plane_sum, the fused-unpool GEMM, the first-block kernel (both stagings)
SUBNORMAL_CASES = [(2, 32, 7, 9, 64), (2, 32, 14, 16, 64), (2, 3, 7, 40, 64), (2, 3, 6, 34, 32)]

FWD_CASES = [
    # split kernel: the three tiles (the 8x32 one ragged in rows, columns and with an odd last row / column), 2 chunks
    (2, 16, 14, 16, 64), (1, 16, 4, 120, 64), (2, 32, 11, 45, 64),
    (7, 16, 8, 352, 640),      # 11 tiles per image, walks of 2 tiles: three walks straddle two images
    # first-block kernel: parts of 2, 2 and 1 column tiles / one part walking both tiles
    (4, 1, 126, 131, 256), (4, 2, 126, 131, 256), (4, 3, 126, 131, 256),
    (48, 1, 64, 34, 128), (48, 2, 64, 34, 128), (48, 3, 64, 34, 128),
    # exact kernels (with flags = 0 these are the fp32 MFMA / direct kernels as well: no split kernel takes them)
    (2, 4, 14, 16, 96),        # <4, 1> on 16x16
    (1, 4, 4, 120, 64),        # <4, 2> on 4x64
    (2, 5, 9, 37, 96),         # <8, 1> on 8x32, odd H and W
    (2, 24, 12, 20, 128),      # <8, 2>, three chunks of 8
    (2, 3, 7, 9, 5),           # direct, odd H and W
]
FIXUP_CASES = [(2, 3, 16, 40, 32), (2, 16, 12, 20, 64)]

PATHS = {
    # unpool
    "unpool:scalar", "unpool:vec4", "unpool:odd_hw",
    # weight gradient
    "dw:first<1>:fast", "dw:first<2>:fast", "dw:first<3>:fast", "dw:first<1>:slow", "dw:first<2>:slow", "dw:first<3>:slow",
    "dw:first<2>:lds_refused", "dw:first<3>:lds_refused", "dw:first:disabled_by_flag",
    "dw:fused_unpool:one_slab", "dw:fused_unpool:reduce_plain", "dw:fused_unpool:reduce_lanes",
    "dw:implicit:one_slab", "dw:implicit:reduce_plain", "dw:implicit:reduce_lanes",
    "dw:chunked:one_chunk:exact_flag", "dw:chunked:one_chunk:hw_not_32",
    "dw:chunked:accumulate:exact_flag", "dw:chunked:accumulate:hw_not_32", "dw:chunked:accumulate:split_last_chunk",
    # data gradient
    "dx:split:wx1:whole", "dx:split:wx2:whole", "dx:split:wx4:whole", "dx:split:wx1:halves", "dx:split:wx2:halves", "dx:split:wx4:halves",
    "dx:mfma_plain:exact_flag", "dx:mfma_plain:odd_hw", "dx:mfma_plain:cout_not_16", "dx:direct", "dx:direct:odd_hw",
    # bias sums
    "db:plane_sum", "db:first",
    # forward
    "fwd:split:wx1:no_argmax", "fwd:split:wx2:no_argmax", "fwd:split:wx4:no_argmax",
    "fwd:split:wx1:argmax", "fwd:split:wx2:argmax", "fwd:split:wx4:argmax",
    "fwd:split:multi_tile_walk:no_argmax", "fwd:split:multi_tile_walk:argmax",
    "fwd:smallk<1>:parts_short_last:no_argmax", "fwd:smallk<2>:parts_short_last:no_argmax", "fwd:smallk<3>:parts_short_last:no_argmax",
    "fwd:smallk<1>:parts_short_last:argmax", "fwd:smallk<2>:parts_short_last:argmax", "fwd:smallk<3>:parts_short_last:argmax",
    "fwd:smallk<1>:single_part:no_argmax", "fwd:smallk<2>:single_part:no_argmax", "fwd:smallk<3>:single_part:no_argmax",
    "fwd:smallk<1>:single_part:argmax", "fwd:smallk<2>:single_part:argmax", "fwd:smallk<3>:single_part:argmax",
    "fwd:mfma<4,1>:no_argmax", "fwd:mfma<4,2>:no_argmax", "fwd:mfma<8,1>:no_argmax", "fwd:mfma<8,2>:no_argmax",
    "fwd:mfma<4,1>:argmax", "fwd:mfma<4,2>:argmax", "fwd:mfma<8,1>:argmax", "fwd:mfma<8,2>:argmax",
    "fwd:mfma:wx1", "fwd:mfma:wx2", "fwd:mfma:wx4",
    "fwd:direct:odd_hw:no_argmax", "fwd:direct:odd_hw:argmax",
    "fwd:fixup:smallk", "fwd:fixup:split",
}


def test_case_lists_cover_every_path():
    """The union of the path names that the restated dispatch gives for this file's case lists is the whole list: every
    kernel, tile shape, staging flavour, reduction kernel and fallback of the conv block runs in some test below."""
    seen = set()
    for case in BWD_CASES:
        for flags, want_dx in _bwd_runs(case):
            seen |= bwd_path(case, flags, want_dx)[1]
    for case in FWD_CASES:
        for flags in (0, EXACT):
            for want_am in (False, True):
                seen |= fwd_path(case, flags, want_am)[1]
    for case in FIXUP_CASES:
        fam, _ = fwd_path(case, 0, True)
        assert fam in ("smallk", "split")
        seen.add("fwd:fixup:" + fam)
    assert seen == PATHS, (sorted(PATHS - seen), sorted(seen - PATHS))
    # the arithmetic quoted in the case lists' comments
    assert [pick_wx(14, 16), pick_wx(4, 64), pick_wx(12, 20), pick_wx(16, 80)] == [1, 4, 2, 1]
    assert split_walk(7, 8, 352, 640) == (2, 11, 2, True)
    assert smallk_parts(4, 126, 131, 256) == (5, 3, 2) and smallk_parts(48, 64, 34, 128) == (2, 1, 2)
    assert [wgrad_first_lds(c, 800, 32) != 0 for c in (1, 2, 3)] == [True, False, False]
    # adversarial and subnormal-gate cases sit on the paths their tests name
    assert bwd_path(BWD_ADVERSARIAL_CASE, 0, True)[0] == {"db": "plane_sum", "dw": "implicit", "dx": "split wx2 whole"}
    assert bwd_path(BWD_ADVERSARIAL_CASE, 0, False)[0]["dw"] == "fused_unpool"
    sub = set()
    for case in SUBNORMAL_CASES:
        for want_dx in (False, True):
            sub |= bwd_path(case, 0, want_dx)[1]
    assert {"unpool:scalar", "unpool:vec4", "db:plane_sum", "dw:fused_unpool:one_slab", "dw:first<3>:fast",
            "dw:first<3>:slow"} <= sub, sorted(sub)


# ---------------------------------------------------------------------------------------------------------------
# 1. The backward as a pure function of (x, w, y, argmax, dy)
# ---------------------------------------------------------------------------------------------------------------
def _bwd_truth(x, w, y, am, dy):
    """float64 dx, dw, db of the restatement in the module docstring and their magnitudes (the same operations on the
    absolute operands).  An odd last row / column of dyp stays zero."""
    B, Cout, Hp, Wp = dy.shape
    H, W = x.shape[2:]
    gated = dy.double() * (y.double() > 0)
    dyp = torch.zeros(B, Cout, H, W, dtype=torch.float64)
    for e in range(4):
        dyp[:, :, e >> 1:2 * Hp:2, e & 1:2 * Wp:2] = gated * (am == e)
    xd, wd = x.double(), w.double()
    dx = torch.nn.grad.conv2d_input(xd.shape, wd, dyp, padding=1)
    dw = torch.nn.grad.conv2d_weight(xd, wd.shape, dyp, padding=1)
    dxm = torch.nn.grad.conv2d_input(xd.shape, wd.abs(), dyp.abs(), padding=1)
    dwm = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, dyp.abs(), padding=1)
    return dx, dw, dyp.sum((0, 2, 3)), dxm, dwm, dyp.abs().sum((0, 2, 3))


@pytest.mark.parametrize("case", [(2, 3, 7, 9, 5), (3, 16, 10, 14, 64)])
def test_restatement_equals_float64_autograd(case):
    """The restatement against float64 autograd of the block itself (conv -> ReLU -> max_pool2d) under the block's own
    decisions: identical (the un-pooled gradient holds at most one nonzero per window, so every sum has the same terms)."""
    B, Cin, H, W, Cout = case
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64, generator=g).requires_grad_()
    w = (torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g) / (3 * Cin ** 0.5)).requires_grad_()
    b = torch.randn(Cout, dtype=torch.float64, generator=g).requires_grad_()
    z = F.conv2d(x, w, b, padding=1)
    y = F.max_pool2d(torch.relu(z), 2)
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g)
    (y * dy).sum().backward()
    am = O.pool_windows(z.detach()).argmax(-1)
    dx, dw, db, _, _, _ = _bwd_truth(x.detach(), w.detach(), y.detach(), am, dy)
    assert float((dx - x.grad).abs().max()) == 0.0
    assert float((dw - w.grad).abs().max()) == 0.0
    assert float((db - b.grad).abs().max()) == 0.0


def _bwd_operands(case, g):
    """x, w, y, argmax, dy: random, with a few y cells at +0.0 and -0.0 (closed under y > 0) and at 2^-130 (open: the
    gradient there is made large so that a gate that flushes subnormals misses by far more than any bound)."""
    B, Cin, H, W, Cout = case
    Hp, Wp = H // 2, W // 2
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    y = torch.randn(B, Cout, Hp, Wp, generator=g)
    am = torch.randint(0, 4, (B, Cout, Hp, Wp), generator=g, dtype=torch.uint8)
    dy = torch.randn(B, Cout, Hp, Wp, generator=g)
    cells = torch.randperm(y.numel(), generator=g)[:12]
    y.view(-1)[cells[0:4]] = 0.0
    y.view(-1)[cells[4:8]] = -0.0
    y.view(-1)[cells[8:12]] = 2.0 ** -130
    dy.view(-1)[cells] = 8.0
    return x, w, y, am, dy


def _run_bwd(L, case, dev, flags, want_dx):
    B, Cin, H, W, Cout = case
    x, w, y, am, dy = dev
    nb = L.i2l_conv_bwd_workspace_bytes(B, Cin, H, W, Cout)
    assert nb > 0
    ws = _ws(nb)
    dx = Out((B, Cin, H, W)) if want_dx else None
    dw, db = Out((Cout, Cin, 3, 3)), Out((Cout,))
    rc = L.i2l_conv3x3_relu_pool2_bwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), am.data_ptr(), dy.data_ptr(),
                                      dx.ptr() if dx else None, dw.ptr(), db.ptr(), B, Cin, H, W, Cout, ws.data_ptr(), nb,
                                      flags, None, _lib.stream_ptr())
    assert rc == 0, (case, flags, want_dx, rc)
    return (dx.get() if dx else None), dw.get(), db.get()


DX_BOUND, DW_BOUND = 2.0 ** -21, 2.0 ** -20
DB_BOUND = {"plane_sum": 2.0 ** -23, "first": 2.0 ** -20}


def _check_bwd(case, operands, truth, runs, tag):
    """Every (flags, dx wanted) run of one case against `truth`; zero magnitude means exactly 0.0 (NaN fails either way).
    Every run is measured and record()ed before the case is judged, so one miss hides no figure."""
    L = _lib.lib()
    dx64, dw64, db64, dxm, dwm, dbm = truth
    dev = tuple(_dev(t) for t in operands)
    bad = []
    for flags, want_dx in runs:
        fam, _ = bwd_path(case, flags, want_dx)
        dx, dw, db = _run_bwd(L, case, dev, flags, want_dx)
        got = {"dw": (dw, dw64, dwm, DW_BOUND), "db": (db, db64, dbm, DB_BOUND[fam["db"]])}
        if want_dx:
            got["dx"] = (dx, dx64, dxm, DX_BOUND)
        for what, (t, t64, mag, bound) in got.items():
            r = _ratio(t, t64, mag)
            record(f"conv block bwd {what} {fam[what]} {tag} [err / magnitude]", r)
            print(f"{case} {tag} flags={flags:#x} dx={int(want_dx)} {what} {fam[what]}: 2^{math.log2(r) if r > 0 else -999:.2f}")
            if not bool(torch.isfinite(t).all()):
                bad.append((flags, want_dx, what, fam[what], "not finite"))
            elif not r <= bound:
                bad.append((flags, want_dx, what, fam[what], f"2^{math.log2(r):.2f} > 2^{math.log2(bound):.0f}"))
            elif not bool((t[mag == 0] == 0).all()):
                bad.append((flags, want_dx, what, fam[what], "nonzero where every contribution is zero"))
    assert not bad, (case, tag, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bwd_paths_vs_float64(case):
    """dx, dw and db of made-up (y, argmax, dy) on every backward path: flags 0 / EXACT_FP32 (/ CONV_NO_SPARSE_WGRAD where
    the first-block kernel applies), with and without dx."""
    g = torch.Generator().manual_seed(1000 + BWD_CASES.index(case))
    operands = _bwd_operands(case, g)
    _check_bwd(case, operands, _bwd_truth(*operands), _bwd_runs(case), "randn")


@pytest.mark.gpu
def test_bwd_all_gates_closed_is_exactly_zero():
    """y <= 0 everywhere (negative, +0.0 and -0.0): dx, dw and db are exactly 0.0 on the GEMM, chunked and first-block
    paths -- not NaN from an un-initialised slab, workspace or partial."""
    for case in [(2, 32, 14, 16, 64), (33, 16, 6, 10, 64), (2, 3, 7, 40, 64), (2, 3, 6, 34, 32)]:
        g = torch.Generator().manual_seed(7)
        x, w, y, am, dy = _bwd_operands(case, g)
        y = -y.abs()
        y.view(-1)[::3] = 0.0
        y.view(-1)[1::3] = -0.0
        truth = _bwd_truth(x, w, y, am, dy)
        assert all(float(t.abs().max()) == 0.0 for t in truth)
        _check_bwd(case, (x, w, y, am, dy), truth, _bwd_runs(case), "gates closed")


@pytest.mark.gpu
def test_bwd_positive_subnormal_gate_is_open():
    """include/img2latex_hip.h: the gate is y > 0.  Every open cell holds y = 2^-130 here, so a path that flushes the
    subnormal before the comparison returns zeros: both un-pool kernels, plane_sum_pooled_kernel, the fused-unpool GEMM
    and the first-block kernel (both stagings), all held to the bounds of the randn cases."""
    for case in SUBNORMAL_CASES:
        g = torch.Generator().manual_seed(11)
        x, w, y, am, dy = _bwd_operands(case, g)
        y = torch.where(y > 0, torch.full_like(y, 2.0 ** -130), y)
        assert float(y.max()) == 2.0 ** -130 and float(y.double().max()) > 0          # the host keeps subnormals
        truth = _bwd_truth(x, w, y, am, dy)
        assert float(truth[5].min()) > 0                                               # every channel has open cells
        runs = [(fl, dx) for fl in (0, EXACT) for dx in (False, True)]
        _check_bwd(case, (x, w, y, am, dy), truth, runs, "subnormal gate")


@pytest.mark.gpu
def test_bwd_adversarial_dynamic_range():
    """helpers._adversarial "range_2^+-60" inside the backward's two reductions, same bounds.  dx sums over the output
    channels: dy and w are scaled inversely per output channel.  dw sums over (image, position): x is scaled per band of
    positions -- an image, the bands the kernels' flattened (image, position) axis is cut into -- and dy inversely."""
    case = BWD_ADVERSARIAL_CASE
    kind = "range_2^+-60"
    g = torch.Generator().manual_seed(23)
    x, w, y, am, dy = _bwd_operands(case, g)
    dy_c, w_c = _adversarial(kind, dy, w, 1, 0, g)
    runs = [(fl, dx) for fl in (0, EXACT) for dx in (False, True)]
    _check_bwd(case, (x, w_c, y, am, dy_c), _bwd_truth(x, w_c, y, am, dy_c), runs, kind + " over channels")
    x_b, dy_b = _adversarial(kind, x, dy, 0, 0, g)
    _check_bwd(case, (x_b, w, y, am, dy_b), _bwd_truth(x_b, w, y, am, dy_b), runs, kind + " over positions")


# ---------------------------------------------------------------------------------------------------------------
# 2. The forward paths
# ---------------------------------------------------------------------------------------------------------------
AM_TAIL, AM_SENTINEL = 64, 0xEE


def _run_fwd(L, case, dev, flags, want_am):
    """y (NaN-initialised, sentinel tail) and the arg max (0xFF-initialised, sentinel tail) of one forward call, plus
    the workspace (its head holds the first-block kernel's near-decision count)."""
    B, Cin, H, W, Cout = case
    x, w, b = dev
    Hp, Wp = H // 2, W // 2
    nb = L.i2l_conv_workspace_bytes(Cin, Cout)
    ws = _ws(nb)
    y = Out((B, Cout, Hp, Wp))
    n = B * Cout * Hp * Wp
    am = None
    if want_am:
        am = torch.full((n + AM_TAIL,), AM_SENTINEL, dtype=torch.uint8, device="cuda")
        am[:n] = 0xFF
    rc = L.i2l_conv3x3_relu_pool2_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.ptr(), am.data_ptr() if want_am else None,
                                      B, Cin, H, W, Cout, ws.data_ptr(), nb, flags, _lib.stream_ptr())
    assert rc == 0, (case, flags, want_am, rc)
    y_host = y.get()
    if want_am:
        am = am.cpu()
        assert bool((am[n:] == AM_SENTINEL).all()), "an arg max write past the end"
        am = am[:n].reshape(B, Cout, Hp, Wp)
        assert int(am.max()) <= 3, "an arg max was not written"
    return y_host, am, ws


def _fwd_truth(x, w, b):
    """float64: the four pre-bias values of every pooling window, the block's output, its magnitude sum |x||w| + |b|
    (pooled: the window's largest, as test_hip_parity._conv_truth), the window magnitude of helpers.check_decisions."""
    xd, wd, bd = x.double(), w.double(), b.double()
    win = O.pool_windows(F.conv2d(xd, wd, None, padding=1))
    mag = O.pool_windows(F.conv2d(xd.abs(), wd.abs(), None, padding=1)).amax(-1) + bd.abs()[None, :, None, None]
    truth = torch.relu(win.amax(-1) + bd[None, :, None, None])
    return win, truth, mag


def _check_decisions(win, b, mag, am, gate, what, tol=2e-6):
    """helpers.check_decisions for one block whose float64 windows are at hand."""
    top2 = win.topk(2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    pre = top2[..., 0] + b.double()[None, :, None, None]
    ref_am = win.argmax(-1)
    am = am.long()
    wrong_gate = gate != (pre > 0)
    wrong_am = (am != ref_am) & gate & (pre > 0) & (gap > 0)
    if wrong_am.any():
        chosen = win.gather(-1, am.unsqueeze(-1)).squeeze(-1)
        worst = float(((top2[..., 0] - chosen)[wrong_am] / mag[wrong_am]).max())
        assert worst <= tol, f"{what}: arg max differs from float64 at a gap of {worst:.2e} of sum|x||w|"
    if wrong_gate.any():
        worst = float((pre[wrong_gate].abs() / mag[wrong_gate]).max())
        assert worst <= tol, f"{what}: ReLU gate differs from float64 at |pre| = {worst:.2e} of sum|x||w|"
    tie = (gap == 0) & gate & (pre > 0)
    assert bool((am[tie] == ref_am[tie]).all()), f"{what}: an exact tie must take the first index"
    return int(tie.sum())


def _fwd_operands(case, kind, g):
    B, Cin, H, W, Cout = case
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    if kind == "cancellation":
        x, w = _adversarial(kind, x, w, 1, 1, g)
    else:
        x[:, :, :, W - 6:] = 0.5            # a constant region: windows inside it are exact four-way ties
    return x, w, b


def _fwd_kinds(case):
    return ["randn"] + (["cancellation"] if case[1] >= 2 else [])     # cancellation pairs input channels: Cin >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", [(c, k) for c in FWD_CASES for k in _fwd_kinds(c)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_fwd_paths_vs_float64(case, kind):
    """y of every forward path, flags 0 and EXACT_FP32, argmax_out NULL and set; with argmax_out the decisions too."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(2000 + 7 * FWD_CASES.index(case) + len(kind))
    x, w, b = _fwd_operands(case, kind, g)
    win, truth, mag = _fwd_truth(x, w, b)
    oracle_err = (O.conv_block(x, w, b).double() - truth).abs()
    dev = tuple(_dev(t) for t in (x, w, b))
    ties, bad = 0, []
    for flags in (0, EXACT):
        for want_am in (False, True):
            fam, _ = fwd_path(case, flags, want_am)
            y, am, _ = _run_fwd(L, case, dev, flags, want_am)
            err = (y.double() - truth).abs()
            r = float((err / (mag + 1e-300)).max())
            over = float(((err - 4 * oracle_err) / (mag + 1e-300)).max())
            print(f"{case} {kind} flags={flags:#x} argmax={int(want_am)} {fam}: 2^{math.log2(r) if r > 0 else -999:.2f}, "
                  f"beyond 4x the oracle's error: 2^{math.log2(over) if over > 0 else -999:.2f}")
            record(f"conv block fwd {fam} {kind} {'argmax' if want_am else 'inference'} [err / (sum|x||w| + |b|)]", r)
            if not bool(torch.isfinite(y).all()):
                bad.append((flags, want_am, fam, "not finite"))
            if not r <= 2.0 ** -21:
                bad.append((flags, want_am, fam, f"2^{math.log2(r):.2f} > 2^-21"))
            if not over <= 2.0 ** -22:
                bad.append((flags, want_am, fam, f"(err - 4 oracle err) / magnitude = 2^{math.log2(over):.2f} > 2^-22"))
            if want_am:
                ties += _check_decisions(win, b, mag, am, y > 0, f"{case} {kind} flags={flags:#x} {fam}")
    assert not bad, (case, kind, bad)
    if kind == "randn" and case[3] >= 12:
        assert ties > 0, "the constant region gave no exact tie"


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIXUP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fwd_fixup_pass_decides_near_ties(case):
    """A constant image plus 1e-6 noise: most windows are near-ties, the split kernels list them (far below the list's
    capacity at this size) and conv_pool_fixup_kernel re-evaluates them in fp32.  The count must be above 0 and the
    decisions after the fix-up within the rule; y within the forward bound."""
    L = _lib.lib()
    B, Cin, H, W, Cout = case
    g = torch.Generator().manual_seed(5)
    x = 0.5 + 1e-6 * torch.randn(B, Cin, H, W, generator=g)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) / (9 * Cin) ** 0.5
    b = torch.rand(Cout, generator=g) * 0.1 + 0.5
    fam, _ = fwd_path(case, 0, True)
    win, truth, mag = _fwd_truth(x, w, b)
    y, am, ws = _run_fwd(L, case, tuple(_dev(t) for t in (x, w, b)), 0, True)
    # the list: at the workspace's head for the first-block kernel, behind the packed filters for the split kernel
    # (i2l_conv_bf16x3_workspace_bytes: 9 taps x 3 splits x 2 halves x 64 channels 16-byte pieces per 16-channel chunk)
    head = 0 if fam == "smallk" else cdiv(cdiv(Cout, 64) * (Cin // 16) * 9 * 3 * 2 * 64 * 16, 256) * 256
    listed = int(ws[head:head + 4].view(torch.int32).cpu()[0])
    assert 0 < listed <= B * Cout * (H // 2) * (W // 2) < (1 << 20), listed
    r = _ratio(y, truth, mag)
    record(f"conv block fwd {fam} near-ties after the fix-up [err / (sum|x||w| + |b|)]", r)
    assert r <= 2.0 ** -21, (case, r)
    _check_decisions(win, b, mag, am, y > 0, f"{case} near-ties")
