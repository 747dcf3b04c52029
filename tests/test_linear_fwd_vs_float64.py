"""i2l_linear_bias_act_fwd (csrc/gemm.hip) called on its own through the C ABI on every plan of the two GEMM planners
and every path beneath them -- the fp32 matrix-core kernel with vector and non-vector loads, its direct epilogue and
its split-K slabs, the 3 x bf16 split kernel at both tile heights and all three block-index mappings, and the slab-sum
kernel's 8-wide loop, tail loop and second grid-stride pass -- and compared with a plain float64 CPU computation,
x.double() @ w.double().T + b, followed by ReLU where it applies.

1. A Python mirror of plan(), plan_bf16x3(), bf16x3_mt() and bf16x3_applicable() says, for (M, K, N, flags, operand
   alignment), which kernel runs, with how many slabs of which k_chunk, which tile height and block mapping, and how long
   the last K slice is.  A CPU test holds the mirror to the library's own workspace query over a sweep of shapes, and
   every GPU case asserts through the mirror the branch it is meant to reach BEFORE it calls the kernel: a planner change
   cannot silently empty a case.

2. What carries the sensitivity are four EXACT operand families, whose float64 truth is an fp32 number and which both
   kernels must reproduce bit for bit in any summation order (torch.equal): small integers, and three "selection"
   families in which every output is a single product.  A CPU emulation of the six-product split scheme shows that
   leaving out any one of the six products breaks at least one of them.

3. The floating family (zero-mean randn operands) is held to the project's bound for a GEMM-shaped result,
   |err| <= 2^-20 (sum |x||w| + |b|).  That bound sees wrong indexing, tails, bias and ReLU, which give O(1) errors.
   It does NOT see a lost split product: a CPU emulation with one of a0 b2, a1 b1, a2 b0 left out came to 0.34 - 0.39
   of the bound at K = 2048, 0.18 - 0.24 at K = 4096 and 0.05 - 0.09 at K = 40960 (the intact scheme: about 0.01).
   The exact families are there for that.

Operands and outputs sit in Buf objects: at an element offset inside a device buffer, between sentinel elements that
must survive; outputs start as NaN.  Workspaces have exactly the queried size and hold 0xFF bytes."""
import math
from collections import namedtuple

import pytest
import torch

from conftest import record
from img2latex_amd import _lib
from test_small_entries_vs_float64 import Buf, nans
from test_train_primitives import _ws

gpu = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3
EXACT = _lib.FLAG_EXACT_FP32
HEAD = 64                                # sentinel elements in front of every operand: keeps 256-byte alignment
BOUND = 2.0 ** -20


# ---------------------------------------------------------------------------------------------------------------
# 1. The planners, restated (csrc/gemm.hip: plan, plan_bf16x3, bf16x3_mt, bf16x3_applicable, slab_stride, i2l_gemm)
# ---------------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "kernel slabs k_chunk last ktiles vec mt mapping tiles epilogue reduce_passes reduce_wide "
                          "reduce_tail need")


def cdiv(a, b):
    return (a + b - 1) // b


def slab_stride(M, N):
    """Floats between two slabs: an odd number of 256-byte units."""
    units = cdiv(M * N, 64)
    return (units + 1 if units % 2 == 0 else units) * 64


def plan_fp32(M, K, N):
    """plan() with nz = 1 -> (tiles, slabs, k_chunk)"""
    tiles = cdiv(M, 64) * cdiv(N, 64)
    s = 1
    if tiles < 256 and K >= 1024:
        s = max(1, min(512 // tiles, K // 512))
    elif tiles <= 64 and K >= 256:
        s = max(1, min(256 // tiles, K // 64))
    kc = cdiv(cdiv(K, s), 64) * 64
    return tiles, cdiv(K, kc), kc


def split_mt(M):
    return 1 if M <= 64 else 2


def plan_split(M, K, N):
    """plan_bf16x3() with nz = 1 -> (tiles, S, k_chunk)"""
    tiles = cdiv(M, 64 * split_mt(M)) * cdiv(N, 64)
    s = max(1, min((512 if M * N >= 65536 else 768) // tiles, K // 256))
    kc = cdiv(cdiv(K, s), 32) * 32
    return tiles, cdiv(K, kc), kc


def split_applicable(K, x_al16, w_al16):
    """bf16x3_applicable() for the linear entry's operands: both K-contiguous with a row stride of K"""
    return K >= 64 and K % 8 == 0 and x_al16 and w_al16


def slab_bytes(M, N, slabs):
    need = slabs * slab_stride(M, N) * 4 if slabs > 1 else 0
    return cdiv(need, 256) * 256


def workspace_need(M, K, N):
    """i2l_linear_workspace_bytes: the larger of what the two kernels need, whichever a call then runs."""
    if M <= 0 or K <= 0 or N <= 0:
        return 0
    need = slab_bytes(M, N, plan_fp32(M, K, N)[1])
    if K >= 64:
        need = max(need, slab_bytes(M, N, plan_split(M, K, N)[1]))
    return need


def mirror(M, K, N, flags=0, x_al16=True, w_al16=True):
    """What one i2l_linear_bias_act_fwd call runs.  bias and y have no say: both kernels touch them element by element."""
    split = K >= 2048 and not (flags & EXACT) and split_applicable(K, x_al16, w_al16)
    if split:
        tiles, slabs, kc = plan_split(M, K, N)
        mapping = "xcd8" if slabs % 8 == 0 else "rowwalk" if slabs == 1 and tiles % 8 == 0 else "plain"
        vec, mt, step = None, split_mt(M), 32
    else:
        tiles, slabs, kc = plan_fp32(M, K, N)
        vec, mt, mapping, step = x_al16 and w_al16 and K % 4 == 0, None, None, 64
    blocks = min(cdiv(M * N, 256), 2048)
    return Plan(kernel="split" if split else "fp32", slabs=slabs, k_chunk=kc, last=K - (slabs - 1) * kc,
                ktiles=cdiv(min(K, kc), step), vec=vec, mt=mt, mapping=mapping, tiles=tiles,
                epilogue="direct" if slabs == 1 else "slab sum",
                reduce_passes=cdiv(M * N, blocks * 256) if slabs > 1 else 0,
                reduce_wide=slabs // 8 if slabs > 1 else 0, reduce_tail=slabs % 8 if slabs > 1 else 0,
                need=slab_bytes(M, N, slabs))


# ---------------------------------------------------------------------------------------------------------------
# 2. The case table: (M, K, N) -> what the mirror must say at flags = 0.  Each shape is the smallest that reaches its
#    branch.  Under I2L_FLAG_EXACT_FP32 every shape runs the fp32 kernel.
# ---------------------------------------------------------------------------------------------------------------
FP32_CASES = [
    # direct epilogue, ragged tiles, K % 4 != 0: the non-vector loads
    ((1, 7, 3), dict(slabs=1, tiles=1, vec=False, epilogue="direct")),
    ((5, 33, 70), dict(slabs=1, tiles=2, vec=False, epilogue="direct")),
    ((67, 130, 65), dict(slabs=1, tiles=4, vec=False, epilogue="direct")),
    # BK = 64 edge: one and two k-tiles
    ((3, 63, 5), dict(slabs=1, ktiles=1, vec=False)),
    ((3, 64, 5), dict(slabs=1, ktiles=1, vec=True)),
    ((3, 65, 5), dict(slabs=1, ktiles=2, vec=False)),
    ((65, 255, 65), dict(slabs=1, ktiles=4, last=255)),                 # the last K without a split
    ((2, 256, 3), dict(slabs=4, k_chunk=64, last=64)),                  # the planner's second branch
    ((2, 257, 3), dict(slabs=3, k_chunk=128, last=1)),                  # a last slab of one element
    ((9, 520, 9), dict(slabs=5, reduce_wide=0, reduce_tail=5)),         # slab sum: the tail loop only
    ((9, 576, 9), dict(slabs=9, reduce_wide=1, reduce_tail=1)),         # the 8-wide loop plus a tail
    ((70, 1023, 130), dict(slabs=8, reduce_wide=1, reduce_tail=0)),     # the 8-wide loop exactly
    ((70, 1024, 130), dict(slabs=2, k_chunk=512)),                      # the planner's first branch
    ((256, 512, 1024), dict(tiles=64, slabs=4)),                        # second branch: 64 tiles split,
    ((320, 512, 832), dict(tiles=65, slabs=1)),                         # 65 do not
    ((960, 1024, 1088), dict(tiles=255, slabs=2)),                      # first branch: 255 tiles split,
    ((1024, 1024, 1024), dict(tiles=256, slabs=1)),                     # 256 do not
    ((704, 1024, 1024), dict(slabs=2, reduce_passes=2)),                # slab sum: second grid-stride pass
    # K >= 2048 but K % 8 != 0: the split kernel does not apply
    ((3, 2050, 5), dict(kernel="fp32", vec=False, slabs=4)),
    ((3, 2052, 5), dict(kernel="fp32", vec=True, slabs=4)),
]
SPLIT_CASES = [
    ((1, 2048, 1), dict(mt=1, slabs=8, tiles=1, mapping="xcd8")),                      # the smallest
    ((64, 2048, 33), dict(mt=1, tiles=1)),                                             # MT = 1 / MT = 2 boundary
    ((65, 2048, 33), dict(mt=2, tiles=1)),
    ((5, 4096, 70), dict(slabs=16, tiles=2, mapping="xcd8")),
    ((130, 2056, 70), dict(mt=2, k_chunk=288, ktiles=9, last=40, mapping="xcd8")),     # odd chunk count, last slice 40
    ((5, 2312, 70), dict(slabs=9, mapping="plain", last=8)),                           # last slice: stage 0 only
    ((70, 2304, 130), dict(slabs=9, mt=2, tiles=3, mapping="plain")),
    ((704, 2048, 1024), dict(slabs=5, k_chunk=416, ktiles=13, mapping="plain", reduce_passes=2)),
    ((4224, 2048, 512), dict(tiles=264, slabs=1, mapping="rowwalk", epilogue="direct")),  # in-kernel epilogue
    ((4736, 2048, 448), dict(tiles=259, slabs=1, mapping="plain", epilogue="direct")),
    ((16, 40960, 64), dict(slabs=160, k_chunk=256, mapping="xcd8")),                   # the FC layer's own K
]
CASES = [(s, "fp32", e) for s, e in FP32_CASES] + [(s, "split", e) for s, e in SPLIT_CASES]


def check_plan(shape, kernel, expect, flags=0, x_al16=True, w_al16=True):
    p = mirror(*shape, flags, x_al16, w_al16)
    assert p.kernel == kernel, (shape, flags, p)
    for k, v in expect.items():
        assert getattr(p, k) == v, (shape, flags, k, v, p)
    return p


def test_case_table_reaches_its_branches():
    """Every row of the table against the mirror, and the table as a whole against the list of branches."""
    plans = [check_plan(s, k, e) for s, k, e in CASES]
    for s, _, _ in CASES:
        assert mirror(*s, EXACT).kernel == "fp32"
    f = [p for p in plans if p.kernel == "fp32"]
    s = [p for p in plans if p.kernel == "split"]
    assert {p.vec for p in f} == {True, False}
    assert {p.epilogue for p in f} == {p.epilogue for p in s} == {"direct", "slab sum"}
    assert {p.mapping for p in s} == {"xcd8", "rowwalk", "plain"} and {p.mt for p in s} == {1, 2}
    assert any(p.mapping == "plain" and p.slabs > 1 for p in s) and any(p.mapping == "plain" and p.slabs == 1 for p in s)
    assert any(p.last <= 32 for p in s)                                      # a last slice of a single 32-chunk
    assert any(p.ktiles % 2 for p in s) and any(p.ktiles % 2 == 0 for p in s)
    assert any(p.reduce_passes == 2 for p in f) and any(p.reduce_passes == 2 for p in s)
    assert any(p.reduce_wide and p.reduce_tail for p in plans) and any(p.reduce_wide == 0 and p.reduce_tail for p in plans)
    assert any(p.reduce_wide and not p.reduce_tail for p in plans)


def test_planner_mirror_matches_the_workspace_query():
    """max(fp32 need, split need) from the mirror == i2l_linear_workspace_bytes (host code: no GPU), over the edges
    of both planners and random triples; 0 for every non-positive dimension."""
    L = _lib.lib()
    MN = [1, 5, 64, 65, 130, 704, 4224]
    KS = [7, 63, 64, 255, 256, 257, 520, 1023, 1024, 2048, 2050, 2056, 2312, 40960]
    triples = [(M, K, N) for M in MN for K in KS for N in MN] + [s for s, _, _ in CASES]
    g = torch.Generator().manual_seed(11)
    for _ in range(400):
        M, N = (int(v) for v in torch.randint(1, 5000, (2,), generator=g))
        triples.append((M, int(torch.randint(1, 50000, (1,), generator=g)), N))
    for (M, K, N) in triples:
        assert L.i2l_linear_workspace_bytes(M, K, N) == workspace_need(M, K, N), (M, K, N)
        for flags in (0, EXACT):
            for al in (True, False):
                p = mirror(M, K, N, flags, al, al)
                assert p.need <= workspace_need(M, K, N) and 1 <= p.last <= p.k_chunk
                assert (p.slabs - 1) * p.k_chunk + p.last == K
    for bad in (0, -1, -70000):
        for (M, K, N) in [(bad, 2048, 64), (64, bad, 64), (64, 2048, bad), (bad, bad, bad)]:
            assert L.i2l_linear_workspace_bytes(M, K, N) == 0, (M, K, N)


# ---------------------------------------------------------------------------------------------------------------
# 3. Operand families.  Each returns x (M,K), w (N,K), b (N), the float64 x w^T (without the bias) and, for the
#    floating family, sum |x||w|.
# ---------------------------------------------------------------------------------------------------------------
EXACT_FAMILIES = ["integers", "selection A", "selection B", "selection C"]
FAMILIES = EXACT_FAMILIES + ["floating"]


def _pow2(n, g):
    """n values +-2^e, e in [-6, 6]"""
    e = torch.randint(-6, 7, (n,), generator=g).double()
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (sign * 2.0 ** e).float()


def _one_hot_rows(rows, K, val):
    """Row r holds val[r] at column 7 r mod K: every lane and k-group position is walked.  Returns the matrix, the columns."""
    col = (7 * torch.arange(rows)) % K
    m = torch.zeros(rows, K)
    m[torch.arange(rows), col] = val
    return m, col


def family(name, M, K, N, g, matmul=False):
    """matmul=True computes the selection families' truth by the float64 matrix product as well and asserts that it is
    the closed form the GPU tests use (one product per output)."""
    mag = None
    if name == "integers":            # every partial sum below 2^24 in any order: 8 * 8 * 40960 + 8 < 2^24
        x = torch.randint(-8, 9, (M, K), generator=g).float()
        w = torch.randint(-8, 9, (N, K), generator=g).float()
        b = torch.randint(-8, 9, (N,), generator=g).float()
        t = x.double() @ w.double().t()
    elif name == "floating":
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g)
        t = x.double() @ w.double().t()
        mag = x.double().abs() @ w.double().abs().t()
    else:
        b = torch.zeros(N)
        if name == "selection A":     # dense x with full 24-bit mantissas, w one-hot: y[m][n] = +-2^e x[m][k(n)]
            x = torch.randn(M, K, generator=g)
            w, col = _one_hot_rows(N, K, _pow2(N, g))
            t = x.double()[:, col] * w[torch.arange(N), col].double()[None, :]
        elif name == "selection B":   # the roles swapped: y[m][n] = +-2^e w[n][k(m)]
            x, col = _one_hot_rows(M, K, _pow2(M, g))
            w = torch.randn(N, K, generator=g)
            t = x[torch.arange(M), col].double()[:, None] * w.double()[:, col].t()
        else:                         # both +-2^e (1 + 2^-9): the product's 2^-18 bit lives in the a1 b1 term alone
            x = (_pow2(M * K, g).double() * (1 + 2.0 ** -9)).float().reshape(M, K)
            w, col = _one_hot_rows(N, K, (_pow2(N, g).double() * (1 + 2.0 ** -9)).float())
            t = x.double()[:, col] * w[torch.arange(N), col].double()[None, :]
        if matmul:
            assert torch.equal(t, x.double() @ w.double().t()), name
    return x, w, b, t, mag


def truth(t, b, relu):
    t = t if b is None else t + b.double()[None, :]
    return torch.relu(t) if relu else t


def split3(x):
    """bf16_split.inc.h: x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), round to nearest even"""
    s0 = x.bfloat16().float()
    r1 = x - s0
    s1 = r1.bfloat16().float()
    return s0, s1, (r1 - s1).bfloat16().float()


SPLIT_ORDER = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]          # gemm_bf16x3_kernel: TI, TJ


def emulate_split(x, w, drop=None):
    """The split kernel's arithmetic in fp32 on the CPU: per 16-deep k step (one MFMA) the six products in the kernel's
    order, each added to the fp32 accumulator; `drop` leaves one of them out."""
    (M, K), N = x.shape, w.shape[0]
    pad = cdiv(K, 16) * 16 - K
    a = [torch.nn.functional.pad(p, (0, pad)).reshape(M, -1, 16).transpose(0, 1) for p in split3(x)]
    b = [torch.nn.functional.pad(p, (0, pad)).reshape(N, -1, 16).transpose(0, 1) for p in split3(w)]
    prod = {ij: torch.bmm(a[ij[0]], b[ij[1]].transpose(1, 2)) for ij in SPLIT_ORDER if ij != drop}
    acc = torch.zeros(M, N)
    for c in range(a[0].shape[0]):
        for ij in SPLIT_ORDER:
            if ij != drop:
                acc = acc + prod[ij][c]
    return acc


def test_exact_families_are_exact_and_see_every_split_product():
    """(a) every exact family's float64 truth is an fp32 number (with and without bias and ReLU), and the selection
    families' closed form is the float64 matrix product; (b) the intact six-product scheme reproduces A, B and C bit
    for bit; (c) leaving out any one of the six products changes at least one of them."""
    g = torch.Generator().manual_seed(23)
    for (M, K, N) in [(70, 2056, 130), (5, 33, 70), (67, 130, 65), (16, 40960, 64)]:
        for name in EXACT_FAMILIES:
            x, w, b, t, _ = family(name, M, K, N, g, matmul=True)
            for bias in (b, None):
                for relu in (0, 1):
                    want = truth(t, bias, relu)
                    assert torch.equal(want.float().double(), want), (name, M, K, N)
            assert float(t.abs().max()) > 0
    M, K, N = 70, 2056, 130
    ops = {name: family(name, M, K, N, g) for name in EXACT_FAMILIES[1:]}
    for name, (x, w, _, t, _) in ops.items():
        assert torch.equal(emulate_split(x, w), t.float()), name
    seen = {}
    for drop in SPLIT_ORDER:
        seen[drop] = [name for name, (x, w, _, t, _) in ops.items() if not torch.equal(emulate_split(x, w, drop), t.float())]
        assert seen[drop], f"no exact family sees a lost a{drop[0]} b{drop[1]}"
    assert "selection A" in seen[(2, 0)] and "selection A" in seen[(1, 0)]
    assert "selection B" in seen[(0, 2)] and "selection B" in seen[(0, 1)]
    assert "selection C" in seen[(1, 1)] and len(seen[(0, 0)]) == 3


# ---------------------------------------------------------------------------------------------------------------
# 4. GPU: one call, one comparison
# ---------------------------------------------------------------------------------------------------------------
def place(host, off=0):
    """On the device behind HEAD + off sentinel elements: off = 0 and 4 keep 16-byte alignment, 1 and 2 break it."""
    buf = Buf(host, HEAD + off)
    assert buf.buf.data_ptr() % 256 == 0
    return buf


def al16(buf):
    return buf.ptr() % 16 == 0


def run(X, W, B, M, K, N, relu, flags, y_off=0, ws="exact"):
    """One call into a fresh NaN output with a fresh 0xFF workspace of exactly the queried size; returns (rc, output)."""
    L = _lib.lib()
    Y = place(nans(M, N), y_off)
    nbytes = L.i2l_linear_workspace_bytes(M, K, N)
    assert nbytes == workspace_need(M, K, N)
    wsbuf = _ws(nbytes)
    rc = L.i2l_linear_bias_act_fwd(X.ptr(), W.ptr(), B.ptr() if B is not None else None, Y.ptr(), M, K, N, relu,
                                   wsbuf.data_ptr(), nbytes, flags, _lib.stream_ptr())
    return rc, Y


def run_checked(X, W, B, M, K, N, relu, flags, what, y_off=0):
    """Two identical calls: rc, determinism (bit-equal buffers, sentinels included), sentinels, finiteness, ReLU's sign."""
    rc, Y = run(X, W, B, M, K, N, relu, flags, y_off)
    rc2, Y2 = run(X, W, B, M, K, N, relu, flags, y_off)
    assert rc == OK and rc2 == OK, (what, rc, rc2)
    torch.cuda.synchronize()
    assert torch.equal(Y.buf.view(torch.int32), Y2.buf.view(torch.int32)), ("a second call differs", what)
    got = Y.get().reshape(M, N)                  # asserts the head and tail sentinels
    assert torch.isfinite(got).all(), what
    if relu:
        assert float(got.min()) >= 0, what
    return got


def check_family(name, M, K, N, g, flag_list, worst, offs=None, group=None):
    """Every (flags, relu, bias) combination of one operand family at one shape.  offs: element offsets of x, w, b, y."""
    ox, ow, ob, oy = offs or (0, 0, 0, 0)
    x, w, b, t, mag = family(name, M, K, N, g)
    X, W, B = place(x, ox), place(w, ow), place(b, ob)
    for flags in flag_list:
        kernel = mirror(M, K, N, flags, al16(X), al16(W)).kernel
        for relu in (0, 1):
            for bias, Bd in ((b, B), (None, None)):
                what = (name, (M, K, N), f"flags={flags}", f"relu={relu}", "bias" if Bd else "no bias", kernel, offs)
                got = run_checked(X, W, Bd, M, K, N, relu, flags, what, oy)
                want = truth(t, bias, relu)
                if mag is None:
                    bad = int((got != want.float()).sum())
                    record(f"linear_fwd exact families, {kernel} kernel [mismatching elements]", bad)
                    assert torch.equal(got, want.float()), (what, f"{bad} of {M * N} elements differ")
                else:
                    scale = mag if bias is None else mag + bias.double().abs()[None, :]
                    r = float(((got.double() - want).abs() / (scale + 1e-300)).max())
                    key = (kernel, group)
                    worst[key] = max(worst.get(key, 0.0), r)
                    assert r <= BOUND, (what, r / BOUND)


def record_worst(worst):
    for (kernel, group), r in worst.items():
        record(f"linear_fwd floating, {kernel} kernel, {group} [err / (sum|x||w| + |b|)]", r)


@gpu
@pytest.mark.parametrize("shape,kernel,expect", CASES, ids=["%s-%dx%dx%d" % ((k,) + s) for s, k, _ in CASES])
def test_linear_fwd_every_plan_vs_float64(shape, kernel, expect):
    """One row of the case table: the mirror confirms the branch, then every operand family with ReLU off and on, with a
    bias and with bias = NULL, under flags = 0 and (K >= 64) I2L_FLAG_EXACT_FP32.  Exact families: torch.equal with
    the float64 truth.  Floating family: |err| <= 2^-20 (sum |x||w| + |b|) -- a bound that does not see a lost split
    product (0.05 - 0.39 of it on zero-mean operands, see the module docstring); the exact families do."""
    M, K, N = shape
    check_plan(shape, kernel, expect)
    assert mirror(M, K, N, EXACT).kernel == "fp32"
    flag_list = (0, EXACT) if K >= 64 else (0,)
    g = torch.Generator().manual_seed(1000 + CASES.index((shape, kernel, expect)))
    worst = {}
    for name in FAMILIES:
        check_family(name, M, K, N, g, flag_list, worst, group=f"{kernel}-table cases")
    record_worst(worst)


ALIGN_SHAPES = [(5, 33, 70), (70, 1024, 130), (130, 2056, 70)]
OFFSETS = [(0, 0, 0, 0)] + [tuple(o * (i == j) for j in range(4)) for i in range(4) for o in (1, 2, 4)] + [(1, 1, 1, 1)]


@gpu
@pytest.mark.parametrize("shape", ALIGN_SHAPES, ids=["%dx%dx%d" % s for s in ALIGN_SHAPES])
def test_linear_fwd_operand_alignment(shape):
    """x, w, bias and y at element offsets 1, 2 and 4 inside their buffers, one operand at a time, and all four at 1.
    Offset 4 keeps 16-byte alignment and with it the plan.  x or w at 1 or 2 must take the fp32 kernel's non-vector
    loads, and at K = 2056 leave the split kernel for it; bias and y are touched element by element by either kernel, so
    their offset leaves the plan alone.  The integer family stays exact and the floating family within the bound."""
    M, K, N = shape
    g = torch.Generator().manual_seed(77)
    flag_list = (0, EXACT) if K >= 64 else (0,)
    worst = {}
    for offs in OFFSETS:
        xa, wa = offs[0] % 4 == 0, offs[1] % 4 == 0
        for flags in flag_list:
            p, base = mirror(M, K, N, flags, xa, wa), mirror(M, K, N, flags)
            if xa and wa:
                assert p == base, (shape, offs, flags)
            else:
                assert p.kernel == "fp32" and p.vec is False, (shape, offs, flags, p)
        if K == 2056:
            assert mirror(M, K, N, 0, xa, wa).kernel == ("split" if xa and wa else "fp32")
        for name in ("integers", "floating"):
            check_family(name, M, K, N, g, flag_list, worst, offs=offs, group="alignment cases")
    record_worst(worst)


@gpu
@pytest.mark.parametrize("shape", [(130, 2056, 70), (67, 130, 65)], ids=["130x2056x70", "67x130x65"])
def test_linear_fwd_rows_are_independent(shape):
    """A NaN in one row of x: every other output row is bit-equal to the clean run, on both kernels.  What the poisoned
    row holds is unspecified (include/img2latex_hip.h)."""
    M, K, N = shape
    g = torch.Generator().manual_seed(91)
    x, w, b, _, _ = family("floating", M, K, N, g)
    row = M // 2 + 1
    bad = x.clone()
    bad[row, K // 3] = float("nan")
    X, Xbad, W, B = place(x), place(bad), place(w), place(b)
    keep = torch.arange(M) != row
    for flags in (0, EXACT):
        assert mirror(M, K, N, flags).kernel == ("split" if K >= 2048 and not flags else "fp32")
        for relu in (0, 1):
            clean = run_checked(X, W, B, M, K, N, relu, flags, (shape, flags, relu))
            rc, Y = run(Xbad, W, B, M, K, N, relu, flags)
            assert rc == OK
            got = Y.get().reshape(M, N)
            assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32)), (shape, flags, relu)


@gpu
def test_linear_fwd_refusals():
    """Refusals are return codes and leave the output all-NaN: I2L_ERR_ARG for a NULL x, w or y and a non-positive M, K
    or N; I2L_ERR_WORKSPACE, on both kernels, for a NULL workspace or one 256 bytes short of what the running kernel's
    slabs take.  Where the query returns 0 (K < 256) a NULL workspace of 0 bytes is accepted."""
    L = _lib.lib()
    st = _lib.stream_ptr()
    g = torch.Generator().manual_seed(5)

    def untouched(Y):
        assert torch.isnan(Y.get()).all()

    M, K, N = 5, 33, 70
    x, w, b, t, _ = family("integers", M, K, N, g)
    X, W, B = place(x), place(w), place(b)
    ws = _ws(4096)
    for i in range(3):
        Y = place(nans(M, N))
        ptrs = [X.ptr(), W.ptr(), Y.ptr()]
        ptrs[i] = None
        assert L.i2l_linear_bias_act_fwd(ptrs[0], ptrs[1], B.ptr(), ptrs[2], M, K, N, 0, ws.data_ptr(), 4096, 0, st) == ERR_ARG
        untouched(Y)
    for bad in (0, -1):
        for dims in [(bad, K, N), (M, bad, N), (M, K, bad)]:
            Y = place(nans(M, N))
            assert L.i2l_linear_bias_act_fwd(X.ptr(), W.ptr(), B.ptr(), Y.ptr(), *dims, 0, ws.data_ptr(), 4096, 0, st) == ERR_ARG
            untouched(Y)
    # no slabs, no workspace
    for (M, K, N) in [(5, 33, 70), (65, 255, 65)]:
        assert L.i2l_linear_workspace_bytes(M, K, N) == 0
        x, w, b, t, _ = family("integers", M, K, N, g)
        X, W, B, Y = place(x), place(w), place(b), place(nans(M, N))
        assert L.i2l_linear_bias_act_fwd(X.ptr(), W.ptr(), B.ptr(), Y.ptr(), M, K, N, 1, None, 0, 0, st) == OK
        assert torch.equal(Y.get().reshape(M, N), truth(t, b, 1).float())
    # slabs: the workspace is checked before anything is launched
    for (M, K, N), flags, kernel in [((2, 256, 3), 0, "fp32"), ((70, 1024, 130), 0, "fp32"), ((5, 4096, 70), EXACT, "fp32"),
                                     ((5, 4096, 70), 0, "split"), ((130, 2056, 70), 0, "split"), ((1, 2048, 1), 0, "split")]:
        p = mirror(M, K, N, flags)
        assert p.kernel == kernel and p.slabs > 1 and p.need >= 256
        nbytes = L.i2l_linear_workspace_bytes(M, K, N)
        assert nbytes >= p.need
        x, w, b, t, _ = family("integers", M, K, N, g)
        X, W, B = place(x), place(w), place(b)
        ws = _ws(nbytes)
        for ptr, size in ((None, nbytes), (ws.data_ptr(), p.need - 256)):
            Y = place(nans(M, N))
            rc = L.i2l_linear_bias_act_fwd(X.ptr(), W.ptr(), B.ptr(), Y.ptr(), M, K, N, 0, ptr, size, flags, st)
            assert rc == ERR_WORKSPACE, ((M, K, N), flags, size, rc)
            untouched(Y)
        Y = place(nans(M, N))
        assert L.i2l_linear_bias_act_fwd(X.ptr(), W.ptr(), B.ptr(), Y.ptr(), M, K, N, 0, ws.data_ptr(), nbytes, flags, st) == OK
        assert torch.equal(Y.get().reshape(M, N), truth(t, b, 0).float())
