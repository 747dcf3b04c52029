"""The evaluation kernels of csrc/metrics.hip at validation's own shapes: i2l_teacher_forced_eval against the float64
restatement of tests/test_validation_gpu.py on every row-count regime of its finishing workgroup, on both sides of every
register-tile boundary, on planted ties and on non-finite logits (torch.argmax / torch's float64 cross_entropy on the CPU
are the reference there); i2l_masked_accuracy against torch.argmax, exact integers; Validator's handling of a non-finite
batch loss with a stub model.  The only arithmetic is the loss sum; every id, length and count is compared exactly."""
import random
import types
import warnings

import numpy as np
import pytest
import torch

import metrics_oracle as MO
from conftest import record
from helpers import DEV
from img2latex_amd import _lib
from test_validation_gpu import _case, _np_eval, _run

gpu = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
LOSS_TOL = 2e-6                     # tests/test_validation_gpu.py's criterion: |got - want| / max(1, |want|)


def _first_pad(a, pad):
    T = a.shape[1]
    return np.array([list(r).index(pad) if pad in r else T for r in a.tolist()], dtype=np.int32)


def _torch_eval(x, tgt, pad, eps):
    """The reference where logits are not finite: torch.argmax of the fp32 tensor and torch's float64 cross_entropy per
    row, both on the CPU (targets in range).  Same keys as _np_eval."""
    B, T, V = x.shape
    xt = torch.from_numpy(x)
    arg = xt.argmax(-1).numpy().astype(np.int32)
    rows = torch.nn.functional.cross_entropy(xt.double().reshape(-1, V), torch.from_numpy(tgt).long().reshape(-1),
                                             ignore_index=pad, reduction="none", label_smoothing=eps)
    keep = tgt != pad
    return dict(loss=float(rows.sum()), count=int(keep.sum()), ids=arg, pred_len=_first_pad(arg, pad),
                target_len=_first_pad(tgt, pad), correct=int(((arg == tgt) & keep).sum()), total=int(keep.sum()))


def _check(got, want, what, name=None):
    """Every output of one call against the reference; the loss sum by class (finite / NaN / +inf) and, when finite,
    by the 2e-6 criterion.  Returns the relative loss error (0 for a non-finite sum)."""
    g, w = float(got["lc"][0]), want["loss"]
    err = 0.0
    if np.isfinite(w):
        err = abs(g - w) / max(1.0, abs(w))
        if name:
            record(name, err)
        assert np.isfinite(g) and err <= LOSS_TOL, (what, g, w, err)
    elif np.isnan(w):
        assert np.isnan(g), (what, g, w)
    else:
        assert g == w, (what, g, w)
    assert float(got["lc"][1]) == want["count"], (what, float(got["lc"][1]), want["count"])
    assert np.array_equal(got["ids"], want["ids"]), (what, np.argwhere(got["ids"] != want["ids"])[:8].tolist())
    assert np.array_equal(got["pred_len"], want["pred_len"]), (what, got["pred_len"].tolist(), want["pred_len"].tolist())
    assert np.array_equal(got["target_len"], want["target_len"]), what
    assert got["ct"].tolist() == [want["correct"], want["total"]], (what, got["ct"].tolist(), want["correct"], want["total"])
    return err


# --------------------------------------------------------------------------- teacher-forced eval: row-count regimes
# rows: 1, 1023, 1024, 1025 (one pass of the 1024 threads, on and around it), 3072 / 3073 (the four-in-flight loop not
# entered / entered once), 4096 / 4097 (no tail / a tail of one), 8450 (two four-in-flight passes, B > 16 waves' stride,
# T = 65: a second ballot pass of one position), 9536 = training's 64 x 149 (the tail loop iterates twice)
REGIMES = [(1, 1), (33, 31), (32, 32), (25, 41), (48, 64), (439, 7), (64, 64), (17, 241), (130, 65), (64, 149)]


def _ragged_case(B, T, V, seed, pad=0):
    """Ragged targets (a fifth of the sequences all pad, a fifth without pad, the rest cut at a random step) and the
    pad column the arg max in a tenth of the rows; where T > 64 half of the sequences get their FIRST such row at step
    63, 64 or 65, so pred_len lands on either side of the 64-position ballot boundary."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    tgt = rng.integers(1, V, size=(B, T)).astype(np.int32)
    kind = rng.random(B)
    if B == 1:
        kind[:] = 0.3
    for b in range(B):
        if kind[b] < 0.2:
            tgt[b, :] = pad
        elif kind[b] >= 0.4:
            tgt[b, rng.integers(0, T):] = pad
    hit = rng.random((B, T)) < 0.1
    for b in range(B):
        if T > 64 and b % 2 == 0:
            s = min(63 + (b // 2) % 3, T)                              # s == T: no pad at all, pred_len = T
            hit[b, :s] = False
            x[b, :s, pad] = -9.0                                       # no earlier row has its arg max at pad
            if s < T:
                hit[b, s] = True
        elif b % 5 == 1:
            hit[b, :] = False
    x[hit, pad] = x[hit].max(-1) + 1.0
    return x, tgt


@gpu
@pytest.mark.parametrize("B,T,V", [(b, t, 37) for b, t in REGIMES] + [(64, 149, 512)])
def test_teacher_forced_eval_row_count_regimes(B, T, V):
    x, tgt = _ragged_case(B, T, V, seed=1000 * B + T + V)
    name = f"teacher_forced_eval loss sum [rel] {B}x{T}={B * T} rows V={V}"
    for eps in (0.0, 0.1):
        want = _np_eval(x, tgt, 0, eps)
        got = _run(x, tgt, 0, eps)
        _check(got, want, (B, T, V, eps), name)
        if T > 64:                                                     # the planted lengths are really there
            assert {63, 64, 65} <= set(want["pred_len"].tolist())
        if (B, T) == (64, 149):
            again = _run(x, tgt, 0, eps)                               # deterministic: bit-identical
            assert all(got[k].tobytes() == again[k].tobytes() for k in got)
            bare = _run(x, tgt, 0, eps, want_ids=False, want_len=False)   # NULL id / length pointers: same sums
            assert bare["lc"].tobytes() == got["lc"].tobytes() and bare["ct"].tolist() == got["ct"].tolist()
            assert (bare["ids"] == -7).all() and (bare["pred_len"] == -7).all() and (bare["target_len"] == -7).all()


@gpu
@pytest.mark.parametrize("B,T", [(2, 0), (0, 5)])
def test_teacher_forced_eval_zero_rows(B, T):
    x = np.zeros((B, T, 37), np.float32)
    tgt = np.zeros((B, T), np.int32)
    got = _run(x, tgt, 0, 0.1)                                         # asserts the return code 0
    assert got["lc"].tolist() == [0.0, 0.0] and got["ct"].tolist() == [0, 0]
    assert got["pred_len"].tolist() == [0] * B and got["target_len"].tolist() == [0] * B


# --------------------------------------------------------------------------- register-tile boundaries, ties
@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [255, 256, 257, 260, 511, 513, 1023, 1024, 1025, 2047, 2049, 2052])
def test_teacher_forced_eval_tile_boundaries(V, eps):
    x, tgt = _case(V, seed=V * 10 + int(eps * 10))
    want = _np_eval(x, tgt, 0, eps)
    for misalign in ([False, True] if V % 4 == 0 else [False]):
        _check(_run(x, tgt, 0, eps, misalign=misalign), want, (V, eps, misalign),
               "teacher_forced_eval loss sum [rel] tile boundaries")


def _tie_rows(V, rng, quarters=False):
    """Rows with an exact tie in the maximum: (first index, second index, row) for the index pairs (i, i+1), (i, i+4),
    (i, i+64), (i, i+256) where they fit, (0, V-1), and a row of equal values (first 0, second V-1)."""
    out = []

    def base():
        r = rng.standard_normal(V).astype(np.float32)
        return (np.round(r * 4.0) / 4.0).astype(np.float32) if quarters else r

    for d in (1, 4, 64, 256):
        for i in sorted({0, 3, V // 3, V - 1 - d}):
            if i >= 0 and i + d < V:
                r = base()
                r[i] = r[i + d] = r.max() + 1.0
                out.append((i, i + d, r))
    if V > 1:
        r = base()
        r[0] = r[V - 1] = r.max() + 1.0
        out.append((0, V - 1, r))
    out.append((0, V - 1, np.full(V, 0.75, np.float32)))
    return out


@gpu
@pytest.mark.parametrize("V", [37, 65, 260, 512, 1024, 2048, 2049, 2052, 5000])
def test_teacher_forced_eval_ties_take_the_smaller_index(V):
    rng = np.random.default_rng(V)
    rows = _tie_rows(V, rng)
    x = np.stack([r for _, _, r in rows])[None]                       # (1, rows, V)
    tgt = np.array([[(a if k % 2 else b) or 1 for k, (a, b, _) in enumerate(rows)]], np.int32)   # first / second index
    tgt[0, -1] = 5
    want = _np_eval(x, tgt, 0, 0.1)
    assert want["ids"][0].tolist() == [a for a, _, _ in rows]
    for misalign in ([False, True] if V % 4 == 0 else [False]):       # the vector and the scalar path
        _check(_run(x, tgt, 0, 0.1, misalign=misalign), want, (V, misalign))


# --------------------------------------------------------------------------- non-finite logits
NONFINITE = ["one_nan", "two_nan", "all_nan", "all_ninf", "ninf_elsewhere", "ninf_at_target", "one_pinf", "two_pinf"]
NF_TARGET = 3


def _nonfinite_row(kind, V, rng):
    """One row of the kinds above; NF_TARGET is its (kept) target.  A large finite value stands before the first NaN and
    a larger one behind it, so an ordering that skips NaN or takes the last one answers differently."""
    r = rng.standard_normal(V).astype(np.float32)
    if kind == "one_nan":
        r[1], r[V // 2], r[V - 2] = 30.0, NAN, 40.0
    elif kind == "two_nan":
        r[1], r[V // 3], r[V - 2], r[V - 1] = 30.0, NAN, 40.0, NAN
    elif kind == "all_nan":
        r[:] = NAN
    elif kind == "all_ninf":
        r[:] = -INF
    elif kind == "ninf_elsewhere":
        r[[1, V // 2, V - 1]] = -INF
    elif kind == "ninf_at_target":
        r[NF_TARGET] = -INF
    elif kind == "one_pinf":
        r[V // 2] = INF
    elif kind == "two_pinf":
        r[V // 4], r[V - 2] = INF, INF
    else:
        raise KeyError(kind)
    return r


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [65, 512, 2052])
@pytest.mark.parametrize("kind", NONFINITE)
def test_teacher_forced_eval_non_finite_logits(kind, V, eps):
    rng = np.random.default_rng(V + len(kind))
    x = rng.standard_normal((2, 3, V)).astype(np.float32)
    x[1, 1] = _nonfinite_row(kind, V, rng)
    tgt = rng.integers(1, V, size=(2, 3)).astype(np.int32)
    for target in (NF_TARGET, 0):                                     # kept, then a pad target: the row adds 0
        tgt[1, 1] = target
        want = _torch_eval(x, tgt, 0, eps)
        if target == 0:
            assert np.isfinite(want["loss"])
        for misalign in ([False, True] if V % 4 == 0 else [False]):
            _check(_run(x, tgt, 0, eps, misalign=misalign), want, (kind, V, eps, target, misalign),
                   "teacher_forced_eval loss sum [rel] beside a non-finite row")


# --------------------------------------------------------------------------- masked accuracy
def _torch_masked_accuracy(logits, targets, pad):
    """metrics.py:226-238 on the CPU: torch.argmax, eq, mask."""
    lg, tg = torch.from_numpy(logits), torch.from_numpy(targets)
    mask = tg.ne(pad)
    return int((lg.argmax(-1).eq(tg) & mask).sum()), int(mask.sum())


def _nonfinite_batch(V):
    rng = np.random.default_rng(V)
    logits = np.stack([_nonfinite_row(k, V, rng) for k in NONFINITE])
    return logits, torch.from_numpy(logits).argmax(-1).numpy().astype(np.int64)


@pytest.mark.parametrize("V", [65, 512, 2052])
def test_oracle_masked_accuracy_states_torch_argmax_on_non_finite_rows(V):
    """No GPU: the oracle's arg max is torch.argmax's (NaN above everything, the first of equals) on the rows that the
    device tests feed, so comparing a kernel with the oracle compares it with the reference's formula."""
    logits, arg = _nonfinite_batch(V)
    assert arg.tolist()[:4] == [V // 2, V // 3, 0, 0] and arg[6:].tolist() == [V // 2, V // 4]
    n = len(NONFINITE)
    for targets in (arg, (arg + 1) % V, np.where(np.arange(n) % 2 == 0, arg, 0), np.zeros(n, np.int64)):
        for pad in (0, 3, -100):
            want = _torch_masked_accuracy(logits, targets, pad)
            assert MO.masked_accuracy(logits, targets, pad) == want, (V, pad, targets.tolist())
    assert MO.masked_accuracy(logits, arg, -100) == (n, n)


def _device_masked_accuracy(logits, targets, pad):
    from img2latex_amd.training import metrics as M
    return M.masked_accuracy(torch.from_numpy(logits).to(DEV), torch.from_numpy(targets).to(DEV), pad)


def _ma_case(V, rows, seed, pad):
    """Logits in quarters (ties occur unplanted), the tie plantings with the target once at the first and once at the
    second index, the maximum at the last index in every seventh row; a target is the row's arg max in about half of the
    rows, pad in a tenth, and 2**32 + arg max (equal in its low 32 bits only) in every eleventh."""
    rng = np.random.default_rng(seed)
    logits = (np.round(rng.standard_normal((rows, V)) * 4.0) / 4.0).astype(np.float32)
    logits[::7, V - 1] = logits[::7].max(-1) + 0.25
    ties = _tie_rows(V, rng, quarters=True)
    targets = rng.integers(0, V, size=rows).astype(np.int64)
    arg = np.argmax(logits, -1)
    pick = rng.random(rows) < 0.5
    targets[pick] = arg[pick]
    for k, (a, b, r) in enumerate(ties):
        logits[2 * k], logits[2 * k + 1] = r, r
        targets[2 * k], targets[2 * k + 1] = a, b
    arg = np.argmax(logits, -1)
    targets[5::11] = 2 ** 32 + arg[5::11]
    targets[rng.random(rows) < 0.1] = pad
    return logits, targets


@gpu
@pytest.mark.parametrize("pad", [0, 3, -100])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 127, 500])
def test_masked_accuracy_vs_torch_argmax(V, pad):
    logits, targets = _ma_case(V, 300, seed=V * 7 + pad % 5, pad=pad)
    want = _torch_masked_accuracy(logits, targets, pad)
    assert MO.masked_accuracy(logits, targets, pad) == want
    assert _device_masked_accuracy(logits, targets, pad) == want, (V, pad)
    assert _device_masked_accuracy(logits, np.full_like(targets, pad), pad) == (0, 0)   # an all-pad batch


@gpu
@pytest.mark.parametrize("pad", [0, 3, -100])
def test_masked_accuracy_grid_stride_rows(pad):
    """16384 + 7 rows: the launch is capped at 4096 workgroups of 4 waves, so the last 7 rows are second rows of their
    waves.  They are decisive: a tie whose first index is the target, a maximum at the last index, a target that is the
    second index of a tie (wrong) -- the total count is right only when they are read, and read correctly."""
    V, rows = 5, 16384 + 7
    logits, targets = _ma_case(V, rows, seed=11 + pad % 5, pad=pad)
    tail = np.array([[1, 2, 2, 0, 0], [0, 0, 0, 0, 3], [2, 2, 2, 2, 2], [0, 1, 0, 1, 0], [0, 0, 4, 0, 4],
                     [-1, -2, -3, -4, -0.5], [3, 0, 3, 0, 0]], np.float32)
    logits[-7:] = tail
    targets[-7:] = [1, 4, 0, 1, 2, 4, 2]                             # the last one: the second index of its tie
    if pad == 0:
        targets[-5] = 1                                              # the all-equal row: index 0 is pad here
    want = _torch_masked_accuracy(logits, targets, pad)
    head = _torch_masked_accuracy(logits[:-7], targets[:-7], pad)
    assert (want[0] - head[0], want[1] - head[1]) == ((5, 7) if pad == 0 else (6, 7))
    assert _device_masked_accuracy(logits, targets, pad) == want


@gpu
@pytest.mark.parametrize("V", [65, 512, 2052])
def test_masked_accuracy_non_finite_rows(V):
    logits, arg = _nonfinite_batch(V)
    n = len(NONFINITE)
    assert _torch_masked_accuracy(logits, arg, -100) == (n, n)
    assert _device_masked_accuracy(logits, arg, -100) == (n, n)       # every row counts as correct
    assert _device_masked_accuracy(logits, (arg + 1) % V, -100) == (0, n)


# --------------------------------------------------------------------------- Validator on non-finite batches
class _StubModel(torch.nn.Module):
    """Returns prepared logits: images carry the batch index.  ``nan_rows`` = {batch: [(b, t), ...]} are overwritten
    with NaN whenever decoder.kernel_flags lacks FLAG_NO_GROUP -- NaN as data, nothing times out."""

    def __init__(self, logits, nan_rows=None, flags=0):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.model_type = "cnn_lstm"
        self.decoder = types.SimpleNamespace(kernel_flags=flags)
        self.logits = [torch.from_numpy(l).to(DEV) for l in logits]
        self.nan_rows = nan_rows or {}
        self.calls = []

    def forward(self, images, formulas):
        i = int(images.reshape(-1)[0])
        flags = int(self.decoder.kernel_flags)
        self.calls.append((i, flags))
        out = self.logits[i].clone()
        if not flags & _lib.FLAG_NO_GROUP:
            for b, t in self.nan_rows.get(i, []):
                out[b, t] = NAN
        return out


VAL_V, VAL_T, VAL_PAD = 37, 9, 0
VAL_SIZES = [4, 3, 5, 2, 6, 3, 1]


def _val_batches(seed=5):
    rng = np.random.default_rng(seed)
    logits, loader = [], []
    for i, B in enumerate(VAL_SIZES):
        x = (rng.standard_normal((B, VAL_T, VAL_V)) * 2.0).astype(np.float32)
        forms = rng.integers(1, VAL_V, size=(B, VAL_T + 1)).astype(np.int64)
        for b in range(B):
            forms[b, 1 + rng.integers(3, VAL_T + 1):] = VAL_PAD       # ragged, at least 3 kept targets
        hot = rng.random((B, VAL_T)) < 0.6                            # a prediction that is often right
        bb, tt = np.nonzero(hot)
        x[bb, tt, forms[bb, tt + 1]] += 6.0
        logits.append(x)
        loader.append({"images": torch.full((B, 1, 2, 2), float(i)), "formulas": torch.from_numpy(forms)})
    return logits, loader


def _val_loss_float64(logits, loader, eps):
    """sum(mean_b * B_b) / sum(B_b) from per-batch float64 means; val_acc's exact counts."""
    num = den = correct = total = 0
    for x, batch in zip(logits, loader):
        want = _np_eval(x, batch["formulas"][:, 1:].numpy().astype(np.int32), VAL_PAD, eps)
        num += want["loss"] / want["count"] * x.shape[0]
        den += x.shape[0]
        correct += want["correct"]
        total += want["total"]
    return num / den, correct / total


@gpu
def test_validate_repeats_a_non_finite_pass_without_grouped_kernels():
    from img2latex_amd.training import validate
    logits, loader = _val_batches()
    clean = _StubModel(logits)
    rng = random.Random(5)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        want = validate(clean, loader, VAL_PAD, bleu_batches=2, label_smoothing=0.1, rng=rng, epoch=3, step=40)
    assert clean.calls == [(i, 0) for i in range(len(loader))]
    end_state = rng.getstate()
    # a kept-target row of batches 2 and 6 turns NaN under the grouped flags
    bad = _StubModel(logits, {2: [(1, 0)], 6: [(0, 1)]}, flags=_lib.FLAG_EXACT_FP32)
    rng = random.Random(5)
    with pytest.warns(RuntimeWarning, match="repeating the pass"):
        got = validate(bad, loader, VAL_PAD, bleu_batches=2, label_smoothing=0.1, rng=rng, epoch=3, step=40)
    n = len(loader)
    assert bad.calls == [(i, _lib.FLAG_EXACT_FP32) for i in range(n)] + \
        [(i, _lib.FLAG_EXACT_FP32 | _lib.FLAG_NO_GROUP) for i in range(n)]                  # repeated once
    assert bad.decoder.kernel_flags == _lib.FLAG_EXACT_FP32                                # put back
    assert got == want and np.isfinite(got["val_loss"])
    assert rng.getstate() == end_state          # restored before the repeat: the same draws, the same batches sampled
    loss64, acc = _val_loss_float64(logits, loader, 0.1)
    err = abs(got["val_loss"] - loss64) / abs(loss64)
    record("validate val_loss [rel] stub, unequal batches", err)
    assert err <= LOSS_TOL and got["val_acc"] == acc and got["val_samples"] == sum(VAL_SIZES)


@gpu
def test_validator_nan_in_pad_rows_and_under_no_group():
    from img2latex_amd.training import ValidationTimeout, Validator, validate
    logits, loader = _val_batches()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        want = validate(_StubModel(logits), loader, VAL_PAD, 2, 0.1, rng=random.Random(5))
        # NaN confined to pad-target rows: they add 0 to the loss and are not counted
        forms = loader[2]["formulas"].numpy()
        pads = [(b, t) for b in range(forms.shape[0]) for t in range(VAL_T) if forms[b, t + 1] == VAL_PAD]
        assert len(pads) >= 2
        stub = _StubModel(logits, {2: pads})
        got = validate(stub, loader, VAL_PAD, 2, 0.1, rng=random.Random(5))
        assert len(stub.calls) == len(loader)                         # one pass
        assert got["val_loss"] == want["val_loss"] and got["val_acc"] == want["val_acc"]
    # FLAG_NO_GROUP already set: nothing to repeat; the NaN loss is reported with a warning
    always = _StubModel(logits, flags=_lib.FLAG_NO_GROUP)
    always.logits[2][1, 0] = NAN
    with pytest.warns(RuntimeWarning, match="not finite"):
        got = validate(always, loader, VAL_PAD, 2, 0.1, rng=random.Random(5))
    assert np.isnan(got["val_loss"]) and len(always.calls) == len(loader)
    assert always.decoder.kernel_flags == _lib.FLAG_NO_GROUP
    # the Validator itself raises, naming the batches
    v = Validator(_StubModel(logits, {2: [(1, 0)], 6: [(0, 1)]}), VAL_PAD, len(loader), 2, 0.1, rng=random.Random(5))
    for b in loader:
        v.add(b["images"], b["formulas"])
    with pytest.raises(ValidationTimeout) as exc:
        v.finish()
    assert exc.value.batches == [2, 6]


@gpu
def test_validator_unequal_batches_and_record_growth():
    from img2latex_amd.training import Validator
    logits, loader = _val_batches(seed=9)
    assert VAL_SIZES[-1] == 1 and len(set(VAL_SIZES)) > 3

    def run(batches, announced, eps):
        v = Validator(_StubModel(logits), VAL_PAD, announced, bleu_batches=len(batches), label_smoothing=eps,
                      rng=random.Random(1))
        for b in batches:
            v.add(b["images"], b["formulas"])
        assert v.sampled == list(range(len(batches)))
        return v.finish(1, 2)

    for eps in (0.0, 0.1):
        for first in (0, 2):                                          # all seven batches; the last five
            loss64, acc = _val_loss_float64(logits[first:], loader[first:], eps)
            full = run(loader[first:], len(loader) - first, eps)
            err = abs(full["val_loss"] - loss64) / abs(loss64)
            record("validate val_loss [rel] stub, unequal batches", err)
            assert err <= LOSS_TOL, (full["val_loss"], loss64)
            assert full["val_acc"] == acc and full["val_samples"] == sum(VAL_SIZES[first:])
        # five adds where one batch was announced: the device record grows 1 -> 2 -> 4 -> 8 under the queued kernels
        assert len(loader[2:]) == 5 and run(loader[2:], 1, eps) == full
