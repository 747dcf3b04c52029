"""Distillation on the GPU: i2l_ce_distill_fwd_bwd through the C ABI against the float64 restatement (distill_ref),
its identities, its wiring through TrainStep / Teacher, a student that learns from a teacher, and the CLI.

Tolerance: the rule of test_small_entries_vs_float64.py -- the same formulas are evaluated in float32 on the CPU
(distill_ref.distill_torch, float32) and err <= 4 * err_fp32cpu + floor, a row's dlogits taking the row's largest fp32
error.  The floors and their derivation are distill_ref.floors': 2^-22 (alpha + (1 - alpha) tau) on dlogits, 2^-21 x the
summed magnitudes of the terms that enter each of the three sums.  Both errors are record()ed in units of the floor.
Outputs start as NaN and sit between sentinel elements that must survive the call."""
import copy
import os

import numpy as np
import pytest
import torch

import distill_cases as C
import distill_ref as R
from conftest import record
from img2latex_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK = 0
TAIL = 64
RULE_IDS = {"logprob": _lib.ENSEMBLE_LOGPROB, "prob": _lib.ENSEMBLE_PROB}
ROWS, VS, MS = (1, 5, 257), (1, 3, 64, 65, 512, 513, 1025), (1, 2, 3, 8)
TAUS, ALPHAS, EPSS = (0.5, 1.0, 2.0, 4.0), (0.0, 0.3, 1.0), (0.0, 0.1)


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


def distill_call(x, tgt, pad, eps, z, weights, rule, tau, alpha, ld_extra=0, want_d=True, want_parts=True):
    """x (rows, V), z (M, rows, V) numpy fp32 -> (out (2), parts (2) or None, d (rows, V) or None) as float64 numpy.
    A teacher's rows are stored ``V + ld_extra`` apart, the columns in between NaN."""
    L = _lib.lib()
    rows, V = x.shape
    M = z.shape[0]
    X, T = Buf(torch.from_numpy(x)), Buf(torch.from_numpy(np.asarray(tgt)).to(torch.int32))
    Z, recs = [], (_lib.DistillTeacher * M)()
    for m in range(M):
        wide = nans(rows, V + ld_extra)
        wide[:, :V] = torch.from_numpy(z[m])
        Z.append(Buf(wide, off=m))
        recs[m] = _lib.DistillTeacher(Z[m].ptr(), V + ld_extra, float(weights[m]))
    D = Buf(nans(rows, V)) if want_d else None
    P = Buf(nans(2)) if want_parts else None
    out = Buf(nans(2))
    nbytes = L.i2l_ce_distill_workspace_bytes(rows)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    rc = L.i2l_ce_distill_fwd_bwd(X.ptr(), T.ptr(), rows, V, pad, eps, recs, M, RULE_IDS[rule], tau, alpha, ws.data_ptr(),
                                  nbytes, D.ptr() if want_d else None, out.ptr(), P.ptr() if want_parts else None,
                                  _lib.stream_ptr())
    assert rc == OK, rc
    res = (out.get().double().numpy(), P.get().double().numpy() if want_parts else None,
           D.get().reshape(rows, V).double().numpy() if want_d else None)
    for b in [X, T] + Z:
        b.get()                                                         # the inputs' sentinels too
    return res


def judge(name, err, err_cpu, floor, what, share_row=False):
    """err <= 4 * err_fp32cpu + floor; both recorded in units of the floor."""
    err, err_cpu, floor = (np.asarray(t, dtype=np.float64) for t in (err, err_cpu, floor))
    floor = floor + 1e-300
    record(f"distill gpu {name} err_hip [floors]", float((err / floor).max()))
    record(f"distill gpu {name} err_fp32cpu [floors]", float((err_cpu / floor).max()))
    if share_row:
        err_cpu = err_cpu.max(axis=-1, keepdims=True)
    assert np.isfinite(err).all(), (name, what)
    over = err - (4 * err_cpu + floor)
    assert float(over.max()) <= 0, (name, what, float((err / floor).max()), float((err_cpu / floor).max()))


def sum32(a):
    return float(np.asarray(a).astype(np.float32).sum(dtype=np.float32))


def check(family, x, tgt, pad, eps, z, weights, rule, tau, alpha, ld_extra, what, nulls=True):
    """One call against float64: count, pad rows, dlogits, the three sums, a kept row's dlogits summing to zero, and --
    with ``nulls`` -- the same sums without dlogits_out and / or parts_out."""
    rows, V = x.shape
    keep = np.asarray(tgt) != pad
    zp = z.copy()
    zp[:, ~keep] = np.nan                                               # whatever the teachers hold at pad rows is not read
    out, parts, d = distill_call(x, tgt, pad, eps, zp, weights, rule, tau, alpha, ld_extra)
    if nulls:
        for want_d, want_parts in ((False, True), (True, False), (False, False)):
            o, p, _ = distill_call(x, tgt, pad, eps, zp, weights, rule, tau, alpha, ld_extra, want_d, want_parts)
            assert np.array_equal(o, out) and (p is None or np.array_equal(p, parts)), (what, want_d, want_parts)
    assert out[1] == float(keep.sum()), what                            # an exact integer
    assert np.isfinite(out).all() and np.isfinite(parts).all() and np.isfinite(d).all(), what
    assert not d[~keep].any(), what                                     # +0 or -0: exactly zero
    if not keep.any():
        assert not out.any() and not parts.any() and not d.any(), what
        return out, parts, d
    ref = R.distill_np(x, z, weights, rule, tgt, pad, tau, alpha, eps)
    cpu = R.distill_torch(x, z, weights, rule, tgt, pad, tau, alpha, eps, torch.float32)
    d_floor, hard_floor, soft_floor = R.floors(x, ref["y"], tgt, pad, tau, alpha, eps)
    a = R.f32(alpha)
    judge(f"{family} dlogits", np.abs(d - ref["d"]), np.abs(cpu["d"] - ref["d"]), d_floor, what, share_row=True)
    hard64, soft64 = ref["hard"].sum(), ref["soft"].sum()
    hard32, soft32 = sum32(cpu["hard"]), sum32(cpu["soft"])
    judge(f"{family} hard sum", abs(parts[0] - hard64), abs(hard32 - hard64), hard_floor.sum(), what)
    judge(f"{family} soft sum", abs(parts[1] - soft64), abs(soft32 - soft64), soft_floor.sum(), what)
    loss64, loss32 = a * hard64 + (1 - a) * soft64, float(np.float32(a * hard32 + (1 - a) * soft32))
    judge(f"{family} loss sum", abs(out[0] - loss64), abs(loss32 - loss64), a * hard_floor.sum() + (1 - a) * soft_floor.sum(), what)
    # the loss sum is alpha parts[0] + (1 - alpha) parts[1] up to rounding: of the two parts and of the result
    assert abs(out[0] - (a * parts[0] + (1 - a) * parts[1])) <= 2.0 ** -22 * (a * abs(parts[0]) + (1 - a) * abs(parts[1])), what
    sums = np.abs(d.sum(axis=1))[keep]                                  # the softmaxes sum to 1, the target terms to 1
    bound = V * 2.0 ** -23 * (a + (1 - a) * R.f32(tau))
    record(f"distill gpu {family} |sum_v dlogits| [V x 2^-23 (alpha + (1 - alpha) tau)]", float(sums.max()) / bound)
    assert float(sums.max()) <= bound, what
    return out, parts, d


def operands(rows, V, M, pad, seed, scale=3.0):
    """x (rows, V), z (M, rows, V), weights (M), targets in [0, V) with every fifth row (from row 1) the pad id."""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((rows, V))).astype(np.float32)
    z = (scale * rng.standard_normal((M, rows, V))).astype(np.float32)
    tgt = rng.integers(0, V, rows)
    tgt[1::5] = pad
    return x, z, rng.uniform(0.2, 3.0, M).astype(np.float32), tgt


# ---------------------------------------------------------------------------------------------------------------
# 1. the shape sweep: rows around the 4-rows-per-workgroup grid and the 256-thread stride of the ordered sum, V on both
#    sides of the 64-lane stride and of the 512-column chunk (one, two and three chunks), every M the dispatch names at
#    its ends and in between.  Per case: both rules x (pad 0 with ld == V, pad -100 with ld == V + 7); temperature, alpha
#    and smoothing rotate through the issue's values across the sweep.
# ---------------------------------------------------------------------------------------------------------------
SWEEP = [(r, V, M) for r in ROWS for V in VS for M in MS]


@pytest.mark.parametrize("rows,V,M", SWEEP)
def test_shapes_vs_float64(rows, V, M):
    case = SWEEP.index((rows, V, M))
    for c, (rule, (pad, ld_extra)) in enumerate((r, p) for r in ("logprob", "prob") for p in ((0, 0), (-100, 7))):
        n = 4 * case + c
        tau, alpha, eps = TAUS[n % 4], ALPHAS[(n // 4) % 3], EPSS[(n // 12) % 2]
        x, z, w, tgt = operands(rows, V, M, pad, 1000 * n + V)
        check("shapes", x, tgt, pad, eps, z, w, rule, tau, alpha, ld_extra, (rows, V, M, rule, pad, ld_extra, tau, alpha, eps))


@pytest.mark.parametrize("V", [65, 513, 1025])
def test_extreme_logits_vs_float64(V):
    """Logits scaled by 30 and a row with one logit at +1e4 (student and teacher 0, different columns)."""
    for M, rule, tau, alpha in ((1, "logprob", 0.5, 0.0), (3, "prob", 2.0, 0.3), (2, "logprob", 4.0, 0.3)):
        x, z, w, tgt = operands(6, V, M, -100, 50 + V + M, scale=30.0)
        x[2], z[:, 2] = x[2] / 10, z[:, 2] / 10
        x[2, V // 3], z[0, 2, (2 * V) // 3] = 1e4, 1e4
        check("extreme", x, tgt, -100, 0.1, z, w, rule, tau, alpha, 0, (V, M, rule, tau, alpha), nulls=False)


# ---------------------------------------------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,V", [(5, 65), (257, 513), (5, 1025)])
def test_alpha_one_is_the_plain_cross_entropy(rows, V):
    """alpha = 1: every output agrees with i2l_ce_label_smooth_fwd_bwd on the same inputs within twice the floor (both
    are within one floor of float64)."""
    L = _lib.lib()
    for pad, eps in ((0, 0.1), (-100, 0.0)):
        x, z, w, tgt = operands(rows, V, 2, pad, 7 * rows + V)
        out, parts, d = distill_call(x, tgt, pad, eps, z, w, "prob", 2.0, 1.0)
        X, T = Buf(torch.from_numpy(x)), Buf(torch.from_numpy(tgt).to(torch.int32))
        D, O = Buf(nans(rows, V)), Buf(nans(2))
        nbytes = L.i2l_ce_workspace_bytes(rows)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        assert L.i2l_ce_label_smooth_fwd_bwd(X.ptr(), T.ptr(), rows, V, pad, eps, ws.data_ptr(), nbytes, D.ptr(), O.ptr(),
                                             _lib.stream_ptr()) == OK
        ce_out, ce_d = O.get().double().numpy(), D.get().reshape(rows, V).double().numpy()
        ref = R.distill_np(x, z, w, "prob", tgt, pad, 2.0, 1.0, eps)
        d_floor, hard_floor, _ = R.floors(x, ref["y"], tgt, pad, 2.0, 1.0, eps)
        assert d_floor == 2.0 ** -22
        assert out[1] == ce_out[1]
        assert np.abs(d - ce_d).max() <= 2 * d_floor, (rows, V, pad, float(np.abs(d - ce_d).max()) / d_floor)
        assert abs(out[0] - ce_out[0]) <= 2 * hard_floor.sum() and abs(parts[0] - ce_out[0]) <= 2 * hard_floor.sum()
        record("distill gpu alpha = 1 vs ce: dlogits [floors]", float(np.abs(d - ce_d).max()) / d_floor)
        record("distill gpu alpha = 1 vs ce: loss sum [floors]", abs(out[0] - ce_out[0]) / hard_floor.sum())


@pytest.mark.parametrize("rows,V", [(5, 65), (9, 513), (5, 1025)])
def test_teacher_equal_to_student_has_no_soft_loss(rows, V):
    """Teacher == student logits, M = 1, alpha = 0: parts[1] within its floor of 0 and dlogits within its floor of 0."""
    for tau in (0.5, 2.0):
        x, _, _, tgt = operands(rows, V, 1, 0, 3 * rows + V)
        out, parts, d = distill_call(x, tgt, 0, 0.1, x[None].copy(), [1.0], "logprob", tau, 0.0)
        ref = R.distill_np(x, x[None], [1.0], "logprob", tgt, 0, tau, 0.0, 0.1)
        d_floor, _, soft_floor = R.floors(x, ref["y"], tgt, 0, tau, 0.0, 0.1)
        assert abs(parts[1]) <= soft_floor.sum() and abs(out[0]) <= soft_floor.sum(), (rows, V, tau, parts[1])
        assert np.abs(d).max() <= d_floor, (rows, V, tau, float(np.abs(d).max()) / d_floor)
        assert parts[0] > 0 and out[1] == float((tgt != 0).sum())


@pytest.mark.parametrize("V", [65, 513])
def test_all_pad_batch_is_exactly_zero(V):
    for pad in (0, -100):
        x, z, w, tgt = operands(9, V, 2, pad, V)
        tgt[:] = pad
        check("all pad", x, tgt, pad, 0.1, z, w, "logprob", 2.0, 0.3, 0, (V, pad))


# ---------------------------------------------------------------------------------------------------------------
# 3. wiring through TrainStep
# ---------------------------------------------------------------------------------------------------------------
def model_of(cfg, sd):
    from img2latex_amd import synth
    from img2latex_amd.model import Seq2SeqModel
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return m.to(DEV)


def recording(teacher):
    """The teacher with its ``logits`` wrapped: what TrainStep was given is kept in the returned list."""
    seen, inner = [], teacher.logits

    def logits(images, formulas):
        seen.append(inner(images, formulas))
        return seen[-1]
    teacher.logits = logits
    return seen


@pytest.mark.parametrize("V", [513, 3])
@pytest.mark.parametrize("members", [1, 2])
def test_train_step_wiring_vs_float64(V, members):
    """From the logits forward_backward returns and the logits the teacher gave it, the float64 rule must reproduce
    flat_grads[n], [n + 1], the parts and the output layer's bias gradient (the column sum of dlogits: its floor is rows
    times the dlogits floor)."""
    from img2latex_amd.model import EnsembleModel
    from img2latex_amd.training import Teacher, TrainStep
    (scfg, ssd), teachers, images, formulas = C.wiring_case(V)
    student = model_of(scfg, ssd)
    models = [model_of(cfg, sd) for cfg, sd in teachers[:members]]
    weights, rule = ([1.0], "logprob") if members == 1 else ([2.0, 1.0], "prob")
    teacher = Teacher(models[0]) if members == 1 else Teacher(EnsembleModel(models, weights=weights, combine=rule))
    seen = recording(teacher)
    tau, alpha, eps = 2.0, 0.3, 0.1
    ts = TrainStep(student, pad_token_id=C.PAD, label_smoothing=eps, seed=5, teacher=teacher, distill_alpha=alpha,
                   distill_temperature=tau)
    x_img, forms = torch.from_numpy(images).to(DEV), torch.from_numpy(formulas).to(DEV)
    student.train()
    logits = ts.forward_backward(x_img, forms)
    torch.cuda.synchronize()
    B, T = C.WIRING_B, C.WIRING_T
    assert tuple(logits.shape) == (B, T, V) and len(seen) == 1 and len(seen[0]) == members
    for lg in seen[0]:
        assert tuple(lg.shape) == (B, T, V) and lg.dtype == torch.float32 and lg.is_cuda and not lg.requires_grad
    x = logits.detach().cpu().numpy().reshape(B * T, V)
    z = np.stack([lg.cpu().numpy().reshape(B * T, V) for lg in seen[0]])
    tgt = formulas[:, 1:].reshape(-1)
    ref = R.distill_np(x, z, weights, rule, tgt, C.PAD, tau, alpha, eps)
    cpu = R.distill_torch(x, z, weights, rule, tgt, C.PAD, tau, alpha, eps, torch.float32)
    d_floor, hard_floor, soft_floor = R.floors(x, ref["y"], tgt, C.PAD, tau, alpha, eps)
    a = R.f32(alpha)
    tail = ts.flat_grads[ts.n:ts.n + 2].cpu().double().numpy()
    parts = ts.loss_parts.cpu().double().numpy()
    what = (V, members)
    assert tail[1] == float(ref["keep"].sum()) and tail[1] > 0
    hard64, soft64, hard32, soft32 = ref["hard"].sum(), ref["soft"].sum(), sum32(cpu["hard"]), sum32(cpu["soft"])
    judge("wiring hard sum", abs(parts[0] - hard64), abs(hard32 - hard64), hard_floor.sum(), what)
    judge("wiring soft sum", abs(parts[1] - soft64), abs(soft32 - soft64), soft_floor.sum(), what)
    judge("wiring loss sum", abs(tail[0] - (a * hard64 + (1 - a) * soft64)),
          abs(float(np.float32(a * hard32 + (1 - a) * soft32)) - (a * hard64 + (1 - a) * soft64)),
          a * hard_floor.sum() + (1 - a) * soft_floor.sum(), what)
    bias = ts.grad_views["decoder.output_layer.bias"].cpu().double().numpy()
    bias64, bias32 = ref["d"].sum(axis=0), cpu["d"].astype(np.float32).sum(axis=0, dtype=np.float32).astype(np.float64)
    judge("wiring bias gradient", np.abs(bias - bias64), np.abs(bias32 - bias64).max(), B * T * d_floor, what)
    assert soft64 > 0.01 * hard64                                      # the teachers differ from the student: the soft part is live


@pytest.mark.parametrize("V", [513, 3])
def test_self_distillation_has_no_soft_loss(V):
    """The teacher is a deep copy of the student: soft_loss < 1e-3 hard_loss (the training forward and the teacher's eval
    forward are different kernels, so not exactly 0).  A wiring check, not a precision check: a teacher read one position
    off gives more than 0.1 hard_loss -- asserted here on the float64 restatement of the device's logits, and on the CPU
    with the oracle's logits where the seeds were picked (test_distill_host.py::test_shifted_teacher_shows_in_float64)."""
    from img2latex_amd.training import Teacher, TrainStep
    cfg, sd, images, formulas = C.self_case(V)
    student = model_of(cfg, sd)
    teacher = Teacher(copy.deepcopy(student))
    ts = TrainStep(student, pad_token_id=C.PAD, seed=5, teacher=teacher, distill_alpha=0.5, distill_temperature=C.SELF_TAU)
    x_img, forms = torch.from_numpy(images).to(DEV), torch.from_numpy(formulas).to(DEV)
    out = ts.step(x_img, forms)
    hard, soft = float(out["hard_loss"]), float(out["soft_loss"])
    record("distill gpu self-distillation soft / hard", soft / hard)
    assert np.isfinite(hard) and hard > 0 and abs(soft) < 1e-3 * hard, (hard, soft)
    assert abs(float(out["loss"]) - (0.5 * hard + 0.5 * soft)) <= 1e-5 * hard
    with torch.no_grad():
        z = teacher.logits(x_img, forms)[0].cpu().numpy()
    B, T = C.WIRING_B, C.WIRING_T
    tgt = formulas[:, 1:].reshape(-1)
    off = R.distill_np(z.reshape(B * T, V), np.roll(z, 1, axis=1).reshape(1, B * T, V), [1.0], "logprob", tgt, C.PAD,
                       C.SELF_TAU, 0.5, 0.1)
    assert off["soft"].sum() > 0.1 * off["hard"].sum()


def test_without_a_teacher_nothing_changes():
    """teacher=None: flat_grads (gradients, loss sum, count) bit-identical to a TrainStep built without the keyword, and no
    new keys in the step's result."""
    from img2latex_amd.training import TrainStep
    (scfg, ssd), _, images, formulas = C.wiring_case(513)
    x_img, forms = torch.from_numpy(images).to(DEV), torch.from_numpy(formulas).to(DEV)
    runs = []
    for kw in ({}, dict(teacher=None, distill_alpha=0.25, distill_temperature=3.0)):
        m = model_of(scfg, ssd)
        m.train()
        ts = TrainStep(m, pad_token_id=C.PAD, seed=5, **kw)
        ts.forward_backward(x_img, forms)
        torch.cuda.synchronize()
        runs.append(ts.flat_grads.clone())
        assert ts.loss_parts is None
        assert set(ts.step(x_img, forms)) == {"loss", "total_norm", "count", "skipped"}
    assert torch.equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------------------
# 4. it learns
# ---------------------------------------------------------------------------------------------------------------
def test_student_learns_the_teachers_distribution():
    """alpha = 0, random hard targets: after 40 steps on one fixed batch soft_loss is below its first value and the
    student's arg max agrees with the teacher's on more positions than before the first step.  The seeds were picked on the
    float64 restatement on the CPU (test_distill_host.py::test_learning_seed_holds_in_float64: soft 0.19 -> 0.0007,
    agreement 3 -> 31 of 32)."""
    from img2latex_amd.training import Teacher, TrainStep
    c = C.LEARN
    scfg, ssd, tcfg, tsd, images, formulas = C.learn_case()
    student, teacher = model_of(scfg, ssd), Teacher(model_of(tcfg, tsd))
    ts = TrainStep(student, lr=c["lr"], pad_token_id=C.PAD, label_smoothing=c["eps"], seed=3, teacher=teacher,
                   distill_alpha=c["alpha"], distill_temperature=c["tau"])
    x_img, forms = torch.from_numpy(images).to(DEV), torch.from_numpy(formulas).to(DEV)
    want = teacher.logits(x_img, forms)[0].argmax(-1)
    student.train()
    before = int((ts.forward_backward(x_img, forms).argmax(-1) == want).sum())
    softs = [ts.step(x_img, forms)["soft_loss"] for _ in range(c["steps"])]
    after = int((ts.forward_backward(x_img, forms).argmax(-1) == want).sum())
    softs = [float(s) for s in softs] + [float(ts._loss_parts()["soft_loss"])]
    print(f"soft {softs[0]:.4f} -> {softs[-1]:.5f}, arg max agreement {before} -> {after} of {want.numel()}")
    assert all(np.isfinite(softs)) and softs[-1] < softs[0], softs[::8]
    assert after > before, (before, after)


# ---------------------------------------------------------------------------------------------------------------
# 5. the CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cli_train_with_a_teacher(tmp_path, capsys):
    import yaml
    from img2latex_amd import cli, synth
    from img2latex_amd.training import Predictor, TokenTable, save_checkpoint
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, 50)})                    # the synthetic run's vocabulary
    tcfg = synth.model_config(vocab_size=50, embedding_dim=16, hidden_dim=128, lstm_layers=2, attention=True, **C.TINY)
    teacher_config = {"model": {"name": "cnn_lstm", "embedding_dim": 16, "encoder": {"cnn": synth.encoder_params(tcfg)},
                                "decoder": synth.decoder_params(tcfg)}}
    teacher_path = str(tmp_path / "teacher.pt")
    save_checkpoint(teacher_path, model_of(tcfg, synth.make_state_dict(tcfg, seed=9, out_scale=4.0, enc_scale=16.0)),
                    TokenTable(vocab, max_sequence_length=20), teacher_config)
    config = {
        "model": {"name": "cnn_lstm", "embedding_dim": 32,
                  "encoder": {"cnn": {"img_height": 16, "img_width": 32, "channels": 1, "conv_filters": [4, 8, 16],
                                      "kernel_size": 3, "pool_size": 2, "padding": "same"}},
                  "decoder": {"hidden_dim": 64, "lstm_layers": 1, "dropout": 0.1, "attention": False, "max_seq_length": 20}},
        "data": {"batch_size": 4, "max_seq_length": 20},
        "training": {"device": "cuda", "epochs": 1, "learning_rate": 1e-3, "weight_decay": 0.0, "accumulation_steps": 1},
    }
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(config))
    out_dir = tmp_path / "outputs"
    assert cli.main(["train", "--config-path", str(path), "--experiment-name", "distil", "--device", "cuda", "--seed", "7",
                     "--synthetic-steps", "2", "--synthetic-vocab", "50", "--output-dir", str(out_dir),
                     "--teacher", teacher_path, "--distill-alpha", "0.3", "--distill-temperature", "4"]) == 0
    said = capsys.readouterr().out
    line = [l for l in said.splitlines() if l.startswith("epoch 1:")][0]
    hard, soft = (float(line.split(word)[1].split(",")[0].split(")")[0]) for word in ("(hard ", ", soft "))
    assert np.isfinite(hard) and np.isfinite(soft) and hard > 0 and soft > 0, line
    ck = [f for f in os.listdir(out_dir / "distil" / "checkpoints")]
    assert ck == ["checkpoint_epoch_1_step_2.pt"]
    pred = Predictor.from_checkpoint(str(out_dir / "distil" / "checkpoints" / ck[0]), device=DEV)
    assert pred.tokenizer.token_to_id == vocab
    # a teacher of another vocabulary is refused, naming the first differing token
    other = dict(vocab)
    other["t7"], other["t8"] = vocab["t8"], vocab["t7"]
    save_checkpoint(teacher_path, model_of(tcfg, synth.make_state_dict(tcfg, seed=9)), TokenTable(other, max_sequence_length=20),
                    teacher_config)
    with pytest.raises(SystemExit, match="token 't7'"):
        cli.train(str(path), "refused", None, None, "cuda", 7, synthetic_steps=2, synthetic_vocab=50, output_dir=str(out_dir),
                  teacher=[teacher_path])
