"""Minimum-risk fine-tuning on the GPU: the four entries of csrc/train_risk.hip through the C ABI against the float64
restatement (risk_ref), the wiring through TrainStep(risk=...), and the CLI.

i2l_risk_rows and i2l_rows_repeat are exact.  i2l_ce_weighted_fwd_bwd is pinned bit for bit to
i2l_ce_label_smooth_fwd_bwd where the two must agree, and held to float64 by the rule of test_small_entries_vs_float64.py:
the same formulas are evaluated in float32 on the CPU (risk_ref.weighted_ce_torch, float32) and err <= 4 * err_fp32cpu +
floor, a row's dlogits taking the row's largest fp32 error; the floors are distill_ref's for the hard term scaled by
|coef| (risk_ref.floors).  i2l_rows_fold is an fp32 sum of `times` terms in order: within times * 2^-24 * sum_j |x_j|.
Outputs start as NaN or garbage and sit between sentinel elements that must survive the call."""
import os

import numpy as np
import pytest
import torch

import risk_cases as C
import risk_ref as R
from conftest import record
from img2latex_amd import _lib, synth
from test_distill_gpu import Buf, model_of, nans, sum32

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK = 0


def garbage(*shape):
    return torch.full(shape, -123456, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# 1. i2l_risk_rows
# ---------------------------------------------------------------------------------------------------------------
def risk_rows_call(formulas, draws, alpha, smoothing):
    L = _lib.lib()
    B, N, T = draws.shape
    F, D = Buf(torch.from_numpy(formulas)), Buf(torch.from_numpy(draws), off=3)
    out = dict(rows=Buf(garbage(B * (N + 1), T + 1), off=1), coef=Buf(nans(B * (N + 1))), smooth=Buf(nans(B * (N + 1)), off=2),
               part=Buf(garbage(B * (N + 1))), dist=Buf(garbage(B, N), off=5), len=Buf(garbage(B, N)),
               reward=Buf(nans(B, N), off=1), advantage=Buf(nans(B, N)))
    rc = L.i2l_risk_rows(F.ptr(), D.ptr(), B, N, T, C.START, C.END, C.PAD, alpha, smoothing,
                         *(out[k].ptr() for k in ("rows", "coef", "smooth", "part", "dist", "len", "reward", "advantage")),
                         _lib.stream_ptr())
    assert rc == OK, rc
    got = {k: v.get().numpy() for k, v in out.items()}
    F.get(), D.get()
    got["rows"] = got["rows"].reshape(B * (N + 1), T + 1)
    for k in ("dist", "len", "reward", "advantage"):
        got[k] = got[k].reshape(B, N)
    return got


@pytest.mark.parametrize("T", [7, 64, 65, 130])
@pytest.mark.parametrize("N", [2, 5, 16])
def test_risk_rows_vs_float64(N, T):
    """B = 3 (risk_cases.batch: the corners rotate with the seed), T on both sides of the 64-token blocks (W = 1, 1, 2, 3):
    integers exact, the fp32 outputs bit-identical to the float64 values rounded once."""
    for rep in range(6):
        seed = 1000 * N + 10 * T + rep
        alpha, smoothing = (0.0, 0.3, 0.5, 1.0)[seed % 4], (0.0, 0.1)[rep % 2]
        formulas, draws = C.batch(N, T, seed)
        got = risk_rows_call(formulas, draws, alpha, smoothing)
        ref = R.risk_rows(formulas, draws, C.START, C.END, C.PAD, alpha, smoothing)
        for key in ("rows", "part", "dist", "len"):
            assert np.array_equal(got[key], ref[key]), (N, T, rep, key)
        for key in ("coef", "smooth", "reward", "advantage"):
            assert got[key].dtype == np.float32 and got[key].tobytes() == ref[key].tobytes(), (N, T, rep, key, got[key], ref[key])
        assert (ref["dist"][1, 0], ref["reward"][1, 0]) == (0, 1.0)              # both empty
        assert np.abs(ref["advantage"][2]).max() <= N * 2.0 ** -50                # all draws equal


@pytest.mark.parametrize("N,T", [(2, 256), (5, 257), (3, 512), (16, 1024)])
def test_risk_rows_in_the_wide_blocks(N, T):
    """The remaining widths of the dispatch: W = 4 (steps 256), 8 (257 and 512) and 16 (the step limit, with 16 draws)."""
    formulas, draws = C.batch(N, T, 5)
    got = risk_rows_call(formulas, draws, 0.5, 0.1)
    ref = R.risk_rows(formulas, draws, C.START, C.END, C.PAD, 0.5, 0.1)
    for key in ("rows", "part", "dist", "len"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("coef", "smooth", "reward", "advantage"):
        assert got[key].tobytes() == ref[key].tobytes(), key


# ---------------------------------------------------------------------------------------------------------------
# 2. i2l_ce_weighted_fwd_bwd
# ---------------------------------------------------------------------------------------------------------------
def weighted_call(x, tgt, steps, pad, coef, smooth, part, want_d=True, want_parts=True):
    """-> (out (2), parts (4) or None, d (rows, V) or None) as fp32 torch tensors."""
    L = _lib.lib()
    rows, V = x.shape
    X, T = Buf(torch.from_numpy(x)), Buf(torch.from_numpy(np.asarray(tgt)).to(torch.int32), off=1)
    Cf, S = Buf(torch.from_numpy(np.asarray(coef, dtype=np.float32))), Buf(torch.from_numpy(np.asarray(smooth, dtype=np.float32)), off=2)
    P = Buf(torch.from_numpy(np.asarray(part, dtype=np.int32)), off=1)
    D = Buf(nans(rows, V)) if want_d else None
    parts = Buf(nans(4), off=3) if want_parts else None
    out = Buf(nans(2))
    nbytes = L.i2l_ce_weighted_workspace_bytes(rows)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    rc = L.i2l_ce_weighted_fwd_bwd(X.ptr(), T.ptr(), rows // steps, steps, V, pad, Cf.ptr(), S.ptr(), P.ptr(), ws.data_ptr(),
                                   nbytes, D.ptr() if want_d else None, out.ptr(), parts.ptr() if want_parts else None,
                                   _lib.stream_ptr())
    assert rc == OK, rc
    res = (out.get(), parts.get() if want_parts else None, D.get().reshape(rows, V) if want_d else None)
    for b in (X, T, Cf, S, P):
        b.get()
    return res


def plain_call(x, tgt, pad, eps):
    L = _lib.lib()
    rows, V = x.shape
    X, T = Buf(torch.from_numpy(x)), Buf(torch.from_numpy(np.asarray(tgt)).to(torch.int32))
    D, O = Buf(nans(rows, V)), Buf(nans(2))
    nbytes = L.i2l_ce_workspace_bytes(rows)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)
    assert L.i2l_ce_label_smooth_fwd_bwd(X.ptr(), T.ptr(), rows, V, pad, eps, ws.data_ptr(), nbytes, D.ptr(), O.ptr(),
                                         _lib.stream_ptr()) == OK
    return O.get(), D.get().reshape(rows, V)


def operands(seqs, steps, V, pad, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((seqs * steps, V))).astype(np.float32)
    tgt = rng.integers(0, V, seqs * steps)
    tgt[1::4] = pad
    return x, tgt


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("V", [5, 256, 500, 513])
def test_unit_coefficients_are_the_plain_cross_entropy_bit_for_bit(V):
    """Every coefficient 1 and one smoothing value: dlogits, loss sum and count carry i2l_ce_label_smooth_fwd_bwd's bits
    (300 token rows: the ordered sum's 256-thread stride wraps), and the parts add up to them."""
    for seqs, steps, pad, eps in ((5, 3, 0, 0.1), (7, 1, -100, 0.0), (100, 3, 0, 0.1)):
        x, tgt = operands(seqs, steps, V, pad, 31 * V + seqs)
        part = np.arange(seqs) % 2
        out, parts, d = weighted_call(x, tgt, steps, pad, np.ones(seqs), np.full(seqs, eps), part)
        ce_out, ce_d = plain_call(x, tgt, pad, eps)
        assert torch.equal(bits(out), bits(ce_out)), (V, seqs, out, ce_out)
        assert torch.equal(bits(d), bits(ce_d)), (V, seqs)
        keep = (tgt != pad).reshape(seqs, steps)
        assert parts[1] == keep[part == 0].sum() and parts[3] == keep[part == 1].sum()
        assert abs(float(parts[0]) + float(parts[2]) - float(out[0])) <= 2.0 ** -22 * float(out[0])
        o2, p2, _ = weighted_call(x, tgt, steps, pad, np.ones(seqs), np.full(seqs, eps), part, want_d=False)
        o3, _, _ = weighted_call(x, tgt, steps, pad, np.ones(seqs), np.full(seqs, eps), part, want_parts=False)
        assert torch.equal(bits(o2), bits(out)) and torch.equal(bits(p2), bits(parts)) and torch.equal(bits(o3), bits(out))


def judge(name, err, err_cpu, floor, what, share_row=False):
    """err <= 4 * err_fp32cpu + floor; both recorded in units of the floor (where there is one)."""
    err, err_cpu, floor = (np.asarray(t, dtype=np.float64) for t in (err, err_cpu, floor))
    unit = np.where(floor > 0, floor, np.inf)
    record(f"risk gpu {name} err_hip [floors]", float((err / unit).max()))
    record(f"risk gpu {name} err_fp32cpu [floors]", float((err_cpu / unit).max()))
    if share_row:
        err_cpu = err_cpu.max(axis=-1, keepdims=True)
    assert np.isfinite(err).all(), (name, what)
    over = err - (4 * err_cpu + floor)
    assert float(over.max()) <= 0, (name, what, float((err / unit).max()), float((err_cpu / unit).max()))


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("V", [5, 256, 500, 513])
def test_weighted_ce_vs_float64(V, steps):
    """Mixed coefficients (negative, zero, positive) and mixed smoothing over six sequences, PAD rows among them."""
    coef = np.array([0.5, -0.75, 0.0, 1.25, -0.01, 0.3], dtype=np.float32)
    smooth = np.array([0.1, 0.0, 0.0, 0.1, 0.0, 0.2], dtype=np.float32)
    part = np.array([0, 1, 1, 0, 1, 1], dtype=np.int32)
    for pad in (0, -100):
        x, tgt = operands(6, steps, V, pad, 7 * V + steps)
        what = (V, steps, pad)
        out, parts, d = (t.double().numpy() for t in weighted_call(x, tgt, steps, pad, coef, smooth, part))
        ref = R.weighted_ce_np(x, tgt, steps, pad, coef, smooth, part)
        cpu = R.weighted_ce_torch(x, tgt, steps, pad, coef, smooth, torch.float32)
        d_floor, loss_floor = R.floors(x, tgt, pad, ref["coef"])
        _, plain_floor = R.floors(x, tgt, pad, np.ones_like(ref["coef"]))
        assert out[1] == ref["out"][1] and parts[1] == ref["parts"][1] and parts[3] == ref["parts"][3], what
        assert not d[~ref["keep"]].any() and not d[ref["coef"] == 0].any(), what          # +0 or -0: exactly zero
        judge("weighted dlogits", np.abs(d - ref["d"]), np.abs(cpu["d"] - ref["d"]), d_floor[:, None], what, share_row=True)
        judge("weighted loss sum", abs(out[0] - ref["out"][0]), abs(cpu["total"] - ref["out"][0]), loss_floor.sum(), what)
        gold = part[np.arange(6 * steps) // steps] == 0
        for at, rows in ((0, gold), (2, ~gold)):
            judge(f"part {at // 2} loss sum", abs(parts[at] - ref["parts"][at]), abs(sum32(cpu["loss"][rows]) - ref["parts"][at]),
                  plain_floor[rows].sum(), what)


# ---------------------------------------------------------------------------------------------------------------
# 3. i2l_rows_repeat / i2l_rows_fold
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("times", [3, 17])
@pytest.mark.parametrize("width", [1, 63, 512])
def test_rows_repeat_and_fold(width, times):
    L = _lib.lib()
    rng = np.random.default_rng(100 * width + times)
    for rows in (1, 5):
        x = rng.standard_normal((rows, width)).astype(np.float32)
        X, out = Buf(torch.from_numpy(x), off=1), Buf(nans(rows * times, width))
        assert L.i2l_rows_repeat(X.ptr(), rows, width, times, out.ptr(), _lib.stream_ptr()) == OK
        got = out.get().reshape(rows * times, width)
        assert torch.equal(bits(got), bits(torch.from_numpy(np.repeat(x, times, axis=0)))), (rows, width, times)
        X.get()
        y = (rng.standard_normal((rows * times, width)) * rng.choice([1e-3, 1.0, 50.0], (rows * times, 1))).astype(np.float32)
        Y, folded = Buf(torch.from_numpy(y), off=2), Buf(nans(rows, width), off=1)
        assert L.i2l_rows_fold(Y.ptr(), rows, width, times, folded.ptr(), _lib.stream_ptr()) == OK
        got = folded.get().reshape(rows, width).double().numpy()
        y64 = y.astype(np.float64).reshape(rows, times, width)
        bound = times * 2.0 ** -24 * np.abs(y64).sum(axis=1)
        err = np.abs(got - y64.sum(axis=1))
        record("risk gpu rows_fold err [times x 2^-24 x sum |x|]", float((err / bound).max()))
        assert (err <= bound).all(), (rows, width, times)
        Y.get()


# ---------------------------------------------------------------------------------------------------------------
# 4. wiring through TrainStep
# ---------------------------------------------------------------------------------------------------------------
B, N, T, V = 2, 3, 8, 50
CFG = synth.model_config(vocab_size=V, embedding_dim=32, hidden_dim=64, lstm_layers=1, attention=False, channels=1,
                         img_height=16, img_width=32, conv_filters=(4, 8, 16), dropout=0.0)


def wiring_case():
    sd = synth.make_state_dict(CFG, seed=23, out_scale=4.0, enc_scale=16.0, end_bias=2.0)
    images = synth.make_images(B, CFG, seed=231)
    formulas = synth.make_formulas(B, T + 1, V, seed=232, min_len=4)
    return sd, torch.from_numpy(images).to(DEV), torch.from_numpy(formulas).to(DEV)


def risk_step(sd, alpha, seed=5, **kw):
    from img2latex_amd.training import RiskObjective, TrainStep
    m = model_of(CFG, sd)
    m.train()
    return TrainStep(m, pad_token_id=synth.PAD, label_smoothing=0.1, seed=seed,
                     risk=RiskObjective(synth.START, synth.END, samples=N, alpha=alpha, **kw))


def rel_close(a, b, tol, what):
    """test_hip_training.rel_close: the tolerance of the HIP gradients against autograd there (2e-4 of the largest)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-12)
    err = float(np.abs(a - b).max())
    record(f"risk gpu wiring {what[0]} [rel to max]", err / scale)
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def check_batch(ts, formulas):
    """What the step assembled is the restatement's, from the step's own draws."""
    batch = {k: v.cpu().numpy() for k, v in ts.risk_batch.items()}
    assert batch["draws"].shape == (B, N, T) and batch["rows"].shape == (B * (N + 1), T + 1)
    ref = R.risk_rows(formulas.cpu().numpy(), batch["draws"], synth.START, synth.END, synth.PAD, ts.risk.alpha, 0.1)
    for key in ("rows", "part", "dist", "len"):
        assert np.array_equal(batch[key], ref[key]), key
    for key in ("coef", "smooth", "reward", "advantage"):
        assert batch[key].tobytes() == ref[key].tobytes(), key
    return batch


def test_alpha_one_is_the_plain_step():
    """alpha = 1: the draws' coefficients are 0, so flat_grads[:n] and the loss sum are those of a plain
    TrainStep.forward_backward on the same batch; the count is gold plus draw targets."""
    from img2latex_amd.training import TrainStep
    sd, images, formulas = wiring_case()
    plain_model = model_of(CFG, sd)
    plain_model.train()
    plain = TrainStep(plain_model, pad_token_id=synth.PAD, label_smoothing=0.1, seed=5)
    plain.forward_backward(images, formulas)
    ts = risk_step(sd, 1.0)
    logits = ts.forward_backward(images, formulas)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (B * (N + 1), T, V)
    batch = check_batch(ts, formulas)
    assert not batch["coef"].reshape(B, N + 1)[:, 1:].any() and (batch["coef"].reshape(B, N + 1)[:, 0] == 1.0).all()
    want, got = plain.flat_grads.cpu().numpy(), ts.flat_grads.cpu().numpy()
    sizes = {n: p.numel() for n, p in ts.model.named_parameters()}
    for name, off in ts.offsets.items():
        rel_close(got[off:off + sizes[name]], want[off:off + sizes[name]], 2e-4, (name, "alpha 1"))
    assert abs(got[ts.n] - want[ts.n]) <= 1e-5 * max(1.0, abs(want[ts.n]))
    gold_targets = int((formulas[:, 1:] != synth.PAD).sum())
    assert want[ts.n + 1] == gold_targets
    assert got[ts.n + 1] == int((batch["rows"][:, 1:] != synth.PAD).sum()) and got[ts.n + 1] > gold_targets
    parts = ts.risk_parts.cpu().numpy()
    assert parts[1] == gold_targets and parts[1] + parts[3] == got[ts.n + 1]
    assert abs(parts[0] - want[ts.n]) <= 1e-5 * max(1.0, abs(want[ts.n]))


def test_alpha_half_is_the_autograd_bridges_gradient():
    """alpha = 0.5: flat_grads against the autograd bridges (the model's training forward: CNNEncoderFn,
    DecoderTeacherForcedFn) run on the assembled rows and the repeated images, with dlogits from risk_ref."""
    sd, images, formulas = wiring_case()
    ts = risk_step(sd, 0.5)
    logits = ts.forward_backward(images, formulas)
    torch.cuda.synchronize()
    batch = check_batch(ts, formulas)
    assert np.abs(batch["coef"].reshape(B, N + 1)[:, 1:]).max() > 0.01          # the draws differ: the risk term is live
    bridge = model_of(CFG, sd)
    bridge.train()
    rows = torch.from_numpy(batch["rows"]).to(DEV)
    out = bridge(images.repeat_interleave(N + 1, 0), rows)
    assert tuple(out.shape) == (B * (N + 1), T, V)
    assert float((out.detach() - logits).abs().max()) <= 1e-4
    x = out.detach().cpu().numpy().reshape(-1, V)
    ref = R.weighted_ce_np(x, batch["rows"][:, 1:].reshape(-1), T, synth.PAD, batch["coef"], batch["smooth"], batch["part"])
    out.backward(torch.from_numpy(ref["d"].reshape(out.shape)).float().to(DEV))
    got = ts.flat_grads.cpu().numpy()
    grads = dict(bridge.named_parameters())
    for name, off in ts.offsets.items():
        want = grads[name].grad.cpu().numpy().ravel()
        rel_close(got[off:off + want.size], want, 2e-4, (name, "alpha 0.5"))
    assert abs(got[ts.n] - ref["out"][0]) <= 1e-5 * max(1.0, abs(ref["out"][0]))
    assert got[ts.n + 1] == ref["out"][1]


def test_the_same_seed_draws_and_trains_the_same():
    sd, images, formulas = wiring_case()
    runs = []
    for seed in (5, 5, 6):
        ts = risk_step(sd, 0.5, seed=seed)
        ts.forward_backward(images, formulas)
        torch.cuda.synchronize()
        runs.append((ts.risk_batch["draws"].clone(), ts.flat_grads.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[2][0])                               # another seed, another stream


def test_step_returns_the_new_keys():
    sd, images, formulas = wiring_case()
    ts = risk_step(sd, 0.5, temperature=0.8, top_k=10)
    first = ts.step(images, formulas)
    assert set(first) == {"loss", "total_norm", "count", "skipped", "reward", "hard_loss", "risk_loss"}
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in first.values())
    draws0 = ts.risk_batch["draws"].clone()
    second = ts.micro_step(images, formulas, 2, False)
    assert {"reward", "hard_loss", "risk_loss"} <= set(second)
    assert not torch.equal(draws0, ts.risk_batch["draws"])                       # the next step draws its own stream
    for out in (first, second):
        vals = {k: float(v) for k, v in out.items()}
        assert all(np.isfinite(v) for v in vals.values()), vals
        assert 0.0 <= vals["reward"] <= 1.0 and vals["hard_loss"] > 0 and vals["risk_loss"] > 0
    assert float(first["skipped"]) == 0.0
    want = float(ts.risk_batch["reward"].double().mean())
    assert abs(float(second["reward"]) - want) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------
# 5. the CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cli_train_with_the_risk_objective(tmp_path, capsys):
    import yaml
    from img2latex_amd import cli
    config = {
        "model": {"name": "cnn_lstm", "embedding_dim": 32,
                  "encoder": {"cnn": {"img_height": 16, "img_width": 32, "channels": 1, "conv_filters": [4, 8, 16],
                                      "kernel_size": 3, "pool_size": 2, "padding": "same"}},
                  "decoder": {"hidden_dim": 64, "lstm_layers": 1, "dropout": 0.1, "attention": False, "max_seq_length": 20}},
        "data": {"batch_size": 4, "max_seq_length": 20},
        "training": {"device": "cuda", "epochs": 1, "learning_rate": 1e-3, "weight_decay": 0.0, "accumulation_steps": 1,
                     "risk_alpha": 0.25},
    }
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(config))
    out_dir = tmp_path / "outputs"
    assert cli.main(["train", "--config-path", str(path), "--experiment-name", "risk", "--device", "cuda", "--seed", "7",
                     "--synthetic-steps", "2", "--synthetic-vocab", "50", "--output-dir", str(out_dir),
                     "--risk-samples", "2", "--risk-top-k", "20"]) == 0
    said = capsys.readouterr().out
    line = [l for l in said.splitlines() if l.startswith("epoch 1:")][0]
    reward, hard, risk = (float(line.split(word)[1].split(",")[0].split(")")[0]) for word in ("(reward ", ", hard ", ", risk "))
    assert 0.0 <= reward <= 1.0 and np.isfinite(hard) and hard > 0 and np.isfinite(risk) and risk > 0, line
    assert os.listdir(out_dir / "risk" / "checkpoints") == ["checkpoint_epoch_1_step_2.pt"]
