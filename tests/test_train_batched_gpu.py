"""The step-batched training recurrences (_lib.FLAG_TRAIN_BATCHED: i2l_decoder_train_fwd / _bwd on the matrix cores, one
launch per step and layer) against the float64 restatement of test_decoder_shapes.py and against the default path.
Bounds are the suite's: logits 1e-4 absolute, gradients and d(enc) 2e-4 of max|ref|, attention gradients exactly zero;
where the two paths are compared with each other, twice that (each is within the bound of the same exact result).

Only test_a_shape_the_row_kernels_refuse (and tests/test_train_batched_host.py) fail on a build without the feature: a
library that ignored the flag would run the default path and pass every other test here."""
import numpy as np
import pytest
import torch

import img2latex_oracle as O
from conftest import record
from helpers import END, PAD, START, close, images
from img2latex_amd import _lib, synth
from img2latex_amd.model import Seq2SeqModel
from img2latex_amd.model._train_fn import decoder_train_backward, decoder_train_forward
from test_decoder_shapes import _MODELS, _model, build, enc_for, shape_config, sid

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAG = _lib.FLAG_TRAIN_BATCHED
SHIPPED = (500, 512, 512, 2, True)
DEEP = (777, 36, 192, 3, True)
# (V, E, H, L, attention)
SHAPES = [
    (3, 4, 64, 1, False),       # one column tile
    DEEP,                       # H no multiple of 128; three layers: both backward products below the top
    (2048, 64, 128, 2, True),
    SHIPPED,                    # the shipped decoder
]
# (1, 1): no recurrent slab in either direction; (33, 12): ragged against 16 and 32; (3, 2): the two-chunk K split of the
# backward with both products (T < 3); (257, 5), shipped shape only: 64-row tiles and more than one of them
BT = [(1, 1), (5, 5), (33, 12)]
CASES = [(s, b, t) for s in SHAPES for b, t in BT] + [(SHIPPED, 257, 5), (DEEP, 3, 2)]


_MADE = []        # models a test here built for itself (the shared ones are test_decoder_shapes._MODELS)


@pytest.fixture(autouse=True)
def _flags_are_left_clear():
    yield
    for m in [entry[0] for entry in _MODELS.values()] + _MADE:
        assert m.decoder.kernel_flags == 0
    del _MADE[:]


class flagged:
    """dec.kernel_flags |= flags inside, restored on the way out."""

    def __init__(self, dec, flags):
        self.dec, self.flags = dec, flags

    def __enter__(self):
        self.saved = self.dec.kernel_flags
        self.dec.kernel_flags |= self.flags

    def __exit__(self, *exc):
        self.dec.kernel_flags = self.saved


def _forms(V, B, T):
    forms = torch.from_numpy(synth.randint(777, "forms", (B, T + 1), 0, V)).to(DEV)
    forms[:, 0] = START
    forms[0, 1] = max(V - 1, 1)                       # at least one target is not PAD
    return forms


def _check_training_vs_float64(m, sd64, cfg, V, enc, B, T, tag, flags):
    """test_decoder_training_vs_float64's body with the flag set around the kernel calls."""
    forms = _forms(V, B, T)
    params = {n: v.clone().requires_grad_(True) for n, v in sd64.items()}
    enc64 = enc.double().requires_grad_(True)
    ref_logits = O.decoder_forward(params, cfg, enc64, forms[:, :-1])
    O.ce_label_smooth(ref_logits, forms[:, 1:], PAD).backward()
    dec = m.decoder
    dec.train()
    saved = dec.kernel_flags
    try:
        dec.kernel_flags |= flags
        for p in dec.parameters():
            p.grad = None
        enc_dev = enc.clone().requires_grad_(True)
        logits = dec(enc_dev, forms[:, :-1])
        close(logits.detach().cpu().numpy(), ref_logits.detach().cpu().numpy(), 1e-4, f"{tag} training-forward logits",
              absolute=True)
        crit = torch.nn.CrossEntropyLoss(ignore_index=PAD, reduction="mean", label_smoothing=0.1)
        crit(logits.transpose(1, 2), forms[:, 1:]).backward()
    finally:
        dec.kernel_flags = saved
        dec.eval()
    grads = [("d enc", enc_dev.grad, enc64.grad)]
    grads += [(n, p.grad, params["decoder." + n].grad) for n, p in dec.named_parameters()]
    for n, g, ref in grads:
        if n.startswith("attention."):            # the context over one source position does not depend on them
            assert float(g.abs().max()) == 0.0 and float(ref.abs().max()) == 0.0
            continue
        g, ref = g.double().cpu(), ref.cpu()
        err = float((g - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
        record(f"{tag} training gradient [rel to max|ref|]", err)
        assert err <= 2e-4, (tag, n, err)


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("shape,B,T", CASES, ids=[f"{sid(s)}-B{b}-T{t}" for s, b, t in CASES])
def test_training_vs_float64(shape, B, T):
    m, sd64, cfg = build(shape)
    _check_training_vs_float64(m, sd64, cfg, shape[0], enc_for(shape, B, seed=21), B, T,
                               f"train-batched {sid(shape)} B={B} T={T}", FLAG)


# ------------------------------------------------------------------------------------------------ 2. beyond the row kernels
@pytest.mark.parametrize("H,L", [(1088, 1), (2048, 1), (2048, 4)])
def test_a_shape_the_row_kernels_refuse(H, L):
    """H = 1088 (and the bound, 2048, at one layer and at the four the query accepts) trains with the flag and is refused
    without it: the row kernels keep their state in LDS.  Fails on a build without the feature (the forward raises with
    the flag too)."""
    shape = (10, 4, H, L, False)
    m = _model(*shape[:4])
    _MADE.append(m)
    B, T = 3, 4
    dec = m.decoder
    dec.train()
    try:
        enc0 = torch.zeros(B, 4, device=DEV, requires_grad=True)
        with pytest.raises(RuntimeError):
            dec(enc0, torch.full((B, T), START, dtype=torch.long, device=DEV))
    finally:
        dec.eval()
    sd64 = {"decoder." + n: v.detach().to(torch.float64) for n, v in dec.state_dict().items()}
    _check_training_vs_float64(m, sd64, shape_config(shape), shape[0], enc_for(shape, B, seed=21), B, T,
                               f"train-batched H={H} L={L}", FLAG)


# ------------------------------------------------------------------------------------------------ 3. dropout, same masks
def _run(dec, enc, toks, dlogits, seed, backward=True):
    """One decoder_train_forward (+ backward) under the decoder's current mode and flags."""
    logits, state = decoder_train_forward(dec, enc, toks, seed=seed)
    if not backward:
        return logits, None, None, state
    grads = {n: torch.full_like(p, float("nan")) for n, p in dec.named_parameters()}
    denc = decoder_train_backward(dec, state, dlogits, grads)
    torch.cuda.synchronize()
    return logits, grads, denc, state


def _inputs(shape, B, T):
    V = shape[0]
    enc = enc_for(shape, B, seed=23)
    toks = torch.from_numpy(synth.randint(778, "tok", (B, T), 0, V)).to(DEV, torch.int32).contiguous()
    dlogits = torch.from_numpy(synth.uniform(779, "dlogits", (B, T, V), -1e-2, 1e-2)).to(DEV)
    return enc, toks, dlogits


class dropout_mode:
    """train mode with decoder.dropout = p inside; eval mode and the model's own p on the way out."""

    def __init__(self, dec, p):
        self.dec, self.p = dec, p

    def __enter__(self):
        self.saved = self.dec.dropout
        self.dec.dropout = self.p
        self.dec.train()

    def __exit__(self, *exc):
        self.dec.dropout = self.saved
        self.dec.eval()


@pytest.mark.parametrize("B,T", [(5, 9), (33, 5)])
@pytest.mark.parametrize("shape", [DEEP, SHIPPED], ids=[sid(DEEP), sid(SHIPPED)])
def test_dropout_same_masks_as_the_default_path(shape, B, T):
    m, _, _ = build(shape)
    dec = m.decoder
    enc, toks, dlogits = _inputs(shape, B, T)
    tag = f"train-batched {sid(shape)} B={B} T={T} p=0.3"
    with dropout_mode(dec, 0.3):
        off = _run(dec, enc, toks, dlogits, 1234)
        with flagged(dec, FLAG):
            on = _run(dec, enc, toks, dlogits, 1234)
    with dropout_mode(dec, 0.0), flagged(dec, FLAG):
        on_p0 = _run(dec, enc, toks, dlogits, 1234, backward=False)
    with flagged(dec, FLAG):                                     # eval mode
        on_eval = _run(dec, enc, toks, dlogits, 1234, backward=False)
    err = float((on[0] - off[0]).abs().max())
    record(f"{tag} logits, flag on vs off [abs]", err)
    assert err <= 2e-4, (tag, err)
    pairs = [("d enc", on[2], off[2])] + [(n, on[1][n], off[1][n]) for n in off[1]]
    for n, g, ref in pairs:
        assert bool(torch.isfinite(g).all()), (tag, n)
        if n.startswith("attention."):
            assert float(g.abs().max()) == 0.0
            continue
        rel = float((g - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
        record(f"{tag} gradient, flag on vs off [rel to max|off|]", rel)
        assert rel <= 4e-4, (tag, n, rel)
    assert not torch.equal(on[0], on_p0[0])                      # the masks are live
    assert torch.equal(on_p0[0], on_eval[0])                     # p = 0 in train mode is eval mode, bit for bit


# ------------------------------------------------------------------------------------------------ 4. reproducible, re-entrant
def test_reproducible_and_reentrant():
    m, _, _ = build(SHIPPED)
    dec = m.decoder
    enc, toks, dlogits = _inputs(SHIPPED, 33, 12)
    with dropout_mode(dec, 0.3), flagged(dec, FLAG):
        a = _run(dec, enc, toks, dlogits, 99)
        b = _run(dec, enc, toks, dlogits, 99)
        again = {n: torch.full_like(p, float("nan")) for n, p in dec.named_parameters()}
        denc_again = decoder_train_backward(dec, b[3], dlogits, again)       # the tape is not consumed
        torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(b[2], denc_again)
    for n in a[1]:
        assert bool(torch.isfinite(a[1][n]).all()), n
        assert torch.equal(a[1][n], b[1][n]), n
        assert torch.equal(b[1][n], again[n]), n


# ------------------------------------------------------------------------------------------------ 5. flag hygiene
def test_inference_entries_ignore_the_flag():
    m, _, _ = build(SHIPPED)
    dec = m.decoder
    enc = enc_for(SHIPPED, 5, seed=9)
    tok0 = torch.full((5,), START, dtype=torch.int32, device=DEV)

    def infer():
        ids, _, _ = dec.run_steps(enc, 20, tok0)
        with torch.no_grad():
            beams = m.beam_search_batch(enc[:2], START, END, 12, 3)
        return ids.cpu(), beams

    ids0, beams0 = infer()
    with flagged(dec, FLAG):
        ids1, beams1 = infer()
    assert torch.equal(ids0, ids1) and beams0 == beams1


def test_exact_fp32_wins_over_the_flag():
    shape = (2048, 64, 128, 2, True)
    m, _, _ = build(shape)
    dec = m.decoder
    enc, toks, dlogits = _inputs(shape, 5, 5)
    with dropout_mode(dec, 0.3):
        with flagged(dec, _lib.FLAG_EXACT_FP32):
            a = _run(dec, enc, toks, dlogits, 7)
        with flagged(dec, _lib.FLAG_EXACT_FP32 | FLAG):
            b = _run(dec, enc, toks, dlogits, 7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), n


# ------------------------------------------------------------------------------------------------ 6. through the surface
def test_train_step_follows_the_flag():
    """Three TrainStep steps (its default lr, 1e-3) on a tiny two-layer model, inter-layer dropout live, with and without
    the flag.  Step 1 starts from equal parameters and draws equal masks, so what the surface hands to Adam can be held to
    the suite's bounds: each path's gradients are within 2e-4 of max|exact| per tensor, so they differ by at most 4e-4 of
    max|flag off|; each path's logits are within 1e-4 and the label-smoothed CE moves by at most twice the largest
    logit error, so the losses differ by at most 4e-4.  (A backward that dropped its second product, or a forward that
    lost the mask, misses the gradient bound by orders of magnitude.)  The encoder's gradients hang on d(enc) through its
    own backward and are recorded, not bounded.  After three steps the parameters are held to 4e-4 of max|parameter|:
    Adam moves an element by about lr per step, so gradients that disagreed in sign would part them by up to 6e-3."""
    from img2latex_amd.training import TrainStep
    cfg = synth.model_config(vocab_size=50, embedding_dim=32, hidden_dim=64, lstm_layers=2, attention=True, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16), dropout=0.3)
    x = images(cfg, batch=8, device=DEV)
    forms = torch.from_numpy(synth.make_formulas(8, 14, cfg["vocab_size"], seed=5, min_len=6)).to(DEV)
    out = {}
    for flags in (0, FLAG):
        torch.manual_seed(0)
        m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg)).to(DEV)
        _MADE.append(m)
        ts = TrainStep(m, seed=11)
        with flagged(m.decoder, flags):
            m.train()
            ts.forward_backward(x, forms)
            torch.cuda.synchronize()
            grads = {n: g.detach().clone() for n, g in ts.grad_views.items()}
            losses = [float(ts.flat_grads[ts.n] / ts.flat_grads[ts.n + 1])]
            ts.apply()
            losses += [float(ts.step(x, forms)["loss"]) for _ in range(2)]
        out[flags] = (losses, ts.flat_params.detach().clone(), grads)
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (flags, losses)
    (loss0, ref, g0), (loss1, got, g1) = out[0], out[FLAG]
    for n in g0:
        if n.startswith("decoder.attention."):
            assert float(g1[n].abs().max()) == 0.0
            continue
        rel = float((g1[n] - g0[n]).abs().max()) / max(float(g0[n].abs().max()), 1e-12)
        record(f"train-batched TrainStep step 1 {n.split('.')[0]} gradients, flag on vs off [rel to max|off|]", rel)
        if n.startswith("decoder."):
            assert rel <= 4e-4, (n, rel)
    record("train-batched TrainStep step 1 loss, flag on vs off [abs]", abs(loss1[0] - loss0[0]))
    assert abs(loss1[0] - loss0[0]) <= 4e-4, (loss0, loss1)
    record("train-batched TrainStep step 3 loss, flag on vs off [abs]", abs(loss1[2] - loss0[2]))
    rel = float((got - ref).abs().max()) / float(ref.abs().max())
    record("train-batched TrainStep x3 parameters, flag on vs off [rel to max|parameter|]", rel)
    assert rel <= 4e-4, rel
