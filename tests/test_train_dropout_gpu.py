"""The decoder's training kernels with dropout LIVE (i2l_decoder_train_fwd / _bwd, p > 0) against float64.

The masks are a counter-based hash of (seed, stream, element index) that forward and backward each recompute (DESIGN.md
section 4, "The dropout mask rule"); tests/dropout_ref.py restates the hash and the masked forward, so the whole masked
forward and backward can be held to a float64 reference, and every mask element to the restated one.

(a) logits, d(enc) and every parameter gradient against decoder_forward_masked in float64, on every recurrence path.
    Bounds are the suite's: logits 1e-4 absolute, gradients 2e-4 of max|ref| per tensor, attention gradients exactly
    zero.  Where a tensor misses its bound the same restatement is evaluated in float32 on the same inputs and the bound
    becomes max(suite's bound, 4 x |float32 - float64|): what float32 arithmetic costs at scale 1 / (1 - p), never what
    the kernel gives.  Both numbers are recorded then.
(b) every mask element, exactly, through the public entries only (zero patterns of logits and gradients).  A position is
    judged where the float64 value of what the mask multiplies exceeds 1e-6 in magnitude; at most 1 % may be left out,
    asserted on the float64 numbers alone.  A dropped position must be an exact zero whether judged or not.
(c) through LSTMDecoder.forward and TrainStep: the seed each draws reaches the kernels."""
import numpy as np
import pytest
import torch

import dropout_ref as R
import img2latex_oracle as O
from conftest import record
from helpers import PAD, images
from img2latex_amd import _lib, synth
from img2latex_amd.model import Seq2SeqModel
from img2latex_amd.model._train_fn import decoder_train_backward, decoder_train_forward
from img2latex_amd.training.train_step import step_seed
from test_decoder_shapes import build, enc_for, model_from_sd, shape_config, sid
from test_train_batched_gpu import _forms, _run, dropout_mode, flagged

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 1234
BATCHED, NO_GROUP, EXACT = _lib.FLAG_TRAIN_BATCHED, _lib.FLAG_NO_GROUP, _lib.FLAG_EXACT_FP32
TWO = (40, 36, 64, 2, True)
FOUR = (60, 8, 64, 4, False)
DEEP = (777, 36, 192, 3, True)
SHIPPED = (500, 512, 512, 2, True)
WIDE = (64, 8, 256, 1, False)           # L = 1, H = 256: the grouped recurrences and the resident row kernel
JUDGED = 1e-6


# ------------------------------------------------------------------------------------------------ (a) against float64
def _reference(sd64, cfg, enc, toks, targets, p, seed, dtype):
    """logits, d(enc) and the parameter gradients of the masked forward + label-smoothed CE, evaluated in ``dtype``."""
    params = {n: v.to(dtype).clone().requires_grad_(True) for n, v in sd64.items()}
    e = enc.to(dtype).requires_grad_(True)
    logits = R.decoder_forward_masked(params, cfg, e, toks, p, seed)
    O.ce_label_smooth(logits, targets, PAD).backward()
    out = {"logits": logits.detach().double(), "d enc": e.grad.double()}
    for n, v in params.items():
        out[n[len("decoder."):]] = v.grad.double()
    return out


def _check_masked_vs_float64(shape, B, T, p, flags, seed, tag):
    """test_train_batched_gpu._check_training_vs_float64 with an explicit seed through decoder_train_forward /
    decoder_train_backward and the masked restatement as the reference."""
    m, sd64, cfg = build(shape)
    V = shape[0]
    forms = _forms(V, B, T)
    toks, targets = forms[:, :-1].to(torch.int32).contiguous(), forms[:, 1:]
    enc = enc_for(shape, B, seed=21)
    ref = _reference(sd64, cfg, enc, toks, targets, p, seed, torch.float64)
    dec = m.decoder
    with dropout_mode(dec, p), flagged(dec, flags):
        logits, state = decoder_train_forward(dec, enc, toks, seed=seed)
        lg = logits.detach().clone().requires_grad_(True)
        crit = torch.nn.CrossEntropyLoss(ignore_index=PAD, reduction="mean", label_smoothing=0.1)
        crit(lg.transpose(1, 2), targets).backward()
        grads = {n: torch.full_like(q, float("nan")) for n, q in dec.named_parameters()}
        denc = decoder_train_backward(dec, state, lg.grad.contiguous(), grads)
        torch.cuda.synchronize()
    got = dict(grads)
    got["logits"], got["d enc"] = logits, denc
    ref32 = {}

    def float32_distance(n, scale):
        if not ref32:
            ref32.update(_reference(sd64, cfg, enc, toks, targets, p, seed, torch.float32))
        return float((ref32[n] - ref[n]).abs().max()) / scale

    for n in ["logits", "d enc"] + [k for k in grads]:
        g, want = got[n].double(), ref[n]
        assert bool(torch.isfinite(g).all()), (tag, n)
        if n.startswith("attention."):            # the context over one source position does not depend on them
            assert float(g.abs().max()) == 0.0 and float(want.abs().max()) == 0.0
            continue
        absolute = n == "logits"
        scale = 1.0 if absolute else max(float(want.abs().max()), 1e-12)
        bound = 1e-4 if absolute else 2e-4
        err = float((g - want).abs().max()) / scale
        what = "logits [abs]" if absolute else "gradient [rel to max|ref|]"
        record(f"{tag} masked training {what}", err)
        print(f"{tag} {n}: {err:.3e}")
        if err > bound:
            dist = float32_distance(n, scale)
            record(f"{tag} {n}: float32 restatement vs float64, the bound is 4 x this", dist)
            record(f"{tag} {n}: kernel vs float64 under that bound", err)
            print(f"{tag} {n}: float32 restatement at {dist:.3e}")
            bound = max(bound, 4.0 * dist)
        assert err <= bound, (tag, n, err, bound)


def _cases():
    out = []
    # row kernels, every layer count, both X rules
    for shape in [(40, 4, 64, 1, False), TWO, DEEP, FOUR]:
        for B, T in [(5, 5), (33, 12)]:
            for p in (0.1, 0.5):
                out.append((shape, B, T, p, 0, SEED))
    # 2 and 4 rows per workgroup (B > 256, B > 512), the last workgroup ragged
    for shape in [TWO, FOUR]:
        for B in (257, 515):
            out.append((shape, B, 3, 0.3, 0, SEED))
    # the grouped recurrences (2 and 4 rows per group) and the resident row kernel: masks before and after them
    out += [(WIDE, 70, 8, 0.3, 0, SEED), (WIDE, 130, 8, 0.3, 0, SEED), (WIDE, 5, 8, 0.3, NO_GROUP, SEED)]
    # step-batched, with its dropped copies of the layer outputs
    out += [(DEEP, B, T, 0.3, BATCHED, SEED) for B, T in [(1, 1), (3, 2), (33, 12)]] + [(SHIPPED, 33, 5, 0.3, BATCHED, SEED)]
    out.append((TWO, 5, 5, 0.3, EXACT, SEED))
    # all 64 bits of the seed reach the kernels
    out += [(TWO, 5, 5, 0.3, 0, s) for s in (0, 2 ** 62 - 1, 2 ** 64 - 1)]
    return out


def _case_id(c):
    shape, B, T, p, flags, seed = c
    names = {0: "", BATCHED: "-batched", NO_GROUP: "-nogroup", EXACT: "-exact"}
    return f"{sid(shape)}-B{B}-T{T}-p{p}{names[flags]}" + (f"-seed{seed:x}" if seed != SEED else "")


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_masked_training_vs_float64(case):
    shape, B, T, p, flags, seed = case
    _check_masked_vs_float64(shape, B, T, p, flags, seed, "dropout " + _case_id(case))


# ------------------------------------------------------------------------------------------------ (b) every mask element
_PLAIN = {}


def _plain(shape, edit=None, key=None):
    """build() without the END clock (which zeroes the weights of one unit): every unit has a gradient.  ``edit``
    changes the numpy state dict before it is loaded."""
    k = (shape, key)
    if k not in _PLAIN:
        cfg = shape_config(shape)
        sd = synth.make_state_dict(cfg, seed=500 + shape[2] // 64 + 17 * shape[3], out_scale=1.0)
        if edit is not None:
            edit(sd)
        _PLAIN[k] = model_from_sd(cfg, sd) + (cfg,)
    return _PLAIN[k]


def _pattern(got, keep, unmasked64, what, group=None):
    """got != 0 equals ``keep`` at every judged position, at least 99 % of the positions are judged, and a dropped
    position is an exact zero wherever it lies.  ``group``: the name the share left out is recorded under."""
    got, unmasked64 = np.asarray(got), np.asarray(unmasked64)
    assert got.shape == keep.shape == unmasked64.shape, (what, got.shape, keep.shape, unmasked64.shape)
    judged = np.abs(unmasked64) > JUDGED
    assert judged.mean() >= 0.99, (what, float(judged.mean()))             # float64 numbers alone
    assert np.isfinite(got).all(), what
    wrong = ((got != 0) != keep) & judged
    assert not wrong.any(), (what, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    assert not got[~keep].any(), what
    record(f"dropout mask pattern, share of positions left out: {group or what}", 1.0 - float(judged.mean()))


@pytest.mark.parametrize("H,B,T", [(64, 257, 3), (256, 513, 8)])
def test_out_mask_every_element(H, B, T):
    """V = H, W_out = I, b_out = 0: the logits ARE the dropped top-layer output, so `logits != 0` is the OUT mask and a
    kept logit is scale x h.  h must not depend on p for that, and the input mask would make it: the embedding table
    and enc are zero, so X is zero under any mask and h comes from the biases and the recurrence (the same for every
    row, different at every step and unit).  Two rows per workgroup at B = 257; B = 513, T = 8, H = 256 runs the
    grouped recurrence and makes B T H exceed 4096 x 256, where dropout_rows_kernel's grid-stride loop wraps."""
    shape = (H, 4, H, 1, False)
    p = 0.3

    def edit(sd):
        sd["decoder.embedding.weight"][:] = 0.0
        sd["decoder.output_layer.weight"] = np.eye(H, dtype=np.float32)
        sd["decoder.output_layer.bias"][:] = 0.0

    m, sd64, cfg = _plain(shape, edit, "out")
    dec = m.decoder
    enc = torch.zeros(B, 4, device=DEV)
    toks = torch.from_numpy(synth.randint(31, "tok", (B, T), 0, H)).to(DEV, torch.int32).contiguous()
    assert B * T * H > 4096 * 256 or H == 64
    with dropout_mode(dec, p):
        got = _run(dec, enc, toks, None, SEED, backward=False)[0]
    with dropout_mode(dec, 0.0):
        got_p0 = _run(dec, enc, toks, None, SEED, backward=False)[0]
    with torch.no_grad():
        h64 = R.decoder_forward_masked(sd64, cfg, enc.double(), toks, 0.0, SEED).cpu().numpy()
    keep = R.keep_mask(SEED, R.DS_OUT, B * T * H, p).reshape(B, T, H)
    got, got_p0 = got.cpu().numpy(), got_p0.cpu().numpy()
    err0 = float(np.abs(got_p0 - h64).max())
    record(f"dropout OUT H={H} B={B} T={T}: p = 0 logits vs float64 [abs]", err0)
    assert err0 <= 1e-4
    _pattern(got, keep, h64, f"OUT H={H} B={B} T={T}")
    err = float(np.abs(got - R.scale(p) * got_p0.astype(np.float64))[keep].max())
    record(f"dropout OUT H={H} B={B} T={T}: kept logits vs scale x (p = 0 logits) [abs]", err)
    assert err <= 1e-6, err


def _x_keep(B, T, E, attn, p, seed):
    """(B T, 2E) bool: which elements of X survive -- the flat index on the plain path; bt E + e over the embedding
    half only on the attention path, whose enc half is never masked."""
    if attn:
        emb = R.keep_mask(seed, R.DS_X, B * T * E, p).reshape(B * T, E)
        return np.concatenate([emb, np.ones((B * T, E), dtype=bool)], axis=1)
    return R.keep_mask(seed, R.DS_X, B * T * 2 * E, p).reshape(B * T, 2 * E)


def _backward_both(dec, sd64, cfg, enc, toks, dlogits, p, seed, tokens_for_the_gradient=None):
    """The kernels' backward for a given dlogits (grads, d enc) and the float64 one with its tape."""
    with dropout_mode(dec, p):
        _, state = decoder_train_forward(dec, enc, toks, seed=seed)
        if tokens_for_the_gradient is not None:
            state["tokens"] = tokens_for_the_gradient
        grads = {n: torch.full_like(q, float("nan")) for n, q in dec.named_parameters()}
        denc = decoder_train_backward(dec, state, dlogits, grads)
        torch.cuda.synchronize()
    params = {n: v.clone().requires_grad_(True) for n, v in sd64.items()}
    enc64 = enc.double().requires_grad_(True)
    tape = {}
    ref_logits = R.decoder_forward_masked(params, cfg, enc64, toks, p, seed, tape=tape)
    (ref_logits * dlogits.double()).sum().backward()
    ref = {n[len("decoder."):]: v.grad for n, v in params.items()}
    ref["d enc"] = enc64.grad
    return {n: g.cpu().numpy() for n, g in grads.items()}, denc.cpu().numpy(), ref, tape


def _dlogits(B, T, V):
    """In [-1, 1], no two neighbours alike; made on the device (the largest case has 17 M elements)."""
    n = torch.arange(B * T * V, device=DEV, dtype=torch.float64)
    return torch.sin(n * 0.7371 + 0.5).float().reshape(B, T, V)


# E = 128 at (513, 8), plain path: B T 2E exceeds 4096 x 256, so build_x_kernel's grid-stride loop wraps and
# emb_gather_kernel walks seventeen chunks of tokens
@pytest.mark.parametrize("E,B,T,attn", [(8, 5, 5, False), (36, 33, 4, False), (36, 33, 4, True), (128, 513, 8, False),
                                        (128, 513, 8, True)])
def test_x_mask_embedding_half_every_element(E, B, T, attn):
    """test_embedding_gradient's device: the backward reads its token array for dEmb alone, so with the tokens replaced by
    0, 1, 2, ... (V >= B T) row bt of dEmb is dX[bt][:E] x mask.  Its zeros are the mask; its kept values are held to
    the float64 dX (2e-4 of the largest)."""
    BT = B * T
    V = max(BT, 40)
    shape = (V, E, 64, 1, attn)
    p = 0.3
    m, sd64, cfg = _plain(shape)
    enc = enc_for(shape, B, seed=23)
    toks = torch.from_numpy(synth.randint(32, "tok", (B, T), 0, V)).to(DEV, torch.int32).contiguous()
    alone = torch.arange(BT, dtype=torch.int32, device=DEV).reshape(B, T)
    grads, _, _, tape = _backward_both(m.decoder, sd64, cfg, enc, toks, _dlogits(B, T, V), p, SEED, alone)
    dx64 = torch.stack([x.grad for x in tape["x"]], dim=1).reshape(BT, 2 * E).cpu().numpy()       # d loss / d X
    keep = _x_keep(B, T, E, attn, p, SEED)[:, :E]
    got = grads["embedding.weight"]
    assert not got[BT:].any()
    tag = f"X embedding half E={E} B={B} T={T}" + (" attention" if attn else "")
    _pattern(got[:BT], keep, dx64[:, :E], tag)
    want = dx64[:, :E] * keep * R.scale(p)
    err = float(np.abs(got[:BT] - want).max()) / float(np.abs(want).max())
    record(f"dropout {tag}: dEmb rows vs float64 [rel to max|ref|]", err)
    assert err <= 2e-4, err


@pytest.mark.parametrize("attn,B,T", [(False, 33, 1), (False, 257, 1), (True, 33, 4)])
def test_x_mask_enc_half_every_element(attn, B, T):
    """Plain path, T = 1: d enc[b][e] = dX[b][E + e] x mask at the flat index b 2E + E + e.  Attention path: the enc
    half is not masked, so d enc (a sum over t) has no zero wherever float64 has none."""
    E = 36
    V = 50
    shape = (V, E, 64, 1, attn)
    p = 0.5
    m, sd64, cfg = _plain(shape)
    enc = enc_for(shape, B, seed=24)
    toks = torch.from_numpy(synth.randint(33, "tok", (B, T), 0, V)).to(DEV, torch.int32).contiguous()
    _, denc, ref, tape = _backward_both(m.decoder, sd64, cfg, enc, toks, _dlogits(B, T, V), p, SEED)
    tag = f"X enc half B={B} T={T}" + (" attention" if attn else "")
    if attn:
        _pattern(denc, np.ones((B, E), dtype=bool), ref["d enc"].cpu().numpy(), tag)
    else:
        dx64 = tape["x"][0].grad.cpu().numpy()
        _pattern(denc, _x_keep(B, T, E, False, p, SEED)[:, E:], dx64[:, E:], tag)
    want = ref["d enc"].cpu().numpy()
    err = float(np.abs(denc - want).max()) / float(np.abs(want).max())
    record(f"dropout {tag}: d enc vs float64 [rel to max|ref|]", err)
    assert err <= 2e-4, err


@pytest.mark.parametrize("seed", [SEED, 2 ** 64 - 1])
@pytest.mark.parametrize("attn", [False, True], ids=["plain", "attention"])
@pytest.mark.parametrize("flags", [0, BATCHED], ids=["rows", "batched"])
def test_inter_layer_and_stored_masks_every_element(flags, attn, seed):
    """B = T = 1, L = 3: every gradient is an outer product of one gate-gradient vector and one input vector, so zero
    columns and zero rows read out single mask elements.
      columns of dW_ih_l0        the mask X was STORED with by the forward (both halves plain, embedding half with attention)
      columns of dW_ih_l1 / _l2  stream 8 / 9 as the backward rebuilds the dropped layer input
      rows of db_ih_l0 / _l1     stream 8 / 9 as the BPTT applies it to the gradient handed down (gates i, g, o of unit
                                 j; the forget gate's gradient is zero at t = 0)
      d enc                      the enc half of X (plain), or no zero at all (attention)"""
    V, E, H, L = 50, 36, 64, 3
    shape = (V, E, H, L, attn)
    p = 0.5
    m, sd64, cfg = _plain(shape)
    enc = enc_for(shape, 1, seed=25)
    toks = torch.full((1, 1), 7, dtype=torch.int32, device=DEV)
    with flagged(m.decoder, flags):
        # d logits in [-100, 100]: the smallest of the 64 gate gradients of a layer stays above the 1e-6 of a judged
        # position (at [-1, 1] one unit's input gate sat below it, and one of 64 is more than the 1 % allowed)
        grads, denc, ref, tape = _backward_both(m.decoder, sd64, cfg, enc, toks, 100.0 * _dlogits(1, 1, V), p, seed)
    tag = ("batched" if flags else "rows") + (" attention" if attn else " plain") + f" seed {seed:#x}"
    grp = "B=T=1 L=3 " + ("batched" if flags else "rows")
    dg64 = [ref[f"lstm.bias_ih_l{l}"].cpu().numpy() for l in range(L)]               # gate gradients (B = T = 1)
    x_keep = _x_keep(1, 1, E, attn, p, seed)[0]
    x_raw = torch.cat([sd64["decoder.embedding.weight"][7], enc.double()[0]]).cpu().numpy()
    col = lambda w: np.abs(w).max(axis=0)                                            # noqa: E731
    _pattern(col(grads["lstm.weight_ih_l0"]), x_keep, x_raw * np.abs(dg64[0]).max(), f"stored X, {tag}", grp)
    for l in range(L - 1):
        keep = R.keep_mask(seed, R.DS_LAYER0 + l, H, p)
        h_raw = tape["h"][l][0].detach()[0].cpu().numpy()
        _pattern(col(grads[f"lstm.weight_ih_l{l + 1}"]), keep, h_raw * np.abs(dg64[l + 1]).max(),
                 f"rebuilt input of layer {l + 1}, {tag}", grp)
        low = tape["below"][l][0].grad[0].cpu().numpy()                              # handed down, before the mask
        i, g, o, c = (v[0].cpu().numpy() for v in tape["cell"][l][0])
        tc = np.tanh(c)
        dc = o * (1 - tc * tc)
        factor = {0: dc * g * i * (1 - i), 2: dc * i * (1 - g * g), 3: tc * o * (1 - o)}
        db = grads[f"lstm.bias_ih_l{l}"]
        assert not db[H:2 * H].any()
        for gate, f in factor.items():
            _pattern(db[gate * H:(gate + 1) * H], keep, low * f, f"BPTT into layer {l} gate {gate}, {tag}", grp)
    d64 = ref["d enc"].cpu().numpy()
    if attn:
        _pattern(denc, np.ones((1, E), dtype=bool), d64, f"d enc, {tag}", grp)
    else:
        _pattern(denc[0], x_keep[E:], tape["x"][0].grad[0, E:].cpu().numpy(), f"d enc, {tag}", grp)
    for n, g in [("d enc", denc)] + list(grads.items()):
        if n.startswith("attention."):
            assert not g.any()
            continue
        want = ref[n].cpu().numpy()                             # dW_hh is zero at T = 1: h(-1) = 0
        err = float(np.abs(g - want).max()) / max(float(np.abs(want).max()), 1e-12)
        record(f"dropout B=T=1 L=3 {tag}: gradients vs float64 [rel to max|ref|]", err)
        assert err <= 2e-4, (n, err)


# ------------------------------------------------------------------------------------------------ (c) through the surface
@pytest.mark.parametrize("k", [0, 5])
def test_decoder_forward_draws_the_seed_it_hands_to_the_kernels(k):
    """LSTMDecoder.forward in train mode draws torch.randint(0, 2**62, (1,)) from the default generator; the same draw
    under the same manual_seed gives the seed of the masks the logits were computed with."""
    B, T, p = 5, 5, 0.3
    m, sd64, cfg = build(TWO)
    forms = _forms(TWO[0], B, T)
    enc = enc_for(TWO, B, seed=21)
    with dropout_mode(m.decoder, p):
        torch.manual_seed(k)
        logits = m.decoder(enc, forms[:, :-1])
    torch.manual_seed(k)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    with torch.no_grad():
        ref = R.decoder_forward_masked(sd64, cfg, enc.double(), forms[:, :-1], p, seed)
    err = float((logits.detach().double() - ref).abs().max())
    record("dropout LSTMDecoder.forward logits vs float64 under the drawn seed [abs]", err)
    assert err <= 1e-4, err


def test_train_step_seeds_reach_the_kernels():
    """Two optimizer steps and two accumulation micro-steps of TrainStep on a tiny two-layer model, dropout 0.3: each
    call's logits are the float64 masked forward of the parameters it started from under TrainStep.step_seed of that
    call (the CNN encoder draws nothing: enc = model.encoder(images)), the four seeds differ, and so do the logits."""
    from img2latex_amd.training import TrainStep
    p = 0.3
    cfg = synth.model_config(vocab_size=50, embedding_dim=32, hidden_dim=64, lstm_layers=2, attention=True, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16), dropout=p)
    x = images(cfg, batch=8, device=DEV)
    forms = torch.from_numpy(synth.make_formulas(8, 14, cfg["vocab_size"], seed=5, min_len=6)).to(DEV)
    torch.manual_seed(0)
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg)).to(DEV)
    ts = TrainStep(m, seed=11)
    m.train()
    seen = []

    def observed(call):
        """Runs ``call``; keeps the logits of the forward_backward inside it, its seed and the float64 reference."""
        sd64 = {n: v.detach().double().clone() for n, v in m.state_dict().items() if n.startswith("decoder.")}
        with torch.no_grad():
            enc = m.encoder(x).double()
        inner, kept = ts.forward_backward, {}

        def spy(*a):
            kept["logits"] = inner(*a).detach().clone()
            return kept["logits"]

        ts.forward_backward = spy
        try:
            call()
        finally:
            del ts.forward_backward
        with torch.no_grad():
            ref = R.decoder_forward_masked(sd64, cfg, enc, forms[:, :-1], p, ts.step_seed)
        seen.append((ts.step_seed, kept["logits"], ref))

    observed(lambda: (ts.forward_backward(x, forms), ts.apply()))
    observed(lambda: (ts.forward_backward(x, forms), ts.apply()))
    observed(lambda: ts.micro_step(x, forms, 2, update=False))
    observed(lambda: ts.micro_step(x, forms, 2, update=True))
    assert [s for s, _, _ in seen] == [step_seed(11, 0, 0, 0), step_seed(11, 1, 0, 0), step_seed(11, 2, 0, 0),
                                       step_seed(11, 2, 0, 1)]
    assert len({s for s, _, _ in seen}) == 4
    for i, (s, logits, ref) in enumerate(seen):
        err = float((logits.double() - ref).abs().max())
        record("dropout TrainStep logits vs float64 under step_seed [abs]", err)
        assert err <= 1e-4, (i, err)
    for i in range(3):
        assert not torch.equal(seen[i][1], seen[i + 1][1]), i
    # calls 3 and 4 start from the same parameters: only the micro-step's share of the seed parts them
    assert float((seen[2][1] - seen[3][1]).abs().max()) > 1e-3
