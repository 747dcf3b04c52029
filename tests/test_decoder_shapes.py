"""The decoder kernels (inference, sampling, beam search, training) against a float64 restatement (the oracle evaluated
in float64 on the device) at the dimensions they accept beyond the fixtures' ("Accepted decoder
dimensions"): every shape sits on a branch or LDS boundary.  Bounds are the suite's: logits 1e-4 absolute, h / c 1e-5
relative to max(1,|ref|), gradients and d(enc) 2e-4 relative to max|ref|, sampling probabilities 1e-5; ids equal the
float64 ids up to a row's first step whose float64 top1-top2 margin is below 2e-4 (helpers._margin_guard)."""
import numpy as np
import pytest
import torch

import img2latex_oracle as O
from conftest import record
from helpers import END, PAD, START, _margin_guard, check_sampling, close, load
from img2latex_amd import _lib, synth
from img2latex_amd.model import Seq2SeqModel

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 2e-4

# (V, E, H, L, attention)
SHAPES = [
    (3, 4, 64, 1, False),            # minimum
    (513, 256, 256, 1, False),       # first V off the grouped path: resident kernel, two 512-column passes
    (1024, 256, 256, 1, True),       # Vp 1024 ...
    (1025, 256, 256, 1, True),       # ... -> 1536
    (2048, 64, 128, 2, True),        # the sampling and beam limit
    (777, 36, 192, 3, True),         # the backward's 4-group split
    (5000, 100, 448, 4, False),      # L = 4, large V
    (1000, 512, 1024, 4, True),      # training forward LDS exactly 64 KiB
    (3072, 256, 2048, 2, False),     # inference only; SELECT_SOFTMAX needs 63 544 B of LDS
]
# + the output layer's "negative" variant (see build): every logit negative, no padding column may win
CASES = [(s, None) for s in SHAPES] + [((777, 36, 192, 3, True), "negative")]
MANY_ROWS = {(513, 256, 256, 1, False), (5000, 100, 448, 4, False)}     # rows 257 / 513: two / four rows per workgroup
# beam widths accepted by the generic beam kernel (K <= V, Vp <= 2048, LDS <= 160 KiB); the others are refused below
BEAM_K = {(3, 4, 64, 1, False): (1, 3), (1000, 512, 1024, 4, True): (1,)}
BEAM_SHAPES = [s for s in SHAPES if s[0] <= 2048]


def sid(shape, variant=None):
    V, E, H, L, a = shape
    return f"V{V}_E{E}_H{H}_L{L}" + ("_attn" if a else "") + (f"_{variant}" if variant else "")


_MODELS = {}


def model_from_sd(cfg, sd):
    """(Seq2SeqModel on the device, float64 decoder state dict on the device) of a numpy state dict."""
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV).eval()
    sd64 = {k: torch.from_numpy(v).to(DEV, torch.float64) for k, v in sd.items() if k.startswith("decoder.")}
    return m, sd64


def shape_config(shape):
    V, E, H, L, attn = shape
    return synth.model_config(vocab_size=V, embedding_dim=E, hidden_dim=H, lstm_layers=L, attention=attn,
                              channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16))


def build(shape, variant=None, seed=None):
    """(Seq2SeqModel on the device, float64 decoder state dict on the device, cfg): synthetic weights; the encoder is a
    tiny one and unused -- every test feeds a synthetic encoder output.  ``variant`` "flat": output weights at
    8/sqrt(H) instead of 12 and no END clock, so that the sampling masks keep tens to hundreds of columns; "negative":
    output weights at 1/sqrt(H) and the output bias lowered by 20, so that every logit is negative.  ``seed``: of the
    weights, instead of the one derived from (H, L)."""
    key = (shape, variant, seed)
    if key not in _MODELS:
        V, E, H, L, attn = shape
        cfg = shape_config(shape)
        if seed is None:
            seed = 100 + H // 64 + 17 * L
        if variant == "flat":
            sd = synth.make_state_dict(cfg, seed=seed, out_scale=8.0)
        elif variant == "negative":           # |W_out h| < sqrt(H) < 20
            assert H < 400
            sd = synth.make_state_dict(cfg, seed=seed, out_scale=1.0)
            sd["decoder.output_layer.bias"] = sd["decoder.output_layer.bias"] - np.float32(20.0)
        else:
            sd = synth.make_state_dict(cfg, seed=seed, out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
        _MODELS[key] = model_from_sd(cfg, sd) + (cfg,)
    return _MODELS[key]


def enc_for(shape, rows, seed=5):
    return torch.from_numpy(synth.uniform(seed, "enc", (rows, shape[1]), -1.5, 1.5)).to(DEV)


def tokens(shape, rows, T, seed=6):
    return torch.from_numpy(synth.randint(seed, "tokens", (rows, T), 0, shape[0])).to(DEV)


def oracle_steps(sd64, cfg, enc, toks, hidden=None):
    """float64 decode_step along the given tokens (B,T): logits (B,T,V) and the final (h, c)."""
    e64 = enc.double()
    out = []
    with torch.no_grad():
        for t in range(toks.shape[1]):
            lg, hidden = O.decode_step(sd64, cfg, e64, toks[:, t:t + 1].long(), hidden)
            out.append(lg)
    return torch.cat(out, 1), hidden


def oracle_greedy(sd64, cfg, enc, steps):
    """float64 greedy ids (B, 1 + steps, START first) along its own choices, and the top1-top2 margins (B, steps)."""
    e64 = enc.double()
    B = enc.shape[0]
    tok = torch.full((B, 1), START, dtype=torch.long, device=DEV)
    ids, margins, hidden = [tok], [], None
    with torch.no_grad():
        for _ in range(steps):
            lg, hidden = O.decode_step(sd64, cfg, e64, tok, hidden)
            top = lg.squeeze(1).topk(2, dim=-1)
            margins.append(top.values[:, 0] - top.values[:, 1])
            tok = top.indices[:, :1]
            ids.append(tok)
    return torch.cat(ids, 1).cpu().numpy(), torch.stack(margins, 1).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("T", [3, 9])
@pytest.mark.parametrize("shape,variant", CASES, ids=[sid(*c) for c in CASES])
def test_teacher_forced_logits_vs_float64(shape, variant, T):
    """Forced tokens from the zero state and from a given (h0, c0); T = 9 takes the resident kernels where they apply
    (T >= 8).  The automatic choice and 1, 2 and 4 rows per workgroup each stay within the bounds."""
    m, sd64, cfg = build(shape, variant)
    V, E, H, L, _ = shape
    tag = f"{sid(shape, variant)} T={T}"
    for rows in (1, 5) + ((257, 513) if shape in MANY_ROWS else ()):
        enc = enc_for(shape, rows)
        forced = tokens(shape, rows, T).to(torch.int32).contiguous()
        h0 = torch.from_numpy(synth.uniform(7, "h0", (L, rows, H), -0.9, 0.9)).to(DEV)
        c0 = torch.from_numpy(synth.uniform(7, "c0", (L, rows, H), -2.0, 2.0)).to(DEV)
        for hidden in (None, (h0, c0)):
            got = {}
            for r in (0, 1, 2, 4):
                _, lg, (h, c) = m.decoder.run_steps(enc, T, forced[:, 0].contiguous(), forced=forced, hidden=hidden,
                                                    want_ids=False, want_logits=True, want_state=True,
                                                    rows_per_workgroup=r)
                got[r] = (lg.cpu(), h.cpu(), c.cpu())
            ref, (rh, rc) = oracle_steps(sd64, cfg, enc, forced,
                                         None if hidden is None else (h0.double(), c0.double()))
            for r in (0, 1, 2, 4):
                close(got[r][0].numpy(), ref.cpu().numpy(), 1e-4, f"{tag} teacher-forced logits", absolute=True)
                close(got[r][1].numpy(), rh.cpu().numpy(), 1e-5, f"{tag} teacher-forced h")
                close(got[r][2].numpy(), rc.cpu().numpy(), 1e-5, f"{tag} teacher-forced c")
            # the row kernels' instantiations for 1, 2 and 4 rows round differently in the last bits (measured here)
            for r in (2, 4):
                record(f"{tag} teacher-forced logits, {r} vs 1 row(s) per workgroup [abs]",
                       float((got[r][0] - got[1][0]).abs().max()))


@pytest.mark.parametrize("shape,variant", CASES, ids=[sid(*c) for c in CASES])
def test_greedy_ids_vs_float64(shape, variant):
    """40 greedy steps: arg max of the logits, of the softmax, at temperature 0.7, and the sticky stop."""
    m, sd64, cfg = build(shape, variant)
    V = shape[0]
    tag = sid(shape, variant)
    rows, steps = 5, 40
    enc = enc_for(shape, rows, seed=9)
    ref, margins = oracle_greedy(sd64, cfg, enc, steps)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    runs = {
        "logits": dict(select=_lib.SELECT_LOGITS),
        "softmax": dict(select=_lib.SELECT_SOFTMAX),
        "temperature 0.7": dict(select=_lib.SELECT_LOGITS, temperature=0.7),
    }
    got = {}
    for what, kw in runs.items():
        ids, _, _ = m.decoder.run_steps(enc, steps, tok0, **kw)
        got[what] = ids.cpu().numpy()
        assert got[what].min() >= 0 and got[what].max() < V, (tag, what)
        # logits / 0.7 have the same arg max; their margins are wider by 1 / 0.7
        div = _margin_guard(got[what], ref, margins / kw.get("temperature", 1.0), MARGIN)
        record(f"{tag} greedy ({what}): rows leaving the float64 ids at a near-tie", div)
    sticky, _, _ = m.decoder.run_steps(enc, steps, tok0, stop=_lib.STOP_STICKY, end_id=END)
    sticky = sticky.cpu().numpy()
    for b in range(rows):
        ends = np.nonzero(got["logits"][b] == END)[0]
        n = int(ends[0]) + 1 if ends.size else steps
        assert np.array_equal(sticky[b, :n], got["logits"][b, :n]) and (sticky[b, n:] == -1).all(), (tag, b)


@pytest.mark.parametrize("V", [513, 1000, 2048])
def test_sampling_wide_vocabularies_vs_float64(V):
    """helpers.check_sampling at V > 512 (several columns per thread in the top-k and top-p masks)."""
    shape = next(s for s in SHAPES if s[0] == V)
    m, sd64, cfg = build(shape, "flat")
    enc = enc_for(shape, 6, seed=41)
    e64 = enc.double()

    def step(tok, hidden):
        return O.decode_step(sd64, cfg, e64, tok.to(DEV), hidden)

    for top_k in (1, 7, V):
        for top_p in (0.5, 0.95):
            check_sampling(m.decoder, enc, step, top_k, top_p, 1.0, seed=2024 + top_k, steps=6,
                           what=f"{sid(shape)} sampling top_k={top_k} top_p={top_p} probabilities")


BEAM_CASES = ([(s, None, k) for s in BEAM_SHAPES for k in BEAM_K.get(s, (1, 3, 7, 8))]
              + [(CASES[-1][0], "negative", 3), ("secondary", None, 7)])


@pytest.mark.parametrize("shape,variant,k", BEAM_CASES,
                         ids=[f"{s if isinstance(s, str) else sid(s, v)}-k{k}" for s, v, k in BEAM_CASES])
def test_beam_search_vs_float64(shape, variant, k):
    """The one-workgroup-per-image beam kernel (beam_kernel<K>), 2 images x 30 steps: sequences equal the float64
    search's wherever its ranking has no near-tie (smallest gap between neighbours among the k + 1 best candidates of
    a step >= 1e-4, as in test_cfg3_beam_full_size_vs_reference), winning scores within 1e-4."""
    if shape == "secondary":        # the shipped decoder dims: E = H = 512, L = 2
        _, cfg, sd_kw = load("secondary")
        sd = synth.make_state_dict(cfg, **sd_kw)
        m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
        m.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
        m = m.to(DEV).eval()
        sd64 = {n: torch.from_numpy(v).to(DEV, torch.float64) for n, v in sd.items() if n.startswith("decoder.")}
        shape_ = (cfg["vocab_size"], cfg["embedding_dim"], cfg["hidden_dim"], cfg["lstm_layers"], True)
        tag = "secondary"
    else:
        m, sd64, cfg = build(shape, variant)
        shape_, tag = shape, sid(shape, variant)
    enc = enc_for(shape_, 2, seed=13)
    with torch.no_grad():
        got, scores = m.beam_search_batch(enc, START, END, 30, k, return_scores=True, flags=_lib.FLAG_NO_GROUP)
    near, worst = 0, 0.0
    for j in range(2):
        st = {}
        seq, sc = O.beam_search(sd64, cfg, enc[j:j + 1].double(), START, END, 30, k, return_score=True, stats=st)
        assert all(0 <= t < shape_[0] for t in got[j]), (tag, k, j)
        if got[j] != seq:
            assert st["gap"] < 1e-4, (tag, k, j, st["gap"], got[j], seq)
            near += 1
            continue
        err = abs(scores[j] - sc) / max(1.0, abs(sc))
        worst = max(worst, err)
        assert err <= 1e-4, (tag, k, j, scores[j], sc)
    record(f"{tag} beam k={k} winning score vs float64 [rel to max(1,|score|)]", worst)
    record(f"{tag} beam k={k}: searches leaving the float64 one at a near-tie", near)


# ---------------------------------------------------------------------------------------------------------------- training
TRAIN_SHAPES = [s for s in SHAPES if s[2] <= 1024]


@pytest.mark.parametrize("B,T", [(1, 5), (1, 12), (5, 5), (5, 12), (257, 5), (257, 12)])
@pytest.mark.parametrize("shape", TRAIN_SHAPES, ids=[sid(s) for s in TRAIN_SHAPES])
def test_decoder_training_vs_float64(shape, B, T):
    """Teacher-forced training forward and BPTT backward through model.decoder (autograd + DecoderTeacherForcedFn,
    torch's CE on the logits) against the float64 oracle's autograd: logits, d(enc) and every parameter gradient.
    B = 257 runs two rows per workgroup."""
    m, sd64, cfg = build(shape)
    V = shape[0]
    tag = f"{sid(shape)} B={B} T={T}"
    forms = torch.from_numpy(synth.randint(777, "forms", (B, T + 1), 0, V)).to(DEV)
    forms[:, 0] = START
    forms[0, 1] = max(V - 1, 1)                       # at least one target is not PAD
    enc = enc_for(shape, B, seed=21)
    params = {n: v.clone().requires_grad_(True) for n, v in sd64.items()}
    enc64 = enc.double().requires_grad_(True)
    ref_logits = O.decoder_forward(params, cfg, enc64, forms[:, :-1])
    O.ce_label_smooth(ref_logits, forms[:, 1:], PAD).backward()
    dec = m.decoder
    dec.train()
    try:
        for p in dec.parameters():
            p.grad = None
        enc_dev = enc.clone().requires_grad_(True)
        logits = dec(enc_dev, forms[:, :-1])
        close(logits.detach().cpu().numpy(), ref_logits.detach().cpu().numpy(), 1e-4, f"{tag} training-forward logits",
              absolute=True)
        crit = torch.nn.CrossEntropyLoss(ignore_index=PAD, reduction="mean", label_smoothing=0.1)
        crit(logits.transpose(1, 2), forms[:, 1:]).backward()
    finally:
        dec.eval()
    grads = [("d enc", enc_dev.grad, enc64.grad)]
    grads += [(n, p.grad, params["decoder." + n].grad) for n, p in dec.named_parameters()]
    for n, g, ref in grads:
        if n.startswith("attention."):            # the context over one source position does not depend on them
            assert float(g.abs().max()) == 0.0 and float(ref.abs().max()) == 0.0
            continue
        g, ref = g.double().cpu(), ref.cpu()
        err = float((g - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)
        record(f"{sid(shape)} training gradient [rel to max|ref|]", err)
        assert err <= 2e-4, (tag, n, err)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _model(V, E, H, L, attn=False):
    torch.manual_seed(0)
    cfg = synth.model_config(vocab_size=V, embedding_dim=E, hidden_dim=H, lstm_layers=L, attention=attn,
                             channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16))
    return Seq2SeqModel("cnn_lstm", V, synth.encoder_params(cfg), synth.decoder_params(cfg)).to(DEV).eval()


def _step(m, rows=2, **kw):
    enc = torch.zeros(rows, m.decoder.embedding_dim, device=DEV)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    return m.decoder.run_steps(enc, 3, tok0, want_logits=True, **kw)


@pytest.mark.parametrize("what", ["H=96", "E=30", "L=5", "H=2112", "training H=1088", "softmax V=3073 H=2048",
                                  "sampling V=2049", "sampling hidden of 1 row for 2", "beam Vp>2048", "beam k=8 at E=H=512 L=2", "beam k>V"])
def test_decoder_refusals(what):
    """Dimensions outside DESIGN.md's table raise through the Python surface (the C ABI refuses before it launches
    anything) instead of returning numbers."""
    enc1 = lambda m: torch.zeros(1, m.decoder.embedding_dim, device=DEV)     # noqa: E731
    if what in ("H=96", "E=30", "L=5", "H=2112"):
        m = _model(10, 30 if what == "E=30" else 4, {"H=96": 96, "H=2112": 2112}.get(what, 64), 5 if what == "L=5" else 1)
        with pytest.raises(RuntimeError):
            _step(m)
    elif what == "training H=1088":
        m = _model(10, 4, 1088, 1)
        _, lg, _ = _step(m)                                          # inference takes H = 1088 ...
        assert bool(torch.isfinite(lg).all())
        m.decoder.train()
        enc = torch.zeros(2, 4, device=DEV, requires_grad=True)
        with pytest.raises(RuntimeError):                            # ... training does not
            m.decoder(enc, torch.full((2, 3), START, dtype=torch.long, device=DEV))
    elif what == "softmax V=3073 H=2048":
        m = _model(3073, 256, 2048, 2)
        _step(m, select=_lib.SELECT_LOGITS)
        with pytest.raises(RuntimeError):                            # 65 592 B of LDS
            _step(m, select=_lib.SELECT_SOFTMAX)
    elif what == "sampling V=2049":
        m = _model(2049, 4, 64, 1)
        tok0 = torch.full((2,), START, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError):
            m.decoder.sample_steps(torch.zeros(2, 4, device=DEV), 3, tok0, 1.0, 5, 0.0, 1)
    elif what == "sampling hidden of 1 row for 2":
        m = _model(10, 4, 64, 1)
        tok0 = torch.full((2,), START, dtype=torch.int32, device=DEV)
        short, right = torch.zeros(1, 1, 64, device=DEV), torch.zeros(1, 2, 64, device=DEV)
        for hidden in ((short, short), (right, short), (short, right)):
            for flags in (0, _lib.FLAG_DECODE_BATCHED):
                with pytest.raises(RuntimeError, match="hidden state must be"):      # run_steps' refusal, same words
                    m.decoder.sample_steps(torch.zeros(2, 4, device=DEV), 3, tok0, 1.0, 5, 0.0, 1, hidden=hidden, flags=flags)
        assert m.decoder._ws is None                                 # refused before the workspace: nothing was launched
        with pytest.raises(RuntimeError, match="hidden state must be"):
            _step(m, hidden=(short, short))
    elif what == "beam Vp>2048":
        m = _model(2049, 4, 64, 1)
        with pytest.raises(RuntimeError):
            m.beam_search_batch(enc1(m), START, END, 5, 3)
    elif what == "beam k=8 at E=H=512 L=2":
        m = _model(512, 512, 512, 2, attn=True)
        m.beam_search_batch(enc1(m), START, END, 5, 7)               # 143 992 B: accepted
        with pytest.raises(RuntimeError):                            # 164 624 B > 160 KiB
            m.beam_search_batch(enc1(m), START, END, 5, 8, flags=_lib.FLAG_NO_GROUP)
    elif what == "beam k>V":
        m = _model(3, 4, 64, 1)
        with pytest.raises(RuntimeError):
            m.beam_search_batch(enc1(m), START, END, 5, 5)
