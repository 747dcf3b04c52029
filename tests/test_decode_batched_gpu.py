"""The step-batched matrix-core decode (i2l_greedy_decode_batched, _lib.FLAG_DECODE_BATCHED) against the float64
restatement of test_decoder_shapes.py and the reference's own fixtures.  Shapes sit on the boundaries of the new kernels
(one column tile, Vp past one 512 chunk, H no multiple of 128 with three layers, the widest Vp, the shipped decoder);
rows 1, 5 and 33 are ragged against every row tile (16 / 32 / 64), 257 takes more than one 64-row tile.  Bounds are the
suite's: logits 1e-4 absolute, h / c 1e-5 relative to max(1,|ref|), ids equal to the float64 ids up to a row's first
step whose float64 top1-top2 margin is below 2e-4."""
import ctypes

import numpy as np
import pytest
import torch

import img2latex_oracle as O
from conftest import record
from helpers import END, START, _margin_guard, close, images, load, model_for, np_state_dict, padded_to_lists
from img2latex_amd import _lib, synth
from test_decoder_shapes import build, enc_for, oracle_greedy, oracle_steps, sid, tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 2e-4
FLAG = _lib.FLAG_DECODE_BATCHED
SHIPPED = (500, 512, 512, 2, True)
# (V, E, H, L, attention)
SHAPES = [
    (3, 4, 64, 1, False),           # one column tile; V below one MFMA tile
    (513, 256, 256, 1, False),      # Vp = 1024: first V past one 512 chunk
    (777, 36, 192, 3, True),        # H no multiple of 128; three layers; two-source K
    (2048, 64, 128, 2, True),       # widest Vp of the suite's ids tests
    SHIPPED,                        # the shipped decoder
]
CASES = [(s, None) for s in SHAPES] + [((777, 36, 192, 3, True), "negative")]     # no padding column may win
MANY_ROWS = {(513, 256, 256, 1, False), SHIPPED}
CASE_IDS = [sid(*c) for c in CASES]


def rows_of(shape):
    return (1, 5, 33) + ((257,) if shape in MANY_ROWS else ())


_GREEDY = {}


def greedy_reference(shape, variant, rows, steps=40):
    """float64 ids and margins of (case, rows), computed once and shared by the greedy and the sticky test."""
    key = (shape, variant, rows, steps)
    if key not in _GREEDY:
        _, sd64, cfg = build(shape, variant)
        _GREEDY[key] = oracle_greedy(sd64, cfg, enc_for(shape, rows, seed=9), steps)
    return _GREEDY[key]


# ------------------------------------------------------------------------------------------------ 1. teacher forcing
@pytest.mark.parametrize("T", [3, 9])
@pytest.mark.parametrize("shape,variant", CASES, ids=CASE_IDS)
def test_teacher_forced_logits_vs_float64(shape, variant, T):
    m, sd64, cfg = build(shape, variant)
    V, E, H, L, _ = shape
    tag = f"batched {sid(shape, variant)} T={T}"
    for rows in rows_of(shape):
        enc = enc_for(shape, rows)
        forced = tokens(shape, rows, T).to(torch.int32).contiguous()
        h0 = torch.from_numpy(synth.uniform(7, "h0", (L, rows, H), -0.9, 0.9)).to(DEV)
        c0 = torch.from_numpy(synth.uniform(7, "c0", (L, rows, H), -2.0, 2.0)).to(DEV)
        for hidden in (None, (h0, c0)):
            _, lg, (h, c) = m.decoder.run_steps(enc, T, forced[:, 0].contiguous(), forced=forced, hidden=hidden,
                                                want_ids=False, want_logits=True, want_state=True, flags=FLAG)
            ref, (rh, rc) = oracle_steps(sd64, cfg, enc, forced, None if hidden is None else (h0.double(), c0.double()))
            close(lg.cpu().numpy(), ref.cpu().numpy(), 1e-4, f"{tag} teacher-forced logits", absolute=True)
            close(h.cpu().numpy(), rh.cpu().numpy(), 1e-5, f"{tag} teacher-forced h")
            close(c.cpu().numpy(), rc.cpu().numpy(), 1e-5, f"{tag} teacher-forced c")
    assert m.decoder.kernel_flags == 0


# ------------------------------------------------------------------------------------------------ 2. greedy ids
@pytest.mark.parametrize("shape,variant", CASES, ids=CASE_IDS)
def test_greedy_ids_vs_float64(shape, variant):
    m, _, _ = build(shape, variant)
    V = shape[0]
    steps = 40
    runs = {
        "logits": dict(select=_lib.SELECT_LOGITS),
        "softmax": dict(select=_lib.SELECT_SOFTMAX),
        "temperature 0.7": dict(select=_lib.SELECT_LOGITS, temperature=0.7),
    }
    for rows in rows_of(shape):
        tag = f"batched {sid(shape, variant)} rows={rows}"
        enc = enc_for(shape, rows, seed=9)
        ref, margins = greedy_reference(shape, variant, rows, steps)
        tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
        for what, kw in runs.items():
            ids, _, _ = m.decoder.run_steps(enc, steps, tok0, flags=FLAG, **kw)
            got = ids.cpu().numpy()
            assert got.min() >= 0 and got.max() < V, (tag, what)
            scaled = margins / kw.get("temperature", 1.0)        # logits / 0.7: same arg max, margins wider by 1 / 0.7
            left = _margin_guard(got, ref, scaled, MARGIN)
            near = int((scaled.min(axis=1) < MARGIN).sum())      # rows whose float64 margin dips below 2e-4 somewhere
            record(f"{tag} greedy ({what}): rows leaving the float64 ids at a near-tie", left)
            record(f"{tag} greedy ({what}): rows with a float64 margin below 2e-4", near)
            assert left <= near, (tag, what, left, near)
            if variant != "negative":                           # 2 of its 5 rows are near-ties: the guard carries it
                assert rows - left >= 0.9 * rows, (tag, what, left)


# ------------------------------------------------------------------------------------------------ 3. sticky stop
@pytest.mark.parametrize("shape,variant", CASES, ids=CASE_IDS)
def test_sticky_stop(shape, variant):
    m, _, _ = build(shape, variant)
    steps = 40
    for rows in rows_of(shape):
        tag = (sid(shape, variant), rows)
        enc = enc_for(shape, rows, seed=9)
        tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
        free, _, _ = m.decoder.run_steps(enc, steps, tok0, flags=FLAG)
        sticky, _, _ = m.decoder.run_steps(enc, steps, tok0, stop=_lib.STOP_STICKY, end_id=END, flags=FLAG)
        free, sticky = free.cpu().numpy(), sticky.cpu().numpy()
        last = 0
        for b in range(rows):
            ends = np.nonzero(free[b] == END)[0]
            n = int(ends[0]) + 1 if ends.size else steps
            last = max(last, n)
            assert np.array_equal(sticky[b, :n], free[b, :n]) and (sticky[b, n:] == -1).all(), (tag, b)
        if shape == SHIPPED:      # every row ends well before step 40: the launches of the later steps return at once
            assert last < steps, (tag, last)
        assert (sticky[:, last:] == -1).all(), tag


# ------------------------------------------------------------------------------------------------ 4. the reference's fixtures
FIXTURES = ["tiny_l2_attn", "odd_dims", "odd_hidden", "secondary", "shipped_128x800"]


def _sd64(name):
    return {k: torch.from_numpy(v).to(DEV, torch.float64) for k, v in np_state_dict(name).items() if k.startswith("decoder.")}


def replay_margins(name, cfg, enc, seq):
    """float64 top1-top2 margins (B, n - 1) of the decoder replayed along ``seq`` (B, n), START in column 0: entry t
    belongs to the step that chose seq[:, t + 1]."""
    sd64, e64 = _sd64(name), enc.double()
    seq = torch.as_tensor(np.asarray(seq), dtype=torch.long, device=DEV)
    hidden, out = None, []
    with torch.no_grad():
        for t in range(seq.shape[1] - 1):
            lg, hidden = O.decode_step(sd64, cfg, e64, seq[:, t:t + 1], hidden)
            top = lg.squeeze(1).topk(2, dim=-1).values
            out.append(top[:, 0] - top[:, 1])
    return torch.stack(out, 1).cpu().numpy()


def near_tie_rows(name, cfg, enc, got, want, scale=1.0):
    """``got`` / ``want``: per row a list of ids, START first.  A row may differ from the fixture only from a step on whose
    float64 margin (replayed along the fixture's row, divided by ``scale``) is below 2e-4.  Returns the rows that do."""
    n = max(max(len(r) for r in want), max(len(r) for r in got))
    pad = lambda r: list(r) + [END] * (n + 1 - len(r))                      # noqa: E731
    w, g = np.array([pad(r) for r in want]), np.array([pad(r) for r in got])
    margins = replay_margins(name, cfg, enc, w) / scale
    rows = []
    for b in range(len(want)):
        ne = np.nonzero(w[b] != g[b])[0]
        if ne.size:
            t = int(ne[0]) - 1                                              # the step that chose column ne[0]
            assert t >= 0 and margins[b, t] < MARGIN, f"{name} row {b} step {t}: ids differ at margin {margins[b, t]}"
            rows.append(b)
    return rows


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_decode_step_under_the_flag(name):
    d, cfg, _ = load(name)
    m, _ = model_for(name)
    enc = torch.from_numpy(d["g1_enc"]).to(DEV)
    tok = torch.full((4, 1), START, dtype=torch.long, device=DEV)
    hidden = None
    m.decoder.kernel_flags |= FLAG
    try:
        with torch.no_grad():
            for s in range(3):
                logits, hidden = m.decoder.decode_step(enc, tok, hidden)
                assert logits.shape == (4, 1, cfg["vocab_size"])
                close(logits.cpu().numpy(), d[f"g2_logits{s}"], 1e-4, f"batched {name} decode_step logits", absolute=True)
                close(hidden[0].cpu().numpy(), d[f"g2_h{s}"], 1e-5, f"batched {name} decode_step h")
                close(hidden[1].cpu().numpy(), d[f"g2_c{s}"], 1e-5, f"batched {name} decode_step c")
                got = logits.squeeze(1).argmax(-1, keepdim=True).cpu().numpy()
                top = np.sort(d[f"g2_logits{s}"].reshape(4, -1).astype(np.float64), axis=1)
                for b in np.nonzero(got[:, 0] != d[f"g2_tok{s}"][:, 0])[0]:
                    assert top[b, -1] - top[b, -2] < MARGIN, (name, s, b)
                tok = torch.from_numpy(d[f"g2_tok{s}"]).to(DEV)             # along the fixture's tokens
    finally:
        m.decoder.kernel_flags &= ~FLAG
    assert m.decoder.kernel_flags == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_greedy_and_sticky_ids_under_the_flag(name):
    d, cfg, _ = load(name)
    m, _ = model_for(name)
    x = images(cfg, device=DEV)
    m.decoder.kernel_flags |= FLAG
    try:
        with torch.no_grad():
            enc = m.encoder(x)
            ids = m.inference(x, START, END, max_length=32)
            one = m.inference(x[1:2], START, END, max_length=32)
            idt = m.inference(x, START, END, max_length=12, temperature=0.7)
            stk, _ = m.greedy_ids(enc, START, END, 32, stop=_lib.STOP_STICKY, select=_lib.SELECT_SOFTMAX)
    finally:
        m.decoder.kernel_flags &= ~FLAG
    assert m.decoder.kernel_flags == 0
    moved = 0
    for what, got, want, e, scale in (("b4", ids, d["g3_b4_ids"].tolist(), enc, 1.0),
                                      ("b1", [list(one)], [d["g3_b1_ids"].tolist()], enc[1:2], 1.0),
                                      ("b4 temperature 0.7", idt, d["g3_b4_temp_ids"].tolist(), enc, 0.7)):
        got = [list(map(int, r)) for r in got]
        if got != want:                                                     # only a near-tie of the fixture may move a row
            rows = near_tie_rows(name, cfg, e, got, want, scale)
            assert rows, (name, what, "ids differ without a differing row (length only)")
            moved += len(rows)
    rows = []
    for r in stk.cpu().tolist():
        r = [t for t in r if t >= 0]
        rows.append(r[: r.index(END)] if END in r else r)
    want = padded_to_lists(d["g5_ids"], d["g5_len"])
    if rows != want:
        moved += len(near_tie_rows(name, cfg, enc, [[START] + r for r in rows], [[START] + r for r in want]))
    record(f"batched {name}: fixture id rows moved at a near-tie", moved)


# ------------------------------------------------------------------------------------------------ 5. flag off is the parent
def test_flag_off_is_the_row_kernel_call():
    """run_steps without the flag = i2l_greedy_decode_ex called directly: the routing took nothing over."""
    m, _, _ = build(SHIPPED)
    dec = m.decoder
    assert dec.kernel_flags == 0
    rows, steps = 5, 24
    enc = enc_for(SHIPPED, rows, seed=9)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    for kw in (dict(select=_lib.SELECT_LOGITS, stop=_lib.STOP_NONE), dict(select=_lib.SELECT_SOFTMAX, stop=_lib.STOP_STICKY)):
        via, _, _ = dec.run_steps(enc, steps, tok0, end_id=END, **kw)
        w, keep, enc_c = dec.prepare(enc)
        direct = torch.empty((rows, steps), dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib().i2l_greedy_decode_ex(ctypes.byref(w), dec._ws.data_ptr(), rows, steps, tok0.data_ptr(), None,
                                                   None, None, 1.0, kw["select"], kw["stop"], END, 0, direct.data_ptr(),
                                                   None, None, None, 0, None, 0, _lib.stream_ptr()), "greedy_decode_ex")
        torch.cuda.synchronize()
        del keep
        assert torch.equal(via, direct)
        flagged, _, _ = dec.run_steps(enc, steps, tok0, end_id=END, flags=FLAG, **kw)
        assert flagged.shape == via.shape and flagged.dtype == via.dtype


# ------------------------------------------------------------------------------------------------ 6. Predictor
def test_predictor_decode_flags():
    from img2latex_amd.training import Predictor, TokenTable
    name = "shipped_128x800"
    d, cfg, _ = load(name)
    m, _ = model_for(name)
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, cfg["vocab_size"])})
    table = TokenTable(vocab, max_sequence_length=150)
    x = images(cfg, device=DEV)
    old = getattr(m.encoder, "eval_precision", None)
    if old is not None:
        m.encoder.eval_precision = "fp32"       # one and two trunks in flight then give bit-identical features
    try:
        off = Predictor(m, table, device=torch.device(DEV))
        on = Predictor(m, table, device=torch.device(DEV), decode_flags=FLAG)
        assert off.decode_flags == 0 and on.decode_flags == FLAG
        want = off.predict_batch_ids(x, max_length=32)
        got = on.predict_batch_ids(x, max_length=32)
        if got != want:
            with torch.no_grad():
                enc = m.encoder(x)
            # cut rows end before END: compare them with the END the loop saw put back
            fin = lambda rows: [r + [END] if len(r) < 33 else r for r in rows]      # noqa: E731
            moved = near_tie_rows(name, cfg, enc, fin(got), fin(want))
            record(f"batched {name}: predict_batch_ids rows moved at a near-tie", len(moved))
        stream = list(on.predict_ids_stream(iter([x]), max_length=32))
        assert stream == [got]
    finally:
        if old is not None:
            m.encoder.eval_precision = old
    assert m.decoder.kernel_flags == 0
