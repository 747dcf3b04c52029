"""The argument-complete decode on the device (i2l_arguments_pick_logits, i2l_greedy_decode_arguments,
i2l_sample_decode_arguments and the Python surface above them) against the host restatement of the rules,
``ArgumentTable.replay`` (training/constraint.py; tests/test_argument_rules_host.py holds the C++ rules to the same
restatement and to an independent recogniser).  Everything here is exact: ids, masks and state bytes are integers, and the
sampling rule is compared bit for bit with the unconstrained entry run on a row that holds -inf in the refused columns."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import END, GOLDEN, START
from img2latex_amd import _lib, synth
from img2latex_amd.model import LSTMDecoder
from img2latex_amd.training import constraint as C
from img2latex_amd.training.constraint import ArgumentState, ArgumentTable, BracketTable, argument_byte
from test_decoder_shapes import enc_for, model_from_sd, shape_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAG = _lib.FLAG_DECODE_BATCHED
SEED = 4711
ROWS = 67
SB = C.ARGUMENT_STATE_BYTES
BRACE_OPEN, BRACE_CLOSE = 4, 5


def table_for(V, seed, kinds=3):
    """END = 2 neutral, PAD / START / UNK never, { and } in columns 4 and 5; of the other columns some open or close one of
    ``kinds`` kinds (every kind at least once each way), some demand 1..3 arguments -- strict or loose, opening or not --
    a few are never, the rest plain."""
    rng = np.random.default_rng(seed)
    t = np.zeros(V, dtype=np.uint8)
    t[[0, 1, 3]] = 255
    t[BRACE_OPEN], t[BRACE_CLOSE] = C.open_class(0), C.close_class(0)
    cols = 6 + rng.permutation(V - 6)
    for k in range(1, kinds):
        t[cols[2 * k]], t[cols[2 * k + 1]] = C.open_class(k), C.close_class(k)
    for v in cols[2 * kinds:]:
        r = rng.random()
        if r < 0.3:
            k = int(rng.integers(kinds))
            t[v] = C.open_class(k) if r < 0.15 else C.close_class(k)
        elif r < 0.35:
            t[v] = rng.choice([255, 9, 0x80, 0x40, 0x15])
        elif r < 0.6:
            opening = rng.random() < 0.3
            t[v] = argument_byte(C.open_class(int(rng.integers(kinds))) if opening else 0, int(rng.integers(1, 4)),
                                 bool(rng.random() < 0.5))
    return ArgumentTable(t, END)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def zero_state(rows):
    return torch.zeros(SB * rows, dtype=torch.uint8, device=DEV)


def prominent(table):
    """The columns a biased run pushes: opens and demanding columns."""
    return ((table.classes >= 1) & (table.classes <= 4)) | (table.counts > 0)


_RUNS = {}


def rule_run(V, steps, biased):
    """One run of the greedy rule over random logits, shared by the tests below: the host's logits (steps, ROWS, V + 3)
    with 1e30 in the pad columns, the table, the replay of every row, and the device's ids / masks / state bytes of every
    step from one i2l_arguments_pick_logits call per step."""
    key = (V, steps, biased)
    if key in _RUNS:
        return _RUNS[key]
    rng = np.random.default_rng(1000 * V + steps)
    table = table_for(V, seed=V + steps)
    x = np.full((steps, ROWS, V + 3), 1e30, dtype=np.float32)
    x[:, :, :V] = rng.standard_normal((steps, ROWS, V)).astype(np.float32) * 2.0
    if biased:
        x[:, :, :V][:, :, prominent(table)] += 3.0
    xd = torch.from_numpy(x).to(DEV)
    state = zero_state(ROWS)
    ids, masks, states = [], [], []
    for t in range(steps):
        i, _, a = LSTMDecoder.arguments_pick_logits(xd[t][:, :V], table, END, state, t, steps, want_allowed=True)
        ids.append(i)
        masks.append(a)
        states.append(state.clone())
    ids = torch.stack(ids).cpu().numpy()                         # (steps, ROWS)
    masks = torch.stack(masks).cpu().numpy()                     # (steps, ROWS, V)
    states = torch.stack(states).cpu().numpy().reshape(steps, ROWS, SB)
    want = [table.replay(x[:, r, :V], END, steps) for r in range(ROWS)]
    _RUNS[key] = dict(V=V, steps=steps, table=table, x=x, xd=xd, ids=ids, masks=masks, states=states, want=want)
    return _RUNS[key]


RULE_CASES = [(37, 40, False), (200, 40, False), (37, 80, True)]


@pytest.mark.parametrize("V,steps,biased", RULE_CASES, ids=["V37", "V200", "V37_steps80_bias"])
def test_rule_on_callers_logits_equals_replay(V, steps, biased):
    run = rule_run(V, steps, biased)
    table, deepest = run["table"], 0
    for r, want in enumerate(run["want"]):
        for t, w in enumerate(want):
            assert run["ids"][t, r] == w["id"], (r, t)
            assert np.array_equal(run["masks"][t, r], w["allowed"]), (r, t)
            assert run["states"][t, r].tobytes() == w["state"].to_bytes(), (r, t, w["state"])
            deepest = max(deepest, w["state"].depth)
        ids = run["ids"][:, r].tolist()
        assert table.complete(ids, END), (r, ids)
        s = want[ids.index(END)]["state"]
        assert (s.depth, s.owed, s.pending, s.ended) == (0, 0, 0, 1)
    if biased:
        assert deepest == C.MAX_DEPTH


def test_rule_inputs_fire_every_rule():
    """A condition on the inputs of the three runs above: each rule overrode the unconstrained arg max somewhere."""
    fired = set()
    for case in RULE_CASES:
        fired |= {w["rule"] for want in rule_run(*case)["want"] for w in want if w["rule"]}
    assert fired == set(range(1, 10)), fired


def test_rule_engineered_ties_and_overrides():
    """Equal logits on two allowed columns: the lower index.  The largest logit on a refused column loses: after \\frac
    only { is picked, after ^ a plain token or {."""
    V, steps = 37, 10
    t = np.zeros(V, dtype=np.uint8)
    t[[0, 1, 3]] = 255
    t[10], t[11] = C.open_class(0), C.close_class(0)
    t[12], t[13] = C.open_class(1), C.close_class(1)
    FRAC, HAT, BEGIN, ENDENV = 14, 15, 16, 17
    t[FRAC], t[HAT] = argument_byte(0, 2), argument_byte(0, 1, True)
    t[BEGIN], t[ENDENV] = argument_byte(C.open_class(2), 1), C.close_class(2)
    table = ArgumentTable(t, END)
    x = np.zeros((6, V + 3), dtype=np.float32)
    x[:, V:] = 1e30
    x[0, [20, 30]] = 5.0            # two plain columns tie
    x[0, 11] = 9.0                  # a closer at depth 0
    x[1, FRAC] = 5.0
    x[2, HAT] = 5.0
    x[3, [2, 5]] = 5.0              # END and a plain column tie at depth 0: END is the lower index
    x[4, BEGIN] = 5.0
    x[5, HAT] = 5.0
    state = zero_state(6)
    ids, _, mask = LSTMDecoder.arguments_pick_logits(torch.from_numpy(x).to(DEV)[:, :V], table, END, state, 0, steps,
                                                     want_allowed=True)
    assert ids.cpu().tolist() == [20, FRAC, HAT, 2, BEGIN, HAT]
    mask = mask.cpu().numpy()
    assert not mask[:, [0, 1, 3, 11, 13, ENDENV]].any() and mask[:, [2, 5, 10, 12, FRAC, HAT, BEGIN, 20, 36]].all()
    want = [ArgumentState() for _ in range(6)]
    for s, i in zip(want, ids.cpu().tolist()):
        table.advance(s, i, END)
    assert want[1] == ArgumentState(pending=2, owed=4) and want[2] == ArgumentState(pending=1, loose=1, owed=1)
    assert want[4] == ArgumentState(stack=2, pending=1 << 2, depth=1, owed=2) and want[3] == ArgumentState(ended=1)
    assert state.cpu().numpy().tobytes() == b"".join(s.to_bytes() for s in want)
    # step 1
    y = np.zeros((6, V), dtype=np.float32)
    y[0, [FRAC, HAT]] = 5.0                                     # two demanding columns tie: the lower index
    y[1] = 9.0                                                  # after \frac: every column large, { the smallest
    y[1, 10] = -3.0
    y[2, [FRAC, 11, 2, HAT]] = 9.0                              # after ^: argument expected refuses the largest logits
    y[2, 20] = 2.0                                              #          a plain token wins
    y[3, 3] = 9.0                                               # ended: not constrained any more
    y[4, [ENDENV, 20]] = 9.0                                    # inside \begin{array}: its strict argument first
    y[5, [FRAC, 11, 2]] = 9.0                                   # after ^: { above the plain columns
    y[5, 10] = 1.0
    ids, _, mask = LSTMDecoder.arguments_pick_logits(torch.from_numpy(y).to(DEV), table, END, state, 1, steps,
                                                     want_allowed=True)
    assert ids.cpu().tolist() == [FRAC, 10, 20, 3, 10, 10]
    mask = mask.cpu().numpy()
    plain = np.flatnonzero(table.plain).tolist()
    assert np.flatnonzero(mask[1]).tolist() == [10] and np.flatnonzero(mask[4]).tolist() == [10]
    assert np.flatnonzero(mask[2]).tolist() == sorted(plain + [10]) == np.flatnonzero(mask[5]).tolist()
    assert mask[3].all()
    for s, i in zip(want, ids.cpu().tolist()):
        table.advance(s, i, END)
    assert state.cpu().numpy().tobytes() == b"".join(s.to_bytes() for s in want)


SETTINGS = [(5, 0.9), (5, 0.0), (0, 0.9)]


@pytest.mark.parametrize("V", [37, 200])
def test_sampling_is_the_plain_rule_on_masked_logits(V):
    """ids and probabilities of the constrained draw equal, bit for bit, i2l_sample_logits on a host-built copy of the row
    with -inf in the refused columns (same seed, same step); probabilities are exactly 0 there; a second call gives the
    same bits; the state moves as the host's ``advance`` moves it."""
    run = rule_run(V, 40, False)
    steps, table = run["steps"], run["table"]
    before = np.concatenate([np.zeros((1, ROWS, SB), np.uint8), run["states"][:-1]])
    for t in range(0, steps, 3):
        allowed = run["masks"][t].astype(bool)
        assert not allowed.all()
        masked = torch.from_numpy(np.where(allowed, run["x"][t][:, :V], -np.inf).astype(np.float32)).to(DEV)
        for top_k, top_p in SETTINGS:
            outs = []
            for _ in range(2):
                state = torch.from_numpy(before[t].reshape(-1).copy()).to(DEV)
                ids, probs, mask = LSTMDecoder.arguments_pick_logits(
                    run["xd"][t][:, :V], table, END, state, t, steps, temperature=0.8, top_k=top_k, top_p=top_p, seed=SEED,
                    want_probs=True, want_allowed=True)
                outs.append((ids.cpu().numpy(), probs.cpu().numpy(), mask.cpu().numpy(), state.cpu().numpy()))
            ids, probs, mask, after = outs[0]
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(outs[0], outs[1]))
            want_ids, want_probs = LSTMDecoder.sample_logits(masked, 0.8, top_k, top_p, SEED, step=t, want_probs=True)
            assert np.array_equal(ids, want_ids.cpu().numpy()), (t, top_k, top_p)
            assert np.array_equal(bits(probs), bits(want_probs.cpu().numpy())), (t, top_k, top_p)
            assert np.array_equal(mask.astype(bool), allowed)
            assert (probs[~allowed] == 0.0).all() and allowed[np.arange(ROWS), ids].all()
            for r in range(ROWS):
                st = ArgumentState.from_bytes(before[t, r].tobytes())
                table.advance(st, int(ids[r]), END)
                assert after.reshape(ROWS, SB)[r].tobytes() == st.to_bytes(), (t, r)


# ------------------------------------------------------------------------------------------------ the whole loop
SMALL, SHIPPED = (37, 64, 64, 2, False), (500, 512, 512, 2, True)
# (rows, steps, weight seed, bias on the bracket and demanding columns): picked on the CPU with the float64 oracle decoder
# so that the BRACKET-constrained greedy decode leaves at least a quarter of the rows incomplete (there: all 19 and all 33,
# no top-2 margin among the allowed columns below 1e-3); the test asserts it on the device's ids
LOOP = {SMALL: (19, 24, 5, 2.0), SHIPPED: (33, 20, 6, 2.0)}
_LOOP_MODELS = {}


def loop_table(V):
    t = np.zeros(V, dtype=np.uint8)
    t[[0, 1, 3, 10]] = 255
    for k in range(3):
        t[4 + 2 * k], t[5 + 2 * k] = C.open_class(k), C.close_class(k)
    t[8] = argument_byte(C.open_class(2), 1)                    # \begin{array}: opens and demands its column specification
    t[11], t[12] = argument_byte(0, 2), argument_byte(0, 1, True)          # \frac, ^
    t[13], t[14] = argument_byte(0, 2, True), argument_byte(0, 3)
    return ArgumentTable(t, END)


def loop_model(shape):
    if shape not in _LOOP_MODELS:
        _, _, seed, bias = LOOP[shape]
        cfg = shape_config(shape)
        sd = synth.make_state_dict(cfg, seed=seed, out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
        b = sd["decoder.output_layer.bias"].copy()
        b[4:10] += np.float32(bias)
        b[11:15] += np.float32(bias)
        sd["decoder.output_layer.bias"] = b
        _LOOP_MODELS[shape] = model_from_sd(cfg, sd)[0]
    return _LOOP_MODELS[shape]


def raw_decode(m, enc, steps, table, stop, sample=None, want_out=True):
    """The C entries called directly, so that the state buffer comes back: (ids, logits or probs, state bytes (rows, n)).
    An ArgumentTable goes to the argument entries, a BracketTable to the bracket ones."""
    dec = m.decoder
    arguments = isinstance(table, ArgumentTable)
    rows, V = enc.shape[0], dec.vocab_size
    w, keep, enc_c = dec.prepare(enc)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    ids = torch.empty((rows, steps), dtype=torch.int32, device=DEV)
    out = torch.full((rows, steps, V), float("nan"), dtype=torch.float32, device=DEV) if want_out else None
    L = _lib.lib()
    nbytes = L.i2l_decode_batched_scratch_bytes(rows, V, dec.hidden_dim, dec.lstm_layers)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    per_row = SB if arguments else C.STATE_BYTES
    assert (L.i2l_argument_state_bytes if arguments else L.i2l_bracket_state_bytes)(rows) == per_row * rows
    state = torch.full((per_row * rows,), 0xAB, dtype=torch.uint8, device=DEV)       # the call zeroes it
    cls = table.device(DEV)
    if sample is None:
        entry = "i2l_greedy_decode_arguments" if arguments else "i2l_greedy_decode_constrained"
        _lib.check(getattr(L, entry)(
            ctypes.byref(w), dec._ws.data_ptr(), rows, steps, tok0.data_ptr(), None, None, 1.0, _lib.SELECT_LOGITS, stop, END,
            ids.data_ptr(), _lib.ptr(out), None, None, scratch.data_ptr(), nbytes, 0, None, 0, cls.data_ptr(),
            state.data_ptr(), state.numel(), _lib.stream_ptr()), entry)
    else:
        temperature, top_k, top_p, seed = sample
        entry = "i2l_sample_decode_arguments" if arguments else "i2l_sample_decode_constrained"
        _lib.check(getattr(L, entry)(
            ctypes.byref(w), dec._ws.data_ptr(), rows, steps, tok0.data_ptr(), None, None, temperature, top_k, top_p, seed,
            stop, END, ids.data_ptr(), _lib.ptr(out), None, None, scratch.data_ptr(), nbytes, 0, cls.data_ptr(),
            state.data_ptr(), state.numel(), _lib.stream_ptr()), entry)
    torch.cuda.synchronize()
    del keep
    return ids.cpu().numpy(), None if out is None else out.cpu().numpy(), state.cpu().numpy().reshape(rows, per_row)


@pytest.mark.parametrize("stop", [_lib.STOP_NONE, _lib.STOP_STICKY], ids=["stop_none", "stop_sticky"])
@pytest.mark.parametrize("shape", [SMALL, SHIPPED], ids=["V37_H64_L2", "V500_H512_L2"])
def test_whole_loop_equals_replay_of_its_own_logits(shape, stop):
    rows, steps, _, _ = LOOP[shape]
    V = shape[0]
    m, table = loop_model(shape), loop_table(V)
    brackets = BracketTable(table.classes, END)
    enc = enc_for(shape, rows, seed=41)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    # the inputs: under the bracket constraint alone at least a quarter of the rows is not argument-complete
    nested, _, _ = raw_decode(m, enc, steps, brackets, _lib.STOP_NONE, want_out=False)
    assert all(brackets.well_formed(row.tolist(), END) for row in nested)
    incomplete = sum(not table.complete(row.tolist(), END) for row in nested)
    print(f"bracket-constrained: {incomplete} of {rows} rows lack an argument")
    assert 4 * incomplete >= rows, f"vacuous: only {incomplete} of {rows} bracket-constrained rows lack an argument"

    ids, logits, state = raw_decode(m, enc, steps, table, stop)
    overrode = set()
    for r in range(rows):
        row = ids[r].tolist()
        assert END in row and table.complete(row, END) and table.well_formed(row, END), (r, row)
        n = row.index(END)
        upto = steps if stop == _lib.STOP_NONE else n + 1
        want = table.replay(logits[r, :upto], END, steps)
        assert row[:upto] == [w["id"] for w in want], r
        overrode |= {w["rule"] for w in want if w["rule"]}
        if stop == _lib.STOP_STICKY:
            assert all(i == -1 for i in row[n + 1:]), (r, row)
        got = ArgumentState.from_bytes(state[r].tobytes())
        assert (got.depth, got.owed, got.pending, got.ended) == (0, 0, 0, 1), (r, got)
        assert state[r].tobytes() == want[n]["state"].to_bytes(), r
    assert C.RULE_ARG_EXPECTED in overrode, overrode
    # the public path gives the same ids
    again, _, _ = m.decoder.run_steps(enc, steps, tok0, stop=stop, end_id=END, constraint=table)
    assert np.array_equal(again.cpu().numpy(), ids)
    with pytest.raises(RuntimeError):
        m.decoder.run_steps(enc, steps, tok0, forced=torch.zeros((rows, steps), dtype=torch.int32, device=DEV), end_id=END,
                            constraint=table)
    # sampling: complete rows, the final state, the public path
    sample = (0.9, 5, 0.9, SEED)
    s_ids, s_probs, s_state = raw_decode(m, enc, steps, table, stop, sample=sample)
    for r in range(rows):
        row = s_ids[r].tolist()
        assert END in row and table.complete(row, END), (r, row)
        n = row.index(END)
        st = ArgumentState()
        for t in range(n + 1):
            mask = table.allowed(st, END, steps - t - 1).astype(bool)
            assert mask[row[t]] and (s_probs[r, t][~mask] == 0.0).all(), (r, t)
            table.advance(st, row[t], END)
        assert s_state[r].tobytes() == st.to_bytes() and (st.depth, st.owed, st.ended) == (0, 0, 1), r
    again, _ = m.decoder.sample_steps(enc, steps, tok0, *sample, stop=stop, end_id=END, constraint=table)
    assert np.array_equal(again.cpu().numpy(), s_ids)


@pytest.mark.parametrize("shape", [SMALL, SHIPPED], ids=["V37_H64_L2", "V500_H512_L2"])
def test_a_table_without_argument_bits_is_the_bracket_entry(shape):
    """Through the argument entries a table of plain class bytes gives the ids and logits of
    i2l_greedy_decode_constrained and the ids and probabilities of i2l_sample_decode_constrained, bit for bit."""
    rows, steps, _, _ = LOOP[shape]
    m = loop_model(shape)
    classes = loop_table(shape[0]).classes
    brackets, same = BracketTable(classes, END), ArgumentTable(classes, END)
    assert np.array_equal(same.table, brackets.classes)
    enc = enc_for(shape, rows, seed=41)
    for stop in (_lib.STOP_NONE, _lib.STOP_STICKY):
        for sample in (None, (0.9, 5, 0.9, SEED)):
            b_ids, b_out, b_state = raw_decode(m, enc, steps, brackets, stop, sample=sample)
            a_ids, a_out, a_state = raw_decode(m, enc, steps, same, stop, sample=sample)
            assert np.array_equal(a_ids, b_ids), (stop, sample)
            assert np.array_equal(bits(a_out), bits(b_out)), (stop, sample)
            for r in range(rows):
                a, b = ArgumentState.from_bytes(a_state[r].tobytes()), C.BracketState.from_bytes(b_state[r].tobytes())
                assert (a.stack, a.depth, a.ended, a.pending, a.loose, a.owed) == (b.stack, b.depth, b.ended, 0, 0, 0)
    assert any(not brackets.well_formed(r.tolist(), END) for r in
               m.decoder.run_steps(enc, steps, torch.full((rows,), START, dtype=torch.int32, device=DEV), end_id=END,
                                   flags=FLAG)[0].cpu().numpy())             # the constraint had something to do


# ------------------------------------------------------------------------------------------------ the surface
PT = os.path.join(GOLDEN, "predict_64x800.pt")
PNG = os.path.join(GOLDEN, "predict_page.png")
# the fixture checkpoint's frequent tokens: the six brackets its greedy output is made of, and -- where the bracket
# constraint alone pads its rows -- t13 as \frac and t20 as ^
NAMES = {"t41": "{", "t34": "}", "t27": "\\left(", "t28": "\\right)", "t6": "\\begin{array}", "t15": "\\end{array}",
         "t13": "\\frac", "t20": "^"}


@pytest.fixture(scope="module")
def argument_checkpoint(tmp_path_factory):
    """The fixture checkpoint with eight of its token STRINGS renamed (the ids and weights stay): its bracket-constrained
    output, `... \\begin{array} \\frac \\frac \\frac ... \\end{array}`, nests and gives no \\frac its groups."""
    ck = torch.load(PT, map_location="cpu", weights_only=False)
    ck["tokenizer_config"]["token_to_id"] = {NAMES.get(t, t): i for t, i in ck["tokenizer_config"]["token_to_id"].items()}
    path = str(tmp_path_factory.mktemp("arguments") / "arguments.pt")
    torch.save(ck, path)
    return path


def nests(pred, text):
    tok = pred.tokenizer
    return BracketTable.from_tokenizer(tok).well_formed(tok.encode(text) + [tok.end_token_id])


def complete(pred, text):
    tok = pred.tokenizer
    return ArgumentTable.from_tokenizer(tok).complete(tok.encode(text) + [tok.end_token_id])


def test_predictor_complete_arguments(argument_checkpoint):
    from img2latex_amd.training import Predictor
    dev = torch.device(DEV)
    off = Predictor.from_checkpoint(argument_checkpoint, device=dev)
    nested = Predictor.from_checkpoint(argument_checkpoint, device=dev, well_formed=True)
    on = Predictor.from_checkpoint(argument_checkpoint, device=dev, well_formed="arguments")
    plain = Predictor.from_checkpoint(PT, device=dev)
    rename = lambda s: " ".join(NAMES.get(t, t) for t in s.split())
    table = ArgumentTable.from_tokenizer(on.tokenizer)
    assert table.unsatisfiable == [] and table.unclosable == []
    assert {on.tokenizer.id_to_token[i] for i in np.flatnonzero(table.counts).tolist()} == {"\\frac", "^", "\\begin{array}"}
    T = 40
    # the default and the bracket constraint: today's outputs -- and the nested one lacks arguments, so the option has
    # something to do
    before = off.predict(PNG, max_length=T)
    assert before == rename(plain.predict(PNG, max_length=T))
    formed = nested.predict(PNG, max_length=T)
    assert formed == rename(plain.predict(PNG, max_length=T, well_formed=BracketTable.from_tokenizer(on.tokenizer)))
    assert formed == off.predict(PNG, max_length=T, well_formed=True) == on.predict(PNG, max_length=T, well_formed=True)
    assert nests(on, formed) and not complete(on, formed) and formed != before
    # the option, by constructor, by call and by table
    for text in (on.predict(PNG, max_length=T), off.predict(PNG, max_length=T, well_formed="arguments"),
                 nested.predict(PNG, max_length=T, well_formed=table)):
        assert complete(on, text) and nests(on, text) and text != formed, text
    assert on.predict(PNG, max_length=T, well_formed=False) == before
    for texts in (on.predict_batch([PNG, PNG], max_length=T), off.predict_batch([PNG, PNG], max_length=T, well_formed="arguments"),
                  on.predict_batch([PNG, PNG], max_length=T, temperature=0.9, top_k=5, top_p=0.9, seed=5)):
        assert len(texts) == 2 and all(complete(on, s) for s in texts), texts
    assert off.predict_batch([PNG, PNG], max_length=T) == [before] * 2
    x = torch.cat([on._prepare_image(PNG)] * 3)
    for rows in (on.predict_batch_ids(x, max_length=T), on.predict_batch_ids(x, max_length=T, top_k=5, seed=9)):
        assert all(r[0] == START and table.complete(r[1:] + [END]) for r in rows), rows
    assert off.predict_batch_ids(x, max_length=T) == plain.predict_batch_ids(x, max_length=T)
    assert nested.predict_batch_ids(x, max_length=T) == \
        plain.predict_batch_ids(x, max_length=T, well_formed=BracketTable.from_tokenizer(on.tokenizer))
    streamed = list(on.predict_strings_stream(iter([x, x]), max_length=T))
    assert len(streamed) == 2 and all(complete(on, s) for texts in streamed for s in texts), streamed
    assert streamed[0] == on.predict_batch([PNG] * 3, max_length=T)
    # the evaluate chain, one batch and the two-stream schedule
    tgt = torch.tensor([[START, 5, 6, END, 0, 0]] * 3, dtype=torch.int32, device=DEV)
    assert on.evaluate_batch(x, tgt, max_length=T, return_strings=True)["pred_text"] == streamed[0]
    chain = list(off.evaluate_stream(iter([(x, tgt), (x, tgt)]), max_length=T, return_strings=True, well_formed="arguments"))
    assert [r["pred_text"] for r in chain] == [streamed[0]] * 2
    # the model's surface; beam search has no argument form
    tok = on.tokenizer
    with torch.no_grad():
        seq = on.model.inference(x[:1], tok.start_token_id, tok.end_token_id, max_length=T, constraint=table)
        assert table.complete(seq[1:] + [END] if seq[0] == START else seq + [END])
        with pytest.raises(RuntimeError):
            on.model.inference(x[:1], tok.start_token_id, tok.end_token_id, max_length=T, beam_size=3, constraint=table)
        with pytest.raises(RuntimeError, match="greedy and sampling decode only"):
            on.model.beam_search_nbest(on.model.encoder(x[:1]), START, END, T, 3, constraint=table)
    for pred, kw in ((on, {}), (off, dict(well_formed="arguments")), (nested, dict(well_formed=table))):
        with pytest.raises(RuntimeError, match="greedy and sampling decode only"):
            pred.predict_nbest(PNG, beam_size=3, max_length=T, **kw)
    assert all(nests(on, s) for s, _, _ in on.predict_nbest(PNG, beam_size=3, max_length=T, well_formed=True))


def test_cli_complete_arguments(argument_checkpoint, capsys):
    from img2latex_amd import cli
    from img2latex_amd.training import Predictor
    assert cli.main(["predict", argument_checkpoint, PNG, "--max-length", "40", "--well-formed"]) == 0
    formed = capsys.readouterr().out
    assert cli.main(["predict", argument_checkpoint, PNG, "--max-length", "40", "--complete-arguments"]) == 0
    out = capsys.readouterr().out
    assert out.startswith("Generated LaTeX:\n") and out != formed
    pred = Predictor.from_checkpoint(argument_checkpoint, device=torch.device(DEV))
    assert not complete(pred, formed.split("\n")[1]) and complete(pred, out.split("\n")[1]), out
    assert out.split("\n")[1] == pred.predict(PNG, max_length=40, well_formed="arguments")
    for extra in (["--beam-size", "3"], ["--beam-size", "3", "--nbest", "2"], ["--well-formed", "--beam-size", "3", "--nbest", "1"]):
        with pytest.raises(SystemExit):
            cli.main(["predict", argument_checkpoint, PNG, "--complete-arguments"] + extra)
    capsys.readouterr()


def test_cli_evaluate_complete_arguments(argument_checkpoint, tmp_path, capsys):
    import json
    import shutil
    from img2latex_amd import cli
    from img2latex_amd.training import Predictor
    ck_dir = tmp_path / "outputs" / "tiny_exp" / "checkpoints"
    os.makedirs(ck_dir)
    shutil.copyfile(argument_checkpoint, ck_dir / "ck.pt")
    saved = {}
    for extra, out in ((["--well-formed"], "formed"), (["--complete-arguments"], "complete")):
        assert cli.main(["evaluate", str(ck_dir / "ck.pt"), os.path.join(GOLDEN, "dataset_tiny"), "--batch-size", "5",
                         "--device", "cuda", "--output-dir", str(tmp_path / out)] + extra) == 0
        saved[out] = json.loads((tmp_path / out / "tiny_exp" / "predictions" / "predictions.json").read_text())
    capsys.readouterr()
    pred = Predictor.from_checkpoint(argument_checkpoint, device=torch.device(DEV))
    assert len(saved["complete"]) == len(saved["formed"]) > 0
    assert all(complete(pred, p["prediction"]) and nests(pred, p["prediction"]) for p in saved["complete"]), saved["complete"]
    assert all(nests(pred, p["prediction"]) for p in saved["formed"])
    assert not any(complete(pred, p["prediction"]) for p in saved["formed"])


def test_grouped_pipeline_refuses_the_option(argument_checkpoint):
    from img2latex_amd.pipeline import GreedyPipeline
    from img2latex_amd.training import Predictor
    pred = Predictor.from_checkpoint(argument_checkpoint, device=torch.device(DEV))
    table = ArgumentTable.from_tokenizer(pred.tokenizer)
    for flags in (_lib.FLAG_DECODE_GROUP16, _lib.FLAG_DECODE_GROUP8):
        with pytest.raises(RuntimeError, match="constrained"):
            GreedyPipeline(pred.model, START, END, 40, decode_flags=flags, rows_per_workgroup=0, constraint=table)
    pipe = GreedyPipeline(pred.model, START, END, 40, decode_flags=FLAG, rows_per_workgroup=0, stop=_lib.STOP_STICKY,
                          constraint=table)
    try:
        pipe.submit(torch.cat([pred._prepare_image(PNG)] * 2))
        ids = pipe.collect().numpy()
    finally:
        pipe.close()
    assert all(table.complete(row.tolist()) for row in ids)
