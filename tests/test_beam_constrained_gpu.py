"""The well-formed N-best beam search on the device (i2l_beam_decode_nbest_constrained, Seq2SeqModel.beam_search_nbest(...,
constraint=), Predictor.predict_nbest(..., well_formed=), ``predict --nbest N --well-formed``) against its own structure,
its parent entry, the constrained greedy decode and the float64 restatement (constrained_beam_ref.py; the host test holds
the C++ rules to the same restatement with exact ties).

Structure is exact whatever the precision: every filled row has finished = 1 and nests, keys are score / norm[len + 1],
rows are distinct and key-ordered.  The anchor is the parent: under a neutral table the two searches differ only in what
step steps - 1 may emit, so weights whose END clock ends every search earlier must give i2l_beam_decode_nbest's bits.
Against float64 the rule is test_beam_nbest_gpu.py's: per image the rows' (tokens, finished) lists and the count equal
the float64 ones unless the float64 search has a candidate gap below 1e-4 or a gap below 1e-4, relative to max(1, |key|),
between neighbouring keys among its first N + 1 ranked entries; equal rows have score and key within 1e-4 relative to
max(1, |value|); at most one image per case may leave.  (On the CPU an fp32 run of the same restatement left 0 images in
every case below, with 0 to 3 images per case under a gap.)

The decoders: test_decoder_shapes.build's synthetic weights at V = 37, H = 64, L = 1 and at the shipped 500 / 512 / 2; two
variants of the same recipe come through model_from_sd, because build has no such option: "opens" adds 2.0 to the output
bias of the table's open columns, "early" turns the END clock into a step -- END out of reach (about -30) for two steps and certain (about +30) from the
third on -- so that all K beams end in the same step."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import constrained_beam_ref as R
import nbest_ref
from conftest import record
from helpers import END, GOLDEN, START
from img2latex_amd import _lib, synth
from img2latex_amd.training import constraint as C
from img2latex_amd.training.constraint import BracketTable
from test_decoder_shapes import build, enc_for, model_from_sd, shape_config, sid

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAP = 1e-4
SMALL, SHIPPED = (37, 64, 64, 1, False), (500, 512, 512, 2, True)
SENT_I, SENT_F = -7, 1.25          # what the output buffers hold before a call: no result is either
WEIGHT_SEED, TABLE_SEED, ENC_SEED = 7, 31, 13


def table_for(V, seed, kinds=3):
    """test_constrained_decode_gpu.py's: END = 2 neutral, PAD / START / UNK never; of the other columns about a fifth open
    and a fifth close one of ``kinds`` kinds (every kind at least once each way), a few are never, the rest neutral."""
    rng = np.random.default_rng(seed)
    classes = np.zeros(V, dtype=np.uint8)
    classes[[0, 1, 3]] = 255
    cols = 4 + rng.permutation(V - 4)
    for k in range(kinds):
        classes[cols[2 * k]] = C.open_class(k)
        classes[cols[2 * k + 1]] = C.close_class(k)
    for v in cols[2 * kinds:]:
        r = rng.random()
        if r < 0.4:
            k = int(rng.integers(kinds))
            classes[v] = C.open_class(k) if r < 0.2 else C.close_class(k)
        elif r < 0.45:
            classes[v] = 255
    return BracketTable(classes, END)


def variant_state_dict(shape, variant):
    """numpy state dict of the "opens" / "early" variants (module docstring)."""
    cfg = shape_config(shape)
    if variant == "early":
        return cfg, synth.make_state_dict(cfg, seed=WEIGHT_SEED, out_scale=12.0, end_clock=(0.2, 400.0, 183.0))
    assert variant == "opens"
    sd = synth.make_state_dict(cfg, seed=WEIGHT_SEED, out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
    cls = table_for(shape[0], TABLE_SEED).classes
    b = sd["decoder.output_layer.bias"].copy()
    b[(cls >= 1) & (cls <= C.KINDS)] += np.float32(2.0)
    sd["decoder.output_layer.bias"] = b
    return cfg, sd


_VARIANTS = {}


def model(shape, variant=None):
    """(Seq2SeqModel on the device, float64 decoder state dict on the device, cfg)"""
    if variant is None:
        return build(shape, seed=WEIGHT_SEED)
    if (shape, variant) not in _VARIANTS:
        cfg, sd = variant_state_dict(shape, variant)
        _VARIANTS[(shape, variant)] = model_from_sd(cfg, sd) + (cfg,)
    return _VARIANTS[(shape, variant)]


def penalty_table(steps, a):
    return None if a == 0 else [1.0] + [float(n) ** a for n in range(1, steps + 1)]


def raw(m, enc, steps, k, N, norm=None, table=None, start=START, end=END):
    """The C entry itself -- the parent entry when ``table`` is None -- on sentinel-filled outputs."""
    dec = m.decoder
    w, keep, enc_c = dec.prepare(enc)
    n = enc_c.shape[0]
    L = _lib.lib()
    query = L.i2l_beam_nbest_scratch_bytes if table is None else L.i2l_beam_nbest_constrained_scratch_bytes
    nbytes = query(n, k, N, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, steps)
    assert nbytes > 0
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)        # the call zeroes what it needs zeroed
    tab = None if norm is None else torch.tensor(norm, dtype=torch.float64, device=DEV)
    o = dict(seq=torch.full((n, N, steps + 1), SENT_I, dtype=torch.int32, device=DEV),
             len=torch.full((n, N), SENT_I, dtype=torch.int32, device=DEV),
             score=torch.full((n, N), SENT_F, dtype=torch.float64, device=DEV),
             key=torch.full((n, N), SENT_F, dtype=torch.float64, device=DEV),
             fin=torch.full((n, N), SENT_I, dtype=torch.int32, device=DEV),
             count=torch.full((n,), SENT_I, dtype=torch.int32, device=DEV))
    args = (ctypes.byref(w), dec._ws.data_ptr(), n, k, N, steps, start, end, _lib.ptr(tab), scratch.data_ptr(), nbytes,
            o["seq"].data_ptr(), o["len"].data_ptr(), o["score"].data_ptr(), o["key"].data_ptr(), o["fin"].data_ptr(),
            o["count"].data_ptr(), 0)
    if table is None:
        _lib.check(L.i2l_beam_decode_nbest(*args, _lib.stream_ptr()), "beam_decode_nbest")
    else:
        _lib.check(L.i2l_beam_decode_nbest_constrained(*args, table.device(DEV).data_ptr(), _lib.stream_ptr()),
                   "beam_decode_nbest_constrained")
    torch.cuda.synchronize()
    del keep, scratch, tab
    return {name: t.cpu().numpy() for name, t in o.items()}


def rows_of(o, j):
    c = int(o["count"][j])
    toks = [(o["seq"][j, r, :o["len"][j, r]].tolist(), bool(o["fin"][j, r])) for r in range(c)]
    return toks, o["score"][j, :c].tolist(), o["key"][j, :c].tolist()


def check_structure(o, table, V, N, steps, norm, end=END):
    """What holds of every constrained result whatever the weights."""
    n = o["count"].shape[0]
    for name in ("seq", "len", "fin", "count"):
        assert (o[name] != SENT_I).all(), name                     # every element written
    assert (o["score"] != SENT_F).all() and (o["key"] != SENT_F).all()
    for j in range(n):
        c = int(o["count"][j])
        assert 1 <= c <= N, (j, c)
        seen = set()
        for r in range(N):
            ln, row = int(o["len"][j, r]), o["seq"][j, r]
            sc, key, fin = float(o["score"][j, r]), float(o["key"][j, r]), int(o["fin"][j, r])
            if r >= c:                                             # absent rows
                assert ln == -1 and (row == -1).all() and sc == -math.inf and key == -math.inf and fin == 0, (j, r)
                continue
            assert fin == 1 and 0 <= ln <= steps - 1, (j, r, ln, fin)       # END is one of the steps
            assert (row[ln:] == -1).all(), (j, r, row)
            assert table.well_formed(row[:ln].tolist() + [end], end), (j, r, row)
            assert math.isfinite(sc) and sc <= 0.0, (j, r, sc)
            want = sc if norm is None else sc / norm[ln + 1]
            assert key == want, (j, r, key, want)                  # fp64 division is correctly rounded: exact
            ident = tuple(row[:ln].tolist())
            assert ident not in seen, (j, r, ident)                # all hypotheses of an image are distinct
            seen.add(ident)
        keys = o["key"][j, :c]
        assert (keys[1:] <= keys[:-1]).all(), (j, keys)            # every row comes from `completed`: one key order
    return o


# ------------------------------------------------------------------------------------------------ the cases
# (shape, variant, K, images, steps)
CASES = [
    (SMALL, None, 2, 17, 12),
    (SMALL, "opens", 5, 3, 24),
    (SMALL, None, 8, 3, 12),
    (SMALL, None, 5, 3, 1),
    (SMALL, "opens", 2, 1, 2),
    (SHIPPED, None, 5, 3, 24),
    (SHIPPED, "opens", 2, 17, 12),
    (SHIPPED, "opens", 8, 3, 12),
    (SHIPPED, None, 1, 17, 24),
]
case_id = lambda c: f"{sid(c[0], c[1])}-k{c[2]}-n{c[3]}-t{c[4]}"     # noqa: E731
_SEARCH = {}


def float64_searches(case):
    """The float64 constrained search of every image of the case, once for every ranking of it."""
    if case not in _SEARCH:
        shape, variant, k, n, steps = case
        _, sd64, cfg = model(shape, variant)
        table = table_for(shape[0], TABLE_SEED)
        enc = enc_for(shape, n, seed=ENC_SEED).double()
        with torch.no_grad():
            _SEARCH[case] = [R.search(R.oracle_rows(sd64, cfg, enc[j:j + 1]), table, START, END, steps, k) for j in range(n)]
    return _SEARCH[case]


def check_vs_float64(case, N, norm, tag):
    shape, variant, k, n, steps = case
    m, _, _ = model(shape, variant)
    table = table_for(shape[0], TABLE_SEED)
    enc = enc_for(shape, n, seed=ENC_SEED)
    with torch.no_grad():
        o = check_structure(raw(m, enc, steps, k, N, norm, table), table, shape[0], N, steps, norm)
    left, below, worst = 0, 0, 0.0
    for j, s in enumerate(float64_searches(case)):
        assert not s.ran_out, (tag, j)
        st = {}
        want = nbest_ref.rank(s, START, END, steps, N, norm, st)
        assert all(r.finished and table.well_formed(r.tokens + [END]) for r in want), (tag, j)
        near = st["gap"] < GAP or st["key_gap"] < GAP
        below += near
        got, scores, keys = rows_of(o, j)
        if got != [(r.tokens, r.finished) for r in want]:
            assert near, (tag, j, st, got, want)
            left += 1
            continue
        assert int(o["count"][j]) == len(want)
        for r, row in enumerate(want):
            for a, b in ((scores[r], row.score), (keys[r], row.key)):
                err = abs(a - b) / max(1.0, abs(b))
                worst = max(worst, err)
                assert err <= 1e-4, (tag, j, r, a, b)
    record(f"constrained nbest {tag}: scores and keys vs float64 [rel to max(1,|value|)]", worst)
    record(f"constrained nbest {tag}: images leaving the float64 rows at a near-tie", left)
    record(f"constrained nbest {tag}: images with a float64 candidate or key gap below 1e-4", below)
    assert left <= 1, (tag, left)
    return o


@pytest.mark.parametrize("ranking", ["one", "K_0.7", "2K_1.0"])
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_rows_vs_float64(case, ranking):
    k, steps = case[2], case[4]
    N, a = {"one": (1, 0.0), "K_0.7": (k, 0.7), "2K_1.0": (2 * k, 1.0)}[ranking]
    o = check_vs_float64(case, N, penalty_table(steps, a), f"{case_id(case)} N={N} penalty={a}")
    if steps == 1:                                                 # the only candidate of step 0 is END
        assert (o["count"] == 1).all() and (o["len"][:, 0] == 0).all() and (o["score"][:, 0] == 0.0).all()


@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=[case_id(CASES[1]), case_id(CASES[6])])
def test_the_constraint_has_work_to_do(case):
    """The same weights without the table return ill-formed rows; with it the rows differ and nest."""
    shape, variant, k, n, steps = case
    m, _, _ = model(shape, variant)
    table = table_for(shape[0], TABLE_SEED)
    enc = enc_for(shape, n, seed=ENC_SEED)
    with torch.no_grad():
        free = raw(m, enc, steps, k, k)
        held = check_structure(raw(m, enc, steps, k, k, None, table), table, shape[0], k, steps, None)
    ill = total = 0
    for j in range(n):
        for toks, fin in rows_of(free, j)[0]:
            total += 1
            ill += not (fin and table.well_formed(toks + [END]))
    print(f"unconstrained: {ill} of {total} rows ill-formed")
    assert ill > 0, "vacuous: every unconstrained row is well formed"
    assert any(rows_of(free, j)[0] != rows_of(held, j)[0] for j in range(n))


# ------------------------------------------------------------------------------------------------ the anchor
@pytest.mark.parametrize("shape,k,n", [(SMALL, 5, 17), (SHIPPED, 2, 3), (SHIPPED, 8, 3)],
                         ids=lambda v: sid(v) if isinstance(v, tuple) else str(v))
def test_a_neutral_table_on_early_ending_weights_is_the_parent_entry(shape, k, n):
    steps = 12
    m, sd64, cfg = model(shape, "early")
    neutral = BracketTable(np.zeros(shape[0], dtype=np.uint8), END)
    enc = enc_for(shape, n, seed=ENC_SEED)
    # the condition on the inputs: in float64 every image's search breaks before step steps - 1, the only step at which
    # a neutral table forbids anything
    with torch.no_grad():
        for j in range(n):
            trace = []
            s = R.search(R.oracle_rows(sd64, cfg, enc[j:j + 1].double()), None, START, END, steps, k, trace=trace)
            assert not s.ran_out and len(trace) <= steps - 1, (j, len(trace))
    for N, norm in ((1, None), (2 * k, penalty_table(steps, 0.7))):
        with torch.no_grad():
            parent = raw(m, enc, steps, k, N, norm)
            o = check_structure(raw(m, enc, steps, k, N, norm, neutral), neutral, shape[0], N, steps, norm)
        for name in ("seq", "len", "fin", "count"):
            assert np.array_equal(o[name], parent[name]), name
        for name in ("score", "key"):
            assert np.array_equal(o[name].view(np.int64), parent[name].view(np.int64)), name       # bit-identical


# ------------------------------------------------------------------------------------------------ k = 1
@pytest.mark.parametrize("case", [CASES[8], (SMALL, "opens", 1, 17, 24)], ids=["shipped", "small_opens"])
def test_one_beam_is_the_constrained_greedy_decode(case):
    shape, variant, k, n, steps = case
    m, sd64, cfg = model(shape, variant)
    table = table_for(shape[0], TABLE_SEED)
    enc = enc_for(shape, n, seed=ENC_SEED)
    tok0 = torch.full((n,), START, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        o = check_structure(raw(m, enc, steps, 1, 1, None, table), table, shape[0], 1, steps, None)
        ids, _, _ = m.decoder.run_steps(enc, steps, tok0, stop=_lib.STOP_NONE, end_id=END, constraint=table)
    ids = ids.cpu().numpy()
    near = 0
    for j in range(n):
        greedy = ids[j].tolist()
        greedy = greedy[:greedy.index(END)]
        if rows_of(o, j)[0] != [(greedy, True)]:
            with torch.no_grad():
                gap = R.allowed_gap(R.oracle_rows(sd64, cfg, enc[j:j + 1].double()), table, START, END, steps)
            assert gap < GAP, (j, gap, rows_of(o, j)[0], greedy)
            near += 1
    record(f"constrained nbest {case_id(case)}: rows leaving the constrained greedy ids at a float64 near-tie", near)
    assert near <= 1


# ------------------------------------------------------------------------------------------------ edges
def test_start_equals_end():
    m, _, _ = model(SHIPPED)
    table = table_for(500, TABLE_SEED)
    enc = enc_for(SHIPPED, 3, seed=ENC_SEED)
    for norm in (None, [2.0] + [1.0] * 5):
        with torch.no_grad():
            o = raw(m, enc, 5, 3, 4, norm, table, END, END)
        assert (o["count"] == 1).all() and (o["len"][:, 0] == 0).all() and (o["fin"][:, 0] == 1).all()
        assert (o["score"][:, 0] == 0.0).all() and (o["key"][:, 0] == 0.0).all() and (o["seq"] == -1).all()
        assert (o["len"][:, 1:] == -1).all() and (o["score"][:, 1:] == -math.inf).all()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_beam_search_nbest_with_a_constraint_is_the_raw_entry():
    m, _, _ = model(SHIPPED, "opens")
    table = table_for(500, TABLE_SEED)
    enc = enc_for(SHIPPED, 3, seed=ENC_SEED)
    steps, k, N = 12, 5, 7
    with torch.no_grad():
        o = raw(m, enc, steps, k, N, penalty_table(steps, 0.7), table)
        hyps = m.beam_search_nbest(enc, START, END, steps, k, nbest=N, length_penalty=0.7, constraint=table)
        plain = m.beam_search_nbest(enc, START, END, steps, k, nbest=N, length_penalty=0.7)
        parent = raw(m, enc, steps, k, N, penalty_table(steps, 0.7))
    for j in range(3):
        got, scores, keys = rows_of(o, j)
        assert [(h.tokens, h.finished) for h in hyps[j]] == got
        assert [h.score for h in hyps[j]] == scores and [h.key for h in hyps[j]] == keys
        got, scores, keys = rows_of(parent, j)                      # constraint=None is the call it was
        assert [(h.tokens, h.finished) for h in plain[j]] == got and [h.score for h in plain[j]] == scores
    with pytest.raises(RuntimeError):
        m.beam_search_nbest(enc, START, END, steps, k, constraint=BracketTable(np.zeros(499, dtype=np.uint8), END))
    with pytest.raises(ValueError):
        m.beam_search_nbest(enc, START, END, steps, k, constraint=BracketTable([0, 0, 1] + [0] * 497))   # END not neutral
    with pytest.raises(RuntimeError):
        m.beam_search_nbest(enc, START, END, steps, 9, nbest=2, constraint=table)


PT = os.path.join(GOLDEN, "predict_64x800.pt")
PNG = os.path.join(GOLDEN, "predict_page.png")
BRACKETS = {"t41": "{", "t34": "}", "t27": "\\left(", "t28": "\\right)", "t6": "\\begin{array}", "t15": "\\end{array}",
            "t13": "\\leftarrow"}


@pytest.fixture(scope="module")
def bracket_checkpoint(tmp_path_factory):
    """test_constrained_decode_gpu.py's: the fixture checkpoint with seven of its token STRINGS renamed to brackets (the
    ids and weights stay), so that its output reads `\\left( { { { } ...` and does not nest."""
    ck = torch.load(PT, map_location="cpu", weights_only=False)
    ck["tokenizer_config"]["token_to_id"] = {BRACKETS.get(t, t): i for t, i in ck["tokenizer_config"]["token_to_id"].items()}
    path = str(tmp_path_factory.mktemp("constrained_beam") / "brackets.pt")
    torch.save(ck, path)
    return path


def passes(pred, text):
    tok = pred.tokenizer
    return BracketTable.from_tokenizer(tok).well_formed(tok.encode(text) + [tok.end_token_id])


def test_predictor_nbest_well_formed(bracket_checkpoint):
    from img2latex_amd.training import Predictor
    dev = torch.device(DEV)
    off = Predictor.from_checkpoint(bracket_checkpoint, device=dev)
    on = Predictor.from_checkpoint(bracket_checkpoint, device=dev, well_formed=True)
    plain = Predictor.from_checkpoint(PT, device=dev)
    rename = lambda s: " ".join(BRACKETS.get(t, t) for t in s.split())      # noqa: E731
    k, N, T = 3, 4, 40
    # without the option: today's rows, and not all of them nest -- so the option has something to do
    before = off.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T)
    assert before == [(rename(s), sc, key) for s, sc, key in plain.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T)]
    assert not all(passes(off, s) for s, _, _ in before)
    rows = off.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T, well_formed=True)
    assert 1 <= len(rows) <= N and all(passes(off, s) and key == sc <= 0.0 for s, sc, key in rows), rows
    assert [key for _, _, key in rows] == sorted((key for _, _, key in rows), reverse=True)
    assert on.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T) == rows                 # by constructor
    assert on.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T, well_formed=False) == before
    assert off.predict_batch_nbest([PNG, PNG], beam_size=k, nbest=N, max_length=T, well_formed=True) == [rows, rows]
    one = off.predict_nbest(PNG, beam_size=k, nbest=1, max_length=T, well_formed=True)       # the single best
    assert one == rows[:1]
    normed = on.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T, length_penalty=1.0)
    assert all(passes(on, s) and key == sc / (len(on.tokenizer.encode(s)) + 1) for s, sc, key in normed), normed


def test_cli_prints_well_formed_lines(bracket_checkpoint, capsys):
    from img2latex_amd import cli
    from img2latex_amd.training import Predictor
    argv = ["predict", bracket_checkpoint, PNG, "--max-length", "40", "--beam-size", "3", "--nbest", "4"]
    assert cli.main(argv) == 0
    before = capsys.readouterr().out
    assert cli.main(argv + ["--well-formed"]) == 0
    lines = capsys.readouterr().out.split("\n")
    pred = Predictor.from_checkpoint(bracket_checkpoint, device=torch.device(DEV))
    want = pred.predict_nbest(PNG, beam_size=3, nbest=4, max_length=40, well_formed=True)
    assert lines[-1] == "" and lines[:-1] == [f"{key!r}\t{latex}" for latex, _, key in want]
    assert all(passes(pred, ln.split("\t", 1)[1]) for ln in lines[:-1]), lines
    assert not all(passes(pred, ln.split("\t", 1)[1]) for ln in before.split("\n")[:-1])
