"""The argument rules on the host (no GPU): csrc/argument_rules.inc.h as a stand-alone program
(csrc/argument_rules_host_main.cpp), a process of its own under the host sanitizers.

* Every sequence the program enumerates for a small table equals, as a set, what an independent recursive-descent
  recogniser of the same little language accepts -- soundness and completeness over every token sequence shorter than
  ``steps`` -- and the Python restatement ``ArgumentTable.enumerate`` gives the same list.
* Replays against ``ArgumentTable.replay``: per step the allowed mask, the pick and the 32 state bytes.
* A table without argument bits is the bracket constraint, mask for mask.
* ``from_tokenizer``, the state bytes, and the refusals of the three C entries, which answer before the first HIP call."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import png_cases
from img2latex_amd import _lib
from img2latex_amd.training import constraint as C
from img2latex_amd.training.constraint import ArgumentState, ArgumentTable, BracketTable, argument_byte
from img2latex_amd.training.predictor import TokenTable

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe, sanitized = png_cases.build_host_program(str(tmp_path_factory.mktemp("argument_rules")), "argument_rules_host_main")
    print("argument_rules_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of argument_rules_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])


# ------------------------------------------------------------------------------ 1, 2: the little language, exhaustively
END, X, LB, RB, FRAC, HAT, LEFT, RIGHT, BEGIN, ENDENV, BINOM = range(11)
SMALL = [0, 0, argument_byte(1), argument_byte(5), argument_byte(0, 2), argument_byte(0, 1, True), argument_byte(2),
         argument_byte(6), argument_byte(3, 1), argument_byte(7), argument_byte(0, 2, True)]


class _More(Exception):
    pass


class _Dead(Exception):
    pass


def recognise(seq):
    """Recursive descent over
         item   := x | { item* } | \\left( item* \\right) | \\begin{array} strict item* \\end{array}
                 | \\frac strict strict | ^ loose | \\binom loose loose
         strict := { item* }          loose := x | { item* }
    -> "ok" (seq is item*), "more" (a proper prefix of one), "dead" (no extension is one).  It knows nothing of stacks,
    budgets or pending counts."""
    pos = 0

    def take():
        nonlocal pos
        if pos >= len(seq):
            raise _More
        pos += 1
        return seq[pos - 1]

    def group(closer):
        nonlocal pos
        while True:
            if pos < len(seq) and seq[pos] == closer:
                pos += 1
                return
            item()

    def strict():
        if take() != LB:
            raise _Dead
        group(RB)

    def loose():
        tok = take()
        if tok == LB:
            group(RB)
        elif tok != X:
            raise _Dead

    def item():
        tok = take()
        if tok == X:
            return
        if tok == LB:
            group(RB)
        elif tok == LEFT:
            group(RIGHT)
        elif tok == BEGIN:
            strict()
            group(ENDENV)
        elif tok == FRAC:
            strict()
            strict()
        elif tok == HAT:
            loose()
        elif tok == BINOM:
            loose()
            loose()
        else:
            raise _Dead                       # a closer nothing opened, or of another kind

    try:
        while pos < len(seq):
            item()
        return "ok"
    except _More:
        return "more"
    except _Dead:
        return "dead"


def accepted(longest):
    """Every token sequence of at most ``longest`` tokens the recogniser accepts; a dead prefix has no live extension, so
    the walk over ALL sequences skips below it."""
    out, frontier = set(), [()]
    while frontier:
        seq = frontier.pop()
        verdict = recognise(seq)
        if verdict == "dead":
            continue
        if verdict == "ok":
            out.add(seq)
        if len(seq) < longest:
            frontier.extend(seq + (v,) for v in range(1, 11))
    return out


def test_the_recogniser_itself():
    assert recognise((FRAC, LB, X, RB, LB, RB)) == "ok" and recognise((FRAC, LB, X, RB)) == "more"
    assert recognise((FRAC, X)) == "dead" and recognise((HAT, X)) == "ok" and recognise((HAT, HAT)) == "dead"
    assert recognise((BEGIN, LB, RB, X, ENDENV)) == "ok" and recognise((BEGIN, X)) == "dead"
    assert recognise((LEFT, RB)) == "dead" and recognise((LEFT, X, RIGHT)) == "ok" and recognise((RB,)) == "dead"
    assert recognise((BINOM, X, LB, X, RB)) == "ok" and recognise((BINOM, X, FRAC)) == "dead" and recognise(()) == "ok"


def enumerate_on_host(exe, tmp, table, steps, end=END):
    src, dst = os.path.join(tmp, f"table{steps}.bin"), os.path.join(tmp, f"enum{steps}.bin")
    with open(src, "wb") as f:
        f.write(b"ARGE" + struct.pack("<3i", len(table), steps, end) + bytes(bytearray(int(b) for b in table)))
    run(exe, "--enumerate", src, dst)
    data, pos, seqs = open(dst, "rb").read(), 0, []
    while True:
        (n,) = struct.unpack_from("<i", data, pos)
        pos += 4
        if n < 0:
            break
        seqs.append(struct.unpack_from(f"<{n}i", data, pos))
        pos += 4 * n
    visited, empty, unfinished = struct.unpack_from("<3q", data, pos)
    assert pos + 24 == len(data)
    return seqs, visited, empty, unfinished


@pytest.mark.parametrize("steps,count", [(6, 188), (7, 671)])
def test_sound_and_complete_against_the_recogniser(host_program, tmp_path, steps, count):
    seqs, visited, empty, unfinished = enumerate_on_host(host_program, str(tmp_path), SMALL, steps)
    assert all(s[-1] == END and END not in s[:-1] for s in seqs)
    got = {s[:-1] for s in seqs}
    assert len(got) == len(seqs)
    want = accepted(steps - 1)
    print(f"steps {steps}: the rules allow {len(got)} formulas, the recogniser accepts {len(want)}; {visited} states visited")
    assert got - want == set(), sorted(got - want)[:5]                      # sound: nothing the rules allow is malformed
    assert want - got == set(), sorted(want - got)[:5]                      # complete: nothing well formed is refused
    assert len(got) == count
    assert empty == 0 and unfinished == 0 and visited > 0                   # the allowed set is never empty along the way
    table = ArgumentTable(SMALL, END)
    assert all(table.complete(s) for s in seqs)
    # 2: the restatement walks the same tree
    assert table.enumerate(steps) == [tuple(s) for s in seqs]


def test_complete_is_the_recognisers_language_on_short_sequences():
    table = ArgumentTable(SMALL, END)
    want = accepted(4)
    frontier = [()]
    while frontier:
        seq = frontier.pop()
        assert table.complete(seq + (END,)) == (seq in want), seq
        assert not table.complete(seq)                                      # no END
        if len(seq) < 4:
            frontier.extend(seq + (v,) for v in range(1, 11))


# ------------------------------------------------------------------------------------------------------- 3: the replays
def make_table(rng, V, kinds, demanding=0.3, never=0.08):
    """(table bytes, end_id): {, } and a plain token always; every kind with an open and a closer where V has room;
    demanding columns of every count, strict and loose, opening and not."""
    cols = rng.permutation(V)
    end = int(cols[0])
    table = np.zeros(V, dtype=np.uint8)
    table[cols[1]], table[cols[2]] = C.open_class(0), C.close_class(0)        # cols[3] stays a plain token
    kinds = max(1, min(kinds, (V - 2) // 2))
    for k in range(1, kinds):
        table[cols[2 + 2 * k]], table[cols[3 + 2 * k]] = C.open_class(k), C.close_class(k)
    for v in cols[2 + 2 * kinds:] if kinds > 1 else cols[4:]:
        r = rng.random()
        if r < never:
            table[v] = rng.choice([255, 9, 0x80, 0x40, 0x15, 0x4F])          # invalid bytes of every sort
        elif r < never + demanding:
            count, loose = int(rng.integers(1, 4)), bool(rng.random() < 0.5)
            opening = rng.random() < 0.4
            table[v] = argument_byte(C.open_class(int(rng.integers(kinds))) if opening else 0, count, loose)
        elif r < never + demanding + 0.25:
            k = int(rng.integers(kinds))
            table[v] = C.open_class(k) if rng.random() < 0.5 else C.close_class(k)
    return table, end


def make_cases():
    rng = np.random.default_rng(20250321)
    out = []
    for V in (5, 37, 200):
        for steps in (1, 2, 3, 40, 80):
            for kinds in (1, 2, 3, 4):
                for biased in (False, True):
                    table, end = make_table(rng, V, kinds)
                    x = rng.standard_normal((steps, V)).astype(np.float32)
                    if biased:                  # toward opens and demanding columns: depth 32 is reached at steps 80
                        valid = C._valid_bytes(table.astype(np.int64))
                        lo, n = table & 15, (table >> 4) & 3
                        x[:, valid & (((lo >= 1) & (lo <= 4)) | (n > 0))] += 6.0
                    out.append(dict(V=V, steps=steps, end=end, table=table, logits=x, broken=False, biased=biased))
    # V = 5 by hand: END, x, {, }, and one demanding column of each sort in turn
    for byte in (argument_byte(0, 2), argument_byte(0, 3, True), argument_byte(1, 1), argument_byte(1, 2, True)):
        for steps in (1, 2, 3, 40, 80):
            x = rng.standard_normal((steps, 5)).astype(np.float32)
            x[:, 4] += 3.0
            out.append(dict(V=5, steps=steps, end=0, table=np.array([0, 0, 1, 5, byte], dtype=np.uint8), logits=x,
                            broken=False, biased=True))
    # a deliberately broken table: kind 1 opens and nothing closes it -> at some step no column is allowed
    table = np.zeros(6, dtype=np.uint8)
    table[1] = C.open_class(1)
    x = np.zeros((6, 6), dtype=np.float32)
    x[:, 1] = 5.0
    out.append(dict(V=6, steps=6, end=0, table=table, logits=x, broken=True, biased=True))
    return out


def write_cases(path, cs):
    with open(path, "wb") as f:
        f.write(b"ARGS" + struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<3i", c["V"], c["steps"], c["end"]))
            f.write(c["table"].tobytes())
            f.write(np.ascontiguousarray(c["logits"], dtype="<f4").tobytes())


def read_results(path, cs):
    data, pos, out = open(path, "rb").read(), 0, []
    for c in cs:
        rows = []
        for _ in range(c["steps"]):
            mask = np.frombuffer(data, dtype=np.uint8, count=c["V"], offset=pos)
            pos += c["V"]
            (pick,) = struct.unpack_from("<i", data, pos)
            pos += 4
            rows.append((mask, pick, data[pos:pos + 32]))
            pos += 32
        out.append(rows)
    assert pos == len(data)
    return out


def test_the_rules_as_a_sanitized_host_program(host_program, tmp_path):
    cs = make_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write_cases(src, cs)
    run(host_program, src, dst)

    fired, deepest, sorts, owed_deepest = set(), 0, set(), 0
    for i, (c, rows) in enumerate(zip(cs, read_results(dst, cs))):
        table = ArgumentTable(c["table"])
        sorts |= {(int(n), bool(l), bool(1 <= k <= 4)) for n, l, k in zip(table.counts, table.loose, table.classes) if n}
        want = table.replay(c["logits"], end_id=c["end"])
        assert len(want) == len(rows) == c["steps"]
        for t, (w, (mask, pick, state)) in enumerate(zip(want, rows)):
            assert np.array_equal(mask, w["allowed"]), (i, t)
            assert pick == w["id"], (i, t)
            assert state == w["state"].to_bytes(), (i, t, ArgumentState.from_bytes(state), w["state"])
            if w["rule"]:
                fired.add(w["rule"])
            deepest = max(deepest, w["state"].depth)
            if w["state"].pending_here():
                owed_deepest = max(owed_deepest, w["state"].depth)
        ids = [w["id"] for w in want]
        if c["broken"]:
            empty = [t for t, w in enumerate(want) if not w["allowed"].any()]
            assert empty and all(ids[t] == c["end"] for t in empty), (i, ids)
            assert not table.complete(ids, c["end"])
            continue
        assert all(w["allowed"].any() for w in want), i                     # the allowed set is never empty
        assert c["end"] in ids, (i, ids)
        n = ids.index(c["end"])
        s = want[n]["state"]
        assert (s.depth, s.owed, s.pending, s.ended) == (0, 0, 0, 1), (i, s)
        assert table.complete(ids, c["end"]) and table.well_formed(ids, c["end"]), (i, ids)
        if c["steps"] == 1:
            assert ids == [c["end"]], i
    assert deepest == C.MAX_DEPTH and owed_deepest == C.MAX_DEPTH - 1, (deepest, owed_deepest)
    assert sorts == {(n, l, o) for n in (1, 2, 3) for l in (False, True) for o in (False, True)}
    assert fired == set(range(1, 10)), fired                                # every rule overrode the free arg max somewhere


# ------------------------------------------------------------------------------- 4: without argument bits, the brackets
def test_a_table_without_argument_bits_is_the_bracket_constraint():
    rng = np.random.default_rng(7)
    deepest = 0
    for V in (5, 37, 200):
        for steps in (1, 3, 40, 80):
            for biased in (False, True):
                classes = rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 9, 15], size=V).astype(np.uint8)
                end = int(rng.integers(V))
                classes[end] = 0
                x = rng.standard_normal((steps, V)).astype(np.float32)
                if biased:
                    x[:, (classes >= 1) & (classes <= 4)] += 6.0
                a = ArgumentTable(classes).replay(x, end_id=end)
                b = BracketTable(classes).replay(x, end_id=end)
                for t, (wa, wb) in enumerate(zip(a, b)):
                    assert np.array_equal(wa["allowed"], wb["allowed"]) and wa["id"] == wb["id"], (V, steps, t)
                    assert wa["rule"] == wb["rule"] and wa["free"] == wb["free"]
                    sa, sb = wa["state"], wb["state"]
                    assert (sa.stack, sa.depth, sa.ended) == (sb.stack, sb.depth, sb.ended)
                    assert (sa.pending, sa.loose, sa.owed) == (0, 0, 0)
                    deepest = max(deepest, sa.depth)
    assert deepest == C.MAX_DEPTH


# ---------------------------------------------------------------------------------------------- 5: building the table
TOKENS = ["<PAD>", "<START>", "<END>", "<UNK>", "{", "}", "\\left(", "\\leftarrow", "\\right)", "\\begin{array}",
          "\\end{array}", "x", "3", "[", "]", "\\frac", "^", "_", "\\sqrt", "\\mathrm", "\\begin{matrix}", "\\end{matrix}"]


def test_from_tokenizer_gives_the_bytes():
    tok = TokenTable({t: i for i, t in enumerate(TOKENS)})
    table = ArgumentTable.from_tokenizer(tok)
    want = {"<PAD>": 255, "<START>": 255, "<UNK>": 255, "<END>": 0, "{": 1, "}": 5, "\\left(": 2, "\\leftarrow": 0,
            "\\right)": 6, "\\begin{array}": 0x13, "\\end{array}": 7, "x": 0, "3": 0, "[": 0, "]": 0, "\\frac": 0x20,
            "^": 0x50, "_": 0x50, "\\sqrt": 0x50, "\\mathrm": 0x50, "\\begin{matrix}": 3, "\\end{matrix}": 7}
    assert {t: int(table.table[i]) for i, t in enumerate(TOKENS)} == want
    assert table.end_id == tok.end_token_id and table.unclosable == [] and table.unsatisfiable == []
    assert table.vocab == len(TOKENS) and C.as_table("arguments", tok) is C.as_table("arguments", tok)
    assert isinstance(C.as_table("arguments", tok), ArgumentTable) and isinstance(C.as_table(True, tok), BracketTable)
    assert np.array_equal(table.classes, BracketTable.from_tokenizer(tok).classes)
    enc = lambda s: tok.encode(s) + [tok.end_token_id]
    assert table.complete(enc("\\frac { x } { \\left( x \\right) }"))
    assert table.complete(enc("\\sqrt [ 3 ] { x }")) and table.complete(enc("\\sqrt { x }")) and table.complete(enc("x ^ 3 _ { x }"))
    assert table.complete(enc("\\begin{array} { x } x \\end{array}"))
    assert table.complete(enc("x ^ 3 ^ 3"))                                 # double scripts are not the rules' business
    for bad in ("\\frac { x }", "\\frac x { x }", "x ^", "x ^ }", "{ x ^ }", "\\sqrt \\right)", "\\begin{array} x \\end{array}",
                "x ^ \\frac { x } { x }", "^ ^ x", "{ x", "x <UNK>", "\\mathrm \\left( x \\right)"):
        assert not table.complete(enc(bad)), bad
        assert table.well_formed(enc(bad)) == BracketTable.from_tokenizer(tok).well_formed(enc(bad))
    assert not table.complete(tok.encode("x ^ 3"))                          # no END
    # after \sqrt the plain token [ is allowed, after \frac only {
    ids = {t: i for i, t in enumerate(TOKENS)}
    st = ArgumentState()
    table.advance(st, ids["\\sqrt"], table.end_id)
    assert set(np.flatnonzero(table.allowed(st, table.end_id, 10))) == {ids[t] for t in ("{", "x", "3", "[", "]", "\\leftarrow")}
    st = ArgumentState()
    table.advance(st, ids["\\frac"], table.end_id)
    assert np.flatnonzero(table.allowed(st, table.end_id, 10)).tolist() == [ids["{"]]
    # a caller's mapping replaces the default
    own = ArgumentTable.from_tokenizer(tok, {"x": (3, True)})
    assert own.table[ids["x"]] == 0x70 and own.table[ids["\\frac"]] == 0 and own.table[ids["\\begin{array}"]] == 3


def test_a_demand_that_cannot_be_met_is_dropped_and_listed():
    tokens = [t for t in TOKENS if t not in ("{", "}")]
    tok = TokenTable({t: i for i, t in enumerate(tokens)})
    table = ArgumentTable.from_tokenizer(tok)
    assert sorted(table.unsatisfiable) == sorted(["\\frac", "\\begin{array}"])
    ids = {t: i for i, t in enumerate(tokens)}
    assert table.table[ids["\\frac"]] == 0 and table.table[ids["\\begin{array}"]] == 3 and table.table[ids["^"]] == 0x50
    # loose demands without any plain token
    table = ArgumentTable.from_brackets(BracketTable([0, 1, 5, 0, 0], end_id=0), {3: (1, True), 4: (2, True)})
    assert table.table.tolist() == [0, 1, 5, 0, 0] and table.unsatisfiable == ["3", "4"]
    table = ArgumentTable.from_brackets(BracketTable([0, 1, 5, 0, 0], end_id=0), {3: (1, True), 2: (1, False)})
    assert table.table.tolist() == [0, 1, 5, 0x50, 0] and table.unsatisfiable == ["2"]      # a closer demands nothing
    with pytest.raises(ValueError):
        ArgumentTable([0, 0, 0x20])                                         # strict demand, no braces
    with pytest.raises(ValueError):
        ArgumentTable([0, 0x50, 1, 5], end_id=0)                            # loose demand, no plain token
    with pytest.raises(ValueError):
        ArgumentTable([0, 0x50, 0], end_id=1)                               # END's byte must be 0
    assert ArgumentTable([0, 9, 0x80, 0x40, 0x15, 0x4F, 255, 0x38, 8, 0x74, 0, 1, 5]).table.tolist() == \
        [0, 255, 255, 255, 255, 255, 255, 255, 8, 0x74, 0, 1, 5]


def test_state_bytes_round_trip():
    s = ArgumentState(stack=0x2D, pending=0x91, loose=0x5, depth=3, owed=7, ended=0)
    assert len(s.to_bytes()) == C.ARGUMENT_STATE_BYTES == 32 and ArgumentState.from_bytes(s.to_bytes()) == s
    assert ArgumentState().to_bytes() == bytes(32)
    assert s.to_bytes() == struct.pack("<QQIiii", 0x2D, 0x91, 0x5, 3, 7, 0)
    assert s.top() == 2 and s.pending_here() == 2 and not s.loose_here()


# ---------------------------------------------------------------------------------------------- the C entries' refusals
def _weights(V=500, E=512, H=512, L=2):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _greedy(w, rows=4, steps=3, select=_lib.SELECT_LOGITS, end_id=2, scratch=FAKE, scratch_bytes=1 << 40, cls=FAKE,
            state=FAKE, state_bytes=1 << 20):
    return _lib.lib().i2l_greedy_decode_arguments(ctypes.byref(w), FAKE, rows, steps, FAKE, None, None, 1.0, select,
                                                  _lib.STOP_NONE, end_id, FAKE, None, None, None, scratch, scratch_bytes,
                                                  0, None, 0, cls, state, state_bytes, None)


def _sample(w, rows=4, steps=3, temperature=1.0, top_k=5, top_p=0.9, end_id=2, scratch=FAKE, scratch_bytes=1 << 40,
            cls=FAKE, state=FAKE, state_bytes=1 << 20):
    return _lib.lib().i2l_sample_decode_arguments(ctypes.byref(w), FAKE, rows, steps, FAKE, None, None, temperature,
                                                  top_k, top_p, 7, _lib.STOP_NONE, end_id, FAKE, None, None, None,
                                                  scratch, scratch_bytes, 0, cls, state, state_bytes, None)


def _pick(logits=FAKE, ld=500, rows=4, vocab=500, temperature=1.0, select=_lib.SELECT_LOGITS, top_k=0, top_p=0.0, step=0,
          steps=3, cls=FAKE, end_id=2, state=FAKE, ids=FAKE):
    return _lib.lib().i2l_arguments_pick_logits(logits, ld, rows, vocab, temperature, select, top_k, top_p, 7, step,
                                                steps, cls, end_id, state, ids, None, None, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_greedy_decode_arguments", "i2l_sample_decode_arguments", "i2l_arguments_pick_logits"):
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"^size_t\s+i2l_argument_state_bytes\s*\(", header, flags=re.M)
    L = _lib.lib()
    for new, old in (("i2l_greedy_decode_arguments", "i2l_greedy_decode_constrained"),
                     ("i2l_sample_decode_arguments", "i2l_sample_decode_constrained"),
                     ("i2l_arguments_pick_logits", "i2l_constrained_pick_logits")):
        assert getattr(L, new).argtypes == getattr(L, old).argtypes, new     # the same argument lists
    assert L.i2l_version() >= 113
    assert [L.i2l_argument_state_bytes(r) for r in (-1, 0, 1, 67)] == [0, 0, 32, 32 * 67]


COMMON_REFUSALS = [
    ("end_id -1", dict(end_id=-1), _lib.ERR_ARG),
    ("end_id == vocab", dict(end_id=500), _lib.ERR_ARG),
    ("cls null", dict(cls=None), _lib.ERR_ARG),
    ("state null", dict(state=None), _lib.ERR_ARG),
    ("state one byte short", dict(state_bytes=4 * 32 - 1), _lib.ERR_WORKSPACE),
    ("state of the bracket size", dict(state_bytes=4 * 16), _lib.ERR_WORKSPACE),
    ("rows 0", dict(rows=0), _lib.ERR_ARG),
    ("steps 0", dict(steps=0), _lib.ERR_ARG),
    ("hidden 96", dict(H=96), _lib.ERR_UNSUPPORTED),
    ("scratch null", dict(scratch=None), _lib.ERR_WORKSPACE),
    ("scratch one byte short", dict(short=1), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", COMMON_REFUSALS, ids=[r[0] for r in COMMON_REFUSALS])
def test_decode_refusals_need_no_device(what, kw, code):
    """Every pointer is null or fake: a call that touched the device, or followed one of them, would not return a code."""
    kw = dict(kw)
    w, keep = _weights(H=kw.pop("H", 512))
    if kw.pop("short", 0):
        kw["scratch_bytes"] = _lib.lib().i2l_decode_batched_scratch_bytes(4, 500, 512, 2) - 1
    assert _greedy(w, **kw) == code, what
    assert _sample(w, **kw) == code, what
    del keep


def test_the_entries_own_argument_rules():
    w, keep = _weights()
    assert _greedy(w, select=_lib.SELECT_SAMPLE) == _lib.ERR_ARG
    assert _sample(w, top_k=0, top_p=0.0) == _lib.ERR_ARG
    assert _sample(w, temperature=0.0) == _lib.ERR_ARG
    assert _sample(w, top_p=float("nan")) == _lib.ERR_ARG
    w2, keep2 = _weights(V=2049)
    assert _sample(w2) == _lib.ERR_UNSUPPORTED
    del keep, keep2


PICK_REFUSALS = [
    ("ld < vocab", dict(ld=499), _lib.ERR_ARG),
    ("temperature 0", dict(temperature=0.0), _lib.ERR_ARG),
    ("top_k -1", dict(top_k=-1), _lib.ERR_ARG),
    ("top_p -0.1", dict(top_p=-0.1), _lib.ERR_ARG),
    ("top_p nan", dict(top_p=float("nan")), _lib.ERR_ARG),
    ("select sample", dict(select=_lib.SELECT_SAMPLE), _lib.ERR_ARG),
    ("rows 0", dict(rows=0), _lib.ERR_ARG),
    ("vocab 0", dict(vocab=0, ld=0), _lib.ERR_ARG),
    ("step -1", dict(step=-1), _lib.ERR_ARG),
    ("step == steps", dict(step=3), _lib.ERR_ARG),
    ("steps 0", dict(steps=0), _lib.ERR_ARG),
    ("end_id -1", dict(end_id=-1), _lib.ERR_ARG),
    ("end_id == vocab", dict(end_id=500), _lib.ERR_ARG),
    ("logits null", dict(logits=None), _lib.ERR_ARG),
    ("cls null", dict(cls=None), _lib.ERR_ARG),
    ("state null", dict(state=None), _lib.ERR_ARG),
    ("ids null", dict(ids=None), _lib.ERR_ARG),
    ("sampling at vocab 2049", dict(vocab=2049, ld=2049, top_k=5), _lib.ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("what,kw,code", PICK_REFUSALS, ids=[r[0] for r in PICK_REFUSALS])
def test_pick_logits_refusals_need_no_device(what, kw, code):
    assert _pick(**kw) == code, what


def test_the_python_surface_refuses_what_has_no_argument_form():
    """The N-best beam search would misread the bytes: refused before anything is launched."""
    from img2latex_amd.model.seq2seq_model import Seq2SeqModel
    table = ArgumentTable(SMALL, END)
    with pytest.raises(RuntimeError, match="greedy and sampling decode only"):
        Seq2SeqModel.beam_search_nbest(None, None, 1, END, 8, 3, constraint=table)      # refused before `self` is touched
