"""The bracket constraint on the host (no GPU): csrc/bracket_rules.inc.h as a stand-alone program
(csrc/bracket_rules_host_main.cpp), a process of its own under the host sanitizers, against the Python restatement
``BracketTable.replay`` -- per step the allowed mask, the pick and the 16 state bytes; the token classification of
``BracketTable.from_tokenizer``; and the refusals of the three C entries, which answer before the first HIP call."""
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
from img2latex_amd.training.constraint import BracketState, BracketTable
from img2latex_amd.training.predictor import TokenTable

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows


def make_table(rng, V, kinds, never=0.1):
    """(classes, end_id): every kind with at least one open and one closer where V has room, END neutral."""
    kinds = max(1, min(kinds, (V - 1) // 2))
    cols = rng.permutation(V)
    end = int(cols[0])
    classes = np.zeros(V, dtype=np.uint8)
    for k in range(kinds):
        classes[cols[1 + 2 * k]] = C.open_class(k)
        classes[cols[2 + 2 * k]] = C.close_class(k)
    for v in cols[1 + 2 * kinds:]:
        r = rng.random()
        if r < never:
            classes[v] = rng.choice([255, 9, 100])          # every value outside 0..8 is "never"
        elif r < never + 0.3:
            k = int(rng.integers(kinds))
            classes[v] = C.open_class(k) if rng.random() < 0.5 else C.close_class(k)
    return classes, end


def make_cases():
    rng = np.random.default_rng(20240611)
    out = []
    for V in (5, 37, 200):
        for steps in (1, 2, 3, 40, 80):
            for kinds in (1, 2, 3, 4):
                for biased in (False, True):
                    classes, end = make_table(rng, V, kinds)
                    x = rng.standard_normal((steps, V)).astype(np.float32)
                    if biased:                              # toward opens: depth 32 is reached at steps 80
                        x[:, (classes >= 1) & (classes <= 4)] += 6.0
                    out.append(dict(V=V, steps=steps, end=end, classes=classes, logits=x, broken=False, biased=biased))
    # a deliberately broken table: kind 1 opens and nothing closes it -> at some step no column is allowed
    classes = np.zeros(6, dtype=np.uint8)
    classes[1] = C.open_class(1)
    x = np.zeros((6, 6), dtype=np.float32)
    x[:, 1] = 5.0
    out.append(dict(V=6, steps=6, end=0, classes=classes, logits=x, broken=True, biased=True))
    return out


def write_cases(path, cs):
    with open(path, "wb") as f:
        f.write(b"BRKT" + struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<3i", c["V"], c["steps"], c["end"]))
            f.write(c["classes"].tobytes())
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
            rows.append((mask, pick, data[pos:pos + 16]))
            pos += 16
        out.append(rows)
    assert pos == len(data)
    return out


def test_the_rules_as_a_sanitized_host_program(tmp_path):
    cs = make_cases()
    exe, sanitized = png_cases.build_host_program(str(tmp_path), "bracket_rules_host_main")
    print("bracket_rules_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of bracket_rules_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write_cases(src, cs)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])

    fired, deepest = set(), 0
    for i, (c, rows) in enumerate(zip(cs, read_results(dst, cs))):
        table = BracketTable(c["classes"])
        want = table.replay(c["logits"], end_id=c["end"])
        assert len(want) == len(rows) == c["steps"]
        for t, (w, (mask, pick, state)) in enumerate(zip(want, rows)):
            assert np.array_equal(mask, w["allowed"]), (i, t)
            assert pick == w["id"], (i, t)
            assert state == w["state"].to_bytes(), (i, t, BracketState.from_bytes(state), w["state"])
            if w["rule"]:
                fired.add(w["rule"])
            deepest = max(deepest, w["state"].depth)
        ids = [w["id"] for w in want]
        if c["broken"]:
            # depth 1, END forbidden, no closer of kind 1, budget gone: nothing is allowed and the pick is end_id
            empty = [t for t, w in enumerate(want) if not w["allowed"].any()]
            assert empty and all(ids[t] == c["end"] for t in empty), (i, ids)
            assert not table.well_formed(ids, c["end"])
            continue
        assert all(w["allowed"].any() for w in want), i                     # the allowed set is never empty
        assert c["end"] in ids, (i, ids)
        n = ids.index(c["end"])
        assert want[n]["state"].depth == 0 and want[n]["state"].ended == 1, i
        assert table.well_formed(ids, c["end"]), (i, ids)
        if c["steps"] == 1:
            assert ids == [c["end"]], i
    assert deepest == C.MAX_DEPTH
    assert fired == set(range(1, 7)), fired                                 # every rule overrode the free arg max somewhere


def test_state_bytes_round_trip():
    s = BracketState(stack=0x2D, depth=3, ended=0)
    assert len(s.to_bytes()) == C.STATE_BYTES == 16 and BracketState.from_bytes(s.to_bytes()) == s
    assert BracketState().to_bytes() == bytes(16)
    assert s.top() == 2


TOKENS = ["<PAD>", "<START>", "<END>", "<UNK>", "{", "}", "\\{", "\\}", "\\left(", "\\left", "\\leftarrow", "\\right)",
          "\\right.", "\\rightarrow", "\\begin{array}", "\\end{array}", "x", "\\frac"]


def test_from_tokenizer_classifies_the_token_strings():
    tok = TokenTable({t: i for i, t in enumerate(TOKENS)})
    table = BracketTable.from_tokenizer(tok)
    want = {"<PAD>": 255, "<START>": 255, "<UNK>": 255, "<END>": 0, "{": 1, "}": 5, "\\{": 0, "\\}": 0, "\\left(": 2,
            "\\left": 2, "\\leftarrow": 0, "\\right)": 6, "\\right.": 6, "\\rightarrow": 0, "\\begin{array}": 3,
            "\\end{array}": 7, "x": 0, "\\frac": 0}
    assert {t: int(table.classes[i]) for i, t in enumerate(TOKENS)} == want
    assert table.end_id == tok.end_token_id and table.unclosable == [] and table.vocab == len(TOKENS)
    enc = lambda s: tok.encode(s) + [tok.end_token_id]
    assert table.well_formed(enc("\\frac { x } { \\left( x \\right. }"))
    assert table.well_formed(enc("\\begin{array} { x \\{ } \\end{array}"))
    assert not table.well_formed(enc("{ x"))                                # a group left open
    assert not table.well_formed(enc("{ \\left( } \\right)"))               # closed out of order
    assert not table.well_formed(enc("x }"))                                # closes what was never opened
    assert not table.well_formed(tok.encode("{ }"))                         # no END
    assert not table.well_formed(enc("x <UNK>"))                            # a never column


def test_an_open_without_a_closer_is_never_emitted():
    tokens = [t for t in TOKENS if not t.startswith("\\right") and t != "\\end{array}"]
    tok = TokenTable({t: i for i, t in enumerate(tokens)})
    table = BracketTable.from_tokenizer(tok)
    assert sorted(table.unclosable) == sorted(["\\left(", "\\left", "\\begin{array}"])
    for t in table.unclosable:
        assert table.classes[tok.token_to_id[t]] == 255
    assert table.classes[tok.token_to_id["{"]] == 1 and table.classes[tok.token_to_id["\\leftarrow"]] == 0


def test_the_builder_keeps_end_neutral_and_folds_unknown_classes():
    with pytest.raises(ValueError):
        BracketTable([0, 1, 5], end_id=1)
    with pytest.raises(ValueError):
        BracketTable([0, 1, 5], end_id=3)
    with pytest.raises(ValueError):
        BracketTable([0, 1, 5]).replay(np.zeros((2, 3), np.float32), end_id=2)
    assert BracketTable([0, 9, 77, 255, 8]).classes.tolist() == [0, 255, 255, 255, 8]


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
    return _lib.lib().i2l_greedy_decode_constrained(ctypes.byref(w), FAKE, rows, steps, FAKE, None, None, 1.0, select,
                                                    _lib.STOP_NONE, end_id, FAKE, None, None, None, scratch, scratch_bytes,
                                                    0, None, 0, cls, state, state_bytes, None)


def _sample(w, rows=4, steps=3, temperature=1.0, top_k=5, top_p=0.9, end_id=2, scratch=FAKE, scratch_bytes=1 << 40,
            cls=FAKE, state=FAKE, state_bytes=1 << 20):
    return _lib.lib().i2l_sample_decode_constrained(ctypes.byref(w), FAKE, rows, steps, FAKE, None, None, temperature,
                                                    top_k, top_p, 7, _lib.STOP_NONE, end_id, FAKE, None, None, None,
                                                    scratch, scratch_bytes, 0, cls, state, state_bytes, None)


def _pick(logits=FAKE, ld=500, rows=4, vocab=500, temperature=1.0, select=_lib.SELECT_LOGITS, top_k=0, top_p=0.0, step=0,
          steps=3, cls=FAKE, end_id=2, state=FAKE, ids=FAKE):
    return _lib.lib().i2l_constrained_pick_logits(logits, ld, rows, vocab, temperature, select, top_k, top_p, 7, step,
                                                  steps, cls, end_id, state, ids, None, None, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_greedy_decode_constrained", "i2l_sample_decode_constrained", "i2l_constrained_pick_logits"):
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"^size_t\s+i2l_bracket_state_bytes\s*\(", header, flags=re.M)
    assert len(_lib.lib().i2l_greedy_decode_constrained.argtypes) == 24
    assert len(_lib.lib().i2l_sample_decode_constrained.argtypes) == 24
    assert len(_lib.lib().i2l_constrained_pick_logits.argtypes) == 18
    assert _lib.lib().i2l_version() >= 111
    L = _lib.lib()
    assert [L.i2l_bracket_state_bytes(r) for r in (-1, 0, 1, 67)] == [0, 0, 16, 16 * 67]


COMMON_REFUSALS = [
    ("end_id -1", dict(end_id=-1), _lib.ERR_ARG),
    ("end_id == vocab", dict(end_id=500), _lib.ERR_ARG),
    ("cls null", dict(cls=None), _lib.ERR_ARG),
    ("state null", dict(state=None), _lib.ERR_ARG),
    ("state one byte short", dict(state_bytes=4 * 16 - 1), _lib.ERR_WORKSPACE),
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
