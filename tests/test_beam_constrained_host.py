"""The well-formed N-best beam search on the host (no GPU).

csrc/beam_bracket_rules.inc.h -- the bracket rules inside the beam rules -- as a stand-alone program
(csrc/beam_constrained_host_main.cpp), a process of its own under the host sanitizers, running WHOLE constrained searches
on a table-driven model: ``lp[t][last token][V]`` float32 multiples of 1/8, taken as they are (the renormalisation is the
device's and is held on the GPU), so sums are exact in fp64 and score ties are exact and frequent.  Compared with the
Python restatement (constrained_beam_ref.py) on the same tables: per step the slots' tokens, parents, score bits,
candidate counts and 16 state bytes, then rows, score and key bits, ``finished`` and the count.

Also here: ``beam_rank`` under a null count against counts all K on the exact-tie inputs of test_beam_rules_host.py, the
refusals of i2l_beam_decode_nbest_constrained (they answer before the first HIP call), the CLI's option rules, and the
restatement itself pinned in float64 -- all-allowing it IS nbest_ref.search."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import constrained_beam_ref as R
import nbest_ref
import png_cases
import test_beam_rules_host as BR
from helpers import END, START, load, np_state_dict
from img2latex_amd import _lib, synth
from img2latex_amd.training import constraint as C
from img2latex_amd.training.constraint import BracketState, BracketTable
from test_bracket_rules_host import make_table

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows


# ------------------------------------------------------------------------------------------------ whole searches
def make_case(rng, V, K, T, kinds, N, norm=False, biased=False, start=None, classes=None, end=None, lp=None):
    if classes is None:
        classes, end = make_table(rng, V, kinds)
    if lp is None:
        lp = rng.integers(-24, 1, size=(T, V, V)).astype(np.float32) / 8          # multiples of 1/8 in [-3, 0]
        if biased:                                                               # toward opens: depth 32 at steps 80
            lp[:, :, (classes >= 1) & (classes <= 4)] += 6.0
    start = int(rng.integers(V)) if start is None else start
    table_norm = [1.0] + [float(n) ** 0.7 for n in range(1, T + 1)] if norm else None
    return dict(V=V, K=K, T=T, N=N, start=start, end=end, classes=classes, lp=lp, norm=table_norm)


def make_cases():
    rng = np.random.default_rng(20240917)
    out = []
    for V in (5, 37):
        for K in (1, 2, 5, 8):
            for T in (1, 2, 3, 12, 40):
                for kinds in (1, 2, 3, 4):
                    out.append(make_case(rng, V, K, T, kinds, N=(1, 3, 16)[len(out) % 3], norm=len(out) % 2 == 1))
    special = {}
    special["deep"] = len(out)                  # an open-biased table: depth 32 is reached at steps 80
    out.append(make_case(rng, 37, 3, 80, 2, N=4, biased=True))
    special["few"] = len(out)                   # steps 2, one neutral column: END and it are all step 0 allows, K = 5
    classes = np.array([0, 0, C.open_class(0), C.close_class(0), 255, C.open_class(1), C.close_class(1)], dtype=np.uint8)
    out.append(make_case(rng, 7, 5, 2, 2, N=5, classes=classes, end=0, start=4))
    special["broken"] = len(out)                # test_bracket_rules_host's: kind 1 opens and nothing closes it
    classes = np.zeros(6, dtype=np.uint8)
    classes[1] = C.open_class(1)
    lp = np.zeros((6, 6, 6), dtype=np.float32)
    lp[:, :, 1] = 5.0
    out.append(make_case(rng, 6, 3, 6, 1, N=4, classes=classes, end=0, start=2, lp=lp))
    special["start_is_end"] = len(out)
    c = make_case(rng, 37, 5, 12, 3, N=3, norm=True)
    c["start"] = c["end"]
    out.append(c)
    return out, special


def write_cases(path, cs):
    with open(path, "wb") as f:
        f.write(b"BMCN" + struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<7i", c["V"], c["K"], c["T"], c["N"], c["start"], c["end"], c["norm"] is not None))
            if c["norm"] is not None:
                f.write(struct.pack(f"<{c['T'] + 1}d", *c["norm"]))
            f.write(np.ascontiguousarray(c["classes"], dtype=np.uint8).tobytes())
            f.write(np.ascontiguousarray(c["lp"], dtype="<f4").tobytes())


class Reader:
    def __init__(self, path):
        self.data, self.pos = open(path, "rb").read(), 0

    def take(self, fmt):
        v = struct.unpack_from(fmt, self.data, self.pos)
        self.pos += struct.calcsize(fmt)
        return v

    def rows(self, N, T):
        (count,) = self.take("<i")
        rows = []
        for _ in range(N):
            ln, fin, sc, key = self.take("<ii8s8s")
            rows.append((ln, fin, sc, key, list(self.take(f"<{T + 1}i"))))
        return count, rows


def read_results(path, cs):
    """[(steps: [(t, nnew, [(token, parent, score bytes, candidates, state bytes)] * K)], count, rows)]"""
    rd, out = Reader(path), []
    for c in cs:
        steps = []
        while True:
            (t,) = rd.take("<i")
            if t < 0:
                break
            (nnew,) = rd.take("<i")
            steps.append((t, nnew, [rd.take("<ii8si16s") for _ in range(c["K"])]))
        out.append((steps,) + rd.rows(c["N"], c["T"]))
    assert rd.pos == len(rd.data)
    return out


def run_program(tmp_path, writer, cs):
    exe, sanitized = png_cases.build_host_program(str(tmp_path), "beam_constrained_host_main")
    print("beam_constrained_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of beam_constrained_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    writer(src, cs)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return dst


def table_rows(c):
    lp = torch.from_numpy(c["lp"])
    return lambda t, tokens, hidden: (lp[t, tokens[-1]], None)


def check_rows(count, rows, want, T, where):
    assert count == len(want), where
    for j, row in enumerate(rows):
        if j < count:
            w = want[j]
            assert row == (len(w.tokens), int(w.finished), BR.bits(w.score), BR.bits(w.key), BR.padded(w.tokens, T)), (where, j)
        else:
            assert row == (-1, 0, BR.bits(float("-inf")), BR.bits(float("-inf")), [-1] * (T + 1)), (where, j)


def test_whole_searches_as_a_sanitized_host_program(tmp_path):
    cs, special = make_cases()
    dst = run_program(tmp_path, write_cases, cs)
    deepest, short_lists, ties = 0, 0, 0
    for i, (c, (steps, count, rows)) in enumerate(zip(cs, read_results(dst, cs))):
        K, T, N, end = c["K"], c["T"], c["N"], c["end"]
        table = BracketTable(c["classes"])
        trace = []
        s = R.search(table_rows(c), table, c["start"], end, T, K, softmax=False, trace=trace)
        assert [t for t, _, _ in steps] == list(range(len(trace))), i
        for (t, nnew, slots), w in zip(steps, trace):
            assert nnew == len(w["tokens"]), (i, t)
            for q, (tok, par, sc, nc, state) in enumerate(slots):
                assert nc == (w["counts"][q] if q < len(w["counts"]) else 0), (i, t, q)
                if q < nnew:
                    assert (tok, par, sc) == (w["tokens"][q], w["parents"][q], BR.bits(w["scores"][q])), (i, t, q)
                    assert state == w["states"][q].to_bytes(), (i, t, q, BracketState.from_bytes(state), w["states"][q])
                    deepest = max(deepest, w["states"][q].depth)
                else:
                    assert (tok, par, sc, state) == (0, 0, BR.bits(0.0), bytes(16)), (i, t, q)
            live = [n for n in w["counts"] if n]
            short_lists += any(n < K for n in live)
            ties += len(set(w["scores"])) < len(w["scores"])
            if t == T - 1 and i != special["broken"]:
                assert live and all(n == 1 for n in live) and all(tok == end for tok in w["tokens"]), (i, t)
        want = nbest_ref.rank(s, c["start"], end, T, N, c["norm"])
        check_rows(count, rows, want, T, i)
        ids = [w.tokens + [end] for w in want]
        if i == special["broken"]:
            # depth 1, END forbidden, no closer of kind 1, budget gone: the fallback END at 0.0, not well formed
            assert any(tok == end and st.depth > 0 for w in trace for tok, st in zip(w["tokens"], w["states"])), i
            assert any(not table.well_formed(x, end) for x in ids), ids
            assert all(w.finished for w in want)
            continue
        assert not s.ran_out and 1 <= count <= N, i                         # a constrained search never runs out of steps
        assert all(w.finished and table.well_formed(x, end) for w, x in zip(want, ids)), (i, ids)
        if T == 1 or i == special["start_is_end"]:
            assert [w.tokens for w in want] == [[]], i
        if i == special["start_is_end"]:
            assert not trace and want[0].score == 0.0
        if i == special["few"]:
            assert trace[0]["counts"] == [2], trace[0]                      # END and the neutral column, K = 5
    assert deepest == C.MAX_DEPTH
    assert short_lists > 50 and ties > 50, (short_lists, ties)


def test_every_live_slot_has_a_candidate():
    """For a BracketTable-built table and finite values: at least one candidate in every state the rules can reach, and
    END alone at rem 0.  States are walked breadth first on a small table."""
    table = BracketTable([0, 0, C.open_class(0), C.close_class(0), C.open_class(3), C.close_class(3), 255])
    end, steps = 0, 7
    row = np.linspace(-1.0, 1.0, 7).astype(np.float32)
    frontier = [BracketState()]
    for t in range(steps):
        rem, nxt = steps - t - 1, []
        for st in frontier:
            picks = table.candidates(st, row, end, rem, 8)
            assert picks and all(table.allowed(st, end, rem)[v] for v, _ in picks), (t, st)
            assert [lp for _, lp in picks] == sorted((lp for _, lp in picks), reverse=True)
            if rem == 0:
                assert [v for v, _ in picks] == [end], (t, st)
            for v, _ in picks:
                if v != end:
                    s2 = st.copy()
                    table.advance(s2, v, end)
                    nxt.append(s2)
        frontier = nxt
    assert not frontier


def test_candidates_renormalise_over_the_allowed_columns():
    table = BracketTable([0, 0, C.open_class(0), C.close_class(0), 255])
    x = np.array([0.5, 2.0, 1.0, 3.0, 9.0])
    st = BracketState()
    picks = table.candidates(st, x, 0, 5, 2, logits=True)                  # closer and never are out: columns 0, 1, 2
    lse = np.log(np.exp(x[:3] - 2.0).sum())
    assert [v for v, _ in picks] == [1, 2]
    assert picks[0][1] == (2.0 - 2.0) - lse and picks[1][1] == (1.0 - 2.0) - lse
    table.advance(st, 2, 0)
    assert table.candidates(st, x, 0, 1, 3, logits=True) == [(3, 0.0)]      # a forced closer costs 0
    assert table.candidates(st, np.full(5, -np.inf), 0, 1, 3, logits=True) == [(0, 0.0)]   # nothing finite: the fallback
    ties = table.candidates(BracketState(), np.zeros(5, dtype=np.float32), 0, 5, 3)
    assert [v for v, _ in ties] == [0, 1, 2]                                # the lower index first


def test_null_counts_are_counts_all_k(tmp_path):
    """beam_rank(ncand = null), what every caller from before the constraint passes, against counts all K on the exact-tie
    inputs of test_beam_rules_host.py: the same bytes, and the rows that test expects."""
    cs = BR.cases()
    rd = Reader(run_program(tmp_path, BR.write_cases, cs))
    for i, c in enumerate(cs):
        null = rd.rows(c["N"], c["T"])
        full = rd.rows(c["N"], c["T"])
        assert null == full, i
        check_rows(null[0], null[1], nbest_ref.rank(BR.search(c), c["start"], c["end"], c["T"], c["N"], c["norm"]), c["T"], i)
    assert rd.pos == len(rd.data)


# ------------------------------------------------------------------------------------------------ the C entry's refusals
def _weights(V=500, E=512, H=512, L=2):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _call(w, images=4, beam=3, nbest=5, steps=5, end_id=2, workspace=FAKE, norm=None, scratch=FAKE, scratch_bytes=1 << 40,
          seq=FAKE, ln=FAKE, score=FAKE, key=None, fin=None, count=FAKE, cls=FAKE):
    return _lib.lib().i2l_beam_decode_nbest_constrained(ctypes.byref(w) if w is not None else None, workspace, images, beam,
                                                        nbest, steps, 1, end_id, norm, scratch, scratch_bytes, seq, ln, score,
                                                        key, fin, count, 0, cls, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    assert re.search(r"^size_t\s+i2l_beam_nbest_constrained_scratch_bytes\s*\(", header, flags=re.M)
    assert re.search(r"^int\s+i2l_beam_decode_nbest_constrained\s*\(", header, flags=re.M)
    for name in ("i2l_beam_nbest_constrained_scratch_bytes", "i2l_beam_decode_nbest_constrained"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert len(_lib.lib().i2l_beam_nbest_constrained_scratch_bytes.argtypes) == 7
    assert len(_lib.lib().i2l_beam_decode_nbest_constrained.argtypes) == 20
    assert _lib.lib().i2l_version() >= 112


def test_scratch_size_query():
    q, parent = _lib.lib().i2l_beam_nbest_constrained_scratch_bytes, _lib.lib().i2l_beam_nbest_scratch_bytes
    V, H, L = 500, 512, 2
    for what, args in {"nbest 0": (4, 2, 0, V, H, L, 150), "nbest 17": (4, 2, 17, V, H, L, 150),
                       "beam 9": (4, 9, 5, V, H, L, 150), "V 2049": (4, 2, 5, 2049, H, L, 150),
                       "H 96": (4, 2, 5, V, 96, L, 150), "steps 0": (4, 2, 5, V, H, L, 0),
                       "images 0": (0, 2, 5, V, H, L, 150), "beam 0": (4, 0, 5, V, H, L, 150),
                       "beam > vocab": (4, 4, 5, 3, 64, 1, 10)}.items():
        assert q(*args) == 0, what
    for n, k, nb in ((1, 2, 1), (16, 5, 5), (128, 5, 10), (3, 8, 16)):      # the parent's scratch plus 16 bytes per slot
        assert q(n, k, nb, V, H, L, 150) >= parent(n, k, nb, V, H, L, 150) + 16 * n * k
    assert q(1, 1, 1, 37, 64, 1, 1) > 0


REFUSALS = [
    ("weights null", dict(w=None), _lib.ERR_ARG), ("workspace null", dict(workspace=None), _lib.ERR_ARG),
    ("scratch null", dict(scratch=None), _lib.ERR_ARG), ("seq_out null", dict(seq=None), _lib.ERR_ARG),
    ("len_out null", dict(ln=None), _lib.ERR_ARG), ("score_out null", dict(score=None), _lib.ERR_ARG),
    ("count_out null", dict(count=None), _lib.ERR_ARG), ("cls null", dict(cls=None), _lib.ERR_ARG),
    ("end_id -1", dict(end_id=-1), _lib.ERR_ARG), ("end_id == vocab", dict(end_id=500), _lib.ERR_ARG),
    ("images 0", dict(images=0), _lib.ERR_ARG), ("steps 0", dict(steps=0), _lib.ERR_ARG), ("beam 0", dict(beam=0), _lib.ERR_ARG),
    ("nbest 0", dict(nbest=0), _lib.ERR_ARG), ("nbest 17", dict(nbest=17), _lib.ERR_UNSUPPORTED),
    ("beam 9", dict(beam=9), _lib.ERR_UNSUPPORTED), ("V 2049", dict(V=2049), _lib.ERR_UNSUPPORTED),
    ("H 96", dict(H=96), _lib.ERR_UNSUPPORTED), ("L 5", dict(L=5), _lib.ERR_UNSUPPORTED),
    ("scratch one byte short", dict(short=1), _lib.ERR_WORKSPACE), ("scratch 0 bytes", dict(scratch_bytes=0), _lib.ERR_WORKSPACE),
    ("the unconstrained scratch size", dict(short="parent"), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_need_no_device(what, kw, code):
    """Every pointer is null or fake: a call that touched the device, or followed one of them, would not return a code."""
    kw = dict(kw)
    w, keep = _weights(**{k: kw.pop(k) for k in ("V", "H", "L") if k in kw})
    if "w" in kw:
        w = kw.pop("w")
    short = kw.pop("short", None)
    if short == 1:
        kw["scratch_bytes"] = _lib.lib().i2l_beam_nbest_constrained_scratch_bytes(4, 3, 5, 500, 512, 2, 5) - 1
    elif short == "parent":
        kw["scratch_bytes"] = _lib.lib().i2l_beam_nbest_scratch_bytes(4, 3, 5, 500, 512, 2, 5)
    assert _call(w, **kw) == code, what
    del keep


def test_optional_outputs_and_the_table_are_no_refusal():
    w, keep = _weights()
    for kw in (dict(), dict(key=FAKE, fin=FAKE, norm=FAKE)):
        assert _call(w, scratch_bytes=0, **kw) == _lib.ERR_WORKSPACE, kw
    del keep


# ------------------------------------------------------------------------------------------------ the Python surface
def test_inference_with_a_beam_still_refuses_a_constraint():
    from img2latex_amd.model import Seq2SeqModel
    cfg = synth.model_config(vocab_size=5, embedding_dim=4, hidden_dim=64, lstm_layers=1, attention=False, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16))
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))

    class Encoded(torch.nn.Module):                        # the refusal comes before any kernel: no device is needed
        def forward(self, image):
            return torch.zeros(1, 4)
    m.encoder = Encoded()
    with pytest.raises(RuntimeError, match="beam_search_nbest"):
        m.inference(torch.zeros(1, 1, 16, 32), START, END, 6, beam_size=3, constraint=BracketTable([0] * 5))


def test_cli_option_rules(monkeypatch, capsys):
    from img2latex_amd import cli
    for argv in (["predict", "ck.pt", "x.png", "--well-formed", "--beam-size", "3"],
                 ["predict", "ck.pt", "x.png", "--well-formed", "--nbest", "2"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv                     # argparse's error exit
    assert "--nbest 1" in capsys.readouterr().err
    seen = []

    def fake(checkpoint_path, image_path, beam_size, nbest, *args, **kw):
        seen.append((beam_size, nbest, kw.get("well_formed")))
        return [("x ^ { 2 }", -1.0, -0.5)]
    monkeypatch.setattr(cli, "predict_nbest", fake)
    assert cli.main(["predict", "ck.pt", "x.png", "--nbest", "2", "--beam-size", "3", "--well-formed"]) == 0
    assert cli.main(["predict", "ck.pt", "x.png", "--nbest", "1", "--beam-size", "3"]) == 0
    assert seen == [(3, 2, True), (3, 1, False)]
    assert capsys.readouterr().out == "-0.5\tx ^ { 2 }\n" * 2


# ------------------------------------------------------------------------------------------------ the restatement, pinned
@pytest.mark.parametrize("name", ["tiny_l1", "tiny_l2_attn"])
def test_restatement_in_float64(name):
    """All-allowing, constrained_beam_ref.search IS nbest_ref.search: the same completed and final beams, the same
    Python-float scores, the same gap.  With a real table every row is well formed and the search does not run out."""
    _, cfg, _ = load(name)
    sd64 = {k: torch.from_numpy(v).double() for k, v in np_state_dict(name).items() if k.startswith("decoder.")}
    n, steps, V = 3, 16, cfg["vocab_size"]
    enc = torch.from_numpy(synth.uniform(13, "enc", (n, cfg["embedding_dim"]), -1.5, 1.5)).double()
    rng = np.random.default_rng(5)
    classes, _ = make_table(rng, V, 2, never=0.0)
    classes[END] = 0
    if classes[START] in (C.open_class(0), C.close_class(0)):
        classes[START] = 0
    table = BracketTable(classes, END)
    for k in (1, 3, 5):
        if k > V:
            continue
        for j in range(n):
            with torch.no_grad():
                rows = R.oracle_rows(sd64, cfg, enc[j:j + 1])
                assert R.search(rows, None, START, END, steps, k) == nbest_ref.search(sd64, cfg, enc[j:j + 1], START, END, steps, k)
                s = R.search(rows, table, START, END, steps, k)
            assert not s.ran_out and s.completed
            want = nbest_ref.rank(s, START, END, steps, 2 * k)
            assert want and all(r.finished and table.well_formed(r.tokens + [END]) for r in want), (name, k, j, want)
            assert all(r.score <= 0.0 for r in want)
