"""The error analysis on the host (no GPU).

csrc/edit_align_rules.inc.h -- the canonical edit script of a (target, prediction) pair and what it adds to the token
confusion matrix -- as a stand-alone program (csrc/edit_align_host_main.cpp), a process of its own under the host
sanitizers, compared with the Python restatement (edit_align_ref.py): scripts byte for byte, counts and matrices exactly,
from the full table AND from the bit vectors of the device's column pass.  Exhaustively over every pair of sequences of
0..4 tokens over a 3-token alphabet (121 x 121 pairs), on hand cases for the tie rules, and on longer pairs that span
several 64-row blocks.  Independently of the restatement every pair is held to the oracle's Levenshtein distance, to the
length identities, and to replaying the script.

Also here: the refusals of the three entries (they answer before the first HIP call), the report arithmetic, the bucket
edges, the CLI flag and the ``errors=None`` defaults."""
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import edit_align_ref as R
import metrics_oracle
import png_cases
from img2latex_amd import _lib, cli
from img2latex_amd.training import metrics as M
from img2latex_amd.training.predictor import Predictor

FAKE = 0x1000          # a non-null pointer that a refusing call never follows
a, b, c, d, e = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("edit_align_host")
    exe, sanitized = png_cases.build_host_program(str(out), "edit_align_host_main")
    return exe, str(out), sanitized


def _run(program, cases, tag):
    exe, work, _ = program
    src, dst = os.path.join(work, tag + ".bin"), os.path.join(work, tag + ".out")
    R.write_cases(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return R.read_results(dst, cases)


def _check(cases, results):
    """Every case, both paths: the restatement exactly, and the properties that do not need it."""
    for (r, p, V), both in zip(cases, results):
        want = R.script(r, p)
        C = np.zeros((V + 1, V + 1), dtype=np.int64)
        R.confusion_update(C, r, p, want, V)
        for ops, script, got_C in both:
            assert script == want, (r, p, script, want)
            assert ops == R.counts(want)
            assert (got_C == C).all()
            n_match, n_sub, n_del, n_ins = ops
            assert n_sub + n_del + n_ins == metrics_oracle.levenshtein_raw(r, p)
            assert n_match + n_sub + n_del == len(r)
            assert n_match + n_sub + n_ins == len(p)
            assert R.replay(r, p, script) == list(p)
            assert got_C[V, V] == 0


def test_sanitizers_are_on(program):
    assert program[2], "the host program was built without -fsanitize=address,undefined"


def test_every_pair_up_to_four_tokens(program):
    seqs = [list(s) for n in range(5) for s in itertools.product((a, b, c), repeat=n)]
    assert len(seqs) == 121
    cases = [(r, p, 3) for r in seqs for p in seqs]
    assert len(cases) == 14641
    _check(cases, _run(program, cases, "all"))


def test_tie_rules_by_hand(program):
    S, Dl, I, Mt = R.SUB, R.DEL, R.INS, R.MATCH
    hand = [
        # r = a a b, p = a b: the walk from the end matches b, matches r[1] with p[0], and the deletion lands on r[0]
        ([a, a, b], [a, b], [Dl, Mt, Mt]),
        ([a, a, a], [a, a], [Dl, Mt, Mt]),
        ([a, a], [a, a, a], [I, Mt, Mt]),
        # disjoint, unequal lengths: substitutions are taken before deletions / insertions, which end up in front
        ([a, a, a, a], [b, b], [Dl, Dl, S, S]),
        ([a, a], [b, b, b, b, b], [I, I, I, S, S]),
        ([], [a, b], [I, I]),
        ([a, b], [], [Dl, Dl]),
        ([], [], []),
    ]
    cases = [(r, p, 3) for r, p, _ in hand]
    results = _run(program, cases, "hand")
    _check(cases, results)
    for (r, p, want), both in zip(hand, results):
        assert R.script(r, p) == want
        assert both[0][1] == want and both[1][1] == want
    C = results[0][0][2]                                    # a a b -> a b: a deleted once, a and b matched once
    assert C[a, 3] == 1 and C[a, a] == 1 and C[b, b] == 1 and C.sum() == 3


def test_longer_pairs_span_blocks_and_ids_outside_the_vocabulary(program):
    rng = np.random.default_rng(7)
    cases = []
    for m, n in [(63, 64), (64, 65), (65, 63), (127, 129), (128, 128), (129, 200), (200, 130), (257, 70), (70, 257)]:
        for alphabet in (2, 3, 40):
            cases.append((rng.integers(0, alphabet, m).tolist(), rng.integers(0, alphabet, n).tolist(), 40))
        r = rng.integers(0, 5, m).tolist()
        cases.append((r, (r[1:] + r[:1])[:n], 40))          # the sequence against itself shifted by one
    r = rng.integers(-2, 12, 90).tolist()                   # ids < 0 and >= V inside the length
    p = rng.integers(-2, 12, 80).tolist()
    cases.append((r, p, 9))
    results = _run(program, cases, "long")
    _check(cases, results)
    for r, p, _ in cases:                                   # the numpy table the GPU test takes for its long pairs
        assert (R.table_fast(r, p) == np.array(R.table(r, p))).all()
    ops, _, C = results[-1][0]
    assert C.sum() < sum(ops)                               # the outside ids are counted in ops and absent from C


# ------------------------------------------------------------------------------------------------ the library's refusals
def test_symbols_and_version():
    L = _lib.lib()
    for name in ("i2l_edit_alignment", "i2l_edit_alignment_scratch_bytes", "i2l_confusion_margins", "i2l_confusion_top",
                 "i2l_confusion_top_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.i2l_version() >= 116 and _lib.ABI_VERSION >= 116


def test_refusals_answer_before_any_launch():
    L = _lib.lib()
    UNSUPPORTED, WORKSPACE, ARG = -2, -3, -1
    call = lambda ps, ts, V, scratch, nbytes, ops=FAKE, script=None, slen=None, conf=None, pairs=2: L.i2l_edit_alignment(
        FAKE, FAKE, ps, FAKE, FAKE, ts, pairs, V, scratch, nbytes, ops, script, slen, conf, None)
    assert call(1025, 64, 10, FAKE, 1 << 30) == UNSUPPORTED
    assert call(64, 1025, 10, FAKE, 1 << 30) == UNSUPPORTED
    assert call(64, 64, 2049, FAKE, 1 << 30) == UNSUPPORTED
    assert L.i2l_edit_alignment_scratch_bytes(3, 256, 256) == 0            # the vectors fit in LDS
    assert L.i2l_edit_alignment_scratch_bytes(3, 257, 256) == 3 * 257 * 4 * 16
    assert L.i2l_edit_alignment_scratch_bytes(3, 256, 257) == 3 * 256 * 8 * 16
    need = L.i2l_edit_alignment_scratch_bytes(2, 1024, 1024)
    assert need == 2 * 1024 * 16 * 16
    assert call(1024, 1024, 10, FAKE, need - 1) == WORKSPACE
    assert call(1024, 1024, 10, None, 0) == WORKSPACE
    assert call(64, 64, 10, None, 0, ops=None) == ARG                      # nothing asked for
    assert call(64, 64, 10, None, 0, script=FAKE) == ARG                   # the script without its lengths
    assert call(64, 64, 10, None, 0, pairs=0) == ARG
    assert L.i2l_confusion_margins(FAKE, 2049, FAKE, FAKE, FAKE, None) == UNSUPPORTED
    assert L.i2l_confusion_margins(FAKE, 10, None, None, None, None) == ARG
    top = lambda V, kinds, n, nbytes: L.i2l_confusion_top(FAKE, V, kinds, n, FAKE, nbytes, FAKE, FAKE, FAKE, FAKE, None)
    assert top(2049, 1, 5, 1 << 30) == UNSUPPORTED
    assert top(10, 1, 1025, 1 << 30) == UNSUPPORTED
    assert top(10, 0, 5, 1 << 30) == ARG and top(10, 16, 5, 1 << 30) == ARG and top(10, 1, 0, 1 << 30) == ARG
    assert top(2048, 1, 5, L.i2l_confusion_top_scratch_bytes(2048) - 1) == WORKSPACE
    assert L.i2l_confusion_top_scratch_bytes(3) == 1024 * 8


def test_python_entries_refuse_host_tensors():
    ids, lens = torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        M.device_edit_alignment(ids, lens, ids, lens, 10)
    with pytest.raises(RuntimeError):
        M.confusion_margins(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        M.ErrorAnalysis(2049, "cpu")


# ------------------------------------------------------------------------------------------------ the report
class _Tok:
    id_to_token = {0: "x", 1: "y", 2: "\\frac"}


def test_report_arithmetic_on_a_hand_made_matrix():
    V = 3
    C = np.array([[5, 2, 0, 1],        # x: 5 matched, 2 read as y, 1 deleted
                  [0, 4, 3, 0],        # y: 4 matched, 3 read as \frac
                  [0, 0, 0, 2],        # \frac: never right, 2 deleted
                  [0, 1, 6, 0]])       # inserted: y once, \frac 6 times
    row, col, diag = C.sum(1).tolist(), C.sum(0).tolist(), np.diag(C)[:V].tolist()
    subs, dels, ins = [(1, 2, 3), (0, 1, 2)], [(2, 3, 2), (0, 3, 1)], [(3, 2, 6), (3, 1, 1)]
    rep = M.build_report(V, row, col, diag, subs, dels, ins, [0, 0, 1, 2, 3, 4, 9], _Tok())
    assert rep["operations"] == {"match": 9, "substitution": 5, "deletion": 3, "insertion": 7}
    assert rep["top_substitutions"] == [{"target": "y", "predicted": "\\frac", "count": 3},
                                        {"target": "x", "predicted": "y", "count": 2}]
    assert rep["top_deletions"] == [{"target": "\\frac", "count": 2}, {"target": "x", "count": 1}]
    assert rep["top_insertions"] == [{"predicted": "\\frac", "count": 6}, {"predicted": "y", "count": 1}]
    per = {t["token"]: t for t in rep["per_token"]}
    assert per["x"]["recall"] == 5 / 8 and per["x"]["precision"] == 5 / 5
    assert per["y"]["recall"] == 4 / 7 and per["y"]["precision"] == 4 / 7
    assert per["\\frac"]["recall"] == 0.0 and per["\\frac"]["precision"] == 0 / 9
    assert [bk["count"] for bk in rep["distance_buckets"]] == [2, 1, 2, 2] and rep["pairs"] == 7
    ids = M.build_report(V, row, col, diag, subs, dels, ins, [])
    assert ids["top_substitutions"][0] == {"target": 1, "predicted": 2, "count": 3}
    md = M.report_markdown(rep)
    for heading in ("## Edit-distance buckets", "## Operation totals", "## Top substitutions", "## Top deleted tokens",
                    "## Top inserted tokens"):
        assert heading in md
    assert "counted in tokens" in md and "characters" in md
    absent = M.build_report(V, [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0], [], [(1, 3, 1)], [], [1])
    assert absent["per_token"] == [{"token": 1, "id": 1, "target_count": 1, "predicted_count": 0, "matches": 0,
                                    "recall": 0.0, "precision": None}]


def test_bucket_edges():
    assert M.DEFAULT_DISTANCE_RANGES == [[0, 0], [1, 1], [2, 3], [4, "inf"]]
    got = M.distance_buckets([0, 1, 1, 2, 3, 4, 5, 1000])
    assert [g["count"] for g in got] == [1, 2, 2, 3]
    assert [g["range"] for g in got] == [[0, 0], [1, 1], [2, 3], [4, "inf"]]
    assert got[3]["fraction"] == 3 / 8
    got = M.distance_buckets([0, 5, 6, 10, 11], [[0, 5], [6, 10], [11, float("inf")]])
    assert [g["count"] for g in got] == [2, 2, 1] and got[2]["range"] == [11, "inf"]
    assert [g["count"] for g in M.distance_buckets([])] == [0, 0, 0, 0]
    assert M.ErrorAnalysis.ranges_from_config({"analysis": {"error_distance_ranges": [[0, 2], [3, "inf"]]}}) == [[0, 2], [3, "inf"]]
    assert M.ErrorAnalysis.ranges_from_config({}) is None and M.ErrorAnalysis.ranges_from_config({"analysis": {}}) is None


# ------------------------------------------------------------------------------------------------ the public surface
def test_errors_is_off_by_default():
    for fn in (Predictor.evaluate_batch, Predictor.evaluate_stream, Predictor._evaluate_launch):
        assert inspect.signature(fn).parameters["errors"].default is None
    sig = inspect.signature(cli.evaluate).parameters
    assert sig["errors"].default is False and sig["errors_top"].default == 20


def test_cli_flag(monkeypatch):
    calls = []
    monkeypatch.setattr(cli, "evaluate", lambda *args, **kw: calls.append((args, kw)) or {})
    assert cli.main(["evaluate", "ckpt.pt", "data"]) == 0
    assert calls[-1][1] == {}                               # without the flag the call is the one it always was
    assert cli.main(["evaluate", "ckpt.pt", "data", "--errors"]) == 0
    assert calls[-1][1] == {"errors": True, "errors_top": 20}
    assert calls[-1][0] == calls[0][0]
    assert cli.main(["evaluate", "ckpt.pt", "data", "--errors", "--errors-top", "7"]) == 0
    assert calls[-1][1] == {"errors": True, "errors_top": 7}
    for bad in ("0", "1025"):
        with pytest.raises(SystemExit):
            cli.main(["evaluate", "ckpt.pt", "data", "--errors", "--errors-top", bad])
    with pytest.raises(SystemExit):
        cli.main(["predict", "ckpt.pt", "image.png", "--errors"])
