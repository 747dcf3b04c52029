"""The N-best, length-normalised beam search (i2l_beam_decode_nbest, Seq2SeqModel.beam_search_nbest) against its parent
entry, the float64 restatement of the rule (nbest_ref.py) and its own structure.

The search is i2l_beam_decode_batched's, so the parent is the anchor: nbest = 1 without a table must return its bits.
Against float64 the rule is the one of test_beam_batched_gpu.py, extended to the ranking: per image the rows' (tokens,
finished) lists and the count equal the float64 ones unless the float64 search has a candidate gap below 1e-4
(``stats["gap"]``) or a gap below 1e-4, relative to max(1, |key|), between neighbouring keys among its first N + 1
ranked entries (``stats["key_gap"]``); equal rows have score and key within 1e-4 relative to max(1, |value|); at most
one image per case may leave.  (On the CPU an fp32 run of the same restatement left 0 images in every case below, with
up to 7 of 8 images under a gap.)"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import nbest_ref
from conftest import record
from helpers import END, GOLDEN, START
from img2latex_amd import _lib
from test_decoder_shapes import build, enc_for, sid

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAP = 1e-4
SHIPPED = (500, 512, 512, 2, True)
TINY = (3, 4, 64, 1, False)
SENT_I, SENT_F = -7, 1.25          # what the output buffers hold before a call: no result is either


def penalty_table(steps, a):
    """norm[n] = float(n) ** a, norm[0] = 1; None at a = 0 (the entry's NULL)."""
    return None if a == 0 else [1.0] + [float(n) ** a for n in range(1, steps + 1)]


def gnmt_table(steps):
    return [((5 + n) / 6) ** 0.6 for n in range(steps + 1)]


def raw(m, enc, steps, k, N, norm=None, start=START, end=END, optional=True):
    """The C entry itself on sentinel-filled outputs; every array as the call left it."""
    dec = m.decoder
    w, keep, enc_c = dec.prepare(enc)
    n = enc_c.shape[0]
    L = _lib.lib()
    nbytes = L.i2l_beam_nbest_scratch_bytes(n, k, N, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, steps)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    tab = None if norm is None else torch.tensor(norm, dtype=torch.float64, device=DEV)
    o = dict(seq=torch.full((n, N, steps + 1), SENT_I, dtype=torch.int32, device=DEV),
             len=torch.full((n, N), SENT_I, dtype=torch.int32, device=DEV),
             score=torch.full((n, N), SENT_F, dtype=torch.float64, device=DEV),
             key=torch.full((n, N), SENT_F, dtype=torch.float64, device=DEV),
             fin=torch.full((n, N), SENT_I, dtype=torch.int32, device=DEV),
             count=torch.full((n,), SENT_I, dtype=torch.int32, device=DEV))
    _lib.check(L.i2l_beam_decode_nbest(ctypes.byref(w), dec._ws.data_ptr(), n, k, N, steps, start, end, _lib.ptr(tab),
                                       scratch.data_ptr(), nbytes, o["seq"].data_ptr(), o["len"].data_ptr(),
                                       o["score"].data_ptr(), o["key"].data_ptr() if optional else None,
                                       o["fin"].data_ptr() if optional else None, o["count"].data_ptr(), 0,
                                       _lib.stream_ptr()), "beam_decode_nbest")
    torch.cuda.synchronize()
    del keep, scratch, tab
    return {name: t.cpu().numpy() for name, t in o.items()}


def raw_parent(m, enc, steps, k, start=START, end=END):
    dec = m.decoder
    w, keep, enc_c = dec.prepare(enc)
    n = enc_c.shape[0]
    L = _lib.lib()
    nbytes = L.i2l_beam_batched_scratch_bytes(n, k, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, steps)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    seq = torch.full((n, steps + 1), SENT_I, dtype=torch.int32, device=DEV)
    ln = torch.full((n,), SENT_I, dtype=torch.int32, device=DEV)
    score = torch.full((n,), SENT_F, dtype=torch.float64, device=DEV)
    _lib.check(L.i2l_beam_decode_batched(ctypes.byref(w), dec._ws.data_ptr(), n, k, steps, start, end, scratch.data_ptr(),
                                         nbytes, seq.data_ptr(), ln.data_ptr(), score.data_ptr(), 0, _lib.stream_ptr()),
               "beam_decode_batched")
    torch.cuda.synchronize()
    del keep, scratch
    return seq.cpu().numpy(), ln.cpu().numpy(), score.cpu().numpy()


def rows_of(o, j):
    """Image j's filled rows as (tokens, finished), with their scores and keys."""
    c = int(o["count"][j])
    toks = [(o["seq"][j, r, :o["len"][j, r]].tolist(), bool(o["fin"][j, r])) for r in range(c)]
    return toks, o["score"][j, :c].tolist(), o["key"][j, :c].tolist()


def check_structure(o, V, k, N, steps, norm, start=START, end=END):
    """What holds of every result whatever the weights: section 3 of the module's subject."""
    n = o["count"].shape[0]
    for name in ("seq", "len", "fin", "count"):
        assert (o[name] != SENT_I).all(), name                     # every element written
    assert (o["score"] != SENT_F).all() and (o["key"] != SENT_F).all()
    for j in range(n):
        c = int(o["count"][j])
        assert 1 <= c <= N, (j, c)
        seen = set()
        lengths = []
        for r in range(N):
            ln, row = int(o["len"][j, r]), o["seq"][j, r]
            sc, key, fin = float(o["score"][j, r]), float(o["key"][j, r]), int(o["fin"][j, r])
            if r >= c:                                             # absent rows
                assert ln == -1 and (row == -1).all() and sc == -math.inf and key == -math.inf and fin == 0, (j, r)
                continue
            assert 0 <= ln <= steps and fin in (0, 1), (j, r, ln, fin)
            assert ((row[:ln] >= 0) & (row[:ln] < V)).all() and (start == end or end not in row[:ln]), (j, r, row)
            assert (row[ln:] == -1).all(), (j, r, row)
            assert math.isfinite(sc) and sc <= 0.0, (j, r, sc)
            nn = ln + 1 if fin else ln                             # tokens after START, END included
            assert fin or ln == steps, (j, r, ln)                  # an unfinished row ran all the steps
            want = sc if norm is None else sc / norm[0 if start == end else nn]
            assert key == want, (j, r, key, want)                  # fp64 division is correctly rounded: exact
            ident = (tuple(row[:ln].tolist()), fin)
            assert ident not in seen, (j, r, ident)                # all hypotheses of an image are distinct
            seen.add(ident)
            lengths.append(nn)
        # rows from `completed` (n <= steps, or the all-ended break at n == steps) come first with keys non-increasing,
        # then the leftover rows, all of n == steps, with keys non-increasing
        keys = o["key"][j, :c]
        drops = [r for r in range(1, c) if keys[r] > keys[r - 1]]
        assert len(drops) <= 1, (j, keys)
        if drops:
            assert all(nn == steps for nn in lengths[drops[0]:]), (j, keys, lengths)
    return o


# ------------------------------------------------------------------------------------------------ 1. the anchor
ANCHOR = [(TINY, 3, 7), ((777, 36, 192, 3, True), 5, 7), (SHIPPED, 2, 8), (SHIPPED, 5, 8)]


@pytest.mark.parametrize("shape,k,n", ANCHOR, ids=[f"{sid(s)}-k{k}-n{n}" for s, k, n in ANCHOR])
def test_one_row_without_a_table_is_the_parent_entry(shape, k, n):
    m, _, _ = build(shape)
    enc = enc_for(shape, n, seed=13)
    with torch.no_grad():
        seq, ln, sc = raw_parent(m, enc, 24, k)
        o = check_structure(raw(m, enc, 24, k, 1), shape[0], k, 1, 24, None)
        bare = raw(m, enc, 24, k, 1, optional=False)               # key_out and finished_out NULL
    assert (o["count"] == 1).all()
    assert np.array_equal(o["seq"][:, 0], seq) and np.array_equal(o["len"][:, 0], ln)
    assert np.array_equal(o["score"][:, 0].view(np.int64), sc.view(np.int64))         # bit-identical
    assert np.array_equal(o["key"][:, 0].view(np.int64), sc.view(np.int64))
    for name in ("seq", "len", "score", "count"):
        assert np.array_equal(bare[name], o[name]), name
    assert (bare["key"] == SENT_F).all() and (bare["fin"] == SENT_I).all()             # and left alone


# ------------------------------------------------------------------------------------------------ 2. the float64 restatement
# (shape, variant, K, images, steps)
CASES = [
    (TINY, None, 3, 7, 24),                          # N = 6 > K = 3 returns 6 rows
    ((40, 8, 64, 2, True), None, 3, 7, 24),
    ((40, 8, 64, 2, True), "flat", 5, 7, 16),        # no completed entry: every row is a leftover row
    ((777, 36, 192, 3, True), None, 5, 7, 24),
    (SHIPPED, None, 5, 8, 24),                       # 19 - 29 completed entries per image: more than any N
    (SHIPPED, None, 2, 8, 24),
    (SHIPPED, "flat", 5, 4, 24),                     # N = 10: an image with 8 completed + 2 leftover rows
]
RANKINGS = ["one", "K_0.7", "2K_1.0"]
_SEARCH, _RESULTS = {}, {}


def float64_searches(case):
    """The float64 search of every image of the case, once for every ranking of it."""
    if case not in _SEARCH:
        shape, variant, k, n, steps = case
        _, sd64, cfg = build(shape, variant)
        enc = enc_for(shape, n, seed=13)
        with torch.no_grad():
            _SEARCH[case] = [nbest_ref.search(sd64, cfg, enc[j:j + 1].double(), START, END, steps, k) for j in range(n)]
    return _SEARCH[case]


def check_vs_float64(case, N, norm, tag):
    shape, variant, k, n, steps = case
    m, _, _ = build(shape, variant)
    enc = enc_for(shape, n, seed=13)
    with torch.no_grad():
        o = check_structure(raw(m, enc, steps, k, N, norm), shape[0], k, N, steps, norm)
    left, below, worst, stats = 0, 0, 0.0, []
    for j, s in enumerate(float64_searches(case)):
        st = {}
        want = nbest_ref.rank(s, START, END, steps, N, norm, st)
        stats.append(st)
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
    record(f"nbest {tag}: scores and keys vs float64 [rel to max(1,|value|)]", worst)
    record(f"nbest {tag}: images leaving the float64 rows at a near-tie", left)
    record(f"nbest {tag}: images with a float64 candidate or key gap below 1e-4", below)
    assert left <= 1, (tag, left)
    return o, stats


@pytest.mark.parametrize("ranking", RANKINGS)
@pytest.mark.parametrize("case", CASES, ids=[f"{sid(c[0], c[1])}-k{c[2]}-n{c[3]}-t{c[4]}" for c in CASES])
def test_rows_vs_float64(case, ranking):
    k, steps = case[2], case[4]
    N, a = {"one": (1, 0.0), "K_0.7": (k, 0.7), "2K_1.0": (2 * k, 1.0)}[ranking]
    tag = f"{sid(case[0], case[1])} k={k} N={N} penalty={a} x {case[3]} images x {steps} steps"
    _RESULTS[(case, ranking)] = check_vs_float64(case, N, penalty_table(steps, a), tag)


def test_explicit_gnmt_table_vs_float64():
    """((5 + n) / 6) ** 0.6 through length_norm: norm[0] != 1 and no power of n."""
    case = CASES[4]
    check_vs_float64(case, 5, gnmt_table(24), f"{sid(SHIPPED)} k=5 N=5 GNMT table x 8 images x 24 steps")


def _result(case, ranking):
    if (case, ranking) not in _RESULTS:                            # run alone: compute what the case's own test would
        test_rows_vs_float64(case, ranking)
    return _RESULTS[(case, ranking)]


def test_the_cases_exercise_what_they_are_meant_to():
    # more completed entries than N: the list overflowed and dropped its tail
    o, stats = _result(CASES[4], "K_0.7")
    assert max(st["completed"] for st in stats) > 5 and all(st["completed"] >= 5 for st in stats)
    assert (o["count"] == 5).all() and (o["fin"] == 1).all()
    # no completed entry at all: every row is a leftover row of 16 tokens
    o, stats = _result(CASES[2], "2K_1.0")
    assert all(st["completed"] == 0 and st["leftover"] == 5 for st in stats)
    assert (o["count"] == 5).all() and (o["len"][:, :5] == 16 - o["fin"][:, :5]).all()
    # N > K returns more than K rows
    o, stats = _result(CASES[0], "2K_1.0")
    assert (o["count"] == 6).all() and all(st["completed"] > 6 for st in stats)
    # completed and leftover rows in one image
    o, stats = _result(CASES[6], "2K_1.0")
    mixed = [j for j, st in enumerate(stats) if 0 < st["completed"] < 10 and st["leftover"] > 0]
    assert mixed, stats
    for j in mixed:
        c = stats[j]["completed"]
        assert int(o["count"][j]) == min(10, c + stats[j]["leftover"])
        assert (o["fin"][j, :c] == 1).all()
        assert (o["len"][j, c:int(o["count"][j])] == 24 - o["fin"][j, c:int(o["count"][j])]).all()


# ------------------------------------------------------------------------------------------------ 4. edges
def test_start_equals_end():
    m, _, _ = build(SHIPPED)
    enc = enc_for(SHIPPED, 3, seed=13)
    for norm in (None, [2.0] + [1.0] * 5):
        with torch.no_grad():
            o = check_structure(raw(m, enc, 5, 3, 4, norm, START, START), SHIPPED[0], 3, 4, 5, norm, START, START)
        assert (o["count"] == 1).all() and (o["len"][:, 0] == 0).all() and (o["fin"][:, 0] == 1).all()
        assert (o["score"][:, 0] == 0.0).all() and (o["key"][:, 0] == 0.0).all() and (o["seq"] == -1).all()


@pytest.mark.parametrize("k,n,steps,N", [(1, 3, 24, 3), (3, 1, 24, 5), (3, 3, 1, 5), (1, 1, 1, 1), (2, 3, 24, 16)],
                         ids=["k1", "one_image", "one_step", "all_ones", "nbest16_k2"])
def test_edges_vs_float64(k, n, steps, N):
    """k = 1 (one hypothesis per search, whatever N), one image, one step (every row a leftover row, or the all-ended
    break), nbest = 16 beside k = 2."""
    case = (SHIPPED, None, k, n, steps)
    o, stats = check_vs_float64(case, N, penalty_table(steps, 0.7), f"edge k={k} N={N} x {n} images x {steps} steps")
    if k == 1:
        assert (o["count"] == 1).all()
    if steps == 1:
        assert (o["count"] == min(k, N)).all() and (o["len"][:, :min(k, N)] <= 1).all()
    if N == 16:
        assert max(int(c) for c in o["count"]) > k


# ------------------------------------------------------------------------------------------------ 5. the Python surface
def test_beam_search_nbest_is_the_raw_entry():
    m, _, _ = build(SHIPPED)
    enc = enc_for(SHIPPED, 4, seed=13)
    steps, k, N = 24, 5, 7
    with torch.no_grad():
        o = raw(m, enc, steps, k, N, penalty_table(steps, 0.7))
        hyps = m.beam_search_nbest(enc, START, END, steps, k, nbest=N, length_penalty=0.7)
        table = m.beam_search_nbest(enc, START, END, steps, k, nbest=N, length_norm=penalty_table(steps, 0.7))
        default = m.beam_search_nbest(enc, START, END, steps, k)
        parent = m.beam_search_batch(enc, START, END, steps, k, return_scores=True, flags=_lib.FLAG_BEAM_BATCHED)
    assert hyps == table and len(hyps) == 4
    for j in range(4):
        got, scores, keys = rows_of(o, j)
        assert [(h.tokens, h.finished) for h in hyps[j]] == got
        assert [h.score for h in hyps[j]] == scores and [h.key for h in hyps[j]] == keys
        assert len(default[j]) == k                                 # nbest=None means beam_size
        assert default[j][0].tokens == parent[0][j] and default[j][0].score == parent[1][j] == default[j][0].key
    with pytest.raises(RuntimeError):
        m.beam_search_nbest(enc, START, END, steps, k, nbest=17)
    with pytest.raises(RuntimeError):
        m.beam_search_nbest(enc, START, END, steps, 9, nbest=2)
    assert m.decoder.kernel_flags == 0


PT = os.path.join(GOLDEN, "predict_64x800.pt")
PNG = os.path.join(GOLDEN, "predict_page.png")


def test_predictor_nbest_on_the_fixture_checkpoint():
    """``Predictor.predict`` clamps beam_size to greedy as the reference does (test_predict_chain pins that), so the
    beam result to agree with at penalty 0 is the model's own under FLAG_BEAM_BATCHED, decoded by the same tokenizer."""
    from img2latex_amd.training import Predictor
    pred = Predictor.from_checkpoint(PT, device=torch.device(DEV))
    k, N, T = 3, 5, 40
    rows = pred.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T)
    assert 1 <= len(rows) <= N and all(isinstance(s, str) and key == sc <= 0.0 for s, sc, key in rows)
    with torch.no_grad():
        enc = pred.model.encoder(pred._prepare_image(PNG))
        beam, score = pred.model.beam_search_batch(enc, pred.tokenizer.start_token_id, pred.tokenizer.end_token_id, T, k,
                                                   return_scores=True, flags=_lib.FLAG_BEAM_BATCHED)
        hyps = pred.model.beam_search_nbest(enc, pred.tokenizer.start_token_id, pred.tokenizer.end_token_id, T, k, nbest=N)
    assert rows[0][0] == pred.tokenizer.decode(beam[0]) and rows[0][1] == score[0]
    assert len(rows) == len(hyps[0])
    assert rows == [(pred.tokenizer.decode(h.tokens), h.score, h.key) for h in hyps[0]]
    normed = pred.predict_nbest(PNG, beam_size=k, nbest=N, max_length=T, length_penalty=1.0)
    with torch.no_grad():
        hyps = pred.model.beam_search_nbest(enc, pred.tokenizer.start_token_id, pred.tokenizer.end_token_id, T, k, nbest=N,
                                            length_penalty=1.0)
    assert normed == [(pred.tokenizer.decode(h.tokens), h.score, h.key) for h in hyps[0]]
    assert len(pred.predict_nbest(PNG, beam_size=k, max_length=T)) <= k            # nbest=None means beam_size
    batch = pred.predict_batch_nbest([PNG, PNG], beam_size=k, nbest=N, max_length=T, length_penalty=1.0)
    assert batch == [normed, normed]
    assert pred.predict(PNG, beam_size=k, max_length=T) == json.loads(str(np.load(os.path.join(
        GOLDEN, "predict_64x800.npz"))["texts"]))["path_gray_png"]                     # and predict() did not move


def test_cli_prints_one_line_per_hypothesis(capsys):
    from img2latex_amd import cli
    from img2latex_amd.training import Predictor
    texts = json.loads(str(np.load(os.path.join(GOLDEN, "predict_64x800.npz"))["texts"]))
    for extra in ([], ["--beam-size", "3"], ["--nbest", "0", "--beam-size", "3", "--length-penalty", "0.7"]):
        assert cli.main(["predict", PT, PNG, "--max-length", "40"] + extra) == 0
        assert capsys.readouterr().out == "Generated LaTeX:\n" + texts["path_gray_png"] + "\n", extra     # the parent's bytes
    assert cli.main(["predict", PT, PNG, "--max-length", "40", "--beam-size", "3", "--nbest", "4", "--length-penalty",
                     "0.7"]) == 0
    lines = capsys.readouterr().out.split("\n")
    assert len(lines) == 5 and lines[-1] == ""
    want = Predictor.from_checkpoint(PT, device=torch.device(DEV)).predict_nbest(PNG, beam_size=3, nbest=4, max_length=40,
                                                                                 length_penalty=0.7)
    assert lines[:4] == [f"{key!r}\t{latex}" for latex, _, key in want]
    assert [float(ln.split("\t")[0]) for ln in lines[:4]] == [key for _, _, key in want]
