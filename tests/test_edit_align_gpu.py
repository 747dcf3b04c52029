"""The error analysis on the device: i2l_edit_alignment, i2l_confusion_margins, i2l_confusion_top and the public path on
top of them, against the Python restatement (edit_align_ref.py) and numpy.  Everything is integer work: every comparison
is exact equality.

The batches put lengths on the borders of the 64-row bit-vector blocks (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024)
and on both sides of the place where the columns' vectors leave LDS for the caller's scratch (256 / 257), each with an
equal, a shorter and a longer partner, and contents where ties are dense: identical sequences, sequences sharing no
token, a sequence against itself shifted by one, two-token alphabets.  Rows are wider than the lengths and filled with
-1 and V + 7 behind them; some ids inside the lengths lie outside [0, V)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import edit_align_ref as R
from helpers import END, GOLDEN, PAD, START
from img2latex_amd import _lib
from img2latex_amd.training import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
PT = os.path.join(GOLDEN, "predict_64x800.pt")
PNG = os.path.join(GOLDEN, "predict_page.png")


# ------------------------------------------------------------------------------------------------ the batches
def _content(rng, kind, m, n, V):
    """(target, prediction) id lists of the lengths m, n."""
    if kind == "identical":
        r = rng.integers(0, V, max(m, n)).tolist()
        return r[:m], r[:n]
    if kind == "disjoint":
        half = max(V // 2, 1)
        return rng.integers(0, half, m).tolist(), (rng.integers(0, max(V - half, 1), n) + half).tolist()
    if kind == "shifted":
        r = rng.integers(0, min(V, 5), max(m, n) + 1).tolist()
        return r[:m], r[1:n + 1]
    if kind == "two tokens":
        return rng.integers(0, 2, m).tolist(), rng.integers(0, 2, n).tolist()
    if kind == "outside":                                   # a few ids >= V and < 0 inside the length, and the id V - 1
        r, p = rng.integers(0, V, m), rng.integers(0, V, n)
        for s in (r, p):
            if len(s):
                at = rng.integers(0, len(s), max(1, len(s) // 8))
                s[at] = rng.choice(np.array([-1, -5, V, V + 7, V - 1]), size=len(at))
        return r.tolist(), p.tolist()
    raise KeyError(kind)


KINDS = ("identical", "disjoint", "shifted", "two tokens", "outside")


def _pack(pairs, ps, ts, V):
    """[(r, p)] -> (p_ids (P, ps), p_len, t_ids (P, ts), t_len) numpy, the rows filled with -1 / V + 7 behind the lengths."""
    P = len(pairs)
    fill = np.where(np.arange(max(ps, ts)) % 2 == 0, -1, V + 7).astype(np.int32)
    p_ids, t_ids = np.tile(fill[:ps], (P, 1)), np.tile(fill[:ts], (P, 1))
    p_len, t_len = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    for k, (r, p) in enumerate(pairs):
        t_ids[k, :len(r)], p_ids[k, :len(p)] = r, p
        t_len[k], p_len[k] = len(r), len(p)
    return p_ids, p_len, t_ids, t_len


def _partners(L, cap):
    return (L, L // 2, min(L + L // 3 + 1, cap))            # equal, shorter, longer


def _border_pairs(rng, lengths, cap, V):
    pairs, k = [], 0
    for L in lengths:
        for other in _partners(L, cap):
            for m, n in ((L, other), (other, L)):
                pairs.append(_content(rng, KINDS[k % len(KINDS)], m, n, V))
                k += 1
    return pairs


def _batches():
    """{name: (pairs, pred_stride, target_stride, V)}"""
    rng = np.random.default_rng(2024)
    out = {}
    out["empty and short"] = ([([], []), ([], [0, 1, 2, 1, 0]), ([0, 1, 2, 1, 0], []), ([1], [1]), ([1], [0]), ([2], [0, 2, 1])],
                              8, 8, 3)
    out["one pair"] = ([_content(rng, "two tokens", 9, 7, 3)], 16, 12, 3)
    out["three pairs"] = ([_content(rng, k, 40, 33, 500) for k in ("shifted", "outside", "disjoint")], 64, 64, 500)
    out["257 pairs"] = ([_content(rng, KINDS[k % 5], int(rng.integers(0, 17)), int(rng.integers(0, 17)), 3) for k in range(257)],
                        16, 16, 3)
    out["one block"] = (_border_pairs(rng, (1, 63, 64), 64, 500), 64, 64, 500)
    out["LDS, four blocks"] = (_border_pairs(rng, (65, 127, 128, 129, 255, 256), 256, 500), 256, 256, 500)
    out["three blocks, unequal strides"] = (_border_pairs(rng, (129, 150), 160, 2048), 160, 192, 2048)
    out["scratch, just past LDS"] = (_border_pairs(rng, (256, 257), 272, 500), 272, 272, 500)
    out["scratch, 1024"] = ([_content(rng, "two tokens", 1024, 1024, 3), _content(rng, "outside", 1024, 513, 3),
                             _content(rng, "shifted", 513, 1024, 3)], 1024, 1024, 3)
    out["long predictions, short targets"] = ([_content(rng, "shifted", 60, 1000, 500), _content(rng, "two tokens", 64, 300, 500)],
                                              1024, 64, 500)
    out["short predictions, long targets"] = ([_content(rng, "outside", 1000, 60, 500), _content(rng, "two tokens", 700, 64, 500)],
                                              64, 1024, 500)
    return out


BATCHES = _batches()
_REFERENCE = {}


def reference(name):
    """The restatement's answer for a batch, computed once."""
    if name not in _REFERENCE:
        pairs, ps, ts, V = BATCHES[name]
        packed = _pack(pairs, ps, ts, V)
        _REFERENCE[name] = (packed, R.align_batch(*packed, V, table=R.table_fast))
    return _REFERENCE[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _unsigned(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(BATCHES))
def test_alignment_is_the_restatements(name):
    pairs, ps, ts, V = BATCHES[name]
    (p_ids, p_len, t_ids, t_len), (want_ops, want_scripts, want_C) = reference(name)
    d = [_dev(x) for x in (p_ids, p_len, t_ids, t_len)]
    C = torch.zeros((V + 1, V + 1), dtype=torch.int32, device=DEV)
    got = M.device_edit_alignment(*d, V, C, want_ops=True, want_script=True)
    ops, script, slen = got["ops"].cpu().numpy(), got["script"].cpu().numpy(), got["script_len"].cpu().numpy()
    assert script.shape == (len(pairs), ps + ts)
    assert np.array_equal(ops, want_ops)
    assert slen.tolist() == [len(s) for s in want_scripts]
    for k, s in enumerate(want_scripts):
        assert script[k, :len(s)].tolist() == s, (name, k)
    assert np.array_equal(_unsigned(C), want_C)
    assert _unsigned(C)[V, V] == 0
    # the distance of the script is the one the statistics kernel already returns
    width = max(ps, ts)
    wide = lambda a: np.pad(a, ((0, 0), (0, width - a.shape[1])))
    st = M.device_sequence_statistics(_dev(wide(p_ids)), d[1], _dev(wide(t_ids)), d[3], _max_len=width)
    assert np.array_equal(st["lev"].numpy(), ops[:, 1:].sum(axis=1))
    # every output alone, and a second call into the same matrix
    only = M.device_edit_alignment(*d, V, None, want_ops=True)
    assert set(only) == {"ops"} and np.array_equal(only["ops"].cpu().numpy(), want_ops)
    only = M.device_edit_alignment(*d, V, None, want_ops=False, want_script=True)
    assert set(only) == {"script", "script_len"} and np.array_equal(only["script_len"].cpu().numpy(), slen)
    assert M.device_edit_alignment(*d, V, C, want_ops=False) == {}
    assert np.array_equal(_unsigned(C), 2 * want_C)


def test_two_batches_into_one_matrix():
    V = 500
    C = torch.zeros((V + 1, V + 1), dtype=torch.int32, device=DEV)
    total = np.zeros((V + 1, V + 1), dtype=np.uint32)
    for name in ("three pairs", "one block", "LDS, four blocks"):
        packed, (_, _, want_C) = reference(name)
        M.device_edit_alignment(*[_dev(x) for x in packed], V, C, want_ops=False)
        total += want_C
    assert np.array_equal(_unsigned(C), total)


def test_lengths_are_clamped_to_the_strides():
    V = 7
    p_ids, p_len, t_ids, t_len = _pack([([1, 2, 3, 4], [1, 2, 9, 4, 5, 6]), ([0, 1], [0])], 6, 4, V)
    p_len[0], t_len[0], p_len[1], t_len[1] = 50, 2000000000, -3, -1
    want_ops, want_scripts, want_C = R.align_batch(p_ids, p_len, t_ids, t_len, V)
    C = torch.zeros((V + 1, V + 1), dtype=torch.int32, device=DEV)
    got = M.device_edit_alignment(*[_dev(x) for x in (p_ids, p_len, t_ids, t_len)], V, C, want_script=True)
    assert np.array_equal(got["ops"].cpu().numpy(), want_ops) and want_ops[1].tolist() == [0, 0, 0, 0]
    assert got["script_len"].cpu().tolist() == [len(s) for s in want_scripts]
    assert np.array_equal(_unsigned(C), want_C)


def test_list_entry_point():
    preds, tgts = [[5, 6, 7], [], [1, 1, 2]], [[5, 7], [3], [1, 2, 2]]
    out = M.edit_alignment(preds, tgts, 10, want_script=True)
    assert out["script"] == [R.script(t, p) for p, t in zip(preds, tgts)]
    assert out["ops"].tolist() == [R.counts(s) for s in out["script"]]
    assert int(_unsigned(out["confusion"]).sum()) == sum(len(s) for s in out["script"])
    assert M.edit_alignment([], [], 10)["ops"].shape == (0, 4)


def test_refusals_with_real_buffers():
    L = _lib.lib()
    ids = torch.zeros((2, 1100), dtype=torch.int32, device=DEV)
    lens = torch.zeros((2,), dtype=torch.int32, device=DEV)
    ops = torch.full((2, 4), -7, dtype=torch.int32, device=DEV)
    big = torch.empty((L.i2l_edit_alignment_scratch_bytes(2, 1024, 1024),), dtype=torch.uint8, device=DEV)
    call = lambda ps, ts, V, nbytes: L.i2l_edit_alignment(ids.data_ptr(), lens.data_ptr(), ps, ids.data_ptr(), lens.data_ptr(), ts,
                                                         2, V, big.data_ptr(), nbytes, ops.data_ptr(), None, None, None,
                                                         _lib.stream_ptr())
    assert call(1025, 64, 10, big.numel()) == -2
    assert call(64, 64, 2049, big.numel()) == -2
    assert call(1024, 1024, 10, big.numel() - 1) == -3
    torch.cuda.synchronize()
    assert (ops.cpu() == -7).all()                          # nothing was launched
    assert call(1024, 1024, 10, big.numel()) == 0
    torch.cuda.synchronize()
    assert (ops.cpu() == 0).all()


# ------------------------------------------------------------------------------------------------ margins and top cells
def _matrices():
    rng = np.random.default_rng(99)
    out = {}
    C = rng.integers(0, 4, (38, 38)).astype(np.uint32)      # V = 37: small counts, ties everywhere
    C[37, 37] = 0
    out["ties"] = C
    out["zero"] = np.zeros((38, 38), dtype=np.uint32)
    C = np.zeros((2049, 2049), dtype=np.uint32)             # V = 2048: sparse, more non-zero cells than the longest list
    at = rng.integers(0, 2049, (6000, 2))
    C[at[:, 0], at[:, 1]] = rng.integers(1, 40, 6000)
    C[np.arange(0, 2048, 3), np.arange(0, 2048, 3)] = 1000
    C[5, 9] = 3000000000                                    # above 2^31: the counts are unsigned
    C[2048, 2048] = 0
    out["sparse 2048"] = C
    C = (rng.integers(1, 6, (201, 201))).astype(np.uint32)  # V = 200: every cell non-zero, a merge at every pass
    C[200, 200] = 0
    out["dense 200"] = C
    return out


MATRICES = _matrices()


def _kind_mask(V):
    k = np.full((V + 1, V + 1), M.KIND_SUBSTITUTIONS, dtype=np.int64)
    k[np.arange(V), np.arange(V)] = M.KIND_MATCHES
    k[:, V] = M.KIND_DELETIONS
    k[V, :] = M.KIND_INSERTIONS
    k[V, V] = 0
    return k


def _top_ref(C, kinds, n):
    V = C.shape[0] - 1
    rows, cols = np.nonzero((C > 0) & ((_kind_mask(V) & kinds) != 0))
    counts = C[rows, cols].astype(np.int64)
    order = np.lexsort((cols, rows, -counts))[:n]
    return list(zip(rows[order].tolist(), cols[order].tolist(), counts[order].tolist()))


@pytest.mark.parametrize("name", list(MATRICES))
def test_margins(name):
    C = MATRICES[name]
    V = C.shape[0] - 1
    row, col, diag = M.confusion_margins(_dev(C.view(np.int32)))
    wide = C.astype(np.uint64)
    assert np.array_equal(_unsigned(row), wide.sum(axis=1).astype(np.uint32))
    assert np.array_equal(_unsigned(col), wide.sum(axis=0).astype(np.uint32))
    assert np.array_equal(_unsigned(diag), np.diag(C)[:V])


@pytest.mark.parametrize("name,masks,ns", [("ties", tuple(range(1, 16)), (1, 5, 1024)), ("zero", (1, 15), (1, 1024)),
                                           ("sparse 2048", (1, 2, 8, 15), (1, 20, 1024)), ("dense 200", (1, 15), (7, 1024))])
def test_top_cells(name, masks, ns):
    C = MATRICES[name]
    dC = _dev(C.view(np.int32))
    for kinds in masks:
        for n in ns:
            assert M.confusion_top(dC, kinds, n) == _top_ref(C, kinds, n), (name, kinds, n)
    if name == "ties":                                      # n above the number of non-zero cells: all of them, in order
        assert len(M.confusion_top(dC, M.KIND_INSERTIONS, 1024)) == int((C[37, :37] > 0).sum()) < 1024
    if name == "sparse 2048":
        assert M.confusion_top(dC, 15, 1)[0] == (5, 9, 3000000000)


# ------------------------------------------------------------------------------------------------ the public path
def _own_matrix(out, tgt, V):
    """edit_alignment on a result's own returned ids against the targets without PAD."""
    rows, lens = out["pred_ids"].cpu().tolist(), out["pred_len"].cpu().tolist()
    preds = [r[:n] for r, n in zip(rows, lens)]
    targets = [[v for v in row if v != PAD] for row in tgt.cpu().tolist()]
    got = M.edit_alignment(preds, targets, V)
    return _unsigned(got["confusion"]), got["ops"].numpy()


@pytest.fixture(scope="module")
def second_checkpoint(tmp_path_factory):
    """The fixture checkpoint with seeded noise on its decoder's weights: same vocabulary, another model."""
    ck = torch.load(PT, map_location="cpu", weights_only=False)
    g = torch.Generator().manual_seed(77)
    for k, v in ck["model_state_dict"].items():
        if k.startswith("decoder.") and v.dtype == torch.float32:
            ck["model_state_dict"][k] = v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g)
    path = str(tmp_path_factory.mktemp("edit_align") / "second.pt")
    torch.save(ck, path)
    return path


def test_evaluate_with_errors(second_checkpoint):
    from img2latex_amd.training import Predictor
    dev, T = torch.device(DEV), 40
    single = Predictor.from_checkpoint(PT, device=dev)
    V = single.tokenizer.vocab_size
    x = torch.cat([single._prepare_image(PNG)] * 3)
    x[1] = x[1].flip(-1)                                    # three different pages
    x[2] = x[2].roll(37, -1)
    tgt = torch.tensor([[START, 5, 6, 7, 8, END, PAD, PAD], [START, 9, 5, END, PAD, PAD, PAD, PAD],
                        [START, 6, 6, 6, 7, 9, 8, END]], dtype=torch.int32, device=DEV)
    for predictor in (single, Predictor.from_checkpoints([PT, second_checkpoint], device=dev)):
        plain = predictor.evaluate_batch(x, tgt, max_length=T, return_statistics=True)
        errors = M.ErrorAnalysis(V, dev)
        out = predictor.evaluate_batch(x, tgt, max_length=T, return_statistics=True, errors=errors)
        assert (out["bleu"], out["levenshtein"]) == (plain["bleu"], plain["levenshtein"])
        assert torch.equal(out["statistics"], plain["statistics"]) and torch.equal(out["pred_ids"], plain["pred_ids"])
        want_C, want_ops = _own_matrix(out, tgt, V)
        assert np.array_equal(_unsigned(errors.confusion), want_C)
        assert errors.distances == out["statistics"][:, 0].tolist() == want_ops[:, 1:].sum(axis=1).tolist()
        rep = errors.report(predictor.tokenizer, top=5)
        ops = rep["operations"]
        assert [ops[k] for k in ("match", "substitution", "deletion", "insertion")] == want_ops.sum(axis=0).tolist()
        assert ops["substitution"] + ops["deletion"] + ops["insertion"] == rep["edit_distance_total"] == sum(errors.distances)
        row, col, diag = want_C.sum(1), want_C.sum(0), np.diag(want_C)[:V]
        by_ids = M.build_report(V, row.tolist(), col.tolist(), diag.tolist(), _top_ref(want_C, M.KIND_SUBSTITUTIONS, 5),
                                _top_ref(want_C, M.KIND_DELETIONS, 5), _top_ref(want_C, M.KIND_INSERTIONS, 5),
                                errors.distances, predictor.tokenizer)
        assert rep == by_ids
    # the look-ahead pipeline: two batches, one matrix
    errors = M.ErrorAnalysis(V, dev)
    batches = [(x, tgt), (x.flip(0), tgt)]
    plain = list(single.evaluate_stream(iter(batches), max_length=T, return_statistics=True))
    outs = list(single.evaluate_stream(iter(batches), max_length=T, return_statistics=True, errors=errors))
    total = np.zeros((V + 1, V + 1), dtype=np.uint32)
    for o, q, (_, t) in zip(outs, plain, batches):
        assert (o["bleu"], o["levenshtein"]) == (q["bleu"], q["levenshtein"]) and torch.equal(o["statistics"], q["statistics"])
        total += _own_matrix(o, t, V)[0]
    assert np.array_equal(_unsigned(errors.confusion), total)
    assert errors.distances == torch.cat([o["statistics"][:, 0] for o in outs]).tolist()
    # a batch taken out again leaves the matrix of the other
    o = outs[1]
    t_ids = [[v for v in row if v != PAD] for row in tgt.cpu().tolist()]
    width = o["pred_ids"].shape[1]
    t_pad = torch.tensor([r + [0] * (width - len(r)) for r in t_ids], dtype=torch.int32, device=DEV)
    t_len = torch.tensor([len(r) for r in t_ids], dtype=torch.int32, device=DEV)
    errors.retract(o["pred_ids"], o["pred_len"], t_pad, t_len)
    assert np.array_equal(_unsigned(errors.confusion), _own_matrix(outs[0], tgt, V)[0])


def test_cli_evaluate_errors(tmp_path, capsys):
    from img2latex_amd import cli
    ck_dir = tmp_path / "outputs" / "tiny_exp" / "checkpoints"
    os.makedirs(ck_dir)
    shutil.copyfile(PT, ck_dir / "ck.pt")
    args = ["evaluate", str(ck_dir / "ck.pt"), os.path.join(GOLDEN, "dataset_tiny"), "--batch-size", "5", "--device", "cuda"]
    assert cli.main(args + ["--output-dir", str(tmp_path / "plain")]) == 0
    said_plain = capsys.readouterr().out
    assert cli.main(args + ["--output-dir", str(tmp_path / "out"), "--errors", "--errors-top", "4"]) == 0
    said = capsys.readouterr().out
    lines = lambda s: [l for l in s.splitlines() if l.startswith(("BLEU", "Levenshtein", "Number"))]
    assert lines(said) == lines(said_plain) and len(lines(said)) == 3
    pred_dir = tmp_path / "out" / "tiny_exp" / "predictions"
    assert sorted(os.listdir(pred_dir)) == ["error_analysis.json", "error_analysis_report.md", "predictions.json"]
    assert sorted(os.listdir(tmp_path / "plain" / "tiny_exp" / "predictions")) == ["predictions.json"]
    assert (pred_dir / "predictions.json").read_text() == (tmp_path / "plain" / "tiny_exp" / "predictions" / "predictions.json").read_text()
    rep = json.loads((pred_dir / "error_analysis.json").read_text())
    ops = rep["operations"]
    assert rep["pairs"] == len(json.loads((pred_dir / "predictions.json").read_text())) > 0
    assert ops["substitution"] + ops["deletion"] + ops["insertion"] == rep["edit_distance_total"]
    assert sum(b["count"] for b in rep["distance_buckets"]) == rep["pairs"]
    assert len(rep["top_substitutions"]) <= 4 and all(isinstance(e["target"], str) for e in rep["top_deletions"])
    md = (pred_dir / "error_analysis_report.md").read_text()
    assert "## Top substitutions" in md and "counted in tokens" in md
