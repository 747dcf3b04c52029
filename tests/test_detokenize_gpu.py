"""i2l_detokenize (ids -> packed UTF-8 text on the device) through the C ABI, and the layers on top of it: GreedyPipeline's
``detokenize=`` / ``collect_strings``, Predictor.predict_strings_stream, evaluate_batch(return_strings=True).  Every
comparison is exact byte / string equality with the host rule, ``TokenTable.decode`` (tokenizer.py:166-192) of the row
cut before its first stop position (predictor.py:350-358): no tolerance anywhere."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import END, GOLDEN, START, load, model_for
from img2latex_amd import _lib, synth
from img2latex_amd.training import DetokenizeTable, Predictor, TokenTable, detokenize_table, token_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAP = 20                                                             # an id inside the range that is in no map


def synthetic_table():
    """~40 tokens of 0, 1, 2, 3 (non-ASCII), 13, 40 and 300 bytes + the four special tokens; id GAP is missing."""
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3, "": 4}
    words = list("abcdefghij") + ["α", "β", "γ", "δ", "é"] + ["∑", "∫", "→", "≤", "∞"] + \
        ["\\operatorname", "\\longleftarrow", "\\mathfrak{abc}"[:13]] + ["\\" + "x" * 39, "\\" + "y" * 39] + ["{" + "z" * 298 + "}"]
    words += [f"w{i}" for i in range(12)]
    v = 5
    for w in words:
        if v == GAP:
            v += 1
        vocab[w] = v
        v += 1
    tok = TokenTable(vocab)
    lens = sorted({len(t.encode("utf-8")) for t in vocab})
    assert {0, 1, 2, 3, 13, 40, 300} <= set(lens) and GAP not in tok.id_to_token and max(tok.id_to_token) > GAP
    return tok


TOK = synthetic_table()
VOCAB = max(TOK.id_to_token) + 1
_CASES = {}


def make_ids(rows, width):
    """Random ids (a few beyond the vocabulary, END among them) with the edge rows planted, as many as the shape has rows."""
    rng = np.random.default_rng(rows * 1000 + width)
    a = rng.integers(0, VOCAB + 3, size=(rows, width)).astype(np.int32)
    plain = np.array([v for v in TOK.id_to_token if v > 4], dtype=np.int32)
    cyc = lambda vals: np.array(vals, dtype=np.int64)[np.arange(width) % len(vals)]
    some = lambda: plain[rng.integers(0, plain.size, width)]
    mid = width // 2
    planted = []
    r = a[0].copy(); r[0] = END; planted.append(r)                                      # END at position 0
    planted.append(some())                                                              # no END at all
    r = some(); r[mid:] = -1; planted.append(r)                                         # a -1 filler tail
    planted.append(cyc([0, 1, 3, 3, 0, 1]))                                             # only special ids
    planted.append(cyc([VOCAB, 7, VOCAB + 5, 10000, 2 ** 31 - 1, 9]))                   # ids >= vocab
    planted.append(cyc([GAP, 6, GAP, GAP]))                                             # the gap in the id map
    r = some(); r[0] = 4; r[mid:mid + 2] = 4; r[max(width - 2, 0)] = 4; r[width - 1] = END
    planted.append(r)                                                                   # "" first, doubled, last before END
    planted.append(cyc([4]))                                                            # nothing but "": separators only
    step = 7 if rows >= 7 * len(planted) else 1
    for i, r in enumerate(planted[:rows]):
        a[i * step] = r
    return a


def host_rule(a, end_id, skip_special):
    """TokenTable.decode of every row cut before its first stop position -> (bytes, offsets)."""
    rows = []
    for r in a.tolist():
        n = next((i for i, v in enumerate(r) if v < 0 or v == end_id), len(r))
        rows.append(TOK.decode(r[:n], skip_special_tokens=skip_special).encode("utf-8"))
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in rows], out=off[1:])
    return b"".join(rows), off


def case(rows, width):
    if (rows, width) not in _CASES:
        a = make_ids(rows, width)
        _CASES[(rows, width)] = (a, host_rule(a, END, True), host_rule(a, END, False))
    return _CASES[(rows, width)]


def table():
    t = detokenize_table(TOK, DEV)
    assert t is detokenize_table(TOK, DEV) and t.vocab == VOCAB and t.longest == 300       # built once per (tokenizer, device)
    return t


def run(t, ids, width, capacity, n_drop, end_id=END, guard=64, rows=None, vocab=None, stride=None):
    rows = ids.shape[0] if rows is None else rows
    stride = ids.stride(0) if stride is None else stride
    out = torch.full((max(capacity, 0) + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    off = torch.full((rows + 1 if rows < 1 << 16 else 4,), 77, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    L = _lib.lib()
    ws = torch.empty((L.i2l_detokenize_workspace_bytes(min(rows, 1 << 16)),), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = L.i2l_detokenize(ids.data_ptr(), rows, width, stride, end_id, t.drop.data_ptr(), n_drop, t.tok_bytes.data_ptr(),
                          t.tok_off.data_ptr(), t.vocab if vocab is None else vocab, t.unk_id, out.data_ptr(), capacity,
                          off.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), off.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("rows,width,stride", [(1, 1, 1), (3, 64, 64), (3, 65, 65), (67, 150, 160), (2500, 3, 3), (256, 150, 150)],
                         ids=["1x1", "3x64", "3x65", "67x150_stride160", "2500x3", "256x150"])
def test_bytes_and_offsets_equal_the_host_rule(rows, width, stride):
    a, with_drop, no_drop = case(rows, width)
    t = table()
    dev = torch.full((rows, stride), 7, dtype=torch.int32, device=DEV)                  # the padding would be kept if read
    dev[:, :width] = torch.from_numpy(a).to(DEV)
    ids = dev[:, :width]
    for n_drop, (want, want_off) in ((t.n_drop, with_drop), (0, no_drop)):
        total = int(want_off[-1])
        rc, out, off, status = run(t, ids, width, total + 100, n_drop)
        assert rc == 0 and status == 0
        assert np.array_equal(off, want_off), (n_drop, off[:8], want_off[:8])
        assert out[:total].tobytes() == want
        assert bool((out[total:] == 0xA5).all())                                        # nothing behind the last row
    assert with_drop[0] != no_drop[0] or rows <= 8          # (up to 8 rows every row is a planted one; three hold no special id)


def test_negative_one_as_end_id_stops_at_negative_ids_only():
    a, _, _ = case(67, 150)
    want, want_off = host_rule(a, -1, True)
    rc, out, off, status = run(table(), torch.from_numpy(a).to(DEV), 150, int(want_off[-1]), table().n_drop, end_id=-1)
    assert rc == 0 and status == 0 and np.array_equal(off, want_off) and out[:int(want_off[-1])].tobytes() == want


def test_capacity():
    a, (want, want_off), _ = case(67, 150)
    t = table()
    ids = torch.from_numpy(a).to(DEV)
    total = int(want_off[-1])
    rc, out, off, status = run(t, ids, 150, total, t.n_drop)                            # exactly what is needed
    assert rc == 0 and status == 0 and np.array_equal(off, want_off) and out[:total].tobytes() == want
    assert bool((out[total:] == 0xA5).all())
    rc, out, off, status = run(t, ids, 150, total - 1, t.n_drop)                        # one byte short
    assert rc == 0 and status == 1
    assert np.array_equal(off, want_off)                                                # the size needed is still reported
    assert out[:total - 1].tobytes() == want[:-1]
    assert out.size == total - 1 + 64 and bool((out[total - 1:] == 0xA5).all())         # the 64-byte guard is intact


def test_refusals_launch_nothing():
    t = table()
    ids = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    untouched = lambda r: r[0] == -2 and bool((r[1] == 0xA5).all()) and bool((r[2] == 77).all()) and r[3] == 77
    assert untouched(run(t, ids, 8, 4096, 9))                                           # n_drop > 8
    assert untouched(run(t, ids, 8, 4096, t.n_drop, vocab=0))
    assert untouched(run(t, ids, 8, 4096, t.n_drop, vocab=-3))
    # rows * width * (longest token + 1) beyond int32 (nothing is launched, so the small `ids` is never read):
    # 2^31 * 301, and the first product past the limit: 2 * 3567249 * 301 = 2^31 + 250
    assert untouched(run(t, ids, 1 << 11, 4096, t.n_drop, rows=1 << 20, stride=1 << 11))
    assert untouched(run(t, ids, 3567249, 4096, t.n_drop, rows=2, stride=3567249))
    assert 2 * 3567249 * 301 == 2 ** 31 + 250 and 1024 * 6967 * 301 < 2 ** 31 - 1
    # just inside it the call runs: 1024 x 6967 PAD ids, every one dropped -> 1024 empty strings
    big = torch.zeros((1024, 6967), dtype=torch.int32, device=DEV)
    rc, out, off, status = run(t, big, 6967, 4096, t.n_drop)
    assert rc == 0 and status == 0 and not off.any() and bool((out == 0xA5).all())


# ---------------------------------------------------------------------------------------------- the layers on top
def tiny():
    d, cfg, _ = load("tiny_l1")
    m, _ = model_for("tiny_l1")
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({(f"τ{i}" if i % 3 else f"\\t{i}"): i for i in range(4, cfg["vocab_size"])})
    return m, cfg, TokenTable(vocab, max_sequence_length=12)


def test_strings_stream_pipeline_and_evaluate_on_a_tiny_model():
    from img2latex_amd.pipeline import GreedyPipeline
    m, cfg, tok = tiny()
    pred = Predictor(m, tok, device=torch.device(DEV))
    x = torch.from_numpy(synth.make_images(20, cfg, seed=1234)).to(DEV)
    batches = [x[i:i + 5] for i in range(0, 20, 5)]
    want = [[tok.decode(seq[1:]) for seq in b] for b in pred.predict_ids_stream(iter(batches), max_length=12)]
    assert len(want) == 4 and any(s for b in want for s in b)
    assert list(pred.predict_strings_stream(iter(batches), max_length=12)) == want
    pipe = GreedyPipeline(m, START, END, 12, rows_per_workgroup=0, decode_flags=_lib.FLAG_DECODE_GROUP16, decode_priority=-1,
                          stop=_lib.STOP_STICKY, select=_lib.SELECT_SOFTMAX, detokenize=detokenize_table(tok, DEV))
    got = []
    for b in batches:
        if pipe.pending() >= pipe.depth:
            got.append(pipe.collect_strings())
        pipe.submit(b)
    while pipe.pending():
        got.append(pipe.collect_strings())
    pipe.close()
    assert got == want
    with pytest.raises(RuntimeError):
        GreedyPipeline(m, START, END, 12).collect_strings()
    # predict_batch's device route: the same strings as decode of predict_batch_ids (greedy and sampling branches)
    pred._prepare_image = lambda im: im.unsqueeze(0)                 # tensors sized for THIS model (as test_hip_parity does)
    for kw in ({"seed": 11}, {"temperature": 0.8, "top_k": 5, "seed": 11}):
        rows = pred.predict_batch_ids(x[:5], max_length=12, **kw)
        assert pred.predict_batch([x[i] for i in range(5)], max_length=12, batch_size=5, **kw) == [tok.decode(r[1:]) for r in rows]
    del pred._prepare_image
    targets = torch.from_numpy(synth.make_formulas(5, 12, cfg["vocab_size"], seed=777, min_len=4)).to(DEV)
    plain = pred.evaluate_batch(batches[1], targets, max_length=12)
    out = pred.evaluate_batch(batches[1], targets, max_length=12, return_strings=True)
    assert "pred_text" not in plain and out["bleu"] == plain["bleu"] and out["levenshtein"] == plain["levenshtein"]
    p_ids, p_len = out["pred_ids"].cpu().tolist(), out["pred_len"].cpu().tolist()
    assert out["pred_text"] == [tok.decode(r[:n]) for r, n in zip(p_ids, p_len)]
    assert any(out["pred_text"])


def test_strings_stream_of_the_reference_checkpoint():
    """Predictor.from_checkpoint(predict_64x800.pt) through predict_strings_stream: the strings the REFERENCE's predict
    gave for the tensor inputs (tests/golden/predict_64x800.npz), each prepared by `_prepare_image` as predict does."""
    sys.path.insert(0, GOLDEN)
    from predict_inputs import inputs
    d = np.load(os.path.join(GOLDEN, "predict_64x800.npz"))
    texts = json.loads(str(d["texts"]))
    pred = Predictor.from_checkpoint(os.path.join(GOLDEN, "predict_64x800.pt"), device=torch.device(DEV))
    cases = inputs()
    names = [n for n in json.loads(str(d["names"])) if n.startswith("tensor_")]
    assert len(names) == 3
    batches = [pred._prepare_image(cases[n]) for n in names]
    got = list(pred.predict_strings_stream(iter(batches), max_length=40))
    assert got == [[texts[n]] for n in names]


def test_strings_after_the_pipeline_fallback():
    """The grouped decode is made to time out the way test_pipeline_falls_back_when_the_grouped_decode_times_out does
    (silent member + short limits): collect_strings() detokenizes the re-run's ids, equal to the host route's."""
    from img2latex_amd.pipeline import GreedyPipeline
    d, cfg, sd_kw = load("primary_cfg2_clock")
    m, _ = model_for("primary_cfg2_clock", sd_kw, cfg)
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, cfg["vocab_size"])})
    tok = TokenTable(vocab, max_sequence_length=150)
    x = torch.from_numpy(synth.make_images(64, cfg, seed=1234)).to(DEV)
    bad = _lib.FLAG_DECODE_GROUP16 | _lib.FLAG_TEST_DROP_MEMBER | _lib.FLAG_TEST_SHORT_TIMEOUT
    host = GreedyPipeline(m, START, END, 60, rows_per_workgroup=0, decode_flags=bad)
    host.submit(x)
    with pytest.warns(RuntimeWarning):
        a = host.collect().numpy()
    want = []
    for r in a.tolist():
        n = next((i for i, v in enumerate(r) if v < 0 or v == END), len(r))
        want.append(tok.decode(r[:n]))
    host.close()
    pipe = GreedyPipeline(m, START, END, 60, rows_per_workgroup=0, decode_flags=bad, detokenize=DetokenizeTable(tok, DEV))
    pipe.submit(x)
    with pytest.warns(RuntimeWarning):
        got = pipe.collect_strings()
    pipe.close()
    assert got == want and any(got)
