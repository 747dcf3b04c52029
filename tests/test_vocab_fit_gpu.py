"""i2l_vocab_fit (packed UTF-8 text -> the fitted vocabulary on the device) through the C ABI, and the layers on top of it:
fit_vocabulary, TokenTable.fit / fit_on_formulas_file, the ``vocab`` command.  Every comparison is exact equality with
the REFERENCE's results (tests/golden/vocab_fit.npz, tokenize.npz); there is no tolerance anywhere."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd.training import (TokenTable, detokenize_table, fit_vocabulary, pack_texts, split_lines, tokenize_table)
from img2latex_amd.training import vocab as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SPECIAL = ["<PAD>", "<START>", "<END>", "<UNK>"]
GUARD = 0xA5
_CACHE = {}


def golden():
    if "npz" not in _CACHE:
        _CACHE["npz"] = np.load(os.path.join(GOLDEN, "vocab_fit.npz"))
    return _CACHE["npz"]


def unpack(raw, off):
    raw = np.asarray(raw).tobytes()
    return [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]


def expected(case):
    """The reference's result for a case, computed once: (data, off, tokens behind the special ones, their counts, their
    first byte offsets in the corpus, the special strings' counts, total tokens, longest row)."""
    if case in _CACHE:
        return _CACHE[case]
    d = golden()
    data = d[f"{case}_bytes"]
    off = split_lines(data) if case == "e" else d[f"{case}_off"]
    texts = unpack(data, off)
    vocab = unpack(d[f"{case}_tok_bytes"], d[f"{case}_tok_off"])
    counts = d[f"{case}_counts"].copy()
    longest = int(d[f"{case}_longest"])
    if case == "e":                                                  # the file's rows carry no START / END of their own
        counts[1] -= len(texts)
        counts[2] -= len(texts)
        longest -= 2
    assert vocab[:4] == SPECIAL
    first, pos = {}, 0                                               # first byte offset of every token
    for text in texts:
        byte, last = pos, 0
        found = []
        for m in re.finditer(r"\S+", text):
            byte += len(text[last:m.start()].encode("utf-8"))
            first.setdefault(m.group(), byte)
            found.append(m.group())
            byte += len(m.group().encode("utf-8"))
            last = m.end()
        assert found == text.split()
        pos += len(text.encode("utf-8"))
    _CACHE[case] = (data, off, vocab[4:], counts[4:].tolist(), [first[t] for t in vocab[4:]], counts[:4].tolist(),
                    int(counts.sum()), longest)
    return _CACHE[case]


def run(data, off, slots, skip=SPECIAL, out_cap=None, byte_cap=None, flags=0):
    """The C call -> (rc, meta, tokens, counts, firsts, raw output arrays with their guard words)."""
    L = _lib.lib()
    rows = off.size - 1
    out_cap = slots // 2 if out_cap is None else out_cap
    byte_cap = int(data.size) if byte_cap is None else byte_cap
    text = torch.from_numpy(np.concatenate([np.asarray(data, np.uint8), np.zeros(1, np.uint8)])).to(DEV)
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int32)).to(DEV)
    out_bytes = torch.full((byte_cap + 64,), GUARD, dtype=torch.uint8, device=DEV)
    ints = torch.full((3, out_cap + 1 + 16), -77, dtype=torch.int32, device=DEV)      # off / count / first, guards behind
    meta = torch.full((V.META_WORDS + 4,), -77, dtype=torch.int32, device=DEV)
    ws = torch.empty((L.i2l_vocab_fit_workspace_bytes(rows, slots),), dtype=torch.uint8, device=DEV)
    skip_b = [s.encode("utf-8") for s in skip]
    skip_bytes = np.frombuffer(b"".join(skip_b) + b"\0", dtype=np.uint8)
    skip_off = np.zeros(len(skip_b) + 1, np.int32)
    np.cumsum([len(s) for s in skip_b], out=skip_off[1:])
    torch.cuda.synchronize()
    rc = L.i2l_vocab_fit(text.data_ptr(), int(data.size), d_off.data_ptr(), rows, skip_bytes.ctypes.data, skip_off.ctypes.data,
                         len(skip_b), slots, flags, out_bytes.data_ptr(), byte_cap, ints[0].data_ptr(), ints[1].data_ptr(),
                         ints[2].data_ptr(), out_cap, meta.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    meta_h, ints_h, bytes_h = meta.cpu().numpy(), ints.cpu().numpy(), out_bytes.cpu().numpy()
    assert np.all(meta_h[V.META_WORDS:] == -77) and np.all(bytes_h[byte_cap:] == GUARD)
    assert np.all(ints_h[0, out_cap + 1:] == -77) and np.all(ints_h[1:, out_cap:] == -77)
    n = min(int(meta_h[0]), out_cap)
    o = ints_h[0, :n + 1]
    raw = bytes_h[:byte_cap].tobytes()
    tokens = [raw[a:b] for a, b in zip(o[:-1], o[1:])]
    return rc, meta_h[:V.META_WORDS].tolist(), tokens, ints_h[1, :n].tolist(), ints_h[2, :n].tolist(), (ints_h, bytes_h)


@pytest.mark.parametrize("case", ("a", "b", "c", "d1", "d2", "e"))
def test_golden_cases_through_the_abi(case):
    data, off, want_tokens, want_counts, want_first, want_special, want_total, want_longest = expected(case)
    slots = 1 << 14                                                  # case b: 5200 distinct tokens, a sort of 8192
    results = [run(data, off, slots), run(data, off, slots), run(data, off, slots, flags=V.NO_AGGREGATE)]
    rc, meta, tokens, counts, firsts, raw = results[0]
    assert rc == 0 and meta[5] == 0, meta
    assert [t.decode("utf-8") for t in tokens] == want_tokens
    assert counts == want_counts and firsts == want_first
    assert meta[0] == len(want_tokens) and meta[1] == sum(1 for c in want_special if c) and meta[2] == want_total
    assert meta[3] == want_longest and meta[4] == sum(len(t) for t in tokens) and meta[6:8] == [0, 0]
    assert meta[8:12] == want_special and meta[12:] == [0, 0, 0, 0]
    for other in results[1:]:                                        # bit-identical from run to run, with or without LDS tables
        assert other[0] == 0 and other[1] == meta
        n = meta[0]
        assert np.array_equal(other[5][0][:, :n + 1], raw[0][:, :n + 1]) and np.array_equal(other[5][1][:meta[4]], raw[1][:meta[4]])


def test_full_table_is_reported_and_retried():
    data, off, want_tokens, want_counts, _, _, want_total, want_longest = expected("b")
    rc, meta, _, _, _, _ = run(data, off, 1024)
    assert rc == 0 and meta[5] & V.STATUS_FULL and meta[2] == want_total and meta[3] == want_longest
    rc, meta, _, _, _, _ = run(data, off, 8192)                      # 5200 distinct tokens > 8192 / 2: every probe finds a slot
    assert rc == 0 and meta[5] & V.STATUS_FULL
    fitted = fit_vocabulary((data, off), device=DEV, slots=1024)
    assert list(fitted.token_to_id) == SPECIAL + want_tokens and list(fitted.token_to_id.values()) == list(range(4 + len(want_tokens)))
    assert fitted.counts[4:].tolist() == want_counts and fitted.total_tokens == want_total and fitted.longest_row == want_longest


def test_short_output_buffers():
    data, off, want_tokens, want_counts, want_first, _, _, _ = expected("c")
    need = sum(len(t.encode("utf-8")) for t in want_tokens)
    rc, meta, tokens, counts, firsts, _ = run(data, off, 1 << 12, byte_cap=need - 301)     # run() checks the guard bytes
    assert rc == 0 and meta[5] == V.STATUS_OUT_TOO_SMALL and meta[0] == len(want_tokens) and meta[4] == need
    assert counts == want_counts and firsts == want_first
    whole = [t.decode("utf-8") for t, w in zip(tokens, want_tokens) if len(t) == len(w.encode("utf-8"))]
    assert whole == want_tokens[:len(whole)] and len(whole) > 100    # everything in front of the cut is right
    rc, meta, tokens, counts, firsts, _ = run(data, off, 1 << 12, out_cap=100)
    assert rc == 0 and meta[5] == V.STATUS_OUT_TOO_SMALL and meta[0] == len(want_tokens) and meta[4] == need
    assert [t.decode("utf-8") for t in tokens] == want_tokens[:100] and counts == want_counts[:100] and firsts == want_first[:100]
    rc, meta, tokens, _, _, _ = run(data, off, 1 << 12, byte_cap=need, out_cap=len(want_tokens))   # exactly enough
    assert rc == 0 and meta[5] == 0 and [t.decode("utf-8") for t in tokens] == want_tokens
    rc, meta, tokens, _, _, _ = run(data, off, 1 << 12, byte_cap=0, out_cap=0)
    assert rc == 0 and meta[5] == V.STATUS_OUT_TOO_SMALL and meta[0] == len(want_tokens) and tokens == []


def test_bad_offsets_make_an_empty_row():
    texts = ["a b a", "c c c c c c", "b a d", "e e"]
    data, off = pack_texts(texts)                                    # offsets 0 5 16 21 24
    backwards, beyond = off.copy(), off.copy()
    backwards[2] = 3                                                 # row 1 = [5, 3): empty; row 2 = [3, 21) starts early
    beyond[4] = data.size + 5                                        # row 3 ends behind the text
    for bad, rows in ((backwards, ["a b a", "", " a" + "c c c c c c" + "b a d", "e e"]), (beyond, texts[:3] + [""])):
        rc, meta, tokens, counts, _, _ = run(data, bad, 1 << 10)
        assert rc == 0 and meta[5] == V.STATUS_BAD_OFFSETS
        want = {}
        for r in rows:
            for t in r.split():
                want[t] = want.get(t, 0) + 1
        assert dict(zip([t.decode() for t in tokens], counts)) == want and meta[2] == sum(want.values())
        assert meta[3] == max(len(r.split()) for r in rows)
        with pytest.raises(ValueError, match="offsets"):
            fit_vocabulary((data, bad), device=DEV)


def test_token_table_fit():
    data, off, want_tokens, want_counts, _, want_special, want_total, want_longest = expected("a")
    texts = unpack(data, off)
    table = TokenTable({"<PAD>": 3, "<START>": 2, "<END>": 1, "<UNK>": 0, "old": 4}, max_sequence_length=want_longest)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                               # the longest row fits: no warning
        fitted = table.fit(texts, device=DEV)
    want = {t: i for i, t in enumerate(SPECIAL + want_tokens)}
    assert table.token_to_id == want and list(table.token_to_id) == list(want)
    assert table.id_to_token == {i: t for t, i in want.items()} and table.vocab_size == len(want)
    assert (table.pad_token_id, table.start_token_id, table.end_token_id, table.unk_token_id) == (0, 1, 2, 3)
    assert fitted.token_to_id == want and fitted.counts.tolist() == want_special + want_counts
    assert fitted.total_tokens == want_total and fitted.longest_row == want_longest
    freq = {}
    for t in texts:
        for w in t.split():
            freq[w] = freq.get(w, 0) + 1
    assert fitted.frequencies() == freq
    table.max_sequence_length = want_longest - 1
    with pytest.warns(UserWarning, match=f"Found sequences of length {want_longest}"):
        table.fit(texts, device=DEV)
    old = np.load(os.path.join(GOLDEN, "tokenize.npz"))
    assert list(table.token_to_id) == [str(t) for t in old["tokens"]]


def test_token_table_fit_on_formulas_file(tmp_path):
    d = golden()
    for case, raw in (("e", d["e_bytes"].tobytes()), ("a", ("\n".join(unpack(*expected("a")[:2])) + "\n").encode("utf-8"))):
        path = tmp_path / f"{case}.lst"
        path.write_bytes(raw)
        want = unpack(d[f"{case}_tok_bytes"], d[f"{case}_tok_off"])
        longest = int(d[f"{case}_longest"]) + (2 if case == "a" else 0)              # e's is per wrapped line already
        table = TokenTable(max_sequence_length=longest - 1)
        with pytest.warns(UserWarning, match=f"Found sequences of length {longest},"):
            fitted = table.fit_on_formulas_file(str(path), device=DEV)
        assert list(table.token_to_id) == want and list(table.token_to_id.values()) == list(range(len(want)))
        assert table.vocab_size == len(want) and fitted.longest_row == longest
        assert (table.pad_token_id, table.start_token_id, table.end_token_id, table.unk_token_id) == (0, 1, 2, 3)
        if case == "e":                                              # the reference's Counter, START / END of the wrapping included
            assert fitted.counts.tolist() == d["e_counts"].tolist() and fitted.rows == int(d["e_lines"])
            assert fitted.frequencies() == {t: int(c) for t, c in zip(want, d["e_counts"]) if c}
            assert any(t.startswith("\ufeff\\frac") for t in want)         # the BOM stays part of the first token


def test_round_trip_through_tokenize_and_detokenize():
    old = np.load(os.path.join(GOLDEN, "tokenize.npz"))
    table = TokenTable(max_sequence_length=150)
    table.fit(unpack(*expected("a")[:2]), device=DEV)
    texts = unpack(old["text_bytes"], old["text_off"])
    ids = tokenize_table(table, DEV).encode_batch(texts)
    assert np.array_equal(ids.cpu().numpy(), old["enc_s0_m150"])
    strings, _ = detokenize_table(table, DEV).decode_now(ids, -1)
    assert strings == [table.decode(row) for row in old["enc_s0_m150"].tolist()]


def test_refit_drops_the_cached_device_tables():
    table = TokenTable(max_sequence_length=8)
    table.fit(["a a a b b c"], device=DEV)
    first = tokenize_table(table, DEV)
    assert first.encode_batch(["c b a zz"]).cpu().tolist()[0][:4] == [6, 5, 4, 3]
    assert detokenize_table(table, DEV).decode_now(torch.tensor([[4, 5, 6]], dtype=torch.int32, device=DEV), -1)[0] == ["a b c"]
    table.fit(["zz zz c c c a"], device=DEV)
    assert table.token_to_id == {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3, "c": 4, "zz": 5, "a": 6}
    second = tokenize_table(table, DEV)
    assert second is not first
    assert second.encode_batch(["c b a zz"]).cpu().tolist()[0][:4] == [4, 3, 6, 5]
    assert detokenize_table(table, DEV).decode_now(torch.tensor([[4, 5, 6]], dtype=torch.int32, device=DEV), -1)[0] == ["c zz a"]


def test_vocab_command(tmp_path):
    d = golden()
    src, out = tmp_path / "formulas.lst", tmp_path / "made" / "vocab.pt"
    src.write_bytes(d["e_bytes"].tobytes())
    r = subprocess.run([sys.executable, "-m", "img2latex_amd", "vocab", str(src), str(out), "--max-sequence-length", "33",
                        "--device", "cuda"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=os.path.join(REPO, "hmer-img2latex_amd")))
    assert r.returncode == 0, r.stderr[-2000:]
    saved = torch.load(str(out))
    want = unpack(d["e_tok_bytes"], d["e_tok_off"])
    assert saved == {"token_to_id": {t: i for i, t in enumerate(want)}, "max_sequence_length": 33,
                     "special_tokens": {"PAD": "<PAD>", "START": "<START>", "END": "<END>", "UNK": "<UNK>"}}
    assert list(saved["token_to_id"]) == want
