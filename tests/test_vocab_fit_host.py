"""The host side of the device vocabulary fit (i2l_vocab_fit): the stored reference results against the Python rule
(``Counter`` over ``str.split()`` + a stable ``sorted``, tokenizer.py:87-104), the numpy line splitter against Python's
text mode, the workspace size query (pure host code, through ctypes), TokenTable's encode / save / load, and the
declarations.  No GPU."""
import ctypes
import os
import re
import warnings
from collections import Counter

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd.training import TokenTable, split_lines

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SPECIAL = ["<PAD>", "<START>", "<END>", "<UNK>"]
CASES = ("a", "b", "c", "d1", "d2")


def golden():
    return np.load(os.path.join(GOLDEN, "vocab_fit.npz"))


def unpack(raw, off):
    raw = np.asarray(raw).tobytes()
    return [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]


def python_rule(texts, special=SPECIAL):
    """(vocabulary in id order, counts aligned with it, total tokens, longest row) -- tokenizer.py:87-107 restated."""
    counter = Counter()
    for text in texts:
        counter.update(text.split())
    vocab = list(special)
    for token, _ in sorted(counter.items(), key=lambda kv: kv[1], reverse=True):
        if token not in special:
            vocab.append(token)
    return vocab, [counter.get(t, 0) for t in vocab], sum(counter.values()), max(len(t.split()) for t in texts)


@pytest.mark.parametrize("case", CASES)
def test_fixture_is_consistent_with_the_python_rule(case):
    d = golden()
    texts = unpack(d[f"{case}_bytes"], d[f"{case}_off"])
    vocab, counts, _, longest = python_rule(texts)
    assert unpack(d[f"{case}_tok_bytes"], d[f"{case}_tok_off"]) == vocab
    assert d[f"{case}_counts"].tolist() == counts and int(d[f"{case}_longest"]) == longest


def test_fixture_holds_the_cases_it_must():
    d = golden()
    a = unpack(d["a_tok_bytes"], d["a_tok_off"])
    old = np.load(os.path.join(GOLDEN, "tokenize.npz"))
    assert a == [str(t) for t in old["tokens"]] and old["token_ids"].tolist() == list(range(len(a)))
    b_counts = d["b_counts"][4:]
    assert (b_counts == 1).sum() == 5000 and (b_counts == 2).sum() == 100 and (b_counts == 3).sum() == 100
    c_texts, c_vocab = unpack(d["c_bytes"], d["c_off"]), unpack(d["c_tok_bytes"], d["c_tok_off"])
    whitespace = [chr(c) for c in range(0x3001) if chr(c).isspace()]
    assert len(whitespace) == 29 and all(any(w in t for t in c_texts) for w in whitespace)
    assert all(any(n in tok for tok in c_vocab) for n in "\u200b\u180e\ufeff")
    assert max(len(t.encode("utf-8")) for t in c_vocab) == 301 and "Q" * 300 in c_vocab and "Q" * 299 + "R" in c_vocab
    assert "" in c_texts and any(t and not t.split() for t in c_texts)
    assert any(x.split() and y.split() and x.split()[-1] == y.split()[0] and x == x.rstrip() and y == y.lstrip()
               for x, y in zip(c_texts, c_texts[1:]))
    assert all(d["c_counts"][i] > 0 for i in range(4)) and {"\\cmd1", "\\cmd11", "\\cmd111", "\\cmd"} <= set(c_vocab)
    assert sum(1 for t in c_vocab if re.fullmatch(r"s\d\d\de", t)) == 300
    # a token straddles every 64-byte chunk boundary of some row, and a 3-byte separator does at 62 and 63
    raw, off = d["c_bytes"].tobytes(), d["c_off"]
    assert any(raw[o + 62:o + 65] == "\u3000".encode() for o in off[:-1]) and any(raw[o + 63:o + 66] == "\u3000".encode() for o in off[:-1])
    for case, rows in (("d1", 4), ("d2", 503)):
        assert d[f"{case}_off"].size - 1 == rows and d[f"{case}_counts"][4] == 50001
        assert unpack(d[f"{case}_tok_bytes"], d[f"{case}_tok_off"])[4] == "{"
    e = d["e_bytes"].tobytes()
    assert e.startswith(b"\xef\xbb\xbf") and b"\r\n" in e and b"\r\r" in e and "\u2028".encode() in e and e[-1:] not in (b"\n", b"\r")


def python_lines(raw, tmp_path):
    path = tmp_path / "formulas.lst"
    path.write_bytes(raw)
    with open(path, "r", encoding="utf-8") as f:
        return [line for line in f]


def test_line_splitter_agrees_with_text_mode(tmp_path):
    d = golden()
    samples = [d["e_bytes"].tobytes(), b"", b"\n", b"\r", b"\r\n", b"a", b"a\n", b"a\r", b"a\r\nb", b"\n\r", b"\r\r\n\n", b"a\rb\nc\r\nd",
               "x\u2028y\x0bz\x0cw\x1cv\x85u\n\u2029".encode("utf-8")]
    for raw in samples:
        off = split_lines(np.frombuffer(raw, dtype=np.uint8))
        assert off.dtype == np.int32 and off[0] == 0 and (raw == b"" or off[-1] == len(raw)) and np.all(np.diff(off) > 0)
        mine = [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
        want = python_lines(raw, tmp_path)
        assert len(mine) == len(want), raw
        assert [m.strip() for m in mine] == [w.strip() for w in want], raw
        assert [m.replace("\r\n", "\n").replace("\r", "\n") for m in mine] == want, raw      # universal newlines
    # case (e) is the reference's own reading: its vocabulary, counts and longest line from these lines
    raw = d["e_bytes"].tobytes()
    off = split_lines(d["e_bytes"])
    lines = [raw[a:b].decode("utf-8").strip() for a, b in zip(off[:-1], off[1:])]
    assert len(lines) == int(d["e_lines"]) == 7 and lines[0].startswith("\ufeff")
    vocab, counts, _, longest = python_rule([f"<START> {line} <END>" for line in lines])
    assert unpack(d["e_tok_bytes"], d["e_tok_off"]) == vocab and d["e_counts"].tolist() == counts and int(d["e_longest"]) == longest
    # ... and the bytes as they are, unwrapped, give the same ids: START / END are special
    assert python_rule([raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])])[0] == vocab


def test_header_declares_the_symbols():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for kind, sym in (("size_t", "i2l_vocab_fit_workspace_bytes"), ("int", "i2l_vocab_fit")):
        assert re.search(r"^" + kind + r"\s+" + sym + r"\s*\(", header, flags=re.M), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    assert isinstance(_lib.lib().i2l_vocab_fit, ctypes._CFuncPtr)
    assert _lib.lib().i2l_version() >= 102


def test_workspace_size_query():
    size = _lib.lib().i2l_vocab_fit_workspace_bytes
    for bad in (0, 1, 3, 1000, 1025, (1 << 17) + 1, -1024, 1 << 40):
        assert size(10, bad) == 0, bad
    assert size(-1, 1024) == 0 and size(0, 1024) > 0
    sizes = [size(10, 1 << k) for k in range(1, 25)]
    assert all(s > 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(s >= 16 * (1 << k) for k, s in zip(range(1, 25), sizes))       # a 64-bit key, a count and an offset per slot


def test_fit_argument_errors_come_before_any_launch():
    """Every refusal below returns before the first HIP call: no device is needed (or touched)."""
    L = _lib.lib()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    off = np.array([0, 3], np.int32)

    def call(text_bytes=3, rows=1, n_skip=0, slots=1024, flags=0, out_cap=8, meta=p, ws=p, ws_bytes=1 << 30, row_off=p):
        return L.i2l_vocab_fit(p, text_bytes, row_off, rows, p, off.ctypes.data, n_skip, slots, flags, p, 64, p, p, p, out_cap,
                               meta, ws, ws_bytes, None)

    assert call(slots=1000) == -1 and call(slots=0) == -1 and call(rows=-1) == -1 and call(text_bytes=-1) == -1
    assert call(flags=2) == -1 and call(out_cap=-1) == -1 and call(meta=None) == -1 and call(row_off=None) == -1
    assert call(text_bytes=1 << 31) == -2 and call(n_skip=9) == -2
    assert call(ws=None) == -3 and call(ws_bytes=64) == -3
    long_skip = np.array([0, 300], np.int32)
    assert L.i2l_vocab_fit(p, 3, p, 1, p, long_skip.ctypes.data, 1, 1024, 0, p, 64, p, p, p, 8, p, p, 1 << 30, None) == -2
    down = np.array([5, 2], np.int32)
    assert L.i2l_vocab_fit(p, 3, p, 1, p, down.ctypes.data, 1, 1024, 0, p, 64, p, p, p, 8, p, p, 1 << 30, None) == -1


def test_token_table_encode_save_load(tmp_path):
    d = golden()
    vocab = unpack(d["c_tok_bytes"], d["c_tok_off"])
    table = TokenTable({t: i for i, t in enumerate(vocab)}, max_sequence_length=77)
    unk = table.unk_token_id
    for text in unpack(d["c_bytes"], d["c_off"]) + ["nothing known here", "x\u3000<END>\tzzz"]:
        want = [table.token_to_id.get(t, unk) for t in text.split()]
        assert table.encode(text) == want
        assert table.encode(text, add_special_tokens=True) == [table.start_token_id] + want + [table.end_token_id]
    path = str(tmp_path / "sub" / "dir" / "vocab.pt")
    table.save(path)
    saved = torch.load(path)
    assert set(saved) == {"token_to_id", "special_tokens", "max_sequence_length"}                 # tokenizer.py:268-272
    assert saved["token_to_id"] == table.token_to_id and saved["max_sequence_length"] == 77
    assert saved["special_tokens"] == {"PAD": "<PAD>", "START": "<START>", "END": "<END>", "UNK": "<UNK>"}
    back = TokenTable.load(path)
    assert back.token_to_id == table.token_to_id and back.id_to_token == table.id_to_token and back.vocab_size == len(vocab)
    assert back.special_tokens == table.special_tokens and back.max_sequence_length == 77
    assert (back.pad_token_id, back.start_token_id, back.end_token_id, back.unk_token_id) == (0, 1, 2, 3)
    assert back.decode(back.encode("\\cmd1 \\cmd11 zzz", True), False) == "<START> \\cmd1 \\cmd11 <UNK> <END>"
    with pytest.raises(FileNotFoundError):
        TokenTable.load(str(tmp_path / "missing.pt"))
    # a file as the reference's LaTeXTokenizer.save writes it (the same three keys, other special strings)
    special = {"PAD": "[p]", "START": "[s]", "END": "[e]", "UNK": "[u]"}
    torch.save({"token_to_id": {"[u]": 0, "[s]": 1, "[p]": 2, "[e]": 3, "x": 4}, "special_tokens": special,
                "max_sequence_length": 9}, str(tmp_path / "theirs.pt"))
    theirs = TokenTable.load(str(tmp_path / "theirs.pt"))
    assert (theirs.pad_token_id, theirs.start_token_id, theirs.end_token_id, theirs.unk_token_id) == (2, 1, 3, 0)
    assert theirs.encode("x y", True) == [1, 4, 0, 3]


def test_fit_refuses_what_the_reference_refuses(tmp_path):
    """Raised on the host, before anything is uploaded."""
    table = TokenTable()
    with pytest.raises(ValueError):
        table.fit([])
    empty = tmp_path / "empty.lst"
    empty.write_bytes(b"")
    with pytest.raises(ValueError):
        table.fit_on_formulas_file(str(empty))
    bad = tmp_path / "bad.lst"
    bad.write_bytes(b"a b\n\xff\xfe c\n")
    with pytest.raises(UnicodeDecodeError):
        table.fit_on_formulas_file(str(bad))
    with pytest.raises(FileNotFoundError):
        table.fit_on_formulas_file(str(tmp_path / "missing.lst"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert table.vocab_size == 4 and table.token_to_id == {t: i for i, t in enumerate(SPECIAL)}
