#!/usr/bin/env python3
"""Golden vectors for the device vocabulary fit (i2l_vocab_fit): runs the REAL reference LaTeXTokenizer.fit and
fit_on_formulas_file of img2latex/data/tokenizer.py (imported through make_golden_tokenize.py: its path, its inert
torchvision shim, its generators and its fixed-timestamp writer) on generated corpora and stores, per case c in
tests/golden/vocab_fit.npz:

    {c}_bytes, {c}_off          the corpus in UTF-8, rows back to back (case e: the raw bytes of a formulas FILE, no offsets)
    {c}_tok_bytes, {c}_tok_off  the reference's vocabulary in id order (special tokens first), UTF-8, packed
    {c}_counts                  the count of every vocabulary entry (Counter over str.split(); a special token's is how
                                often its string occurred -- for e, with the START / END the reference wraps each line in)
    {c}_longest                 the reference's max_found_length, read from its own warning

    a   the 300-formula corpus behind tokenize.npz (same seed; the vocabulary equals tokenize.npz's)
    b   ties: 5000 tokens once each, then 200 tokens with counts 2 and 3 interleaved -- order = first occurrence
    c   separators and edges (all 29 whitespace code points, U+200B / U+180E / U+FEFF, 64-byte chunk boundaries, a
        300-byte token, empty rows, a row boundary between equal tokens, literal special tokens, prefixes, same-length
        tokens that differ in one byte)
    d1  one token 50 000 times in ONE row between rare tokens
    d2  one token 50 000 times over 500 rows between rare tokens
    e   a formulas file with \\n, \\r\\n, a lone \\r, U+2028 inside a line, a BOM and no trailing newline

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vocab_fit.py
"""
import logging
import os
import re
import sys
import tempfile
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import make_golden_tokenize as G  # noqa: E402  (puts the reference on the path, with the torchvision shim)
import img2latex.data.tokenizer as ref_tokenizer  # noqa: E402  (the reference)

WHITESPACE = "".join(chr(c) for c in range(0x3001) if chr(c).isspace())      # the 29 code points of str.isspace()
assert len(WHITESPACE) == 29


class _Longest(logging.Handler):
    """Catches the reference's "Found sequences of length N" warning."""

    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.found = None

    def emit(self, record):
        m = re.search(r"Found sequences of length (\d+)", record.getMessage())
        if m:
            self.found = int(m.group(1))


def reference_fit(texts=None, file_bytes=None):
    """(vocabulary in id order, max_found_length) of the reference, with max_sequence_length = 0 so that it always warns."""
    catch = _Longest()
    logging.disable(logging.NOTSET)
    ref_tokenizer.logger.addHandler(catch)
    try:
        tok = ref_tokenizer.LaTeXTokenizer(max_sequence_length=0)
        tok.max_sequence_length = 0                                  # the constructor reads 0 as "not given"
        if texts is not None:
            tok.fit(texts)
        else:
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "formulas.norm.lst")
                with open(path, "wb") as f:
                    f.write(file_bytes)
                tok.fit_on_formulas_file(path)
    finally:
        ref_tokenizer.logger.removeHandler(catch)
        logging.disable(logging.CRITICAL)
    items = sorted(tok.token_to_id.items(), key=lambda kv: kv[1])
    assert [v for _, v in items] == list(range(len(items)))
    return [k for k, _ in items], (catch.found if catch.found is not None else 0)


def case_b():
    toks = [f"u{i}" for i in range(5000)]
    twice = [f"p{i}" for i in range(200)]
    toks += twice + twice + twice[1::2]
    return [" ".join(toks[i:i + 50]) for i in range(0, len(toks), 50)]


def case_c():
    rows = ["a" + "".join(w + f"w{i}" for i, w in enumerate(WHITESPACE)) + " z",
            "".join(WHITESPACE), "x\u200by x\u180ey x\ufeffy \ufeff \u200b",
            " ".join(("chunk%04d" % i)[:5 + i % 4] for i in range(120)),
            "a" * 62 + "\u3000" + "b62", "a" * 63 + "\u3000" + "b63", "a" * 63 + "\u00a0" + "c63", "a" * 61 + "\u2003" + "d61",
            "a" * 64 + " " + "e64", "a" * 63 + " " + "e63", "\u03b1" * 31 + "x" + "\u3000" + "f",
            "Q" * 300, "Q" * 299 + "R" + " " + "Q" * 300 + "\t" + "Q" * 301, "", "   ", "\t\u3000", "",
            "foo ab", "ab bar", "ab", "ab",
            "x <START> y <END>", "<PAD> <UNK> <PAD> <END", "END> <START><END>",
            "\\cmd1 \\cmd11 \\cmd1 \\cmd111 \\cmd \\cmd11"]
    same = [f"s{i:03d}e" for i in range(300)]
    for rep in range(3):
        rows.append(" ".join(t for i, t in enumerate(same) if i % 3 >= rep))
    return rows


def case_d(rows_of_hot):
    per = 50000 // rows_of_hot
    rows = ["rare0 rare1 \\alpha"]
    rows += [" ".join(["{"] * per) for _ in range(rows_of_hot)]
    rows += ["rare2 { rare0", "\\alpha rare3"]
    return rows


def case_e():
    lines = ["\ufeff\\frac { a } { b }", "x ^ { 2 } \u2028 + y", "a   b \\alpha", "", "\\sum _ { i } x _ { i } \\alpha \\beta \\gamma",
             "  lead and trail  ", "last \\frac line"]
    ends = ["\n", "\r\n", "\r", "\r", "\n", "\r\n", ""]
    return "".join(l + e for l, e in zip(lines, ends)).encode("utf-8")


def pack(strings):
    enc = [s.encode("utf-8") for s in strings]
    return (np.frombuffer(b"".join(enc), dtype=np.uint8),
            np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int32))


def main():
    out = {}
    words = G.make_words()
    cases = {"a": G.make_formulas(words, 300, G.Lcg(2024)), "b": case_b(), "c": case_c(), "d1": case_d(1), "d2": case_d(500)}
    for name, texts in cases.items():
        vocab, longest = reference_fit(texts=texts)
        counter = Counter(t for text in texts for t in text.split())
        out[f"{name}_bytes"], out[f"{name}_off"] = pack(texts)
        out[f"{name}_tok_bytes"], out[f"{name}_tok_off"] = pack(vocab)
        out[f"{name}_counts"] = np.array([counter.get(t, 0) for t in vocab], np.int64)
        out[f"{name}_longest"] = np.array(longest, np.int64)
        print(name, "rows", len(texts), "bytes", out[f"{name}_bytes"].size, "vocab", len(vocab), "longest", longest)
    old = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tokenize.npz"))
    assert list(old["tokens"]) == reference_fit(texts=cases["a"])[0] and list(old["token_ids"]) == list(range(len(old["tokens"])))
    raw = case_e()
    vocab, longest = reference_fit(file_bytes=raw)
    with tempfile.TemporaryDirectory() as d:                         # the Counter the reference's own reading gives
        path = os.path.join(d, "f.lst")
        with open(path, "wb") as f:
            f.write(raw)
        with open(path, "r", encoding="utf-8") as f:
            lines = [line.strip() for line in f]
    counter = Counter(t for line in lines for t in f"<START> {line} <END>".split())
    out["e_bytes"] = np.frombuffer(raw, dtype=np.uint8)
    out["e_lines"] = np.array(len(lines), np.int64)
    out["e_tok_bytes"], out["e_tok_off"] = pack(vocab)
    out["e_counts"] = np.array([counter.get(t, 0) for t in vocab], np.int64)
    out["e_longest"] = np.array(longest, np.int64)
    print("e", "lines", len(lines), "bytes", len(raw), "vocab", len(vocab), "longest", longest)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vocab_fit.npz")
    G.write_npz(path, out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
