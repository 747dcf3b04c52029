#!/usr/bin/env python3
"""Golden vectors for the device tokenizer (i2l_tokenize): runs the REAL reference LaTeXTokenizer of
img2latex/data/tokenizer.py (imported unmodified from /root/reference; same inert torchvision shim as make_golden.py
because img2latex/__init__ pulls the model package) and stores inputs + outputs in tests/golden/tokenize.npz:

    tokens, token_ids          the vocabulary the reference's own fit_on_formulas_file made on a small generated formulas
                               file (a few hundred tokens, some non-ASCII)
    text_bytes, text_off       ~64 texts in UTF-8, back to back (empty, whitespace-only, leading / trailing / doubled
                               separators, tabs, U+00A0 / U+2003 / U+3000 as separators, unknown tokens, a literal <END>,
                               rows of more than 150 tokens)
    enc_s{0,1}_m{5,150}        encode_batch(texts, add_special_tokens=s) at max_sequence_length = m
    collated                   Im2LatexCollator's padded matrix of encode(f"{START} {t} {END}") (dataset.py:333-335,59-66)

The archive is written with fixed zip timestamps, so a re-run gives the same bytes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tokenize.py
"""
import io
import os
import sys
import tempfile
import types
import zipfile

sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True
_tv = types.ModuleType("torchvision")
_tv.__path__ = []
for _sub in ("models", "transforms", "transforms.functional"):
    _m = types.ModuleType("torchvision." + _sub)
    _m.__path__ = []
    sys.modules["torchvision." + _sub] = _m
    setattr(sys.modules["torchvision." + _sub.rsplit(".", 1)[0]] if "." in _sub else _tv, _sub.rsplit(".", 1)[-1], _m)
sys.modules["torchvision"] = _tv

import logging  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

logging.disable(logging.CRITICAL)
from img2latex.data.tokenizer import LaTeXTokenizer  # noqa: E402  (the reference)


class Lcg:
    """A generator that is the same everywhere."""

    def __init__(self, seed):
        self.s = seed

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (self.s >> 33) % n


def make_words():
    words = ["\\frac", "\\alpha", "\\beta", "{", "}", "^", "_", "(", ")", "=", "+", "-", "\\sum", "\\int", "\\left(", "\\right)",
             "α", "β", "γ", "∑", "∫", "→", "≤", "∞", "é", "𝔽", "\\operatorname", "\\longleftrightarrow", "x", "y", "z", "0", "1", "2"]
    words += [f"\\cmd{i}" for i in range(120)] + [f"v_{{{i}}}" for i in range(80)] + [f"π{i}" for i in range(40)]
    return words


def make_formulas(words, n, rng):
    out = []
    for _ in range(n):
        k = 3 + rng.below(40)
        out.append(" ".join(words[rng.below(len(words))] for _ in range(k)))
    return out


def make_texts(words, rng):
    pick = lambda k: [words[rng.below(len(words))] for _ in range(k)]
    texts = ["", " ", "   \t  ", "  \u3000", "x", " x", "x ", "  x  y  ", "\\frac  {  x  }  {  y  }",
             "\tx\ty\t", "x\u00a0y", "x\u2003y", "x\u3000y z", "\u00a0x\u2003\u2003y\u3000", "\u3000x  y\t\n",
             "x\ny\r\nz", "x\x0by\x0cz", "x\x1cy\x1dz\x1ey\x1fx", "x\u0085y", "x\u1680y\u2000z\u200ax\u2028y\u2029z\u202fx\u205fy",
             "notaword", "x notaword y", "\\cmd5x", "\\cmd", "\u03b1\u03b2", "\u03b1 \u03b2", "x\u200by", "x\u180ey", "x\ufeffy",
             "<END>", "x <END> y", "<START> x <END>", "<PAD> <UNK> x", "<END", "END>", "\U0001d53d \u2192 \u221e",
             "\\cmd119 \\cmd0 v_{79} \u03c039"]
    texts += [" ".join(pick(150)), " ".join(pick(151)), " ".join(pick(149)), " ".join(pick(148)), " ".join(pick(200)),
              "  ".join(pick(160)) + " ", " ".join(["x"] * 400), " ".join(pick(155)), " ".join(pick(4)), " ".join(pick(5)),
              " ".join(pick(6)), " ".join(pick(3))]
    while len(texts) < 64:
        toks = pick(1 + rng.below(60))
        if rng.below(3) == 0:
            toks[rng.below(len(toks))] = "unk" + str(rng.below(1000))
        seps = [" ", "  ", "\t", "\u00a0", "\u2003", "\u3000"]
        texts.append("".join(t + seps[rng.below(len(seps)) if rng.below(4) == 0 else 0] for t in toks))
    return texts


def fitted(words, max_sequence_length):
    rng = Lcg(2024)
    formulas = make_formulas(words, 300, rng)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "formulas.norm.lst")
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(formulas) + "\n")
        tok = LaTeXTokenizer(max_sequence_length=max_sequence_length)
        tok.fit_on_formulas_file(path)
    return tok


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    words = make_words()
    texts = make_texts(words, Lcg(7))
    out = {}
    vocab = None
    for m in (5, 150):
        tok = fitted(words, m)
        items = sorted(tok.token_to_id.items(), key=lambda kv: kv[1])
        if vocab is None:
            vocab = items
            out["tokens"] = np.array([k for k, _ in items])
            out["token_ids"] = np.array([v for _, v in items], np.int32)
        assert items == vocab
        for s in (0, 1):
            out[f"enc_s{s}_m{m}"] = tok.encode_batch(texts, add_special_tokens=bool(s)).numpy().astype(np.int32)
    sp = tok.special_tokens
    rows = [torch.tensor(tok.encode(f"{sp['START']} {t} {sp['END']}"), dtype=torch.long) for t in texts]   # dataset.py:333-335
    max_len = max(len(r) for r in rows)                                                                    # collator :59-66
    padded = torch.full((len(rows), max_len), tok.pad_token_id, dtype=torch.long)
    for i, r in enumerate(rows):
        padded[i, :len(r)] = r
    out["collated"] = padded.numpy().astype(np.int32)
    enc = [t.encode("utf-8") for t in texts]
    out["text_bytes"] = np.frombuffer(b"".join(enc), dtype=np.uint8)
    out["text_off"] = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int32)
    out["special_ids"] = np.array([tok.pad_token_id, tok.start_token_id, tok.end_token_id, tok.unk_token_id], np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tokenize.npz")
    write_npz(path, out)
    print("vocab", len(vocab), "texts", len(texts), "collated", out["collated"].shape, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
