"""i2l_tokenize (packed UTF-8 text -> padded token id rows on the device) through the C ABI, and the layers on top of it:
TokenizeTable.encode_batch / collate, Predictor.evaluate_batch / evaluate_stream with string targets.  Every comparison is
exact integer equality: with the REFERENCE's results (tests/golden/tokenize.npz) or with the Python rule --
``str.split()`` + ``dict.get`` + cut + pad (tokenizer.py:143-164,196-232)."""
import os

import numpy as np
import pytest
import torch

from helpers import END, GOLDEN, START, load, model_for
from img2latex_amd import _lib, synth
from img2latex_amd.training import DetokenizeTable, Predictor, TokenTable, TokenizeTable, pack_texts, tokenize_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, UNK = 0, 3
SENTINEL = -77
WHITESPACE = [chr(c) for c in list(range(0x09, 0x0e)) + list(range(0x1c, 0x21)) + [0x85, 0xa0, 0x1680] + list(range(0x2000, 0x200b)) +
              [0x2028, 0x2029, 0x202f, 0x205f, 0x3000]]
NEAR_MISSES = [chr(c) for c in (0x1b, 0x7f, 0x84, 0x86, 0xa1, 0x180e, 0x200b, 0x2027, 0x2060, 0x3001, 0xfeff)]


def synthetic_table():
    """Tokens of 1, 2, 3 (non-ASCII), 13, 40 and 300 bytes + the four special tokens + the empty key."""
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3, "": 4}
    words = list("abcdefghij") + ["α", "β", "γ", "δ", "é"] + ["∑", "∫", "→", "≤", "∞"] + \
        ["\\operatorname", "\\longleftarrow", "\\mathfrak{abc}"[:13]] + ["\\" + "x" * 39, "\\" + "y" * 39] + ["{" + "z" * 298 + "}"]
    words += [f"w{i}" for i in range(12)]
    for v, w in enumerate(words, start=5):
        vocab[w] = v
    assert {0, 1, 2, 3, 13, 40, 300} <= {len(t.encode("utf-8")) for t in vocab}
    return TokenTable(vocab, max_sequence_length=150), words


TOK, WORDS = synthetic_table()
_STATE = {}


def table():
    t = tokenize_table(TOK, DEV)
    assert t is tokenize_table(TOK, DEV) and (t.pad_id, t.start_id, t.end_id, t.unk_id) == (PAD, START, END, UNK)
    return t


def python_rule(texts, add_special, width, vocab=None):
    vocab = TOK.token_to_id if vocab is None else vocab
    rows, counts = [], []
    for t in texts:
        ids = [vocab.get(w, UNK) for w in t.split()]
        ids = [START] + ids + [END] if add_special else ids
        counts.append(len(ids))
        rows.append(ids[:width] + [PAD] * max(0, width - len(ids)))
    counts = np.array(counts, np.int32)
    return np.array(rows, np.int32).reshape(len(texts), width), np.minimum(counts, width).astype(np.int32), counts


def run(data, off, width, add_special, stride=None, rows=None, text_bytes=None, t=None):
    """The C call on (bytes, offsets) -> (rc, out matrix with its sentinel columns, out_len, out_count, status)."""
    t = table() if t is None else t
    rows = off.size - 1 if rows is None else rows
    stride = width + 3 if stride is None else stride
    text = torch.from_numpy(np.concatenate([np.asarray(data, np.uint8), np.zeros(1, np.uint8)])).to(DEV)
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int32)).to(DEV)
    n = max(off.size - 1, 1)
    out = torch.full((n, max(stride, 1)), SENTINEL, dtype=torch.int32, device=DEV)
    meta = torch.full((2 * n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    rc = _lib.lib().i2l_tokenize(text.data_ptr(), int(data.size if text_bytes is None else text_bytes), d_off.data_ptr(), rows,
                                 t.image.data_ptr(), t.image.numel(), t.unk_id, t.pad_id, t.start_id, t.end_id, int(add_special),
                                 width, out.data_ptr(), stride, meta.data_ptr(), meta.data_ptr() + 4 * n, meta.data_ptr() + 8 * n,
                                 _lib.stream_ptr())
    torch.cuda.synchronize()
    m = meta.cpu().numpy()
    return rc, out.cpu().numpy(), m[:n], m[n:2 * n], int(m[2 * n])


def check(texts, width, add_special, what=None):
    data, off = pack_texts(texts)
    want, want_len, want_count = python_rule(texts, add_special, width)
    rc, out, out_len, out_count, status = run(data, off, width, add_special)
    assert rc == 0, what
    bad = np.nonzero((out[:, :width] != want).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad[0]), texts[int(bad[0])][:80], out[bad[0], :12], want[bad[0], :12])
    assert bool((out[:, width:] == SENTINEL).all()), what                               # nothing behind the row
    assert np.array_equal(out_len, want_len) and np.array_equal(out_count, want_count), what
    assert status == int(bool((want_count > width).any())), what
    return want


# ------------------------------------------------------------------------------------------------ against the fixture
def test_the_reference_results():
    d = np.load(os.path.join(GOLDEN, "tokenize.npz"))
    raw, off = d["text_bytes"].tobytes(), d["text_off"]
    texts = [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
    vocab = {str(t): int(i) for t, i in zip(d["tokens"], d["token_ids"])}
    for m in (5, 150):
        t = TokenizeTable(TokenTable(vocab, max_sequence_length=m), DEV)
        for s in (0, 1):
            got = t.encode_batch(texts, add_special_tokens=bool(s))
            assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (64, m)
            assert np.array_equal(got.cpu().numpy(), d[f"enc_s{s}_m{m}"]), (s, m)
    got = t.collate(texts)
    assert got.dtype == torch.int32 and got.is_cuda and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), d["collated"])
    assert tuple(t.collate([]).shape) == (0, 0)


# ----------------------------------------------------------------------------------------- against the Python rule
def make_row(rng, n_bytes):
    """A row of exactly n_bytes: known tokens, unknown ones and separators of every width, drawn at random."""
    unknown = ["q", "zz", "ab", "\\operatornamf", "w12", "α∑", "ω"]
    seps = [" ", " ", " ", "  ", "\t", "\n", "\u00a0", "\u2003", "\u3000", " \u2029 ", "\u1680"]
    parts, left = [], n_bytes
    want_sep = bool(rng.integers(0, 2))
    while left > 0:
        pool = seps if want_sep else (WORDS if rng.integers(0, 5) else unknown)
        fits = [p for p in pool if len(p.encode("utf-8")) <= left]
        piece = fits[rng.integers(0, len(fits))] if fits else (" " if want_sep else "a")
        parts.append(piece)
        left -= len(piece.encode("utf-8"))
        want_sep = not want_sep
    text = "".join(parts)
    assert len(text.encode("utf-8")) == n_bytes
    return text


def texts_for(rows):
    if rows not in _STATE:
        rng = np.random.default_rng(rows)
        lens = [0, 1, 63, 64, 65, 255, 256, 257, 6000 + rows % 7]
        _STATE[rows] = [make_row(rng, lens[(i + rows) % len(lens)]) for i in range(rows)]
    return _STATE[rows]


@pytest.mark.parametrize("add_special", [0, 1])
@pytest.mark.parametrize("width", [1, 2, 5, 150])
@pytest.mark.parametrize("rows", [1, 3, 67, 257])
def test_ids_equal_the_python_rule(rows, width, add_special):
    texts = texts_for(rows)
    want = check(texts, width, add_special, (rows, width, add_special))
    if rows >= 67 and width == 150:
        assert bool((want == UNK).any()) and bool((want > 4).any()) and bool((want == PAD).any())


def test_every_row_length_untruncated():
    """All nine row lengths in one launch at a width that cuts nothing (a 6000-byte row holds up to 3000 tokens)."""
    rng = np.random.default_rng(99)
    texts = [make_row(rng, n) for n in (0, 1, 63, 64, 65, 255, 256, 257, 6001, 128, 127, 129, 192, 2)]
    for s in (0, 1):
        want = check(texts, 3002 + 2 * s, s, ("untruncated", s))
    assert (want != PAD).sum(axis=1).max() > 150


def test_planted_rows():
    texts = ["", " ", " \t\u3000 \u00a0 \n\x1c", "\u3000", " ".join(["a"] * 3000), "b" * 5000, "x" + "q" * 4999 + " a",
             "a " + "{" + "z" * 298 + "}" + " b", "{" + "z" * 299 + "}", "{" + "z" * 297 + "}", "{" + "z" * 298, "{" + "z" * 298 + "}}"]
    texts += [f"a{w}\\operatorname" for w in WHITESPACE] + [f"∑{w}{w}α{w}" for w in WHITESPACE]
    texts += [f"a{c}b" for c in NEAR_MISSES] + [f"a {c} b" for c in NEAR_MISSES]
    # unknown tokens next to known ones: first / middle / last byte differs, proper prefix, one byte more
    for w in ("\\operatorname", "\\" + "x" * 39, "w11", "∑", "a"):
        b = w.encode("utf-8")
        for i in sorted({0, len(b) // 2, len(b) - 1}):
            m = bytearray(b)
            m[i] = m[i] ^ 0x01 if m[i] < 0x80 else (m[i] ^ 0x01) | 0x80
            try:
                texts.append(f"a {bytes(m).decode('utf-8')} {w}")
            except UnicodeDecodeError:
                pass
        texts += [f"{w[:-1]} b" if len(w) > 1 else "b", f"b {w}a", f"{w}{w}", f"a{w}"]
    texts += ["<START> a <END> b <PAD> <UNK> <START>", "<START>a", "<END", "START>"]
    for s in (0, 1):
        for width in (150, 3002):
            check(texts, width, s, ("planted", s, width))
    # each whitespace character separates, each near miss does not (the Python rule says so; spelled out once)
    assert all(len(f"a{w}b".split()) == 2 for w in WHITESPACE) and all(len(f"a{c}b".split()) == 1 for c in NEAR_MISSES)


def test_three_byte_separator_across_every_chunk_boundary():
    """U+3000 (E3 80 80) beginning at row offsets 61 + shift + 64 j: it ends at, straddles (2|1, 1|2) and begins at the
    64-byte boundaries of the wave's chunks; so do U+00A0 (C2 A0) and a token's first and last bytes."""
    texts = []
    for sep in ("\u3000", "\u00a0", " "):
        n = len(sep.encode("utf-8"))
        piece = sep + "b " + "q" * (64 - n - 4) + " c"
        assert len(piece.encode("utf-8")) == 64
        for shift in range(0, 5):
            texts.append("x" * (61 + shift) + piece * 5 + sep + "a")
            texts.append("a " * 30 + "a"[:shift] + piece * 3 + sep + "\\operatorname")
    for s in (0, 1):
        check(texts, 150, s, ("straddle", s))


def test_unusable_offsets_are_empty_rows():
    text = "a b c d e f g h i j " * 5                                                    # 100 bytes
    data = np.frombuffer(text.encode(), np.uint8)
    off = np.array([0, 10, 5, 20, 200, 30, 40, -4, 8, 100, 101], np.int32)
    ok = {0: text[0:10], 2: text[5:20], 5: text[30:40], 8: text[8:100]}                 # rows whose [start, end) is usable
    rc, out, out_len, out_count, status = run(data, off, 8, 0)
    assert rc == 0 and status & 2
    for r in range(10):
        want, want_len, want_count = python_rule([ok.get(r, "")], 0, 8)
        assert np.array_equal(out[r, :8], want[0]) and out_len[r] == want_len[0] and out_count[r] == want_count[0], r
        if r not in ok:
            assert bool((out[r, :8] == PAD).all()) and out_len[r] == 0
    assert status == 3 and bool((out[:, 8:] == SENTINEL).all())                         # row 8 was cut: bit 0 as well
    rc, out, _, _, status = run(data, off[:2], 8, 0)
    assert rc == 0 and status == 0                                                      # the word is cleared by every call


def test_refusals_launch_nothing():
    data, off = pack_texts(["a b", "c"])
    untouched = lambda r, rc: r[0] == rc and all(bool((a == SENTINEL).all()) for a in r[1:4]) and r[4] == SENTINEL
    assert untouched(run(data, off, 0, 0, stride=4), -2)
    assert untouched(run(data, off, -1, 0, stride=4), -2)
    assert untouched(run(data, off, 5, 1, stride=4), -2)                                # out_stride < width
    assert untouched(run(data, off, 4, 0, text_bytes=2 ** 31), -2)                      # text_bytes beyond int32
    assert untouched(run(data, off, 4, 0, rows=0), 0)                                   # no rows: success, no launch
    rc, out, out_len, _, status = run(data, off, 4, 1, stride=4)
    assert rc == 0 and status == 0 and out.tolist() == [[START, 5, 6, END], [START, 7, END, PAD]] and out_len.tolist() == [4, 3]


def test_round_trip_through_detokenize():
    rng = np.random.default_rng(5)
    seps = [" ", "  ", "\t", "\u00a0", " \u3000 ", "\n"]
    texts = ["", "  ", "a"]
    for _ in range(40):
        n = int(rng.integers(1, 60))
        texts.append("".join(WORDS[rng.integers(0, len(WORDS))] + seps[rng.integers(0, len(seps))] for _ in range(n)))
    ids = table().encode_batch(texts)
    got, _ = DetokenizeTable(TOK, DEV).decode_now(ids, -1)
    assert got == [" ".join(t.split()) for t in texts]


# ---------------------------------------------------------------------------------------------- the evaluate chain
def tiny():
    d, cfg, _ = load("tiny_l1")
    m, _ = model_for("tiny_l1")
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({(f"τ{i}" if i % 3 else f"\\t{i}"): i for i in range(4, cfg["vocab_size"])})
    return m, cfg, TokenTable(vocab, max_sequence_length=12)


def formulas(tok, rng, n, longest=9):
    seps = [" ", "  ", "\t", "\u2003"]
    out = []
    for _ in range(n):
        ids = rng.integers(4, tok.vocab_size, int(rng.integers(3, longest + 1)))
        out.append("".join(tok.id_to_token[int(i)] + seps[rng.integers(0, len(seps))] for i in ids) + ("zzz" if rng.integers(0, 3) == 0 else ""))
    return out


def host_collate(tok, texts):
    _, _, counts = python_rule(texts, 1, 1, tok.token_to_id)
    return torch.from_numpy(python_rule(texts, 1, int(counts.max()), tok.token_to_id)[0])


def same(a, b):
    assert (a["bleu"], a["levenshtein"], a["batch_size"]) == (b["bleu"], b["levenshtein"], b["batch_size"])
    la, lb = a["pred_len"].cpu().numpy(), b["pred_len"].cpu().numpy()
    n = int(max(la.max(), 1))
    assert np.array_equal(la, lb) and np.array_equal(a["pred_ids"][:, :n].cpu().numpy(), b["pred_ids"][:, :n].cpu().numpy())


def test_evaluate_with_string_targets():
    m, cfg, tok = tiny()
    pred = Predictor(m, tok, device=torch.device(DEV))
    rng = np.random.default_rng(3)
    x = torch.from_numpy(synth.make_images(15, cfg, seed=1234)).to(DEV)
    images = [x[i:i + 5] for i in range(0, 15, 5)]
    texts = [formulas(tok, rng, 5) for _ in range(3)]
    texts[2][1] = " ".join(tok.id_to_token[4 + i] for i in range(15))                   # 15 tokens: more than max_sequence_length
    tensors = [host_collate(tok, t) for t in texts]
    assert tensors[2].shape[1] == 17 and all(t.shape[1] <= 12 for t in tensors[:2])
    for im, t, ids in zip(images, texts, tensors):
        want = pred.evaluate_batch(im, ids, max_length=12)
        got = pred.evaluate_batch(im, t, max_length=12)
        same(got, want)
        assert tuple(got["pred_ids"].shape) == tuple(want["pred_ids"].shape)
    want = list(pred.evaluate_stream(zip(images, tensors), max_length=12))
    for mix in ([texts[0], tensors[1], texts[2]], [tensors[0], texts[1], tensors[2]], texts):
        got = list(pred.evaluate_stream(zip(images, mix), max_length=12))
        assert len(got) == 3
        for g, w in zip(got, want):
            same(g, w)

    class IdOnly:                                                    # no vocabulary: strings are refused, not guessed at
        pad_token_id, start_token_id, end_token_id, max_sequence_length = 0, 1, 2, 12

    with pytest.raises(ValueError, match="string targets"):
        Predictor(m, IdOnly(), device=torch.device(DEV)).evaluate_batch(images[0], texts[0], max_length=12)

