"""Formula strings -> the fitted vocabulary on the device: LaTeXTokenizer.fit / fit_on_formulas_file (reference
img2latex/data/tokenizer.py:80-141) through i2l_vocab_fit.  The third part of the string boundary beside
``TokenizeTable`` and ``DetokenizeTable``: the corpus is uploaded once, counted and ordered there, and only the distinct
tokens (a few hundred to a few thousand) come back to become ``token_to_id``."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib
from .predictor import DEFAULT_SPECIAL_TOKENS
from .tokenizer import pack_texts, upload_packed

STATUS_FULL, STATUS_BAD_OFFSETS, STATUS_OUT_TOO_SMALL = 1, 2, 4      # i2l_vocab_fit's status bits (meta[5])
META_WORDS = 16                                                      # I2L_VOCAB_FIT_META_WORDS
NO_AGGREGATE = 1                                                     # I2L_VOCAB_FIT_NO_AGGREGATE
FIRST_SLOTS = 1 << 17                                                # room for 65536 distinct tokens; 3 MB of workspace
MAX_SLOTS = 1 << 28


class VocabFit:
    """What a fit found.  ``token_to_id``: the special tokens at 0 .. n - 1, then every other token by descending count,
    ties in first-seen order; ``counts[id]`` (int64, a special token's is how often its string occurred);
    ``first_offsets[id]`` (byte offset of the first occurrence in the packed corpus, -1 for a special token);
    ``total_tokens``; ``longest_row`` (the reference's ``max_found_length``)."""

    def __init__(self, token_to_id: Dict[str, int], counts: np.ndarray, first_offsets: np.ndarray, total_tokens: int,
                 longest_row: int, rows: int):
        self.token_to_id, self.counts, self.first_offsets = token_to_id, counts, first_offsets
        self.total_tokens, self.longest_row, self.rows = int(total_tokens), int(longest_row), int(rows)

    def frequencies(self) -> Dict[str, int]:
        """Equal to the reference's ``Counter``: every string that occurred, special strings included."""
        return {tok: int(self.counts[i]) for tok, i in self.token_to_id.items() if self.counts[i] > 0}


def split_lines(raw: np.ndarray) -> np.ndarray:
    """Offsets (int32, lines + 1) of the lines of a file's bytes as Python's text mode iterates them (universal
    newlines: ``\\n``, ``\\r\\n`` and a lone ``\\r`` end a line; what follows the last one is a line when it is not empty).
    Line i is ``raw[off[i]:off[i + 1]]`` with its line end, which is whitespace to the token rule."""
    if raw.size > 0x7fffffff:
        raise ValueError("img2latex_amd: more than 2^31 - 1 bytes of text in one file")
    cr = raw == 13
    ends_here = raw == 10
    ends_here[:-1] |= cr[:-1] & ~ends_here[1:]                       # a \r ends a line unless a \n follows it
    if raw.size:
        ends_here[-1] |= cr[-1]
    ends = np.flatnonzero(ends_here) + 1
    tail = [raw.size] if raw.size and (ends.size == 0 or ends[-1] != raw.size) else []
    return np.concatenate([[0], ends, tail]).astype(np.int32)


def launch(text: torch.Tensor, row_off: torch.Tensor, skip: Sequence[bytes], slots: int, flags: int = 0):
    """i2l_vocab_fit on the current stream, no host wait: ``(ints int32, out_bytes uint8, capacity)``; ``ints`` is the
    meta block, then ``out_off`` (capacity + 1), ``out_count`` and ``out_first`` (capacity each)."""
    L, dev = _lib.lib(), row_off.device
    rows, cap = row_off.numel() - 1, slots // 2
    ws_bytes = L.i2l_vocab_fit_workspace_bytes(rows, slots)
    if ws_bytes == 0:
        raise ValueError(f"img2latex_amd: vocab_fit cannot use slots = {slots}")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    ints = torch.empty((META_WORDS + 3 * cap + 1,), dtype=torch.int32, device=dev)
    out = torch.empty((max(text.numel(), 1),), dtype=torch.uint8, device=dev)   # the distinct tokens are part of the text
    skip_bytes = np.frombuffer(b"".join(skip) + b"\0", dtype=np.uint8)
    skip_off = np.zeros(len(skip) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in skip], out=skip_off[1:])
    p = ints.data_ptr() + 4 * META_WORDS
    with torch.cuda.device(dev):
        _lib.check(L.i2l_vocab_fit(
            text.data_ptr() if text.numel() else None, text.numel(), row_off.data_ptr(), rows, skip_bytes.ctypes.data,
            skip_off.ctypes.data, len(skip), slots, flags, out.data_ptr(), out.numel(), p, p + 4 * (cap + 1),
            p + 4 * (2 * cap + 1), cap, ints.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "vocab_fit")
    return ints, out, cap


def fit_vocabulary(texts_or_packed: Union[Sequence[str], Tuple[np.ndarray, np.ndarray]],
                   special_tokens: Optional[Dict[str, str]] = None, device=None, slots: int = FIRST_SLOTS,
                   flags: int = 0) -> VocabFit:
    """LaTeXTokenizer.fit's rule (tokenizer.py:87-104) on the device.  ``texts_or_packed``: the texts, or
    ``pack_texts``' ``(bytes uint8, offsets int32)`` of them.  One upload, the launches, one small read of the meta
    block -- which decides whether the table was big enough; when it was not (more than ``slots / 2`` distinct tokens),
    ONE retry with ``slots`` sized from the now-known total token count -- then one read of the distinct tokens."""
    special = dict(special_tokens or DEFAULT_SPECIAL_TOKENS)
    packed = isinstance(texts_or_packed, tuple) and len(texts_or_packed) == 2 and isinstance(texts_or_packed[0], np.ndarray)
    data, off = texts_or_packed if packed else pack_texts(texts_or_packed)
    data, off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int32)
    rows = off.size - 1
    if rows <= 0:
        raise ValueError("img2latex_amd: fit_vocabulary needs at least one text")
    names = list(dict.fromkeys(special.values()))                    # dict order, as _init_special_tokens numbers them
    skip = [s.encode("utf-8") for s in names]
    if len(skip) > 8 or sum(map(len, skip)) > 256:
        raise ValueError("img2latex_amd: at most 8 special tokens of 256 bytes together")
    device = torch.device("cuda" if device is None else device)
    text, row_off = upload_packed(data, off, device)
    for attempt in (0, 1):
        ints, out, cap = launch(text, row_off, skip, slots, flags)
        meta = ints[:META_WORDS].cpu().tolist()
        status = meta[5]
        if status & STATUS_BAD_OFFSETS:
            raise ValueError("img2latex_amd: fit_vocabulary: the row offsets do not ascend inside the text")
        if not status & STATUS_FULL:
            break
        if attempt == 1 or slots >= MAX_SLOTS:
            raise RuntimeError(f"img2latex_amd: vocab_fit: {slots} slots do not hold the distinct tokens of {meta[2]}")
        need = 2 * max(meta[2], 1)                                   # every token distinct still fits in half the table
        slots = min(MAX_SLOTS, max(2 * slots, 1 << (need - 1).bit_length()))
    if status & STATUS_OUT_TOO_SMALL:                                # cannot happen: capacity = slots / 2, bytes = the text
        raise RuntimeError("img2latex_amd: vocab_fit: output buffers too small")
    n, n_bytes = meta[0], meta[4]
    base = META_WORDS
    host = torch.cat([ints[base:base + n + 1], ints[base + cap + 1:base + cap + 1 + n],
                      ints[base + 2 * cap + 1:base + 2 * cap + 1 + n]]).cpu().numpy()
    tok_off, tok_count, tok_first = host[:n + 1], host[n + 1:2 * n + 1], host[2 * n + 1:]
    blob = out[:n_bytes].cpu().numpy().tobytes()
    token_to_id = {s: i for i, s in enumerate(names)}
    ns = len(token_to_id)
    for r in range(n):
        token_to_id[blob[tok_off[r]:tok_off[r + 1]].decode("utf-8")] = ns + r
    counts = np.concatenate([np.asarray(meta[8:8 + ns], dtype=np.int64), tok_count.astype(np.int64)])
    firsts = np.concatenate([np.full(ns, -1, dtype=np.int64), tok_first.astype(np.int64)])
    return VocabFit(token_to_id, counts, firsts, meta[2], meta[3], rows)


def fit_formulas_file(file_path: str, special_tokens: Optional[Dict[str, str]] = None, device=None) -> VocabFit:
    """LaTeXTokenizer.fit_on_formulas_file's rule (tokenizer.py:126-141): the file's bytes are checked once with
    ``bytes.decode("utf-8")`` (a malformed file raises UnicodeDecodeError, as the reference's ``open`` would), cut into
    lines by ``split_lines`` and fitted as they are (a leading U+FEFF stays part of the first token).  The START / END
    the reference wraps every line in are special, so they change no id: they add 2 to ``longest_row`` and the line
    count to both strings' counts."""
    special = dict(special_tokens or DEFAULT_SPECIAL_TOKENS)
    raw = np.fromfile(file_path, dtype=np.uint8)
    raw.tobytes().decode("utf-8")
    off = split_lines(raw)
    if off.size < 2:
        raise ValueError(f"img2latex_amd: no formulas in {file_path}")
    fitted = fit_vocabulary((raw, off), special, device)
    for name in ("START", "END"):
        fitted.counts[fitted.token_to_id[special[name]]] += fitted.rows
    fitted.total_tokens += 2 * fitted.rows
    fitted.longest_row += 2
    return fitted
