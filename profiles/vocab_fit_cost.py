"""What fitting the vocabulary costs: the device fit (training/vocab.py: upload, i2l_vocab_fit's launches, the read back and
the dict) against the HOST rule (LaTeXTokenizer.fit restated: ``Counter`` over ``str.split()`` + a stable ``sorted``) on
one core of the same box, in ONE process; the same for a formulas FILE (fit_formulas_file against open / strip / wrap /
fit); the HIP-event time of the launches alone, with the per-workgroup LDS aggregation and without it (the ablation).

The corpus is generated at the workload's size: 100 k formulas of 40 - 147 tokens, about 500 distinct tokens of 1 - 15
bytes, Zipf-like frequencies under three dominant tokens ({ and } a quarter of the corpus each, _ a tenth).
usage: python profiles/vocab_fit_cost.py [--formulas N] [--rounds R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from collections import Counter

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd.training import fit_formulas_file, fit_vocabulary, pack_texts   # noqa: E402
from img2latex_amd.training import vocab as V                                       # noqa: E402
from img2latex_amd.training.tokenizer import upload_packed                          # noqa: E402

SPECIAL = ["<PAD>", "<START>", "<END>", "<UNK>"]


def make_corpus(n_formulas, seed=11):
    rng = np.random.default_rng(seed)
    words = ["{", "}", "_"] + [f"\\{i:x}" + "x" * ((i * 7) % 12) for i in range(500)]
    p = np.concatenate([[0.25, 0.25, 0.10], 0.40 / np.arange(1, 501) / np.sum(1.0 / np.arange(1, 501))])
    lens = rng.integers(40, 148, n_formulas)
    draw = rng.choice(len(words), size=int(lens.sum()), p=p)
    texts, at = [], 0
    for n in lens.tolist():
        texts.append(" ".join(words[i] for i in draw[at:at + n].tolist()))
        at += n
    return texts


def host_rule(texts):
    """tokenizer.py:87-104 restated -> token_to_id."""
    counter = Counter()
    for text in texts:
        counter.update(text.split())
    vocab = {t: i for i, t in enumerate(SPECIAL)}
    for token, _ in sorted(counter.items(), key=lambda kv: kv[1], reverse=True):
        if token not in vocab:
            vocab[token] = len(vocab)
    max(len(text.split()) for text in texts)                         # :107, the second pass of the reference
    return vocab


def host_file_rule(path):
    """tokenizer.py:131-141 restated."""
    with open(path, "r", encoding="utf-8") as f:
        formulas = [line.strip() for line in f]
    return host_rule([f"<START> {formula} <END>" for formula in formulas])


def timed(fn, reps, sync=False):
    ts, out = [], None
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def fmt(ts):
    return f"median {statistics.median(ts):.2f} ms (runs: {', '.join(f'{t:.2f}' for t in ts)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formulas", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocab_fit_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    dev = torch.device("cuda:0")
    texts = make_corpus(args.formulas)
    data, off = pack_texts(texts)
    fit_vocabulary(texts[:100], device=dev)                          # loads the library, creates the context
    want, host_ts = timed(lambda: host_rule(texts), min(args.rounds, 3))
    got, dev_ts = timed(lambda: fit_vocabulary(texts, device=dev), args.rounds, sync=True)
    assert got.token_to_id == want and list(got.token_to_id) == list(want), "device and host vocabularies disagree"
    _, packed_ts = timed(lambda: fit_vocabulary((data, off), device=dev), args.rounds, sync=True)
    _, pack_ts = timed(lambda: pack_texts(texts), args.rounds)
    _, upload_ts = timed(lambda: upload_packed(data, off, dev), args.rounds, sync=True)

    # the launches alone (two memsets + count + compact + sort + offsets + emit), HIP events around 5 queued calls
    text, row_off = upload_packed(data, off, dev)
    skip = [s.encode() for s in SPECIAL]
    launches = {}
    for name, flags in (("LDS table per workgroup, one flush", 0), ("one global atomicAdd + atomicMin per token", V.NO_AGGREGATE)):
        ints, _, _ = V.launch(text, row_off, skip, V.FIRST_SLOTS, flags)
        assert ints[:V.META_WORDS].cpu().tolist()[:6] == [len(want) - 4, 0, got.total_tokens, got.longest_row,
                                                          sum(len(t.encode()) for t in list(want)[4:]), 0]
        launches[name] = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                V.launch(text, row_off, skip, V.FIRST_SLOTS, flags)
            e1.record()
            torch.cuda.synchronize()
            launches[name].append(e0.elapsed_time(e1) / 5)

    # a formulas file
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "formulas.norm.lst")
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(texts) + "\n")
        want_file, host_file_ts = timed(lambda: host_file_rule(path), min(args.rounds, 3))
        got_file, dev_file_ts = timed(lambda: fit_formulas_file(path, device=dev), args.rounds, sync=True)
    assert got_file.token_to_id == want_file and list(got_file.token_to_id) == list(want_file)

    lines = [f"vocab_fit_cost: {len(texts)} formulas, {got.total_tokens} tokens ({got.total_tokens / len(texts):.1f} per formula, "
             f"longest {got.longest_row}), {data.size} bytes, {len(want) - 4} distinct tokens; the three most frequent hold "
             f"{100.0 * np.sort(got.counts)[-3:].sum() / got.total_tokens:.1f} % of the corpus; slots = {V.FIRST_SLOTS}", "",
             f"host rule (Counter over str.split() + sorted + the max() pass), one core: {fmt(host_ts)}",
             f"fit_vocabulary(list of str), end to end (pack_texts, upload, launches, meta + token read back, dict): {fmt(dev_ts)}",
             f"fit_vocabulary(packed bytes + offsets), end to end: {fmt(packed_ts)}",
             f"  pack_texts alone, host, one core: {fmt(pack_ts)}",
             f"  upload alone (one blocking copy): {fmt(upload_ts)}", ""]
    for name, ts in launches.items():
        lines.append(f"i2l_vocab_fit's launches alone, HIP events over 5 queued calls, {name}: {fmt(ts)} per call")
    lines += ["", f"formulas file, host rule (open, strip, wrap in START / END, fit), one core: {fmt(host_file_ts)}",
              f"formulas file, fit_formulas_file (np.fromfile, utf-8 check, split_lines, device fit): {fmt(dev_file_ts)}"]
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
