"""What string targets cost: Predictor.evaluate_stream fed with raw formula strings (packed on the host, tokenized by
i2l_tokenize on the device) against the same stream fed with id tensors the HOST rule makes per batch (split, dict.get, pad,
torch.tensor: LaTeXTokenizer's encoding restated) and against the stream fed with ready tensors, in ONE process,
alternating; the HIP-event time of the tokenize launch alone; the host times of pack_texts and of the host rule.

B = 256, primary dims, the END-clock weights, a 512-token vocabulary of 2 - 15 byte tokens, formulas of 40 - 148 tokens.
usage: python profiles/tokenize_cost.py [--batches N] [--rounds R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import synth                                                      # noqa: E402
from img2latex_amd.model import Seq2SeqModel                                     # noqa: E402
from img2latex_amd.training import Predictor, TokenTable, pack_texts, tokenize_table   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenize_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    dev = torch.device("cuda:0")
    B, T = 256, 150
    cfg = synth.model_config()
    sd_kw = dict(seed=42, out_scale=12.0, enc_scale=16.0, end_clock=(0.05, 12.0, 6.0))
    model = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, **sd_kw).items()})
    model = model.to(dev).eval()
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"\\{i:x}" + "x" * ((i * 7) % 12): i for i in range(4, cfg["vocab_size"])})     # 2 - 15 bytes
    tok = TokenTable(vocab, max_sequence_length=T)
    pred = Predictor(model, tok, device=dev)
    x = torch.from_numpy(synth.make_images(B, cfg, seed=1234)).to(dev)
    rng = np.random.default_rng(7)
    words = list(vocab)[4:]
    texts = [" ".join(words[i] for i in rng.integers(0, len(words), int(rng.integers(40, 149)))) for _ in range(B)]
    start, end, pad, unk = tok.start_token_id, tok.end_token_id, tok.pad_token_id, tok.unk_token_id

    def host_rule(batch):
        """dataset.py:333-335 + collator :59-66 on the host: START formula END, padded to the longest row."""
        rows = [[vocab.get(w, unk) for w in f"<START> {t} <END>".split()] for t in batch]
        n = max(len(r) for r in rows)
        return torch.tensor([r + [pad] * (n - len(r)) for r in rows], dtype=torch.int32)

    ready = host_rule(texts).to(dev)

    def stream(targets_of, n):
        out = None
        for out in pred.evaluate_stream(((x, targets_of()) for _ in range(n)), max_length=T):
            pass
        return out

    routes = {"evaluate_stream, string targets (pack_texts + i2l_tokenize)": lambda n: stream(lambda: texts, n),
              "evaluate_stream, tensors from the host rule per batch": lambda n: stream(lambda: host_rule(texts), n),
              "evaluate_stream, ready device tensors": lambda n: stream(lambda: ready, n)}
    warm = [fn(12) for fn in routes.values()]
    assert all((w["bleu"], w["levenshtein"]) == (warm[0]["bleu"], warm[0]["levenshtein"]) for w in warm), "the routes disagree"
    table = tokenize_table(tok, dev)
    assert torch.equal(table.collate(texts), ready), "device and host tokenization disagree"
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.batches)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.batches * 1e3)

    # host pieces, one core
    def host_time(fn, reps=30):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    pack = host_time(lambda: pack_texts(texts))
    rule = host_time(lambda: host_rule(texts))
    upload = host_time(lambda: table.upload(texts))

    # the tokenize launch alone: 20 calls queued behind a busy stream, one event pair
    text, row_off = table.upload(texts)
    side = torch.cuda.Stream(device=dev)
    busy = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    per_call, host_call = {}, {}
    with torch.cuda.stream(side):
        for width in (T + 2, 302):
            table.launch(text, row_off, width, True)
            per_call[width], host_call[width] = [], []
            for _ in range(5):
                for _ in range(6):
                    busy @ busy                                      # keeps the stream busy while the calls queue up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                t0 = time.perf_counter()
                for _ in range(20):
                    table.launch(text, row_off, width, True)
                host_call[width].append((time.perf_counter() - t0) / 20 * 1e6)
                e1.record(side)
                side.synchronize()
                per_call[width].append(e0.elapsed_time(e1) / 20 * 1e3)

    n_tok = [len(t.split()) for t in texts]
    lines = [f"tokenize_cost: B={B}, steps={T}, vocab={cfg['vocab_size']}, tokens per formula min/mean/max = "
             f"{min(n_tok)}/{sum(n_tok) / len(n_tok):.1f}/{max(n_tok)}, {int(text.numel())} bytes of text per batch, "
             f"{args.batches} batches per timing, {args.rounds} rounds (alternating)", ""]
    for name, ts in times.items():
        lines.append(f"{name}: median {statistics.median(ts):.3f} ms per batch (rounds: {', '.join(f'{t:.3f}' for t in ts)})")
    lines.append("")
    for width in per_call:
        lines.append(f"i2l_tokenize alone (memset + 1 kernel, width {width}), HIP events over 20 queued calls: median "
                     f"{statistics.median(per_call[width]):.1f} us per call (runs: {', '.join(f'{t:.1f}' for t in per_call[width])}); "
                     f"host time of the call {statistics.median(host_call[width]):.1f} us")
    for name, (med, lo, hi) in (("pack_texts", pack), ("pack_texts + upload (one blocking copy)", upload),
                                ("host rule (split, dict.get, pad, torch.tensor): the yardstick", rule)):
        lines.append(f"{name}, host, one core: median {med:.3f} ms per batch (min {lo:.3f}, max {hi:.3f}, 30 runs)")
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
