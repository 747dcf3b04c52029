"""What the error analysis costs: the alignment launch (i2l_edit_alignment, accumulating into a confusion matrix) beside
i2l_sequence_metrics on the same pairs, HIP events over queued calls in ONE process; Predictor.evaluate_stream's per-batch
period from ready device tensors with ``errors`` off and on, alternating in the same process; the margins and top-cells
launches alone; and the host-side alternative, a Python alignment of the same pairs on one core.

256 pairs, targets of 40 - 147 tokens over V = 512, predictions = the targets with about one token in eight substituted,
dropped or doubled.  B = 256, primary dims, the END-clock weights for the stream.
usage: python profiles/error_analysis_cost.py [--batches N] [--rounds R] [--out FILE]
       python profiles/error_analysis_cost.py --period-only [--package-root DIR]    (the errors-off period alone; also runs
                                                                                     on a tree from before the feature)
       python profiles/error_analysis_cost.py --host-only                           (no GPU: the Python alignment alone)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
B, T, V = 256, 150, 512


def make_pairs(seed=7):
    rng = np.random.default_rng(seed)
    targets, preds = [], []
    for _ in range(B):
        t = rng.integers(4, V, int(rng.integers(40, 148))).tolist()
        p = []
        for tok in t:
            u = rng.random()
            if u < 0.04:
                p.append(int(rng.integers(4, V)))           # substituted
            elif u < 0.08:
                continue                                    # dropped
            elif u < 0.12:
                p += [tok, tok]                             # doubled
            else:
                p.append(tok)
        targets.append(t)
        preds.append(p[:T])
    return preds, targets


def python_alignment(preds, targets):
    """The host-side alternative: table, backtrace and confusion counts in the interpreter (dict of cells)."""
    C, total = {}, 0
    for p, r in zip(preds, targets):
        m, n = len(r), len(p)
        D = [list(range(n + 1))] + [[i] + [0] * n for i in range(1, m + 1)]
        for i in range(1, m + 1):
            ri, Di, Dp = r[i - 1], D[i], D[i - 1]
            for j in range(1, n + 1):
                Di[j] = Dp[j - 1] if ri == p[j - 1] else 1 + min(Dp[j - 1], Dp[j], Di[j - 1])
        i, j = m, n
        total += D[m][n]
        while i > 0 or j > 0:
            if i > 0 and j > 0 and r[i - 1] == p[j - 1] and D[i][j] == D[i - 1][j - 1]:
                key = (r[i - 1], p[j - 1]); i -= 1; j -= 1
            elif i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + 1:
                key = (r[i - 1], p[j - 1]); i -= 1; j -= 1
            elif i > 0 and D[i][j] == D[i - 1][j] + 1:
                key = (r[i - 1], V); i -= 1
            else:
                key = (V, p[j - 1]); j -= 1
            C[key] = C.get(key, 0) + 1
    return C, total


def host_line(preds, targets):
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        C, total = python_alignment(preds, targets)
        ts.append(time.perf_counter() - t0)
    return (f"host-side alternative: Python table + backtrace + confusion counts of the same {B} pairs, one core: median "
            f"{statistics.median(ts):.2f} s per batch (runs: {', '.join(f'{t:.2f}' for t in ts)}); summed distance {total}"), C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_analysis_cost.txt"))
    ap.add_argument("--period-only", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--package-root", default=os.path.join(ROOT, "hmer-img2latex_amd"))
    args = ap.parse_args()
    preds, targets = make_pairs()
    if args.host_only:
        print(host_line(preds, targets)[0])
        return
    import torch
    sys.path.insert(0, args.package_root)
    from img2latex_amd import _lib, synth
    from img2latex_amd.model import Seq2SeqModel
    from img2latex_amd.training import Predictor, TokenTable
    from img2latex_amd.training import metrics as M
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    dev = torch.device("cuda:0")
    cfg = synth.model_config()
    assert cfg["vocab_size"] == V
    sd_kw = dict(seed=42, out_scale=12.0, enc_scale=16.0, end_clock=(0.05, 12.0, 6.0))
    model = Seq2SeqModel("cnn_lstm", V, synth.encoder_params(cfg), synth.decoder_params(cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, **sd_kw).items()})
    model = model.to(dev).eval()
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"\\{i:x}": i for i in range(4, V)})
    tok = TokenTable(vocab, max_sequence_length=T)
    pred = Predictor(model, tok, device=dev)
    x = torch.from_numpy(synth.make_images(B, cfg, seed=1234)).to(dev)
    width = max(len(t) for t in targets) + 2
    ready = torch.tensor([[1] + t + [2] + [0] * (width - 2 - len(t)) for t in targets], dtype=torch.int32, device=dev)

    def stream(n, errors):
        kw = {} if errors is None else {"errors": errors}
        out = None
        for out in pred.evaluate_stream(((x, ready) for _ in range(n)), max_length=T, **kw):
            pass
        return out

    def period(errors):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stream(args.batches, errors)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.batches * 1e3

    head = (f"error_analysis_cost: B={B}, steps={T}, vocab={V}, target tokens min/mean/max = {min(map(len, targets))}/"
            f"{sum(map(len, targets)) / B:.1f}/{max(map(len, targets))}, prediction tokens {min(map(len, preds))}/"
            f"{sum(map(len, preds)) / B:.1f}/{max(map(len, preds))}, {args.batches} batches per timing, {args.rounds} rounds")
    if args.period_only:
        stream(12, None)
        ts = [period(None) for _ in range(args.rounds)]
        print(head)
        print(f"evaluate_stream, ready device tensors, no error analysis ({os.path.abspath(args.package_root)}): median "
              f"{statistics.median(ts):.3f} ms per batch (rounds: {', '.join(f'{t:.3f}' for t in ts)})")
        return

    analysis = M.ErrorAnalysis(V, dev)
    off, on = stream(12, None), stream(12, analysis)
    assert (off["bleu"], off["levenshtein"]) == (on["bleu"], on["levenshtein"]), "the metrics changed under errors="
    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        times["off"].append(period(None))
        times["on"].append(period(analysis))

    # the launches alone: 20 calls queued behind a busy stream, one event pair (profiles/tokenize_cost.py's way)
    p_ids, p_len = M._pack(preds, dev, T)
    t_ids, t_len = M._pack(targets, dev, T)
    C = torch.zeros((V + 1, V + 1), dtype=torch.int32, device=dev)
    L = _lib.lib()
    lev, match, tla = (torch.empty((B, k), dtype=torch.int32, device=dev) for k in (1, 4, 2))
    ops = torch.empty((B, 4), dtype=torch.int32, device=dev)
    top_scratch = torch.empty((L.i2l_confusion_top_scratch_bytes(V),), dtype=torch.uint8, device=dev)
    top_out = torch.empty((4, 1024), dtype=torch.int32, device=dev)
    margins = torch.empty((3, V + 1), dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    sp = lambda: side.cuda_stream
    calls = {
        "i2l_sequence_metrics (sequence_metrics_bp_kernel<3>, width 150)": lambda: L.i2l_sequence_metrics(
            p_ids.data_ptr(), p_len.data_ptr(), T, t_ids.data_ptr(), t_len.data_ptr(), T, B, T, 4, 0, lev.data_ptr(),
            match.data_ptr(), tla.data_ptr(), sp()),
        "i2l_edit_alignment, confusion only (what ErrorAnalysis.update enqueues)": lambda: L.i2l_edit_alignment(
            p_ids.data_ptr(), p_len.data_ptr(), T, t_ids.data_ptr(), t_len.data_ptr(), T, B, V, None, 0, None, None, None,
            C.data_ptr(), sp()),
        "i2l_edit_alignment, ops only": lambda: L.i2l_edit_alignment(
            p_ids.data_ptr(), p_len.data_ptr(), T, t_ids.data_ptr(), t_len.data_ptr(), T, B, V, None, 0, ops.data_ptr(), None,
            None, None, sp()),
        "i2l_confusion_margins (2 launches)": lambda: L.i2l_confusion_margins(
            C.data_ptr(), V, margins[0].data_ptr(), margins[1].data_ptr(), margins[2].data_ptr(), sp()),
        "i2l_confusion_top, substitutions, n = 20 (2 launches)": lambda: L.i2l_confusion_top(
            C.data_ptr(), V, 1, 20, top_scratch.data_ptr(), top_scratch.numel(), top_out[0].data_ptr(), top_out[1].data_ptr(),
            top_out[2].data_ptr(), top_out[3].data_ptr(), sp()),
        "i2l_confusion_top, every kind, n = 1024 (2 launches)": lambda: L.i2l_confusion_top(
            C.data_ptr(), V, 15, 1024, top_scratch.data_ptr(), top_scratch.numel(), top_out[0].data_ptr(), top_out[1].data_ptr(),
            top_out[2].data_ptr(), top_out[3].data_ptr(), sp()),
    }
    busy = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    per_call = {}
    with torch.cuda.stream(side):
        for name, fn in calls.items():
            assert fn() == 0, name
            per_call[name] = []
            for _ in range(5):
                for _ in range(6):
                    busy @ busy                                      # keeps the stream busy while the calls queue up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(20):
                    fn()
                e1.record(side)
                side.synchronize()
                per_call[name].append(e0.elapsed_time(e1) / 20 * 1e3)
    assert int(lev.sum()) == int(ops[:, 1:].sum()), "the script's distance is not the statistics kernel's"

    host, C_host = host_line(preds, targets)
    fresh = M.edit_alignment(preds, targets, V)["confusion"].cpu().numpy()
    assert all(int(fresh[a, b]) == c for (a, b), c in C_host.items()) and int(fresh.sum()) == sum(C_host.values())

    med = {k: statistics.median(v) for k, v in times.items()}
    align_us = statistics.median(per_call["i2l_edit_alignment, confusion only (what ErrorAnalysis.update enqueues)"])
    grew_us = (med["on"] - med["off"]) * 1e3
    lines = [head, ""]
    lines.append(f"evaluate_stream, ready device tensors, errors=None: median {med['off']:.3f} ms per batch (rounds: "
                 f"{', '.join(f'{t:.3f}' for t in times['off'])})")
    lines.append(f"evaluate_stream, ready device tensors, errors=ErrorAnalysis: median {med['on']:.3f} ms per batch (rounds: "
                 f"{', '.join(f'{t:.3f}' for t in times['on'])})")
    verdict = "WORSE than" if grew_us > align_us else "within"
    lines.append(f"the period grew by {grew_us:+.1f} us with errors on; the alignment launch alone takes {align_us:.1f} us: "
                 f"{verdict} the launch's own duration")
    lines.append("")
    for name, ts in per_call.items():
        lines.append(f"{name}, HIP events over 20 queued calls: median {statistics.median(ts):.1f} us per call "
                     f"(runs: {', '.join(f'{t:.1f}' for t in ts)})")
    lines += ["", host]
    text_out = "\n".join(lines) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
