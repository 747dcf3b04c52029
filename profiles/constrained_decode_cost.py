"""What the bracket constraint costs on the step-batched decode: i2l_greedy_decode_constrained against
i2l_greedy_decode_batched and i2l_sample_decode_constrained against i2l_sample_decode_batched -- the plain entries' kernels
are the parent commit's (sample_row gained a predicate that is the constant `true` there).

The shipped decoder (V 500, E = H = 512, two layers), ids only, 150 steps, no stop rule (every row runs every step), rows
256 / 16 / 1.  The table has three kinds -- six bracket columns, PAD / START / UNK never, the rest neutral -- and the output
bias favours the bracket columns, so that the mask has work to do.  Plain and constrained alternate inside ONE process;
each figure is the median over --reps launches after --warmup, HIP events on the stream around the run_steps /
sample_steps call (its i2l_decoder_prepare included on both sides alike).  Before any timing every constrained row is
checked to be well formed.  No threshold: the ratios are what the README row carries.
usage: python profiles/constrained_decode_cost.py [--reps N] [--warmup W] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                              # noqa: E402
from img2latex_amd.model import Seq2SeqModel                       # noqa: E402
from img2latex_amd.training.constraint import BracketTable, close_class, open_class   # noqa: E402

STEPS = 150
SEED = 2024
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
MASK = (5, 0.9)
FLAG = _lib.FLAG_DECODE_BATCHED


def table():
    classes = np.zeros(SHIPPED["vocab_size"], dtype=np.uint8)
    classes[[synth.PAD, synth.START, synth.UNK]] = 255
    for k in range(3):
        classes[4 + 2 * k], classes[5 + 2 * k] = open_class(k), close_class(k)
    return BracketTable(classes, synth.END)


def build(dev):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **SHIPPED)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=42, out_scale=8.0)
    sd["decoder.output_layer.bias"][4:10] += np.float32(2.0)
    m = Seq2SeqModel("cnn_lstm", SHIPPED["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def measure(m, rows, reps, warmup, dev, tab):
    dec = m.decoder
    enc = torch.from_numpy(synth.uniform(9, "enc", (rows, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    tok0 = torch.full((rows,), synth.START, dtype=torch.int32, device=dev)
    sets = [
        ("greedy, i2l_greedy_decode_batched", lambda: dec.run_steps(enc, STEPS, tok0, end_id=synth.END, flags=FLAG)[0]),
        ("greedy, i2l_greedy_decode_constrained", lambda: dec.run_steps(enc, STEPS, tok0, end_id=synth.END, constraint=tab)[0]),
        (f"top_k {MASK[0]} top_p {MASK[1]}, i2l_sample_decode_batched",
         lambda: dec.sample_steps(enc, STEPS, tok0, 1.0, MASK[0], MASK[1], SEED, stop=_lib.STOP_NONE, end_id=synth.END, flags=FLAG)[0]),
        (f"top_k {MASK[0]} top_p {MASK[1]}, i2l_sample_decode_constrained",
         lambda: dec.sample_steps(enc, STEPS, tok0, 1.0, MASK[0], MASK[1], SEED, stop=_lib.STOP_NONE, end_id=synth.END, constraint=tab)[0]),
    ]
    formed = {}
    for name, run in sets:                                       # ids first, timing afterwards
        ids = run().cpu().numpy()
        formed[name] = sum(tab.well_formed(r.tolist()) for r in ids)
        if "constrained" in name:
            assert formed[name] == rows, (name, formed[name], rows)
    times = {name: [] for name, _ in sets}
    for i in range(warmup + reps):
        for name, run in sets:                                   # the settings alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return [(name, statistics.median(times[name]), min(times[name]), max(times[name]), formed[name]) for name, _ in sets]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_decode_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    m, tab = build(dev), table()
    lines = [f"constrained_decode_cost: ids only, {STEPS} steps, temperature 1, no stop rule; median (min - max) over "
             f"{args.reps} launches after {args.warmup}, HIP events around run_steps / sample_steps, all settings alternating "
             "in one process", "'well formed' = rows of the timed call's ids that nest and end on END", ""]
    for rows in (256, 16, 1):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), {rows} rows")
        res = measure(m, rows, args.reps, args.warmup, dev, tab)
        for name, med, lo, hi, formed in res:
            lines.append(f"  {name:55s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {med * 1e3 / STEPS:7.1f} us/step"
                         f"  well formed {formed}/{rows}")
        lines.append(f"  greedy:   constrained / plain = {res[1][1] / res[0][1]:.3f}x")
        lines.append(f"  sampling: constrained / plain = {res[3][1] / res[2][1]:.3f}x")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
