"""What the argument rules cost on the step-batched decode, over the bracket constraint: i2l_greedy_decode_arguments
against i2l_greedy_decode_constrained against i2l_greedy_decode_batched, and the three sampling entries alike.  The
yardstick is the bracket-constrained entry in the same process: the argument rules' extra cost per step over it should
not exceed the bracket entry's own extra cost over the unconstrained loop.

The shipped decoder (V 500, E = H = 512, two layers), ids only, 150 steps, no stop rule (every row runs every step), rows
256 / 16 / 1.  The table has three bracket kinds, PAD / START / UNK never, a \\frac-like column (2 strict), a ^-like one
(1 loose), a \\binom-like one (2 loose), one that demands 3 strict groups, and the environment opener demands one strict
argument; the output bias favours all of them, so that the masks have work to do.  The bracket run uses the same table
without its argument bits.  The three settings alternate inside ONE process; each figure is the median over --reps
launches after --warmup, HIP events on the stream around the run_steps / sample_steps call (its i2l_decoder_prepare
included on every side alike).  Before any timing the share of complete rows is counted for all three, and every
argument-constrained row is checked to be complete.  No threshold: the figures are what the README row carries.
usage: python profiles/arguments_decode_cost.py [--reps N] [--warmup W] [--out FILE]"""
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
from img2latex_amd.training.constraint import (ArgumentTable, BracketTable, argument_byte, close_class,   # noqa: E402
                                               open_class)

STEPS = 150
SEED = 2024
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
MASK = (5, 0.9)
FLAG = _lib.FLAG_DECODE_BATCHED
KINDS = ("unconstrained", "brackets", "arguments")


def tables():
    t = np.zeros(SHIPPED["vocab_size"], dtype=np.uint8)
    t[[synth.PAD, synth.START, synth.UNK]] = 255
    for k in range(3):
        t[4 + 2 * k], t[5 + 2 * k] = open_class(k), close_class(k)
    t[8] = argument_byte(open_class(2), 1)
    t[10], t[11], t[12], t[13] = argument_byte(0, 2), argument_byte(0, 1, True), argument_byte(0, 2, True), argument_byte(0, 3)
    arguments = ArgumentTable(t, synth.END)
    return BracketTable(arguments.classes, synth.END), arguments


def build(dev):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **SHIPPED)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=42, out_scale=8.0)
    sd["decoder.output_layer.bias"][4:14] += np.float32(2.0)
    m = Seq2SeqModel("cnn_lstm", SHIPPED["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def measure(m, rows, reps, warmup, dev, brackets, arguments):
    dec = m.decoder
    enc = torch.from_numpy(synth.uniform(9, "enc", (rows, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    tok0 = torch.full((rows,), synth.START, dtype=torch.int32, device=dev)
    how = {"unconstrained": dict(flags=FLAG), "brackets": dict(constraint=brackets), "arguments": dict(constraint=arguments)}
    sets = []
    for kind in KINDS:
        sets.append(("greedy", kind, lambda kw=how[kind]: dec.run_steps(enc, STEPS, tok0, end_id=synth.END, **kw)[0]))
    for kind in KINDS:
        sets.append((f"top_k {MASK[0]} top_p {MASK[1]}", kind,
                     lambda kw=how[kind]: dec.sample_steps(enc, STEPS, tok0, 1.0, MASK[0], MASK[1], SEED, stop=_lib.STOP_NONE,
                                                           end_id=synth.END, **kw)[0]))
    complete = {}
    for mode, kind, run in sets:                                 # ids first, timing afterwards
        ids = run().cpu().numpy()
        complete[mode, kind] = sum(arguments.complete(r.tolist()) for r in ids)
        if kind == "arguments":
            assert complete[mode, kind] == rows, (mode, complete[mode, kind], rows)
        if kind == "brackets":
            assert all(brackets.well_formed(r.tolist()) for r in ids), mode
    times = {(mode, kind): [] for mode, kind, _ in sets}
    for i in range(warmup + reps):
        for mode, kind, run in sets:                             # the settings alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[mode, kind].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v), complete[k]) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arguments_decode_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    m = build(dev)
    brackets, arguments = tables()
    lines = [f"arguments_decode_cost: ids only, {STEPS} steps, temperature 1, no stop rule; median (min - max) over "
             f"{args.reps} launches after {args.warmup}, HIP events around run_steps / sample_steps, all settings alternating "
             "in one process", "'complete' = rows of the timed call's ids that nest, end on END and give every command its "
             "arguments", ""]
    for rows in (256, 16, 1):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), {rows} rows")
        res = measure(m, rows, args.reps, args.warmup, dev, brackets, arguments)
        for mode in ("greedy", f"top_k {MASK[0]} top_p {MASK[1]}"):
            for kind in KINDS:
                med, lo, hi, done = res[mode, kind]
                lines.append(f"  {mode + ', ' + kind:40s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {med * 1e3 / STEPS:7.2f} us/step"
                             f"  complete {done}/{rows}")
            free, br, ar = (res[mode, k][0] * 1e3 / STEPS for k in KINDS)
            lines.append(f"  {mode}: brackets over unconstrained {br - free:+.2f} us/step, arguments over brackets "
                         f"{ar - br:+.2f} us/step" + ("" if ar - br <= br - free else "  (MORE than the bracket constraint's own cost)"))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
