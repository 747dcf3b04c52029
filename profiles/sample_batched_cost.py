"""What the step-batched sampling (i2l_sample_decode_batched, _lib.FLAG_DECODE_BATCHED on LSTMDecoder.sample_steps) costs
against i2l_sample_decode, the row-per-workgroup kernel -- which this change does not edit, so the flag-off figures ARE the
parent commit's.

The shipped decoder (V 500, E = H = 512, two layers), ids only, 150 steps, no stop rule (every row runs every step), rows
1 / 16 / 64 / 256, at (top_k, top_p) = (5, 0.9), the pair a user sets together, and at each mask alone.  Flag off and flag
on alternate inside ONE process; each figure is the median over --reps launches after --warmup, HIP events on the stream
around the sample_steps call (its i2l_decoder_prepare included on both sides alike).  Before any timing the ids of the two
are compared: same seed, same uniforms, so rows part only at fp32 near-ties.  For scale the greedy step-batched loop
(run_steps under the flag, select_batched_kernel as its last launch) is timed beside them.

The selection launch alone: run ``rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python
profiles/sample_batched_cost.py --trace-run`` first and pass the csv with --kernel-trace; the report then gives the mean
time of sample_batched_kernel per mask setting and of select_batched_kernel at 256 rows.
usage: python profiles/sample_batched_cost.py [--reps N] [--warmup W] [--kernel-trace CSV] [--out FILE] | --trace-run"""
import argparse
import csv
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                     # noqa: E402
from img2latex_amd.model import Seq2SeqModel              # noqa: E402

STEPS = 150
SEED = 2024
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
MASKS = [(5, 0.9), (5, 0.0), (0, 0.9)]
TRACE_ROWS = 256


def build(dims, dev):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **dims)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=42, out_scale=8.0)          # flat enough for the masks to keep several columns
    m = Seq2SeqModel("cnn_lstm", dims["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def inputs(rows, dev):
    enc = torch.from_numpy(synth.uniform(9, "enc", (rows, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    return enc, torch.full((rows,), synth.START, dtype=torch.int32, device=dev)


def measure(m, rows, reps, warmup, dev):
    dec = m.decoder
    enc, tok0 = inputs(rows, dev)
    sets = []
    for top_k, top_p in MASKS:
        for name, flags in (("flag off (i2l_sample_decode)", 0), ("flag on (step-batched)", _lib.FLAG_DECODE_BATCHED)):
            sets.append((f"top_k {top_k} top_p {top_p}: {name}", (top_k, top_p),
                         lambda k=top_k, p=top_p, f=flags: dec.sample_steps(enc, STEPS, tok0, 1.0, k, p, SEED,
                                                                            stop=_lib.STOP_NONE, flags=f)[0]))
    sets.append(("greedy, flag on (step-batched, for scale)", None,
                 lambda: dec.run_steps(enc, STEPS, tok0, flags=_lib.FLAG_DECODE_BATCHED)[0]))
    same = {}
    for i in range(0, 2 * len(MASKS), 2):                    # ids first, timing afterwards
        off, on = sets[i][2]().cpu(), sets[i + 1][2]().cpu()
        assert int(on.min()) >= 0 and int(on.max()) < SHIPPED["vocab_size"], sets[i + 1][0]
        same[sets[i][0]] = rows
        same[sets[i + 1][0]] = int((on == off).all(dim=1).sum())
        assert same[sets[i + 1][0]] >= 0.9 * rows, (sets[i + 1][0], same[sets[i + 1][0]], rows)
    times = {name: [] for name, _, _ in sets}
    for i in range(warmup + reps):
        for name, _, run in sets:                           # the settings alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return [(name, mask, statistics.median(times[name]), min(times[name]), max(times[name]), same.get(name))
            for name, mask, _ in sets]


def trace_split(path):
    """Mean time of the selection launches in a rocprofv3 kernel trace of --trace-run, in launch order: the traced run
    samples once per entry of MASKS, then decodes greedily."""
    sample, select = [], []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
        if "sample_batched_kernel" in name:
            sample.append((int(r["Start_Timestamp"]), us))
        elif "select_batched_kernel" in name:
            select.append(us)
    sample = [us for _, us in sorted(sample)]
    assert len(sample) == len(MASKS) * STEPS and len(select) == STEPS, (len(sample), len(select))
    per = {mask: sample[i * STEPS:(i + 1) * STEPS] for i, mask in enumerate(MASKS)}
    return per, select


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None, help="csv of a rocprofv3 --kernel-trace run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="only one flag-on sampling loop per mask setting and one greedy loop, 256 rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_batched_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20 or args.trace_run, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    shipped = build(SHIPPED, dev)
    if args.trace_run:
        enc, tok0 = inputs(TRACE_ROWS, dev)
        for top_k, top_p in MASKS:
            shipped.decoder.sample_steps(enc, STEPS, tok0, 1.0, top_k, top_p, SEED, stop=_lib.STOP_NONE,
                                         flags=_lib.FLAG_DECODE_BATCHED)
        shipped.decoder.run_steps(enc, STEPS, tok0, flags=_lib.FLAG_DECODE_BATCHED)
        torch.cuda.synchronize()
        return
    lines = [f"sample_batched_cost: sampled ids only, {STEPS} steps, temperature 1, no stop rule; median (min - max) over "
             f"{args.reps} launches after {args.warmup}, HIP events around sample_steps, all settings alternating in one process",
             "'rows equal' = rows whose ids equal i2l_sample_decode's end to end at the same seed (the others part at fp32 "
             "near-ties)", ""]
    slower = []
    for rows in (1, 16, 64, 256):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), {rows} rows")
        res = measure(shipped, rows, args.reps, args.warmup, dev)
        for name, mask, med, lo, hi, same in res:
            eq = "" if same is None else f"  rows equal {same}/{rows}"
            lines.append(f"  {name:55s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {med * 1e3 / STEPS:7.1f} us/step{eq}")
        for i in range(0, 2 * len(MASKS), 2):
            off, on = res[i][2], res[i + 1][2]
            lines.append(f"  top_k {res[i][1][0]} top_p {res[i][1][1]}: flag-off / flag-on = {off / on:.2f}x")
            if on > off:
                slower.append((rows, res[i][1]))
        lines.append("")
    lines.append("the step-batched path is slower at: " + (", ".join(f"{r} rows {m}" for r, m in slower) if slower else
                                                           "none of the four row counts, at none of the mask settings"))
    lines.append("")
    if args.kernel_trace:
        per, select = trace_split(args.kernel_trace)
        lines.append(f"selection launch alone, shipped decoder at {TRACE_ROWS} rows (rocprofv3 --kernel-trace of one loop each; "
                     f"{STEPS} launches; mean us, median us)")
        for mask in MASKS:
            lines.append(f"  sample_batched_kernel top_k {mask[0]} top_p {mask[1]}, grid {TRACE_ROWS} x 256 threads"
                         f" {statistics.mean(per[mask]):8.2f} {statistics.median(per[mask]):8.2f}")
        lines.append(f"  select_batched_kernel (greedy), grid {TRACE_ROWS // 4} x 256 threads              "
                     f" {statistics.mean(select):8.2f} {statistics.median(select):8.2f}")
    else:
        lines.append("no kernel trace was taken: the selection launch alone was not measured")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
