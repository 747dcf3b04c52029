"""What the step-batched matrix-core decode (i2l_greedy_decode_batched, _lib.FLAG_DECODE_BATCHED) costs against the kernels
the library picks without the flag -- which this change does not edit, so the flag-off columns ARE the parent commit's.

The shipped decoder (V 500, E = H = 512, two layers), greedy ids only, 150 steps, no stop rule (every row runs every step),
rows 1 / 16 / 64 / 256: flag off at rows_per_workgroup 0 (automatic), 1, 2, 4 and flag on.  The same at the headline
dimensions (V 512, E = H = 256, one layer) at 256 rows, where flag off with rows_per_workgroup 0 is the 4-member grouped
kernel and FLAG_DECODE_GROUP8 / _GROUP16 the 8- and 16-member ones: to record where those still win.  All settings
alternate inside ONE process; the workspace is prepared once per batch (i2l_decoder_prepare is outside the events); each
figure is the median over --reps launches after --warmup, HIP events on the stream around the decode call only.  Before
any timing the ids of every setting are compared with the automatic flag-off ids.

Per-kernel split: run ``rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python profiles/decode_batched_cost.py
--trace-run`` first and pass the csv with --kernel-trace; the report then gives each kernel's mean time and the part of a
step no kernel accounts for (the launch gaps).
usage: python profiles/decode_batched_cost.py [--reps N] [--warmup W] [--kernel-trace CSV] [--out FILE] | --trace-run"""
import argparse
import csv
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                     # noqa: E402
from img2latex_amd.model import Seq2SeqModel              # noqa: E402

STEPS = 150
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
HEADLINE = dict(vocab_size=512, embedding_dim=256, hidden_dim=256, lstm_layers=1, attention=False)


def build(dims, dev):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **dims)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=42, out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
    m = Seq2SeqModel("cnn_lstm", dims["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def settings(headline):
    s = [("flag off, rows_per_workgroup 0" + (" (4-member grouped kernel)" if headline else " (automatic)"), dict()),
         ("flag off, rows_per_workgroup 1", dict(rows_per_workgroup=1)),
         ("flag off, rows_per_workgroup 2", dict(rows_per_workgroup=2)),
         ("flag off, rows_per_workgroup 4", dict(rows_per_workgroup=4))]
    if headline:
        s += [("flag off, FLAG_DECODE_GROUP8", dict(flags=_lib.FLAG_DECODE_GROUP8)),
              ("flag off, FLAG_DECODE_GROUP16", dict(flags=_lib.FLAG_DECODE_GROUP16))]
    return s + [("flag on (step-batched)", dict(flags=_lib.FLAG_DECODE_BATCHED))]


def measure(m, dims, rows, reps, warmup, headline, dev):
    dec = m.decoder
    enc = torch.from_numpy(synth.uniform(9, "enc", (rows, dims["embedding_dim"]), -1.5, 1.5)).to(dev)
    tok0 = torch.full((rows,), synth.START, dtype=torch.int32, device=dev)
    w, keep, enc_c = dec.prepare(enc)
    prepared = (w, keep, enc_c, dec._ws)
    sets = settings(headline)
    run = lambda kw: dec.run_steps(enc, STEPS, tok0, prepared=prepared, **kw)[0]      # noqa: E731
    base = _lib.check_ids(run(sets[0][1]).cpu())
    same = {}
    for name, kw in sets:                                   # ids first, timing afterwards
        ids = _lib.check_ids(run(kw).cpu())
        assert int(ids.min()) >= 0 and int(ids.max()) < dims["vocab_size"], name
        same[name] = int((ids == base).all(dim=1).sum())
        assert same[name] >= 0.9 * rows, (name, same[name], rows)      # rows part only at fp32 near-ties
    times = {name: [] for name, _ in sets}
    for i in range(warmup + reps):
        for name, kw in sets:                               # the settings alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kw)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    del keep
    return [(name, statistics.median(times[name]), min(times[name]), max(times[name]), same[name]) for name, _ in sets]


def trace_split(path):
    """Mean time per kernel of the step-batched launches in a rocprofv3 kernel trace of --trace-run."""
    per = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if any(k in name for k in ("lstm_step_mfma", "logits_mfma", "select_batched", "init_batched", "decode_kernel")):
            key = f"{name} grid ({r['Grid_Size_X']},{r['Grid_Size_Y']}) / wg {r['Workgroup_Size_X']}"
            per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: (len(v), statistics.mean(v), statistics.median(v)) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None, help="csv of a rocprofv3 --kernel-trace run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="only 4 flag-on and 2 flag-off decodes of the shipped shape, 256 rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_batched_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20 or args.trace_run, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    shipped = build(SHIPPED, dev)
    if args.trace_run:
        enc = torch.from_numpy(synth.uniform(9, "enc", (256, 512), -1.5, 1.5)).to(dev)
        tok0 = torch.full((256,), synth.START, dtype=torch.int32, device=dev)
        for kw in [dict(flags=_lib.FLAG_DECODE_BATCHED)] * 4 + [dict()] * 2:
            shipped.decoder.run_steps(enc, STEPS, tok0, **kw)
        torch.cuda.synchronize()
        return
    lines = [f"decode_batched_cost: greedy ids only, {STEPS} steps, no stop rule; median (min - max) over {args.reps} launches "
             f"after {args.warmup}, HIP events around the decode call, all settings alternating in one process",
             "'rows equal' = rows whose ids equal the automatic flag-off ids end to end (the others part at fp32 near-ties)", ""]
    best = {}
    for rows in (1, 16, 64, 256):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), {rows} rows")
        res = measure(shipped, SHIPPED, rows, args.reps, args.warmup, False, dev)
        for name, med, lo, hi, same in res:
            lines.append(f"  {name:45s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {rows * STEPS / med / 1e3:8.3f} M tokens/s"
                         f"  {med * 1e3 / STEPS:7.1f} us/step  rows equal {same}/{rows}")
        off = min(med for name, med, *_ in res if name.startswith("flag off"))
        on = next(med for name, med, *_ in res if name.startswith("flag on"))
        best[rows] = (off, on)
        lines.append(f"  best flag-off / flag-on = {off / on:.2f}x")
        lines.append("")
    head = build(HEADLINE, dev)
    lines.append("headline dimensions (V 512, E 256, H 256, L 1), 256 rows")
    for name, med, lo, hi, same in measure(head, HEADLINE, 256, args.reps, args.warmup, True, dev):
        lines.append(f"  {name:45s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {256 * STEPS / med / 1e3:8.3f} M tokens/s"
                     f"  {med * 1e3 / STEPS:7.1f} us/step  rows equal {same}/256")
    lines.append("")
    if args.kernel_trace:
        split = trace_split(args.kernel_trace)
        lines.append("kernel trace of the shipped decoder at 256 rows (rocprofv3 --kernel-trace; launches, mean us, median us)")
        step = 0.0
        for k in sorted(split):
            n, mean, med = split[k]
            lines.append(f"  {k:75s} {n:6d} {mean:8.2f} {med:8.2f}")
            if any(s in k for s in ("lstm_step_mfma", "logits_mfma", "select_batched")):
                step += mean * n / (4 * STEPS)              # four traced flag-on decodes
        off, on = best[256]
        lines.append(f"  kernels of one flag-on step: {step:.1f} us of the {on * 1e3 / STEPS:.1f} us a step takes on the stream; "
                     f"the rest ({on * 1e3 / STEPS - step:.1f} us) is what the {SHIPPED['lstm_layers'] + 2} launch boundaries cost")
    else:
        lines.append("no kernel trace was taken: per-kernel split not measured")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
