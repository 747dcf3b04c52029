"""What the step-batched training recurrences (_lib.FLAG_TRAIN_BATCHED) cost against the recurrences the library picks
without the flag -- which this change does not edit, so the flag-off columns ARE the parent commit's.

The shipped decoder (V 500, E = H = 512, two layers, dropout 0.3, train mode), T = 149 input tokens, B = 16 / 64 / 256:
the forward call (i2l_decoder_train_fwd), the backward call (i2l_decoder_train_bwd) and a whole TrainStep.step (a tiny CNN
encoder on 16 x 32 images in front, so that the step is the decoder's plus loss, clip and Adam), flag off (row kernels)
against flag on.  One line at the headline dimensions (V 512, E = H = 256, one layer) at B = 64, where flag off is the
grouped recurrences.  All settings alternate inside ONE process; each figure is the median (min - max) over --reps calls
after --warmup, HIP events on the stream around the call.  Before any timing the logits and gradients of the two paths
are compared.

Per-kernel means: run ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python
profiles/train_batched_cost.py --trace-run`` in a run of its own and pass the kernel-trace csv with --kernel-trace.
usage: python profiles/train_batched_cost.py [--reps N] [--warmup W] [--kernel-trace CSV] [--out FILE] | --trace-run"""
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
from img2latex_amd.model._train_fn import decoder_train_backward, decoder_train_forward   # noqa: E402
from img2latex_amd.training import TrainStep              # noqa: E402

T = 149
FLAG = _lib.FLAG_TRAIN_BATCHED
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True, dropout=0.3)
HEADLINE = dict(vocab_size=512, embedding_dim=256, hidden_dim=256, lstm_layers=1, attention=False, dropout=0.3)
SETTINGS = [("flag off", 0), ("flag on (step-batched)", FLAG)]


def build(dims, dev):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **dims)
    sd = synth.make_state_dict(cfg, seed=42, out_scale=12.0)
    m = Seq2SeqModel("cnn_lstm", dims["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).train(), cfg


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def fmt(name, v):
    return f"  {name:32s} {statistics.median(v):9.3f} ms ({min(v):.3f} - {max(v):.3f})"


def measure(m, cfg, dims, B, reps, warmup, dev, whole_step=True):
    dec = m.decoder
    V = dims["vocab_size"]
    enc = torch.from_numpy(synth.uniform(9, "enc", (B, dims["embedding_dim"]), -1.5, 1.5)).to(dev)
    toks = torch.from_numpy(synth.randint(10, "tok", (B, T), 0, V)).to(dev, torch.int32).contiguous()
    dlogits = torch.from_numpy(synth.uniform(11, "dlogits", (B, T, V), -1e-2, 1e-2)).to(dev)
    grads = {n: torch.empty_like(p) for n, p in dec.named_parameters()}

    def fwd(flags):
        dec.kernel_flags = flags
        try:
            return decoder_train_forward(dec, enc, toks, seed=5)
        finally:
            dec.kernel_flags = 0

    def bwd(state):
        return decoder_train_backward(dec, state, dlogits, grads)

    got = {}
    for name, flags in SETTINGS:                            # numbers first, timing afterwards
        logits, state = fwd(flags)
        denc = bwd(state)
        torch.cuda.synchronize()
        got[name] = (logits.clone(), denc.clone(), {n: g.clone() for n, g in grads.items()})
    (l0, d0, g0), (l1, d1, g1) = got["flag off"], got[SETTINGS[1][0]]
    dl = float((l0 - l1).abs().max())
    dg = max(float((g0[n] - g1[n]).abs().max()) / max(float(g0[n].abs().max()), 1e-12) for n in g0 if not n.startswith("attention."))
    assert dl <= 2e-4 and dg <= 4e-4, (dl, dg)
    times = {(name, what): [] for name, _ in SETTINGS for what in ("forward", "backward", "step")}
    steps = {}
    if whole_step:
        x = torch.from_numpy(synth.make_images(B, cfg, seed=3)).to(dev)
        forms = torch.from_numpy(synth.make_formulas(B, T + 1, V, seed=4)).to(dev)
        for name, flags in SETTINGS:
            mm, _ = build(dims, dev)
            mm.decoder.kernel_flags = flags
            steps[name] = TrainStep(mm, seed=11)
    for i in range(warmup + reps):
        for name, flags in SETTINGS:                        # the settings alternate
            tf, (_, state) = timed(lambda: fwd(flags))
            tb, _ = timed(lambda: bwd(state))
            ts = timed(lambda: steps[name].step(x, forms))[0] if whole_step else 0.0
            if i >= warmup:
                times[(name, "forward")].append(tf)
                times[(name, "backward")].append(tb)
                times[(name, "step")].append(ts)
    lines = [f"    max |logits on - off| {dl:.2e}, max gradient difference {dg:.2e} of max|off|"]
    for what in ("forward", "backward") + (("step",) if whole_step else ()):
        for name, _ in SETTINGS:
            lines.append(fmt(f"{what:9s}{name}", times[(name, what)]))
        off, on = (statistics.median(times[(name, what)]) for name, _ in SETTINGS)
        lines.append(f"  {what}: flag off / flag on = {off / on:.2f}x")
    return lines


def trace_split(path):
    """Mean time per launch of the recurrence kernels in a rocprofv3 kernel trace of --trace-run."""
    per = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if "lstm_train" in name:
            key = (f"{name} grid ({r['Grid_Size_X']},{r['Grid_Size_Y']},{r['Grid_Size_Z']}) / wg {r['Workgroup_Size_X']}")
            per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: (len(v), statistics.mean(v), statistics.median(v)) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None, help="csv of a rocprofv3 --kernel-trace run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="only 2 flag-on and 1 flag-off forward + backward, shipped shape, B = 64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batched_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20 or args.trace_run, "medians over at least 20 calls"
    dev = torch.device("cuda:0")
    shipped, cfg = build(SHIPPED, dev)
    if args.trace_run:
        dec = shipped.decoder
        enc = torch.from_numpy(synth.uniform(9, "enc", (64, 512), -1.5, 1.5)).to(dev)
        toks = torch.from_numpy(synth.randint(10, "tok", (64, T), 0, 500)).to(dev, torch.int32).contiguous()
        dlogits = torch.from_numpy(synth.uniform(11, "dlogits", (64, T, 500), -1e-2, 1e-2)).to(dev)
        grads = {n: torch.empty_like(p) for n, p in dec.named_parameters()}
        for flags in (FLAG, FLAG, 0):
            dec.kernel_flags = flags
            _, state = decoder_train_forward(dec, enc, toks, seed=5)
            decoder_train_backward(dec, state, dlogits, grads)
            dec.kernel_flags = 0
        torch.cuda.synchronize()
        return
    lines = [f"train_batched_cost: train mode, dropout 0.3, T = {T}; median (min - max) over {args.reps} calls after {args.warmup}, "
             "HIP events around the call, the two settings alternating in one process",
             "forward = i2l_decoder_train_fwd, backward = i2l_decoder_train_bwd (no side lanes), step = TrainStep.step with a "
             "tiny CNN encoder (16 x 32 images) in front", ""]
    for B in (16, 64, 256):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), B = {B}")
        lines += measure(shipped, cfg, SHIPPED, B, args.reps, args.warmup, dev)
        lines.append("")
    head, hcfg = build(HEADLINE, dev)
    lines.append("headline dimensions (V 512, E 256, H 256, L 1), B = 64: flag off = the grouped recurrences")
    lines += measure(head, hcfg, HEADLINE, 64, args.reps, args.warmup, dev, whole_step=False)
    lines.append("")
    if args.kernel_trace:
        lines.append("kernel trace, shipped decoder, B = 64, two flag-on and one flag-off forward + backward (rocprofv3 --kernel-trace --stats, "
                     "a run of its own; launches, mean us, median us)")
        split = trace_split(args.kernel_trace)
        for k in sorted(split):
            n, mean, med = split[k]
            lines.append(f"  {k:90s} {n:6d} {mean:9.2f} {med:9.2f}")
    else:
        lines.append("no kernel trace was taken: per-kernel means not measured")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
