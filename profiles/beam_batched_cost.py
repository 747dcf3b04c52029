"""What the step-batched matrix-core beam search (i2l_beam_decode_batched, _lib.FLAG_BEAM_BATCHED) costs against the
kernels i2l_beam_decode picks -- which this change does not edit, so the flag-off columns ARE the parent commit's.

The shipped decoder (V 500, E = H = 512, two layers), 150 steps, once with the END clock in the weights (searches end
early) and once without it (output weights at 8 / sqrt(H): the searches run all steps): images x beam = 1 x 2 (the
reference's default call), 16 x 5, 128 x 2, 128 x 5 (BASELINE config 2's count) and 128 x 8 (flag on only: beam_kernel<8>
does not fit in LDS at this shape).  The same at the headline dimensions (V 512, E = H = 256, one layer), 128 x 5, against
both beam_group_kernel and beam_kernel: to record where the grouped kernel stays the right choice.  Both routes alternate
inside ONE process; the workspace is prepared once per setting (i2l_decoder_prepare is outside the events); each figure
is the median over --reps launches after --warmup, HIP events on the stream around the call only.  The steps a call
executed are read from its token history (the region is filled with -1 before an untimed call): the longest search.

Per-kernel split: run ``rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python profiles/beam_batched_cost.py
--trace-run`` first (alone, no counters) and pass the csv with --kernel-trace.
usage: python profiles/beam_batched_cost.py [--reps N] [--warmup W] [--kernel-trace CSV] [--out FILE] | --trace-run"""
import argparse
import csv
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                     # noqa: E402
from img2latex_amd.model import Seq2SeqModel              # noqa: E402

STEPS = 150
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
HEADLINE = dict(vocab_size=512, embedding_dim=256, hidden_dim=256, lstm_layers=1, attention=True)
CLOCK = dict(out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
NO_CLOCK = dict(out_scale=8.0)


def build(dims, dev, seed, **sd_kw):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **dims)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=seed, **sd_kw)
    m = Seq2SeqModel("cnn_lstm", dims["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


class Route:
    """One entry point with its own scratch and outputs for (images, beam)."""

    def __init__(self, name, dec, w, n, k, dev, batched, flags=0):
        L = _lib.lib()
        self.name, self.n, self.k, self.batched, self.flags = name, n, k, batched, flags
        self.dec, self.w = dec, w
        if batched:
            self.nbytes = L.i2l_beam_batched_scratch_bytes(n, k, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, STEPS)
        else:
            self.nbytes = L.i2l_beam_workspace_bytes(n, k, dec.hidden_dim, dec.lstm_layers, STEPS)
        assert self.nbytes > 0, name
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.seq = torch.empty((n, STEPS + 1), dtype=torch.int32, device=dev)
        self.ln = torch.empty((n,), dtype=torch.int32, device=dev)
        self.score = torch.empty((n,), dtype=torch.float64, device=dev)

    def __call__(self):
        fn = _lib.lib().i2l_beam_decode_batched if self.batched else _lib.lib().i2l_beam_decode
        _lib.check(fn(ctypes.byref(self.w), self.dec._ws.data_ptr(), self.n, self.k, STEPS, synth.START, synth.END,
                      self.buf.data_ptr(), self.nbytes, self.seq.data_ptr(), self.ln.data_ptr(), self.score.data_ptr(),
                      self.flags, _lib.stream_ptr()), self.name)

    def result(self):
        """(sequences, steps the longest search executed) of one untimed call."""
        self.buf.fill_(255)                                  # both routes keep tokhist (images, T, k) int32 at offset 0
        self()
        torch.cuda.synchronize()
        lens = self.ln.cpu().tolist()
        assert min(lens) >= 0, (self.name, "a grouped poll timed out")
        hist = self.buf[: 4 * self.n * STEPS * self.k].view(torch.int32).view(self.n, STEPS, self.k)[:, :, 0]
        executed = int((hist != -1).sum(dim=1).max())
        return [row[:m] for row, m in zip(self.seq.cpu().tolist(), lens)], executed


def measure(m, dims, n, k, routes, reps, warmup, dev):
    dec = m.decoder
    enc = torch.from_numpy(synth.uniform(13, "enc", (n, dims["embedding_dim"]), -1.5, 1.5)).to(dev)
    w, keep, _ = dec.prepare(enc)
    rs = [Route(name, dec, w, n, k, dev, batched, flags) for name, batched, flags in routes]
    res = {r.name: r.result() for r in rs}
    base = res[rs[0].name][0]
    times = {r.name: [] for r in rs}
    for i in range(warmup + reps):
        for r in rs:                                         # the routes alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[r.name].append(e0.elapsed_time(e1))
    del keep
    out = []
    for r in rs:
        seqs, executed = res[r.name]
        same = sum(a == b for a, b in zip(seqs, base))
        t = times[r.name]
        out.append((r.name, statistics.median(t), min(t), max(t), executed, same))
    return out


def report(lines, title, res, n, first_is_reference=True):
    lines.append(title)
    for name, med, lo, hi, executed, same in res:
        eq = f"images equal {same}/{n}" if first_is_reference else "no flag-off route at this shape"
        lines.append(f"  {name:42s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {executed:3d} steps executed "
                     f"{med * 1e3 / max(executed, 1):7.1f} us/step  {eq}")
    if len(res) > 1:
        on = res[-1][1]
        for name, med, *_ in res[:-1]:
            lines.append(f"  {name} / flag on = {med / on:.2f}x")
    lines.append("")


def trace_split(path):
    """Mean time per kernel of the step-batched launches in a rocprofv3 kernel trace of --trace-run."""
    per = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if any(k in name for k in ("lstm_step_mfma", "logits_mfma", "beam_step_batched", "beam_init_batched",
                                   "beam_final_batched", "beam_kernel")):
            key = f"{name} grid ({r['Grid_Size_X']},{r['Grid_Size_Y']}) / wg {r['Workgroup_Size_X']}"
            per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: (len(v), statistics.mean(v), statistics.median(v)) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None, help="csv of a rocprofv3 --kernel-trace run of --trace-run")
    ap.add_argument("--trace-run", action="store_true", help="only 4 flag-on and 2 flag-off searches, shipped shape without the END clock, 128 x 5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_batched_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20 or args.trace_run, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    seed = 100 + 512 // 64 + 34
    off = ("flag off (beam_kernel: a workgroup per image)", False, 0)
    on = ("flag on (step-batched)", True, _lib.FLAG_BEAM_BATCHED)
    if args.trace_run:
        m = build(SHIPPED, dev, seed, **NO_CLOCK)
        enc = torch.from_numpy(synth.uniform(13, "enc", (128, 512), -1.5, 1.5)).to(dev)
        w, keep, _ = m.decoder.prepare(enc)
        for r in [Route(on[0], m.decoder, w, 128, 5, dev, True)] * 4 + [Route(off[0], m.decoder, w, 128, 5, dev, False)] * 2:
            r()
        torch.cuda.synchronize()
        del keep
        return
    lines = [f"beam_batched_cost: {STEPS} steps; median (min - max) over {args.reps} launches after {args.warmup}, HIP events "
             "around the call, the routes alternating in one process",
             "'steps executed' = steps of the longest search of the call; us/step = median / steps executed; 'images equal' = "
             "images whose sequence equals the one of the setting's first route (the others part at fp32 near-ties)", ""]
    for what, sd_kw in (("with the END clock", CLOCK), ("without the END clock (out_scale 8)", NO_CLOCK)):
        m = build(SHIPPED, dev, seed, **sd_kw)
        for n, k in ((1, 2), (16, 5), (128, 2), (128, 5), (128, 8)):
            routes = [on] if k == 8 else [off, on]
            res = measure(m, SHIPPED, n, k, routes, args.reps, args.warmup, dev)
            report(lines, f"shipped decoder (V 500, E 512, H 512, L 2) {what}, {n} images x beam {k} = {n * k} rows", res, n, k != 8)
        del m
    head = build(HEADLINE, dev, 42, **CLOCK)
    routes = [("flag off (beam_group_kernel: 4 workgroups share 12 slots)", False, 0),
              ("flag off, FLAG_NO_GROUP (beam_kernel)", False, _lib.FLAG_NO_GROUP), on]
    res = measure(head, HEADLINE, 128, 5, routes, args.reps, args.warmup, dev)
    report(lines, "headline dimensions (V 512, E 256, H 256, L 1) with the END clock, 128 images x beam 5 = 640 rows", res, 128)
    if args.kernel_trace:
        split = trace_split(args.kernel_trace)
        lines.append("kernel trace of the shipped decoder without the END clock, 128 x 5 (rocprofv3 --kernel-trace; launches, mean us, median us)")
        for k in sorted(split):
            cnt, mean, med = split[k]
            lines.append(f"  {k:75s} {cnt:6d} {mean:8.2f} {med:8.2f}")
    else:
        lines.append("no kernel trace was taken: per-kernel split not measured")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
