"""What the N-best beam search (i2l_beam_decode_nbest) costs against the entry it extends (i2l_beam_decode_batched, whose
kernels' arithmetic this change does not edit), both in ONE process.

The shipped decoder (V 500, E = H = 512, two layers), 150 steps, once with the END clock in the weights (beams retire
and the searches end early: the list insertions are exercised) and once without it (output weights at 8 / sqrt(H): the
searches run all steps, the rows are leftover rows): images x beam, nbest = 1 x 2, 1 (the reference's default call,
one row: the parent's result), 16 x 5, 5 and 128 x 5, 10 (BASELINE config 2's count, more rows than beams).  The n-best
call ranks by score / length ** 0.7 except at nbest = 1, where it passes no table as the parent's equal.  The routes
alternate; the workspace is prepared once per setting (i2l_decoder_prepare is outside the events); each figure is the
median over --reps launches after --warmup, HIP events on the stream around the call only.

Per-kernel split: run ``rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python profiles/beam_nbest_cost.py
--trace-run`` first (alone, no counters) and pass the csv with --kernel-trace.
usage: python profiles/beam_nbest_cost.py [--reps N] [--warmup W] [--kernel-trace CSV] [--out FILE] | --trace-run"""
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
CLOCK = dict(out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
NO_CLOCK = dict(out_scale=8.0)


def build(dims, dev, seed, **sd_kw):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **dims)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=seed, **sd_kw)
    m = Seq2SeqModel("cnn_lstm", dims["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


class Route:
    """One entry point with its own scratch and outputs for (images, beam, nbest); nbest 0: the parent entry."""

    def __init__(self, name, dec, w, n, k, nbest, dev):
        L = _lib.lib()
        self.name, self.n, self.k, self.nbest, self.dec, self.w = name, n, k, nbest, dec, w
        dims = (dec.vocab_size, dec.hidden_dim, dec.lstm_layers, STEPS)
        self.nbytes = L.i2l_beam_nbest_scratch_bytes(n, k, nbest, *dims) if nbest else L.i2l_beam_batched_scratch_bytes(n, k, *dims)
        assert self.nbytes > 0, name
        rows = max(nbest, 1)
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.seq = torch.empty((n, rows, STEPS + 1), dtype=torch.int32, device=dev)
        self.ln = torch.empty((n, rows), dtype=torch.int32, device=dev)
        self.score = torch.empty((n, rows), dtype=torch.float64, device=dev)
        self.key = torch.empty((n, rows), dtype=torch.float64, device=dev)
        self.fin = torch.empty((n, rows), dtype=torch.int32, device=dev)
        self.count = torch.ones((n,), dtype=torch.int32, device=dev)
        table = [1.0] + [float(i) ** 0.7 for i in range(1, STEPS + 1)]
        self.norm = torch.tensor(table, dtype=torch.float64, device=dev) if nbest > 1 else None

    def __call__(self):
        L = _lib.lib()
        if self.nbest:
            rc = L.i2l_beam_decode_nbest(ctypes.byref(self.w), self.dec._ws.data_ptr(), self.n, self.k, self.nbest, STEPS,
                                         synth.START, synth.END, _lib.ptr(self.norm), self.buf.data_ptr(), self.nbytes,
                                         self.seq.data_ptr(), self.ln.data_ptr(), self.score.data_ptr(), self.key.data_ptr(),
                                         self.fin.data_ptr(), self.count.data_ptr(), 0, _lib.stream_ptr())
        else:
            rc = L.i2l_beam_decode_batched(ctypes.byref(self.w), self.dec._ws.data_ptr(), self.n, self.k, STEPS, synth.START,
                                           synth.END, self.buf.data_ptr(), self.nbytes, self.seq.data_ptr(),
                                           self.ln.data_ptr(), self.score.data_ptr(), 0, _lib.stream_ptr())
        _lib.check(rc, self.name)

    def result(self):
        """(row 0 of every image, steps the longest search executed, rows returned) of one untimed call."""
        self.buf.fill_(255)                                  # both entries keep tokhist (images, T, k) int32 at offset 0
        self()
        torch.cuda.synchronize()
        lens = self.ln[:, 0].cpu().tolist()
        hist = self.buf[: 4 * self.n * STEPS * self.k].view(torch.int32).view(self.n, STEPS, self.k)[:, :, 0]
        executed = int((hist != -1).sum(dim=1).max())
        first = [row[:m] for row, m in zip(self.seq[:, 0].cpu().tolist(), lens)]
        return first, executed, int(self.count.sum())


def measure(m, n, k, nbest, reps, warmup, dev):
    dec = m.decoder
    enc = torch.from_numpy(synth.uniform(13, "enc", (n, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    w, keep, _ = dec.prepare(enc)
    rs = [Route("i2l_beam_decode_batched (one result)", dec, w, n, k, 0, dev),
          Route(f"i2l_beam_decode_nbest, nbest {nbest}", dec, w, n, k, nbest, dev)]
    res = {r.name: r.result() for r in rs}
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
    return [(r.name, statistics.median(times[r.name]), min(times[r.name]), max(times[r.name])) + res[r.name][1:] +
            (sum(a == b for a, b in zip(res[r.name][0], res[rs[0].name][0])),) for r in rs]


def trace_split(path):
    """Mean time per kernel of both entries' launches in a rocprofv3 kernel trace of --trace-run."""
    per = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if any(k in name for k in ("lstm_step_mfma", "logits_mfma", "beam_step_batched", "beam_init_batched",
                                   "beam_final_batched", "beam_nbest")):
            key = f"{name} grid ({r['Grid_Size_X']},{r['Grid_Size_Y']}) / wg {r['Workgroup_Size_X']}"
            per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: (len(v), statistics.mean(v), statistics.median(v)) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None, help="csv of a rocprofv3 --kernel-trace run of --trace-run")
    ap.add_argument("--trace-run", action="store_true",
                    help="only 3 searches of either entry, shipped shape without the END clock, 128 x 5, nbest 10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_nbest_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20 or args.trace_run, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    if args.trace_run:
        m = build(SHIPPED, dev, 100 + 512 // 64 + 34, **NO_CLOCK)
        enc = torch.from_numpy(synth.uniform(13, "enc", (128, 512), -1.5, 1.5)).to(dev)
        w, keep, _ = m.decoder.prepare(enc)
        for r in [Route("parent", m.decoder, w, 128, 5, 0, dev)] * 3 + [Route("nbest", m.decoder, w, 128, 5, 10, dev)] * 3:
            r()
        torch.cuda.synchronize()
        del keep
        return
    lines = [f"beam_nbest_cost: {STEPS} steps; median (min - max) over {args.reps} launches after {args.warmup}, HIP events "
             "around the call, the two entries alternating in one process",
             "'steps executed' = steps of the longest search of the call; 'rows' = hypotheses returned over all images; 'row 0 "
             "equal' = images whose first row is the parent entry's sequence (nbest > 1 ranks by score / length ** 0.7, so its "
             "row 0 is another hypothesis wherever normalisation changes the winner)", ""]
    for what, sd_kw in (("with the END clock", CLOCK), ("without the END clock (out_scale 8)", NO_CLOCK)):
        m = build(SHIPPED, dev, 100 + 512 // 64 + 34, **sd_kw)
        for n, k, nbest in ((1, 2, 1), (16, 5, 5), (128, 5, 10)):
            res = measure(m, n, k, nbest, args.reps, args.warmup, dev)
            lines.append(f"shipped decoder (V 500, E 512, H 512, L 2) {what}, {n} images x beam {k} = {n * k} rows, nbest {nbest}")
            for name, med, lo, hi, executed, rows, same in res:
                lines.append(f"  {name:40s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {executed:3d} steps executed  "
                             f"{rows:5d} rows  row 0 equal {same}/{n}")
            lines.append(f"  nbest / parent = {res[1][1] / res[0][1]:.3f}x")
            lines.append("")
        del m
    if args.kernel_trace:
        split = trace_split(args.kernel_trace)
        lines.append("kernel trace of the shipped decoder without the END clock, 128 x 5, nbest 10, 3 calls of either entry "
                     "(rocprofv3 --kernel-trace; launches, mean us, median us)")
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
