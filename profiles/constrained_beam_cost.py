"""What the bracket constraint costs inside the N-best beam search: i2l_beam_decode_nbest_constrained against
i2l_beam_decode_nbest, whose kernels are the parent commit's (beam_topk_row gained a pick policy that is the constant
`true` there), both in ONE process.

The shipped decoder (V 500, E = H = 512, two layers), 150 steps, the bracket-biased synthetic weights and the table of
constrained_decode_cost.py (three kinds on six columns, PAD / START / UNK never, the output bias favouring the bracket
columns, so that the mask has work to do): images x beam = 1 x 2, 16 x 5 and 128 x 5, nbest = beam, ranked by
score / length ** 0.7.  The two entries alternate; the workspace is prepared once per setting (i2l_decoder_prepare is
outside the events); each figure is the median over --reps launches after --warmup, HIP events on the stream around the
call only.  Before any timing every constrained row is checked to be well formed, and the share of well-formed rows is
reported for both sides.  No threshold: the ratios are what the README row carries.
usage: python profiles/constrained_beam_cost.py [--reps N] [--warmup W] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from img2latex_amd import _lib, synth                     # noqa: E402
from constrained_decode_cost import SHIPPED, build, table   # noqa: E402

STEPS = 150


class Route:
    """One entry point with its own scratch and outputs for (images, beam, nbest = beam); tab None: the parent entry."""

    def __init__(self, name, dec, w, n, k, tab, dev):
        L = _lib.lib()
        self.name, self.n, self.k, self.dec, self.w, self.tab = name, n, k, dec, w, tab
        dims = (dec.vocab_size, dec.hidden_dim, dec.lstm_layers, STEPS)
        query = L.i2l_beam_nbest_scratch_bytes if tab is None else L.i2l_beam_nbest_constrained_scratch_bytes
        self.nbytes = query(n, k, k, *dims)
        assert self.nbytes > 0, name
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.seq = torch.empty((n, k, STEPS + 1), dtype=torch.int32, device=dev)
        self.ln = torch.empty((n, k), dtype=torch.int32, device=dev)
        self.score = torch.empty((n, k), dtype=torch.float64, device=dev)
        self.key = torch.empty((n, k), dtype=torch.float64, device=dev)
        self.fin = torch.empty((n, k), dtype=torch.int32, device=dev)
        self.count = torch.ones((n,), dtype=torch.int32, device=dev)
        self.norm = torch.tensor([1.0] + [float(i) ** 0.7 for i in range(1, STEPS + 1)], dtype=torch.float64, device=dev)
        self.cls = None if tab is None else tab.device(dev)

    def __call__(self):
        L = _lib.lib()
        args = (ctypes.byref(self.w), self.dec._ws.data_ptr(), self.n, self.k, self.k, STEPS, synth.START, synth.END,
                self.norm.data_ptr(), self.buf.data_ptr(), self.nbytes, self.seq.data_ptr(), self.ln.data_ptr(),
                self.score.data_ptr(), self.key.data_ptr(), self.fin.data_ptr(), self.count.data_ptr(), 0)
        if self.tab is None:
            rc = L.i2l_beam_decode_nbest(*args, _lib.stream_ptr())
        else:
            rc = L.i2l_beam_decode_nbest_constrained(*args, self.cls.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, self.name)

    def result(self, tab):
        """(rows returned, rows among them that are finished and nest) of one untimed call."""
        self()
        torch.cuda.synchronize()
        seq, ln, fin, count = (t.cpu().tolist() for t in (self.seq, self.ln, self.fin, self.count))
        rows = formed = 0
        for j in range(self.n):
            for r in range(count[j]):
                rows += 1
                formed += bool(fin[j][r]) and tab.well_formed(seq[j][r][:ln[j][r]] + [synth.END])
        return rows, formed


def measure(m, n, k, reps, warmup, dev, tab):
    dec = m.decoder
    enc = torch.from_numpy(synth.uniform(9, "enc", (n, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    w, keep, _ = dec.prepare(enc)
    rs = [Route(f"i2l_beam_decode_nbest, nbest {k}", dec, w, n, k, None, dev),
          Route(f"i2l_beam_decode_nbest_constrained, nbest {k}", dec, w, n, k, tab, dev)]
    res = {r.name: r.result(tab) for r in rs}
    assert res[rs[1].name][0] == res[rs[1].name][1], res                # every constrained row is well formed
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
    return [(r.name, statistics.median(times[r.name]), min(times[r.name]), max(times[r.name])) + res[r.name] for r in rs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_beam_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    m, tab = build(dev), table()
    lines = [f"constrained_beam_cost: {STEPS} steps, nbest = beam, ranked by score / length ** 0.7; median (min - max) over "
             f"{args.reps} launches after {args.warmup}, HIP events around the call, the two entries alternating in one process",
             "'well formed' = returned rows that are finished and nest", ""]
    for n, k in ((1, 2), (16, 5), (128, 5)):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), bracket-biased weights, {n} images x beam {k} = {n * k} rows")
        res = measure(m, n, k, args.reps, args.warmup, dev, tab)
        for name, med, lo, hi, rows, formed in res:
            lines.append(f"  {name:48s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  well formed {formed}/{rows}")
        lines.append(f"  constrained / plain = {res[1][1] / res[0][1]:.3f}x")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
