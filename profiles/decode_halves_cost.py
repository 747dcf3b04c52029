"""What the two-tile 16-member grouped launch (i2l_greedy_decode_halves, decode_group16_kernel<2>) costs against the
one-tile launch it is built from (decode_group16_kernel<1>, which this change leaves as it was), and what GreedyPipeline's
split decode makes of it.

1. The launch alone, headline decoder (V 512, E = H = 256, one layer), B = 256, nothing else on the GPU:
     - one RT = 1 launch of 150 steps (today's decode of one batch);
     - two RT = 1 launches of 75 steps, back to back (the same 2 x 256 x 75 row steps the RT = 2 launch runs);
     - one RT = 2 launch: the last 75 steps of one batch beside the first 75 of another.
   HIP events on the stream around the calls only, the workspaces prepared once outside them, median over --reps after
   --warmup; the ids of the split batches are compared with the one-launch ids before any timing.
2. The pipeline as bench.py builds it (depth 3, co-resident 16-member decode, B = 256, 150 steps) with split_decode on and
   off, alternating in ONE process: wall-clock per batch over --batches submits between synchronisations, median of
   --rounds.
usage: python profiles/decode_halves_cost.py [--reps N] [--warmup W] [--batches N] [--rounds R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                     # noqa: E402
from img2latex_amd.model import Seq2SeqModel              # noqa: E402
from img2latex_amd.model.lstm_decoder import DecodeHalf   # noqa: E402
from img2latex_amd.pipeline import GreedyPipeline         # noqa: E402

STEPS, B = 150, 256
G16 = _lib.FLAG_DECODE_GROUP16


def build(dev):
    cfg = synth.model_config()
    sd = synth.make_state_dict(cfg, seed=42, out_scale=12.0, enc_scale=16.0, end_clock=(0.05, 12.0, 6.0))
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return m.to(dev).eval(), cfg


def timed(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def launch_alone(m, cfg, reps, warmup, dev, out):
    dec = m.decoder
    xs = [torch.from_numpy(synth.make_images(B, cfg, seed=s)).to(dev) for s in (1234, 77)]
    encs = [m.encoder(x).clone() for x in xs]
    tok0 = torch.full((B,), synth.START, dtype=torch.int32, device=dev)
    batches = []
    for i, enc in enumerate(encs):
        w, keep, enc_c = dec.prepare(enc, slot=("cost", "decode-halves-cost", i))
        batches.append(dict(prepared=(w, keep, enc_c, dec._ws), ws=dec._ws, version=dec._ws_key[2], enc=enc,
                            ids=torch.empty((B, STEPS), dtype=torch.int32, device=dev)))
    first = (STEPS + 1) // 2
    half = lambda b, t0, n: DecodeHalf(b["ws"], b["version"], B, STEPS, t0, n, tok0, b["ids"])
    one = lambda b, steps: dec.run_steps(b["enc"], steps, tok0, flags=G16, end_id=synth.END, prepared=b["prepared"])[0]
    want = [one(b, STEPS).cpu() for b in batches]
    dec.decode_halves(None, half(batches[0], 0, first), end_id=synth.END)
    dec.decode_halves(half(batches[0], first, STEPS - first), half(batches[1], 0, first), end_id=synth.END)
    dec.decode_halves(half(batches[1], first, STEPS - first), None, end_id=synth.END)
    for b, w_ in zip(batches, want):
        assert torch.equal(b["ids"].cpu(), w_), "split ids differ from the one-launch ids"
    # steady state of the pair: batch 0 has run its first half, so (batch 0 second half, batch 1 first half) can repeat
    dec.decode_halves(None, half(batches[0], 0, first), end_id=synth.END)
    pair = lambda: dec.decode_halves(half(batches[0], first, STEPS - first), half(batches[1], 0, first), end_id=synth.END)
    rows = [("RT = 1, one launch of 150 steps", lambda: one(batches[0], STEPS), 150),
            ("RT = 1, two launches of 75 steps", lambda: (one(batches[0], first), one(batches[1], first)), 150),
            ("RT = 2, one launch: 75 + 75 steps of two batches", pair, 75)]
    out.append(f"1. the launch alone, B = {B} (median / min / max ms over {reps} launches; us per launch step)")
    for name, fn, steps in rows:
        med, lo, hi = timed(fn, reps, warmup)
        out.append(f"   {name:52s} {med:7.4f} / {lo:7.4f} / {hi:7.4f} ms   {med * 1e3 / steps:6.3f} us per step")
    dec.release_slots("decode-halves-cost")


def pipeline(m, cfg, batches, rounds, dev, out):
    x = torch.from_numpy(synth.make_images(B, cfg, seed=1234)).to(dev)
    res = {True: [], False: []}
    for _ in range(rounds):
        for split in (True, False):
            pipe = GreedyPipeline(m, synth.START, synth.END, STEPS, depth=3, rows_per_workgroup=0, decode_streams=1,
                                  decode_flags=G16, decode_priority=-1, split_decode=None if split else False)
            assert pipe.split_decode == split
            for phase in range(2):                       # a warm-up pass, then the timed one
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(batches):
                    if pipe.pending() >= pipe.depth:
                        pipe.collect()
                    pipe.submit(x)
                while pipe.pending():
                    pipe.collect()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            res[split].append(dt * 1e3 / batches)
            pipe.close()
    out.append(f"2. GreedyPipeline, depth 3, B = {B}, {STEPS} steps: ms per batch over {batches} batches, {rounds} alternating rounds")
    for split in (True, False):
        v = res[split]
        out.append(f"   split_decode {'on ' if split else 'off'}  median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}"
                   f"   ({B * STEPS / statistics.median(v) / 1e3:.2f} M tokens/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    with torch.no_grad():
        m, cfg = build(dev)
        launch_alone(m, cfg, a.reps, a.warmup, dev, out)
        pipeline(m, cfg, a.batches, a.rounds, dev, out)
    text = "\n".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
