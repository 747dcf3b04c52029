"""What the ensemble decode costs against its members decoded one after the other: i2l_ensemble_decode with M members
against the SUM of the members' own i2l_greedy_decode_batched / i2l_sample_decode_batched calls in the same process.  The
yardstick is those entries, which the ensemble does not touch: per step the ensemble replaces M selection launches by one
combine and one selection, so it should cost no more than the sum; 3 % are allowed for run-to-run spread, and a ratio
above 1.03 is written down as WORSE.

The shipped decoder (V 500, E = H = 512, two layers), M = 2 and 4 members of that shape with distinct weight seeds, ids
only, 150 steps, no stop rule (every row runs every step), rows 256 / 16 / 1; greedy, and top_k 5 + top_p 0.9 sampling.
The settings alternate inside ONE process; each figure is the median over --reps launches after --warmup, HIP events on
the stream around the call(s) -- every member's i2l_decoder_prepare included on both sides alike.  "members" is ONE event
pair around the M single-model calls issued back to back.  Before any timing the ensemble's greedy ids are compared with
member 0's: an ensemble that ignored its other members would give the same.

--trace ROWS: one ensemble call per setting at ROWS rows and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python profiles/ensemble_decode_cost.py --trace 256); the combine kernel's own
time in the .txt is copied from that trace's statistics by hand.
usage: python profiles/ensemble_decode_cost.py [--reps N] [--warmup W] [--out FILE] | --trace ROWS"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                              # noqa: E402
from img2latex_amd.model import EnsembleDecoder, Seq2SeqModel      # noqa: E402

STEPS = 150
SEED = 2024
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
MASK = (5, 0.9)
FLAG = _lib.FLAG_DECODE_BATCHED
SIZES = (2, 4)
MODES = ("greedy", f"top_k {MASK[0]} top_p {MASK[1]}")


def build(dev, seed):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **SHIPPED)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=seed, out_scale=8.0)
    m = Seq2SeqModel("cnn_lstm", SHIPPED["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval().decoder


def settings(decoders, rows, dev):
    """[(mode, M, "members" | "ensemble", run)]; run() enqueues the call(s) and returns the ids of the last one."""
    encs = [torch.from_numpy(synth.uniform(9 + m, "enc", (rows, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
            for m in range(max(SIZES))]
    tok0 = torch.full((rows,), synth.START, dtype=torch.int32, device=dev)

    def greedy(dec, enc):
        return dec.run_steps(enc, STEPS, tok0, end_id=synth.END, flags=FLAG)[0]

    def sample(dec, enc):
        return dec.sample_steps(enc, STEPS, tok0, 1.0, MASK[0], MASK[1], SEED, stop=_lib.STOP_NONE, end_id=synth.END,
                                flags=FLAG)[0]

    out = []
    for M in SIZES:
        ens = EnsembleDecoder(decoders[:M])
        for mode, call in zip(MODES, (greedy, sample)):
            out.append((mode, M, "members", lambda call=call, M=M: [call(d, e) for d, e in zip(decoders[:M], encs[:M])][-1]))
            out.append((mode, M, "ensemble", lambda call=call, ens=ens, M=M: call(ens, encs[:M])))
    return out


def measure(decoders, rows, reps, warmup, dev):
    sets = settings(decoders, rows, dev)
    differ = {}
    enc0 = torch.from_numpy(synth.uniform(9, "enc", (rows, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    own = decoders[0].run_steps(enc0, STEPS, torch.full((rows,), synth.START, dtype=torch.int32, device=dev),
                                end_id=synth.END, flags=FLAG)[0]
    for mode, M, what, run in sets:                                  # ids first, timing afterwards
        ids = run()
        assert int(ids.min()) >= 0 and int(ids.max()) < SHIPPED["vocab_size"], (mode, M, what)
        if what == "ensemble" and mode == "greedy":
            differ[M] = int((ids != own).any(dim=1).sum())
            assert rows < 16 or 2 * differ[M] >= rows, f"the ensemble of {M} gives member 0's ids in {rows - differ[M]} of {rows} rows"
    times = {(mode, M, what): [] for mode, M, what, _ in sets}
    for i in range(warmup + reps):
        for mode, M, what, run in sets:                              # the settings alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[mode, M, what].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}, differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_decode_cost.txt"))
    ap.add_argument("--trace", type=int, default=0, metavar="ROWS")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    dev = torch.device("cuda:0")
    decoders = [build(dev, 42 + m) for m in range(max(SIZES))]
    if args.trace:
        for mode, M, what, run in settings(decoders, args.trace, dev):
            if what == "ensemble":
                run()
        torch.cuda.synchronize()
        return
    assert args.reps >= 20, "medians over at least 20 launches"
    lines = [f"ensemble_decode_cost: ids only, {STEPS} steps, temperature 1, no stop rule; median (min - max) over {args.reps} "
             f"launches after {args.warmup}, HIP events around the call(s), all settings alternating in one process",
             "'members' = the M members' own i2l_greedy_decode_batched / i2l_sample_decode_batched calls back to back (the "
             "yardstick); 'ensemble' = one i2l_ensemble_decode, logprob rule, equal weights", ""]
    for rows in (256, 16, 1):
        lines.append(f"shipped decoder (V 500, E 512, H 512, L 2), {rows} rows")
        res, differ = measure(decoders, rows, args.reps, args.warmup, dev)
        for M in SIZES:
            for mode in MODES:
                for what in ("members", "ensemble"):
                    med, lo, hi = res[mode, M, what]
                    lines.append(f"  M = {M}, {mode + ', ' + what:32s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})  {med * 1e3 / STEPS:7.2f} us/step")
                a, b = res[mode, M, "members"][0], res[mode, M, "ensemble"][0]
                lines.append(f"  M = {M}, {mode}: ensemble over members {(b - a) * 1e3 / STEPS:+.2f} us/step, ratio {b / a:.3f}"
                             + ("" if b / a <= 1.03 else "  (WORSE than the yardstick)"))
            lines.append(f"  M = {M}: greedy ensemble ids differ from member 0's own in {differ[M]} of {rows} rows")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
