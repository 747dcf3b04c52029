"""What the consensus decode (i2l_sample_decode_multi: `samples` draws of each image in one step-batched loop, scored and
ranked on the device) costs against its yardstick, i2l_sample_decode_batched at the SAME row count on a workspace prepared
from the encoder rows repeated `samples` times -- what a caller had to do before the entry existed, without a score.

The shipped decoder (V 500, E = H = 512, two layers), top_k 5 + top_p 0.9, 150 steps, (images, samples) = (16, 16), (64, 4)
and (1, 16), without a constraint and under a bracket table (yardstick: i2l_sample_decode_constrained).  Both sides are the
C entries called directly on workspaces prepared beforehand, the sticky stop on both; without a constraint end_id is -1, so
every row runs every step on both sides, under the table the rows end where the rules let them and the two sides draw
the same tokens (same seed, same uniforms).  Yardstick, whole call and the ranking alone (i2l_sample_rank on the call's
ids) alternate inside ONE process; each figure is the median over --reps launches after --warmup, HIP events on the
stream.  "decode part" = whole call - ranking alone; the score accumulation must keep it within 1.03x of the yardstick.

Also: i2l_sample_decode_batched's own lines as profiles/sample_batched_cost.py measures them (sample_steps, prepare
included, no stop rule), beside the figures that file holds from the parent commit; the drift between two processes
was about +-1.2 % when those were taken, a difference inside that is not a finding.
usage: python profiles/sample_rank_cost.py [--reps N] [--warmup W] [--out FILE]"""
import argparse
import ctypes
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                                      # noqa: E402
from img2latex_amd.model import Seq2SeqModel                               # noqa: E402
from img2latex_amd.training.constraint import BracketTable, close_class, open_class   # noqa: E402

STEPS = 150
SEED = 2024
TOP_K, TOP_P = 5, 0.9
SHIPPED = dict(vocab_size=500, embedding_dim=512, hidden_dim=512, lstm_layers=2, attention=True)
SHAPES = [(16, 16), (64, 4), (1, 16)]
BOUND = 1.03


def build(dev):
    cfg = synth.model_config(channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **SHIPPED)   # the encoder is unused
    sd = synth.make_state_dict(cfg, seed=42, out_scale=8.0)          # sample_batched_cost.py's weights
    m = Seq2SeqModel("cnn_lstm", SHIPPED["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


def bracket_table():
    t = np.zeros(SHIPPED["vocab_size"], dtype=np.uint8)
    t[[synth.PAD, synth.START, 3]] = 255
    for k in range(3):
        t[4 + 2 * k], t[5 + 2 * k] = open_class(k), close_class(k)
    return BracketTable(t, synth.END)


def timed(sets, reps, warmup):
    times = {name: [] for name, _ in sets}
    for i in range(warmup + reps):
        for name, run in sets:                              # the settings alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in times.items()}


def measure(multi_m, yard_m, images, samples, table, reps, warmup, dev):
    L, rows, V = _lib.lib(), images * samples, SHIPPED["vocab_size"]
    H, layers = SHIPPED["hidden_dim"], SHIPPED["lstm_layers"]
    enc = torch.from_numpy(synth.uniform(9, "enc", (images, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
    w_m, keep_m, _ = multi_m.decoder.prepare(enc)
    w_y, keep_y, _ = yard_m.decoder.prepare(enc.repeat_interleave(samples, 0))
    kind = _lib.CONSTRAIN_NONE if table is None else table.kind
    end_id = -1 if table is None else synth.END
    cls = None if table is None else table.device(dev)
    tok_i = torch.full((images,), synth.START, dtype=torch.int32, device=dev)
    tok_r = torch.full((rows,), synth.START, dtype=torch.int32, device=dev)
    ids_m = torch.empty((images, samples, STEPS), dtype=torch.int32, device=dev)
    ids_y = torch.empty((rows, STEPS), dtype=torch.int32, device=dev)
    ln, fin, risk, order = (torch.empty((images, samples), dtype=torch.int32, device=dev) for _ in range(4))
    score, key = (torch.empty((images, samples), dtype=torch.float64, device=dev) for _ in range(2))
    nb_m = L.i2l_sample_multi_scratch_bytes(images, samples, V, H, layers, STEPS, kind)
    nb_y = L.i2l_decode_batched_scratch_bytes(rows, V, H, layers)
    assert nb_m > 0 and nb_y > 0
    sc_m, sc_y = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (nb_m, nb_y))
    state = None if table is None else torch.empty(table.state_bytes(rows), dtype=torch.uint8, device=dev)

    def whole():
        _lib.check(L.i2l_sample_decode_multi(ctypes.byref(w_m), multi_m.decoder._ws.data_ptr(), images, samples, STEPS,
                                             tok_i.data_ptr(), 1.0, TOP_K, TOP_P, SEED, end_id, kind, _lib.ptr(cls),
                                             _lib.RANK_CONSENSUS, None, sc_m.data_ptr(), nb_m, ids_m.data_ptr(), ln.data_ptr(),
                                             fin.data_ptr(), score.data_ptr(), risk.data_ptr(), key.data_ptr(),
                                             order.data_ptr(), 0, _lib.stream_ptr()), "sample_decode_multi")

    def yardstick():
        if table is None:
            _lib.check(L.i2l_sample_decode_batched(ctypes.byref(w_y), yard_m.decoder._ws.data_ptr(), rows, STEPS,
                                                   tok_r.data_ptr(), None, None, 1.0, TOP_K, TOP_P, SEED, _lib.STOP_STICKY,
                                                   end_id, ids_y.data_ptr(), None, None, None, sc_y.data_ptr(), nb_y, 0,
                                                   _lib.stream_ptr()), "sample_decode_batched")
        else:
            _lib.check(L.i2l_sample_decode_constrained(ctypes.byref(w_y), yard_m.decoder._ws.data_ptr(), rows, STEPS,
                                                       tok_r.data_ptr(), None, None, 1.0, TOP_K, TOP_P, SEED,
                                                       _lib.STOP_STICKY, end_id, ids_y.data_ptr(), None, None, None,
                                                       sc_y.data_ptr(), nb_y, 0, cls.data_ptr(), state.data_ptr(),
                                                       state.numel(), _lib.stream_ptr()), "sample_decode_constrained")

    def ranking():
        _lib.check(L.i2l_sample_rank(ids_m.data_ptr(), images, samples, STEPS, end_id, score.data_ptr(), _lib.RANK_CONSENSUS,
                                     None, ln.data_ptr(), fin.data_ptr(), risk.data_ptr(), key.data_ptr(), order.data_ptr(),
                                     None, _lib.stream_ptr()), "sample_rank")

    whole()
    yardstick()
    torch.cuda.synchronize()
    same = int((ids_m.view(rows, STEPS) == ids_y).all(dim=1).sum())      # ids first, timing afterwards
    live = int((ids_m.view(rows, STEPS) >= 0).any(dim=0).sum())
    res = timed([("yardstick", yardstick), ("whole", whole), ("ranking", ranking)], reps, warmup)
    del keep_m, keep_y
    return res, same, live


def own_lines(m, reps, warmup, dev):
    """sample_batched_cost.py's flag-on (5, 0.9) line at its four row counts, measured its way."""
    out = []
    for rows in (1, 16, 64, 256):
        enc = torch.from_numpy(synth.uniform(9, "enc", (rows, SHIPPED["embedding_dim"]), -1.5, 1.5)).to(dev)
        tok0 = torch.full((rows,), synth.START, dtype=torch.int32, device=dev)
        run = lambda: m.decoder.sample_steps(enc, STEPS, tok0, 1.0, TOP_K, TOP_P, SEED, stop=_lib.STOP_NONE,   # noqa: E731
                                             flags=_lib.FLAG_DECODE_BATCHED)
        out.append((rows, timed([("own", run)], reps, warmup)["own"]))
    return out


def parent_lines():
    path, rows, out = os.path.join(ROOT, "profiles", "sample_batched_cost.txt"), None, {}
    for line in open(path):
        head = re.match(r"shipped decoder .*, (\d+) rows", line)
        if head:
            rows = int(head.group(1))
        hit = re.match(r"\s+top_k 5 top_p 0.9: flag on \(step-batched\)\s+([\d.]+) ms", line)
        if hit and rows is not None:
            out[rows] = float(hit.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rank_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    multi_m, yard_m = build(dev), build(dev)
    lines = [f"sample_rank_cost: shipped decoder (V 500, E 512, H 512, L 2), top_k {TOP_K} top_p {TOP_P}, {STEPS} steps, sticky "
             f"stop; median (min - max) over {args.reps} launches after {args.warmup}, HIP events around the C entry, the three "
             "settings alternating in one process",
             "yardstick = i2l_sample_decode_batched (brackets: i2l_sample_decode_constrained) at images * samples rows on the "
             "encoder rows repeated; decode part = whole call - ranking alone; 'rows equal' = rows whose ids equal the "
             "yardstick's end to end; 'steps run' = steps at which a row was still live", ""]
    missed = []
    for what, table in (("no constraint (end_id -1: every row runs every step)", None), ("brackets", bracket_table())):
        for images, samples in SHAPES:
            res, same, live = measure(multi_m, yard_m, images, samples, table, args.reps, args.warmup, dev)
            rows = images * samples
            y, wh, rk = res["yardstick"], res["whole"], res["ranking"]
            part = wh[0] - rk[0]
            ratio = part / y[0]
            lines.append(f"{images} images x {samples} samples = {rows} rows, {what}; rows equal {same}/{rows}, steps run {live}")
            lines.append(f"  yardstick at {rows} rows                      {y[0]:8.3f} ms ({y[1]:.3f} - {y[2]:.3f})")
            lines.append(f"  i2l_sample_decode_multi, whole call        {wh[0]:8.3f} ms ({wh[1]:.3f} - {wh[2]:.3f})")
            lines.append(f"  ranking alone (i2l_sample_rank, 2 launches){rk[0]:8.3f} ms ({rk[1]:.3f} - {rk[2]:.3f})")
            verdict = "within" if ratio <= BOUND else "WORSE than"
            lines.append(f"  decode part {part:.3f} ms = {ratio:.3f}x the yardstick: {verdict} the {BOUND}x allowance; "
                         f"whole call {wh[0] / y[0]:.3f}x")
            lines.append("")
            if ratio > BOUND:
                missed.append((images, samples, what.split()[0]))
    lines.append("the decode part is WORSE than the yardstick's 1.03x at: " +
                 (", ".join(f"{i}x{s} {w}" for i, s, w in missed) if missed else "none of the six settings"))
    lines.append("")
    parent = parent_lines()
    lines.append("i2l_sample_decode_batched's own lines (sample_steps, prepare included, no stop rule) beside "
                 "profiles/sample_batched_cost.txt (the parent commit's, another process)")
    for rows, (med, lo, hi) in own_lines(yard_m, args.reps, args.warmup, dev):
        was = parent.get(rows)
        cmp_ = "" if was is None else f"  parent {was:.3f} ms  {100.0 * (med - was) / was:+.2f} %"
        lines.append(f"  {rows:4d} rows  {med:8.3f} ms ({lo:.3f} - {hi:.3f}){cmp_}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
