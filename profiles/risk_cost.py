"""What minimum-risk fine-tuning costs: a whole TrainStep.step with the risk objective against the pieces it is made of,
and the three launches it adds on their own.

1. A whole TrainStep(risk=RiskObjective(samples=4)).step at B = 64 images, T = 149 on the primary dimensions (V 512,
   E = H = 256, 3 x 64 x 320) against the YARDSTICK: a plain step on 64 x 5 = 320 rows plus Seq2SeqModel.sample_multi_device
   at 64 images x 4 samples x 149 steps, back to back inside one event pair.  The risk step runs the decoder, its loss and
   its backward on those 320 rows and the draws on 64 x 4, but the encoder on 64 images only, so it should cost no more
   than the sum; 3 % are allowed for run-to-run spread (the allowance of profiles/ensemble_decode_cost.py and
   profiles/distill_cost.py), and a ratio above 1.03 is written down as WORSE.  lr = 0: the parameters do not move, every
   repetition is the same work -- and the draws of a step depend on the step number only through their seed.
2. i2l_risk_rows at 64 x 4 x 149, i2l_ce_weighted_fwd_bwd on 320 x 149 token rows of V = 512 beside
   i2l_ce_label_smooth_fwd_bwd on the same logits, and i2l_rows_repeat + i2l_rows_fold of 64 rows of 256 by 5.

The settings alternate inside ONE process; each figure is the median over --reps launches after --warmup, HIP events on
the stream around the call(s).
usage: python profiles/risk_cost.py [--reps N] [--warmup W] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                              # noqa: E402
from img2latex_amd.model import Seq2SeqModel                       # noqa: E402
from img2latex_amd.training import RiskObjective, TrainStep        # noqa: E402
from img2latex_amd.training.risk import rows_fold, rows_repeat     # noqa: E402

B, T, V, N, E = 64, 149, 512, 4, 256
ALPHA, EPS = 0.5, 0.1


def timed(sets, reps, warmup):
    """sets: [(key, run)] -> {key: (median, min, max) ms}; the settings alternate."""
    times = {k: [] for k, _ in sets}
    for i in range(warmup + reps):
        for k, run in sets:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def build(dev, seed):
    cfg = synth.model_config()
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    sd = synth.make_state_dict(cfg, seed=seed, out_scale=4.0, enc_scale=16.0, end_clock=(0.05, 12.0, 6.0))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev), cfg


def whole_steps(dev, reps, warmup):
    cfg = synth.model_config()
    images = torch.from_numpy(synth.make_images(B, cfg, seed=1234)).to(dev)
    forms = torch.from_numpy(synth.make_formulas(B, T + 1, cfg["vocab_size"], seed=777)).to(dev)
    wide_images = images.repeat_interleave(N + 1, 0).contiguous()
    wide_forms = forms.repeat_interleave(N + 1, 0).contiguous()
    plain = TrainStep(build(dev, 42)[0], lr=0.0, weight_decay=0.0, seed=1)
    small = TrainStep(build(dev, 42)[0], lr=0.0, weight_decay=0.0, seed=1)
    objective = RiskObjective(synth.START, synth.END, samples=N, alpha=ALPHA)
    risk = TrainStep(build(dev, 42)[0], lr=0.0, weight_decay=0.0, seed=1, risk=objective)
    sampler = build(dev, 42)[0].eval()
    with torch.no_grad():
        enc = sampler.encoder(images)

    def draws():
        return objective.draw(sampler, enc, T, 77)

    def yardstick():
        plain.step(wide_images, wide_forms)
        draws()

    res = timed([("plain 64", lambda: small.step(images, forms)), ("plain 320", lambda: plain.step(wide_images, wide_forms)),
                 ("draws", draws), ("yardstick", yardstick), ("risk", lambda: risk.step(images, forms))], reps, warmup)
    lines = [f"whole TrainStep.step, B {B}, T {T}, N {N}, primary dimensions (V {V}, E = H = 256, 3 x 64 x 320), lr 0"]
    for key, label in (("plain 64", f"plain step, {B} rows"), ("plain 320", f"plain step, {B * (N + 1)} rows"),
                       ("draws", f"sample_multi_device, {B} x {N} x {T}"),
                       ("yardstick", f"plain step on {B * (N + 1)} rows + the draws (yardstick)"),
                       ("risk", "step with the risk objective")):
        med, lo, hi = res[key]
        lines.append(f"  {label:52s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})")
    a, b = res["yardstick"][0], res["risk"][0]
    lines.append(f"  risk step over the yardstick {b - a:+.3f} ms, ratio {b / a:.3f}"
                 + ("" if b / a <= 1.03 else "  (WORSE than the yardstick)"))
    lines.append(f"  risk step over the plain step on {B} rows: {b / res['plain 64'][0]:.2f} x")
    return lines


def launches(dev, reps, warmup):
    L = _lib.lib()
    gen = torch.Generator().manual_seed(5)
    cfg = synth.model_config()
    forms = torch.from_numpy(synth.make_formulas(B, T + 1, cfg["vocab_size"], seed=777)).to(torch.int32).to(dev)
    draws = torch.randint(4, V, (B, N, T), generator=gen).to(torch.int32)
    for b in range(B):
        for n in range(N):
            end = 20 + (7 * b + 13 * n) % (T - 20)
            draws[b, n, end] = synth.END
            draws[b, n, end + 1:] = -1
    objective = RiskObjective(synth.START, synth.END, samples=N, alpha=ALPHA)
    draws = draws.to(dev)
    batch = objective.assemble(forms, draws, synth.PAD, EPS)
    seqs = B * (N + 1)
    rows = seqs * T
    x = (3 * torch.randn(rows, V, generator=gen)).to(dev)
    tgt = batch["rows"][:, 1:].contiguous()
    d, out, parts = torch.empty_like(x), torch.empty(2, device=dev), torch.empty(4, device=dev)
    ws = torch.empty(L.i2l_ce_weighted_workspace_bytes(rows), dtype=torch.uint8, device=dev)
    enc = torch.randn(B, E, generator=gen).to(dev)
    denc = torch.randn(seqs, E, generator=gen).to(dev)

    def ce():
        _lib.check(L.i2l_ce_label_smooth_fwd_bwd(x.data_ptr(), tgt.data_ptr(), rows, V, synth.PAD, EPS, ws.data_ptr(), ws.numel(),
                                                 d.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "ce")

    def weighted():
        _lib.check(L.i2l_ce_weighted_fwd_bwd(x.data_ptr(), tgt.data_ptr(), seqs, T, V, synth.PAD, batch["coef"].data_ptr(),
                                             batch["smooth"].data_ptr(), batch["part"].data_ptr(), ws.data_ptr(), ws.numel(),
                                             d.data_ptr(), out.data_ptr(), parts.data_ptr(), _lib.stream_ptr()), "weighted")

    res = timed([("rows", lambda: objective.assemble(forms, draws, synth.PAD, EPS)), ("ce", ce), ("weighted", weighted),
                 ("repeat", lambda: rows_repeat(enc, N + 1)), ("fold", lambda: rows_fold(denc, N + 1))], reps, warmup)
    lines = [f"the new launches alone ({B} images, {N} draws, {T} steps; {rows} token rows of V {V}; each figure includes the "
             "allocation of the call's outputs where the Python wrapper makes it)"]
    for key, label in (("rows", "i2l_risk_rows"), ("ce", "i2l_ce_label_smooth_fwd_bwd, same logits"),
                       ("weighted", "i2l_ce_weighted_fwd_bwd"), ("repeat", f"i2l_rows_repeat, {B} x {E} by {N + 1}"),
                       ("fold", f"i2l_rows_fold, {seqs} x {E} by {N + 1}")):
        med, lo, hi = res[key]
        lines.append(f"  {label:44s} {med * 1e3:8.1f} us ({lo * 1e3:.1f} - {hi * 1e3:.1f})")
    lines.append(f"  weighted over the plain cross entropy launch: {res['weighted'][0] / res['ce'][0]:.3f} x")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "risk_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    lines = [f"risk_cost: median (min - max) over {args.reps} launches after {args.warmup}, HIP events around the call(s), all "
             "settings of a section alternating in one process", ""]
    a = whole_steps(dev, args.reps, args.warmup)
    b = launches(dev, args.reps, args.warmup)
    text = "\n".join(lines + a + [""] + b + [""])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
