"""What distillation costs: the fused loss launch beside the plain cross entropy, and a whole distilled training step
against the undistilled step plus the teachers' forwards.

1. i2l_ce_distill_fwd_bwd with M = 1, 2, 4 teachers beside i2l_ce_label_smooth_fwd_bwd on the SAME student logits, 64 x 149
   = 9536 rows of V = 512, in one process, with the bytes each moves (CE reads one (rows, V) fp32 matrix and writes one;
   the distillation launch reads M + 1 and writes one) and the rate those bytes come to.
2. A whole TrainStep.step at B = 64, T = 149 on the primary dimensions (V 512, E = H = 256, 3 x 64 x 320) with a teacher
   of M = 1 and of M = 2 members of the same shape, against the YARDSTICK: the undistilled step plus the members'
   eval-mode teacher-forced forwards, timed back to back inside one event pair.  The distilled step does exactly that
   work plus M more rows per row in the loss launch, so it should cost no more than the sum; 3 % are allowed for
   run-to-run spread (the allowance of profiles/ensemble_decode_cost.py), and a ratio above 1.03 is written down as
   WORSE.  lr = 0: the parameters do not move, every repetition is the same work.

The settings alternate inside ONE process; each figure is the median over --reps launches after --warmup, HIP events on
the stream around the call(s).
usage: python profiles/distill_cost.py [--reps N] [--warmup W] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hmer-img2latex_amd"))
from img2latex_amd import _lib, synth                              # noqa: E402
from img2latex_amd.model import EnsembleModel, Seq2SeqModel        # noqa: E402
from img2latex_amd.training import Teacher, TrainStep              # noqa: E402

B, T, V = 64, 149, 512
SIZES = (1, 2, 4)
STEP_SIZES = (1, 2)
TAU, ALPHA, EPS = 2.0, 0.5, 0.1


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


def loss_launches(dev, reps, warmup):
    L = _lib.lib()
    rows = B * T
    gen = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(rows, V, generator=gen)).to(dev)
    z = [(3 * torch.randn(rows, V, generator=gen)).to(dev) for _ in range(max(SIZES))]
    tgt = torch.randint(1, V, (rows,), generator=gen).to(torch.int32)
    tgt[::7] = 0                                                    # pad rows, as a batch has them
    tgt = tgt.to(dev)
    d, out, parts = torch.empty_like(x), torch.empty(2, device=dev), torch.empty(2, device=dev)
    ce_ws = torch.empty(L.i2l_ce_workspace_bytes(rows), dtype=torch.uint8, device=dev)
    ws = torch.empty(L.i2l_ce_distill_workspace_bytes(rows), dtype=torch.uint8, device=dev)

    def ce():
        _lib.check(L.i2l_ce_label_smooth_fwd_bwd(x.data_ptr(), tgt.data_ptr(), rows, V, 0, EPS, ce_ws.data_ptr(), ce_ws.numel(),
                                                 d.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "ce")

    def distill(M):
        recs = (_lib.DistillTeacher * M)(*[_lib.DistillTeacher(z[m].data_ptr(), V, 1.0) for m in range(M)])

        def run():
            _lib.check(L.i2l_ce_distill_fwd_bwd(x.data_ptr(), tgt.data_ptr(), rows, V, 0, EPS, recs, M, _lib.ENSEMBLE_LOGPROB,
                                                TAU, ALPHA, ws.data_ptr(), ws.numel(), d.data_ptr(), out.data_ptr(),
                                                parts.data_ptr(), _lib.stream_ptr()), "distill")
        return run

    res = timed([("ce", ce)] + [(M, distill(M)) for M in SIZES], reps, warmup)
    lines = [f"loss launches, {rows} rows x V {V} (each figure: the rows kernel AND its ordered sum, one event pair)"]
    for k in ["ce"] + list(SIZES):
        med, lo, hi = res[k]
        mats = 2 if k == "ce" else k + 2
        mb = mats * rows * V * 4 / 1e6
        name = "i2l_ce_label_smooth_fwd_bwd" if k == "ce" else f"i2l_ce_distill_fwd_bwd, M = {k}"
        lines.append(f"  {name:32s} {med * 1e3:8.1f} us ({lo * 1e3:.1f} - {hi * 1e3:.1f})  {mb:6.1f} MB moved  {mb / med:8.1f} GB/s"
                     + ("" if k == "ce" else f"  {med / res['ce'][0]:.2f} x the CE launch"))
    return lines, {k: res[k][0] for k in res}


def build(dev, seed):
    cfg = synth.model_config()
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=seed, out_scale=4.0, enc_scale=16.0).items()})
    return m.to(dev), cfg


def whole_steps(dev, reps, warmup):
    members = [build(dev, 50 + m)[0] for m in range(max(STEP_SIZES))]
    cfg = synth.model_config()
    images = torch.from_numpy(synth.make_images(B, cfg, seed=1234)).to(dev)
    forms = torch.from_numpy(synth.make_formulas(B, T + 1, cfg["vocab_size"], seed=777)).to(dev)
    plain = TrainStep(build(dev, 42)[0], lr=0.0, weight_decay=0.0, seed=1)
    sets, teachers = [], {}
    for M in STEP_SIZES:
        teachers[M] = Teacher(EnsembleModel(members[:M]))
        ts = TrainStep(build(dev, 42)[0], lr=0.0, weight_decay=0.0, seed=1, teacher=teachers[M], distill_alpha=ALPHA,
                       distill_temperature=TAU)

        def yardstick(M=M):
            plain.step(images, forms)
            teachers[M].logits(images, forms)

        sets += [((M, "step + forwards"), yardstick), ((M, "distilled step"), lambda ts=ts: ts.step(images, forms))]
    sets.append(((0, "undistilled step"), lambda: plain.step(images, forms)))
    res = timed(sets, reps, warmup)
    lines = [f"whole TrainStep.step, B {B}, T {T}, primary dimensions (V {V}, E = H = 256, 3 x 64 x 320), lr 0"]
    med, lo, hi = res[0, "undistilled step"]
    lines.append(f"  {'undistilled step':44s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})")
    ratios = {}
    for M in STEP_SIZES:
        for what in ("step + forwards", "distilled step"):
            med, lo, hi = res[M, what]
            label = f"M = {M}, " + ("undistilled step + the members' eval forwards" if what == "step + forwards" else what)
            lines.append(f"  {label:44s} {med:8.3f} ms ({lo:.3f} - {hi:.3f})")
        a, b = res[M, "step + forwards"][0], res[M, "distilled step"][0]
        ratios[M] = b / a
        lines.append(f"  M = {M}: distilled step over the yardstick {b - a:+.3f} ms, ratio {b / a:.3f}"
                     + ("" if b / a <= 1.03 else "  (WORSE than the yardstick)"))
    return lines, ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run says nothing about these times"
    assert args.reps >= 20, "medians over at least 20 launches"
    dev = torch.device("cuda:0")
    lines = [f"distill_cost: median (min - max) over {args.reps} launches after {args.warmup}, HIP events around the call(s), all "
             "settings of a section alternating in one process", ""]
    a, _ = loss_launches(dev, args.reps, args.warmup)
    b, _ = whole_steps(dev, args.reps, args.warmup)
    text = "\n".join(lines + a + [""] + b + [""])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
