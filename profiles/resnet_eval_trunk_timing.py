"""Times the three forward passes of the ResNet trunk that exist, at BASELINE config 4 (B = 256, 3x64x320, resnet50):

  fp32 eval    eval_precision = "fp32": one i2l_conv_bn_act_f32_fwd launch per conv unit (folded running statistics)
  fp32 train   _trunk_train(x, None): i2l_conv_f32_fwd + i2l_bn_train_fwd_f32 per unit (batch statistics) -- the only
               fp32-grade forward before the fused eval trunk existed
  bf16 eval    eval_precision = "bf16": i2l_conv_bn_act_bf16_fwd

HIP events on one stream, same process: `--warmup` untimed passes, then `--repeats` timed ones; the median is reported,
with the per-stage split (stem incl. max-pool, layer1..4 incl. the average pool) from an event in front of every unit.

    python profiles/resnet_eval_trunk_timing.py [--out profiles/resnet_eval_trunk_timing.txt]
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "hmer-img2latex_amd"))

from img2latex_amd import synth  # noqa: E402
from img2latex_amd.model import ResNetEncoder  # noqa: E402

STAGES = ["stem", "layer1", "layer2", "layer3", "layer4"]


def build(model_name, h, w, dev):
    enc = ResNetEncoder(h, w, 3, model_name=model_name, embedding_dim=256)
    shapes = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    sd = synth.make_resnet_state_dict(shapes, seed=5)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return enc.to(dev)


def time_trunk(enc, unit_method, x, warmup, repeats):
    """Median total ms and median ms per stage of enc.trunk(x); `unit_method` is the per-unit method of the path."""
    stage_of = {id(enc.resnet[0]): 0}
    for li in range(4, 8):
        for mod in enc.resnet[li].modules():
            if isinstance(mod, torch.nn.Conv2d):
                stage_of[id(mod)] = li - 3
    inner = getattr(enc, unit_method)
    marks = []

    def unit(x_, shape, conv, *a, **kw):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((stage_of[id(conv)], ev))
        return inner(x_, shape, conv, *a, **kw)

    setattr(enc, unit_method, unit)
    totals, per_stage = [], [[] for _ in STAGES]
    try:
        with torch.no_grad():
            for it in range(warmup + repeats):
                marks.clear()
                enc.trunk(x)
                end = torch.cuda.Event(enable_timing=True)
                end.record()
                torch.cuda.synchronize()
                if it < warmup:
                    continue
                evs = [ev for _, ev in marks] + [end]
                acc = [0.0] * len(STAGES)
                for i, (st, ev) in enumerate(marks):
                    acc[st] += ev.elapsed_time(evs[i + 1])
                totals.append(marks[0][1].elapsed_time(end))
                for s, v in enumerate(acc):
                    per_stage[s].append(v)
    finally:
        delattr(enc, unit_method)
    return statistics.median(totals), [statistics.median(v) for v in per_stage], len(marks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    x = torch.from_numpy(synth.uniform(9, "rimg", (args.batch, 3, args.height, args.width), -1.0, 1.0)).to(dev)
    rows = []
    enc = build(args.model, args.height, args.width, dev).eval()
    enc.eval_precision = "fp32"
    rows.append(("fp32 eval (fused)",) + time_trunk(enc, "_conv_bn_f32", x, args.warmup, args.repeats))
    enc.eval_precision = "bf16"
    rows.append(("bf16 eval",) + time_trunk(enc, "_conv_bn", x, args.warmup, args.repeats))
    enc.train()                                        # last: it moves the running statistics
    rows.append(("fp32 train forward",) + time_trunk(enc, "_conv_bn_train", x, args.warmup, args.repeats))
    lines = [f"{args.model} trunk forward, B = {args.batch}, 3x{args.height}x{args.width}, {torch.cuda.get_device_name(0)}",
             f"median of {args.repeats} passes after {args.warmup} warm-up passes, HIP events, ms",
             f"{'path':<20}{'units':>6}{'total':>10}" + "".join(f"{s:>10}" for s in STAGES)]
    for name, total, stages, units in rows:
        lines.append(f"{name:<20}{units:>6}{total:>10.3f}" + "".join(f"{v:>10.3f}" for v in stages))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
