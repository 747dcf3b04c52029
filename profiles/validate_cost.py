"""Cost of a validation pass (training.Validator) at the BASELINE config-3 shape: 20 batches of 64 x 149 target tokens,
V = 512, the primary CNN-LSTM (3 x 64 x 320, E = H = 256).  HIP events around (a) the eval forward alone over the 20
batches and (b) the Validator's pass (forward + i2l_teacher_forced_eval + the sampled batches' sequence statistics +
finish's one host read), median of --reps passes after one warm-up pass.  Run it under
``rocprofv3 --kernel-trace --stats -- python profiles/validate_cost.py --reps 1`` for the kernel's own time.

    python profiles/validate_cost.py [--reps 5] [--out validate_cost.json]
"""
import argparse
import json
import os
import random
import statistics
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "hmer-img2latex_amd"))

import torch  # noqa: E402

from img2latex_amd import synth  # noqa: E402
from img2latex_amd.model import Seq2SeqModel  # noqa: E402
from img2latex_amd.training import Validator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--bleu-batches", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = synth.model_config()
    sd = synth.make_state_dict(cfg, seed=42, out_scale=12.0, enc_scale=16.0, end_clock=(0.05, 12.0, 6.0))
    model = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to(dev).eval()
    batches = [{"images": torch.from_numpy(synth.make_images(64, cfg, seed=1000 + i)).to(dev),
                "formulas": torch.from_numpy(synth.make_formulas(64, 150, cfg["vocab_size"], seed=2000 + i)).to(dev)}
               for i in range(a.batches)]

    def forward_only():
        with torch.no_grad():
            for b in batches:
                model(b["images"], b["formulas"])

    def validator_pass():
        v = Validator(model, synth.PAD, len(batches), a.bleu_batches, 0.1, rng=random.Random(0))
        for b in batches:
            v.add(b["images"], b["formulas"])
        return v.finish(0, 0)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    forward_only()
    validator_pass()
    fwd, val = [], []
    res = None
    for _ in range(a.reps):
        fwd.append(timed(forward_only)[0])
        t, res = timed(validator_pass)
        val.append(t)
    n = len(batches)
    out = {"batches": n, "batch": 64, "target_tokens": 149, "vocab": cfg["vocab_size"], "reps": a.reps,
           "forward_ms_per_batch": statistics.median(fwd) / n, "validator_ms_per_batch": statistics.median(val) / n,
           "forward_ms_all": fwd, "validator_ms_all": val,
           "overhead_pct": 100.0 * (statistics.median(val) / statistics.median(fwd) - 1.0),
           "val_loss": res["val_loss"], "val_acc": res["val_acc"], "bleu": res.get("bleu"),
           "device": torch.cuda.get_device_name(0)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
