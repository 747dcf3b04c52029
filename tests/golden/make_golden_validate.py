#!/usr/bin/env python3
"""Generate tests/golden/validate.npz by running the REAL reference's Trainer.validate (trainer.py:461-665).

Like make_golden.py: the reference package is imported unmodified (with the same inert ``torchvision`` shim), weights
and inputs come from img2latex_amd.synth, and only outputs plus the generator arguments are stored.  ``validate`` is
called unbound on a small stub that carries the attributes it reads; ``current_epoch`` 1 with a large
``detailed_eval_frequency`` / ``max_epochs`` keeps ``use_detailed_metrics`` false (nothing is written), and
``save_basic_metrics`` is off.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_validate.py

Per configuration ``<name>_*``: the batch sizes and generator seeds, the formulas (their bodies follow the model's
own arg max, which the reference computes, so they are stored as inputs), the reference's per-batch ``loss.item()``, every
position's arg max id and top-1 / top-2 logit gap (all above 1e-4: seeds are drawn until they are, so that id equality
is a fair demand of a float32 forward), the indices of the batches it sampled for BLEU, and every scalar of the dict it
returns (token_distribution and samples excluded).
"""
import json
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the torchvision shim, puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import img2latex.training.trainer as RT  # noqa: E402  (the reference)
from img2latex_amd import synth  # noqa: E402

# name: (fixture whose cfg / state-dict kwargs are used, batch sizes (smaller last one), formula length incl. START,
#        bleu_batches, first image / formula seed tried, random.seed)
RUNS = {
    "tiny_l1": ("tiny_l1", [4, 4, 4, 4, 4, 4, 4, 4, 3], 24, 3, 100, 5),
    "odd_dims": ("odd_dims", [3, 3, 3, 3, 3, 3, 3, 3, 2], 21, 2, 200, 11),
}


class RecordingModel(torch.nn.Module):
    def __init__(self, ref):
        super().__init__()
        self.ref = ref
        self.outputs = []

    def forward(self, images, formulas):
        out = self.ref(images, formulas)
        self.outputs.append(out.detach().clone())
        return out


class RecordingLoss(torch.nn.Module):
    def __init__(self, pad):
        super().__init__()
        self.ce = torch.nn.CrossEntropyLoss(ignore_index=pad, reduction="mean", label_smoothing=0.1)   # trainer.py:111-115
        self.losses = []

    def forward(self, logits, targets):
        loss = self.ce(logits, targets)
        self.losses.append(loss.item())
        return loss


class Tok:
    pad_token_id, start_token_id, end_token_id = synth.PAD, synth.START, synth.END
    special_tokens = {}
    id_to_token = {}

    def decode(self, ids):
        return json.dumps([int(i) for i in ids])


class RecordingRandom:
    """random.random() draws of the reference, in order (the sampling rule of trainer.py:537 is then recomputed from
    them and cross-checked against what compute_all_metrics received)."""

    def __init__(self):
        self.draws = []

    def random(self):
        v = random.random()
        self.draws.append(v)
        return v

    def randint(self, a, b):
        return random.randint(a, b)


def batches_for(ref, cfg, sizes, length, seed):
    """Images from synth; formulas = synth's ragged START / body / END / PAD layout whose body follows the model's own
    teacher-forced arg max at ~80 % of the positions (so that BLEU-4 has n-grams to match), random tokens elsewhere."""
    n = sum(sizes)
    imgs = torch.from_numpy(synth.make_images(n, cfg, seed=seed))
    forms = torch.from_numpy(synth.make_formulas(n, length, cfg["vocab_size"], seed=seed + 1, min_len=3))
    follow = torch.from_numpy(synth.uniform(seed + 1, "follow", (n, length), 0.0, 1.0) < 0.8)
    body = (forms != synth.PAD) & (forms != synth.END) & (forms != synth.START)
    with torch.no_grad():
        for t in range(1, length):
            arg = ref(imgs, forms).argmax(-1)[:, t - 1]
            pick = body[:, t] & follow[:, t] & (arg >= 4)
            forms[:, t] = torch.where(pick, arg, forms[:, t])
    out, o = [], 0
    for b in sizes:
        out.append({"images": imgs[o:o + b], "formulas": forms[o:o + b]})
        o += b
    return out


def run(name, base, sizes, length, bleu_batches, seed0, rng_seed):
    d, cfg, sd_kw = None, None, None
    d = np.load(os.path.join(HERE, base + ".npz"))
    cfg = json.loads(str(d["cfg_json"]))
    sd_kw = json.loads(str(d["sd_kw_json"]))
    if sd_kw.get("end_clock") is not None:
        sd_kw["end_clock"] = tuple(sd_kw["end_clock"])
    ref = G.build_reference(cfg, synth.make_state_dict(cfg, **sd_kw))
    seed = seed0
    while True:                                              # inputs whose every position has a clear arg max
        loader = batches_for(ref, cfg, sizes, length, seed)
        with torch.no_grad():
            gaps = []
            for b in loader:
                top = torch.topk(ref(b["images"], b["formulas"]), 2, dim=-1).values
                gaps.append((top[..., 0] - top[..., 1]).reshape(-1))
            gap = torch.cat(gaps)
        if float(gap.min()) > 1e-4:
            break
        seed += 2
    stub = types.SimpleNamespace(
        model=RecordingModel(ref), config={"model": {"name": "cnn_lstm"},
                                           "evaluation": {"save_basic_metrics": False, "bleu_batches": bleu_batches},
                                           "logging": {"val_log_frequency": 1000, "detailed_eval_frequency": 1000}},
        bleu_batches=bleu_batches, enhanced_samples=2, val_loader=loader, current_epoch=1, max_epochs=1000,
        global_step=17, device=torch.device("cpu"), criterion=RecordingLoss(synth.PAD), tokenizer=Tok(),
        experiment_name="golden_validate")
    seen = {}
    real_cam = RT.compute_all_metrics

    def cam(*a, **k):
        seen["preds"], seen["targets"] = [list(p) for p in k["all_predictions"]], [list(t) for t in k["all_targets"]]
        return real_cam(*a, **k)

    total = len(loader)
    rate = bleu_batches / total if total > bleu_batches else 1.0
    while True:                                              # a seed whose draws sample some later batches, not all
        rec_rng = RecordingRandom()
        stub.model.outputs, stub.criterion.losses = [], []
        RT.random, RT.compute_all_metrics = rec_rng, cam
        try:
            random.seed(rng_seed)
            res = RT.Trainer.validate(stub)
        finally:
            RT.random, RT.compute_all_metrics = random, real_cam
        draws = iter(rec_rng.draws)
        sampled = [i for i in range(total) if i < bleu_batches or next(draws) < rate]
        assert next(draws, None) is None
        if bleu_batches < len(sampled) < total:
            break
        rng_seed += 1
    ids = [o.argmax(-1) for o in stub.model.outputs]
    # cross-check: what compute_all_metrics received is the pad-truncated arg max / targets of the sampled batches
    want_p, want_t = [], []
    for i in sampled:
        for p, t in zip(ids[i].tolist(), loader[i]["formulas"][:, 1:].tolist()):
            want_p.append(p[:p.index(synth.PAD)] if synth.PAD in p else p)
            want_t.append(t[:t.index(synth.PAD)] if synth.PAD in t else t)
    assert want_p == seen["preds"] and want_t == seen["targets"]
    out = {
        f"{name}_cfg_json": np.array(json.dumps(cfg)), f"{name}_sd_kw_json": np.array(json.dumps(sd_kw)),
        f"{name}_gen_json": np.array(json.dumps(dict(sizes=sizes, length=length, seed=seed, bleu_batches=bleu_batches,
                                                     rng_seed=rng_seed, epoch=1, step=17))),
        f"{name}_batch_loss": np.array(stub.criterion.losses, dtype=np.float64),
        f"{name}_ids": torch.cat([i.reshape(-1) for i in ids]).numpy().astype(np.int16),
        f"{name}_gap": gap.numpy().astype(np.float32),
        f"{name}_sampled": np.array(sampled, dtype=np.int32),
        f"{name}_formulas": torch.cat([b["formulas"] for b in loader]).numpy().astype(np.int16),
    }
    for k, v in res.items():
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            out[f"{name}_res_{k}"] = np.array(v, dtype=np.float64 if isinstance(v, float) else np.int64)
    print(name, "seed", seed, "min gap", float(gap.min()), "sampled", sampled,
          {k: v for k, v in res.items() if isinstance(v, (int, float))})
    return out


if __name__ == "__main__":
    torch.set_num_threads(8)
    arrays = {}
    for name, args in RUNS.items():
        arrays.update(run(name, *args))
    np.savez_compressed(os.path.join(HERE, "validate.npz"), **arrays)
