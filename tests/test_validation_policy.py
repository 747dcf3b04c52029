"""Epoch-end policy of Trainer.train on the host (trainer.py:490-495,537,667-766): the plateau LR schedule against
torch's ReduceLROnPlateau, the best / patience / stop bookkeeping against a restatement of the reference's branch, and
the BLEU sampling rule against the batches the reference sampled (tests/golden/validate.npz).  No GPU."""
import json
import math
import os
import random
import types

import numpy as np
import pytest
import torch

from img2latex_amd.training import BleuSampler, EarlyStopping, PlateauSchedule

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

SEQUENCES = {
    "improving": [5.0, 4.0, 3.0, 2.5, 2.0, 1.5],
    "plateau": [3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0],
    "inside_threshold": [1.0, 0.99995, 0.9999, 0.99991, 0.99985, 0.9998, 0.99979, 0.99975, 0.9997],
    "nan": [2.0, float("nan"), float("nan"), float("nan"), 1.9, float("nan"), 1.0, float("nan"), float("nan"), 2.0],
    "inf_then_finite": [float("inf"), float("inf"), float("inf"), float("inf"), 5.0, 5.0, 5.0, 5.0],
    "mixed": [4.0, 3.9, 3.95, 3.99, 4.2, 3.5, 3.5, 3.4999, 3.6, 3.7, 3.8, 1.0, 1.0, 1.0, 1.0],
    "long_plateau": [1.0] * 40,                     # 0.5^13 x 1e-3 < eps: the LR stops moving
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
@pytest.mark.parametrize("lr", [1e-3, 1e-6])
def test_plateau_schedule_matches_torch(name, lr):
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=2)   # trainer.py:94-98
    target = types.SimpleNamespace(lr=lr)
    ours = PlateauSchedule(target, mode="min", factor=0.5, patience=2)
    for i, v in enumerate(SEQUENCES[name]):
        ref.step(v)
        ours.step(v)
        assert target.lr == opt.param_groups[0]["lr"], (name, i, target.lr, opt.param_groups[0]["lr"])
        assert ours.num_bad_epochs == ref.num_bad_epochs


def test_plateau_schedule_lr_decay_stops_below_eps():
    target = types.SimpleNamespace(lr=3e-8)
    s = PlateauSchedule(target)
    for _ in range(4):
        s.step(1.0)
    assert target.lr == 1.5e-8                      # 3e-8 - 1.5e-8 > 1e-8: reduced once
    for _ in range(3):
        s.step(1.0)
    assert target.lr == 1.5e-8                      # 1.5e-8 - 7.5e-9 < 1e-8: torch leaves it


def _reference_policy(losses, patience, best=float("inf")):
    """trainer.py:727-766, the branch as written."""
    best_val_loss, patience_counter, log = best, 0, []
    for v in losses:
        if v < best_val_loss:
            best_val_loss = v
            patience_counter = 0
            log.append((True, False))
        else:
            patience_counter += 1
            if patience_counter >= patience:
                log.append((False, True))
                break
            log.append((False, False))
    return log, best_val_loss


@pytest.mark.parametrize("name", sorted(SEQUENCES))
@pytest.mark.parametrize("patience", [1, 2, 3, 10])
def test_early_stopping_matches_reference(name, patience):
    want, want_best = _reference_policy(SEQUENCES[name], patience)
    es = EarlyStopping(patience)
    got = []
    for v in SEQUENCES[name]:
        got.append(es.update({"val_loss": v}))
        if got[-1][1]:
            break
    assert got == want
    assert es.best_val_loss == want_best or (math.isnan(want_best) and math.isnan(es.best_val_loss))


def test_early_stopping_resume_best_from_checkpoint():
    es = EarlyStopping.from_checkpoint(2, {"metrics": {"val_loss": 1.5}})        # trainer.py:257-262
    assert es.best_val_loss == 1.5
    assert es.update({"val_loss": 1.5}) == (False, False)                        # strict improvement only
    assert es.update({"val_loss": 1.4}) == (True, False)
    assert EarlyStopping.from_checkpoint(2, {"metrics": {"loss": 3.0}}).best_val_loss == math.inf
    assert EarlyStopping.from_checkpoint(2, None).best_val_loss == math.inf


def _sampling_replay(total, bleu_batches, rng, size=4):
    """Validator's host decision per batch (BleuSampler), no device needed."""
    sampler = BleuSampler(total, bleu_batches, rng)
    picked = [i for i in range(total) if sampler(i, size)]
    assert picked == sampler.sampled
    return picked, sampler.sampling_rate


@pytest.mark.parametrize("name", ["tiny_l1", "odd_dims"])
def test_sampling_rule_replays_reference(name):
    d = np.load(os.path.join(GOLDEN, "validate.npz"))
    gen = json.loads(str(d[f"{name}_gen_json"]))
    random.seed(gen["rng_seed"])
    picked, _ = _sampling_replay(len(gen["sizes"]), gen["bleu_batches"], random)
    assert picked == d[f"{name}_sampled"].tolist()
    assert gen["bleu_batches"] < len(picked) < len(gen["sizes"])    # the random branch was exercised both ways


def test_sampling_rate_all_batches_when_few():
    picked, rate = _sampling_replay(3, 10, random.Random(0))
    assert rate == 1.0 and picked == [0, 1, 2]


def test_sampling_rule_draw_order():
    """No draw for the first bleu_batches batches (short-circuit), one per later batch, plus the reference's
    sample-logging randint every 25th batch once something was sampled (trainer.py:575-579)."""
    calls = []

    class Rng:
        def random(self):
            calls.append("random")
            return 0.99

        def randint(self, a, b):
            calls.append(("randint", a, b))
            return a

    picked, rate = _sampling_replay(60, 10, Rng(), size=2)
    assert rate == 10 / 60 and picked == list(range(10))
    want = ["random"] * 16 + [("randint", 0, 19)] + ["random"] * 25 + [("randint", 0, 19)] + ["random"] * 9
    assert calls == want
