"""Minimum-risk (self-critical) fine-tuning (this package: the reference trains on the gold prefix alone): the decoder is
trained on formulas it sampled itself, each draw weighted by how its Levenshtein similarity to the gold formula -- the
figure ``evaluate`` reports -- compares with the image's other draws.

Per batch of ``B`` images with gold ``formulas (B, T + 1)``, ``N = samples`` draws per image and a mixing weight ``alpha``
(csrc/risk_rules.inc.h states every rule once):

    draws      Seq2SeqModel.sample_multi_device on the step's own (detached) encoder rows, without dropout
    reward     r[b,n] = 1 - d / max(len_draw, len_gold), 1 when both are empty; d the exact Levenshtein distance
    advantage  A[b,n] = r[b,n] - sum_{m != n} r[b,m] / (N - 1)                      (leave-one-out baseline)
    rows       per image the gold row (coefficient alpha, the step's label smoothing) and N rows
               [START, draw through its END, PAD ...] (coefficient (1 - alpha) A[b,n], no smoothing)
    loss       L = (1 / C) sum over token rows of coef[seq] keep CE_smooth[seq](logits, target),
               C = the number of non-PAD targets of all B (N + 1) sequences

``RiskObjective`` holds the arguments and makes the three calls the objective adds in front of the decoder's training
forward; ``TrainStep(risk=...)`` runs them (training/train_step.py).  A PAD id that the model itself sampled before its
END is masked in the loss exactly as a gold PAD is, but it counts in the distance.

Not offered, and refused with a message: a greedy-decode baseline, BLEU as the reward, a constraint on the draws, a
teacher beside the objective, an ensemble as the student, decoders the step-batched sampling loop refuses.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from .. import _lib

REWARDS = ("levenshtein",)
BASELINES = ("leave_one_out",)


def risk_seed(step_seed: int) -> int:
    """The seed of a step's draws from ``train_step.step_seed(seed, step, rank, micro)``: one round of Knuth's 64-bit
    linear congruential generator, cut to the 62 bits ``step_seed`` has.  The map is one to one on those 62 bits, so
    every (step, rank, micro-step) draws its own stream, and it is not the stream the dropout masks hash."""
    return (int(step_seed) * 6364136223846793005 + 1442695040888963407) & 0x3FFFFFFFFFFFFFFF


class RiskObjective:
    def __init__(self, start_token_id: int, end_token_id: int, samples: int = 4, alpha: float = 0.5,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, reward: str = "levenshtein",
                 baseline: str = "leave_one_out", constraint=None):
        """Checked here, without a device.  ``top_k == 0 and top_p == 0`` (the defaults) draw from the model's whole
        distribution -- what the objective's expectation is over; the decode is then given ``top_k = vocab_size``, which
        masks nothing (it refuses 0, 0 itself)."""
        if reward not in REWARDS:
            raise ValueError(f"img2latex_amd: the risk objective's reward is the Levenshtein similarity ({REWARDS[0]!r}); "
                             f"{reward!r} (BLEU, ...) is not offered")
        if baseline not in BASELINES:
            raise ValueError(f"img2latex_amd: the risk objective's baseline is the leave-one-out mean ({BASELINES[0]!r}); "
                             f"{baseline!r} (a greedy decode, ...) is not offered")
        if constraint is not None:
            raise ValueError("img2latex_amd: the risk objective draws without a constraint")
        for name, value in (("start_token_id", start_token_id), ("end_token_id", end_token_id), ("samples", samples),
                            ("top_k", top_k)):
            if isinstance(value, bool) or not isinstance(value, int):
                raise TypeError(f"img2latex_amd: RiskObjective({name}=...) takes an int, got {type(value).__name__}")
        if start_token_id < 0 or end_token_id < 0:
            raise ValueError(f"img2latex_amd: token ids are >= 0, got start {start_token_id}, end {end_token_id}")
        if not 2 <= samples <= _lib.MAX_NBEST:
            raise ValueError(f"img2latex_amd: risk samples must be 2 .. {_lib.MAX_NBEST} (the leave-one-out baseline needs "
                             f"two draws), got {samples}")
        alpha, temperature, top_p = float(alpha), float(temperature), float(top_p)
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"img2latex_amd: risk alpha must be in [0, 1], got {alpha}")
        if not (0.0 < temperature < math.inf):
            raise ValueError(f"img2latex_amd: risk temperature must be finite and > 0, got {temperature}")
        if top_k < 0:
            raise ValueError(f"img2latex_amd: risk top_k must be >= 0, got {top_k}")
        if not 0.0 <= top_p <= 1.0:
            raise ValueError(f"img2latex_amd: risk top_p must be in [0, 1], got {top_p}")
        self.start, self.end, self.samples, self.alpha = start_token_id, end_token_id, samples, alpha
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p

    def check_model(self, model) -> None:
        """The student is one Seq2SeqModel whose decoder knows both token ids."""
        if not hasattr(model, "sample_multi_device") or hasattr(model, "models"):
            raise TypeError("img2latex_amd: the risk objective trains one Seq2SeqModel (an ensemble is not a student), got "
                            f"{type(model).__name__}")
        if max(self.start, self.end) >= int(model.vocab_size):
            raise ValueError(f"img2latex_amd: token ids {self.start}, {self.end} outside the vocabulary of {int(model.vocab_size)}")

    def draw(self, model, enc: torch.Tensor, steps: int, seed: int) -> torch.Tensor:
        """``samples`` formulas per row of ``enc`` (B, E) from the model as it stands: (B, samples, steps) int32, -1 behind
        END.  One call of the step-batched sampling loop on the shared encoder rows; the decode entries apply no dropout,
        whatever mode the model is in.  A decoder that loop refuses raises RuntimeError there."""
        top_k = self.top_k if (self.top_k or self.top_p) else int(model.vocab_size)
        with torch.no_grad():
            out = model.sample_multi_device(enc.detach(), self.start, self.end, int(steps), self.samples, self.temperature,
                                            top_k, self.top_p, int(seed))
        return out["ids"]

    def assemble(self, formulas: torch.Tensor, draws: torch.Tensor, pad_id: int, label_smoothing: float) -> Dict[str, torch.Tensor]:
        """i2l_risk_rows: formulas (B, T + 1) int32, draws (B, samples, T) int32 -> "rows" (B (samples + 1), T + 1) int32,
        "coef", "smooth" fp32 and "part" int32 per sequence, "dist", "len" int32 and "reward", "advantage" fp32 (B, samples)."""
        formulas = _lib.require_gpu(formulas, "formulas", torch.int32)
        draws = _lib.require_gpu(draws, "draws", torch.int32)
        B, T1 = formulas.shape
        N, T = self.samples, T1 - 1
        if tuple(draws.shape) != (B, N, T):
            raise RuntimeError(f"img2latex_amd: draws are {tuple(draws.shape)}, expected {(B, N, T)}")
        dev = formulas.device
        out = dict(rows=torch.empty((B * (N + 1), T + 1), dtype=torch.int32, device=dev),
                   coef=torch.empty(B * (N + 1), dtype=torch.float32, device=dev),
                   smooth=torch.empty(B * (N + 1), dtype=torch.float32, device=dev),
                   part=torch.empty(B * (N + 1), dtype=torch.int32, device=dev),
                   dist=torch.empty((B, N), dtype=torch.int32, device=dev),
                   len=torch.empty((B, N), dtype=torch.int32, device=dev),
                   reward=torch.empty((B, N), dtype=torch.float32, device=dev),
                   advantage=torch.empty((B, N), dtype=torch.float32, device=dev))
        _lib.check(_lib.lib().i2l_risk_rows(formulas.data_ptr(), draws.data_ptr(), B, N, T, self.start, self.end, int(pad_id),
                                            self.alpha, float(label_smoothing), out["rows"].data_ptr(), out["coef"].data_ptr(),
                                            out["smooth"].data_ptr(), out["part"].data_ptr(), out["dist"].data_ptr(),
                                            out["len"].data_ptr(), out["reward"].data_ptr(), out["advantage"].data_ptr(),
                                            _lib.stream_ptr()), "risk_rows")
        return out


def rows_repeat(x: torch.Tensor, times: int) -> torch.Tensor:
    """i2l_rows_repeat: x (rows, width) fp32 -> (rows * times, width), row r of x at rows r * times .. r * times + times - 1."""
    x = _lib.require_gpu(x, "rows")
    rows, width = x.shape
    out = torch.empty((rows * int(times), width), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().i2l_rows_repeat(x.data_ptr(), rows, width, int(times), out.data_ptr(), _lib.stream_ptr()), "rows_repeat")
    return out


def rows_fold(x: torch.Tensor, times: int) -> torch.Tensor:
    """i2l_rows_fold, the gradient of ``rows_repeat``: x (rows * times, width) fp32 -> (rows, width), each the fp32 sum of
    its ``times`` rows in order."""
    x = _lib.require_gpu(x, "rows")
    total, width = x.shape
    if total % int(times):
        raise RuntimeError(f"img2latex_amd: {total} rows do not fold by {times}")
    out = torch.empty((total // int(times), width), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().i2l_rows_fold(x.data_ptr(), total // int(times), width, int(times), out.data_ptr(), _lib.stream_ptr()),
               "rows_fold")
    return out
