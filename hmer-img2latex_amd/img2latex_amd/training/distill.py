"""Word-level knowledge distillation (this package: the reference trains on the data set's tokens alone): the student
trains against the token distribution of one model or of an ensemble at every teacher-forced position, so that what
``--ensemble`` buys at decode time, for every image, is bought once, at training time, and lands in ONE checkpoint that
every fast decode path reads unchanged.

``Teacher`` holds the frozen members and produces their logits for a batch; ``TrainStep(teacher=...)`` hands those to
i2l_ce_distill_fwd_bwd (csrc/distill_rules.inc.h states the loss, csrc/train_distill.inc.h evaluates it in one fused
launch) in place of the plain cross entropy.  The members' logits are combined inside that launch by the ensemble decode's
own rule (csrc/ensemble_rules.inc.h); nothing of size (rows, V) is formed on the way.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..model.ensemble import EnsembleModel, combine_rule, member_weights


def check_distill_arguments(alpha: float, temperature: float) -> Tuple[float, float]:
    """0 <= alpha <= 1 and a finite temperature > 0, as floats; ValueError otherwise (what the C entry refuses too)."""
    alpha, temperature = float(alpha), float(temperature)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"img2latex_amd: distill_alpha must be in [0, 1], got {alpha}")
    if not (0.0 < temperature < float("inf")):
        raise ValueError(f"img2latex_amd: distill_temperature must be finite and > 0, got {temperature}")
    return alpha, temperature


class Teacher:
    """``model``: one ``Seq2SeqModel``, or an ``EnsembleModel`` -- then its members, its ``member_weights`` and its
    combination rule are the teacher's.  The members are put in eval mode and frozen (``requires_grad_(False)``); they
    must not share modules with the student.  ``vocab_size``: the student's, checked here when given and by
    ``TrainStep`` in any case."""

    def __init__(self, model, vocab_size: Optional[int] = None):
        if isinstance(model, EnsembleModel):
            self.members = list(model.models)
            self.weights = list(model.decoder.weights)
            self.combine = int(model.decoder.combine)
        else:
            self.members = [model]
            self.weights = member_weights(None, 1)
            self.combine = combine_rule("logprob")
        if not 1 <= len(self.members) <= _lib.MAX_ENSEMBLE:
            raise ValueError(f"img2latex_amd: a teacher has 1 .. {_lib.MAX_ENSEMBLE} members, got {len(self.members)}")
        for m in self.members:
            m.eval()
            m.requires_grad_(False)
        self.vocab_size = int(self.members[0].vocab_size)
        self.check_vocab(self.vocab_size if vocab_size is None else vocab_size)

    def check_vocab(self, vocab_size: int) -> None:
        """Every member's vocabulary size must be the student's: the loss compares distributions column by column."""
        sizes = [int(m.vocab_size) for m in self.members]
        if any(v != int(vocab_size) for v in sizes):
            raise ValueError(f"img2latex_amd: the teacher's vocabulary sizes {sizes} differ from the student's {int(vocab_size)}")

    def to(self, device) -> "Teacher":
        for m in self.members:
            m.to(device)
        return self

    def logits(self, images: torch.Tensor, formulas: torch.Tensor) -> List[torch.Tensor]:
        """The members' eval-mode teacher-forced forward (``model(images, formulas)`` as training/validate.py calls it)
        under ``torch.no_grad()`` on the current stream: one (B, T, V) fp32 device tensor per member, T =
        formulas.shape[1] - 1.  A ResNet member is given ``batch_convert_for_resnet(images)`` when the batch has one
        channel; a three-channel batch for a one-channel member is refused.  (A grouped decode kernel that times out on
        an oversubscribed GPU leaves NaN logits; the step's loss is then NaN and the optimizer skips the update.)"""
        from ..data import batch_convert_for_resnet
        out, converted = [], None
        for m in self.members:
            x = images
            want = int(m.encoder.channels)
            if images.shape[1] == 1 and want == 3 and getattr(m, "model_type", "cnn_lstm") == "resnet_lstm":
                if converted is None:
                    converted = batch_convert_for_resnet(images)
                x = converted
            elif images.shape[1] != want:
                raise RuntimeError(f"img2latex_amd: a {images.shape[1]}-channel batch for a {want}-channel teacher member")
            m.eval()
            with torch.no_grad():
                lg = m(x, formulas)
            if lg.dtype != torch.float32:
                lg = lg.float()
            if lg.stride(2) != 1 or lg.stride(0) != lg.shape[1] * lg.stride(1):
                lg = lg.contiguous()
            out.append(lg)
        return out

    @classmethod
    def from_checkpoints(cls, paths: Sequence[str], weights: Optional[Sequence[float]] = None, combine: str = "logprob",
                         device=None):
        """Loads the members the way ``Predictor.from_checkpoints`` does (tokenizer table and model from each
        checkpoint's own config, strict ``load_state_dict``) -> ``(teacher, tables)``: ``tables`` are the members'
        ``TokenTable`` s, one per path, for the caller to compare with the student's tokenizer.  ValueError for a bad
        count, weight or rule, and for members of different vocabulary sizes."""
        from .predictor import TokenTable, model_from_checkpoint_config
        paths = list(paths)
        if not 1 <= len(paths) <= _lib.MAX_ENSEMBLE:
            raise ValueError(f"img2latex_amd: a teacher has 1 .. {_lib.MAX_ENSEMBLE} checkpoints, got {len(paths)}")
        weights = member_weights(weights, len(paths))
        combine_rule(combine)
        models, tables = [], []
        for path in paths:
            checkpoint = torch.load(path, map_location="cpu", weights_only=False)
            tcfg = checkpoint.get("tokenizer_config", {})
            table = TokenTable(tcfg.get("token_to_id"), tcfg.get("special_tokens"), tcfg.get("max_sequence_length", 141))
            model = model_from_checkpoint_config(checkpoint.get("config", {}), table.vocab_size)
            model.load_state_dict(checkpoint["model_state_dict"])
            models.append(model)
            tables.append(table)
        teacher = cls(EnsembleModel(models, weights, combine))
        if device is not None:
            teacher.to(device)
        return teacher, tables
