"""Epoch-end policy of the reference's Trainer.train (img2latex/training/trainer.py:667-822), host arithmetic only:

* ``PlateauSchedule``: torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min", factor=0.5, patience=2) with torch's
  defaults (threshold 1e-4 relative, cooldown 0, min_lr 0, eps 1e-8), trainer.py:94-98,720.  It sets the ``lr``
  attribute of its target (TrainStep: the fused Adam kernel takes the rate as an argument on every step), so no
  optimizer object is needed.
* ``EarlyStopping``: the best / patience / stop bookkeeping of trainer.py:727-766.  Best means a STRICTLY lower
  val_loss (not the scheduler's thresholded test); the patience counter moves only in the no-improvement branch.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple


class PlateauSchedule:
    def __init__(self, target, mode: str = "min", factor: float = 0.5, patience: int = 2, threshold: float = 1e-4,
                 threshold_mode: str = "rel", cooldown: int = 0, min_lr: float = 0.0, eps: float = 1e-8):
        if mode != "min":
            raise NotImplementedError("PlateauSchedule: mode 'min' only (the reference's)")
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError(f"threshold mode {threshold_mode} is unknown!")
        self.target = target
        self.factor, self.patience, self.threshold = float(factor), int(patience), float(threshold)
        self.threshold_mode, self.cooldown, self.min_lr, self.eps = threshold_mode, int(cooldown), float(min_lr), float(eps)
        self.best = math.inf
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def _is_better(self, a: float, best: float) -> bool:
        if self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        return a < best - self.threshold

    def step(self, metrics) -> None:
        """ReduceLROnPlateau.step, in torch's order."""
        current = float(metrics)
        self.last_epoch += 1
        if self._is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old_lr = float(self.target.lr)
            new_lr = max(old_lr * self.factor, self.min_lr)
            if old_lr - new_lr > self.eps:
                self.target.lr = new_lr
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0


class EarlyStopping:
    """trainer.py:727-766.  ``update(val_metrics)`` -> (is_best, stop).  ``best_val_loss`` starts at +inf, or at the
    resumed checkpoint's ``metrics["val_loss"]`` (trainer.py:257-262: ``from_checkpoint``)."""

    def __init__(self, patience: int = 10, best_val_loss: float = math.inf):
        self.patience = int(patience)
        self.best_val_loss = best_val_loss
        self.best_val_metrics: Dict = {}
        self.patience_counter = 0

    @classmethod
    def from_checkpoint(cls, patience: int, checkpoint: Optional[Dict]) -> "EarlyStopping":
        best = math.inf
        if checkpoint is not None and "metrics" in checkpoint and "val_loss" in checkpoint["metrics"]:
            best = checkpoint["metrics"]["val_loss"]
        return cls(patience, best)

    def update(self, val_metrics: Dict) -> Tuple[bool, bool]:
        if val_metrics["val_loss"] < self.best_val_loss:
            self.best_val_loss = val_metrics["val_loss"]
            self.best_val_metrics = val_metrics
            self.patience_counter = 0
            return True, False
        self.patience_counter += 1
        return False, self.patience_counter >= self.patience
