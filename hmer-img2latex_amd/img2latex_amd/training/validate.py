"""The validation pass of the reference's Trainer (img2latex/training/trainer.py:461-665) for the drop-in Seq2SeqModel.

Per batch (trainer.py:510-559): the eval-mode teacher-forced forward (the persistent decode kernel with forced tokens),
then ONE fused kernel over its logits (i2l_teacher_forced_eval): label-smoothed CE sum and count, masked-accuracy counts,
first-index arg max ids and the pad-truncated prediction / target lengths.  The per-batch numbers go into a device record;
nothing is copied to the host and nothing synchronises until ``finish``, which reads the record once.  The batches that
the reference samples for BLEU (its rule and its ``random`` call order, :490-495,537) get their sequence statistics
(i2l_sequence_metrics) enqueued in batch order; ``finish`` turns them into compute_all_metrics' scores
(metrics.py:546-656) with the reference's float64 formulas (i2l_scores_from_statistics: bit-identical).

Not produced: ``token_distribution`` and ``samples`` (analysis / visualisation of compute_all_metrics), the detailed
per-epoch metrics files (use_detailed_metrics) and the sample predictions the reference logs.
"""
from __future__ import annotations

import random as _random
import warnings
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from .. import _lib
from .metrics import device_sequence_statistics, metrics_from_packed

_REC = 6          # int32 words per batch: [loss_sum f32, count f32, correct i64, total i64]


class ValidationTimeout(RuntimeError):
    """The grouped decode of the eval forward gave up on a bounded wait (its logits are NaN) for these batches."""

    def __init__(self, batches: List[int]):
        super().__init__(f"img2latex_amd: non-finite validation loss in batch(es) {batches[:8]}: the grouped decode "
                         "timed out (GPU oversubscribed?); re-run with model.decoder.kernel_flags |= FLAG_NO_GROUP")
        self.batches = batches


def teacher_forced_eval(logits: torch.Tensor, targets: torch.Tensor, pad_token_id: int, label_smoothing: float = 0.1,
                        record: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """i2l_teacher_forced_eval on device tensors, no synchronisation: logits (B,T,V) fp32, targets (B,T) int32.
    Returns (ids (B,T) int32, lengths (2,B) int32 = [pred_len, target_len], record): ``record`` is a (6,) int32 device
    tensor (allocated when not given) whose words [0:2] hold float32 [loss_sum, count] and [2:6] int64 [correct, total]."""
    logits = _lib.require_gpu(logits, "logits")
    targets = _lib.require_gpu(targets, "targets", torch.int32)
    B, T, V = logits.shape
    if tuple(targets.shape) != (B, T):
        raise RuntimeError(f"logits {tuple(logits.shape)} do not match targets {tuple(targets.shape)}")
    dev = logits.device
    L = _lib.lib()
    nbytes = L.i2l_teacher_forced_eval_workspace_bytes(B, T)
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if record is None:
        record = torch.empty((_REC,), dtype=torch.int32, device=dev)
    ids = torch.empty((B, T), dtype=torch.int32, device=dev)
    lens = torch.empty((2, B), dtype=torch.int32, device=dev)
    _lib.check(L.i2l_teacher_forced_eval(
        logits.data_ptr(), targets.data_ptr(), B, T, V, int(pad_token_id), float(label_smoothing), workspace.data_ptr(),
        workspace.numel(), ids.data_ptr(), lens[0].data_ptr(), lens[1].data_ptr(), record.data_ptr(),
        record.data_ptr() + 8, _lib.stream_ptr()), "teacher_forced_eval")
    return ids, lens, record


class BleuSampler:
    """Which validation batches feed BLEU / Levenshtein / token-list accuracy (trainer.py:490-495,537,575-579): the
    first ``bleu_batches``, then each later one with probability bleu_batches / total_batches (all of them when there
    are no more than bleu_batches), drawn with ``rng.random()`` only past the first bleu_batches (short-circuit).  Every
    25th batch the reference also draws ``rng.randint`` for the sample it logs; that draw is kept so that the stream of
    ``rng`` stays the reference's.  Host only."""

    def __init__(self, total_batches: int, bleu_batches: int = 10, rng=None):
        self.bleu_batches = int(bleu_batches)
        self.total_batches = int(total_batches)
        self.sampling_rate = self.bleu_batches / self.total_batches if self.total_batches > self.bleu_batches else 1.0
        self.rng = _random if rng is None else rng
        self.sampled: List[int] = []
        self.sampled_rows = 0

    def __call__(self, batch_idx: int, batch_size: int) -> bool:
        take = batch_idx < self.bleu_batches or self.rng.random() < self.sampling_rate
        if take:
            self.sampled.append(batch_idx)
            self.sampled_rows += batch_size
        if batch_idx % 25 == 0 and batch_idx > 0 and self.sampled_rows > 0 and hasattr(self.rng, "randint"):
            self.rng.randint(0, self.sampled_rows - 1)
        return take


class Validator:
    """Trainer.validate, one ``add(images, formulas)`` per batch and ``finish(epoch, step)`` at the end of the pass.

    ``total_batches`` is what the reference takes from ``len(val_loader)`` for its sampling rate; ``rng`` is any object
    with ``.random()`` (and ``.randint`` for the reference's sample-logging draw every 25 batches), the ``random``
    module by default, as in the reference (BleuSampler).

    ``val_loss`` is the reference's ``sum_b loss_b.item() * B_b / sum_b B_b``: each batch's float32 MEAN over its
    non-pad tokens, weighted by the batch size -- not a mean over all tokens of the pass.

    A batch whose loss sum is not finite makes ``finish`` raise ``ValidationTimeout`` while the decoder may still use
    its grouped kernels (a timed-out grouped decode fills its logits with NaN); ``validate`` then repeats the pass on
    the row-per-workgroup kernels.  With FLAG_NO_GROUP set, a non-finite loss is reported as it is, with a warning.
    """

    def __init__(self, model, pad_token_id: int, total_batches: int, bleu_batches: int = 10,
                 label_smoothing: float = 0.1, rng=None):
        self.model = model
        self.pad = int(pad_token_id)
        self.eps = float(label_smoothing)
        self.total_batches = int(total_batches)
        self.sampler = BleuSampler(total_batches, bleu_batches, rng)
        self.model_type = getattr(model, "model_type", "cnn_lstm")
        dev = next(model.parameters()).device
        self._dev = dev
        self._rec = torch.zeros((max(self.total_batches, 1), _REC), dtype=torch.int32, device=dev)
        self._sizes: List[int] = []
        self._stats: List[torch.Tensor] = []
        self._ws = None

    def _workspace(self, B: int, T: int) -> torch.Tensor:
        nbytes = _lib.lib().i2l_teacher_forced_eval_workspace_bytes(B, T)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self._dev)
        return self._ws

    def add(self, images: torch.Tensor, formulas: torch.Tensor) -> None:
        """One validation batch (trainer.py:510-559): forward, loss, accuracy, and -- when sampled -- the sequence
        statistics for BLEU / Levenshtein / token-list accuracy.  No device->host copy, no synchronisation."""
        from .. import data as D
        batch_idx = len(self._sizes)
        self.model.eval()
        images = images.to(self._dev)                                      # data/utils.py:113-135 prepare_batch
        formulas = formulas.to(self._dev)
        if self.model_type == "resnet_lstm" and images.shape[1] == 1:
            images = D.batch_convert_for_resnet(images)
        with torch.no_grad():
            logits = self.model(images, formulas)
        targets = formulas[:, 1:].to(torch.int32).contiguous()             # :519
        B, T = targets.shape
        if batch_idx >= self._rec.shape[0]:                                # more batches than announced: grow
            self._rec = torch.cat([self._rec, torch.zeros_like(self._rec)])
        ids, lens, _ = teacher_forced_eval(logits, targets, self.pad, self.eps, record=self._rec[batch_idx],
                                           workspace=self._workspace(B, T))
        self._sizes.append(B)
        if self.sampler(batch_idx, B):                                    # trainer.py:537
            self._stats.append(device_sequence_statistics(ids, lens[0], targets, lens[1], 4, self.pad, _max_len=T,
                                                          defer=True))

    @property
    def sampled(self) -> List[int]:
        """Indices of the batches sampled for the sequence metrics so far."""
        return self.sampler.sampled

    def finish(self, epoch: int = 0, step: int = 0) -> Dict:
        """trainer.py:581-643: the validation dict.  One device->host copy."""
        n = len(self._sizes)
        parts = [self._rec[:n].reshape(-1)] + [s.reshape(-1) for s in self._stats]
        host = torch.cat(parts).cpu() if n else torch.zeros((0,), dtype=torch.int32)
        rec = host[:n * _REC].reshape(n, _REC)
        loss = rec[:, 0:2].contiguous().view(torch.float32).numpy()        # [loss_sum, count] per batch
        ct = rec[:, 2:6].contiguous().view(torch.int64).numpy()            # [correct, total] per batch
        bad = [i for i in range(n) if not np.isfinite(loss[i, 0])]
        if bad:
            if not int(self.model.decoder.kernel_flags) & _lib.FLAG_NO_GROUP:
                raise ValidationTimeout(bad)
            warnings.warn(f"img2latex_amd: validation loss is not finite in batch(es) {bad[:8]}", RuntimeWarning)
        val_loss, val_correct, val_tokens, val_samples = 0.0, 0.0, 0, 0
        with np.errstate(invalid="ignore", divide="ignore"):
            for i, bs in enumerate(self._sizes):
                # loss.item() * batch_size (:530): the float32 mean of the batch, then Python floats
                val_loss += float(loss[i, 0] / loss[i, 1]) * bs
                val_correct += int(ct[i, 0])
                val_tokens += int(ct[i, 1])
                val_samples += bs
        out = {
            "val_loss": val_loss / val_samples if val_samples else float("nan"),
            "val_acc": val_correct / val_tokens if val_tokens > 0 else 0,
            "val_samples": val_samples,
            "epoch": epoch,
            "step": step,
        }
        if self._stats:                                                    # compute_all_metrics, metrics.py:546-656
            packed = host[n * _REC:].reshape(-1, 9)
            correct, num_tokens = (int(v) for v in packed[:, 5:7].to(torch.int64).sum(dim=0))
            out["accuracy"] = correct / num_tokens if num_tokens > 0 else 0.0
            out["num_tokens"] = num_tokens
            scores = metrics_from_packed(packed.contiguous())
            out["bleu"] = scores["bleu"]
            out["levenshtein"] = scores["levenshtein"]
            out["batch_size"] = scores["batch_size"]
            out["epoch"] = epoch
        return out


def validate(model, loader: Iterable, pad_token_id: int, bleu_batches: int = 10, label_smoothing: float = 0.1,
             rng=None, epoch: int = 0, step: int = 0) -> Dict:
    """Trainer.validate over any sized iterable of {"images", "formulas"} batches (``len(loader)`` = total_batches,
    as trainer.py:490).  A grouped-decode timeout repeats the pass once on the row-per-workgroup kernels, with the
    RNG restored to where this call found it (when it has getstate / setstate) so the same batches are sampled.
    A resnet_lstm model is validated through whatever ``model.encoder.eval_precision`` says ("bf16" by default); set it
    to "fp32" for a model trained here, so that val_loss comes from the arithmetic being optimised."""
    rng = _random if rng is None else rng
    state = rng.getstate() if hasattr(rng, "getstate") else None

    def one_pass():
        v = Validator(model, pad_token_id, len(loader), bleu_batches, label_smoothing, rng)
        for batch in loader:
            v.add(batch["images"], batch["formulas"])
        return v.finish(epoch, step)

    try:
        return one_pass()
    except ValidationTimeout as exc:
        warnings.warn(f"{exc}; repeating the pass on the row-per-workgroup kernels", RuntimeWarning)
        if state is not None:
            rng.setstate(state)
        dec = model.decoder
        flags = dec.kernel_flags
        dec.kernel_flags = int(flags) | _lib.FLAG_NO_GROUP
        try:
            return one_pass()
        finally:
            dec.kernel_flags = flags
