"""One optimisation step of the reference's Trainer, fp32 branch (trainer.py:303-343):

    targets = formulas[:, 1:]                                        :306
    outputs = model(images, formulas)                                :334
    loss = CrossEntropyLoss(ignore_index=PAD, label_smoothing=0.1)   :111-115,335-336
    loss.backward(); clip_grad_norm_(5.0); Adam(lr, weight_decay).step(); zero_grad   :337-343

(with ``teacher=``: the distillation loss of training/distill.py in place of the plain cross entropy; with ``risk=``: the
minimum-risk objective of training/risk.py -- the decoder runs on the gold row and on N draws of every image)

run entirely with the HIP kernels: training forward of encoder and decoder, fused CE, BPTT,
conv/linear backward writing straight into ONE flat gradient buffer, one all-reduce of that
buffer when data-parallel, then a fused clip + Adam over the flat parameter buffer.  No host
synchronisation inside the step; ``loss`` / ``total_norm`` stay on the device until read.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _lib
from ..model._train_fn import (decoder_train_backward, decoder_train_forward, encoder_train_backward,
                               encoder_train_forward)
from .dp import OverlappedAllReduce, broadcast_parameters, rank_of
from .risk import RiskObjective, risk_seed, rows_fold, rows_repeat


def step_seed(seed: int, step: int, rank: int, micro: int) -> int:
    """The dropout seed of one forward_backward: one mask stream per (seed, optimizer step, data-parallel rank,
    accumulation micro-step).  The kernels hash the LOCAL element index, so without the rank every replica would reuse
    rank 0's masks for its own rows.  62 bits: what LSTMDecoder.forward draws too."""
    return ((seed * 1000003 + step) * 4099 + rank + 7919 * micro) & 0x3FFFFFFFFFFFFFFF


class TrainStep:
    def __init__(self, model, lr: float = 1e-3, weight_decay: float = 1e-4, clip_grad_norm: float = 5.0,
                 pad_token_id: int = 0, label_smoothing: float = 0.1, betas=(0.9, 0.999), eps: float = 1e-8,
                 process_group=None, seed: int = 0, overlap_all_reduce: bool = True, side_wgrad: bool = True,
                 teacher=None, distill_alpha: float = 0.5, distill_temperature: float = 2.0, risk=None):
        # teacher (training/distill.py: Teacher, or None): the loss becomes distill_alpha x today's cross entropy +
        # (1 - distill_alpha) x temperature^2 KL(teacher || student) at distill_temperature (i2l_ce_distill_fwd_bwd).  With
        # None nothing changes: the same entry is called with the same arguments.  Refused before anything else is looked at
        self.teacher = teacher
        if teacher is not None:
            from .distill import Teacher, check_distill_arguments
            if not isinstance(teacher, Teacher):
                raise TypeError("img2latex_amd: TrainStep(teacher=...) takes a training.distill.Teacher "
                                f"(wrap the model: Teacher(model)), got {type(teacher).__name__}")
            self.distill_alpha, self.distill_temperature = check_distill_arguments(distill_alpha, distill_temperature)
            teacher.check_vocab(model.vocab_size)
        # risk (training/risk.py: RiskObjective, or None): the step draws risk.samples formulas per image from the model
        # itself and trains on the gold row and on the draws, each draw weighted by its leave-one-out advantage in
        # Levenshtein similarity.  With None nothing changes.  Refused, like a bad teacher, before a device is looked at
        self.risk = risk
        if risk is not None:
            if not isinstance(risk, RiskObjective):
                raise TypeError("img2latex_amd: TrainStep(risk=...) takes a training.risk.RiskObjective, got "
                                f"{type(risk).__name__}")
            if teacher is not None:
                raise ValueError("img2latex_amd: TrainStep takes a teacher or a risk objective, not both")
            risk.check_model(model)
        self.model = model
        self.lr, self.weight_decay, self.clip = lr, weight_decay, clip_grad_norm
        self.pad, self.smoothing, self.betas, self.eps = pad_token_id, label_smoothing, betas, eps
        self.group = process_group
        self.step_count = 0
        self.seed = seed
        self.rank = rank_of(process_group)           # mixed into the dropout seed: every rank draws its own masks
        params = [p for p in model.parameters()]
        if not params or not params[0].is_cuda:
            raise RuntimeError("img2latex_amd: TrainStep needs the model on a ROCm device (no CPU fallback)")
        dev = params[0].device
        # 16-byte aligned slices of one flat buffer; parameters become views into it (state_dict unchanged).  The conv
        # stack's parameters go LAST: their gradients are the last the backward pass produces, so everything in front
        # of them can be all-reduced while the conv backward still runs (dp.OverlappedAllReduce)
        self.offsets: Dict[str, int] = {}
        # only what requires a gradient is optimised: torch.optim.Adam skips parameters whose .grad is None, i.e. the
        # frozen part of a ResNet backbone (encoder.py:201-210) gets neither an update nor weight decay
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        is_late = lambda n: n.startswith("encoder.cnn_layers.") or n.startswith("encoder.resnet.")
        late = [(n, p) for n, p in named if is_late(n)]
        early = [(n, p) for n, p in named if not is_late(n)]
        off = 0
        for name, p in early + late:
            if late and name == late[0][0]:
                self.n_early = off
            self.offsets[name] = off
            off += (p.numel() + 3) // 4 * 4
        self.n = off
        if not late:
            self.n_early = off
        self.flat_params = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(self.n + 4, dtype=torch.float32, device=dev)   # [n] loss sum, [n+1] count
        self.exp_avg = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4, dtype=torch.float32, device=dev)
        # distillation only: [sum of hard, sum of soft] of the last forward_backward, unweighted, and its non-PAD count;
        # this rank's own rows (never all-reduced)
        self.loss_parts = torch.zeros(2, dtype=torch.float32, device=dev) if teacher is not None else None
        self._parts_count = None
        # the risk objective only: [loss sum, non-PAD count] of the gold rows, then of the draws' rows, unweighted, and the
        # mean reward of the last forward_backward's draws; this rank's own rows
        self.risk_parts = torch.zeros(4, dtype=torch.float32, device=dev) if risk is not None else None
        self.risk_batch = None        # what RiskObjective.assemble returned for the last forward_backward, plus "draws"
        self.grad_views: Dict[str, torch.Tensor] = {}
        with torch.no_grad():
            for name, p in named:
                o = self.offsets[name]
                view = self.flat_params[o:o + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
                self.grad_views[name] = self.flat_grads[o:o + p.numel()].view_as(p)
        broadcast_parameters(self.flat_params, 0, self.group)
        # overlap_all_reduce=False: literally ONE all-reduce of the whole flat buffer after the backward pass (BASELINE
        # north_star's wording); True (default): the same element-wise sums issued in two pieces, the first -- everything
        # but the conv gradients -- as soon as the FC backward is enqueued, beside ~1 ms of conv backward (dp.py)
        self.overlap_all_reduce = bool(overlap_all_reduce)
        # weight gradients on two side streams OWNED BY THIS OBJECT beside the data-gradient chain (csrc/api.hip: i2l_lanes;
        # r03 used streams hidden inside the library); False keeps the whole backward on one stream (same kernels, same
        # sums either way)
        self.side_wgrad = bool(side_wgrad)
        self._lanes = _lib.Lanes(dev, 2) if self.side_wgrad else None
        self._side_keep = []          # buffers the side lanes' kernels still read; released after the join
        self._accum = None            # gradient accumulation (micro_step): sum over micro-batches of grad(mean loss) / k
        self._micro = 0               # micro-batches accumulated since the last update
        self._ar_stream = None        # helper stream the early all-reduce piece is issued from (data parallel only)
        self._reducer = OverlappedAllReduce(self.flat_grads, self.n_early, self.group)
        L = _lib.lib()
        # zeroed once: besides scratch it carries the count of skipped (non-finite) updates across calls
        self._opt_ws = torch.zeros(L.i2l_optimizer_workspace_bytes(), dtype=torch.uint8, device=dev)

    # ------------------------------------------------------------------
    def forward_backward(self, images: torch.Tensor, formulas: torch.Tensor) -> torch.Tensor:
        """Training forward + backward for this rank's shard; fills flat_grads (gradient of the SUM of the
        per-token losses), flat_grads[n] = loss sum, flat_grads[n+1] = non-PAD count.  Returns logits.  With a teacher
        the loss is the distillation loss and ``loss_parts`` holds its two unweighted sums.  With a risk objective the
        decoder runs on ``B (samples + 1)`` sequences -- per image the gold row, then its draws (``risk_batch``) -- and the
        logits returned are theirs; the count is the number of non-PAD targets of all of them."""
        model = self.model
        L = _lib.lib()
        formulas = formulas.to(torch.int32) if formulas.dtype != torch.int32 else formulas
        tokens_in = formulas[:, :-1].contiguous()                    # seq2seq.py:115-120
        targets = formulas[:, 1:].contiguous()                       # trainer.py:306
        B, T = tokens_in.shape
        self.step_seed = step_seed(self.seed, self.step_count, self.rank, self._micro)
        enc, enc_state = encoder_train_forward(model.encoder, images)
        if self.risk is not None:
            # the draws come from the encoder rows of this very forward; the decoder then sees every row samples + 1 times
            tokens_in, targets = self._risk_rows(enc, formulas, T)
            times = self.risk.samples + 1
            enc = rows_repeat(enc, times)
        logits, dec_state = decoder_train_forward(model.decoder, enc, tokens_in, self.step_seed)
        V = logits.shape[-1]
        dlogits = torch.empty_like(logits)
        if self.risk is not None:
            self._risk_loss(logits, targets, dlogits)
        elif self.teacher is None:
            nbytes = L.i2l_ce_workspace_bytes(B * T)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
            _lib.check(L.i2l_ce_label_smooth_fwd_bwd(logits.data_ptr(), targets.data_ptr(), B * T, V, self.pad,
                                                     self.smoothing, ws.data_ptr(), nbytes, dlogits.data_ptr(),
                                                     self.flat_grads.data_ptr() + 4 * self.n, _lib.stream_ptr()),
                       "ce_label_smooth_fwd_bwd")
        else:
            self._distill_loss(images, formulas, logits, targets, dlogits)
        dgr = {n[len("decoder."):]: g for n, g in self.grad_views.items() if n.startswith("decoder.")}
        # weight gradients feed nothing in the backward chain: they go to this object's side lanes and fill the launch
        # gaps and tile tails of the data-gradient chain; the join at the end of this method orders them before the
        # all-reduce / Adam.  Everything those kernels read is held in _side_keep until then.
        side = self._lanes.handle if self.side_wgrad else None
        self._join_side()                                            # a previous forward_backward() without apply()
        denc = decoder_train_backward(model.decoder, dec_state, dlogits, dgr, lanes=side)
        if side:
            self._side_keep.extend((dec_state, dlogits, enc_state, images, tokens_in))
        if self.risk is not None:
            if side:
                self._side_keep.append(enc)                          # the repeated rows the side lanes still read
            denc = rows_fold(denc, times)                            # d(repeat): the rows of an image summed, in order
        egr = {n[len("encoder."):]: g for n, g in self.grad_views.items() if n.startswith("encoder.")}

        def after_linear():
            # decoder + FC gradients are final once the FC backward is enqueued -- and, with side-stream weight
            # gradients, once the side lanes have produced them: the early all-reduce is issued from a helper stream that
            # waits for both, so that the conv backward on the step's own stream is not held up by the join
            if not self._reducer._active():
                return
            if not self._side_keep:
                self._reducer.start_early()
                return
            main = torch.cuda.current_stream()
            if self._ar_stream is None:
                self._ar_stream = torch.cuda.Stream(device=self.flat_grads.device)
            self._ar_stream.wait_stream(main)
            with torch.cuda.stream(self._ar_stream):
                self._lanes.join()
                self._reducer.start_early()
        encoder_train_backward(model.encoder, enc_state, denc, egr,
                               after_linear=after_linear if self.overlap_all_reduce else None, lanes=side,
                               keep=self._side_keep)
        self._join_side()          # flat_grads is complete for whatever the current stream does next (all-reduce, Adam, a reader)
        return logits

    def _distill_loss(self, images, formulas, logits, targets, dlogits) -> None:
        """The teacher's logits for this batch and i2l_ce_distill_fwd_bwd: sum and count where the plain loss puts them
        (flat_grads[n], [n+1]), the two parts in ``loss_parts``."""
        L = _lib.lib()
        B, T, V = logits.shape
        rows = self.teacher.logits(images, formulas)
        records = (_lib.DistillTeacher * len(rows))()
        for m, lg in enumerate(rows):
            if tuple(lg.shape) != (B, T, V) or not lg.is_cuda:
                raise RuntimeError(f"img2latex_amd: teacher member {m} gave logits {tuple(lg.shape)} on {lg.device}, the "
                                   f"student's are {(B, T, V)} on {logits.device}")
            records[m] = _lib.DistillTeacher(lg.data_ptr(), lg.stride(1), self.teacher.weights[m])
        nbytes = L.i2l_ce_distill_workspace_bytes(B * T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
        _lib.check(L.i2l_ce_distill_fwd_bwd(logits.data_ptr(), targets.data_ptr(), B * T, V, self.pad, self.smoothing,
                                            records, len(rows), self.teacher.combine, self.distill_temperature,
                                            self.distill_alpha, ws.data_ptr(), nbytes, dlogits.data_ptr(),
                                            self.flat_grads.data_ptr() + 4 * self.n, self.loss_parts.data_ptr(),
                                            _lib.stream_ptr()), "ce_distill_fwd_bwd")
        self._parts_count = self.flat_grads[self.n + 1].clone()      # this rank's count: apply() all-reduces the slot
        del rows, records, ws                                        # stream-ordered: the allocator reuses them after the launch

    def _risk_rows(self, enc, formulas, T):
        """The step's draws and i2l_risk_rows -> the decoder's (tokens_in, targets) of the B (samples + 1) sequences;
        ``risk_batch`` keeps everything the kernel wrote."""
        draws = self.risk.draw(self.model, enc, T, risk_seed(self.step_seed))
        batch = self.risk.assemble(formulas, draws, self.pad, self.smoothing)
        batch["draws"] = draws
        self.risk_batch = batch
        return batch["rows"][:, :-1].contiguous(), batch["rows"][:, 1:].contiguous()

    def _risk_loss(self, logits, targets, dlogits) -> None:
        """i2l_ce_weighted_fwd_bwd on the assembled sequences: the weighted sum and the count of ALL non-PAD targets where
        the plain loss puts them (flat_grads[n], [n+1]), the two unweighted parts in ``risk_parts``."""
        L = _lib.lib()
        rows, T, V = logits.shape
        batch = self.risk_batch
        nbytes = L.i2l_ce_weighted_workspace_bytes(rows * T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
        _lib.check(L.i2l_ce_weighted_fwd_bwd(logits.data_ptr(), targets.data_ptr(), rows, T, V, self.pad,
                                             batch["coef"].data_ptr(), batch["smooth"].data_ptr(), batch["part"].data_ptr(),
                                             ws.data_ptr(), nbytes, dlogits.data_ptr(),
                                             self.flat_grads.data_ptr() + 4 * self.n, self.risk_parts.data_ptr(),
                                             _lib.stream_ptr()), "ce_weighted_fwd_bwd")
        del ws                                                       # stream-ordered: the allocator reuses it after the launch

    def _loss_parts(self) -> Dict[str, torch.Tensor]:
        """{} for the plain loss; with a teacher the last forward_backward's hard and soft loss per non-PAD token; with a
        risk objective its mean reward and the unweighted cross entropy per non-PAD token of the gold rows (hard_loss) and
        of the draws' rows (risk_loss).  Device tensors."""
        if self.risk is not None:
            parts = self.risk_parts
            return dict(reward=self.risk_batch["reward"].mean(), hard_loss=parts[0] / parts[1].clamp(min=1.0),
                        risk_loss=parts[2] / parts[3].clamp(min=1.0))
        if self.teacher is None:
            return {}
        per_token = self.loss_parts / self._parts_count.clamp(min=1.0)
        return dict(hard_loss=per_token[0], soft_loss=per_token[1])

    def _join_side(self, clear: bool = True) -> None:
        """The current stream waits for the side lanes' weight gradients (no-op when none are pending)."""
        if self._side_keep:
            self._lanes.join()
            if clear:
                # the buffers may be reused by later work on this stream only: that work is ordered after the join
                self._side_keep = []

    def apply(self) -> None:
        """All-reduce (data parallel), then clip + Adam; bumps the step counter."""
        L = _lib.lib()
        self._join_side()
        self._reducer.finish()
        self.step_count += 1
        _lib.check(L.i2l_grad_clip_adam_step(
            self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(),
            self.exp_avg_sq.data_ptr(), self.n, self.flat_grads.data_ptr() + 4 * (self.n + 1), float(self.clip),
            float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
            self.step_count, self._opt_ws.data_ptr(), self._opt_ws.numel(), self.stats.data_ptr(),
            _lib.stream_ptr()), "grad_clip_adam_step")
        # the kernel wrote the parameters through raw pointers: tell autograd / the weight-image caches
        # (LSTMDecoder.prepare, ResNetEncoder) that they changed
        for p in self.model.parameters():
            torch.autograd.graph.increment_version(p)

    def step(self, images: torch.Tensor, formulas: torch.Tensor) -> Dict[str, torch.Tensor]:
        """trainer.py:303-343 for one batch.  Returns device tensors (no sync): loss, total_norm, count, skipped -- and
        with a teacher ``hard_loss`` / ``soft_loss``, the two unweighted parts of the loss per non-PAD token of this rank;
        with a risk objective ``reward`` (the mean over this rank's draws), ``hard_loss`` and ``risk_loss``.
        ``skipped`` is 1.0 when the gradients were not finite (e.g. a grouped recurrence kernel timed out on a shared
        GPU and poisoned its outputs with NaN): the fused clip + Adam kernel then leaves parameters and moments
        untouched -- on every rank, since the all-reduce spreads the NaN -- and the caller may simply repeat the
        batch, if it keeps happening with ``model.decoder.kernel_flags |= FLAG_NO_GROUP``."""
        self.model.train()
        self.forward_backward(images, formulas)
        self.apply()
        count = self.flat_grads[self.n + 1]
        return dict(loss=self.flat_grads[self.n] / count.clamp(min=1.0), total_norm=self.stats[0], count=count,
                    skipped=self.stats[3], **self._loss_parts())

    def micro_step(self, images: torch.Tensor, formulas: torch.Tensor, accumulation_steps: int, update: bool) -> Dict[str, torch.Tensor]:
        """Gradient accumulation, trainer.py:345-383 (the shipped configuration: accumulation_steps 4): every micro-batch
        contributes the gradient of ITS mean loss divided by ``accumulation_steps`` (``loss = criterion(...) /
        accumulation_steps; loss.backward()``), and with ``update`` -- every accumulation_steps-th batch or the last one of
        the epoch, :374 -- the sum is clipped and Adam steps.  Data parallel: a micro-batch's mean is over the GLOBAL
        micro-batch, so its [loss sum, count] pair is all-reduced at once (8 bytes) and the accumulated gradients once, at
        the update.  Returns the micro-batch's mean loss (what the reference logs, :386-388) and, after an update,
        ``total_norm`` / ``skipped``."""
        import torch.distributed as dist
        if accumulation_steps < 1:
            raise ValueError("accumulation_steps must be >= 1")
        if accumulation_steps == 1 and self._micro == 0 and update:
            return self.step(images, formulas)
        self.model.train()
        overlap, self.overlap_all_reduce = self.overlap_all_reduce, False      # nothing of a micro-batch is reduced early
        try:
            self.forward_backward(images, formulas)
        finally:
            self.overlap_all_reduce = overlap
        tail = self.flat_grads[self.n:self.n + 2].clone()                      # [loss sum, count] of this micro-batch
        if self._reducer._active():
            dist.all_reduce(tail, op=dist.ReduceOp.SUM, group=self.group)
        inv = 1.0 / (tail[1].clamp(min=1.0) * float(accumulation_steps))
        if self._accum is None:
            self._accum = torch.zeros(self.n, dtype=torch.float32, device=self.flat_grads.device)
        self._accum.addcmul_(self.flat_grads[:self.n], inv.expand(self.n))
        self._micro += 1
        out = dict(loss=tail[0] / tail[1].clamp(min=1.0), count=tail[1], **self._loss_parts())
        if update:
            world = dist.get_world_size(self.group) if self._reducer._active() else 1
            self.flat_grads[:self.n].copy_(self._accum)
            self.flat_grads[self.n] = out["loss"] / world                      # the slots the fused kernel divides by: the sum
            self.flat_grads[self.n + 1] = 1.0 / world                          # over ranks of the count slot is exactly 1
            self._accum.zero_()
            self._micro = 0
            self.apply()
            out.update(total_norm=self.stats[0], skipped=self.stats[3])
        return out

    def applied_steps(self) -> int:
        """Optimizer steps actually applied (host sync): step_count minus the skipped, non-finite ones.  Called at
        checkpoint / logging time; warns when every step since the last call was skipped (gradients that STAY
        non-finite are divergence, not a one-off timeout -- the silent no-op updates would otherwise go unnoticed)."""
        skipped = int(self._opt_ws[-256:-252].view(torch.int32).item())
        last_steps, last_skipped = getattr(self, "_last_counts", (0, 0))
        if self.step_count - last_steps >= 8 and skipped - last_skipped == self.step_count - last_steps:
            import warnings
            warnings.warn(f"img2latex_amd: all {self.step_count - last_steps} optimizer steps since the last check were "
                          "skipped (non-finite gradients): the run has diverged or the grouped kernels keep timing out")
        self._last_counts = (self.step_count, skipped)
        return self.step_count - skipped

    # ------------------------------------------------------------------ checkpoint compatibility
    def optimizer_state_dict(self) -> Dict:
        """torch.optim.Adam.state_dict() layout (what trainer.py:213 stores): resuming in the reference works."""
        state, params = {}, []
        applied = self.applied_steps()
        for i, (name, p) in enumerate(self.model.named_parameters()):
            if name not in self.offsets:                      # frozen: torch's Adam holds no state for it either
                params.append(i)
                continue
            o = self.offsets[name]
            state[i] = {"step": torch.tensor(float(applied)),
                        "exp_avg": self.exp_avg[o:o + p.numel()].view_as(p).detach().cpu().clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + p.numel()].view_as(p).detach().cpu().clone()}
            params.append(i)
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": False, "params": params}
        # like torch's Adam under GradScaler, the state stays empty until an update has actually been APPLIED
        return {"state": state if applied > 0 else {}, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: Dict) -> None:
        """Inverse of the above (trainer.py:255, resume from a reference checkpoint)."""
        names = [n for n, _ in self.model.named_parameters()]
        for i, st in sd.get("state", {}).items():
            name = names[int(i)]
            if name not in self.offsets:
                continue
            p = dict(self.model.named_parameters())[name]
            o = self.offsets[name]
            self.exp_avg[o:o + p.numel()].view_as(p).copy_(st["exp_avg"])
            self.exp_avg_sq[o:o + p.numel()].view_as(p).copy_(st["exp_avg_sq"])
            self.step_count = int(float(st["step"]))
            self._opt_ws.zero_()
        g = sd.get("param_groups", [{}])[0]
        self.lr = g.get("lr", self.lr)
        self.weight_decay = g.get("weight_decay", self.weight_decay)
