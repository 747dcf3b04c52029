"""The three entry points of the reference's CLI that sit on the hot path, with its argument and option names
(img2latex/cli.py:104-120 ``train``, :253-269 ``predict``, :315-332 ``evaluate``), and ``vocab``, which this package adds:

    python -m img2latex_amd predict CHECKPOINT IMAGE [--beam-size N] [--max-length N] [--temperature T]
                                                     [--nbest N --length-penalty A]  (this package: N-best beam search)
                                                     [--well-formed]  (this package: greedy, sampling or --nbest)
                                                     [--complete-arguments]  (this package: greedy or sampling)
                                                     [--top-k K] [--top-p P] [--device cuda]
                                                     [--samples N --rank {consensus,logprob} --seed S]  (this package:
                                                      N draws ranked on the device, with --top-k / --top-p)
                                                     [--ensemble CHECKPOINT ... --ensemble-weights a,b,...
                                                      --ensemble-rule {logprob,prob}]  (this package: greedy or sampling)
    python -m img2latex_amd train [--config-path F] [--experiment-name S] [--checkpoint-path F] [--data-dir D]
                                  [--device cuda] [--seed N] [--synthetic-steps N [--synthetic-val-steps N]]
                                  [--augment] [--data {auto,native,reference}] [--decode {host,device}]
                                  [--teacher CHECKPOINT ... --teacher-weights a,b,... --teacher-rule {logprob,prob}
                                   --distill-alpha A --distill-temperature T]  (this package: distillation)
                                  [--risk-samples N --risk-alpha A --risk-temperature T --risk-top-k K --risk-top-p P]
                                                                   (this package: minimum-risk fine-tuning)
    python -m img2latex_amd evaluate CHECKPOINT DATA_DIR [--split test] [--batch-size 32] [--num-samples N] [--errors]
                                                         [--beam-size 0] [--device cuda] [--output-dir outputs]
                                                         [--decode {host,device}]
                                                         [--ensemble CHECKPOINT ... --ensemble-weights a,b,...
                                                          --ensemble-rule {logprob,prob}]  (this package)
    python -m img2latex_amd vocab FORMULAS_FILE OUT [--max-sequence-length N] [--device cuda]

``predict`` is the reference's chain end to end on the device: Predictor.from_checkpoint (predictor.py:61-137) ->
Predictor.predict(image_path) (:139-203) -> load_image (data/utils.py:18-90) -> encoder -> greedy search -> string.

``train`` builds the model from the YAML exactly as cli.py:195-217 does, resumes model + Adam state from a reference
checkpoint (trainer.py:235-269) and drives ``TrainStep`` (the optimisation step of trainer.py:303-343 on the HIP
kernels) over the batches of the data loaders.  ``--data native``: the vocabulary is fitted on the device
(``TokenTable.fit_on_formulas_file``) and the batches come from this package's device-resident data set
(``data.create_data_loaders``, data/dataset.py: pages decoded and uploaded once, formulas tokenized once, the
reference's samples, order and batches).  ``--data reference``: the reference's own ``create_data_loaders`` with its
``LaTeXTokenizer``, which needs the ``img2latex`` package beside this one.  ``--data auto`` (the default) takes the
reference's when that package is importable, as before, and the native ones otherwise.  ``--synthetic-steps N``: the
deterministic generator the benchmarks use instead of a data directory.  After every epoch it validates as Trainer.train does
(trainer.py:667-766): ``training.validate`` on the validation batches, ReduceLROnPlateau on val_loss, a best checkpoint
(``best_checkpoint_epoch_E_step_S.pt`` + ``best_checkpoint.pt``) or a plain one, early stopping after
``training.early_stopping_patience`` epochs without improvement, and ``metrics/metrics.json`` when
``evaluation.save_basic_metrics`` is set.  A synthetic run validates only with ``--synthetic-val-steps N`` (N synthetic
batches from a seed disjoint from the training batches; it then runs ``training.epochs`` epochs over the same training
batches); without it, it makes one pass and writes one plain checkpoint, as before.  ``--augment`` warps every training
batch on the device as the reference's training split is warped (data/dataset.py:486-492: rotation within 5 degrees,
then a shift within 2 %, NEAREST, white fill; ``data.Augment.tensor``), never a validation batch.  One difference: the
batches arrive preprocessed, so the 2 % is a fraction of the preprocessed tensor's size, not of the raw page's as in the
reference; ``data.preprocess_batch(pages, augment=...)`` is the reference-order path for raw pages, and the one the
native loaders take: with ``--data native`` the warp is applied to the raw page, inside the loader.  Experiment
registry, logging setup and rich console output are the reference's host-side orchestration and are not rebuilt here.

``evaluate`` is cli.py:315-518: Predictor.from_checkpoint, the native loaders built from the checkpoint's config and
tokenizer, ``Predictor.evaluate_stream`` over the split (greedy; a beam size above 0 is clamped with a warning, as the
reference clamps it), the three result lines, and ``<output-dir>/<experiment>/predictions/predictions.json`` with the
experiment name taken from the checkpoint's path.  BLEU and Levenshtein are means over all pairs of the split.

``vocab`` fits the vocabulary of a formulas file on the device (LaTeXTokenizer.fit_on_formulas_file, tokenizer.py:
119-141, through ``TokenTable.fit_on_formulas_file``) and writes it in LaTeXTokenizer.save's layout (:257-275), which both
``TokenTable.load`` and the reference's ``LaTeXTokenizer.load`` read.

The device is a ROCm GPU; ``--device cpu`` is refused (there is no CPU fallback in this package).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional

import torch


def _device(name: Optional[str]) -> torch.device:
    """cli.py:266-268 / mps_utils.set_device, minus the silent fall-back to the CPU."""
    if name not in (None, "cuda") and not str(name).startswith("cuda:"):
        raise SystemExit(f"img2latex_amd: --device {name}: this package runs on a ROCm GPU only (no CPU / MPS path)")
    if not torch.cuda.is_available():
        raise SystemExit("img2latex_amd: no ROCm device is visible")
    return torch.device(name or "cuda")


def _decode_flags(decode_kernel: str) -> int:
    """--decode-kernel: "auto" = the library's own choice (grouped kernels where the dimensions have them, else a row per
    workgroup); "batched" = the step-batched matrix-core decode (_lib.FLAG_DECODE_BATCHED), built for decoders the grouped
    kernels do not take, such as the shipped two-layer, 512-wide one.  It covers the greedy loop and, with --top-k /
    --top-p, the sampling loop (i2l_sample_decode_batched)."""
    from . import _lib
    if decode_kernel not in ("auto", "batched"):
        raise SystemExit(f"img2latex_amd: --decode-kernel {decode_kernel}: expected auto or batched")
    return _lib.FLAG_DECODE_BATCHED if decode_kernel == "batched" else 0


def _train_flags(train_kernel: str) -> int:
    """--train-kernel: "auto" = the library's own choice (grouped recurrences at one layer of 256 units, else a row per
    workgroup); "batched" = the step-batched matrix-core recurrences (_lib.FLAG_TRAIN_BATCHED), built for decoders the
    grouped kernels do not take, such as the shipped two-layer, 512-wide one, and the only ones above 1024 units."""
    from . import _lib
    if train_kernel not in ("auto", "batched"):
        raise SystemExit(f"img2latex_amd: --train-kernel {train_kernel}: expected auto or batched")
    return _lib.FLAG_TRAIN_BATCHED if train_kernel == "batched" else 0


def _well_formed(well_formed):
    """False / True (the bracket constraint) / "arguments" (the argument rules on top) or a table, as Predictor takes it."""
    return well_formed if isinstance(well_formed, str) or hasattr(well_formed, "vocab") else bool(well_formed)


def _predictor(checkpoint_path: str, device, decode_kernel: str, well_formed, ensemble=(), ensemble_weights=None,
               ensemble_rule: str = "logprob"):
    """Predictor.from_checkpoint, or with ``ensemble`` (further checkpoints) Predictor.from_checkpoints over
    ``[checkpoint_path, *ensemble]`` -- ``ensemble_weights`` one per checkpoint, the positional one first."""
    from .training import Predictor
    if not ensemble:
        return Predictor.from_checkpoint(checkpoint_path=checkpoint_path, device=device,
                                         decode_flags=_decode_flags(decode_kernel), well_formed=_well_formed(well_formed))
    return Predictor.from_checkpoints([checkpoint_path, *ensemble], weights=ensemble_weights, combine=ensemble_rule,
                                      device=device, decode_flags=_decode_flags(decode_kernel),
                                      well_formed=_well_formed(well_formed))


def _ensemble_weights(text: Optional[str], n: int, option: str = "--ensemble-weights", order: str = " (the positional one first)"):
    """--ensemble-weights "a,b,..." (or ``option``) -> n floats (None when absent); ValueError with the reason otherwise."""
    if text is None:
        return None
    try:
        weights = [float(t) for t in text.split(",")]
    except ValueError:
        raise ValueError(f"{option} {text}: expected comma-separated numbers")
    if len(weights) != n:
        raise ValueError(f"{option} has {len(weights)} values for {n} checkpoints{order}")
    if not all(w > 0 and w != float("inf") for w in weights):
        raise ValueError(f"{option} {text}: every weight must be finite and above 0")
    return weights


def _check_teacher_tokens(paths, tables, tokenizer) -> None:
    """SystemExit naming the first differing token when a teacher checkpoint's ``token_to_id`` is not the student's: the
    distillation loss compares the two distributions column by column, so column v must be the same token in both."""
    mine = dict(tokenizer.token_to_id)
    for path, table in zip(paths, tables):
        theirs = dict(table.token_to_id)
        if theirs == mine:
            continue
        for tok, i in sorted(mine.items(), key=lambda kv: kv[1]):
            if theirs.get(tok) != i:
                raise SystemExit(f"img2latex_amd train: --teacher {path}: its token_to_id differs from the student's "
                                 f"tokenizer at token {tok!r} (student id {i}, teacher id {theirs.get(tok)})")
        tok, i = min(((t, i) for t, i in theirs.items() if t not in mine), key=lambda kv: kv[1])
        raise SystemExit(f"img2latex_amd train: --teacher {path}: its token_to_id differs from the student's tokenizer "
                         f"at token {tok!r} (teacher id {i}, not in the student's vocabulary)")


def predict(checkpoint_path: str, image_path: str, beam_size: int = 0, max_length: int = 141, temperature: float = 1.0,
            top_k: int = 0, top_p: float = 0.0, device: Optional[str] = None, decode_kernel: str = "auto",
            well_formed: bool = False, ensemble=(), ensemble_weights=None, ensemble_rule: str = "logprob") -> str:
    """cli.py:253-308: returns the LaTeX string the command prints.  ``decode_kernel``: see ``_decode_flags``.
    ``well_formed``: the bracket-constrained decode (training/constraint.py): braces, \\left / \\right and \\begin / \\end
    nest and the formula ends within ``max_length`` tokens; ``"arguments"``: every command also gets the arguments it
    demands (``\\frac`` its two groups, ``^`` its operand).  ``ensemble``: further checkpoints that choose every token
    together with the first one (``Predictor.from_checkpoints``)."""
    predictor = _predictor(checkpoint_path, _device(device), decode_kernel, well_formed, ensemble, ensemble_weights,
                           ensemble_rule)
    return predictor.predict(image=image_path, beam_size=beam_size, max_length=max_length, temperature=temperature,
                             top_k=top_k, top_p=top_p)


def predict_nbest(checkpoint_path: str, image_path: str, beam_size: int, nbest: int, max_length: int = 141,
                  length_penalty: float = 0.0, device: Optional[str] = None, well_formed: bool = False):
    """(this package) the ``nbest`` best beam-search hypotheses of the image as (latex, score, key), in rank order.
    ``well_formed``: the bracket-constrained search, every hypothesis nesting its groups and ending on END."""
    from .training import Predictor
    predictor = Predictor.from_checkpoint(checkpoint_path=checkpoint_path, device=_device(device))
    return predictor.predict_nbest(image=image_path, beam_size=beam_size, nbest=nbest, max_length=max_length,
                                   length_penalty=length_penalty, well_formed=_well_formed(well_formed))


def predict_samples(checkpoint_path: str, image_path: str, samples: int, rank: str = "consensus", max_length: int = 141,
                    temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0,
                    length_penalty: float = 0.0, device: Optional[str] = None, well_formed=False):
    """(this package) ``samples`` top-k / top-p draws of the image as (latex, score, key), best first: the consensus
    (minimum-Bayes-risk) order, or with ``rank="logprob"`` the length-normalised log-probability.  ``well_formed``: as in
    ``predict``; "arguments" gives argument-complete candidates."""
    from .training import Predictor
    predictor = Predictor.from_checkpoint(checkpoint_path=checkpoint_path, device=_device(device))
    return predictor.predict_samples(image=image_path, samples=samples, rank=rank, max_length=max_length,
                                     temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                     well_formed=_well_formed(well_formed), length_penalty=length_penalty)


def vocab(formulas_file: str, out_path: str, max_sequence_length: int = 150, device: Optional[str] = None):
    """Fit on ``formulas_file``, save to ``out_path``; returns the fitted TokenTable."""
    from .training import TokenTable
    table = TokenTable(max_sequence_length=max_sequence_length)
    fitted = table.fit_on_formulas_file(formulas_file, device=_device(device))
    table.save(out_path)
    print(f"vocabulary of {table.vocab_size} tokens from {fitted.rows} formulas ({fitted.total_tokens} tokens, longest "
          f"{fitted.longest_row}) -> {out_path}")
    return table


def load_config(config_path: str) -> Dict:
    """cli.py:83-101."""
    import yaml
    if not os.path.exists(config_path):
        raise FileNotFoundError(f"Config file not found: {config_path}")
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def build_model(config: Dict, vocab_size: int):
    """cli.py:195-217: config["model"] -> Seq2SeqModel."""
    from .model import Seq2SeqModel
    model_cfg = config["model"]
    enc = dict(model_cfg["encoder"]["cnn" if model_cfg["name"] == "cnn_lstm" else "resnet"])
    enc["embedding_dim"] = model_cfg["embedding_dim"]
    return Seq2SeqModel(model_type=model_cfg["name"], vocab_size=vocab_size, encoder_params=enc,
                        decoder_params=model_cfg["decoder"])


def _synthetic_batches(config: Dict, steps: int, vocab_size: int, seed: int):
    from . import synth
    model_cfg, batch = config["model"], int(config.get("data", {}).get("batch_size", 64))
    enc = model_cfg["encoder"]["cnn" if model_cfg["name"] == "cnn_lstm" else "resnet"]
    length = int(config.get("data", {}).get("max_seq_length", 150))
    for s in range(steps):
        images = synth.uniform(seed + s, "images", (batch, enc["channels"], enc["img_height"], enc["img_width"]), -1.0, 1.0)
        yield {"images": torch.from_numpy(images),
               "formulas": torch.from_numpy(synth.make_formulas(batch, length, vocab_size, seed=seed + s))}


RISK_KEYS = ("samples", "alpha", "temperature", "top_k", "top_p")


def _risk_objective(options: Optional[Dict], tcfg: Dict, tokenizer, has_teacher: bool):
    """The RiskObjective of a ``train`` run, or None: ``options`` (the command line's, any of RISK_KEYS) over the config's
    ``training.risk_<key>``.  It is on when ``samples`` is set in either place.  SystemExit for the other options without
    it, for a teacher beside it and for values RiskObjective refuses."""
    merged = {k: tcfg["risk_" + k] for k in RISK_KEYS if tcfg.get("risk_" + k) is not None}
    merged.update({k: v for k, v in (options or {}).items() if v is not None})
    unknown = sorted(set(merged) - set(RISK_KEYS))
    if unknown:
        raise SystemExit(f"img2latex_amd train: unknown risk option(s) {unknown}; expected {list(RISK_KEYS)}")
    if not merged:
        return None
    if "samples" not in merged:
        raise SystemExit(f"img2latex_amd train: risk option(s) {sorted(merged)} need --risk-samples (training.risk_samples)")
    if has_teacher:
        raise SystemExit("img2latex_amd train: --risk-samples with --teacher: the step takes a teacher or the risk "
                         "objective, not both")
    from .training import RiskObjective
    try:
        merged["samples"] = int(merged["samples"])
        if "top_k" in merged:
            merged["top_k"] = int(merged["top_k"])
        return RiskObjective(int(tokenizer.start_token_id), int(tokenizer.end_token_id), **merged)
    except (TypeError, ValueError) as exc:
        raise SystemExit(f"img2latex_amd train: --risk-samples: {exc}")


def train(config_path: str = "img2latex/configs/config.yaml", experiment_name: str = "img2latex_v1",
          checkpoint_path: Optional[str] = None, data_dir: Optional[str] = None, device: Optional[str] = None,
          seed: int = 42, synthetic_steps: int = 0, synthetic_vocab: int = 512, output_dir: str = "outputs",
          synthetic_val_steps: int = 0, augment: bool = False, data: str = "auto", decode: Optional[str] = None,
          train_kernel: str = "auto", teacher=(), teacher_weights=None, teacher_rule: str = "logprob",
          distill_alpha: float = 0.5, distill_temperature: float = 2.0, risk: Optional[Dict] = None) -> Dict:
    """cli.py:104-250 reduced to the hot path: model from the config, optional resume, TrainStep over the batches, a
    checkpoint in the reference's layout (trainer.py:209-224) per epoch, and -- with validation batches -- the epoch-end
    validation / LR schedule / best checkpoint / early stop of trainer.py:713-766.  Returns {"loss", "steps",
    "global_step", "checkpoint"}, plus {"best_val_loss", "val_metrics"} when validation ran.  ``augment``: warp each
    training batch with ``data.Augment(seed=seed).tensor`` (keyed by epoch and the sample's position in the epoch); the
    native loaders warp the raw pages with the same keys instead.  ``data``: "auto", "native" or "reference" (see the
    module docstring).  ``decode``: where the native loaders decode the page files, "host" (PIL) or "device"
    (i2l_png_decode); None leaves it to the config key ``data.decode`` (default "host").  ``train_kernel``: see
    ``_train_flags`` (training and the epoch-end validation follow it).  ``teacher``: checkpoint paths of one teacher or
    of an ensemble (``teacher_weights`` one per path, ``teacher_rule`` "logprob" / "prob"); the student then trains on
    ``distill_alpha`` x the cross entropy + (1 - ``distill_alpha``) x the divergence from the teacher's token distribution
    at ``distill_temperature`` (training/distill.py).  Every teacher checkpoint's ``token_to_id`` must be the student's
    tokenizer's (SystemExit naming the first differing token).  Validation is untouched: ``val_loss`` stays the hard loss.
    ``risk``: the options of minimum-risk fine-tuning (training/risk.py) given on the command line, a dict with any of
    ``samples``, ``alpha``, ``temperature``, ``top_k``, ``top_p``; the config's ``training.risk_samples`` ... ``risk_top_p``
    stand behind them.  The objective is on when ``samples`` is set in either place; it does not combine with a teacher."""
    import random
    from . import data as D
    from .training import EarlyStopping, PlateauSchedule, TokenTable, TrainStep, save_checkpoint, validate
    random.seed(seed)                                                       # mps_utils.set_seed
    torch.manual_seed(seed)
    config = load_config(config_path)
    if data_dir:
        config.setdefault("data", {})["data_dir"] = data_dir
    config.setdefault("training", {})["experiment_name"] = experiment_name
    dev = _device(device or config["training"].get("device"))
    tcfg = config["training"]
    resume = torch.load(checkpoint_path, map_location="cpu", weights_only=False) if checkpoint_path else None
    native = False                                                          # the native loaders warp the raw pages themselves
    if synthetic_steps > 0:
        if resume is not None:
            tk = resume["tokenizer_config"]
            tokenizer = TokenTable(tk.get("token_to_id"), tk.get("special_tokens"), tk.get("max_sequence_length", 141))
        else:
            vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
            vocab.update({f"t{i}": i for i in range(4, synthetic_vocab)})
            tokenizer = TokenTable(vocab, max_sequence_length=int(config.get("data", {}).get("max_seq_length", 150)))
        max_epochs, loaders = None, None                                    # one pass over the synthetic batches ...
        if synthetic_val_steps > 0:                                         # ... unless there is something to validate on
            max_epochs = int(tcfg.get("epochs", 50))
    else:
        if data not in ("auto", "native", "reference"):
            raise SystemExit(f"img2latex_amd train: --data {data}: expected auto, native or reference")
        create_data_loaders = None
        if data != "native":
            try:
                from img2latex.data.dataset import create_data_loaders      # the reference's own dataset + tokenizer
                from img2latex.data.tokenizer import LaTeXTokenizer
            except ImportError as exc:
                if data == "reference":
                    raise SystemExit("img2latex_amd train --data reference: the reference's datasets and tokenizer "
                                     "(img2latex.data.dataset / tokenizer) are not importable; install that package "
                                     f"beside this one, or use --data native.  ({exc})")
        formulas_path = os.path.join(config["data"]["data_dir"], config["data"].get("formulas_file", "im2latex_formulas.norm.lst"))
        if create_data_loaders is not None:
            tokenizer = LaTeXTokenizer(max_sequence_length=config["data"]["max_seq_length"])
            tokenizer.fit_on_formulas_file(formulas_path)
            loaders = create_data_loaders(config=config, tokenizer=tokenizer, max_samples=None)
        else:
            native = True
            tokenizer = TokenTable(max_sequence_length=int(config["data"].get("max_seq_length", 150)))
            tokenizer.fit_on_formulas_file(formulas_path, device=dev)
            loaders = D.create_data_loaders(config, tokenizer, device=dev, augment=D.Augment(seed=seed) if augment else None,
                                            decode=decode)
            if not loaders:
                raise SystemExit(f"img2latex_amd train: no samples under {config['data']['data_dir']}")
        max_epochs = int(tcfg.get("epochs", 50))                            # trainer.py:118
    teacher = list(teacher or ())
    distill = None
    if teacher:
        from .training import Teacher
        try:
            distill, tables = Teacher.from_checkpoints(teacher, weights=teacher_weights, combine=teacher_rule, device=dev)
        except ValueError as exc:
            raise SystemExit(f"img2latex_amd train: --teacher: {exc}")
        _check_teacher_tokens(teacher, tables, tokenizer)
    objective = _risk_objective(risk, tcfg, tokenizer, bool(teacher))
    model = build_model(config, tokenizer.vocab_size)
    if resume is not None:
        model.load_state_dict(resume["model_state_dict"])                   # trainer.py:253
    model = model.to(dev)
    model.decoder.kernel_flags |= _train_flags(train_kernel)
    ts = TrainStep(model, lr=float(tcfg.get("learning_rate", 1e-3)), weight_decay=float(tcfg.get("weight_decay", 1e-4)),
                   clip_grad_norm=float(tcfg.get("clip_grad_norm", 5.0)), pad_token_id=tokenizer.pad_token_id,
                   label_smoothing=0.1, seed=seed,                          # trainer.py:91-93,111-115
                   **(dict(teacher=distill, distill_alpha=distill_alpha, distill_temperature=distill_temperature)
                      if distill is not None else {}),
                   **(dict(risk=objective) if objective is not None else {}))
    if resume is not None and resume.get("optimizer_state_dict"):
        ts.load_optimizer_state_dict(resume["optimizer_state_dict"])        # trainer.py:255
    # trainer.py:257-258,697: a checkpoint's "epoch" is the number of COMPLETED epochs and "step" the global step; a resumed
    # run continues both and stops at the configured total (it used to restart the step count and always run
    # `epochs` more epochs)
    start_epoch = int(resume.get("epoch", 0)) if resume is not None else 0
    step0 = step = int(resume.get("step", 0)) if resume is not None else 0
    if max_epochs is None:
        max_epochs = start_epoch + 1
    ck_dir = os.path.join(output_dir, experiment_name, "checkpoints")
    os.makedirs(ck_dir, exist_ok=True)
    last, path = None, None
    is_resnet = config["model"]["name"] == "resnet_lstm"
    if loaders is not None:
        val_batches = loaders["val"]
    elif synthetic_val_steps > 0:                                           # seeds after the training batches' ones
        val_batches = list(_synthetic_batches(config, synthetic_val_steps, tokenizer.vocab_size, seed + synthetic_steps))
    else:
        val_batches = None
    ecfg = config.get("evaluation", {}) or {}
    scheduler = PlateauSchedule(ts, mode="min", factor=0.5, patience=2)    # trainer.py:94-98
    stopper = EarlyStopping.from_checkpoint(int(tcfg.get("early_stopping_patience", 10)), resume)   # :120-122,257-262
    val_metrics = None
    accum = max(1, int(tcfg.get("accumulation_steps", 1)))                  # trainer.py:86-88 (the shipped config: 4)
    warp = D.Augment(seed=seed) if augment and not native else None         # dataset.py:486-492, the defaults are its values
    for epoch in range(start_epoch + 1, max_epochs + 1):                    # `epoch` = trainer.py's current_epoch + 1
        batches = _synthetic_batches(config, synthetic_steps, tokenizer.vocab_size, seed) if loaders is None else loaders["train"]
        if native:
            batches.set_epoch(epoch - 1)                                    # the warp's key, as below
        it = iter(batches)
        batch, batch_idx, seen = next(it, None), 0, 0
        reward_sum, reward_batches = 0.0, 0
        while batch is not None:
            nxt = next(it, None)                                            # one batch of look-ahead: "is this the last one?" (:374)
            images = batch["images"].to(dev)                                # data/utils.py:113-135 prepare_batch
            if warp is not None:                                            # white after load_image's normalisation
                ids = range(seen, seen + images.shape[0])
                images = warp.tensor(images.float(), D.white_fill(images.shape[1], True), ids, epoch - 1)
            seen += images.shape[0]
            if is_resnet and images.shape[1] == 1:
                images = D.batch_convert_for_resnet(images)
            update = (batch_idx + 1) % accum == 0 or nxt is None
            last = ts.micro_step(images, batch["formulas"].to(dev), accum, update)
            if "reward" in last:                                            # summed on the device: no sync in the loop
                reward_sum, reward_batches = reward_sum + last["reward"], reward_batches + 1
            step += 1                                                      # the reference's global_step counts batches (:399)
            batch, batch_idx = nxt, batch_idx + 1
        loss = float(last["loss"]) if last is not None else float("nan")
        parts = ""
        if last is not None and "reward" in last:                          # risk objective: the epoch's mean reward
            parts = (f" (reward {reward_sum / max(1, reward_batches):.4f}, hard {float(last['hard_loss']):.4f}, "
                     f"risk {float(last['risk_loss']):.4f})")
        elif last is not None and "hard_loss" in last:                     # distillation: the last batch's two parts
            parts = f" (hard {float(last['hard_loss']):.4f}, soft {float(last['soft_loss']):.4f})"
        if val_batches is None:
            path = os.path.join(ck_dir, f"checkpoint_epoch_{epoch}_step_{step}.pt")
            save_checkpoint(path, model, tokenizer, config, epoch=epoch, step=step, metrics={"loss": loss},
                            optimizer_state_dict=ts.optimizer_state_dict())
            print(f"epoch {epoch}: {step} steps, loss {loss:.4f}{parts}, checkpoint {path}")
            continue
        # trainer.py:716-766: validate, step the LR schedule on val_loss, best or plain checkpoint, early stop
        val_metrics = validate(model, val_batches, tokenizer.pad_token_id, int(ecfg.get("bleu_batches", 10)),
                               label_smoothing=0.1, epoch=epoch - 1, step=step)
        scheduler.step(val_metrics.get("val_loss", float("inf")))
        is_best, stop = stopper.update(val_metrics)
        name = f"checkpoint_epoch_{epoch}_step_{step}.pt"
        path = os.path.join(ck_dir, "best_" + name if is_best else name)
        save_checkpoint(path, model, tokenizer, config, epoch=epoch, step=step, metrics=val_metrics,
                        optimizer_state_dict=ts.optimizer_state_dict())
        if is_best:
            save_checkpoint(os.path.join(ck_dir, "best_checkpoint.pt"), model, tokenizer, config, epoch=epoch, step=step,
                            metrics=val_metrics, optimizer_state_dict=ts.optimizer_state_dict())
        if ecfg.get("save_basic_metrics", False):                           # trainer.py:645-661
            _save_basic_metrics(os.path.join(output_dir, experiment_name, "metrics"), epoch, val_metrics)
        extra = "".join(f", {k} {val_metrics[k]:.4f}" for k in ("bleu", "levenshtein") if k in val_metrics)
        print(f"epoch {epoch}: {step} steps, loss {loss:.4f}{parts}, val_loss {val_metrics['val_loss']:.4f}, "
              f"val_acc {val_metrics['val_acc']:.4f}{extra}, lr {ts.lr:g}, checkpoint {path}")
        if stop:
            print(f"early stopping after {epoch} epochs ({stopper.patience_counter} epochs without improvement)")
            break
    out = {"loss": float(last["loss"]) if last is not None else None, "steps": step - step0, "global_step": step,
           "checkpoint": path}
    if last is not None and "reward" in last:
        out.update(reward=float(reward_sum) / max(1, reward_batches), hard_loss=float(last["hard_loss"]),
                   risk_loss=float(last["risk_loss"]))
    elif last is not None and "hard_loss" in last:
        out.update(hard_loss=float(last["hard_loss"]), soft_loss=float(last["soft_loss"]))
    if val_metrics is not None:
        out.update(best_val_loss=stopper.best_val_loss, val_metrics=val_metrics)
    return out


def evaluate(checkpoint_path: str, data_dir: str, split: str = "test", batch_size: int = 32,
             num_samples: Optional[int] = None, beam_size: int = 0, device: Optional[str] = None,
             output_dir: str = "outputs", decode: Optional[str] = None, decode_kernel: str = "auto",
             well_formed: bool = False, ensemble=(), ensemble_weights=None, ensemble_rule: str = "logprob",
             errors: bool = False, errors_top: int = 20) -> Dict:
    """cli.py:315-518 on the device: returns {"bleu", "levenshtein", "batch_size"} over the whole split -- the means over
    all pairs, as ``calculate_metrics`` on the reference's two lists computes them -- after printing the three result
    lines and writing ``predictions.json``.

    One thing the reference does on the way is kept because it decides the predictions: its loop hands the loader's
    image TENSORS to ``predict_batch``, whose ``_prepare_image`` (predictor.py:464-499) rescales every tensor with a value
    below 0 or above 1 once more, ``x / 255 * 2 - 1`` -- which is every normalised page, but not the zero image of an
    unreadable file.  ``_prepare_image``'s other step, the bilinear resize of a tensor that is not 64 x 800, is not
    repeated: the loaders are built at the model's own input size, and the reference's encoder cannot run any other.
    ``decode``: "host" or "device", where the page files are decoded (``data.PageStore``); None: the checkpoint's
    config key ``data.decode``, "host" when absent.  ``well_formed``: as in ``predict``.  ``ensemble``: as in ``predict``;
    the split is then walked with ``evaluate_batch``, one batch at a time (the look-ahead pipeline is single-model).
    ``errors``: also write ``error_analysis.json`` and ``error_analysis_report.md`` beside ``predictions.json``: the token
    confusion matrix of the split, accumulated on the device behind every batch's statistics (``metrics.ErrorAnalysis``;
    token-level, where the reference's offline analysis/errors.py is character-level); ``errors_top``: the length of
    its lists.  The returned dict then carries the report under "error_analysis"."""
    import json
    import warnings
    from pathlib import Path
    from . import data as D
    from .training import metrics as M
    dev = _device(device)
    experiment_name = Path(checkpoint_path).parent.parent.name              # cli.py:340-349: outputs/<experiment>/checkpoints/<file>
    config = torch.load(checkpoint_path, map_location="cpu", weights_only=False).get("config", {}) or {}
    predictor = _predictor(checkpoint_path, dev, decode_kernel, well_formed, ensemble, ensemble_weights, ensemble_rule)
    max_samples = {"train": None, "val": None, "test": None}
    if num_samples:
        max_samples[split] = num_samples
    cfg_data = config.setdefault("data", {})                                # cli.py:412-420
    cfg_data.setdefault("data_dir", data_dir)
    cfg_data.setdefault("batch_size", batch_size)
    cfg_data.setdefault("num_workers", 0)
    loaders = D.create_data_loaders(config, predictor.tokenizer, max_samples=max_samples, device=dev, decode=decode)
    if split not in loaders:
        raise SystemExit(f"Invalid split: {split}")
    loader = loaders[split]
    if beam_size > 0:                                                       # predictor.py:231-235
        warnings.warn("Beam search is unsupported; using greedy decoding (beam_size=0).")
    print(f"Evaluating on {split} split with {len(loader.dataset)} samples")
    is_resnet = predictor.model_type == "resnet_lstm"
    raw: List[str] = []

    def batches():
        for batch in loader:
            x = batch["images"]
            lo, hi = x.amin(dim=(1, 2, 3), keepdim=True), x.amax(dim=(1, 2, 3), keepdim=True)
            x = torch.where((lo < 0) | (hi > 1), x / 255.0 * 2.0 - 1.0, x)  # predictor.py:493-497, per image
            if is_resnet and x.shape[1] == 1:                               # :453-455
                x = D.batch_convert_for_resnet(x)
            raw.extend(batch["raw_formulas"])
            yield x, batch["formulas"]

    stats, predictions = [], []
    analysis = M.ErrorAnalysis(predictor.tokenizer.vocab_size, dev) if errors else None
    if ensemble:
        results = (predictor.evaluate_batch(x, formulas, predictor.tokenizer.max_sequence_length, return_strings=True,
                                            return_statistics=True, errors=analysis) for x, formulas in batches())
    else:
        results = predictor.evaluate_stream(batches(), max_length=predictor.tokenizer.max_sequence_length,
                                            return_strings=True, return_statistics=True, errors=analysis)
    for out in results:
        stats.append(out["statistics"])
        predictions.extend(out["pred_text"])
    if not stats:
        raise SystemExit(f"img2latex_amd evaluate: the {split} split is empty")
    metrics = M.metrics_from_packed(torch.cat(stats).contiguous())
    print("Evaluation Results:")
    print(f"BLEU-4 Score: {metrics['bleu']:.4f}")
    print(f"Levenshtein Similarity: {metrics['levenshtein']:.4f}")
    print(f"Number of Samples: {metrics['batch_size']}")
    if experiment_name:                                                     # cli.py:504-517
        predictions_dir = os.path.join(output_dir, experiment_name, "predictions")
        os.makedirs(predictions_dir, exist_ok=True)
        save_path = os.path.join(predictions_dir, "predictions.json")
        with open(save_path, "w") as f:
            json.dump([{"prediction": p, "reference": r} for p, r in zip(predictions, raw)], f, indent=2)
        print(f"Predictions saved to: {save_path}")
    if analysis is not None:
        report = analysis.report(predictor.tokenizer, top=errors_top, ranges=M.ErrorAnalysis.ranges_from_config(config))
        metrics = dict(metrics, error_analysis=report)
        if experiment_name:
            json_path = os.path.join(predictions_dir, "error_analysis.json")
            with open(json_path, "w") as f:
                json.dump(report, f, indent=2)
            with open(os.path.join(predictions_dir, "error_analysis_report.md"), "w") as f:
                f.write(M.report_markdown(report))
            print(f"Error analysis saved to: {json_path}")
    return metrics


def _save_basic_metrics(metrics_dir: str, epoch: int, val_metrics: Dict) -> None:
    """trainer.py:645-661: metrics.json keyed by the 1-based epoch, merged into what the file already holds."""
    import json
    os.makedirs(metrics_dir, exist_ok=True)
    metrics_path = os.path.join(metrics_dir, "metrics.json")
    try:
        with open(metrics_path, "r") as f:
            basic_metrics = json.load(f)
    except Exception:
        basic_metrics = {}
    basic_metrics[str(epoch)] = val_metrics
    with open(metrics_path, "w") as f:
        json.dump(basic_metrics, f, indent=2)


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="img2latex_amd", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("predict", help="Predict LaTeX for an image.")
    p.add_argument("checkpoint_path", help="Path to trained model checkpoint")
    p.add_argument("image_path", help="Path to image file")
    p.add_argument("--beam-size", type=int, default=0, help="Beam size for beam search (0 for greedy search)")
    p.add_argument("--max-length", type=int, default=141, help="Maximum length of the generated sequence")
    p.add_argument("--temperature", type=float, default=1.0, help="Temperature for sampling")
    p.add_argument("--top-k", type=int, default=0, help="Top-k sampling parameter")
    p.add_argument("--top-p", type=float, default=0.0, help="Top-p (nucleus) sampling parameter")
    p.add_argument("--device", default=None, help="Device to use for inference (cuda)")
    p.add_argument("--decode-kernel", choices=("auto", "batched"), default="auto",
                   help="(this package) decode kernel, greedy and --top-k / --top-p sampling: auto, or the step-batched matrix-core decode")
    p.add_argument("--well-formed", action="store_true",
                   help="(this package) bracket-constrained decode: { }, \\left \\right and \\begin \\end nest and the formula "
                        "ends within the maximum length (nesting only: no arity, no semantics); greedy, sampling, or beam "
                        "search with --nbest N (--nbest 1: the single best well-formed formula)")
    p.add_argument("--complete-arguments", action="store_true",
                   help="(this package) implies --well-formed, and every command gets the arguments it demands: \\frac its "
                        "two groups, ^ and _ an operand (greedy and sampling only: refused with --beam-size)")
    p.add_argument("--nbest", type=int, default=0,
                   help="(this package) with --beam-size K > 0: print the N best hypotheses, one key<TAB>latex line each, "
                        "in rank order (0: the single result as before)")
    p.add_argument("--length-penalty", type=float, default=0.0,
                   help="(this package) with --nbest: rank by score / length ** A (0: by the raw score)")
    p.add_argument("--samples", type=int, default=0,
                   help="(this package) with --top-k / --top-p: draw N (1..16) samples in one decode and print them best "
                        "first, one key<TAB>latex line each (0: the single result as before); combines with "
                        "--well-formed and --complete-arguments")
    p.add_argument("--rank", choices=("consensus", "logprob"), default="consensus",
                   help="(this package) with --samples: consensus = the sample closest to the others first (key: its "
                        "summed edit distance), logprob = by score / length ** --length-penalty")
    p.add_argument("--seed", type=int, default=0, help="(this package) with --samples: the seed of the draws")
    t = sub.add_parser("train", help="Train the image-to-LaTeX model.")
    t.add_argument("--config-path", default="img2latex/configs/config.yaml", help="Path to configuration file")
    t.add_argument("--experiment-name", default="img2latex_v1", help="Name of the experiment")
    t.add_argument("--checkpoint-path", default=None, help="Path to checkpoint to resume training from")
    t.add_argument("--data-dir", default=None, help="Path to data directory (overrides config)")
    t.add_argument("--device", default=None, help="Device to use for training (cuda)")
    t.add_argument("--seed", type=int, default=42, help="Random seed for reproducibility")
    t.add_argument("--synthetic-steps", type=int, default=0,
                   help="(this package) train N steps on synthetic batches instead of the reference's data loaders")
    t.add_argument("--synthetic-vocab", type=int, default=512, help="(this package) vocabulary size of the synthetic batches")
    t.add_argument("--output-dir", default="outputs", help="(this package) root of <experiment>/checkpoints")
    t.add_argument("--synthetic-val-steps", type=int, default=0,
                   help="(this package) with --synthetic-steps: validate every epoch on N synthetic batches and run "
                        "training.epochs epochs with LR scheduling and early stopping")
    t.add_argument("--augment", action="store_true",
                   help="(this package) warp each training batch on the device as the reference's training split is "
                        "(rotation within 5 degrees, shift within 2 %% of the batch's size, NEAREST, white fill)")
    t.add_argument("--data", choices=("auto", "native", "reference"), default="auto",
                   help="(this package) where the batches come from: this package's device-resident data set (native), the "
                        "reference's data loaders (reference), or the reference's when importable and else the native ones (auto)")
    t.add_argument("--decode", choices=("host", "device"), default=None,
                   help="(this package, --data native) decode the page files with PIL on the host or with the PNG kernel on "
                        "the device; default: the config key data.decode, else host")
    t.add_argument("--train-kernel", choices=("auto", "batched"), default="auto",
                   help="(this package) decoder recurrences of a training step: auto, or the step-batched matrix-core ones")
    t.add_argument("--teacher", action="append", default=[], metavar="CHECKPOINT",
                   help="(this package) distil: train against the token distribution of this checkpoint; repeat the "
                        "option for an ensemble of teachers (all of the student's vocabulary)")
    t.add_argument("--teacher-weights", default=None, metavar="A,B,...",
                   help="(this package) with --teacher: one weight per teacher checkpoint, in order (default: equal)")
    t.add_argument("--teacher-rule", choices=("logprob", "prob"), default=None,
                   help="(this package) with --teacher: how the teachers' distributions combine (default logprob)")
    t.add_argument("--distill-alpha", type=float, default=None, metavar="A",
                   help="(this package) with --teacher: weight of the data set's tokens in the loss, 0 .. 1 (default 0.5)")
    t.add_argument("--distill-temperature", type=float, default=None, metavar="T",
                   help="(this package) with --teacher: temperature of both distributions in the soft term (default 2.0)")
    t.add_argument("--risk-samples", type=int, default=None, metavar="N",
                   help="(this package) minimum-risk fine-tuning: draw N formulas per image from the model (2 .. 16) and "
                        "train on them, weighted by their edit-distance reward, beside the gold formula; also the config "
                        "key training.risk_samples.  Not with --teacher")
    t.add_argument("--risk-alpha", type=float, default=None, metavar="A",
                   help="(this package) with --risk-samples: weight of the gold formula's cross entropy, 0 .. 1 (default 0.5)")
    t.add_argument("--risk-temperature", type=float, default=None, metavar="T",
                   help="(this package) with --risk-samples: temperature of the draws (default 1.0)")
    t.add_argument("--risk-top-k", type=int, default=None, metavar="K",
                   help="(this package) with --risk-samples: draw from the K most likely tokens (default 0: no limit)")
    t.add_argument("--risk-top-p", type=float, default=None, metavar="P",
                   help="(this package) with --risk-samples: draw from the nucleus of mass P (default 0: no limit)")
    e = sub.add_parser("evaluate", help="Evaluate the model on a dataset.")
    e.add_argument("checkpoint_path", help="Path to trained model checkpoint")
    e.add_argument("data_dir", help="Path to data directory")
    e.add_argument("--split", default="test", help="Data split to evaluate on (train, val, test)")
    e.add_argument("--batch-size", type=int, default=32, help="Batch size for evaluation")
    e.add_argument("--num-samples", type=int, default=None, help="Number of samples to evaluate (None for all)")
    e.add_argument("--beam-size", type=int, default=0, help="Beam size for beam search (0 for greedy search)")
    e.add_argument("--device", default=None, help="Device to use for evaluation (cuda)")
    e.add_argument("--output-dir", default="outputs", help="(this package) root of <experiment>/predictions")
    e.add_argument("--decode-kernel", choices=("auto", "batched"), default="auto",
                   help="(this package) decode kernel, greedy and --top-k / --top-p sampling: auto, or the step-batched matrix-core decode")
    e.add_argument("--decode", choices=("host", "device"), default=None,
                   help="(this package) decode the page files with PIL on the host or with the PNG kernel on the device")
    e.add_argument("--well-formed", action="store_true",
                   help="(this package) bracket-constrained decode: { }, \\left \\right and \\begin \\end nest and the formula "
                        "ends within the maximum length (nesting only: no arity, no semantics)")
    e.add_argument("--complete-arguments", action="store_true",
                   help="(this package) implies --well-formed, and every command gets the arguments it demands: \\frac its "
                        "two groups, ^ and _ an operand")
    e.add_argument("--errors", action="store_true",
                   help="(this package) also write error_analysis.json and error_analysis_report.md beside predictions.json: "
                        "edit-distance buckets, operation totals, the top substituted / deleted / inserted tokens and per-token "
                        "recall and precision, from edit alignments computed on the device.  Distances and operations are "
                        "counted in TOKENS (the reference's offline error report counts characters)")
    e.add_argument("--errors-top", type=int, default=20, metavar="N",
                   help="(this package) with --errors: the length of the top lists (1 .. 1024, default 20)")
    for q in (p, e):
        q.add_argument("--ensemble", action="append", default=[], metavar="CHECKPOINT",
                       help="(this package) a further checkpoint of the same vocabulary; repeatable.  The checkpoints choose "
                            "every token together (greedy and sampling only: refused with --beam-size)")
        q.add_argument("--ensemble-weights", default=None, metavar="A,B,...",
                       help="(this package) one weight per checkpoint, the positional one first (default: equal)")
        q.add_argument("--ensemble-rule", choices=("logprob", "prob"), default="logprob",
                       help="(this package) logprob: weighted geometric mean of the members' distributions; prob: arithmetic mean")
    v = sub.add_parser("vocab", help="(this package) Fit the vocabulary of a formulas file on the device and save it.")
    v.add_argument("formulas_file", help="Path to the formulas file, one formula per line")
    v.add_argument("out_path", help="Path to save the vocabulary to (LaTeXTokenizer.save's layout)")
    v.add_argument("--max-sequence-length", type=int, default=150, help="Maximum sequence length stored with the vocabulary")
    v.add_argument("--device", default=None, help="Device to fit on (cuda)")
    args = ap.parse_args(argv)
    if args.command == "predict" and args.nbest < 0:
        ap.error("--nbest must be >= 0")
    ensemble_weights = None
    if args.command in ("predict", "evaluate"):
        if args.ensemble and args.beam_size > 0:
            ap.error("--ensemble with --beam-size: the ensemble decode is greedy or sampling (beam search is single-model)")
        if not args.ensemble and args.ensemble_weights is not None:
            ap.error("--ensemble-weights needs --ensemble")
        try:
            ensemble_weights = _ensemble_weights(args.ensemble_weights, 1 + len(args.ensemble))
        except ValueError as exc:
            ap.error(str(exc))
    distill_kw = {}
    if args.command == "train":
        if not args.teacher:
            for name in ("teacher_weights", "teacher_rule", "distill_alpha", "distill_temperature"):
                if getattr(args, name) is not None:
                    ap.error(f"--{name.replace('_', '-')} needs --teacher")
        else:
            from .training.distill import check_distill_arguments
            try:
                weights = _ensemble_weights(args.teacher_weights, len(args.teacher), "--teacher-weights", "")
                alpha, temperature = check_distill_arguments(0.5 if args.distill_alpha is None else args.distill_alpha,
                                                             2.0 if args.distill_temperature is None else args.distill_temperature)
            except ValueError as exc:
                ap.error(str(exc))
            distill_kw = dict(teacher=args.teacher, teacher_weights=weights, teacher_rule=args.teacher_rule or "logprob",
                              distill_alpha=alpha, distill_temperature=temperature)
        risk = {k: getattr(args, "risk_" + k) for k in RISK_KEYS if getattr(args, "risk_" + k) is not None}
        if risk:
            # what needs neither the config nor the tokenizer is answered here, with the parser's exit; train() checks
            # again once the config's keys are merged in
            if args.teacher:
                ap.error("--risk-samples with --teacher: the step takes a teacher or the risk objective, not both")
            if "samples" in risk:
                from .training.risk import RiskObjective
                try:
                    RiskObjective(1, 2, **risk)
                except (TypeError, ValueError) as exc:
                    ap.error(str(exc))
            distill_kw = dict(distill_kw, risk=risk)
    if args.command == "evaluate" and not 1 <= args.errors_top <= 1024:
        ap.error("--errors-top must be 1 .. 1024")
    if args.command == "predict" and args.complete_arguments and args.beam_size > 0:
        ap.error("--complete-arguments with --beam-size: the argument rules exist for the greedy and sampling decode only "
                 "(--well-formed --nbest N is the constrained beam search)")
    if args.command == "predict" and args.samples != 0:
        if args.beam_size > 0:
            ap.error("--samples with --beam-size: the samples are draws of the sampling decode, not beams")
        if args.nbest > 0:
            ap.error("--samples with --nbest: --nbest lists beam-search hypotheses (it needs --beam-size)")
        if args.ensemble:
            ap.error("--samples with --ensemble: the consensus decode is single-model")
        if not 1 <= args.samples <= 16:
            ap.error("--samples must be 1 .. 16")
        if args.top_k <= 0 and args.top_p <= 0.0:
            ap.error("--samples needs --top-k or --top-p: the samples are top-k / top-p draws")
    if args.command in ("predict", "evaluate") and args.complete_arguments:
        args.well_formed = "arguments"
    if args.command == "predict" and args.well_formed and args.beam_size > 0 and args.nbest == 0:
        ap.error("--well-formed with --beam-size needs --nbest: add --nbest 1 for the single best well-formed formula "
                 "(plain --beam-size runs the grouped beam kernels, which carry no constraint)")
    if args.command == "predict" and args.nbest > 0:
        if args.beam_size <= 0:
            ap.error("--nbest needs --beam-size above 0")
        for latex, _, key in predict_nbest(args.checkpoint_path, args.image_path, args.beam_size, args.nbest,
                                           args.max_length, args.length_penalty, args.device,
                                           well_formed=args.well_formed):
            print(f"{key!r}\t{latex}")
        return 0
    if args.command == "predict" and args.samples > 0:
        for latex, _, key in predict_samples(args.checkpoint_path, args.image_path, args.samples, args.rank, args.max_length,
                                             args.temperature, args.top_k, args.top_p, args.seed, args.length_penalty,
                                             args.device, well_formed=args.well_formed):
            print(f"{key!r}\t{latex}")
        return 0
    if args.command == "predict":
        latex = predict(args.checkpoint_path, args.image_path, args.beam_size, args.max_length, args.temperature,
                        args.top_k, args.top_p, args.device, args.decode_kernel, args.well_formed, args.ensemble,
                        ensemble_weights, args.ensemble_rule)
        print("Generated LaTeX:")
        print(latex)
        return 0
    if args.command == "vocab":
        vocab(args.formulas_file, args.out_path, args.max_sequence_length, args.device)
        return 0
    if args.command == "evaluate":
        evaluate(args.checkpoint_path, args.data_dir, args.split, args.batch_size, args.num_samples, args.beam_size,
                 args.device, args.output_dir, args.decode, args.decode_kernel, args.well_formed, args.ensemble,
                 ensemble_weights, args.ensemble_rule, **(dict(errors=True, errors_top=args.errors_top) if args.errors else {}))
        return 0
    try:
        train(args.config_path, args.experiment_name, args.checkpoint_path, args.data_dir, args.device, args.seed,
              args.synthetic_steps, args.synthetic_vocab, args.output_dir, args.synthetic_val_steps, args.augment,
              args.data, args.decode, args.train_kernel, **distill_kw)
    except SystemExit:
        raise
    except Exception as exc:                                                # cli.py:247-250: failure -> exit code 1
        print(f"Training failed: {exc}", file=sys.stderr)
        return 1
    return 0
