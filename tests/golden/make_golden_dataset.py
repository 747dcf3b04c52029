#!/usr/bin/env python3
"""The data-set fixture: writes the small data directory tests/golden/dataset_tiny/ and runs the REAL reference over it
(img2latex/data/dataset.py ``create_data_loaders`` and the evaluation loop of img2latex/cli.py:449-495 with the
reference's ``Predictor``; imported unmodified from /root/reference behind the same inert torchvision shim as
make_golden_tokenize.py), storing what it yields in tests/golden/dataset.npz.

``import torchvision.transforms`` is made to FAIL before ``create_data_loaders`` runs: the reference then takes its
``except ImportError`` branch (no train transform), where the shim's empty module would raise AttributeError instead.

dataset_tiny/
    img/p00.png .. p11.png          strokes on white, ``L`` and ``RGB`` mixed, different sizes: wider and narrower than
                                    the 32 x 128 target after the resize, one already 32 rows high
    im2latex_formulas.norm.lst      an empty line, a whitespace-only line, non-ASCII tokens, doubled separators, tabs, a
                                    CR LF line end, unknown tokens, one formula of more than 150 tokens; the other
                                    tokens come from the vocabulary of the checkpoint below
    im2latex_{train,validate,test}_filter.lst
                                    with a malformed line (1 and 3 fields), an out-of-range and a negative index, a
                                    non-integer index, a name with no file (the zero image) and a repeated page

dataset.npz
    config_c{1,3}                   the config handed to create_data_loaders (JSON): batch size 4, img_size (32, 128)
    c{1,3}_{train0,train1,val,test}_{k}_{names,idx,ids,images}
                                    batch k of two training epochs under torch.manual_seed(SEED) and of val / test
                                    (num_workers = 0): image names (JSON), formula indices, the padded id matrix, images
    c{1,3}_samples_{train,val,test} the samples each split file yields (JSON: [[name, idx], ...])
    eval_*                          cli.py:449-495 over ``test`` with the reference's Predictor on EVAL_CHECKPOINT:
                                    predictions and references (JSON), bleu, levenshtein, count

The evaluation checkpoint is tests/golden/predict_64x800.pt, not ref_checkpoint.pt: the reference's ``predict_batch``
resizes every tensor that is not 64 x 800 to that size (predictor.py:409-414,482-491), which the 16 x 32 encoder of
ref_checkpoint.pt cannot take -- the reference's own loop raises on it (main() shows it).  The generator asserts that on
every decode step of every evaluated row the top-2 logit margin is at least 1e-3 (the project's logits parity is 1e-4).

The archive is written with fixed zip timestamps and the PNGs carry no time stamp, so a re-run gives the same bytes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dataset.py
"""
import io
import json
import os
import shutil
import sys
import types
import zipfile

sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True
_tv = types.ModuleType("torchvision")
_tv.__path__ = []
for _sub in ("models", "transforms", "transforms.functional"):
    _m = types.ModuleType("torchvision." + _sub)
    _m.__path__ = []
    sys.modules["torchvision." + _sub] = _m
    setattr(sys.modules["torchvision." + _sub.rsplit(".", 1)[0]] if "." in _sub else _tv, _sub.rsplit(".", 1)[-1], _m)
sys.modules["torchvision"] = _tv

import logging  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

logging.disable(logging.CRITICAL)
from img2latex.data.dataset import create_data_loaders  # noqa: E402  (the reference)
from img2latex.training.metrics import calculate_metrics  # noqa: E402
from img2latex.training.predictor import Predictor  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "dataset_tiny")
EVAL_CHECKPOINT = os.path.join(HERE, "predict_64x800.pt")
SEED = 1234
BATCH = 4
IMG_SIZE = (32, 128)
MIN_MARGIN = 1e-3


class Lcg:
    """A generator that is the same everywhere."""

    def __init__(self, seed):
        self.s = seed

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (self.s >> 33) % n


def make_page(seed, h, w, rgb):
    """Dark strokes on white, no noise (the pages and what the loaders make of them compress well)."""
    rng = Lcg(seed)
    a = np.full((h, w, 3 if rgb else 1), 255, np.uint8)
    for _ in range(8 + rng.below(8)):
        y, x = rng.below(max(h - 6, 1)), rng.below(max(w - 12, 1))
        dh, dw = 1 + rng.below(5), 2 + rng.below(11)
        a[y:y + dh, x:x + dw] = [20 * rng.below(7) for _ in range(a.shape[2])]
    return a if rgb else a[..., 0]


# (seed, h, w, rgb): 32 * w / h against 128 -> crop, pad, exact; p04 needs no vertical pass, p07 is taller than wide
PAGES = [(1, 20, 200, False), (2, 40, 60, False), (3, 24, 96, True), (4, 32, 100, False), (5, 32, 128, True),
         (6, 50, 330, False), (7, 17, 93, True), (8, 64, 40, False), (9, 28, 111, False), (10, 33, 131, True),
         (11, 16, 64, False), (12, 45, 290, True)]


def make_formulas(vocab_tokens):
    rng = Lcg(99)
    pick = lambda k: [vocab_tokens[rng.below(len(vocab_tokens))] for _ in range(k)]
    lines = [" ".join(pick(5)), "", " ".join(pick(9)), "  ".join(pick(4)) + "  ", "\t".join(pick(6)),
             " ".join(pick(3) + ["α", "∑", "\U0001d53d"] + pick(2)), " ".join(pick(7)) + "\r",
             " ".join(pick(2) + ["notaword", "\\frac"] + pick(3)), " ".join(pick(155)), "   ", " ".join(pick(12)),
             " ".join(pick(3)) + "　" + " ".join(pick(2)), " ".join(pick(1)), " ".join(pick(20)),
             " ".join(pick(8) + ["<END>"] + pick(2)), " ".join(pick(40))]
    return ("\n".join(lines) + "\n").encode("utf-8")


SPLITS = {
    "train": ["p00.png 0", "p01.png 2", "only_one_field", "p02.png 3", "p03.png 99", "p04.png 4", "p05.png x7", "p06.png 5",
              "missing_a.png 6", "p07.png 7", "p00.png 8", "three fields 1", "p08.png 10", "p09.png -1", "p09.png 11", "",
              "p10.png 13"],
    "validate": ["p10.png 12", "p11.png 1", "p03.png 16", "p02.png 15", "p11.png 14", "p05.png 9"],
    "test": ["p00.png 0", "p06.png 4", "p11.png 2", "missing_b.png 10", "p03.png 5", "p08.png 13", "bad line here", "p05.png 7",
             "p06.png 11", "p09.png 1.5", "p01.png 3", "p10.png 15", "p07.png 12", "p04.png 9"],
}


def write_tiny(vocab_tokens):
    shutil.rmtree(TINY, ignore_errors=True)
    os.makedirs(os.path.join(TINY, "img"))
    for k, (seed, h, w, rgb) in enumerate(PAGES):
        Image.fromarray(make_page(seed, h, w, rgb), "RGB" if rgb else "L").save(os.path.join(TINY, "img", f"p{k:02d}.png"),
                                                                                 optimize=True)
    with open(os.path.join(TINY, "im2latex_formulas.norm.lst"), "wb") as f:
        f.write(make_formulas(vocab_tokens))
    for split, lines in SPLITS.items():
        with open(os.path.join(TINY, f"im2latex_{split}_filter.lst"), "wb") as f:
            f.write(("\n".join(lines) + "\n").encode("utf-8"))


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def loader_config(channels):
    enc = {"channels": channels, "img_height": IMG_SIZE[0], "img_width": IMG_SIZE[1]}
    model = {"name": "cnn_lstm", "encoder": {"cnn": enc}} if channels == 1 else {"name": "resnet_lstm", "encoder": {"resnet": enc}}
    return {"data": {"batch_size": BATCH, "num_workers": 0}, "model": model}


def record(out, key, loader):
    for k, batch in enumerate(loader):
        out[f"{key}_{k}_names"] = np.array(json.dumps(batch["image_paths"]))
        out[f"{key}_{k}_idx"] = np.array(batch["formula_idxs"], np.int64)
        out[f"{key}_{k}_ids"] = batch["formulas"].numpy().astype(np.int32)
        out[f"{key}_{k}_images"] = batch["images"].numpy().astype(np.float32)
        out[f"{key}_{k}_raw"] = np.array(json.dumps(batch["raw_formulas"]))


def evaluation(out, tokenizer_check):
    """cli.py:402-495 with the reference's objects: the loaders from the checkpoint's config, predict_batch per batch,
    calculate_metrics over all pairs.  The decoder's step is wrapped only to look at the logits it returns."""
    # the checkpoint the issue names cannot run the reference's loop: show it, then use the 64 x 800 one
    small = Predictor.from_checkpoint(os.path.join(HERE, "ref_checkpoint.pt"), device=torch.device("cpu"))
    try:
        small.predict_batch(images=torch.zeros((1, 1, 16, 32)) - 0.5, max_length=4, batch_size=1)
        raise AssertionError("ref_checkpoint.pt runs the reference's predict_batch after all: use it")
    except RuntimeError as exc:
        print("ref_checkpoint.pt in predict_batch:", str(exc).splitlines()[0])
    pred = Predictor.from_checkpoint(EVAL_CHECKPOINT, device=torch.device("cpu"))
    config = torch.load(EVAL_CHECKPOINT, map_location="cpu", weights_only=False).get("config", {})
    config.setdefault("data", {})
    config["data"].setdefault("data_dir", TINY)
    config["data"].setdefault("batch_size", 32)
    config["data"].setdefault("num_workers", 0)
    sys.modules["torchvision.transforms"] = None
    loader = create_data_loaders(config=config, tokenizer=pred.tokenizer, max_samples={"train": None, "val": None, "test": None})["test"]
    steps = []
    inner = pred.model.decoder.decode_step

    def watched(*a, **kw):
        output, hidden = inner(*a, **kw)
        steps.append(output.squeeze(1).detach().clone())
        return output, hidden

    pred.model.decoder.decode_step = watched
    all_predictions, all_targets, results, worst = [], [], [], float("inf")
    for batch in loader:
        del steps[:]
        latex = pred.predict_batch(images=batch["images"], beam_size=0, max_length=pred.tokenizer.max_sequence_length,
                                   batch_size=len(batch["images"]))
        logits = torch.stack(steps, dim=1)                                   # (B, steps, V)
        top = torch.topk(logits, 2, dim=-1).values
        margin = (top[..., 0] - top[..., 1])
        ended = (logits.argmax(-1) == pred.tokenizer.end_token_id).cumsum(1)
        live = (ended - (logits.argmax(-1) == pred.tokenizer.end_token_id).long()) == 0   # steps up to and including the first END
        worst = min(worst, float(margin[live].min()))
        for i, text in enumerate(latex):
            target_ids = [t for t in batch["formulas"][i].tolist() if t != pred.tokenizer.pad_token_id]
            all_predictions.append(pred.tokenizer.encode(text))
            all_targets.append(target_ids)
            results.append({"prediction": text, "reference": batch["raw_formulas"][i]})
    assert worst >= MIN_MARGIN, f"top-2 logit margin {worst:.3g} < {MIN_MARGIN}: choose other pages"
    metrics = calculate_metrics(all_predictions, all_targets)
    out["eval_results"] = np.array(json.dumps(results))
    out["eval_bleu"] = np.array(metrics["bleu"], np.float64)
    out["eval_levenshtein"] = np.array(metrics["levenshtein"], np.float64)
    out["eval_count"] = np.array(metrics["batch_size"], np.int64)
    out["eval_min_margin"] = np.array(worst, np.float64)
    print("evaluate:", metrics, "min margin", worst, "distinct predictions", len({r["prediction"] for r in results}))
    return pred.tokenizer


def main():
    tok_cfg = torch.load(EVAL_CHECKPOINT, map_location="cpu", weights_only=False)["tokenizer_config"]
    special = set(tok_cfg["special_tokens"].values())
    vocab_tokens = [t for t, _ in sorted(tok_cfg["token_to_id"].items(), key=lambda kv: kv[1]) if t not in special]
    write_tiny(vocab_tokens)
    out = {}
    tokenizer = evaluation(out, None)
    sys.modules["torchvision.transforms"] = None                             # create_data_loaders: `except ImportError`
    for channels in (1, 3):
        config = loader_config(channels)
        out[f"config_c{channels}"] = np.array(json.dumps(config))
        config["data"]["data_dir"] = TINY
        torch.manual_seed(SEED)
        loaders = create_data_loaders(config=config, tokenizer=tokenizer, max_samples=None)
        for split in ("train", "val", "test"):
            ds = loaders[split].dataset
            out[f"c{channels}_samples_{split}"] = np.array(json.dumps([[s["image_filename"], s["formula_idx"]] for s in ds.samples]))
        record(out, f"c{channels}_train0", loaders["train"])
        record(out, f"c{channels}_train1", loaders["train"])
        record(out, f"c{channels}_val", loaders["val"])
        record(out, f"c{channels}_test", loaders["test"])
    path = os.path.join(HERE, "dataset.npz")
    write_npz(path, out)
    pngs = sum(os.path.getsize(os.path.join(TINY, "img", f)) for f in os.listdir(os.path.join(TINY, "img")))
    print("dataset.npz", os.path.getsize(path), "bytes;", len(PAGES), "pages,", pngs, "bytes of PNG;", len(out), "arrays")


if __name__ == "__main__":
    main()
