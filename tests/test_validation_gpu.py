"""The validation pass of Trainer.train on the device (trainer.py:461-766): the fused teacher-forced evaluation kernel
against a float64 NumPy restatement, Validator against the reference's own Trainer.validate (tests/golden/validate.npz),
a resnet_lstm smoke, and the train command's epoch-end policy (validate, plateau LR, best checkpoint, early stop)."""
import json
import os
import random

import numpy as np
import pytest
import torch
import yaml

import img2latex_oracle as O
import metrics_oracle as MO
from conftest import record
from helpers import DEV, GOLDEN, PAD, model_for
from img2latex_amd import _lib, synth
from img2latex_amd.model import Seq2SeqModel
from img2latex_amd.training import Validator, teacher_forced_eval, validate

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernel
def _np_eval(x, tgt, pad, eps):
    """float64 restatement: CE term of CrossEntropyLoss(ignore_index=pad, label_smoothing=eps) per row (out-of-range
    targets clamped), first-index arg max, masked accuracy and the first-pad lengths of trainer.py:547-559."""
    B, T, V = x.shape
    x64 = x.astype(np.float64)
    m = x64.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(x64 - m).sum(-1, keepdims=True)))[..., 0]
    tg = np.clip(tgt, 0, V - 1)
    nll = lse - np.take_along_axis(x64, tg[..., None], -1)[..., 0]
    row = (1 - eps) * nll + eps * (lse - x64.mean(-1))
    keep = tgt != pad
    arg = np.argmax(x, -1).astype(np.int32)
    first = lambda a: np.array([list(r).index(pad) if pad in r else T for r in a.tolist()], dtype=np.int32)
    correct, total = MO.masked_accuracy(x, tgt, pad)
    return dict(loss=float((row * keep).sum()), count=int(keep.sum()), ids=arg, pred_len=first(arg),
                target_len=first(tgt), correct=correct, total=total)


def _case(V, seed, B=3, T=7, pad=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    x[1, 2] *= 80.0 / max(1e-6, float(np.abs(x[1, 2]).max()))       # magnitude 80: no overflow in exp
    x[1, 3] = -x[1, 2]
    if V > 1:
        x[2, 1, V // 2] = x[2, 1, V - 1] = x[2, 1].max() + 1.0       # an exact tie in the max: the first index wins
        x[0, 0, pad] = x[0, 0].max() + 2.0                           # arg max == pad: ends the prediction early
    tgt = rng.integers(1, max(V, 2), size=(B, T)).astype(np.int32)   # V == 1: target 1 is out of range (clamped)
    tgt[0, :] = pad                                                  # a sequence of pad rows only
    tgt[2, 4:] = pad                                                 # ragged; sequence 1 has no pad
    if V > 3:
        tgt[1, 5] = V + 3                                            # out of range, non-pad: clamped for the loss
    return x, tgt


def _run(x, tgt, pad, eps, want_ids=True, want_len=True, misalign=False):
    B, T, V = x.shape
    flat = torch.from_numpy(x.reshape(-1)).to(DEV)
    if misalign:                                                     # logits off 16-byte alignment: the scalar path
        buf = torch.empty(flat.numel() + 1, dtype=torch.float32, device=DEV)
        buf[1:].copy_(flat)
        flat = buf[1:]
    t = torch.from_numpy(tgt).to(DEV)
    L = _lib.lib()
    nbytes = L.i2l_teacher_forced_eval_workspace_bytes(B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ids = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    pl = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    tl = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    lc = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    ct = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    rc = L.i2l_teacher_forced_eval(flat.data_ptr(), t.data_ptr(), B, T, V, pad, eps, ws.data_ptr(), nbytes,
                                   ids.data_ptr() if want_ids else None, pl.data_ptr() if want_len else None,
                                   tl.data_ptr() if want_len else None, lc.data_ptr(), ct.data_ptr(), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(ids=ids.cpu().numpy(), pred_len=pl.cpu().numpy(), target_len=tl.cpu().numpy(), lc=lc.cpu().numpy(),
                ct=ct.cpu().numpy())


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [1, 37, 63, 64, 65, 512, 1000, 2048, 5000])
def test_teacher_forced_eval_kernel_vs_float64(V, eps):
    x, tgt = _case(V, seed=V * 10 + int(eps * 10))
    want = _np_eval(x, tgt, 0, eps)
    paths = [False, True] if V % 4 == 0 else [False]
    for misalign in paths:
        got = _run(x, tgt, 0, eps, misalign=misalign)
        err = abs(float(got["lc"][0]) - want["loss"]) / max(1.0, abs(want["loss"]))
        record("teacher_forced_eval loss sum [rel]", err)
        assert err <= 2e-6, (V, eps, misalign, float(got["lc"][0]), want["loss"])
        assert float(got["lc"][1]) == want["count"]
        assert np.array_equal(got["ids"], want["ids"]), (V, misalign)
        assert np.array_equal(got["pred_len"], want["pred_len"]) and np.array_equal(got["target_len"], want["target_len"])
        assert got["ct"].tolist() == [want["correct"], want["total"]]
    # the loss mean is the oracle's CrossEntropyLoss(ignore_index, label_smoothing) where every target is in range
    if V > 3:
        ok = tgt.copy()
        ok[1, 5] = 1
        mean = O.ce_label_smooth(torch.from_numpy(x).double(), torch.from_numpy(ok).long(), 0, eps).item()
        got = _run(x, ok, 0, eps)
        assert abs(float(got["lc"][0] / got["lc"][1]) - mean) <= 2e-6 * max(1.0, abs(mean))
    # NULL id / length pointers: same sums; two identical calls: bit-identical outputs
    a, b = _run(x, tgt, 0, eps), _run(x, tgt, 0, eps, want_ids=False, want_len=False)
    assert a["lc"].tobytes() == b["lc"].tobytes() and a["ct"].tolist() == b["ct"].tolist()
    assert (b["ids"] == -7).all() and (b["pred_len"] == -7).all()
    c = _run(x, tgt, 0, eps)
    assert all(a[k].tobytes() == c[k].tobytes() for k in a)


def test_teacher_forced_eval_rejects_bad_arguments():
    L = _lib.lib()
    B, T, V = 2, 3, 8
    x = torch.zeros((B, T, V), dtype=torch.float32, device=DEV)
    t = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    nbytes = L.i2l_teacher_forced_eval_workspace_bytes(B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lc = torch.zeros(2, dtype=torch.float32, device=DEV)
    ct = torch.zeros(2, dtype=torch.int64, device=DEV)

    def call(b=B, v=V, eps=0.1, nb=nbytes, lcp=lc.data_ptr()):
        return L.i2l_teacher_forced_eval(x.data_ptr(), t.data_ptr(), b, T, v, 0, eps, ws.data_ptr(), nb, None, None,
                                         None, lcp, ct.data_ptr(), _lib.stream_ptr())
    assert call() == 0
    assert call(b=-1) < 0 and call(v=0) < 0 and call(nb=nbytes - 1) < 0 and call(lcp=None) < 0
    assert call(eps=1.0) < 0 and call(eps=-0.1) < 0 and call(eps=float("nan")) < 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ Validator vs reference
def _fixture(name):
    d = np.load(os.path.join(GOLDEN, "validate.npz"))
    gen = json.loads(str(d[f"{name}_gen_json"]))
    cfg = json.loads(str(d[f"{name}_cfg_json"]))
    n = sum(gen["sizes"])
    imgs = torch.from_numpy(synth.make_images(n, cfg, seed=gen["seed"]))
    forms = torch.from_numpy(d[f"{name}_formulas"].astype(np.int64))
    loader, o = [], 0
    for b in gen["sizes"]:
        loader.append({"images": imgs[o:o + b], "formulas": forms[o:o + b]})
        o += b
    return d, gen, loader


@pytest.mark.parametrize("name", ["tiny_l1", "odd_dims"])
def test_validator_matches_reference_validate(name):
    d, gen, loader = _fixture(name)
    model, _ = model_for(name)
    ids = []
    with torch.no_grad():
        for b in loader:
            logits = model(b["images"].to(DEV), b["formulas"].to(DEV))
            got_ids, _, _ = teacher_forced_eval(logits, b["formulas"][:, 1:].to(DEV).to(torch.int32).contiguous(), PAD)
            ids.append(got_ids.cpu().reshape(-1))
    assert np.array_equal(torch.cat(ids).numpy(), d[f"{name}_ids"].astype(np.int32)), "arg max ids differ"
    random.seed(gen["rng_seed"])
    v = Validator(model, PAD, len(loader), gen["bleu_batches"], 0.1, rng=random)
    for b in loader:
        v.add(b["images"], b["formulas"])
    res = v.finish(gen["epoch"], gen["step"])
    assert v.sampled == d[f"{name}_sampled"].tolist()
    want = {k[len(name) + 5:]: d[k].item() for k in d.files if k.startswith(f"{name}_res_")}
    assert set(want) <= set(res), set(want) - set(res)
    for k in ("val_acc", "accuracy", "num_tokens", "batch_size", "val_samples", "epoch", "step"):
        assert res[k] == want[k], (k, res[k], want[k])
    assert res["bleu"] == want["bleu"] and res["levenshtein"] == want["levenshtein"]   # bit-identical
    assert res["bleu"] > 0.0
    err = abs(res["val_loss"] - want["val_loss"]) / abs(want["val_loss"])
    record(f"validate val_loss [rel] {name}", err)
    assert err <= 1e-5, (res["val_loss"], want["val_loss"])
    # the convenience wrapper: same pass, same RNG stream
    random.seed(gen["rng_seed"])
    again = validate(model, loader, PAD, gen["bleu_batches"], 0.1, epoch=gen["epoch"], step=gen["step"])
    assert again == res


def test_validator_resnet_lstm_smoke():
    """resnet_lstm (grayscale batches converted to RGB, data/utils.py:131-133): its bf16 trunk is not id-exact by
    design, so finite numbers, ids in range and the reference's keys."""
    cfg = synth.model_config(vocab_size=60, embedding_dim=64, hidden_dim=64, dropout=0.0)
    enc_p = dict(img_height=32, img_width=96, channels=3, model_name="resnet18", embedding_dim=64, freeze_backbone=True)
    m = Seq2SeqModel("resnet_lstm", 60, enc_p, synth.decoder_params(cfg))
    shapes = [(k, tuple(v.shape)) for k, v in m.encoder.state_dict().items()]
    full = {"encoder." + k: torch.from_numpy(v) for k, v in synth.make_resnet_state_dict(shapes, seed=3).items()}
    full.update({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=4).items() if k.startswith("decoder.")})
    m.load_state_dict(full)
    m = m.to(DEV)
    loader = [{"images": torch.from_numpy(synth.uniform(20 + i, "images", (4, 1, 32, 96), -1.0, 1.0)),
               "formulas": torch.from_numpy(synth.make_formulas(4, 14, 60, seed=30 + i, min_len=5))} for i in range(3)]
    res = validate(m, loader, PAD, bleu_batches=2, rng=random.Random(1), epoch=0, step=5)
    for k in ("val_loss", "val_acc", "val_samples", "epoch", "step", "accuracy", "num_tokens", "bleu", "levenshtein",
              "batch_size"):
        assert k in res, k
    assert np.isfinite(res["val_loss"]) and res["val_samples"] == 12 and 0.0 <= res["val_acc"] <= 1.0
    with torch.no_grad():
        imgs = loader[0]["images"].to(DEV).expand(-1, 3, -1, -1).contiguous()
        logits = m(imgs, loader[0]["formulas"].to(DEV))
    ids, lens, _ = teacher_forced_eval(logits, loader[0]["formulas"][:, 1:].to(DEV).to(torch.int32).contiguous(), PAD)
    ids = ids.cpu()
    assert int(ids.min()) >= 0 and int(ids.max()) < 60 and int(lens.max()) <= 13


# ------------------------------------------------------------------------------------------------ the train command
def _cli_config(tmp_path, lr=0.0):
    config = {
        "model": {"name": "cnn_lstm", "embedding_dim": 32,
                  "encoder": {"cnn": {"img_height": 16, "img_width": 32, "channels": 1, "conv_filters": [4, 8, 16],
                                      "kernel_size": 3, "pool_size": 2, "padding": "same"}},
                  "decoder": {"hidden_dim": 64, "lstm_layers": 1, "dropout": 0.1, "attention": False,
                              "max_seq_length": 20}},
        "data": {"batch_size": 4, "max_seq_length": 20},
        "training": {"device": "cuda", "epochs": 4, "early_stopping_patience": 1, "learning_rate": lr,
                     "weight_decay": 0.0, "accumulation_steps": 1},
        "evaluation": {"bleu_batches": 1, "save_basic_metrics": True},
    }
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(config))
    return str(path)


def test_cli_train_validates_and_stops_early(tmp_path, capsys):
    """lr 0: no epoch after the first improves on it, so epoch 1 is best (best_checkpoint_* + best_checkpoint.pt),
    epoch 2 writes a plain checkpoint and patience 1 stops the run (trainer.py:727-766)."""
    from img2latex_amd import cli
    from img2latex_amd.training import Predictor
    out_dir = tmp_path / "outputs"
    out = cli.train(_cli_config(tmp_path), "val_test", None, None, "cuda", 7, synthetic_steps=3, synthetic_vocab=50,
                    output_dir=str(out_dir), synthetic_val_steps=2)
    ck_dir = out_dir / "val_test" / "checkpoints"
    assert sorted(os.listdir(ck_dir)) == ["best_checkpoint.pt", "best_checkpoint_epoch_1_step_3.pt",
                                          "checkpoint_epoch_2_step_6.pt"]
    assert out["steps"] == 6 and out["global_step"] == 6 and out["checkpoint"] == str(ck_dir / "checkpoint_epoch_2_step_6.pt")
    best = torch.load(ck_dir / "best_checkpoint.pt", map_location="cpu", weights_only=False)
    last = torch.load(ck_dir / "checkpoint_epoch_2_step_6.pt", map_location="cpu", weights_only=False)
    for ck, ep in ((best, 1), (last, 2)):
        assert ck["epoch"] == ep and ck["metrics"]["epoch"] == ep - 1
        assert {"val_loss", "val_acc", "val_samples", "step", "accuracy", "num_tokens", "bleu", "levenshtein",
                "batch_size"} <= set(ck["metrics"])
        assert ck["metrics"]["val_samples"] == 8
        assert ck["optimizer_state_dict"]["param_groups"][0]["lr"] == 0.0   # no plateau yet: 0 epochs past patience 2
    assert last["metrics"]["val_loss"] == best["metrics"]["val_loss"] == out["best_val_loss"]
    assert out["val_metrics"] == last["metrics"]
    metrics = json.loads((out_dir / "val_test" / "metrics" / "metrics.json").read_text())
    assert sorted(metrics) == ["1", "2"] and metrics["2"]["val_loss"] == last["metrics"]["val_loss"]
    assert "val_loss" in capsys.readouterr().out
    p = Predictor.from_checkpoint(str(ck_dir / "best_checkpoint.pt"), device=torch.device("cuda"))
    assert p.model is not None


def test_cli_train_plateau_lowers_saved_lr(tmp_path):
    """lr > 0 with a patience that does not stop: the plateau rule (factor 0.5, patience 2) acts on TrainStep.lr and
    the checkpoint's optimizer state carries the rate it left, replayed here from the saved val_loss sequence."""
    import types
    from img2latex_amd import cli
    from img2latex_amd.training import PlateauSchedule
    cfg_path = _cli_config(tmp_path, lr=1e-3)
    config = yaml.safe_load(open(cfg_path))
    config["training"].update(epochs=4, early_stopping_patience=100)
    config["evaluation"]["save_basic_metrics"] = True
    open(cfg_path, "w").write(yaml.safe_dump(config))
    out_dir = tmp_path / "outputs"
    cli.train(cfg_path, "plateau", None, None, "cuda", 7, synthetic_steps=2, synthetic_vocab=50, output_dir=str(out_dir),
              synthetic_val_steps=1)
    metrics = json.loads((out_dir / "plateau" / "metrics" / "metrics.json").read_text())
    target = types.SimpleNamespace(lr=1e-3)
    sched = PlateauSchedule(target)
    ck_dir = out_dir / "plateau" / "checkpoints"
    for e in range(1, 5):
        sched.step(metrics[str(e)]["val_loss"])
        names = [f for f in os.listdir(ck_dir) if f.endswith(f"_epoch_{e}_step_{2 * e}.pt")]
        assert len(names) == 1
        ck = torch.load(ck_dir / names[0], map_location="cpu", weights_only=False)
        assert ck["optimizer_state_dict"]["param_groups"][0]["lr"] == target.lr
