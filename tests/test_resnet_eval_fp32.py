"""ResNetEncoder in EVAL mode at fp32 grade (``eval_precision = "fp32"``; encoder.py:185-249 under model.eval(), the
arithmetic of the reference's fp32 branch, trainer.py:334-343): every conv + running-statistics BatchNorm (+ shortcut)
(+ ReLU) unit is one i2l_conv_bn_act_f32_fwd launch (csrc/resnet_train.hip, epilogue in csrc/gemm.hip).

Parity stays UNPINNED against the reference itself (torchvision absent, remote weights: SURVEY 8c).  The yardstick is
float64: a float64 torch-CPU evaluation of one unit, and oracle/resnet_oracle.py evaluated in float64 for the whole
trunk.  Every bound is a multiple of the distance that the SAME computation in torch fp32 on the CPU keeps to float64,
measured in the test itself -- never a number taken from the kernels."""
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import img2latex_oracle as O
import resnet_oracle as RO
from conftest import record
from helpers import PAD
from img2latex_amd import _lib, synth
from img2latex_amd.model import ResNetEncoder, Seq2SeqModel

DEV = "cuda"
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODELS = [("resnet18", (32, 64)), ("resnet50", (64, 96)), ("resnet34", (32, 64)), ("resnet101", (32, 96)),
          ("resnet152", (32, 64))]                      # the shapes of test_resnet_encoder_vs_oracle


def _rel(a, ref):
    return float((a.double() - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ (1) one unit
# (B, H, W, Cin, Cout, k, stride, pad, NCHW input, residual, relu); M = B * Ho * Wo rows, K = Cin * k * k.
# "split": the split-bf16 GEMM's plan (gemm.hip plan_bf16x3) cuts K into slabs; the stem's K = 147 is no multiple of 8
# and runs on the fp32 MFMA GEMM either way.  Under I2L_FLAG_EXACT_FP32 (gemm.hip plan) the 1x1/2, both 3x3 and the
# 2048-column case are split and the others are not.
UNITS = {
    "stem 7x7/2 NCHW": (3, 32, 64, 3, 64, 7, 2, 3, True, False, True),                # M 1536, K 147
    "1x1/1 64->256 +res": (3, 8, 15, 64, 256, 1, 1, 0, False, True, True),            # M 360 (not a multiple of 128), no split
    "1x1/1 64->64": (3, 16, 32, 64, 64, 1, 1, 0, False, False, True),                 # M 1536, no split
    "1x1/2 projection 256->512": (3, 8, 16, 256, 512, 1, 2, 0, False, False, False),  # M 96, no split
    "3x3/1 128->128 +res": (3, 8, 16, 128, 128, 3, 1, 1, False, True, True),          # M 384, K 1152: split
    "3x3/1 64->64 +res, no relu": (3, 8, 15, 64, 64, 3, 1, 1, False, True, False),    # M 360, K 576
    "3x3/2 128->256": (3, 8, 16, 128, 256, 3, 2, 1, False, False, True),              # M 96, K 1152: split
    "1x1/1 512->2048 +res": (3, 2, 4, 512, 2048, 1, 1, 0, False, True, True),         # M 24, K 512: split
}


def _unit_inputs(name, B, H, W, Cin, Cout, k):
    seed = 100 + sorted(UNITS).index(name)
    x = torch.from_numpy(synth.uniform(seed, "x", (B, Cin, H, W), -1.0, 1.0))
    fan_out = Cout * k * k
    w = torch.from_numpy(synth.normal_like(seed, "w", (Cout, Cin, k, k)) * np.float32(np.sqrt(2.0 / fan_out)))
    bn = {n: torch.from_numpy(synth.uniform(seed, n, (Cout,), lo, hi)) for n, lo, hi in
          (("gamma", 0.5, 1.5), ("beta", -0.2, 0.2), ("mean", -0.2, 0.2), ("var", 0.5, 1.5))}
    return x, w, bn


def _fold(bn, eps=1e-5):
    L = _lib.lib()
    C = bn["gamma"].numel()
    d = {k: v.to(DEV) for k, v in bn.items()}
    out = torch.empty((2, C), dtype=torch.float32, device=DEV)
    rc = L.i2l_bn_eval_fold_f32(d["gamma"].data_ptr(), d["beta"].data_ptr(), d["mean"].data_ptr(), d["var"].data_ptr(), eps,
                                out[0].data_ptr(), out[1].data_ptr(), C, _lib.stream_ptr())
    assert rc == 0, rc
    return out


def _run_unit(x_dev, kind, w_dev, fold, res_dev, shape, relu, flags, nbytes=None, **null):
    B, H, W, Cin, Cout, k, s, pd = shape
    L = _lib.lib()
    Ho, Wo = (H + 2 * pd - k) // s + 1, (W + 2 * pd - k) // s + 1
    need = L.i2l_conv_f32_workspace_bytes(kind, B, H, W, Cin, Cout, k, k, s, pd, 0)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float32, device=DEV)
    ptr = dict(x=x_dev.data_ptr(), w=w_dev.data_ptr(), scale=fold[0].data_ptr(), shift=fold[1].data_ptr(), y=y.data_ptr())
    ptr.update(null)
    rc = L.i2l_conv_bn_act_f32_fwd(ptr["x"], kind, ptr["w"], ptr["scale"], ptr["shift"], _lib.ptr(res_dev), ptr["y"], B, H, W,
                                   Cin, Cout, k, k, s, pd, 1 if relu else 0, ws.data_ptr(), need if nbytes is None else nbytes,
                                   flags, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["split_bf16", "exact_fp32"])
@pytest.mark.parametrize("name", sorted(UNITS))
def test_conv_bn_act_f32_unit_vs_float64(name, exact):
    """y = act(scale * conv(x, w) + shift + residual) against float64 on the CPU, with the SAME fp32 scale / shift (the
    fold is checked on its own, against its float64 formula rounded once).
    Bound: 8 x the distance torch's fp32 evaluation of the same unit on the CPU keeps to float64, both relative to the
    float64 maximum (a different summation order, dropped split terms <= 2^-24 |a||b| per product, three roundings in
    the epilogue).  Two runs are bit-identical; the result does not depend on whether K was split (the same epilogue
    runs on the complete sum)."""
    B, H, W, Cin, Cout, k, s, pd, nchw, with_res, relu = UNITS[name]
    x, w, bn = _unit_inputs(name, B, H, W, Cin, Cout, k)
    fold = _fold(bn)
    # the fold: double arithmetic, one rounding each; the shift against the ROUNDED scale
    eps = np.float64(np.float32(1e-5))
    g, b, mu, var = (bn[n].numpy().astype(np.float64) for n in ("gamma", "beta", "mean", "var"))
    sc = (g / np.sqrt(var + eps)).astype(np.float32)
    sh = (b - mu * sc.astype(np.float64)).astype(np.float32)
    got_fold = fold.cpu().numpy()
    assert np.all(np.abs(got_fold[0] - sc) <= np.spacing(np.abs(sc))) and np.all(np.abs(got_fold[1] - sh) <= np.spacing(np.abs(sh)))
    scale, shift = fold[0].cpu(), fold[1].cpu()

    z64 = F.conv2d(x.double(), w.double(), stride=s, padding=pd)
    pre64 = z64 * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    res = None
    if with_res:                                     # the activations' magnitude
        res = torch.from_numpy(synth.uniform(7, "res" + name, tuple(pre64.shape), -1.0, 1.0)) * float(pre64.abs().max())
    y64 = pre64 if res is None else pre64 + res.double()
    y64 = torch.relu(y64) if relu else y64
    z32 = F.conv2d(x, w, stride=s, padding=pd)
    y32 = z32 * scale[None, :, None, None] + shift[None, :, None, None]
    y32 = y32 if res is None else y32 + res
    y32 = torch.relu(y32) if relu else y32
    e_torch = _rel(y32, y64)

    x_dev = (x if nchw else x.permute(0, 2, 3, 1)).contiguous().to(DEV)
    res_dev = None if res is None else res.permute(0, 2, 3, 1).contiguous().to(DEV)
    flags = _lib.FLAG_EXACT_FP32 if exact else 0
    shape = (B, H, W, Cin, Cout, k, s, pd)
    rc, y = _run_unit(x_dev, 2 if nchw else 1, w.to(DEV), fold, res_dev, shape, relu, flags)
    assert rc == 0, rc
    e_hip = _rel(y.cpu().permute(0, 3, 1, 2), y64)
    tag = f"conv_bn_act_f32 {name} [{'exact' if exact else 'split'}]"
    record(tag + " HIP vs float64 [rel to max]", e_hip)
    record(tag + " torch fp32 CPU vs float64 [rel to max]", e_torch)
    print(f"{tag}: HIP {e_hip:.3e}  torch fp32 {e_torch:.3e}")
    assert e_hip <= 8.0 * e_torch, (name, exact, e_hip, e_torch)
    rc, y2 = _run_unit(x_dev, 2 if nchw else 1, w.to(DEV), fold, res_dev, shape, relu, flags)
    assert rc == 0 and torch.equal(y, y2)


@pytest.mark.gpu
def test_conv_bn_act_f32_refusals():
    """Every refusal comes before any launch (y keeps its NaN fill) and carries its code."""
    B, H, W, Cin, Cout, k, s, pd = shape = (2, 8, 8, 16, 64, 3, 1, 1)
    x = torch.zeros((B, H, W, Cin), dtype=torch.float32, device=DEV)
    w = torch.zeros((Cout, Cin, k, k), dtype=torch.float32, device=DEV)
    fold = torch.ones((2, Cout), dtype=torch.float32, device=DEV)
    L = _lib.lib()
    need = L.i2l_conv_f32_workspace_bytes(1, *shape[:5], k, k, s, pd, 0)
    ok, y = _run_unit(x, 1, w, fold, None, shape, True, 0)
    assert ok == 0 and float(y.abs().max()) == 1.0                      # relu(1 * 0 + 1)
    for name in ("x", "w", "scale", "shift", "y"):
        rc, y = _run_unit(x, 1, w, fold, None, shape, True, 0, **{name: None})
        assert rc == -1 and torch.isnan(y).all(), name                  # I2L_ERR_ARG
    for kind in (0, 3, -1):
        rc, y = _run_unit(x, kind, w, fold, None, shape, True, 0, nbytes=need)
        assert rc == -2 and torch.isnan(y).all(), kind                  # I2L_ERR_UNSUPPORTED
    rc, y = _run_unit(x, 1, w, fold, None, shape, True, 0, nbytes=need - 1)
    assert rc == -3 and torch.isnan(y).all()                            # I2L_ERR_WORKSPACE
    rc, y = _run_unit(x, 1, w, fold, None, (B, H, W, Cin, 0, k, s, pd), True, 0, nbytes=need)
    assert rc == -1
    c = torch.zeros(8, dtype=torch.float32, device=DEV)
    assert L.i2l_bn_eval_fold_f32(None, c.data_ptr(), c.data_ptr(), c.data_ptr(), 1e-5, c.data_ptr(), c.data_ptr(), 8,
                                  _lib.stream_ptr()) == -1
    assert L.i2l_bn_eval_fold_f32(c.data_ptr(), c.data_ptr(), c.data_ptr(), c.data_ptr(), 1e-5, c.data_ptr(), c.data_ptr(), 0,
                                  _lib.stream_ptr()) == -1


# ------------------------------------------------------------------------------------------------ (2) the whole trunk
def _encoder(name, hw, seed=5, embedding_dim=64):
    enc = ResNetEncoder(hw[0], hw[1], 3, model_name=name, embedding_dim=embedding_dim)
    shapes = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    np_sd = synth.make_resnet_state_dict(shapes, seed=seed)
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in np_sd.items()}, strict=True)
    return enc.to(DEV).eval(), {"encoder." + k: torch.from_numpy(v.copy()) for k, v in np_sd.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("model_name,hw", MODELS)
def test_resnet_eval_fp32_vs_float64_oracle(model_name, hw):
    """Trunk features and encoder output of every model name the reference accepts (encoder.py:185-196) against
    resnet_oracle in float64.  Bound: 8 x the distance of the oracle's own fp32 evaluation to float64 (relative to the
    float64 maximum; 4.4e-7 .. 1.05e-6 for the features).  The bf16 trunk sits at 6e-3 .. 1.1e-2.  The call leaves the
    BatchNorm buffers bit-unchanged, and the default "bf16" output of the same module is bit-identical before and
    after the attribute was toggled."""
    enc, sd = _encoder(model_name, hw)
    x = torch.from_numpy(synth.uniform(9, "rimg", (3, 3, hw[0], hw[1]), -1.0, 1.0))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        feat64, out64 = RO.resnet_trunk(sd64, model_name, x.double()), RO.resnet_encoder(sd64, model_name, x.double())
        o_feat, o_out = _rel(RO.resnet_trunk(sd, model_name, x), feat64), _rel(RO.resnet_encoder(sd, model_name, x), out64)
        assert enc.eval_precision == "bf16"
        bf_before = enc(x.to(DEV)).clone()
        buffers = {k: v.clone() for k, v in enc.state_dict().items() if "running" in k or "num_batches" in k}
        enc.eval_precision = "fp32"
        feat, out = enc.trunk(x.to(DEV)).cpu(), enc(x.to(DEV)).cpu()
        for k, v in enc.state_dict().items():
            if k in buffers:
                assert torch.equal(v, buffers[k]), k
        enc.eval_precision = "bf16"
        assert torch.equal(enc(x.to(DEV)), bf_before)
    assert feat.dtype == torch.float32 and out.shape == (3, 64)
    e_feat, e_out = _rel(feat, feat64), _rel(out, out64)
    tag = f"{model_name} {hw[0]}x{hw[1]} eval fp32"
    record(tag + " trunk features HIP vs float64 oracle [rel to max]", e_feat)
    record(tag + " trunk features fp32 oracle vs float64 oracle [rel to max]", o_feat)
    record(tag + " encoder output HIP vs float64 oracle [rel to max]", e_out)
    record(tag + " encoder output fp32 oracle vs float64 oracle [rel to max]", o_out)
    print(f"{tag}: features HIP {e_feat:.3e} oracle32 {o_feat:.3e}; output HIP {e_out:.3e} oracle32 {o_out:.3e}")
    assert e_feat <= 8.0 * o_feat and e_out <= 8.0 * o_out, (e_feat, o_feat, e_out, o_out)
    # FLAG_EXACT_FP32 goes through; the bf16 trunk's tile-shape hints are ignored (same bits), not rejected
    with torch.no_grad():
        enc.eval_precision = "fp32"
        enc.kernel_flags = ResNetEncoder.MULTI_STREAM_FLAGS
        assert torch.equal(enc.trunk(x.to(DEV)).cpu(), feat)
        enc.kernel_flags = _lib.FLAG_EXACT_FP32
        e_exact = _rel(enc.trunk(x.to(DEV)).cpu(), feat64)
        enc.kernel_flags = 0
    record(tag + " trunk features HIP exact-fp32 vs float64 oracle [rel to max]", e_exact)
    assert e_exact <= 8.0 * o_feat, (e_exact, o_feat)


# ------------------------------------------------------------------------------------------------ (3) train / eval consistency
def _resnet_lstm(cfg, hw, res_seed, dec_kw):
    enc_p = dict(img_height=hw[0], img_width=hw[1], channels=3, model_name="resnet18", embedding_dim=cfg["embedding_dim"],
                 freeze_backbone=True)
    m = Seq2SeqModel("resnet_lstm", cfg["vocab_size"], enc_p, synth.decoder_params(cfg))
    shapes = [(k, tuple(v.shape)) for k, v in m.encoder.state_dict().items()]
    full = {"encoder." + k: torch.from_numpy(v.copy()) for k, v in synth.make_resnet_state_dict(shapes, seed=res_seed).items()}
    full.update({k: torch.from_numpy(v.copy()) for k, v in synth.make_state_dict(cfg, **dec_kw).items() if k.startswith("decoder.")})
    m.load_state_dict(full)
    return m.to(DEV).eval(), full


@pytest.mark.gpu
def test_validation_loss_is_the_fp32_arithmetic():
    """What a user who trained at fp32 grade needs: with ``model.encoder.eval_precision = "fp32"`` the teacher-forced
    logits and the loss of training.validate are those of the fp32 eval forward (resnet_oracle in fp32 -> the decoder
    oracle): 1e-4 absolute on the logits (the project's logit tolerance) and 1e-5 relative on val_loss (the tolerance of
    test_validator_matches_reference_validate, tests/test_validation_gpu.py line 173).  Validator and
    Seq2SeqModel see (B, E) fp32 features only and run unchanged."""
    from img2latex_amd.training import validate
    cfg = synth.model_config(vocab_size=60, embedding_dim=64, hidden_dim=64, dropout=0.0)      # dims of test_validator_resnet_lstm_smoke
    m, sd = _resnet_lstm(cfg, (32, 96), 3, dict(seed=4))
    m.encoder.eval_precision = "fp32"
    imgs = torch.from_numpy(synth.uniform(20, "images", (4, 3, 32, 96), -1.0, 1.0))
    forms = torch.from_numpy(synth.make_formulas(4, 14, 60, seed=30, min_len=5))
    with torch.no_grad():
        want_logits = O.decoder_forward(sd, cfg, RO.resnet_encoder(sd, "resnet18", imgs), forms[:, :-1])
        want_loss = float(O.ce_label_smooth(want_logits, forms[:, 1:], PAD))
        logits = m(imgs.to(DEV), forms.to(DEV)).cpu()
    e_logits = float((logits - want_logits).abs().max())
    record("resnet18_lstm eval fp32 teacher-forced logits vs fp32 oracle [abs]", e_logits)
    assert e_logits <= 1e-4, e_logits
    res = validate(m, [{"images": imgs, "formulas": forms}], PAD, bleu_batches=1, rng=random.Random(1))
    e_loss = abs(res["val_loss"] - want_loss) / abs(want_loss)
    record("resnet18_lstm eval fp32 val_loss vs fp32 oracle [rel]", e_loss)
    assert e_loss <= 1e-5, (res["val_loss"], want_loss)
    assert not m.training and res["val_samples"] == 4


# ------------------------------------------------------------------------------------------------ (4) kernel-shape independence
@pytest.mark.gpu
@pytest.mark.filterwarnings("error::RuntimeWarning")
def test_fp32_predict_ids_stream_equals_predict_batch_ids():
    """Predictor.predict_ids_stream runs two encoder streams, hence ResNetEncoder.MULTI_STREAM_FLAGS; predict_batch_ids
    runs one trunk with no flags.  With "fp32" the trunk has no tile-shape choice: the features of the two settings
    are bit-identical and so are the ids, row for row.  (The decoder differs between the two paths -- 16-member
    grouped decode against the 4-member one -- and may leave a row at an fp32 near-tie, as in
    test_predict_ids_stream_equals_predict_batch_ids: at most 2 rows.)  resnet18, primary-dims decoder."""
    from img2latex_amd.training import Predictor, TokenTable
    cfg = synth.model_config()                                          # E = H = 256, V = 512: the grouped decodes
    m, _ = _resnet_lstm(cfg, (32, 96), 5, dict(seed=42, out_scale=12.0, end_clock=(0.05, 12.0, 6.0)))
    m.encoder.eval_precision = "fp32"
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, cfg["vocab_size"])})
    pred = Predictor(m, TokenTable(vocab, max_sequence_length=150), device=torch.device(DEV))
    x = torch.from_numpy(synth.uniform(1234, "images", (160, 3, 32, 96), -1.0, 1.0)).to(DEV)
    batches = [x[i:i + 64] for i in range(0, 160, 64)]
    with torch.no_grad():
        plain = [m.encoder(b) for b in batches]
        m.encoder.kernel_flags = ResNetEncoder.MULTI_STREAM_FLAGS
        hinted = [m.encoder(b) for b in batches]
        m.encoder.kernel_flags = 0
    assert all(torch.equal(a, b) for a, b in zip(plain, hinted))
    want = [pred.predict_batch_ids(b, max_length=60) for b in batches]
    got = list(pred.predict_ids_stream(iter(batches), max_length=60))
    assert [len(g) for g in got] == [len(w) for w in want]
    assert len({tuple(r) for w in want for r in w}) > 16                # the rows decode to different sequences
    differ = sum(1 for g, w in zip(got, want) for a, b in zip(g, w) if a != b)
    record("resnet18 eval fp32 predict_ids_stream rows differing from predict_batch_ids", differ)
    assert differ <= 2, differ


# ------------------------------------------------------------------------------------------------ (5) host
def test_eval_precision_attribute_and_header():
    enc = ResNetEncoder(32, 64, 3, model_name="resnet18", embedding_dim=16)
    assert enc.eval_precision == "bf16"
    for bad in ("fp16", "FP32", None, 32):
        with pytest.raises(ValueError):
            enc.eval_precision = bad
    assert enc.eval_precision == "bf16"
    enc.eval_precision = "fp32"
    sd = enc.state_dict()
    assert not any("eval_precision" in k for k in sd)                   # neither a parameter nor a buffer
    assert "eval_precision" not in dict(enc.named_parameters()) and "eval_precision" not in dict(enc.named_buffers())
    enc.load_state_dict(sd, strict=True)
    assert enc.eval_precision == "fp32"
    other = ResNetEncoder(32, 64, 3, model_name="resnet18", embedding_dim=16)
    other.load_state_dict(sd, strict=True)
    assert other.eval_precision == "bf16"                               # not carried by a state_dict
    assert enc.train().eval().eval_precision == "fp32"
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for sym in ("i2l_bn_eval_fold_f32", "i2l_conv_bn_act_f32_fwd"):
        assert re.search(r"^int\s+" + sym + r"\s*\(", header, flags=re.M), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    assert _lib.lib().i2l_version() >= 101
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the fp32 trunk is a GPU path like the others
        with torch.no_grad():
            enc.eval()(torch.zeros(1, 3, 32, 64))
