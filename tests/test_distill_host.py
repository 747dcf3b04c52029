"""Distillation on the host (no GPU).

* distill_ref's two float64 forms -- the closed form on numpy arrays and torch autograd over F.cross_entropy + F.kl_div --
  agree to 1e-12: that pins the closed-form gradient the kernel evaluates.
* csrc/distill_rules.inc.h as a stand-alone program (csrc/distill_rules_host_main.cpp), a process of its own under the
  host sanitizers, evaluates rows in fp32 and is held to the float64 restatement by the rule of
  test_small_entries_vs_float64.py: the same formulas are evaluated in float32 on the CPU (distill_torch, float32) and
  err <= 4 * err_fp32cpu + floor, row-shared quantities (dlogits) taking the row's largest fp32 error.  The floors and
  their derivation are distill_ref.floors'.
* Every refusal of i2l_ce_distill_fwd_bwd is pure host code: it answers before the first HIP call, outputs untouched.
* TrainStep / Teacher refuse what they must without a device, and the CLI its bad option combinations."""
import ctypes
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import distill_ref as R
import png_cases
from conftest import record
from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows
RULE_IDS = {"logprob": _lib.ENSEMBLE_LOGPROB, "prob": _lib.ENSEMBLE_PROB}
MS, VS = (1, 2, 3, 8), (1, 3, 64, 65, 512, 513, 1025)
TAUS, ALPHAS, EPSS = (0.5, 1.0, 2.0, 4.0), (0.0, 0.3, 1.0), (0.0, 0.1)
KINDS = ("x3", "x30", "spike", "same")


def kind_rows(rng, M, V):
    """Four rows, one per kind: logits scaled by 3, by 30, one logit at +1e4 (student and teacher 0, in different columns
    where V allows), teacher equal to student.  -> x (4, V), z (M, 4, V) fp32."""
    x = rng.standard_normal((4, V)).astype(np.float32)
    z = rng.standard_normal((M, 4, V)).astype(np.float32)
    x[0] *= 3; z[:, 0] *= 3
    x[1] *= 30; z[:, 1] *= 30
    x[2] *= 3; z[:, 2] *= 3
    x[2, V // 3] = 1e4
    z[0, 2, (2 * V) // 3] = 1e4
    x[3] *= 3
    z[:, 3] = x[3]
    return x, z


# ------------------------------------------------------------------------------------------------ 1. the two float64 forms
def test_closed_form_is_the_autograd_gradient():
    rng = np.random.default_rng(4401)
    worst = 0.0
    for M, V, rule in itertools.product(MS, (1, 3, 65, 513), ("logprob", "prob")):
        for tau, alpha, eps in itertools.product(TAUS, ALPHAS, EPSS):
            x, z = kind_rows(rng, M, V)
            w = rng.uniform(0.2, 3.0, M).astype(np.float32)
            tgt = rng.integers(0, V, 4)
            pad = -100
            if V > 1:
                tgt[1], pad = 0, 0                                      # a pad row among them, its teacher rows NaN
                z[:, 1] = np.nan
            a = R.distill_np(x, z, w, rule, tgt, pad, tau, alpha, eps)
            b = R.distill_torch(x, z, w, rule, tgt, pad, tau, alpha, eps, torch.float64)
            for key in ("hard", "soft", "d"):
                assert np.isfinite(a[key]).all() and np.isfinite(b[key]).all(), (M, V, rule, tau, alpha, eps, key)
                err = np.abs(a[key] - b[key]) / np.maximum(1.0, np.abs(b[key]))
                worst = max(worst, float(err.max()))
                assert err.max() <= 1e-12, (M, V, rule, tau, alpha, eps, key, float(err.max()))
            if V > 1:
                assert not a["d"][1].any() and a["hard"][1] == 0 and a["soft"][1] == 0
            assert (a["soft"] >= -1e-9).all()                           # a divergence
    record("distill: numpy closed form vs torch autograd, float64 [max |err| / max(1, |ref|)]", worst)


def _oracle_logits(cfg, sd, images, formulas):
    import img2latex_oracle as O
    with torch.no_grad():
        return O.seq2seq_forward({k: torch.from_numpy(v).double() for k, v in sd.items()}, cfg,
                                 torch.from_numpy(images).double(), torch.from_numpy(formulas))


def test_learning_seed_holds_in_float64():
    """The scenario of test_distill_gpu.py's "it learns", in float64 on the CPU (oracle forward, autograd, the oracle's clip
    and Adam): this is where its seeds were picked.  After 40 steps on the fixed batch the soft loss is below its first
    value and the student's arg max agrees with the teacher's on more positions than before the first step."""
    import distill_cases as C
    c = C.LEARN
    scfg, ssd, tcfg, tsd, images, formulas = C.learn_case()
    assert (formulas[:, 1:] != C.PAD).all()
    teacher = _oracle_logits(tcfg, tsd, images, formulas)
    softs, first, last = R.simulate_training(ssd, scfg, teacher, images, formulas, C.PAD, c["tau"], c["alpha"], c["eps"],
                                             c["steps"], c["lr"])
    want = teacher.argmax(-1)
    before, after = int((first.argmax(-1) == want).sum()), int((last.argmax(-1) == want).sum())
    print(f"float64: soft {softs[0]:.4f} -> {softs[-1]:.5f}, arg max agreement {before} -> {after} of {want.numel()}")
    assert softs[-1] < 0.1 * softs[0] and after >= before + 8          # with room for fp32 and another Adam rounding


@pytest.mark.parametrize("V", [513, 3])
def test_shifted_teacher_shows_in_float64(V):
    """The control of the self-distillation check: with the teacher's rows read one position off, the float64 restatement
    gives a soft loss above 0.1 of the hard loss at the chosen seeds -- so "soft < 1e-3 hard" does tell aligned from shifted."""
    import distill_cases as C
    cfg, sd, images, formulas = C.self_case(V)
    x = _oracle_logits(cfg, sd, images, formulas).numpy()
    B, T, _ = x.shape
    tgt = formulas[:, 1:].reshape(-1)
    rows = x.reshape(B * T, V)
    same = R.distill_np(rows, rows[None], [1.0], "logprob", tgt, C.PAD, C.SELF_TAU, 0.5, 0.1)
    off = R.distill_np(rows, np.roll(x, 1, axis=1).reshape(1, B * T, V), [1.0], "logprob", tgt, C.PAD, C.SELF_TAU, 0.5, 0.1)
    assert same["soft"].sum() == 0.0 and same["hard"].sum() > 0
    assert off["soft"].sum() > 0.1 * off["hard"].sum(), (off["soft"].sum(), off["hard"].sum())


# ------------------------------------------------------------------------------------------------ 2. the rule in fp32
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe, sanitized = png_cases.build_host_program(str(tmp_path_factory.mktemp("distill_rules")), "distill_rules_host_main")
    print("distill_rules_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of distill_rules_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    return exe


def rule_cases():
    """(M, V, rule, tau, alpha, eps, w, x (4, V), z (M, 4, V), tgt (4)): the full cross of the issue's values, four rows
    (one per kind) each."""
    rng = np.random.default_rng(20270)
    out = []
    for M, V, rule in itertools.product(MS, VS, ("logprob", "prob")):
        for tau, alpha, eps in itertools.product(TAUS, ALPHAS, EPSS):
            x, z = kind_rows(rng, M, V)
            out.append((M, V, rule, tau, alpha, eps, rng.uniform(0.2, 3.0, M).astype(np.float32), x, z, rng.integers(0, V, 4)))
    return out


def judge(name, err, err_cpu, floor, what, share_row=False):
    err, err_cpu, floor = (np.asarray(t, dtype=np.float64) for t in (err, err_cpu, floor))
    floor = floor + 1e-300
    record(f"distill host {name} err [floors]", float((err / floor).max()))
    record(f"distill host {name} err_fp32cpu [floors]", float((err_cpu / floor).max()))
    if share_row:
        err_cpu = err_cpu.max(axis=-1, keepdims=True)
    assert np.isfinite(err).all(), (name, what)
    over = err - (4 * err_cpu + floor)
    assert float(over.max()) <= 0, (name, what, float((err / floor).max()), float((err_cpu / floor).max()))


def test_rule_vs_float64(host_program, tmp_path):
    cases = rule_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"DSTL" + struct.pack("<i", 4 * len(cases)))
        for M, V, rule, tau, alpha, eps, w, x, z, tgt in cases:
            for r in range(4):
                f.write(struct.pack("<iiiifff", M, V, RULE_IDS[rule], int(tgt[r]), tau, alpha, eps) + w.astype("<f4").tobytes()
                        + x[r].astype("<f4").tobytes() + z[:, r].astype("<f4").tobytes())
    r = subprocess.run([host_program, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    got_all = np.fromfile(dst, dtype="<f4").astype(np.float64)
    os.remove(src)
    os.remove(dst)
    assert got_all.size == sum(4 * (3 + c[1]) for c in cases)
    at = 0
    for M, V, rule, tau, alpha, eps, w, x, z, tgt in cases:
        got = got_all[at:at + 4 * (3 + V)].reshape(4, 3 + V)
        at += 4 * (3 + V)
        what = (M, V, rule, tau, alpha, eps)
        ref = R.distill_np(x, z, w, rule, tgt, -100, tau, alpha, eps)
        cpu = R.distill_torch(x, z, w, rule, tgt, -100, tau, alpha, eps, torch.float32)
        d_floor, hard_floor, soft_floor = R.floors(x, ref["y"], tgt, -100, tau, alpha, eps)
        a = R.f32(alpha)
        cpu_loss = a * cpu["hard"] + (1 - a) * cpu["soft"]
        judge("dlogits", np.abs(got[:, 3:] - ref["d"]), np.abs(cpu["d"] - ref["d"]), d_floor, what, share_row=True)
        judge("hard", np.abs(got[:, 0] - ref["hard"]), np.abs(cpu["hard"] - ref["hard"]), hard_floor, what)
        judge("soft", np.abs(got[:, 1] - ref["soft"]), np.abs(cpu["soft"] - ref["soft"]), soft_floor, what)
        judge("loss", np.abs(got[:, 2] - ref["loss"]), np.abs(cpu_loss - ref["loss"]), a * hard_floor + (1 - a) * soft_floor, what)
        if M == 1:                                       # teacher == student: every column's log q - log p is exactly 0
            assert got[3, 1] == 0.0, what
        sums = np.abs(got[:, 3:].sum(axis=1))
        assert (sums <= V * 2.0 ** -23 * (a + (1 - a) * R.f32(tau))).all(), (what, sums)


# ------------------------------------------------------------------------------------------------ 3. the C entry
def test_header_declares_and_lib_binds_the_entry():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    assert re.search(r"^int\s+i2l_ce_distill_fwd_bwd\s*\(", header, flags=re.M)
    assert re.search(r"^size_t\s+i2l_ce_distill_workspace_bytes\s*\(", header, flags=re.M)
    assert "typedef struct i2l_distill_teacher" in header
    for name in ("i2l_ce_distill_fwd_bwd", "i2l_ce_distill_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    assert len(L.i2l_ce_distill_fwd_bwd.argtypes) == 17
    assert L.i2l_version() >= 117 and _lib.ABI_VERSION >= 117
    assert L.i2l_ce_distill_workspace_bytes(0) == 0 and L.i2l_ce_distill_workspace_bytes(-3) == 0
    assert L.i2l_ce_distill_workspace_bytes(9536) >= 3 * 9536 * 4


def _teachers(n=2, logits=FAKE, ld=10, weights=None):
    recs = (_lib.DistillTeacher * max(n, 1))()
    for m in range(max(n, 0)):
        recs[m] = _lib.DistillTeacher(logits, ld, 1.0 if weights is None else weights[m])
    return recs


NEED = 3 * 256          # i2l_ce_distill_workspace_bytes(4)
REFUSALS = [
    ("logits null", dict(logits=None), _lib.ERR_ARG),
    ("targets null", dict(targets=None), _lib.ERR_ARG),
    ("sum and count null", dict(out_null=True), _lib.ERR_ARG),
    ("teachers null", dict(teachers_null=True), _lib.ERR_ARG),
    ("rows 0", dict(rows=0), _lib.ERR_ARG),
    ("rows -1", dict(rows=-1), _lib.ERR_ARG),
    ("vocab 0", dict(vocab=0), _lib.ERR_ARG),
    ("vocab -5", dict(vocab=-5), _lib.ERR_ARG),
    ("n 0", dict(n=0), _lib.ERR_ARG),
    ("n -1", dict(n=-1), _lib.ERR_ARG),
    ("n 9", dict(n=9), _lib.ERR_ARG),
    ("combine 2", dict(combine=2), _lib.ERR_ARG),
    ("combine -1", dict(combine=-1), _lib.ERR_ARG),
    ("temperature 0", dict(temperature=0.0), _lib.ERR_ARG),
    ("temperature negative", dict(temperature=-2.0), _lib.ERR_ARG),
    ("temperature inf", dict(temperature=float("inf")), _lib.ERR_ARG),
    ("temperature nan", dict(temperature=float("nan")), _lib.ERR_ARG),
    ("alpha below 0", dict(alpha=-0.01), _lib.ERR_ARG),
    ("alpha above 1", dict(alpha=1.01), _lib.ERR_ARG),
    ("alpha nan", dict(alpha=float("nan")), _lib.ERR_ARG),
    ("a teacher without logits", dict(teacher_logits=None), _lib.ERR_ARG),
    ("a teacher's ld below vocab", dict(ld=9), _lib.ERR_ARG),
    ("weight 0", dict(weights=(1.0, 0.0)), _lib.ERR_ARG),
    ("weight negative", dict(weights=(-0.5, 1.0)), _lib.ERR_ARG),
    ("weight nan", dict(weights=(float("nan"), 1.0)), _lib.ERR_ARG),
    ("weight inf", dict(weights=(1.0, float("inf"))), _lib.ERR_ARG),
    ("workspace null", dict(workspace=None), _lib.ERR_WORKSPACE),
    ("workspace one byte short", dict(workspace_bytes=NEED - 1), _lib.ERR_WORKSPACE),
    ("workspace empty", dict(workspace_bytes=0), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_need_no_device(what, kw, code):
    """Every input pointer is null or fake: a call that touched the device, or followed one of them, would not return a
    code.  The outputs and the workspace are host arrays of sentinels: a refused call leaves them as they were."""
    L = _lib.lib()
    assert L.i2l_ce_distill_workspace_bytes(4) == NEED
    kw = dict(kw)
    n = kw.pop("n", 2)
    recs = _teachers(n=max(n, 2) if n <= 8 else n, logits=kw.pop("teacher_logits", FAKE), ld=kw.pop("ld", 10),
                     weights=kw.pop("weights", None))
    d, out, parts = (ctypes.c_float * 40)(*([-1536.0] * 40)), (ctypes.c_float * 2)(-1536.0, -1536.0), (ctypes.c_float * 2)(-1536.0, -1536.0)
    ws = (ctypes.c_ubyte * NEED)(*([0xA5] * NEED))
    rc = L.i2l_ce_distill_fwd_bwd(
        kw.pop("logits", FAKE), kw.pop("targets", FAKE), kw.pop("rows", 4), kw.pop("vocab", 10), 0, 0.1,
        None if kw.pop("teachers_null", False) else recs, n, kw.pop("combine", _lib.ENSEMBLE_LOGPROB),
        kw.pop("temperature", 2.0), kw.pop("alpha", 0.5), kw.pop("workspace", ctypes.addressof(ws)),
        kw.pop("workspace_bytes", NEED), ctypes.addressof(d), None if kw.pop("out_null", False) else ctypes.addressof(out),
        ctypes.addressof(parts), None)
    assert not kw, kw
    assert rc == code, (what, rc)
    assert all(v == -1536.0 for v in d) and all(v == -1536.0 for v in out) and all(v == -1536.0 for v in parts), what
    assert all(b == 0xA5 for b in ws), what


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def _model(vocab=10, channels=1, hidden=64):
    from img2latex_amd import synth
    from img2latex_amd.model import Seq2SeqModel
    cfg = synth.model_config(vocab_size=vocab, embedding_dim=8, hidden_dim=hidden, lstm_layers=1, attention=False,
                             channels=channels, img_height=16, img_width=32, conv_filters=(4, 8, 16))
    return Seq2SeqModel("cnn_lstm", vocab, synth.encoder_params(cfg), synth.decoder_params(cfg))


def test_teacher_freezes_its_members_and_takes_the_ensembles_rule():
    from img2latex_amd.model import EnsembleModel
    from img2latex_amd.training import Teacher
    one = Teacher(_model())
    assert len(one.members) == 1 and one.weights == [1.0] and one.combine == _lib.ENSEMBLE_LOGPROB
    ens = Teacher(EnsembleModel([_model(), _model(hidden=128)], weights=[2.0, 1.0], combine="prob"), vocab_size=10)
    assert len(ens.members) == 2 and ens.weights == [2.0, 1.0] and ens.combine == _lib.ENSEMBLE_PROB
    for t in (one, ens):
        for m in t.members:
            assert not m.training and not any(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError, match="differ from the student's 11"):
        Teacher(_model(), vocab_size=11)
    with pytest.raises(ValueError, match="differ from the student's 12"):
        ens.check_vocab(12)
    with pytest.raises(RuntimeError, match="3-channel batch for a 1-channel teacher member"):
        one.logits(torch.zeros(2, 3, 16, 32), torch.zeros(2, 5, dtype=torch.int32))


def test_train_step_refuses_bad_distillation_arguments_before_it_needs_a_device():
    from img2latex_amd.training import Teacher, TrainStep
    student, teacher = _model(), Teacher(_model())
    with pytest.raises(TypeError, match="training.distill.Teacher"):
        TrainStep(student, teacher=_model())
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="distill_alpha"):
            TrainStep(student, teacher=teacher, distill_alpha=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="distill_temperature"):
            TrainStep(student, teacher=teacher, distill_temperature=bad)
    with pytest.raises(ValueError, match="differ from the student's 10"):
        TrainStep(student, teacher=Teacher(_model(vocab=11)))
    # accepted arguments get as far as the device check, which is the first thing TrainStep does without a teacher
    with pytest.raises(RuntimeError, match="needs the model on a ROCm device"):
        TrainStep(student, teacher=teacher, distill_alpha=0.3, distill_temperature=4.0)
    with pytest.raises(RuntimeError, match="needs the model on a ROCm device"):
        TrainStep(student, teacher=None, distill_alpha=7.0)             # without a teacher the two values are not looked at


def _vocab(extra):
    v = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    v.update({t: 4 + i for i, t in enumerate(extra)})
    return v


def _checkpoint(path, vocab, hidden=64):
    from img2latex_amd import synth
    from img2latex_amd.training.predictor import TokenTable, save_checkpoint
    cfg = synth.model_config(vocab_size=len(vocab), embedding_dim=8, hidden_dim=hidden, lstm_layers=1, attention=False,
                             channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16))
    config = {"model": {"name": "cnn_lstm", "embedding_dim": 8, "encoder": {"cnn": synth.encoder_params(cfg)},
                        "decoder": synth.decoder_params(cfg)}}
    save_checkpoint(str(path), _model(len(vocab), hidden=hidden), TokenTable(vocab, max_sequence_length=20), config)
    return str(path)


def test_teacher_from_checkpoints(tmp_path):
    from img2latex_amd.training import Teacher
    a = _checkpoint(tmp_path / "a.pt", _vocab(["x", "y"]))
    b = _checkpoint(tmp_path / "b.pt", _vocab(["x", "z"]), hidden=128)
    teacher, tables = Teacher.from_checkpoints([a, b], weights=[1.0, 3.0], combine="prob")
    assert len(teacher.members) == 2 and teacher.weights == [1.0, 3.0] and teacher.combine == _lib.ENSEMBLE_PROB
    assert [t.token_to_id for t in tables] == [_vocab(["x", "y"]), _vocab(["x", "z"])]
    assert teacher.members[1].decoder.hidden_dim == 128
    with pytest.raises(ValueError, match="2 ensemble weights for 1 members"):
        Teacher.from_checkpoints([a], weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="finite and > 0"):
        Teacher.from_checkpoints([a, b], weights=[1.0, 0.0])
    with pytest.raises(ValueError, match="unknown ensemble rule"):
        Teacher.from_checkpoints([a], combine="mean")
    with pytest.raises(ValueError, match="1 .. 8"):
        Teacher.from_checkpoints([a] * 9)
    with pytest.raises(ValueError, match="one vocabulary"):
        Teacher.from_checkpoints([a, _checkpoint(tmp_path / "c.pt", _vocab(["x"]))])


def test_cli_names_the_first_differing_token(tmp_path):
    from img2latex_amd import cli
    from img2latex_amd.training import TokenTable
    student = TokenTable(_vocab(["a", "b", "c"]))
    cli._check_teacher_tokens(["t.pt"], [TokenTable(_vocab(["a", "b", "c"]))], student)
    with pytest.raises(SystemExit, match=r"--teacher u\.pt: .*token 'b' \(student id 5, teacher id 6\)"):
        cli._check_teacher_tokens(["t.pt", "u.pt"], [TokenTable(_vocab(["a", "b", "c"])), TokenTable(_vocab(["a", "c", "b"]))], student)
    with pytest.raises(SystemExit, match=r"token 'c' \(student id 6, teacher id None\)"):
        cli._check_teacher_tokens(["t.pt"], [TokenTable(_vocab(["a", "b"]))], student)
    with pytest.raises(SystemExit, match=r"token 'd' \(teacher id 7, not in the student's vocabulary\)"):
        cli._check_teacher_tokens(["t.pt"], [TokenTable(_vocab(["a", "b", "c", "d"]))], student)


def test_cli_rejects_bad_distillation_options(capsys):
    from img2latex_amd import cli
    for argv, said in ((["train", "--teacher-weights", "1,2"], "--teacher-weights needs --teacher"),
                       (["train", "--teacher-rule", "prob"], "--teacher-rule needs --teacher"),
                       (["train", "--distill-alpha", "0.3"], "--distill-alpha needs --teacher"),
                       (["train", "--distill-temperature", "2"], "--distill-temperature needs --teacher"),
                       (["train", "--teacher", "a.pt", "--teacher-weights", "1,2"], "2 values for 1 checkpoints"),
                       (["train", "--teacher", "a.pt", "--teacher", "b.pt", "--teacher-weights", "1"], "1 values for 2 checkpoints"),
                       (["train", "--teacher", "a.pt", "--teacher-weights", "0"], "finite and above 0"),
                       (["train", "--teacher", "a.pt", "--distill-alpha", "1.5"], "distill_alpha must be in [0, 1]"),
                       (["train", "--teacher", "a.pt", "--distill-temperature", "0"], "distill_temperature must be finite and > 0"),
                       (["train", "--teacher", "a.pt", "--teacher-rule", "mean"], "invalid choice")):
        with pytest.raises(SystemExit) as exit_:
            cli.main(argv)
        assert exit_.value.code == 2, argv
        assert said in capsys.readouterr().err, argv


def test_train_takes_the_distillation_keywords_off_by_default():
    import inspect
    from img2latex_amd import cli
    from img2latex_amd.training import TrainStep
    p = inspect.signature(cli.train).parameters
    assert not p["teacher"].default and p["teacher_weights"].default is None and p["teacher_rule"].default == "logprob"
    assert p["distill_alpha"].default == 0.5 and p["distill_temperature"].default == 2.0
    q = inspect.signature(TrainStep.__init__).parameters
    assert q["teacher"].default is None and q["distill_alpha"].default == 0.5 and q["distill_temperature"].default == 2.0
