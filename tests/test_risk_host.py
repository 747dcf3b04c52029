"""Minimum-risk fine-tuning on the host (no GPU).

* csrc/risk_rules.inc.h as a stand-alone program (csrc/risk_rules_host_main.cpp), a process of its own under the host
  sanitizers, against the Python / float64 restatement (risk_ref.py) on random batches and on the corners: an empty draw, a
  draw without END, a draw equal to the gold formula, an empty gold formula, all draws equal, N = 2 and N = 16.  Rows,
  distances, lengths and parts are exact; rewards, advantages and coefficients are the float64 values rounded to fp32 once.
* risk_ref's closed-form dlogits of the weighted cross entropy is torch's float64 autograd of L.
* The header declares and _lib binds the four entries; every refusal answers without a device and leaves the outputs as
  they were.
* RiskObjective / TrainStep refuse what they must without a device, the CLI options are off by default, and the CLI rejects
  bad values and a teacher beside the objective."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import png_cases
import risk_cases as C
import risk_ref as R
from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows


# ------------------------------------------------------------------------------------------------ 1. the rules
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    out = tmp_path_factory.mktemp("risk_host")
    exe, sanitized = png_cases.build_host_program(str(out), "risk_rules_host_main")
    return exe, sanitized, out


def run_host(host_program, cases):
    """cases: [(formulas (T + 1), draws (N, T), alpha, smoothing)] -> per case the dict risk_ref.risk_rows gives."""
    exe, _, out = host_program
    src, dst = str(out / "cases.bin"), str(out / "results.bin")
    with open(src, "wb") as f:
        f.write(b"RISK" + struct.pack("<i", len(cases)))
        for formulas, draws, alpha, smoothing in cases:
            N, T = draws.shape
            f.write(struct.pack("<5i2f", N, T, C.START, C.END, C.PAD, alpha, smoothing))
            f.write(np.ascontiguousarray(formulas, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(draws, dtype=np.int32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    raw, at, res = open(dst, "rb").read(), 0, []

    def take(count, dtype):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at)
        at += 4 * count
        return a
    for _, draws, _, _ in cases:
        N, T = draws.shape
        res.append(dict(rows=take((N + 1) * (T + 1), np.int32).reshape(N + 1, T + 1), coef=take(N + 1, np.float32),
                        smooth=take(N + 1, np.float32), part=take(N + 1, np.int32), dist=take(N, np.int32),
                        len=take(N, np.int32), reward=take(N, np.float32), advantage=take(N, np.float32)))
    assert at == len(raw)
    return res


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(got, ref, what):
    """Integers exact; the fp32 outputs bit-identical to the float64 values rounded once."""
    for key in ("rows", "part", "dist", "len"):
        assert np.array_equal(got[key], ref[key]), (what, key, got[key], ref[key])
    for key in ("coef", "smooth", "reward", "advantage"):
        assert same_bits(np.ascontiguousarray(got[key]), np.ascontiguousarray(ref[key])), (what, key, got[key], ref[key])


def test_the_row_wise_distance_is_the_table():
    rng = np.random.default_rng(3)
    for _ in range(200):
        a, b = (rng.integers(0, 4, int(rng.integers(0, 40))).tolist() for _ in range(2))
        assert R.levenshtein(a, b) == R.levenshtein_table(a, b), (a, b)
    assert R.levenshtein([], []) == 0 and R.levenshtein([1, 2], []) == 2 and R.levenshtein([], [5]) == 1


def test_the_sanitizers_are_on(host_program):
    assert host_program[1], "the host program was built without -fsanitize=address,undefined"


@pytest.mark.parametrize("N", [2, 3, 5, 16])
def test_rules_vs_float64_on_batches(host_program, N):
    """The batches of risk_cases (their corners rotate with the seed) at T on both sides of the 64-token blocks."""
    cases, refs = [], []
    for k, T in enumerate((1, 2, 7, 64, 65, 130)):
        for rep in range(6):
            seed = 100 * N + 10 * k + rep
            alpha, smoothing = (0.0, 0.3, 0.5, 1.0)[seed % 4], (0.0, 0.1)[seed % 2]
            formulas, draws = C.batch(N, T, seed)
            ref = R.risk_rows(formulas, draws, C.START, C.END, C.PAD, alpha, smoothing)
            for b in range(3):
                cases.append((formulas[b], draws[b], alpha, smoothing))
                sl = slice(b * (N + 1), (b + 1) * (N + 1))
                refs.append({k_: (v[sl] if v.shape[0] == 3 * (N + 1) else v[b]) for k_, v in ref.items()})
    for i, (got, ref) in enumerate(zip(run_host(host_program, cases), refs)):
        compare(got, ref, (N, i))


def test_corners_by_hand(host_program):
    """Each corner with its expected numbers written out."""
    T = 5
    gold = np.array([C.START, 3, 4, 5, C.END, C.PAD], dtype=np.int32)
    empty_gold = np.array([C.START, C.END, C.PAD, C.PAD, C.PAD, C.PAD], dtype=np.int32)
    empty, no_end = [C.END, -1, -1, -1, -1], [3, 4, 5, 6, 7]
    equal, sampled_pad = [3, 4, 5, C.END, -1], [3, C.PAD, 5, C.END, -1]
    cases = [(gold, np.array([empty, no_end], dtype=np.int32), 0.5, 0.1),
             (gold, np.array([equal, sampled_pad], dtype=np.int32), 0.25, 0.0),
             (empty_gold, np.array([empty, equal], dtype=np.int32), 0.0, 0.1),
             (gold, np.array([no_end] * 16, dtype=np.int32), 0.5, 0.1)]
    a, b, c, d = run_host(host_program, cases)
    # empty draw: d = 3 of max(0, 3) -> 0; no END: [3 4 5 6 7] against [3 4 5]: d = 2 of 5 -> 0.6
    assert a["dist"].tolist() == [3, 2] and a["len"].tolist() == [0, 5]
    assert a["reward"].tolist() == [0.0, np.float32(1 - 2 / 5)]
    assert a["advantage"].tolist() == [np.float32(0.0 - (1 - 2 / 5)), np.float32((1 - 2 / 5) - 0.0)]
    assert a["rows"].tolist() == [gold.tolist(), [C.START, C.END, C.PAD, C.PAD, C.PAD, C.PAD], [C.START, 3, 4, 5, 6, 7]]
    assert a["coef"].tolist() == [0.5, np.float32(0.5 * -(1 - 2 / 5)), np.float32(0.5 * (1 - 2 / 5))]
    assert a["smooth"].tolist() == [np.float32(0.1), 0.0, 0.0] and a["part"].tolist() == [0, 1, 1]
    # equal to gold: reward 1; a sampled PAD counts in the distance (one substitution of three) and stays in the row
    assert b["dist"].tolist() == [0, 1] and b["reward"].tolist() == [1.0, np.float32(1 - 1 / 3)]
    assert b["rows"][2].tolist() == [C.START, 3, C.PAD, 5, C.END, C.PAD]
    # empty gold: the empty draw has reward 1, the other 1 - 3 / 3 = 0
    assert c["dist"].tolist() == [0, 3] and c["reward"].tolist() == [1.0, 0.0] and c["coef"].tolist() == [0.0, 1.0, -1.0]
    # all draws equal: every advantage is 0 up to the rounding of the double sum of the 15 other rewards (15 x 0.6 is not
    # a double; each of the 15 additions rounds by at most half an ulp of a sum below 16)
    assert np.abs(d["advantage"]).max() <= 15 * 2.0 ** -50 and np.abs(d["coef"][1:]).max() <= 15 * 2.0 ** -50
    assert d["coef"][0] == 0.5 and d["reward"].tolist() == [np.float32(1 - 2 / 5)] * 16
    same2 = run_host(host_program, [(gold, np.array([no_end] * 2, dtype=np.int32), 0.5, 0.1)])[0]
    assert not same2["advantage"].any() and not same2["coef"][1:].any()          # N = 2: exactly 0 (+0 or -0)
    for got, (formulas, draws, alpha, smoothing) in zip((a, b, c, d), cases):
        ref = R.risk_rows(formulas[None], draws[None], C.START, C.END, C.PAD, alpha, smoothing)
        compare(got, {k: (v[0] if k in ("dist", "len", "reward", "advantage", "reward64", "advantage64") else v)
                      for k, v in ref.items()}, "by hand")


def test_host_program_refuses_what_the_entry_refuses(host_program, tmp_path):
    exe, _, _ = host_program
    for N, T, alpha in ((1, 5, 0.5), (17, 5, 0.5), (2, 1025, 0.5), (2, 5, 1.5), (2, 0, 0.5)):
        src = tmp_path / "bad.bin"
        src.write_bytes(b"RISK" + struct.pack("<i", 1) + struct.pack("<5i2f", N, T, 1, 2, 0, alpha, 0.1))
        assert subprocess.run([exe, str(src), str(tmp_path / "out.bin")], capture_output=True).returncode == 2, (N, T, alpha)


# ------------------------------------------------------------------------------------------------ 2. the loss
@pytest.mark.parametrize("V", [5, 256, 513])
def test_closed_form_dlogits_is_the_autograd_gradient(V):
    rng = np.random.default_rng(V)
    for steps in (1, 3):
        seqs = 6
        x = 3.0 * rng.standard_normal((seqs * steps, V))
        tgt = rng.integers(0, V, seqs * steps)
        tgt[1::4] = C.PAD
        coef = np.array([0.5, -0.75, 0.0, 1.25, -0.01, 0.3], dtype=np.float32)
        smooth = np.array([0.1, 0.0, 0.0, 0.1, 0.0, 0.2], dtype=np.float32)
        part = np.array([0, 1, 1, 0, 1, 1], dtype=np.int32)
        ref = R.weighted_ce_np(x, tgt, steps, C.PAD, coef, smooth, part)
        auto = R.weighted_ce_torch(x, tgt, steps, C.PAD, coef, smooth, torch.float64)
        assert np.abs(ref["d"] - auto["d"]).max() <= 1e-12
        assert np.abs(ref["loss"] - auto["loss"]).max() <= 1e-12 * max(1.0, np.abs(ref["loss"]).max())
        assert abs(ref["out"][0] - auto["total"]) <= 1e-12 * max(1.0, abs(auto["total"]))
        assert ref["out"][1] == (tgt != C.PAD).sum() and ref["parts"][1] + ref["parts"][3] == ref["out"][1]
        assert abs(ref["parts"][0] + ref["parts"][2] - ref["loss"].sum()) <= 1e-12 * ref["loss"].sum()


# ------------------------------------------------------------------------------------------------ 3. the C entries
def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_risk_rows", "i2l_ce_weighted_fwd_bwd", "i2l_rows_repeat", "i2l_rows_fold"):
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"^size_t\s+i2l_ce_weighted_workspace_bytes\s*\(", header, flags=re.M)
    assert "i2l_ce_weighted_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    assert len(L.i2l_risk_rows.argtypes) == 19 and len(L.i2l_ce_weighted_fwd_bwd.argtypes) == 15
    assert len(L.i2l_rows_repeat.argtypes) == 6 and len(L.i2l_rows_fold.argtypes) == 6
    assert L.i2l_version() >= 118 and _lib.ABI_VERSION >= 118
    assert L.i2l_ce_weighted_workspace_bytes(0) == 0 and L.i2l_ce_weighted_workspace_bytes(-3) == 0
    assert L.i2l_ce_weighted_workspace_bytes(12) == L.i2l_ce_workspace_bytes(12)
    makefile = open(os.path.join(REPO, "hmer-img2latex_amd", "csrc", "Makefile")).read()
    assert "train_risk.hip" in makefile


def _sentinels(n, ctype=ctypes.c_float, value=-1536.0):
    return (ctype * n)(*([value] * n))


def _untouched(*arrays):
    return all(all(v == a[0] for v in a) for a in arrays)


ROWS_REFUSALS = [
    ("formulas null", dict(formulas=None), _lib.ERR_ARG),
    ("draws null", dict(draws=None), _lib.ERR_ARG),
    ("an output null", dict(null_out=3), _lib.ERR_ARG),
    ("the last output null", dict(null_out=7), _lib.ERR_ARG),
    ("images 0", dict(images=0), _lib.ERR_ARG),
    ("steps 0", dict(steps=0), _lib.ERR_ARG),
    ("samples 0", dict(samples=0), _lib.ERR_ARG),
    ("samples -1", dict(samples=-1), _lib.ERR_ARG),
    ("alpha below 0", dict(alpha=-0.01), _lib.ERR_ARG),
    ("alpha above 1", dict(alpha=1.01), _lib.ERR_ARG),
    ("alpha nan", dict(alpha=float("nan")), _lib.ERR_ARG),
    ("smoothing 1", dict(smoothing=1.0), _lib.ERR_ARG),
    ("smoothing negative", dict(smoothing=-0.1), _lib.ERR_ARG),
    ("samples 1", dict(samples=1), _lib.ERR_UNSUPPORTED),
    ("samples 17", dict(samples=17), _lib.ERR_UNSUPPORTED),
    ("steps 1025", dict(steps=1025), _lib.ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("what,kw,code", ROWS_REFUSALS, ids=[r[0] for r in ROWS_REFUSALS])
def test_risk_rows_refusals_need_no_device(what, kw, code):
    """Every input pointer is null or fake: a call that touched the device, or followed one of them, would not return a
    code.  The outputs are host arrays of sentinels: a refused call leaves them as they were."""
    L = _lib.lib()
    kw = dict(kw)
    outs = [_sentinels(64, ctypes.c_int32, -77777), _sentinels(8), _sentinels(8), _sentinels(8, ctypes.c_int32, -77777),
            _sentinels(8, ctypes.c_int32, -77777), _sentinels(8, ctypes.c_int32, -77777), _sentinels(8), _sentinels(8)]
    ptrs = [ctypes.addressof(o) for o in outs]
    if "null_out" in kw:
        ptrs[kw.pop("null_out")] = None
    rc = L.i2l_risk_rows(kw.pop("formulas", FAKE), kw.pop("draws", FAKE), kw.pop("images", 2), kw.pop("samples", 3),
                         kw.pop("steps", 7), 1, 2, 0, kw.pop("alpha", 0.5), kw.pop("smoothing", 0.1), *ptrs, None)
    assert not kw, kw
    assert rc == code, (what, rc)
    assert _untouched(*outs), what


NEED = 2 * 256          # i2l_ce_weighted_workspace_bytes(12)
CE_REFUSALS = [
    ("logits null", dict(logits=None), _lib.ERR_ARG),
    ("targets null", dict(targets=None), _lib.ERR_ARG),
    ("coef null", dict(coef=None), _lib.ERR_ARG),
    ("smooth null", dict(smooth=None), _lib.ERR_ARG),
    ("part null", dict(part=None), _lib.ERR_ARG),
    ("sum and count null", dict(out_null=True), _lib.ERR_ARG),
    ("seqs 0", dict(seqs=0), _lib.ERR_ARG),
    ("steps -1", dict(steps=-1), _lib.ERR_ARG),
    ("vocab 0", dict(vocab=0), _lib.ERR_ARG),
    ("2^31 token rows", dict(seqs=1 << 16, steps=1 << 15), _lib.ERR_UNSUPPORTED),
    ("workspace null", dict(workspace=None), _lib.ERR_WORKSPACE),
    ("workspace one byte short", dict(workspace_bytes=NEED - 1), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", CE_REFUSALS, ids=[r[0] for r in CE_REFUSALS])
def test_weighted_ce_refusals_need_no_device(what, kw, code):
    L = _lib.lib()
    assert L.i2l_ce_weighted_workspace_bytes(12) == NEED
    kw = dict(kw)
    d, out, parts = _sentinels(120), _sentinels(2), _sentinels(4)
    ws = (ctypes.c_ubyte * NEED)(*([0xA5] * NEED))
    rc = L.i2l_ce_weighted_fwd_bwd(kw.pop("logits", FAKE), kw.pop("targets", FAKE), kw.pop("seqs", 4), kw.pop("steps", 3),
                                   kw.pop("vocab", 10), 0, kw.pop("coef", FAKE), kw.pop("smooth", FAKE), kw.pop("part", FAKE),
                                   kw.pop("workspace", ctypes.addressof(ws)), kw.pop("workspace_bytes", NEED),
                                   ctypes.addressof(d), None if kw.pop("out_null", False) else ctypes.addressof(out),
                                   ctypes.addressof(parts), None)
    assert not kw, kw
    assert rc == code, (what, rc)
    assert _untouched(d, out, parts) and all(b == 0xA5 for b in ws), what


@pytest.mark.parametrize("entry", ["i2l_rows_repeat", "i2l_rows_fold"])
def test_rows_refusals_need_no_device(entry):
    f = getattr(_lib.lib(), entry)
    out = _sentinels(64)
    for args in ((None, 2, 3, 4, ctypes.addressof(out)), (FAKE, 2, 3, 4, None), (FAKE, 0, 3, 4, ctypes.addressof(out)),
                 (FAKE, 2, 0, 4, ctypes.addressof(out)), (FAKE, 2, 3, 0, ctypes.addressof(out)),
                 (FAKE, 2, 3, -1, ctypes.addressof(out)), (FAKE, 1 << 20, 1 << 20, 4, ctypes.addressof(out))):
        assert f(*args, None) == _lib.ERR_ARG, (entry, args[1:4])
    assert _untouched(out)


# ------------------------------------------------------------------------------------------------ 4. the Python surface
def _model(vocab=10):
    from img2latex_amd import synth
    from img2latex_amd.model import Seq2SeqModel
    cfg = synth.model_config(vocab_size=vocab, embedding_dim=8, hidden_dim=64, lstm_layers=1, attention=False, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16))
    return Seq2SeqModel("cnn_lstm", vocab, synth.encoder_params(cfg), synth.decoder_params(cfg))


def test_risk_objective_checks_its_arguments_without_a_device():
    from img2latex_amd.training import RiskObjective
    ok = RiskObjective(1, 2)
    assert (ok.samples, ok.alpha, ok.temperature, ok.top_k, ok.top_p) == (4, 0.5, 1.0, 0, 0.0)
    RiskObjective(1, 2, samples=2, alpha=0.0, temperature=0.5, top_k=5, top_p=0.9)
    RiskObjective(1, 2, samples=16, alpha=1.0)
    for bad in (1, 0, 17, -3):
        with pytest.raises(ValueError, match="risk samples must be 2 .. 16"):
            RiskObjective(1, 2, samples=bad)
    with pytest.raises(TypeError, match="samples"):
        RiskObjective(1, 2, samples=2.5)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="risk alpha"):
            RiskObjective(1, 2, alpha=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="risk temperature"):
            RiskObjective(1, 2, temperature=bad)
    with pytest.raises(ValueError, match="risk top_k"):
        RiskObjective(1, 2, top_k=-1)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="risk top_p"):
            RiskObjective(1, 2, top_p=bad)
    with pytest.raises(ValueError, match="token ids"):
        RiskObjective(-1, 2)
    # out of scope, refused with a message
    with pytest.raises(ValueError, match="BLEU"):
        RiskObjective(1, 2, reward="bleu")
    with pytest.raises(ValueError, match="greedy"):
        RiskObjective(1, 2, baseline="greedy")
    with pytest.raises(ValueError, match="without a constraint"):
        RiskObjective(1, 2, constraint=object())


def test_risk_seed_is_a_fixed_one_to_one_mix():
    from img2latex_amd.training.risk import risk_seed
    from img2latex_amd.training.train_step import step_seed
    assert risk_seed(0) == 1442695040888963407 & 0x3FFFFFFFFFFFFFFF
    assert risk_seed(12345) == (12345 * 6364136223846793005 + 1442695040888963407) & 0x3FFFFFFFFFFFFFFF
    seeds = {risk_seed(step_seed(7, step, rank, micro)) for step in range(50) for rank in range(4) for micro in range(4)}
    assert len(seeds) == 50 * 4 * 4
    assert all(0 <= s < 1 << 62 for s in seeds)


def test_train_step_refuses_bad_risk_arguments_before_it_needs_a_device():
    from img2latex_amd.model import EnsembleModel
    from img2latex_amd.training import RiskObjective, Teacher, TrainStep
    student = _model()
    with pytest.raises(TypeError, match="training.risk.RiskObjective"):
        TrainStep(student, risk=dict(samples=4))
    with pytest.raises(ValueError, match="a teacher or a risk objective, not both"):
        TrainStep(student, teacher=Teacher(_model()), risk=RiskObjective(1, 2))
    with pytest.raises(TypeError, match="an ensemble is not a student"):
        TrainStep(EnsembleModel([_model(), _model()]), risk=RiskObjective(1, 2))
    with pytest.raises(ValueError, match="outside the vocabulary of 10"):
        TrainStep(student, risk=RiskObjective(1, 10))
    # an accepted objective gets as far as the device check, which is the first thing TrainStep does without one
    with pytest.raises(RuntimeError, match="needs the model on a ROCm device"):
        TrainStep(student, risk=RiskObjective(1, 2, samples=3))
    with pytest.raises(RuntimeError, match="needs the model on a ROCm device"):
        TrainStep(student, risk=None)


def test_the_options_are_off_by_default():
    import inspect
    from img2latex_amd import cli
    from img2latex_amd.training import TokenTable, TrainStep
    assert inspect.signature(cli.train).parameters["risk"].default is None
    assert inspect.signature(TrainStep.__init__).parameters["risk"].default is None
    table = TokenTable({"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3, "a": 4})
    assert cli._risk_objective(None, {}, table, False) is None
    assert cli._risk_objective({}, {"learning_rate": 1e-3}, table, True) is None
    # the command line's options stand over the config's keys
    obj = cli._risk_objective(dict(alpha=0.25), dict(risk_samples=3, risk_alpha=0.75, risk_top_k=5), table, False)
    assert (obj.samples, obj.alpha, obj.top_k, obj.start, obj.end) == (3, 0.25, 5, 1, 2)
    with pytest.raises(SystemExit, match="need --risk-samples"):
        cli._risk_objective(dict(alpha=0.25), {}, table, False)
    with pytest.raises(SystemExit, match="a teacher or the risk objective, not both"):
        cli._risk_objective(None, dict(risk_samples=2), table, True)
    with pytest.raises(SystemExit, match="risk samples must be 2 .. 16"):
        cli._risk_objective(None, dict(risk_samples=40), table, False)


def test_cli_rejects_bad_risk_options(capsys):
    from img2latex_amd import cli
    for argv, said in ((["train", "--risk-samples", "1"], "risk samples must be 2 .. 16"),
                       (["train", "--risk-samples", "17"], "risk samples must be 2 .. 16"),
                       (["train", "--risk-samples", "4", "--risk-alpha", "1.5"], "risk alpha must be in [0, 1]"),
                       (["train", "--risk-samples", "4", "--risk-temperature", "0"], "risk temperature must be finite and > 0"),
                       (["train", "--risk-samples", "4", "--risk-top-k", "-2"], "risk top_k must be >= 0"),
                       (["train", "--risk-samples", "4", "--risk-top-p", "1.5"], "risk top_p must be in [0, 1]"),
                       (["train", "--risk-samples", "x"], "invalid int value"),
                       (["train", "--risk-samples", "4", "--teacher", "a.pt"], "--risk-samples with --teacher"),
                       (["train", "--risk-alpha", "0.3", "--teacher", "a.pt"], "--risk-samples with --teacher")):
        with pytest.raises(SystemExit) as exit_:
            cli.main(argv)
        assert exit_.value.code == 2, argv
        assert said in capsys.readouterr().err, argv
