"""The ensemble decode on the host (no GPU).

* csrc/ensemble_rules.inc.h as a stand-alone program (csrc/ensemble_rules_host_main.cpp), a process of its own under the
  host sanitizers, evaluates the combination rule in fp32 and is held to the numpy float64 restatement
  (ensemble_ref.combine_np) within 1e-5 * max(1, |ref|): fp32 rounding of a V <= 2048-term sum, typically
  sqrt(V) * 2^-24 = 3e-6, times three.  No NaN where the restatement has none, -inf exactly where it has -inf.
* Every refusal of i2l_ensemble_decode is pure host code: it answers before the first HIP call.
* The Python surface refuses what has no ensemble form, and the CLI its bad option combinations."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import png_cases
from conftest import record
from ensemble_ref import combine_np
from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows
RULE_IDS = {"logprob": _lib.ENSEMBLE_LOGPROB, "prob": _lib.ENSEMBLE_PROB}


# ------------------------------------------------------------------------------------------------ 1. the rule
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe, sanitized = png_cases.build_host_program(str(tmp_path_factory.mktemp("ensemble_rules")), "ensemble_rules_host_main")
    print("ensemble_rules_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of ensemble_rules_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    return exe


def rule_cases():
    """(M, V, rule, weights, x (M, V) fp32, what): ordinary rows; rows with -inf in some columns of some members (one
    column -inf in EVERY member where V allows); one member all -inf; logits around -1e4 and around +80."""
    rng = np.random.default_rng(20261)
    out = []
    for M in (1, 2, 3, 8):
        for V in (1, 3, 64, 65, 513, 2048):
            for rule in ("logprob", "prob"):
                w = rng.uniform(0.2, 3.0, M).astype(np.float32)
                base = (3.0 * rng.standard_normal((M, V))).astype(np.float32)
                out.append((M, V, rule, w, base, "plain"))
                holes = base.copy()
                holes[rng.random((M, V)) < 0.3] = -np.inf
                holes[:, V // 2] = -np.inf                       # a column no member allows
                out.append((M, V, rule, w, holes, "holes"))
                dead = base.copy()
                dead[M - 1] = -np.inf                            # one member is all -inf
                out.append((M, V, rule, w, dead, "dead member"))
                far = base.copy()
                far[0] += np.float32(80.0)
                far[M // 2] -= np.float32(1e4)
                far[:, ::3] -= np.float32(1e4)
                out.append((M, V, rule, w, far, "far"))
    return out


def test_rule_vs_float64(host_program, tmp_path):
    cases = rule_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"ENSR" + struct.pack("<i", len(cases)))
        for M, V, rule, w, x, _ in cases:
            f.write(struct.pack("<iii", M, V, RULE_IDS[rule]) + w.astype("<f4").tobytes() + x.astype("<f4").tobytes())
    r = subprocess.run([host_program, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    got_all = np.fromfile(dst, dtype="<f4")
    assert got_all.size == sum(c[1] for c in cases)
    at, worst, kinds = 0, 0.0, set()
    for M, V, rule, w, x, what in cases:
        got = got_all[at:at + V].astype(np.float64)
        at += V
        ref = combine_np(x, w, rule)
        tag = (M, V, rule, what)
        assert not np.isnan(ref).any(), tag
        assert not np.isnan(got).any(), tag
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)), tag
        assert not np.isposinf(got).any(), tag
        fin = np.isfinite(ref)
        if fin.any():
            err = np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-5, (tag, float(err.max()))
        if np.isneginf(ref).any():
            kinds.add((rule, what, "some -inf" if fin.any() else "all -inf"))
    record("ensemble rule, fp32 host program vs float64: max |err| / max(1, |ref|)", worst)
    print(f"ensemble rule vs float64: max |err| / max(1, |ref|) = {worst:.3e}")
    # the inputs reach the corners the header names
    assert ("logprob", "dead member", "all -inf") in kinds and ("prob", "dead member", "all -inf") in kinds   # M == 1
    assert ("prob", "holes", "some -inf") in kinds and ("logprob", "holes", "some -inf") in kinds


def test_rule_corners_of_the_restatement():
    """What the header says about -inf, on the float64 restatement itself: one member's veto is final under logprob,
    under prob the other members decide and the dead member's weight is lost mass."""
    x = np.array([[0.0, 1.0, -np.inf], [0.0, -np.inf, -np.inf]])
    lp = combine_np(x, [1, 1], "logprob")
    pr = combine_np(x, [1, 1], "prob")
    assert np.isfinite(lp[0]) and np.isneginf(lp[1]) and np.isneginf(lp[2])
    assert np.isfinite(pr[:2]).all() and np.isneginf(pr[2])
    np.testing.assert_allclose(pr[1], np.log(0.5 * np.exp(1.0) / (1.0 + np.exp(1.0))), rtol=1e-12)
    dead = combine_np(np.array([[0.0, 0.0], [-np.inf, -np.inf]]), [3, 1], "prob")
    np.testing.assert_allclose(dead, np.log(0.75 * 0.5), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. the C entry
def _weights(V=500, E=512, H=512, L=2):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _members(shapes=((500, 512, 512, 2), (500, 64, 128, 1)), weights=None, workspace=FAKE, h0=None, c0=None):
    keep, recs = [], (_lib.EnsembleMember * max(len(shapes), 1))()
    for m, shape in enumerate(shapes):
        w, arrs = _weights(*shape)
        keep.append((w, arrs))
        recs[m] = _lib.EnsembleMember(ctypes.pointer(w), workspace, h0, c0, None, None,
                                      1.0 if weights is None else weights[m])
    return recs, keep


def _decode(recs, n, combine=_lib.ENSEMBLE_LOGPROB, rows=4, steps=3, tok0=FAKE, forced=None, temperature=1.0,
            select=_lib.SELECT_LOGITS, top_k=0, top_p=0.0, stop=_lib.STOP_NONE, end_id=2, cls=None, kind=_lib.CONSTRAIN_NONE,
            state=None, state_bytes=0, scratch=FAKE, scratch_bytes=1 << 40):
    return _lib.lib().i2l_ensemble_decode(recs, n, combine, rows, steps, tok0, forced, temperature, select, top_k, top_p, 7,
                                          stop, end_id, cls, kind, state, state_bytes, FAKE, None, scratch, scratch_bytes,
                                          0, None)


def test_header_declares_and_lib_binds_the_entry():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    assert re.search(r"^int\s+i2l_ensemble_decode\s*\(", header, flags=re.M)
    assert re.search(r"^size_t\s+i2l_ensemble_scratch_bytes\s*\(", header, flags=re.M)
    assert re.search(r"^#define\s+I2L_MAX_ENSEMBLE\s+8\b", header, flags=re.M) and _lib.MAX_ENSEMBLE == 8
    for name in ("i2l_ensemble_decode", "i2l_ensemble_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert len(_lib.lib().i2l_ensemble_decode.argtypes) == 24
    assert _lib.lib().i2l_version() >= 114
    # ONE decode entry: no family of six
    assert len(re.findall(r"^int\s+i2l_ensemble_\w+\s*\(", header, flags=re.M)) == 1


def test_accepted_arguments_get_as_far_as_the_scratch():
    """The calls below are refused for the scratch alone, so everything before it was accepted."""
    recs, keep = _members()
    assert _decode(recs, 2, scratch=None) == _lib.ERR_WORKSPACE
    assert _decode(recs, 2, combine=_lib.ENSEMBLE_PROB, select=_lib.SELECT_SAMPLE, top_k=5, top_p=0.9, scratch=None) == _lib.ERR_WORKSPACE
    assert _decode(recs, 2, cls=FAKE, kind=_lib.CONSTRAIN_BRACKETS, state=FAKE, state_bytes=64, scratch=None) == _lib.ERR_WORKSPACE
    assert _decode(recs, 2, cls=FAKE, kind=_lib.CONSTRAIN_ARGUMENTS, state=FAKE, state_bytes=128, scratch=None) == _lib.ERR_WORKSPACE
    assert _decode(recs, 2, forced=FAKE, scratch=None) == _lib.ERR_WORKSPACE
    assert _decode(recs, 1, scratch=None) == _lib.ERR_WORKSPACE
    del keep


def test_scratch_size():
    L = _lib.lib()
    recs, keep = _members()
    one = L.i2l_decode_batched_scratch_bytes(4, 500, 512, 2)
    two = L.i2l_decode_batched_scratch_bytes(4, 500, 128, 1)
    need = L.i2l_ensemble_scratch_bytes(recs, 2, 4)
    assert need >= one + two + 4 * 512 * 4                      # the members' scratches and the combined [rows][Vp] rows
    assert L.i2l_ensemble_scratch_bytes(recs, 1, 4) >= one
    assert _decode(recs, 2, scratch_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert L.i2l_ensemble_scratch_bytes(recs, 0, 4) == 0 and L.i2l_ensemble_scratch_bytes(recs, 9, 4) == 0
    assert L.i2l_ensemble_scratch_bytes(None, 2, 4) == 0 and L.i2l_ensemble_scratch_bytes(recs, 2, 0) == 0
    bad, keep2 = _members(((500, 512, 512, 2), (501, 64, 128, 1)))
    assert L.i2l_ensemble_scratch_bytes(bad, 2, 4) == 0
    del keep, keep2


NINE = ((500, 64, 64, 1),) * 9
REFUSALS = [
    ("n 0", dict(n=0), _lib.ERR_ARG),
    ("n -1", dict(n=-1), _lib.ERR_ARG),
    ("n 9", dict(shapes=NINE, n=9), _lib.ERR_UNSUPPORTED),
    ("members null", dict(members_null=True), _lib.ERR_ARG),
    ("a member without weights", dict(null_w=1), _lib.ERR_ARG),
    ("a member without workspace", dict(workspace=None), _lib.ERR_ARG),
    ("vocabularies differ", dict(shapes=((500, 512, 512, 2), (501, 64, 128, 1))), _lib.ERR_ARG),
    ("weight 0", dict(weights=(1.0, 0.0)), _lib.ERR_ARG),
    ("weight negative", dict(weights=(1.0, -0.5)), _lib.ERR_ARG),
    ("weight nan", dict(weights=(float("nan"), 1.0)), _lib.ERR_ARG),
    ("weight inf", dict(weights=(1.0, float("inf"))), _lib.ERR_ARG),
    ("unknown combine", dict(combine=2), _lib.ERR_ARG),
    ("unknown select", dict(select=3), _lib.ERR_ARG),
    ("unknown stop", dict(stop=2), _lib.ERR_ARG),
    ("unknown table kind", dict(kind=3, cls=FAKE, state=FAKE, state_bytes=1 << 20), _lib.ERR_ARG),
    ("rows 0", dict(rows=0), _lib.ERR_ARG),
    ("steps 0", dict(steps=0), _lib.ERR_ARG),
    ("tok0 null", dict(tok0=None), _lib.ERR_ARG),
    ("h0 without c0", dict(h0=FAKE), _lib.ERR_ARG),
    ("forced with sampling", dict(forced=FAKE, select=_lib.SELECT_SAMPLE, top_k=5), _lib.ERR_ARG),
    ("forced with brackets", dict(forced=FAKE, cls=FAKE, kind=_lib.CONSTRAIN_BRACKETS, state=FAKE, state_bytes=64), _lib.ERR_ARG),
    ("forced with arguments", dict(forced=FAKE, cls=FAKE, kind=_lib.CONSTRAIN_ARGUMENTS, state=FAKE, state_bytes=128), _lib.ERR_ARG),
    ("sampling: temperature 0", dict(select=_lib.SELECT_SAMPLE, top_k=5, temperature=0.0), _lib.ERR_ARG),
    ("sampling: top_k and top_p zero", dict(select=_lib.SELECT_SAMPLE), _lib.ERR_ARG),
    ("sampling: top_p nan", dict(select=_lib.SELECT_SAMPLE, top_k=5, top_p=float("nan")), _lib.ERR_ARG),
    ("sampling: vocab 2049", dict(shapes=((2049, 64, 64, 1),) * 2, select=_lib.SELECT_SAMPLE, top_k=5), _lib.ERR_UNSUPPORTED),
    ("hidden 96", dict(shapes=((500, 512, 512, 2), (500, 64, 96, 1))), _lib.ERR_UNSUPPORTED),
    ("layers 5", dict(shapes=((500, 512, 512, 2), (500, 64, 128, 5))), _lib.ERR_UNSUPPORTED),
    ("constraint: cls null", dict(kind=_lib.CONSTRAIN_BRACKETS, state=FAKE, state_bytes=64), _lib.ERR_ARG),
    ("constraint: state null", dict(kind=_lib.CONSTRAIN_BRACKETS, cls=FAKE, state_bytes=64), _lib.ERR_ARG),
    ("constraint: end_id -1", dict(kind=_lib.CONSTRAIN_BRACKETS, cls=FAKE, state=FAKE, state_bytes=64, end_id=-1), _lib.ERR_ARG),
    ("constraint: end_id == vocab", dict(kind=_lib.CONSTRAIN_ARGUMENTS, cls=FAKE, state=FAKE, state_bytes=128, end_id=500), _lib.ERR_ARG),
    ("bracket state one byte short", dict(kind=_lib.CONSTRAIN_BRACKETS, cls=FAKE, state=FAKE, state_bytes=63), _lib.ERR_WORKSPACE),
    ("argument state of the bracket size", dict(kind=_lib.CONSTRAIN_ARGUMENTS, cls=FAKE, state=FAKE, state_bytes=64), _lib.ERR_WORKSPACE),
    ("scratch null", dict(scratch=None), _lib.ERR_WORKSPACE),
    ("scratch one byte short", dict(short=1), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_decode_refusals_need_no_device(what, kw, code):
    """Every pointer is null or fake: a call that touched the device, or followed one of them, would not return a code."""
    kw = dict(kw)
    mk = {k: kw.pop(k) for k in ("shapes", "weights", "workspace", "h0") if k in kw}
    recs, keep = _members(**mk)
    n = kw.pop("n", len(mk.get("shapes", (0, 0))))
    if kw.pop("null_w", 0):
        recs[1].w = None
    if kw.pop("short", 0):
        need = _lib.lib().i2l_ensemble_scratch_bytes(recs, n, 4)
        assert need > 0
        kw["scratch_bytes"] = need - 1
    rc = _decode(None if kw.pop("members_null", False) else recs, n, **kw)
    del keep
    assert rc == code, (what, rc)


# ------------------------------------------------------------------------------------------------ 3. the Python surface
def _checkpoint(path, vocab, **cfg_kw):
    from img2latex_amd import synth
    from img2latex_amd.model import Seq2SeqModel
    from img2latex_amd.training.predictor import TokenTable, save_checkpoint
    cfg = synth.model_config(vocab_size=len(vocab), embedding_dim=8, hidden_dim=64, lstm_layers=1, attention=False,
                             channels=1, img_height=16, img_width=32, conv_filters=(4, 8, 16), **cfg_kw)
    model = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    config = {"model": {"name": "cnn_lstm", "embedding_dim": 8, "encoder": {"cnn": synth.encoder_params(cfg)},
                        "decoder": synth.decoder_params(cfg)}}
    save_checkpoint(str(path), model, TokenTable(vocab, max_sequence_length=20), config)
    return str(path)


def _vocab(extra):
    v = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    v.update({t: 4 + i for i, t in enumerate(extra)})
    return v


def test_from_checkpoints_names_the_first_difference(tmp_path):
    from img2latex_amd.training import Predictor
    a = _checkpoint(tmp_path / "a.pt", _vocab(["x", "y"]))
    b = _checkpoint(tmp_path / "b.pt", _vocab(["x", "z"]))
    with pytest.raises(ValueError, match="token_to_id"):
        Predictor.from_checkpoints([a, b])
    with pytest.raises(ValueError, match="2 ensemble weights for 1 members|weights"):
        Predictor.from_checkpoints([a], weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="finite and > 0"):
        Predictor.from_checkpoints([a, a], weights=[1.0, 0.0])
    with pytest.raises(ValueError, match="unknown ensemble rule"):
        Predictor.from_checkpoints([a, a], combine="mean")
    with pytest.raises(ValueError, match="1 .. 8"):
        Predictor.from_checkpoints([a] * 9)


def test_ensemble_model_refuses_beam_search():
    from img2latex_amd import synth
    from img2latex_amd.model import EnsembleDecoder, EnsembleModel, LSTMDecoder, Seq2SeqModel
    cfg = synth.model_config(vocab_size=10, embedding_dim=8, hidden_dim=64, lstm_layers=1, attention=False, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16))
    models = [Seq2SeqModel("cnn_lstm", 10, synth.encoder_params(cfg), synth.decoder_params(cfg)) for _ in range(2)]
    ens = EnsembleModel(models, weights=[2.0, 1.0], combine="prob")
    assert ens.decoder.combine == _lib.ENSEMBLE_PROB and ens.decoder.weights == [2.0, 1.0]
    x = torch.zeros((1, 1, 16, 32))
    with pytest.raises(RuntimeError, match="beam_size=3"):
        ens.inference(x, 1, 2, max_length=8, beam_size=3)
    with pytest.raises(RuntimeError, match="beam_search_batch"):
        ens.beam_search_batch(None, 1, 2, 8, 3)
    with pytest.raises(RuntimeError, match="beam_search_nbest"):
        ens.beam_search_nbest(None, 1, 2, 8, 3, nbest=2)
    with pytest.raises(ValueError, match="one vocabulary"):
        EnsembleDecoder([LSTMDecoder(10, 8, 64), LSTMDecoder(11, 8, 64)])
    with pytest.raises(ValueError, match="1 .. 8"):
        EnsembleDecoder([])


def test_cli_rejects_bad_ensemble_options(capsys):
    from img2latex_amd import cli
    for argv, said in ((["predict", "a.pt", "page.png", "--ensemble", "b.pt", "--beam-size", "3"], "--ensemble with --beam-size"),
                       (["evaluate", "a.pt", "data", "--ensemble", "b.pt", "--beam-size", "3"], "--ensemble with --beam-size"),
                       (["predict", "a.pt", "page.png", "--ensemble", "b.pt", "--ensemble-weights", "1,2,3"], "3 values for 2 checkpoints"),
                       (["predict", "a.pt", "page.png", "--ensemble", "b.pt", "--ensemble", "c.pt", "--ensemble-weights", "1,2"],
                        "2 values for 3 checkpoints"),
                       (["predict", "a.pt", "page.png", "--ensemble", "b.pt", "--ensemble-weights", "1,0"], "finite and above 0"),
                       (["predict", "a.pt", "page.png", "--ensemble-weights", "1"], "needs --ensemble"),
                       (["predict", "a.pt", "page.png", "--ensemble", "b.pt", "--ensemble-rule", "mean"], "invalid choice")):
        with pytest.raises(SystemExit) as exit_:
            cli.main(argv)
        assert exit_.value.code == 2, argv
        assert said in capsys.readouterr().err, argv
