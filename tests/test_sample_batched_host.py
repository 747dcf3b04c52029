"""Host side of the step-batched sampling (i2l_sample_decode_batched, i2l_sample_logits): the header declares both, _lib
binds both, and every refusal is pure host code -- it answers before the first HIP call, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows


def _weights(V=500, E=512, H=512, L=2):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _decode(w, rows=4, steps=3, temperature=1.0, top_k=5, top_p=0.9, scratch=FAKE, scratch_bytes=1 << 40):
    return _lib.lib().i2l_sample_decode_batched(ctypes.byref(w), FAKE, rows, steps, FAKE, None, None, temperature, top_k,
                                                top_p, 7, _lib.STOP_NONE, 2, FAKE, None, None, None, scratch,
                                                scratch_bytes, 0, None)


def _logits(ld=500, rows=4, vocab=500, temperature=1.0, top_k=5, top_p=0.9, step=0):
    return _lib.lib().i2l_sample_logits(FAKE, ld, rows, vocab, temperature, top_k, top_p, 7, step, FAKE, None, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_sample_decode_batched", "i2l_sample_logits"):
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None
    assert len(_lib.lib().i2l_sample_decode_batched.argtypes) == 21
    assert len(_lib.lib().i2l_sample_logits.argtypes) == 12
    assert _lib.lib().i2l_version() >= 109


DECODE_REFUSALS = [
    ("temperature 0", dict(temperature=0.0), _lib.ERR_ARG),
    ("temperature negative", dict(temperature=-1.0), _lib.ERR_ARG),
    ("top_k -1", dict(top_k=-1), _lib.ERR_ARG),
    ("top_p -0.1", dict(top_p=-0.1), _lib.ERR_ARG),
    ("top_k and top_p zero", dict(top_k=0, top_p=0.0), _lib.ERR_ARG),
    ("top_p nan", dict(top_p=float("nan")), _lib.ERR_ARG),
    ("rows 0", dict(rows=0), _lib.ERR_ARG),
    ("steps 0", dict(steps=0), _lib.ERR_ARG),
    ("vocab 2049", dict(V=2049), _lib.ERR_UNSUPPORTED),
    ("hidden 96", dict(H=96), _lib.ERR_UNSUPPORTED),
    ("scratch null", dict(scratch=None), _lib.ERR_WORKSPACE),
    ("scratch one byte short", dict(short=1), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", DECODE_REFUSALS, ids=[r[0] for r in DECODE_REFUSALS])
def test_decode_refusals_need_no_device(what, kw, code):
    """Every pointer below is null or fake: a call that touched the device, or followed one of them, would not return a
    code."""
    kw = dict(kw)
    w, keep = _weights(V=kw.pop("V", 500), H=kw.pop("H", 512))
    if kw.pop("short", 0):
        need = _lib.lib().i2l_decode_batched_scratch_bytes(4, 500, 512, 2)
        assert need > 0
        kw["scratch_bytes"] = need - 1
    rc = _decode(w, **kw)
    if what == "top_p nan":     # one check for all three entries (sample_args_ok): the row kernel's entry refuses it as well
        assert _lib.lib().i2l_sample_decode(ctypes.byref(w), FAKE, 4, 3, FAKE, None, None, 1.0, 5, kw["top_p"], 7,
                                            _lib.STOP_NONE, 2, FAKE, None, None, None, None) == _lib.ERR_ARG
        assert _logits(**kw) == _lib.ERR_ARG
    del keep
    assert rc == code, (what, rc)


def test_greedy_entry_still_refuses_sampling():
    w, keep = _weights()
    rc = _lib.lib().i2l_greedy_decode_batched(ctypes.byref(w), FAKE, 4, 3, FAKE, None, None, None, 1.0, _lib.SELECT_SAMPLE,
                                              _lib.STOP_NONE, 2, FAKE, None, None, None, FAKE, 1 << 40, 0, None, 0, None)
    del keep
    assert rc == _lib.ERR_ARG


LOGITS_REFUSALS = [
    ("ld < vocab", dict(ld=499), _lib.ERR_ARG),
    ("vocab 2049", dict(ld=2049, vocab=2049), _lib.ERR_UNSUPPORTED),
    ("temperature 0", dict(temperature=0.0), _lib.ERR_ARG),
    ("temperature negative", dict(temperature=-0.5), _lib.ERR_ARG),
    ("top_k -1", dict(top_k=-1), _lib.ERR_ARG),
    ("top_p -0.1", dict(top_p=-0.1), _lib.ERR_ARG),
    ("top_k and top_p zero", dict(top_k=0, top_p=0.0), _lib.ERR_ARG),
    ("rows 0", dict(rows=0), _lib.ERR_ARG),
    ("vocab 0", dict(vocab=0), _lib.ERR_ARG),
    ("step -1", dict(step=-1), _lib.ERR_ARG),
]


@pytest.mark.parametrize("what,kw,code", LOGITS_REFUSALS, ids=[r[0] for r in LOGITS_REFUSALS])
def test_sample_logits_refusals_need_no_device(what, kw, code):
    assert _logits(**kw) == code, what
    if what == "rows 0":        # null pointers are refused as well
        assert _lib.lib().i2l_sample_logits(None, 500, 4, 500, 1.0, 5, 0.9, 7, 0, FAKE, None, None) == _lib.ERR_ARG
        assert _lib.lib().i2l_sample_logits(FAKE, 500, 4, 500, 1.0, 5, 0.9, 7, 0, None, None, None) == _lib.ERR_ARG
