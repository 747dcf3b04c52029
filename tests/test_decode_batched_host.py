"""Host side of the step-batched decode (i2l_greedy_decode_batched): the header declares it, _lib binds it, the scratch
size query and every refusal are pure host code -- they answer before the first HIP call, so none of this needs a GPU."""
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


def _call(w, rows=4, steps=3, tok0=FAKE, h0=None, c0=None, select=_lib.SELECT_LOGITS, stop=_lib.STOP_NONE,
          workspace=FAKE, scratch=FAKE, scratch_bytes=1 << 40):
    return _lib.lib().i2l_greedy_decode_batched(ctypes.byref(w), workspace, rows, steps, tok0, None, h0, c0, 1.0, select,
                                                stop, 2, FAKE, None, None, None, scratch, scratch_bytes, 0, None, 0, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_decode_batched_scratch_bytes", "i2l_greedy_decode_batched"):
        assert re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None
    assert re.search(r"#define\s+I2L_FLAG_DECODE_BATCHED\s+0x2000\b", header)
    assert _lib.FLAG_DECODE_BATCHED == 0x2000
    others = [v for k, v in vars(_lib).items() if k.startswith("FLAG_") and k != "FLAG_DECODE_BATCHED" and isinstance(v, int)]
    assert all(v != 0x2000 for v in others)
    assert _lib.lib().i2l_version() >= 105


def test_scratch_size_query():
    q = _lib.lib().i2l_decode_batched_scratch_bytes
    full = q(256, 500, 512, 2)
    # h (2, L, rows, H) + c (L, rows, H) + one padded row of logits per batch row, fp32
    assert full >= 4 * (3 * 2 * 256 * 512 + 256 * 512)
    assert q(0, 500, 512, 2) == 0
    assert q(256, 500, 96, 2) == 0
    assert q(256, 500, 512, 5) == 0
    assert q(256, 500, 2112, 2) == 0
    assert q(256, 0, 512, 2) == 0
    sizes = [q(r, 500, 512, 2) for r in (1, 16, 64, 256, 257)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert q(1, 3, 64, 1) > 0 and q(1, 3072, 2048, 4) > 0


@pytest.mark.parametrize("what,code", [
    ("select sample", _lib.ERR_ARG), ("select 7", _lib.ERR_ARG), ("stop 7", _lib.ERR_ARG), ("rows 0", _lib.ERR_ARG),
    ("steps 0", _lib.ERR_ARG), ("tok0 null", _lib.ERR_ARG), ("workspace null", _lib.ERR_ARG), ("h0 without c0", _lib.ERR_ARG),
    ("weights null", _lib.ERR_ARG), ("H 96", _lib.ERR_UNSUPPORTED), ("L 5", _lib.ERR_UNSUPPORTED),
    ("H 2112", _lib.ERR_UNSUPPORTED), ("E 30", _lib.ERR_UNSUPPORTED), ("scratch null", _lib.ERR_WORKSPACE),
    ("scratch one byte short", _lib.ERR_WORKSPACE), ("scratch 0 bytes", _lib.ERR_WORKSPACE)])
def test_refusals_need_no_device(what, code):
    """Every argument below is a fake pointer: a call that touched the device, or followed one of them, would not
    return a code."""
    w, keep = _weights()
    need = _lib.lib().i2l_decode_batched_scratch_bytes(4, 500, 512, 2)
    if what == "select sample":
        rc = _call(w, select=_lib.SELECT_SAMPLE)
    elif what == "select 7":
        rc = _call(w, select=7)
    elif what == "stop 7":
        rc = _call(w, stop=7)
    elif what == "rows 0":
        rc = _call(w, rows=0)
    elif what == "steps 0":
        rc = _call(w, steps=0)
    elif what == "tok0 null":
        rc = _call(w, tok0=None)
    elif what == "workspace null":
        rc = _call(w, workspace=None)
    elif what == "h0 without c0":
        rc = _call(w, h0=FAKE)
    elif what == "weights null":
        rc = _lib.lib().i2l_greedy_decode_batched(None, FAKE, 4, 3, FAKE, None, None, None, 1.0, 0, 0, 2, FAKE, None, None,
                                                  None, FAKE, 1 << 40, 0, None, 0, None)
    elif what in ("H 96", "L 5", "H 2112", "E 30"):
        w, keep = _weights(H={"H 96": 96, "H 2112": 2112}.get(what, 512), L=5 if what == "L 5" else 2,
                           E=30 if what == "E 30" else 512)
        rc = _call(w)
    elif what == "scratch null":
        rc = _call(w, scratch=None)
    elif what == "scratch one byte short":
        assert need > 0
        rc = _call(w, scratch_bytes=need - 1)
    else:
        rc = _call(w, scratch_bytes=0)
    del keep
    assert rc == code, (what, rc)
