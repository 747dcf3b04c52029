"""Host side of the two-batch grouped launch (i2l_greedy_decode_halves): the header declares it, _lib binds it, the layout
entry points size the exchange region and the state block, and every refusal is pure host code -- it answers before the
first HIP call, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows
DIMS = (512, 256, 256, 1)     # vocab, embed, hidden, layers of the 16-member grouped decode


def _weights(V=512, E=256, H=256, L=1):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _half(rows=32, steps=40, first=0, n=20, workspace=FAKE, tok0=FAKE, ids=FAKE):
    return _lib.DecodeHalf(workspace, rows, steps, first, n, tok0, ids)


def _call(w, older, newer, select=_lib.SELECT_LOGITS, stop=_lib.STOP_NONE):
    ref = lambda h: None if h is None else ctypes.byref(h)
    return _lib.lib().i2l_greedy_decode_halves(ctypes.byref(w), ref(older), ref(newer), 1.0, select, stop, 2, 0, None, 0, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_greedy_decode_halves", "i2l_decoder_group_state_offset", "i2l_decoder_group_state_bytes"):
        assert re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None
    assert re.search(r"\}\s*i2l_decode_half\s*;", header)
    # the Python struct mirrors the C one: two pointers around four ints
    assert [n for n, _ in _lib.DecodeHalf._fields_] == ["workspace", "rows", "steps", "first_step", "n_steps", "tok0", "ids_out"]
    assert ctypes.sizeof(_lib.DecodeHalf) == 8 + 4 * 4 + 8 + 8
    assert _lib.lib().i2l_version() >= 108


@pytest.mark.parametrize("rows", [1, 16, 17, 256, 257])
def test_region_and_state_sizes(rows):
    """The group region holds the two-tile launch's granules -- per group 2 step parities x 16 members x (512 h granules
    + 32 candidates + 32 for the placement granule's line) x 8 bytes, groups of 16 rows padded to a multiple of 8 -- or the
    4-member kernel's, whichever is larger, behind 2048 bytes of status words; the state block follows it: c and h as fp32
    per (row, unit) and the last token per row, rows padded to whole groups, a fin mask and a failed word per group."""
    L = _lib.lib()
    groups = -(-rows // 16)
    two_tile = -(-groups // 8) * 8 * 2 * 16 * (512 + 64) * 8
    four_member = -(-(-(-rows // 4)) // 8) * 8 * 2 * 4 * (256 + 32) * 8
    region = L.i2l_decoder_group_region_bytes(rows, *DIMS)
    assert region == 2048 + max(two_tile, four_member)
    status = L.i2l_decoder_group_status_offset(rows, *DIMS)
    state = L.i2l_decoder_group_state_offset(rows, *DIMS)
    nbytes = L.i2l_decoder_group_state_bytes(rows, *DIMS)
    assert nbytes == groups * 16 * (2 * 256 * 4 + 4) + groups * 2 * 4
    assert status > 0 and state >= status + region and state % 256 == 0
    assert state + nbytes <= L.i2l_decoder_workspace_bytes(rows, *DIMS)


def test_no_state_block_without_the_16_member_kernel():
    L = _lib.lib()
    for dims in ((512, 256, 512, 1), (512, 256, 256, 2), (513, 256, 256, 1)):
        assert L.i2l_decoder_group_state_bytes(32, *dims) == 0 and L.i2l_decoder_group_state_offset(32, *dims) == 0


@pytest.mark.parametrize("what,code", [
    ("sticky stop", _lib.ERR_UNSUPPORTED), ("L 2", _lib.ERR_UNSUPPORTED), ("H 512", _lib.ERR_UNSUPPORTED),
    ("V 513", _lib.ERR_UNSUPPORTED), ("steps 65001", _lib.ERR_UNSUPPORTED), ("older needs more groups", _lib.ERR_UNSUPPORTED),
    ("weights null", _lib.ERR_ARG), ("select sample", _lib.ERR_ARG), ("stop 7", _lib.ERR_ARG), ("ids null", _lib.ERR_ARG),
    ("workspace null", _lib.ERR_ARG), ("range past the end", _lib.ERR_ARG), ("negative first step", _lib.ERR_ARG)])
def test_refusals_need_no_device(what, code):
    """Every pointer below is fake: a call that touched the device, or followed one of them, would not return a code."""
    w, keep = _weights()
    older, newer, kw = _half(first=20, n=20), _half(), {}
    if what == "sticky stop":
        kw["stop"] = _lib.STOP_STICKY
    elif what == "L 2":
        w, keep = _weights(L=2)
    elif what == "H 512":
        w, keep = _weights(H=512)
    elif what == "V 513":
        w, keep = _weights(V=513)
    elif what == "steps 65001":
        newer = _half(steps=65001)
    elif what == "older needs more groups":
        older, newer = _half(rows=256, first=20, n=20), _half(rows=64)     # 16 groups against a region made for 8
    elif what == "weights null":
        w.w_out = None
    elif what == "select sample":
        kw["select"] = _lib.SELECT_SAMPLE
    elif what == "stop 7":
        kw["stop"] = 7
    elif what == "ids null":
        newer = _half(ids=None)
    elif what == "workspace null":
        older = _half(first=20, n=20, workspace=None)
    elif what == "range past the end":
        older = _half(first=21, n=20)
    elif what == "negative first step":
        newer = _half(first=-1)
    assert _call(w, older, newer, **kw) == code
    del keep
