"""Host side of the step-batched beam search (i2l_beam_decode_batched): the header declares it, _lib binds it, the
scratch size query and every refusal are pure host code -- they answer before the first HIP call, so none of this needs
a GPU."""
import ctypes
import os
import re

import pytest

from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows
SHIPPED = (500, 512, 2)


def _weights(V=500, E=512, H=512, L=2):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _call(w, images=4, beam=3, steps=5, workspace=FAKE, scratch=FAKE, scratch_bytes=1 << 40, seq=FAKE, ln=FAKE):
    return _lib.lib().i2l_beam_decode_batched(ctypes.byref(w) if w is not None else None, workspace, images, beam, steps,
                                              1, 2, scratch, scratch_bytes, seq, ln, None, 0, None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_beam_batched_scratch_bytes", "i2l_beam_decode_batched"):
        assert re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None
    assert re.search(r"#define\s+I2L_FLAG_BEAM_BATCHED\s+0x80000\b", header)
    assert _lib.FLAG_BEAM_BATCHED == 0x80000
    others = {k: v for k, v in vars(_lib).items() if k.startswith("FLAG_") and k != "FLAG_BEAM_BATCHED" and isinstance(v, int)}
    assert all(v != 0x80000 for v in others.values()), others
    # nor does it sit inside a multi-bit field of the flags word (ring depth: bits 8-11, patch shape: bits 20-23)
    assert not (_lib.flag_resnet_ring_depth(0xF) | _lib.flag_resnet_patch_shape(0xF)) & 0x80000
    defines = re.findall(r"#define\s+(I2L_FLAG_\w+)\s+(0x[0-9a-fA-F]+)\b", header)
    assert [n for n, v in defines if int(v, 16) == 0x80000] == ["I2L_FLAG_BEAM_BATCHED"]
    assert _lib.lib().i2l_version() >= 106


def test_scratch_size_query():
    q = _lib.lib().i2l_beam_batched_scratch_bytes
    V, H, L = SHIPPED
    one, full = q(1, 2, V, H, L, 150), q(128, 8, V, H, L, 150)
    assert one > 0 and full > 0
    # histories (2, images, steps, beam) int32 + h and c (2, L, rows, H) each + one padded row of logits per slot, fp32
    rows = 128 * 8
    assert full >= 4 * (2 * 128 * 150 * 8 + 2 * 2 * L * rows * H + rows * 512)
    grow = lambda sizes: all(a < b for a, b in zip(sizes, sizes[1:]))      # noqa: E731
    assert grow([q(n, 5, V, H, L, 150) for n in (1, 2, 16, 127, 128)])
    assert grow([q(16, k, V, H, L, 150) for k in range(1, 9)])
    assert grow([q(16, 5, V, H, L, t) for t in (1, 2, 40, 150, 151)])
    for what, args in {"images 0": (0, 2, V, H, L, 150), "beam 0": (4, 0, V, H, L, 150), "beam 9": (4, 9, V, H, L, 150),
                       "H 96": (4, 2, V, 96, L, 150), "H 2112": (4, 2, V, 2112, L, 150), "L 5": (4, 2, V, H, 5, 150),
                       "V 2049": (4, 2, 2049, H, L, 150), "steps 0": (4, 2, V, H, L, 0),
                       "beam > vocab": (4, 4, 3, 64, 1, 10)}.items():
        assert q(*args) == 0, what
    assert q(4, 8, 2048, 2048, 4, 10) > 0 and q(1, 3, 3, 64, 1, 1) > 0


@pytest.mark.parametrize("what,code", [
    ("weights null", _lib.ERR_ARG), ("workspace null", _lib.ERR_ARG), ("scratch null", _lib.ERR_ARG),
    ("seq_out null", _lib.ERR_ARG), ("len_out null", _lib.ERR_ARG), ("images 0", _lib.ERR_ARG), ("steps 0", _lib.ERR_ARG),
    ("beam 0", _lib.ERR_ARG), ("beam 9", _lib.ERR_UNSUPPORTED), ("beam > vocab", _lib.ERR_UNSUPPORTED),
    ("V 2049", _lib.ERR_UNSUPPORTED), ("H 96", _lib.ERR_UNSUPPORTED), ("H 2112", _lib.ERR_UNSUPPORTED),
    ("L 5", _lib.ERR_UNSUPPORTED), ("scratch one byte short", _lib.ERR_WORKSPACE), ("scratch 0 bytes", _lib.ERR_WORKSPACE)])
def test_refusals_need_no_device(what, code):
    """Every argument below is a fake pointer: a call that touched the device, or followed one of them, would not
    return a code."""
    w, keep = _weights()
    need = _lib.lib().i2l_beam_batched_scratch_bytes(4, 3, 500, 512, 2, 5)
    if what == "weights null":
        rc = _call(None)
    elif what == "workspace null":
        rc = _call(w, workspace=None)
    elif what == "scratch null":
        rc = _call(w, scratch=None)
    elif what == "seq_out null":
        rc = _call(w, seq=None)
    elif what == "len_out null":
        rc = _call(w, ln=None)
    elif what == "images 0":
        rc = _call(w, images=0)
    elif what == "steps 0":
        rc = _call(w, steps=0)
    elif what == "beam 0":
        rc = _call(w, beam=0)
    elif what == "beam 9":
        rc = _call(w, beam=9)
    elif what == "beam > vocab":
        w, keep = _weights(V=3, E=4, H=64, L=1)
        rc = _call(w, beam=4)
    elif what in ("V 2049", "H 96", "H 2112", "L 5"):
        w, keep = _weights(V=2049 if what == "V 2049" else 500, H={"H 96": 96, "H 2112": 2112}.get(what, 512),
                           L=5 if what == "L 5" else 2)
        rc = _call(w)
    elif what == "scratch one byte short":
        assert need > 0
        rc = _call(w, scratch_bytes=need - 1)
    else:
        rc = _call(w, scratch_bytes=0)
    del keep
    assert rc == code, (what, rc)


def test_i2l_beam_decode_ignores_the_bit():
    """The bit is the Python layer's switch: the parent's entry refuses and accepts exactly as without it."""
    w, keep = _weights()
    L = _lib.lib()
    for flags in (0, _lib.FLAG_BEAM_BATCHED):
        assert L.i2l_beam_decode(ctypes.byref(w), FAKE, 4, 3, 5, 1, 2, FAKE, 0, FAKE, FAKE, None, flags, None) == _lib.ERR_WORKSPACE
        assert L.i2l_beam_decode(ctypes.byref(w), FAKE, 4, 9, 5, 1, 2, FAKE, 1 << 40, FAKE, FAKE, None, flags, None) == _lib.ERR_UNSUPPORTED
    del keep
