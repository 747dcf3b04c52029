"""Host side of the step-batched training recurrences (I2L_FLAG_TRAIN_BATCHED): the header defines the flag and declares
the query, _lib binds both, the query is pure host code, and the workspace layout did not move.  None of this needs a
GPU; all of it fails on a build without the feature."""
import ctypes
import os
import re

import pytest

from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows
BIT = 0x100000


def test_header_defines_and_lib_binds_the_flag_and_the_query():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    assert re.search(r"#define\s+I2L_FLAG_TRAIN_BATCHED\s+0x100000\b", header)
    assert _lib.FLAG_TRAIN_BATCHED == BIT
    others = {k: v for k, v in vars(_lib).items() if k.startswith("FLAG_") and k != "FLAG_TRAIN_BATCHED" and isinstance(v, int)}
    assert all(v != BIT for v in others.values()), others
    defines = re.findall(r"#define\s+(I2L_FLAG_\w+)\s+(0x[0-9a-fA-F]+)\b", header)
    assert [n for n, v in defines if int(v, 16) == BIT] == ["I2L_FLAG_TRAIN_BATCHED"]
    name = "i2l_decoder_train_batched_ok"
    assert re.search(r"^int\s+" + name + r"\s*\(\s*int\s+vocab,\s*int\s+embed,\s*int\s+hidden,\s*int\s+layers\s*\)", header, flags=re.M)
    assert name in _lib.EXPORTED_SYMBOLS
    fn = getattr(_lib.lib(), name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_int] * 4
    assert _lib.lib().i2l_version() >= 107


@pytest.mark.parametrize("dims,want", [
    ((500, 512, 512, 2), 1),        # the shipped decoder
    ((10, 4, 1088, 1), 1),          # past the row kernels' 1024
    ((10, 4, 2048, 4), 1),          # the bound
    ((10, 4, 256, 1), 1),           # the grouped recurrences' own shape (A/B)
    ((10, 4, 96, 1), 0),            # hidden % 64
    ((10, 30, 64, 1), 0),           # embed % 4
    ((10, 4, 64, 5), 0),            # layers > 4
    ((10, 4, 2112, 1), 0),          # the first hidden size past the bound
    ((0, 4, 64, 1), 0), ((10, 0, 64, 1), 0), ((10, 4, 0, 1), 0), ((10, 4, 64, 0), 0)])
def test_query_values(dims, want):
    assert _lib.lib().i2l_decoder_train_batched_ok(*dims) == want


# recorded from the build before this feature: the flag must not move the layout
WORKSPACE_BYTES = {(64, 149, 500, 512, 512, 2): 687952384,
                   (5, 5, 3, 4, 64, 1): 2284288,
                   (33, 12, 777, 36, 192, 3): 26187264}


@pytest.mark.parametrize("args", sorted(WORKSPACE_BYTES))
def test_workspace_layout_did_not_move(args):
    assert _lib.lib().i2l_decoder_train_workspace_bytes(*args) == WORKSPACE_BYTES[args]


def _weights(V, E, H, L):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


def _fwd(w, flags, workspace_bytes=0):
    return _lib.lib().i2l_decoder_train_fwd(ctypes.byref(w), FAKE, FAKE, 3, 4, 0.0, 1, 0, FAKE, workspace_bytes, FAKE,
                                            flags, None)


def _bwd(w, flags, workspace_bytes=0):
    g = _lib.DecoderGrads()
    return _lib.lib().i2l_decoder_train_bwd(ctypes.byref(w), FAKE, 3, 4, 0.0, 1, 0, FAKE, workspace_bytes, FAKE,
                                            ctypes.byref(g), FAKE, flags, None, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_refusals_follow_the_flag_and_need_no_device(call):
    """Every pointer is fake and the workspace is 0 bytes: a call that passed the dimension check answers
    I2L_ERR_WORKSPACE (forward) or I2L_ERR_ARG (backward: its gradient struct is empty) before it touches anything."""
    passed = _lib.ERR_WORKSPACE if call is _fwd else _lib.ERR_ARG
    exact = _lib.FLAG_EXACT_FP32
    for dims, flags, code in [((10, 4, 1088, 1), 0, _lib.ERR_UNSUPPORTED),              # as before
                              ((10, 4, 1088, 1), BIT, passed),                          # the flag lifts the LDS bound
                              ((10, 4, 1088, 1), BIT | exact, _lib.ERR_UNSUPPORTED),    # exact fp32: the flag is ignored
                              ((10, 4, 2112, 1), BIT, _lib.ERR_UNSUPPORTED),
                              ((10, 4, 96, 1), BIT, _lib.ERR_UNSUPPORTED),
                              ((10, 30, 64, 1), BIT, _lib.ERR_UNSUPPORTED),
                              ((10, 4, 64, 5), BIT, _lib.ERR_UNSUPPORTED),
                              ((500, 512, 512, 2), 0, passed), ((500, 512, 512, 2), BIT, passed)]:
        w, keep = _weights(*dims)
        assert call(w, flags) == code, (dims, hex(flags))
        del keep


def test_cli_option_maps_to_the_flag():
    from img2latex_amd import cli
    assert cli._train_flags("auto") == 0 and cli._train_flags("batched") == BIT
    with pytest.raises(SystemExit):
        cli._train_flags("grouped")
    with pytest.raises(SystemExit):                         # argparse refuses it before anything is built
        cli.main(["train", "--train-kernel", "grouped"])


def test_bits_20_to_23_are_read_by_the_resnet_entry_alone():
    """0x100000 is also I2L_FLAG_RESNET_PATCH_SHAPE(1): the flags word is per entry, and that field is the bf16 ResNet
    conv entry's.  Nothing the decoder's flags reach may read it, in the library or in the Python layer."""
    assert _lib.flag_resnet_patch_shape(1) == BIT
    csrc = os.path.join(REPO, "hmer-img2latex_amd", "csrc")
    readers = sorted(name for name in os.listdir(csrc) if name.endswith((".hip", ".h"))
                     and re.search(r">>\s*20\b|PATCH_SHAPE\s*\(", open(os.path.join(csrc, name)).read()))
    assert readers and all(name.startswith("resnet") for name in readers), readers
    pkg = os.path.join(REPO, "hmer-img2latex_amd", "img2latex_amd")
    users = []
    for root, _, names in os.walk(pkg):
        for name in names:
            if name.endswith(".py") and "flag_resnet_patch_shape" in open(os.path.join(root, name)).read():
                users.append(os.path.relpath(os.path.join(root, name), pkg))
    assert set(users) <= {"_lib.py", os.path.join("model", "resnet_encoder.py")}, users
