"""Host side of the N-best beam search (i2l_beam_decode_nbest): the header declares it, _lib binds it, the scratch size
query, every refusal and the Python layer's validation of the length table are pure host code -- they answer before the
first HIP call, so none of this needs a GPU.  The float64 restatement the GPU tests compare against (nbest_ref.py) is
pinned here to the oracle's beam search at N = 1 without normalisation."""
import ctypes
import math
import os
import re

import pytest
import torch

import img2latex_oracle as O
import nbest_ref
from helpers import END, START, load, np_state_dict
from img2latex_amd import _lib, synth
from img2latex_amd.model import BeamHypothesis, Seq2SeqModel
from img2latex_amd.model.seq2seq_model import length_norm_table

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


def _call(w, images=4, beam=3, nbest=5, steps=5, workspace=FAKE, norm=None, scratch=FAKE, scratch_bytes=1 << 40, seq=FAKE,
          ln=FAKE, score=FAKE, key=None, fin=None, count=FAKE):
    return _lib.lib().i2l_beam_decode_nbest(ctypes.byref(w) if w is not None else None, workspace, images, beam, nbest,
                                            steps, 1, 2, norm, scratch, scratch_bytes, seq, ln, score, key, fin, count, 0,
                                            None)


def test_header_declares_and_lib_binds_the_entries():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_beam_nbest_scratch_bytes", "i2l_beam_decode_nbest"):
        assert re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None
    assert len(_lib.lib().i2l_beam_nbest_scratch_bytes.argtypes) == 7
    assert len(_lib.lib().i2l_beam_decode_nbest.argtypes) == 19
    assert re.search(r"#define\s+I2L_MAX_NBEST\s+16\b", header)
    assert _lib.MAX_NBEST == 16
    assert _lib.lib().i2l_version() >= 110


def test_scratch_size_query():
    q = _lib.lib().i2l_beam_nbest_scratch_bytes
    parent = _lib.lib().i2l_beam_batched_scratch_bytes
    V, H, L = SHIPPED
    for what, args in {"nbest 0": (4, 2, 0, V, H, L, 150), "nbest 17": (4, 2, 17, V, H, L, 150),
                       "beam 9": (4, 9, 5, V, H, L, 150), "V 2049": (4, 2, 5, 2049, H, L, 150),
                       "H 96": (4, 2, 5, V, 96, L, 150), "steps 0": (4, 2, 5, V, H, L, 0),
                       "images 0": (0, 2, 5, V, H, L, 150), "beam 0": (4, 0, 5, V, H, L, 150),
                       "beam > vocab": (4, 4, 5, 3, 64, 1, 10)}.items():
        assert q(*args) == 0, what
    grow = lambda sizes: all(0 < a < b for a, b in zip(sizes, sizes[1:]))      # noqa: E731
    assert grow([q(n, 5, 5, V, H, L, 150) for n in (1, 2, 16, 127, 128)])
    assert grow([q(16, k, 5, V, H, L, 150) for k in range(1, 9)])
    assert grow([q(16, 5, n, V, H, L, 150) for n in range(1, 17)])
    assert grow([q(1, 2, n, V, H, L, 150) for n in range(1, 17)])          # one image: every row still counts
    assert grow([q(16, 5, 5, V, H, L, t) for t in (1, 2, 40, 150, 151)])
    # the parent's scratch plus, per image, nbest entries of (key, score, history row, slot)
    for n, k, nb in ((1, 2, 1), (16, 5, 5), (128, 5, 10), (3, 2, 16)):
        assert q(n, k, nb, V, H, L, 150) >= parent(n, k, V, H, L, 150) + n * nb * 24
    assert q(4, 8, 16, 2048, 2048, 4, 10) > 0 and q(1, 3, 16, 3, 64, 1, 1) > 0     # nbest > beam is legal


@pytest.mark.parametrize("what,code", [
    ("weights null", _lib.ERR_ARG), ("workspace null", _lib.ERR_ARG), ("scratch null", _lib.ERR_ARG),
    ("seq_out null", _lib.ERR_ARG), ("len_out null", _lib.ERR_ARG), ("score_out null", _lib.ERR_ARG),
    ("count_out null", _lib.ERR_ARG), ("images 0", _lib.ERR_ARG), ("steps 0", _lib.ERR_ARG), ("beam 0", _lib.ERR_ARG),
    ("nbest 0", _lib.ERR_ARG), ("nbest -1", _lib.ERR_ARG), ("nbest 17", _lib.ERR_UNSUPPORTED),
    ("beam 9", _lib.ERR_UNSUPPORTED), ("beam > vocab", _lib.ERR_UNSUPPORTED), ("V 2049", _lib.ERR_UNSUPPORTED),
    ("H 96", _lib.ERR_UNSUPPORTED), ("H 2112", _lib.ERR_UNSUPPORTED), ("L 5", _lib.ERR_UNSUPPORTED),
    ("scratch one byte short", _lib.ERR_WORKSPACE), ("scratch 0 bytes", _lib.ERR_WORKSPACE),
    ("parent's scratch size", _lib.ERR_WORKSPACE)])
def test_refusals_need_no_device(what, code):
    """Every argument below is a fake pointer: a call that touched the device, or followed one of them, would not
    return a code."""
    w, keep = _weights()
    need = _lib.lib().i2l_beam_nbest_scratch_bytes(4, 3, 5, 500, 512, 2, 5)
    assert need > 0
    null = {"workspace null": "workspace", "scratch null": "scratch", "seq_out null": "seq", "len_out null": "ln",
            "score_out null": "score", "count_out null": "count"}
    count = {"images 0": dict(images=0), "steps 0": dict(steps=0), "beam 0": dict(beam=0), "nbest 0": dict(nbest=0),
             "nbest -1": dict(nbest=-1), "nbest 17": dict(nbest=17), "beam 9": dict(beam=9)}
    if what == "weights null":
        rc = _call(None)
    elif what in null:
        rc = _call(w, **{null[what]: None})
    elif what in count:
        rc = _call(w, **count[what])
    elif what == "beam > vocab":
        w, keep = _weights(V=3, E=4, H=64, L=1)
        rc = _call(w, beam=4)
    elif what in ("V 2049", "H 96", "H 2112", "L 5"):
        w, keep = _weights(V=2049 if what == "V 2049" else 500, H={"H 96": 96, "H 2112": 2112}.get(what, 512),
                           L=5 if what == "L 5" else 2)
        rc = _call(w)
    elif what == "scratch one byte short":
        rc = _call(w, scratch_bytes=need - 1)
    elif what == "parent's scratch size":
        rc = _call(w, scratch_bytes=_lib.lib().i2l_beam_batched_scratch_bytes(4, 3, 500, 512, 2, 5))
    else:
        rc = _call(w, scratch_bytes=0)
    del keep
    assert rc == code, (what, rc)


def test_optional_outputs_and_the_table_are_no_refusal():
    """key_out, finished_out and length_norm may be NULL or not: the next refusal in line (the scratch) still answers."""
    w, keep = _weights()
    for kw in (dict(), dict(key=FAKE), dict(fin=FAKE), dict(norm=FAKE), dict(key=FAKE, fin=FAKE, norm=FAKE)):
        assert _call(w, scratch_bytes=0, **kw) == _lib.ERR_WORKSPACE, kw
    del keep


def test_length_table_validation():
    assert length_norm_table(4) is None and length_norm_table(4, 0.0) is None
    assert length_norm_table(4, 0.7) == [1.0, 1.0, 2.0 ** 0.7, 3.0 ** 0.7, 4.0 ** 0.7]
    assert length_norm_table(3, 1.0) == [1.0, 1.0, 2.0, 3.0]
    gnmt = [((5 + n) / 6) ** 0.6 for n in range(5)]
    assert length_norm_table(4, 0.0, gnmt) == gnmt
    assert length_norm_table(4, length_norm=tuple(gnmt)) == gnmt


@pytest.mark.parametrize("what", ["short", "long", "zero", "negative", "nan", "inf", "with a penalty"])
def test_beam_search_nbest_validates_the_table_on_the_host(what):
    """The table is checked before the model's weights or the encoder output are looked at: no device is needed."""
    T = 6
    table = [1.0 + n for n in range(T + 1)]
    penalty = 0.0
    if what == "short":
        table = table[:-1]
    elif what == "long":
        table = table + [9.0]
    elif what == "zero":
        table[3] = 0.0
    elif what == "negative":
        table[0] = -1.0
    elif what == "nan":
        table[T] = math.nan
    elif what == "inf":
        table[1] = math.inf
    else:
        penalty = 0.5
    cfg = synth.model_config(vocab_size=3, embedding_dim=4, hidden_dim=64, lstm_layers=1, attention=False, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16))
    m = Seq2SeqModel("cnn_lstm", cfg["vocab_size"], synth.encoder_params(cfg), synth.decoder_params(cfg))
    with pytest.raises(ValueError):
        m.beam_search_nbest(torch.zeros(2, 4), START, END, T, 3, nbest=2, length_penalty=penalty, length_norm=table)
    with pytest.raises(ValueError):
        length_norm_table(T, penalty, table)


def test_hypothesis_tuple():
    h = BeamHypothesis([4, 5], -1.5, -0.75, True)
    assert h._fields == ("tokens", "score", "key", "finished") and tuple(h) == ([4, 5], -1.5, -0.75, True)


def test_cli_refuses_nbest_without_a_beam(capsys):
    from img2latex_amd import cli
    for argv in (["predict", "ck.pt", "x.png", "--nbest", "3"], ["predict", "ck.pt", "x.png", "--nbest", "3", "--beam-size", "0"],
                 ["predict", "ck.pt", "x.png", "--nbest", "-1", "--beam-size", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv                     # argparse's error exit
    assert "--nbest" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the restatement, pinned
@pytest.mark.parametrize("name", ["tiny_l1", "tiny_l2_attn", "odd_dims"])
def test_restatement_at_one_row_is_the_oracle(name):
    """nbest_ref with N = 1 and all-ones norm, in float64, gives exactly O.beam_search's sequence and score (norm None
    and an explicit table of ones alike); with more rows, row 0 stays and the rows are distinct and key-ordered."""
    _, cfg, _ = load(name)
    sd64 = {k: torch.from_numpy(v).double() for k, v in np_state_dict(name).items() if k.startswith("decoder.")}
    n, steps = (4 if name == "tiny_l1" else 3), 16
    enc = torch.from_numpy(synth.uniform(13, "enc", (n, cfg["embedding_dim"]), -1.5, 1.5)).double()
    for k in (3, 5):
        for j in range(n):
            with torch.no_grad():
                st, st1 = {}, {}
                want, wsc = O.beam_search(sd64, cfg, enc[j:j + 1], START, END, steps, k, return_score=True, stats=st)
                for norm in (None, [1.0] * (steps + 1)):
                    rows = nbest_ref.beam_search_nbest(sd64, cfg, enc[j:j + 1], START, END, steps, k, 1, norm, stats=st1)
                    assert len(rows) == 1
                    assert rows[0].tokens == want and rows[0].score == wsc and rows[0].key == wsc, (name, k, j)
                    assert st1["gap"] == st["gap"]
                many = nbest_ref.beam_search_nbest(sd64, cfg, enc[j:j + 1], START, END, steps, k, 2 * k, None, stats=st1)
            assert many[0] == rows[0]
            assert 1 <= len(many) <= 2 * k and len(many) == min(2 * k, st1["completed"] + st1["leftover"])
            nc = min(2 * k, st1["completed"])
            for part in (many[:nc], many[nc:]):
                assert all(a.key >= b.key for a, b in zip(part[:-1], part[1:]))
            assert all(r.finished for r in many[:nc])
            assert len({(tuple(r.tokens), r.finished) for r in many}) == len(many)
