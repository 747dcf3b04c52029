"""The step-batched matrix-core beam search (i2l_beam_decode_batched, _lib.FLAG_BEAM_BATCHED) against the float64 search
of the oracle, the reference's own fixtures and the parent's entry.  A search ranks k * k fp64 sums of fp32
log-probabilities per step; the float64 search records its smallest gap between neighbours among the k + 1 best
candidates of any step (``stats["gap"]``), and an fp32 evaluation in another summation order may rank differently below
1e-4.  So, as in test_decoder_shapes.test_beam_search_vs_float64: sequences equal the float64 ones unless that gap is
below 1e-4, equal sequences score within 1e-4 relative to max(1, |score|), and the searches that leave are capped."""
import ctypes

import numpy as np
import pytest
import torch

import img2latex_oracle as O
from conftest import record
from helpers import END, START, images, load, model_for, np_state_dict, padded_to_lists
from img2latex_amd import _lib, synth
from test_decoder_shapes import build, enc_for, sid

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAG = _lib.FLAG_BEAM_BATCHED
GAP = 1e-4
SHIPPED = (500, 512, 512, 2, True)


def check_vs_float64(tag, m, sd64, cfg, enc, steps, k, V, cap):
    """One batched search of ``enc``'s images under the flag against one float64 search per image.  Returns nothing;
    records the searches that leave the float64 one and those below the gap, asserts the rule of the module docstring."""
    with torch.no_grad():
        got, scores = m.beam_search_batch(enc, START, END, steps, k, return_scores=True, flags=FLAG)
    n = enc.shape[0]
    assert len(got) == n and len(scores) == n
    left, below, worst = 0, 0, 0.0
    for j in range(n):
        st = {}
        with torch.no_grad():
            seq, sc = O.beam_search(sd64, cfg, enc[j:j + 1].double(), START, END, steps, k, return_score=True, stats=st)
        below += st["gap"] < GAP
        assert all(0 <= t < V for t in got[j]), (tag, k, j)
        assert np.isfinite(scores[j]) and scores[j] <= 0.0, (tag, k, j, scores[j])
        if got[j] != seq:
            assert st["gap"] < GAP, (tag, k, j, st["gap"], got[j], seq)
            left += 1
            continue
        err = abs(scores[j] - sc) / max(1.0, abs(sc))
        worst = max(worst, err)
        assert err <= 1e-4, (tag, k, j, scores[j], sc)
    record(f"batched {tag} beam k={k} x {n} images x {steps} steps: winning score vs float64 [rel to max(1,|score|)]", worst)
    record(f"batched {tag} beam k={k} x {n} images x {steps} steps: searches leaving the float64 one at a near-tie", left)
    record(f"batched {tag} beam k={k} x {n} images x {steps} steps: searches with a float64 gap below 1e-4", below)
    assert left <= cap, (tag, k, left, cap)


# ------------------------------------------------------------------------------------------------ 1. against the float64 search
# (shape, variant, k, images)
CASES = [
    ((3, 4, 64, 1, False), None, 1, 7),              # one column tile
    ((3, 4, 64, 1, False), None, 3, 7),              # k == V
    ((513, 256, 256, 1, False), None, 3, 7),         # Vp = 1024
    ((777, 36, 192, 3, True), None, 5, 7),           # H no multiple of 128, three layers, 35 rows ragged against 16
    ((777, 36, 192, 3, True), "negative", 3, 7),     # no padding column may enter a top-k
    ((2048, 64, 128, 2, True), None, 8, 7),          # the vocabulary limit, the widest beam
    (SHIPPED, None, 2, 8),                           # the reference's default call on the shipped decoder
    (SHIPPED, None, 5, 8),
    (SHIPPED, None, 8, 4),                           # refused by beam_kernel<8>: 164 624 B of LDS
]


@pytest.mark.parametrize("shape,variant,k,n", CASES, ids=[f"{sid(s, v)}-k{k}-n{n}" for s, v, k, n in CASES])
def test_beam_search_vs_float64(shape, variant, k, n):
    m, sd64, cfg = build(shape, variant)
    enc = enc_for(shape, n, seed=13)
    if shape == SHIPPED and k == 8:
        with pytest.raises(RuntimeError), torch.no_grad():       # without the flag: one workgroup per image, state in LDS
            m.beam_search_batch(enc, START, END, 24, k)
    check_vs_float64(sid(shape, variant), m, sd64, cfg, enc, 24, k, shape[0], cap=1)
    assert m.decoder.kernel_flags == 0


# ------------------------------------------------------------------------------------------------ 2. many rows; a long search
def test_more_than_one_row_tile():
    """52 images x k = 5 = 260 rows: 64-row tiles, the last one with 4 rows."""
    m, sd64, cfg = build(SHIPPED)
    enc = enc_for(SHIPPED, 52, seed=13)
    check_vs_float64(sid(SHIPPED) + " 260 rows", m, sd64, cfg, enc, 12, 5, SHIPPED[0], cap=int(0.10 * 52))


@pytest.mark.parametrize("k", [5, 2])
def test_long_search_every_beam_live(k):
    """Output weights at 8 / sqrt(H) and no END clock (build's "flat" variant: seed 100 + 512 // 64 + 34): most searches
    run all 60 steps with every beam live, i.e. 60 gathers through two layers and both c buffers 30 times each."""
    m, sd64, cfg = build(SHIPPED, "flat")
    enc = enc_for(SHIPPED, 4, seed=13)
    check_vs_float64(sid(SHIPPED, "flat"), m, sd64, cfg, enc, 60, k, SHIPPED[0], cap=1)


# ------------------------------------------------------------------------------------------------ 3. the reference's fixtures
FIXTURES = ["tiny_l1", "tiny_l2_attn", "odd_dims", "odd_hidden", "secondary", "shipped_128x800", "primary"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_beam_search_under_the_flag(name):
    d, cfg, _ = load(name)
    m, _ = model_for(name)
    bimgs = images(cfg, 8, seed=4321, device=DEV)
    sd64 = None
    with torch.no_grad():
        enc = m.encoder(bimgs)
        for k in (5, 3):
            want = padded_to_lists(d[f"g4_k{k}_ids"], d[f"g4_k{k}_len"])
            got, scores = m.beam_search_batch(enc, START, END, 40, k, return_scores=True, flags=FLAG)
            assert all(np.isfinite(s) and s <= 0.0 for s in scores)
            moved = 0
            for j in range(8):
                if got[j] == want[j]:
                    continue
                if sd64 is None:
                    sd64 = {n: torch.from_numpy(v).to(DEV, torch.float64) for n, v in np_state_dict(name).items()
                            if n.startswith("decoder.")}
                st = {}
                O.beam_search(sd64, cfg, enc[j:j + 1].double(), START, END, 40, k, stats=st)
                assert st["gap"] < GAP, (name, k, j, st["gap"], got[j], want[j])
                moved += 1
            record(f"batched {name} beam k={k}: fixture images moved at a near-tie", moved)
            assert moved <= 1, (name, k, moved)
            if k == 5:
                batch5 = got
        m.decoder.kernel_flags |= FLAG
        try:
            one = m.inference(bimgs[2:3], START, END, max_length=40, beam_size=5)   # the reference's entry point
        finally:
            m.decoder.kernel_flags &= ~FLAG
    assert m.decoder.kernel_flags == 0
    assert one == batch5[2]


# ------------------------------------------------------------------------------------------------ 4. BASELINE configs[2] at its size
@pytest.mark.parametrize("fname", ["primary_cfg3_beam", "primary_cfg3_beam_noend"])
def test_cfg3_beam_full_size_vs_reference(fname):
    """test_hip_parity.test_cfg3_beam_full_size_vs_reference under the flag: 128 (32) images x k = 5 x 150 steps against
    the reference itself; tokens exact wherever the fixture's smallest gap is >= 1e-4, scores within 1e-4 relative."""
    d, cfg, sd_kw = load(fname)
    m, _ = model_for(fname, sd_kw, cfg)
    n, k, T = len(d["lens"]), int(d["k"]), int(d["max_length"])
    x = torch.from_numpy(synth.make_images(n, cfg, seed=int(d["image_seed"]))).to(DEV)
    with torch.no_grad():
        enc = m.encoder(x)
        got, scores = m.beam_search_batch(enc, START, END, T, k, return_scores=True, flags=FLAG)
    want = padded_to_lists(d["ids"].astype(np.int64), d["lens"])
    off, worst = [], 0.0
    for j in range(n):
        if got[j] != want[j]:
            assert d["min_gap"][j] < 1e-4, (fname, j, float(d["min_gap"][j]))
            off.append(j)
            continue
        err = abs(scores[j] - float(d["scores"][j])) / max(1.0, abs(float(d["scores"][j])))
        worst = max(worst, err)
        assert err <= 1e-4, (fname, j, scores[j], float(d["scores"][j]))
    record(f"batched {fname} {n} images x k={k} x {T} steps: images whose tokens leave the reference's at a near-tie "
           f"(of {int((d['min_gap'] < 1e-4).sum())} below the guard)", len(off))
    record(f"batched {fname} winning scores vs the reference [rel to max(1,|score|)]", worst)
    assert len(off) <= 0.05 * n, off


# ------------------------------------------------------------------------------------------------ 5. flag off is the parent
def _direct_beam_decode(m, enc, steps, k, flags=0):
    """i2l_beam_decode called as the parent's beam_search_batch calls it."""
    dec = m.decoder
    w, keep, enc_c = dec.prepare(enc)
    n = enc_c.shape[0]
    L = _lib.lib()
    nbytes = L.i2l_beam_workspace_bytes(n, k, dec.hidden_dim, dec.lstm_layers, steps)
    bws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    seq = torch.empty((n, steps + 1), dtype=torch.int32, device=DEV)
    ln = torch.empty((n,), dtype=torch.int32, device=DEV)
    score = torch.empty((n,), dtype=torch.float64, device=DEV)
    _lib.check(L.i2l_beam_decode(ctypes.byref(w), dec._ws.data_ptr(), n, k, steps, START, END, bws.data_ptr(), nbytes,
                                 seq.data_ptr(), ln.data_ptr(), score.data_ptr(), flags, _lib.stream_ptr()), "beam_decode")
    torch.cuda.synchronize()
    del keep
    lens = ln.cpu().tolist()
    return [row[:n_j] for row, n_j in zip(seq.cpu().tolist(), lens)], score.cpu().tolist()


@pytest.mark.parametrize("which", ["shipped", "primary"])
def test_flag_off_is_the_parent_call(which):
    if which == "shipped":
        m, _, _ = build(SHIPPED)
        enc = enc_for(SHIPPED, 5, seed=13)
    else:
        _, cfg, _ = load("primary")
        m, _ = model_for("primary")
        with torch.no_grad():
            enc = m.encoder(images(cfg, 5, seed=4321, device=DEV))
    assert m.decoder.kernel_flags == 0
    with torch.no_grad():
        via = m.beam_search_batch(enc, START, END, 24, 3, return_scores=True)
        direct = _direct_beam_decode(m, enc, 24, 3)
        greedy_flag = m.beam_search_batch(enc, START, END, 24, 3, return_scores=True, flags=_lib.FLAG_DECODE_BATCHED)
    assert via == direct
    assert greedy_flag == via
    assert m.decoder.kernel_flags == 0


# ------------------------------------------------------------------------------------------------ 6. degenerate and edge behaviour
def _raw(m, enc, steps, k, start=START, end=END):
    """The C entry itself: seq_out (n, steps + 1), len_out and score_out as the call left them."""
    dec = m.decoder
    w, keep, enc_c = dec.prepare(enc)
    n = enc_c.shape[0]
    L = _lib.lib()
    nbytes = L.i2l_beam_batched_scratch_bytes(n, k, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, steps)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    seq = torch.full((n, steps + 1), -7, dtype=torch.int32, device=DEV)
    ln = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    score = torch.full((n,), 1.0, dtype=torch.float64, device=DEV)
    _lib.check(L.i2l_beam_decode_batched(ctypes.byref(w), dec._ws.data_ptr(), n, k, steps, start, end, scratch.data_ptr(),
                                         nbytes, seq.data_ptr(), ln.data_ptr(), score.data_ptr(), 0, _lib.stream_ptr()),
               "beam_decode_batched")
    torch.cuda.synchronize()
    del keep
    return seq.cpu().numpy(), ln.cpu().numpy(), score.cpu().numpy()


def test_degenerate_and_edge_behaviour():
    m, sd64, cfg = build(SHIPPED)
    V = SHIPPED[0]
    enc = enc_for(SHIPPED, 3, seed=13)
    with torch.no_grad():
        # START == END: the one beam retires before the first step
        assert m.beam_search_batch(enc, START, START, 5, 3, flags=FLAG) == [[], [], []]
        seq, ln, sc = _raw(m, enc, 5, 3, START, START)
        assert (ln == 0).all() and (seq == -1).all() and (sc == 0.0).all()
        # k = 1, one image, one step
        for steps, n in ((24, 3), (1, 3), (24, 1), (1, 1)):
            for k in (1, 3):
                got, scores = m.beam_search_batch(enc[:n], START, END, steps, k, return_scores=True, flags=FLAG)
                assert len(got) == n
                for j in range(n):
                    st = {}
                    want, wsc = O.beam_search(sd64, cfg, enc[j:j + 1].double(), START, END, steps, k, return_score=True, stats=st)
                    assert got[j] == want or (k > 1 and st["gap"] < GAP), (steps, n, k, j, got[j], want)
                    assert len(got[j]) <= steps and all(0 <= t < V for t in got[j])
                    assert np.isfinite(scores[j]) and scores[j] <= 0.0
                    if got[j] == want:
                        assert abs(scores[j] - wsc) <= 1e-4 * max(1.0, abs(wsc))
        # a search that ends early (the END clock fires well before step 40) leaves -1 behind len_out
        seq, ln, sc = _raw(m, enc, 40, 3)
        assert (ln >= 0).all() and (ln < 40).all(), ln
        for j in range(3):
            assert (seq[j, :ln[j]] >= 0).all() and (seq[j, :ln[j]] < V).all() and END not in seq[j, :ln[j]]
            assert (seq[j, ln[j]:] == -1).all(), (j, seq[j])
        assert np.isfinite(sc).all() and (sc <= 0.0).all()
    assert m.decoder.kernel_flags == 0
