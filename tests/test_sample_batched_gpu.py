"""Step-batched top-k / top-p sampling (i2l_sample_decode_batched, i2l_sample_logits; _lib.FLAG_DECODE_BATCHED on
LSTMDecoder.sample_steps): the rule in isolation against a float64 restatement, the loop through helpers.check_sampling,
state and sticky stop, agreement with the row kernel, and the Predictor path.  Bounds are the suite's: probabilities 1e-5,
h / c 1e-5 relative to max(1,|ref|); a mask or a draw is judged unless float64 itself puts it within 1e-5 of flipping."""
import ctypes

import numpy as np
import pytest
import torch

import img2latex_oracle as O
from conftest import record
from helpers import END, START, check_sampling, close, images, load, model_for, uniform01
from img2latex_amd import _lib
from img2latex_amd.model import LSTMDecoder
from test_decoder_shapes import build, enc_for, oracle_steps, sid

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAG = _lib.FLAG_DECODE_BATCHED
SHIPPED = (500, 512, 512, 2, True)
GUARD = 1e-5
SEED = 20240


# ------------------------------------------------------------------------------------------------ the rule in float64
def rule64(x, temp, top_k, top_p):
    """One row of the rule in float64, the kernel's steps in the kernel's order.  x: (V,) float32 logits.  Returns the final
    distribution and the mask margin: the smallest relative gap between the k-th value and the value below it, and the
    smallest distance of a sorted-ahead mass to top_p."""
    a = x.astype(np.float64) / temp
    e = np.exp(a - a.max())
    p = e / e.sum()
    V = p.size
    margin = np.inf
    if top_k > 0:
        srt = np.sort(p)[::-1]
        kth = srt[min(top_k, V) - 1]
        below = p[p < kth]
        if below.size and kth > 0:
            margin = min(margin, (kth - below.max()) / kth)
        p = np.where(p < kth, 0.0, p)
        if p.sum() > 0:
            p = p / p.sum()
    if top_p > 0:
        order = np.argsort(-p, kind="stable")            # descending, the lower index first among equal values
        sp = p[order]
        before = np.cumsum(sp) - sp                      # mass sorted strictly ahead
        drop = before > top_p
        drop[0] = False
        live = sp[1:] > 0
        if live.any():
            margin = min(margin, float(np.abs(before[1:][live] - top_p).min()))
        p = p.copy()
        p[order[drop]] = 0.0
        p = p / p.sum()
    return p, margin


def draw64(q, u):
    """Inverse CDF over index order at u * total: (pick, distance of the target to the nearest CDF step around it)."""
    cdf = np.cumsum(q)
    target = float(u) * cdf[-1]
    j = int(np.searchsorted(cdf, target, side="right"))
    j = min(j, q.size - 1)
    lo = cdf[j - 1] if j > 0 else 0.0
    return j, min(abs(target - lo), abs(cdf[j] - target))


def run_rule(x, V, temp, top_k, top_p, step, seed=SEED):
    """sample_logits over the first V columns of x (rows, ld) on the device -> (ids, probs) on the host."""
    xd = torch.from_numpy(x).to(DEV)
    ids, probs = LSTMDecoder.sample_logits(xd[:, :V], temp, top_k, top_p, seed, step=step, want_probs=True)
    return ids.cpu().numpy(), probs.cpu().numpy()


VOCABS = [1, 3, 64, 65, 500, 1000, 2048]
PARAMS = [(1.0, 5, 0.0), (0.7, 0, 0.9), (1.3, 40, 0.95), (1.0, 1, 0.0), (1.0, 0, 0.05), (1.0, 3000, 0.0), (2.0, 0, 1.5)]
_LEFT_OUT = {}


@pytest.mark.parametrize("V", VOCABS)
def test_rule_vs_float64(V):
    """N(0, 3^2) logits; rows 1, 5, 33; ld = V and V + 7 with the padding at +1e30 (a read past V would take all the
    mass).  Per row: probabilities within 1e-5, the kept set and the pick equal to float64's."""
    rng = np.random.default_rng(1000 + V)
    cases = masks_out = draws_out = 0
    step = 0
    for rows in (1, 5, 33):
        base = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
        for pad in (0, 7):
            x = np.full((rows, V + pad), 1e30, dtype=np.float32)
            x[:, :V] = base
            for temp, top_k, top_p in PARAMS:
                step += 1
                tag = f"V={V} rows={rows} ld=V+{pad} T={temp} k={top_k} p={top_p}"
                ids, probs = run_rule(x, V, temp, top_k, top_p, step)
                assert probs.shape == (rows, V) and ids.shape == (rows,)
                assert np.isfinite(probs).all() and ids.min() >= 0 and ids.max() < V, tag
                for r in range(rows):
                    cases += 1
                    want, margin = rule64(base[r], temp, top_k, top_p)
                    if margin < GUARD:
                        masks_out += 1
                        continue
                    assert np.abs(probs[r] - want).max() <= 1e-5, (tag, r, float(np.abs(probs[r] - want).max()))
                    assert np.array_equal(probs[r] > 0, want > 0), (tag, r, "kept set")
                    pick, dist = draw64(want, uniform01(SEED, r, step))
                    if dist < GUARD:
                        draws_out += 1
                        continue
                    assert ids[r] == pick, (tag, r, int(ids[r]), pick)
    record(f"sample_logits V={V}: rows judged", cases)
    record(f"sample_logits V={V}: masks left out at a float64 margin below 1e-5", masks_out)
    record(f"sample_logits V={V}: draws left out within 1e-5 of a CDF step", draws_out)
    _LEFT_OUT[V] = (cases, masks_out + draws_out)      # capped over all vocabularies by the test below


def test_rule_vs_float64_leaves_out_at_most_two_percent():
    """Over all vocabularies of test_rule_vs_float64 (run here for those a selection skipped)."""
    for V in VOCABS:
        if V not in _LEFT_OUT:
            test_rule_vs_float64(V)
    cases = sum(c for c, _ in _LEFT_OUT.values())
    out = sum(o for _, o in _LEFT_OUT.values())
    record("sample_logits: rows left out of all rows", out / cases)
    assert out <= 0.02 * cases, (cases, out)


def test_rule_exact_ties():
    """Hand-written rows, no guard: a tie with the k-th value stays whole, top-p orders equal values by index."""
    # all logits equal (1 / 64 and 1 / 1024 and their sums are exact): top_k = 3 keeps all, top_p = 0.5 the lowest indices
    for V in (64, 1024):
        x = np.full((2, V), 0.25, dtype=np.float32)
        _, probs = run_rule(x, V, 1.0, 3, 0.0, 0)
        assert np.array_equal(probs, np.full((2, V), 1.0 / V, dtype=np.float32)), V
        ids, probs = run_rule(x, V, 1.0, 0, 0.5, 0)
        keep = V // 2 + 1                         # mass ahead of column i is i / V: dropped iff i / V > 0.5
        assert (probs[:, :keep] > 0).all() and (probs[:, keep:] == 0).all(), V
        assert np.abs(probs[:, :keep] - 1.0 / keep).max() <= 1e-6 and (ids < keep).all(), V
    _, probs = run_rule(np.full((1, 500), -3.0, dtype=np.float32), 500, 0.7, 3, 0.0, 0)
    assert (probs > 0).all()
    # a tie group across the k-th place: 5 > 3 = 3 = 3 = 3 > the rest, top_k = 3 keeps five columns
    x = np.full((1, 65), -2.0, dtype=np.float32)
    x[0, [60, 2, 17, 40, 64]] = [5.0, 3.0, 3.0, 3.0, 3.0]
    _, probs = run_rule(x, 65, 1.0, 3, 0.0, 1)
    assert sorted(np.nonzero(probs[0])[0].tolist()) == [2, 17, 40, 60, 64]
    assert probs[0, 2] == probs[0, 17] == probs[0, 40] == probs[0, 64]
    # two equal maxima, a small top_p: the lower index only
    x = np.zeros((3, 65), dtype=np.float32)
    x[:, 7] = x[:, 3] = 10.0
    ids, probs = run_rule(x, 65, 1.0, 0, 0.05, 2)
    assert (ids == 3).all() and (probs[:, 3] == 1.0).all() and (np.delete(probs, 3, axis=1) == 0).all()
    # one +80 among -80s: a single token under either mask
    x = np.full((2, 500), -80.0, dtype=np.float32)
    x[:, 123] = 80.0
    for top_k, top_p in ((5, 0.0), (0, 0.9), (5, 0.9)):
        ids, probs = run_rule(x, 500, 1.0, top_k, top_p, 3)
        assert (ids == 123).all() and (probs[:, 123] == 1.0).all() and np.count_nonzero(probs) == 2


def test_rule_is_bitwise_reproducible():
    rng = np.random.default_rng(77)
    x = (3.0 * rng.standard_normal((33, 2048))).astype(np.float32)
    for V, temp, top_k, top_p in ((2048, 1.3, 40, 0.95), (500, 0.7, 0, 0.9), (1000, 1.0, 5, 0.0)):
        a = run_rule(x, V, temp, top_k, top_p, 4)
        b = run_rule(x, V, temp, top_k, top_p, 4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. the loop
LOOP_SHAPES = [(3, 4, 64, 1, False), (513, 256, 256, 1, False), (777, 36, 192, 3, True), (2048, 64, 128, 2, True), SHIPPED]


def loop_model(shape):
    """"flat" weights at V > 3.  At V = 3 the weights of the default seed leave one token under (top_k = V, top_p = 0.5), so
    that two seeds draw the same ids and check_sampling's "a different seed draws different tokens" cannot hold at any
    kernel; weight seed 12 was picked on the float64 oracle alone (the rule and the draws replayed on the host for rows
    1, 5 and 33 and the five parameter pairs): two seeds differ there in every case."""
    return build(shape, "flat") if shape[0] > 3 else build(shape, None, seed=12)


@pytest.mark.parametrize("rows", [1, 5, 33])
@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=[sid(s) for s in LOOP_SHAPES])
def test_loop_vs_float64(shape, rows):
    """helpers.check_sampling, unchanged, with the decoder's kernel_flags sending sample_steps to the batched entry."""
    m, sd64, cfg = loop_model(shape)
    V = shape[0]
    enc = enc_for(shape, rows, seed=41)
    e64 = enc.double()

    def step(tok, hidden):
        return O.decode_step(sd64, cfg, e64, tok.to(DEV), hidden)

    assert m.decoder.kernel_flags == 0
    m.decoder.kernel_flags |= FLAG
    try:
        for top_k, top_p in ((1, 0.5), (7, 0.95), (V, 0.5), (0, 0.9), (5, 0.0)):
            check_sampling(m.decoder, enc, step, top_k, top_p, 1.0, seed=2024 + top_k, steps=6,
                           what=f"batched {sid(shape)} rows={rows} sampling top_k={top_k} top_p={top_p} probabilities")
    finally:
        m.decoder.kernel_flags &= ~FLAG
    assert m.decoder.kernel_flags == 0


# ------------------------------------------------------------------------------------------------ 3. state, sticky stop
def test_state_vs_float64_replay():
    m, sd64, cfg = build(SHIPPED, "flat")
    rows, steps = 5, 6
    enc = enc_for(SHIPPED, rows, seed=41)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    out = m.decoder.sample_steps(enc, steps, tok0, 1.0, 5, 0.9, 11, stop=_lib.STOP_NONE, flags=FLAG, want_state=True)
    assert len(out) == 3 and out[1] is None
    ids, _, (h, c) = out
    toks = torch.cat([tok0[:, None].long(), ids[:, :-1].long()], 1)
    _, (rh, rc) = oracle_steps(sd64, cfg, enc, toks)
    close(h.cpu().numpy(), rh.cpu().numpy(), 1e-5, "batched sampling: h after 6 sampled steps")
    close(c.cpu().numpy(), rc.cpu().numpy(), 1e-5, "batched sampling: c after 6 sampled steps")
    two = m.decoder.sample_steps(enc, steps, tok0, 1.0, 5, 0.9, 11, stop=_lib.STOP_NONE, flags=FLAG)
    assert len(two) == 2 and torch.equal(two[0], ids)


def test_sticky_stop():
    rows, steps = 5, 12
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    m, _, _ = build(SHIPPED, "flat")
    enc = enc_for(SHIPPED, rows, seed=41)
    free, _ = m.decoder.sample_steps(enc, steps, tok0, 1.0, 5, 0.9, 11, stop=_lib.STOP_NONE, flags=FLAG)
    free = free.cpu().numpy()
    end_id = int(free[2, 1])                     # row 2 draws it at its second step at the latest
    sticky, _ = m.decoder.sample_steps(enc, steps, tok0, 1.0, 5, 0.9, 11, stop=_lib.STOP_STICKY, end_id=end_id, flags=FLAG)
    sticky = sticky.cpu().numpy()
    for b in range(rows):
        ends = np.nonzero(free[b] == end_id)[0]
        n = int(ends[0]) + 1 if ends.size else steps
        assert np.array_equal(sticky[b, :n], free[b, :n]) and (sticky[b, n:] == -1).all(), b
    assert (sticky[2, 2:] == -1).all() and end_id in sticky[2, :2]
    # every row ends: top-1 sampling is the greedy loop, whose END clock ends each row well before step 40
    m, _, _ = build(SHIPPED)
    enc = enc_for(SHIPPED, rows, seed=9)
    steps = 40
    free, _ = m.decoder.sample_steps(enc, steps, tok0, 1.0, 1, 0.5, 11, stop=_lib.STOP_NONE, flags=FLAG)
    sticky, _ = m.decoder.sample_steps(enc, steps, tok0, 1.0, 1, 0.5, 11, stop=_lib.STOP_STICKY, end_id=END, flags=FLAG)
    free, sticky = free.cpu().numpy(), sticky.cpu().numpy()
    last = 0
    for b in range(rows):
        ends = np.nonzero(free[b] == END)[0]
        assert ends.size, b
        n = int(ends[0]) + 1
        last = max(last, n)
        assert np.array_equal(sticky[b, :n], free[b, :n]) and (sticky[b, n:] == -1).all(), b
    assert last < steps and (sticky[:, last:] == -1).all()


# ------------------------------------------------------------------------------------------------ 4. the row kernel
@pytest.mark.parametrize("shape", [SHIPPED, (513, 256, 256, 1, False)], ids=[sid(SHIPPED), sid((513, 256, 256, 1, False))])
def test_ids_agree_with_the_row_kernel(shape):
    """Same seed, same uniforms: the two kernels' logits differ in the last bits, so a row may leave only at a near-tie."""
    m, _, _ = build(shape, "flat")
    rows, steps = 33, 6
    enc = enc_for(shape, rows, seed=41)
    tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
    row, _ = m.decoder.sample_steps(enc, steps, tok0, 1.0, 5, 0.9, 31, stop=_lib.STOP_NONE)
    bat, _ = m.decoder.sample_steps(enc, steps, tok0, 1.0, 5, 0.9, 31, stop=_lib.STOP_NONE, flags=FLAG)
    same = int((row == bat).all(dim=1).sum())
    record(f"batched {sid(shape)} sampling: rows of 33 with the row kernel's ids", same)
    assert same >= 30, same


# ------------------------------------------------------------------------------------------------ 5. the public path
def test_predictor_samples_on_the_batched_path():
    from img2latex_amd.training import Predictor, TokenTable
    name = "shipped_128x800"
    _, cfg, _ = load(name)
    m, _ = model_for(name)
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, cfg["vocab_size"])})
    table = TokenTable(vocab, max_sequence_length=150)
    x = images(cfg, device=DEV)
    dec = m.decoder
    seen = []
    inner = dec.sample_steps

    def spy(*a, **kw):
        seen.append(int(kw.get("flags", 0)))
        return inner(*a, **kw)

    def cut(ids):
        a = ids.cpu().numpy()
        stop = (a == END) | (a < 0)
        lens = np.where(stop.any(axis=1), stop.argmax(axis=1), a.shape[1]).tolist()
        return [[START] + row[:n] for row, n in zip(a.tolist(), lens)]

    old = getattr(m.encoder, "eval_precision", None)
    if old is not None:
        m.encoder.eval_precision = "fp32"
    dec.sample_steps = spy
    try:
        off = Predictor(m, table, device=torch.device(DEV))
        on = Predictor(m, table, device=torch.device(DEV), decode_flags=FLAG)
        got_on = on.predict_batch_ids(x, max_length=32, top_k=5, seed=3)
        got_off = off.predict_batch_ids(x, max_length=32, top_k=5, seed=3)
        assert seen == [FLAG, 0]
        with torch.no_grad():
            enc = m.encoder(x)
        tok0 = torch.full((enc.shape[0],), START, dtype=torch.int32, device=DEV)
        want_on, _ = inner(enc, 32, tok0, 1.0, 5, 0.0, 3, stop=_lib.STOP_STICKY, end_id=END, flags=FLAG)
        assert got_on == cut(want_on)
        # the default predictor still takes i2l_sample_decode: its ids are that entry's, called directly
        w, keep, enc_c = dec.prepare(enc)
        direct = torch.empty((enc.shape[0], 32), dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib().i2l_sample_decode(ctypes.byref(w), dec._ws.data_ptr(), enc.shape[0], 32, tok0.data_ptr(), None,
                                                None, 1.0, 5, 0.0, 3, _lib.STOP_STICKY, END, direct.data_ptr(), None, None,
                                                None, _lib.stream_ptr()), "sample_decode")
        torch.cuda.synchronize()
        del keep
        assert got_off == cut(direct)
    finally:
        del dec.sample_steps
        if old is not None:
            m.encoder.eval_precision = old
    assert dec.kernel_flags == 0
