"""The consensus decode on the device: i2l_sample_rank on crafted ids against the Python restatement
(sample_rank_ref.py), and i2l_sample_decode_multi (Seq2SeqModel.sample_multi_device / sample_nbest) -- its draws, scores
and ranking against the float64 oracle decoder on the replicated encoder rows -- up to Predictor.predict_samples.

The draws are judged by helpers.check_sampling's rule: the float64 distribution rebuilt along the device's own tokens
(test_sample_batched_gpu.rule64), the inverse CDF at the kernel's documented uniform (draw64), a mask or a draw within
1e-5 of a float64 boundary left out and at most 2 % of them left out, the suite's cap.  check_sampling itself reads the
device's distributions and runs without a stop rule; this entry returns ids under the sticky stop and no
distributions, so its rule is applied to the oracle's distribution directly.  Scores: 1e-4 relative to max(1, |ref|),
the bound test_beam_nbest_gpu.py holds beam scores to.  Integers -- len, finished, risk, dist, order -- are exact, and
so is the key.

Which test launches which sample_distance_kernel<W>: test_rank_on_crafted_ids W = 1, 2, 3 (steps 1, 7, 65, 130), the decode
tests W = 1 (12 and 20 steps), test_distance_block_boundaries W = 1, 2, 3, 4, 8, 16 (steps 64 .. 1024)."""
import numpy as np
import pytest
import torch

import sample_rank_ref as R
import test_sample_rank_host as H
from conftest import record
from helpers import END, START, uniform01
from img2latex_amd import _lib
from img2latex_amd.training.constraint import BracketTable
from test_arguments_decode_gpu import PNG, argument_checkpoint, complete, loop_model, loop_table, nests   # noqa: F401
from test_arguments_decode_gpu import SHIPPED as ARG_SHIPPED
from test_arguments_decode_gpu import SMALL as ARG_SMALL
from test_decoder_shapes import build, enc_for, oracle_steps, sid
from test_sample_batched_gpu import GUARD, draw64, rule64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHIPPED = (500, 512, 512, 2, True)
TINY = (3, 4, 64, 1, False)
ODD = (777, 36, 192, 3, True)
STEPS = 12
TOP_K, TOP_P = 5, 0.9


# ------------------------------------------------------------------------------------------------ i2l_sample_rank
def device_rank(ids, score, rank, norm=None, want_dist=True):
    """ids (n, S, T) int32, score (n, S) float64 on the host -> the entry's outputs as numpy arrays."""
    n, S, T = ids.shape
    d_ids, d_score = torch.from_numpy(np.ascontiguousarray(ids)).to(DEV), torch.from_numpy(np.ascontiguousarray(score)).to(DEV)
    d_norm = None if norm is None else torch.tensor(norm, dtype=torch.float64, device=DEV)
    ln, fin, risk, order = (torch.full((n, S), -7, dtype=torch.int32, device=DEV) for _ in range(4))
    key = torch.full((n, S), float("nan"), dtype=torch.float64, device=DEV)
    dist = torch.full((n, S, S), -7, dtype=torch.int32, device=DEV) if want_dist else None
    _lib.check(_lib.lib().i2l_sample_rank(d_ids.data_ptr(), n, S, T, H.END, d_score.data_ptr(), rank, _lib.ptr(d_norm),
                                          ln.data_ptr(), fin.data_ptr(), risk.data_ptr(), key.data_ptr(), order.data_ptr(),
                                          _lib.ptr(dist), _lib.stream_ptr()), "sample_rank")
    torch.cuda.synchronize()
    out = dict(len=ln, finished=fin, risk=risk, key=key, order=order)
    if want_dist:
        out["dist"] = dist
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_ranked(got, ids, score, rank, norm, end_id, where):
    want = R.rank_images(ids, end_id, score, rank, norm)
    for name in ("len", "finished", "risk", "order") + (("dist",) if "dist" in got else ()):
        assert np.array_equal(got[name], want[name]), (where, name, got[name].tolist(), want[name].tolist())
    assert got["key"].astype(np.float64).tobytes() == want["key"].astype(np.float64).tobytes(), (where, "key")


@pytest.mark.parametrize("steps", [1, 7, 65, 130])
@pytest.mark.parametrize("samples", [1, 2, 5, 16])
def test_rank_on_crafted_ids(samples, steps):
    """Three images a call, every crafted kind of the host test (no END, END at step 0, all samples equal, risk ties
    broken by the score, score ties by the index, every length), both ranks with and without a norm table."""
    rng = np.random.default_rng(1000 * samples + steps)
    kinds = list(H.image_kinds(rng, samples, steps).items())
    kinds += kinds[:(-len(kinds)) % 3]
    for at in range(0, len(kinds), 3):
        names = [k for k, _ in kinds[at:at + 3]]
        ids = np.stack([v[0] for _, v in kinds[at:at + 3]]).astype(np.int32)
        score = np.stack([v[1] for _, v in kinds[at:at + 3]]).astype(np.float64)
        for rank in (R.CONSENSUS, R.LOGPROB):
            for norm in (None, H.norm_table(steps)):
                got = device_rank(ids, score, rank, norm, want_dist=rank == R.CONSENSUS)
                assert_ranked(got, ids, score, rank, norm, H.END, (names, samples, steps, rank, norm is not None))


def rank_all_ways(ids, score, where):
    """Both ranks, with and without a norm table; the consensus calls also return dist, held to be symmetric with a zero
    diagonal (each d(i, j) and d(j, i) is a wave's own walk, with the two rows in exchanged roles)."""
    steps = ids.shape[2]
    for rank in (R.CONSENSUS, R.LOGPROB):
        for norm in (None, H.norm_table(steps)):
            got = device_rank(ids, score, rank, norm, want_dist=rank == R.CONSENSUS)
            assert_ranked(got, ids, score, rank, norm, H.END, where + (rank, norm is not None))
            if "dist" in got:
                d = got["dist"]
                assert np.array_equal(d, d.transpose(0, 2, 1)) and (np.diagonal(d, axis1=1, axis2=2) == 0).all(), where


# rows of the first, second and third image for the calls of two samples: the pair equal but for its last token at
# R = steps (bit (R - 1) & 63 of the last block), R = 128 beside a row without END, the empty row beside a shifted one
PAIRS = ((10, 11), (8, 2), (12, 4))


@pytest.mark.parametrize("steps", H.BOUNDARY_STEPS)
def test_distance_block_boundaries(steps):
    """sample_distance_kernel<W> at W = 1, 2, 3, 4, 4, 8, 8, 16, 16, 16 in a block of 16 waves, and at steps 256 and 1024
    (W = 4, 16) in blocks of one and two: test_sample_rank_host.boundary_images -- cut lengths on and around every
    64-token block boundary, identical, disjoint, shifted and last-token pairs, alphabets of 2, 5 and 400 tokens with
    the padding's token 0 among them, random tokens and further ENDs behind the END -- exactly as the restatement, whose
    numpy distance the host test holds to the plain table at these sizes."""
    made = H.boundary_images(steps)
    ids = np.stack([m[0] for m in made]).astype(np.int32)
    score = H.boundary_scores(steps)
    assert ids.shape == (3, 16, steps)
    rank_all_ways(ids, score, ("boundaries", steps, 16))
    if steps in (256, 1024):
        one = np.stack([ids[k, [14]] for k in range(3)])
        rank_all_ways(one, score[:, [14]], ("boundaries", steps, 1))
        two = np.stack([ids[k, list(PAIRS[k])] for k in range(3)])
        rank_all_ways(two, np.stack([score[k, list(PAIRS[k])] for k in range(3)]), ("boundaries", steps, 2))


@pytest.mark.parametrize("what,samples,steps,code", [("steps 1025", 16, 1025, _lib.ERR_UNSUPPORTED),
                                                     ("samples 17", 17, 64, _lib.ERR_UNSUPPORTED),
                                                     ("samples 0", 0, 64, _lib.ERR_ARG)])
def test_rank_refuses_without_a_launch(what, samples, steps, code):
    """check_rank_dims' codes on live device buffers: nothing is launched, so the outputs keep what they held."""
    S = max(samples, 1)
    ids = torch.zeros((2, S, steps), dtype=torch.int32, device=DEV)
    score = torch.zeros((2, S), dtype=torch.float64, device=DEV)
    outs = [torch.full((2, S), -7, dtype=torch.int32, device=DEV) for _ in range(4)]
    key = torch.full((2, S), -7.0, dtype=torch.float64, device=DEV)
    dist = torch.full((2, S, S), -7, dtype=torch.int32, device=DEV)
    for rank in (R.CONSENSUS, R.LOGPROB):
        rc = _lib.lib().i2l_sample_rank(ids.data_ptr(), 2, samples, steps, H.END, score.data_ptr(), rank, None,
                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), key.data_ptr(),
                                        outs[3].data_ptr(), dist.data_ptr(), _lib.stream_ptr())
        assert rc == code, (what, rc)
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs + [key, dist]), what


# ------------------------------------------------------------------------------------------------ i2l_sample_decode_multi
def model_of(shape):
    """test_sample_batched_gpu.loop_model's choice: "flat" weights above V = 3, weight seed 12 at V = 3."""
    return build(shape, "flat") if shape[0] > 3 else build(shape, None, seed=12)


def multi(m, enc, samples, steps=STEPS, seed=77, temperature=1.0, top_k=TOP_K, top_p=TOP_P, **kw):
    with torch.no_grad():
        out = m.sample_multi_device(enc, START, END, steps, samples, temperature, top_k, top_p, seed, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shape", [ODD, (513, 256, 256, 1, False)], ids=sid)
def test_one_sample_is_the_batched_call(shape):
    """samples = 1: the same row count and the same launches as i2l_sample_decode_batched under the sticky stop."""
    m, _, _ = model_of(shape)
    enc = enc_for(shape, 5, seed=41)
    tok0 = torch.full((5,), START, dtype=torch.int32, device=DEV)
    want, _ = m.decoder.sample_steps(enc, STEPS, tok0, 1.0, TOP_K, TOP_P, 77, stop=_lib.STOP_STICKY, end_id=END,
                                     flags=_lib.FLAG_DECODE_BATCHED)
    got = multi(m, enc, 1)
    assert got["ids"].shape == (5, 1, STEPS) and np.array_equal(got["ids"][:, 0], want.cpu().numpy())
    assert (got["order"] == 0).all() and (got["risk"] == 0).all()


def replay64(sd64, cfg, enc, ids, samples):
    """float64 logits (rows, steps, V) of the oracle decoder fed the device's own tokens, row i * samples + s on encoder
    row i; behind END (ids -1) the row is fed END and its logits are not looked at."""
    flat = ids.reshape(-1, ids.shape[-1])
    toks = np.concatenate([np.full((flat.shape[0], 1), START), np.where(flat[:, :-1] < 0, END, flat[:, :-1])], axis=1)
    logits, _ = oracle_steps(sd64, cfg, enc.repeat_interleave(samples, 0), torch.from_numpy(toks).to(DEV))
    return logits.cpu().numpy()


def judge_draws(logits, flat, seed, temperature, top_k, top_p, where):
    judged = left_out = 0
    for r in range(flat.shape[0]):
        for t in range(flat.shape[1]):
            if flat[r, t] < 0:
                assert t > 0 and (flat[r, t:] == -1).all() and flat[r, t - 1] in (END, -1), (where, r, t)
                break
            judged += 1
            p, margin = rule64(logits[r, t], temperature, top_k, top_p)
            pick, dist = draw64(p, uniform01(seed, r, t))
            if margin < GUARD or dist < GUARD:
                left_out += 1
                continue
            assert flat[r, t] == pick, (where, r, t, int(flat[r, t]), pick)
    return judged, left_out


def check_samples(shape, images, samples, seed, temperature=1.0):
    """The draws by judge_draws' rule at ``temperature``; the scores against the float64 log-probabilities of the RAW logits
    (no temperature, no truncation: sample_batched_kernel's documented score); both rankings exactly."""
    m, sd64, cfg = model_of(shape)
    enc = enc_for(shape, images, seed=43)
    got = multi(m, enc, samples, seed=seed, temperature=temperature)
    ids, flat = got["ids"], got["ids"].reshape(images * samples, STEPS)
    assert ids.shape == (images, samples, STEPS) and flat.max() < shape[0]
    logits = replay64(sd64, cfg, enc, ids, samples)
    tag = f"sample_decode_multi {sid(shape)} {images}x{samples}" + (f" T={temperature}" if temperature != 1.0 else "")
    judged, left_out = judge_draws(logits, flat, seed, temperature, TOP_K, TOP_P, tag)
    record(f"{tag}: draws judged", judged)
    record(f"{tag}: draws left out within 1e-5 of a float64 boundary", left_out)
    assert left_out <= 0.02 * judged, (judged, left_out)
    assert any(len({tuple(row) for row in ids[i].tolist()}) > 1 for i in range(images)), "the samples of every image are equal"
    want = R.sequence_scores(logits, flat, END)
    err = np.abs(got["score"].reshape(-1) - want) / np.maximum(1.0, np.abs(want))
    record(f"{tag}: sequence score vs float64 [rel to max(1,|ref|)]", float(err.max()))
    assert err.max() <= 1e-4, (tag, float(err.max()))
    assert_ranked(got, ids, got["score"], R.CONSENSUS, None, END, tag)
    norm = H.norm_table(STEPS)
    again = multi(m, enc, samples, seed=seed, temperature=temperature, rank="logprob", length_norm=norm)
    assert np.array_equal(again["ids"], ids) and again["score"].tobytes() == got["score"].tobytes()
    assert_ranked(again, ids, again["score"], R.LOGPROB, norm, END, tag + " logprob")


@pytest.mark.parametrize("images,samples", [(7, 5), (3, 16)])
@pytest.mark.parametrize("shape", [TINY, ODD, SHIPPED], ids=sid)
def test_samples_vs_float64(shape, images, samples):
    """35 rows (encoder row r / 5 crosses the 16-row tile edges) and 48 rows on encoder rows of 7 and 3 images."""
    check_samples(shape, images, samples, 900 + samples)


# The seed was picked on the float64 oracle alone (CPU): the 7 x 5 rows sampled along the oracle's own logits with rule64 /
# draw64 under the sticky stop, a draw counted when its mask margin or its distance to a CDF step is below GUARD.  Seed 905
# leaves 0 of 334 (TINY, 0.7), 0 of 311 (TINY, 1.3), 0 of 420 (ODD, 0.7) and 0 of 420 (ODD, 1.3) draws there -- at most 1 % was
# asked for, half of the 2 % cap, the other half being the device's own path's; 906 and 908 leave 1 of 420 at ODD.  In all
# four cases some image's five samples are five different sequences.
TEMPERED_SEED = 905


@pytest.mark.parametrize("temperature", [0.7, 1.3])
@pytest.mark.parametrize("shape", [TINY, ODD], ids=sid)
def test_samples_vs_float64_tempered(shape, temperature):
    """Away from temperature 1 the softmax's maximum and sum are those of the scaled logits, and the score's second pass
    takes its own from the raw ones (sample_batched_kernel<Rule, true>, unconstrained: NoRule)."""
    check_samples(shape, 7, 5, TEMPERED_SEED, temperature)


def test_reproducible_and_seeded():
    m, _, _ = model_of(SHIPPED)
    enc = enc_for(SHIPPED, 4, seed=44)
    a, b, c = multi(m, enc, 6, seed=5), multi(m, enc, 6, seed=5), multi(m, enc, 6, seed=6)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not np.array_equal(a["ids"], c["ids"])


def constrained_scores(m, cfg, table, enc, ids, samples):
    """float64 sequence scores under the constraint: the oracle's logits along the device's tokens, the columns the
    Python restatement of the rules allows at each step."""
    import img2latex_oracle as O
    sd64 = {k: v.detach().to(DEV, torch.float64) for k, v in m.state_dict().items() if k.startswith("decoder.")}
    flat = ids.reshape(-1, ids.shape[-1])
    toks = np.concatenate([np.full((flat.shape[0], 1), START), np.where(flat[:, :-1] < 0, END, flat[:, :-1])], axis=1)
    e64, hidden, out = enc.repeat_interleave(samples, 0).double(), None, []
    with torch.no_grad():
        for t in range(toks.shape[1]):
            lg, hidden = O.decode_step(sd64, cfg, e64, torch.from_numpy(toks[:, t:t + 1]).to(DEV), hidden)
            out.append(lg)
    logits = torch.cat(out, 1).cpu().numpy()
    steps = flat.shape[1]
    allowed = np.ones(logits.shape, dtype=bool)
    for r in range(flat.shape[0]):
        st = table.state_class()
        for t in range(steps):
            if flat[r, t] < 0:
                break
            allowed[r, t] = table.allowed(st, END, steps - t - 1).astype(bool)
            assert allowed[r, t, flat[r, t]], (r, t)
            table.advance(st, int(flat[r, t]), END)
    return R.sequence_scores(logits, flat, END, allowed)


@pytest.mark.parametrize("kind", ["brackets", "arguments"])
@pytest.mark.parametrize("shape", [ARG_SMALL, ARG_SHIPPED], ids=["V37_H64_L2", "V500_H512_L2"])
def test_constrained_samples_keep_the_rules(shape, kind):
    """test_arguments_decode_gpu's biased weights: the unconstrained draws fail the check the constrained ones pass.
    Brackets: BracketTable.well_formed (the bracket tables' name for "complete"); arguments: ArgumentTable.complete."""
    from test_decoder_shapes import shape_config
    m, arguments = loop_model(shape), loop_table(shape[0])
    cfg = shape_config(shape)
    table = arguments if kind == "arguments" else BracketTable(arguments.classes, END)
    ok = table.complete if kind == "arguments" else table.well_formed
    images, samples, steps = 5, 7, 20
    enc = enc_for(shape, images, seed=41)
    plain = multi(m, enc, samples, steps=steps, seed=4711, temperature=0.9)
    bad = sum(not ok(row, END) for row in plain["ids"].reshape(-1, steps).tolist())
    assert bad > 0, "vacuous: every unconstrained draw already keeps the rules"
    got = multi(m, enc, samples, steps=steps, seed=4711, temperature=0.9, constraint=table)
    for row in got["ids"].reshape(-1, steps).tolist():
        assert END in row and ok(row, END), row
    assert (got["finished"] == 1).all()
    want = constrained_scores(m, cfg, table, enc, got["ids"], samples)
    err = np.abs(got["score"].reshape(-1) - want) / np.maximum(1.0, np.abs(want))
    record(f"sample_decode_multi {kind} V={shape[0]}: sequence score vs float64 [rel to max(1,|ref|)]", float(err.max()))
    assert err.max() <= 1e-4, float(err.max())
    assert_ranked(got, got["ids"], got["score"], R.CONSENSUS, None, END, kind)
    # the public list: best first, cut rows, the sample index
    with torch.no_grad():
        hyps = m.sample_nbest(enc, START, END, steps, samples, 0.9, TOP_K, TOP_P, 4711, constraint=table)
    assert [[h.sample for h in img] for img in hyps] == got["order"].tolist()
    for i, img in enumerate(hyps):
        for h in img:
            row = got["ids"][i, h.sample].tolist()
            assert h.tokens == row[:row.index(END)] and h.finished and h.risk == got["risk"][i, h.sample]
            assert h.score == got["score"][i, h.sample] and h.key == float(h.risk)


# ------------------------------------------------------------------------------------------------ the predictor
def test_predictor_predict_samples(argument_checkpoint):
    from img2latex_amd.training import Predictor
    dev = torch.device(DEV)
    pred = Predictor.from_checkpoint(argument_checkpoint, device=dev)
    tok, T, S = pred.tokenizer, 40, 5
    rows = pred.predict_samples(PNG, samples=S, max_length=T, top_k=TOP_K, top_p=TOP_P, seed=3)
    assert len(rows) == S and all(isinstance(s, str) for s, _, _ in rows)
    with torch.no_grad():
        enc = pred.model.encoder(pred._prepare_image(PNG).to(dev))
        hyps = pred.model.sample_nbest(enc, tok.start_token_id, tok.end_token_id, T, S, 1.0, TOP_K, TOP_P, 3)[0]
    assert [s for s, _, _ in rows] == [tok.decode(h.tokens) for h in hyps]          # the strings are the detokenised ids
    assert [(sc, k) for _, sc, k in rows] == [(h.score, h.key) for h in hyps]
    assert [k for _, _, k in rows] == sorted(k for _, _, k in rows)                  # consensus: ascending risk
    assert pred.predict_batch_samples([PNG, PNG], samples=S, max_length=T, top_k=TOP_K, top_p=TOP_P, seed=3, batch_size=1)[0] == rows
    by_score = pred.predict_samples(PNG, samples=S, rank="logprob", max_length=T, top_k=TOP_K, top_p=TOP_P, seed=3,
                                    length_penalty=0.7)
    keys = [k for _, _, k in by_score]
    assert keys == sorted(keys, reverse=True) and sorted(s for s, _, _ in by_score) == sorted(s for s, _, _ in rows)
    full = pred.predict_samples(PNG, samples=S, max_length=T, top_k=TOP_K, top_p=TOP_P, seed=3, well_formed="arguments")
    assert len(full) == S and all(complete(pred, s) and nests(pred, s) for s, _, _ in full), full
    formed = pred.predict_samples(PNG, samples=S, max_length=T, top_k=TOP_K, top_p=TOP_P, seed=3, well_formed=True)
    assert len(formed) == S and all(nests(pred, s) for s, _, _ in formed), formed
    ens = Predictor.from_checkpoints([argument_checkpoint, argument_checkpoint], device=dev)
    with pytest.raises(RuntimeError, match="single-model"):
        ens.predict_samples(PNG, samples=S, top_k=TOP_K)
