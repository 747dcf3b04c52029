"""The ensemble decode on the device (i2l_ensemble_decode, model/ensemble.py, Predictor.from_checkpoints) against the
float64 restatement of tests/ensemble_ref.py: per member img2latex_oracle.decode_step along the shared tokens,
log_softmax, the combination rule, the selection on the combined row.

Bounds.  The suite holds every member's logits to 1e-4 absolute; lse is 1-Lipschitz in the sup norm, so each lp_m is
within 2e-4, and both rules are convex in the members: the combined rows are within 2e-4 + 1e-5 |ref| (the second term
is the combine's own fp32 rounding).  Greedy ids equal the float64 ids up to a row's first step whose float64 top1-top2
margin is below the guard: 2e-4 under logprob (the margin between two columns is sum_m w_m (x_m[a] - x_m[b]), every lse_m
cancels: the suite's own bound), 4e-4 under prob (the lse terms do not cancel: two columns, each within 2e-4).

Section 1b takes the members' error out: the rule in float64 on the members' own DEVICE logits, the combined rows within
1e-5 max(1, |ref|) of it -- the second term above, alone -- at every member count and every chunk count of the kernel."""
import os

import numpy as np
import pytest
import torch

import ensemble_ref as E
from conftest import record
from helpers import END, GOLDEN, START, _margin_guard, check_sampling, close
from img2latex_amd import _lib, synth
from img2latex_amd.model import EnsembleDecoder
from img2latex_amd.model.ensemble import EncoderOutputs
from img2latex_amd.training import constraint as C
from img2latex_amd.training.constraint import ArgumentTable, BracketTable, argument_byte
from test_decoder_shapes import build, oracle_greedy, tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAG = _lib.FLAG_DECODE_BATCHED
STEPS = 40
GUARD = {"logprob": 2e-4, "prob": 4e-4}
RULES = ("logprob", "prob")

# (V, E, H, L, attention), weight seed
WIDE, DEEP, TINY = (513, 256, 256, 1, False), (513, 64, 128, 2, True), (3, 4, 64, 1, False)
SETS = {
    "a": ([(WIDE, 121), (WIDE, 7)], [0.5, 0.5]),                          # Vp 1024; V off the lane stride
    "b": ([(WIDE, 121), (DEEP, 55)], [0.7, 0.3]),                         # differing E, H, L, attention; unequal weights
    "c": ([(TINY, 1), (TINY, 2), (TINY, 3)], None),                       # V below one lane stride
    "d": ([(WIDE, 121), (DEEP, 55), (DEEP, 56)], [0.5, 0.25, 0.25]),      # three members
    "e": ([(TINY, s) for s in range(36, 44)], None),                      # M == I2L_MAX_ENSEMBLE
}
# The weight seeds were picked on the float64 restatement alone (CPU): under both rules every set has at most 1 of 33 rows
# (3 of 257; set e: 2 of 33) with a margin below the guard, and member 0 alone decodes at least half of the rows of every
# row count differently (seeds 11..18 for set e left member 0 agreeing with the ensemble in 5 of 5 rows).
MANY_ROWS = ("a", "logprob")         # the one case at 257 rows


def rows_of(name, rule):
    return (1, 5, 33) + ((257,) if (name, rule) == MANY_ROWS else ())


def built(name):
    return [build(shape, seed=seed) for shape, seed in SETS[name][0]]          # [(model, sd64, cfg)]


def decoder_of(name, rule):
    return EnsembleDecoder([m.decoder for m, _, _ in built(name)], SETS[name][1], rule)


def encs_of(name, rows):
    return EncoderOutputs(torch.from_numpy(synth.uniform(9 + m, "enc", (rows, shape[1]), -1.5, 1.5)).to(DEV)
                          for m, (shape, _) in enumerate(SETS[name][0]))


def reference(name, rule, rows):
    encs = encs_of(name, rows)
    return E.Ensemble([(sd64, cfg, enc) for (_, sd64, cfg), enc in zip(built(name), encs)], SETS[name][1], rule)


def tok0_of(rows):
    return torch.full((rows,), START, dtype=torch.int32, device=DEV)


_GREEDY = {}


def greedy_reference(name, rule, rows, table=None):
    """float64 ids and margins of (set, rule, rows), computed once and shared by the tests below."""
    key = (name, rule, rows, None if table is None else type(table).__name__)
    if key not in _GREEDY:
        _GREEDY[key] = reference(name, rule, rows).greedy(STEPS, START, END, table)
    return _GREEDY[key]


# ------------------------------------------------------------------------------------------------ 1. combined rows
@pytest.mark.parametrize("T", [3, 9])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", list(SETS))
def test_combined_rows_teacher_forced(name, rule, T):
    dec = decoder_of(name, rule)
    V = SETS[name][0][0][0][0]
    worst = 0.0
    for rows in rows_of(name, rule):
        encs = encs_of(name, rows)
        ref = reference(name, rule, rows)
        forced = tokens(SETS[name][0][0][0], rows, T).to(torch.int32).contiguous()
        given = [(torch.from_numpy(synth.uniform(7 + m, "h0", (s[3], rows, s[2]), -0.9, 0.9)).to(DEV),
                  torch.from_numpy(synth.uniform(7 + m, "c0", (s[3], rows, s[2]), -2.0, 2.0)).to(DEV))
                 for m, (s, _) in enumerate(SETS[name][0])]
        for hidden in (None, given):
            _, lg, state = dec.run_steps(encs, T, forced[:, 0].contiguous(), forced=forced, hidden=hidden, want_ids=False,
                                         want_logits=True, want_state=True)
            want, want_state = ref.forced(forced, None if hidden is None else [(h.double(), c.double()) for h, c in hidden])
            got, want = lg.cpu().numpy().astype(np.float64), want.cpu().numpy()
            assert got.shape == (rows, T, V) and np.isfinite(got).all()
            err = np.abs(got - want)
            worst = max(worst, float(err.max()))
            over = err - (2e-4 + 1e-5 * np.abs(want))
            assert over.max() <= 0, (name, rule, T, rows, float(err.max()))
            for (h, c), (rh, rc) in zip(state, want_state):
                close(h.cpu().numpy(), rh.cpu().numpy(), 1e-5, f"ensemble {name} teacher-forced h")
                close(c.cpu().numpy(), rc.cpu().numpy(), 1e-5, f"ensemble {name} teacher-forced c")
    record(f"ensemble {name} {rule} T={T}: combined rows vs float64 [abs]", worst)


# ------------------------------------------------------------------------------------------------ 1b. the combine alone
# ensemble_combine_kernel<M> holds 512 columns of every member a chunk: one exactly full chunk, two, three with one column in
# the last, four (the limit), and V on and one past the lane stride.  Every M meets the two- and three-chunk walks with a
# ragged last chunk, every V meets the smallest and the largest but one M.
COMBINE_V = (64, 65, 512, 513, 1024, 1025, 2048)
COMBINE_CASES = sorted({(M, V) for M in range(2, 9) for V in (513, 1025)} | {(M, V) for M in (2, 7) for V in COMBINE_V})


def small(V):
    return (V, 4, 64, 1, False)          # the smallest decoder the step-batched kernels accept


def uneven(M):
    """Unequal weights of sum 1 up to their rounding to fp32, which is done here: the entry takes floats."""
    w = np.arange(1, M + 1, dtype=np.float64) ** 1.5
    return [float(x) for x in (w / w.sum()).astype(np.float32)]


@pytest.mark.parametrize("M,V", COMBINE_CASES)
def test_combine_alone_vs_float64(M, V):
    """The combine without its members' error.  Each member's own device logits come from running it as a one-member
    EnsembleDecoder -- the single-model call bit for bit (test_one_member_is_the_single_model_call), the kernels the
    ensemble launches for that member, unchanged -- along the same forced tokens from the same state on its own encoder
    rows; ensemble_ref's rule applied to them in float64 is what the ensemble's combined rows are held to, within
    1e-5 max(1, |ref|): the term the bound at the head of this file gives to the combine's own fp32 rounding, alone.
    Columns [V, Vp) are never written and not looked at: logits_out has V columns."""
    shape, T = small(V), 3
    decs = [build(shape, seed=300 + m)[0].decoder for m in range(M)]
    worst = {rule: 0.0 for rule in RULES}
    for rows in (1, 5, 33):
        encs = EncoderOutputs(torch.from_numpy(synth.uniform(9 + m, "enc", (rows, shape[1]), -1.5, 1.5)).to(DEV) for m in range(M))
        forced = tokens(shape, rows, T).to(torch.int32).contiguous()
        given = [(torch.from_numpy(synth.uniform(7 + m, "h0", (1, rows, 64), -0.9, 0.9)).to(DEV),
                  torch.from_numpy(synth.uniform(7 + m, "c0", (1, rows, 64), -2.0, 2.0)).to(DEV)) for m in range(M)]
        for hidden in (None, given):
            kw = dict(forced=forced, want_ids=False, want_logits=True)
            own = []
            for m in range(M):
                _, lg, _ = EnsembleDecoder([decs[m]], None, "logprob").run_steps(
                    [encs[m]], T, forced[:, 0].contiguous(), hidden=None if hidden is None else [hidden[m]], **kw)
                assert lg.shape == (rows, T, V) and bool(torch.isfinite(lg).all())
                own.append(lg.cpu().double())
            assert not torch.equal(own[0], own[1]), "vacuous: two members hold the same rows"
            for rule in RULES:
                for weights in (uneven(M), None):
                    _, lg, _ = EnsembleDecoder(decs, weights, rule).run_steps(encs, T, forced[:, 0].contiguous(), hidden=hidden, **kw)
                    got, want = lg.cpu().numpy().astype(np.float64), E.combine(own, weights, rule).numpy()
                    assert got.shape == (rows, T, V) and np.isfinite(got).all()
                    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
                    worst[rule] = max(worst[rule], float(err.max()))
                    at = np.unravel_index(int(err.argmax()), err.shape)
                    assert err.max() <= 1e-5, (M, V, rule, weights is not None, rows, hidden is not None, float(err.max()), at)
    for rule in RULES:
        record(f"ensemble combine alone M={M} V={V} {rule}: combined rows vs float64 of the members' device logits "
               "[rel to max(1,|ref|)]", worst[rule])


# ------------------------------------------------------------------------------------------------ 2. greedy ids
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", list(SETS))
def test_greedy_ids_vs_float64(name, rule):
    dec = decoder_of(name, rule)
    V = SETS[name][0][0][0][0]
    guard = GUARD[rule]
    runs = {
        "logits": dict(select=_lib.SELECT_LOGITS),
        "softmax": dict(select=_lib.SELECT_SOFTMAX),
        "temperature 0.7": dict(select=_lib.SELECT_LOGITS, temperature=0.7),
    }
    for rows in rows_of(name, rule):
        tag = f"ensemble {name} {rule} rows={rows}"
        encs = encs_of(name, rows)
        ref, margins = greedy_reference(name, rule, rows)
        # the inputs: the other members matter -- member 0 alone, in float64, decodes at least half of the rows differently
        _, sd64, cfg = built(name)[0]
        own, _ = oracle_greedy(sd64, cfg, encs[0], STEPS)
        differ = int((own != ref).any(axis=1).sum())
        assert 2 * differ >= rows, f"vacuous: member 0 alone gives the ensemble's ids in {rows - differ} of {rows} rows"
        for what, kw in runs.items():
            ids, _, _ = dec.run_steps(encs, STEPS, tok0_of(rows), **kw)
            got = ids.cpu().numpy()
            assert got.min() >= 0 and got.max() < V, (tag, what)
            scaled = margins / kw.get("temperature", 1.0)
            left = _margin_guard(got, ref, scaled, guard)
            near = int((scaled.min(axis=1) < guard).sum())
            record(f"{tag} greedy ({what}): rows leaving the float64 ids at a near-tie", left)
            record(f"{tag} greedy ({what}): rows with a float64 margin below the guard", near)
            assert left <= near, (tag, what, left, near)
            assert rows - left >= 0.9 * rows, (tag, what, left)


# ------------------------------------------------------------------------------------------------ 3. one member
def loop_table(V):
    """test_arguments_decode_gpu's table: three bracket kinds, \\begin{array}, \\frac, ^, two more demanding columns."""
    t = np.zeros(V, dtype=np.uint8)
    t[[0, 1, 3, 10]] = 255
    for k in range(3):
        t[4 + 2 * k], t[5 + 2 * k] = C.open_class(k), C.close_class(k)
    t[8] = argument_byte(C.open_class(2), 1)
    t[11], t[12] = argument_byte(0, 2), argument_byte(0, 1, True)
    t[13], t[14] = argument_byte(0, 2, True), argument_byte(0, 3)
    return ArgumentTable(t, END)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def steps_run(ids, stop):
    """Steps whose launches did something: all of them, or under the sticky stop those up to the last row's END (the
    later launches return at once and leave the outputs of their steps, and the final state, unwritten)."""
    if stop == _lib.STOP_NONE:
        return ids.shape[1]
    return int((ids >= 0).any(dim=0).sum())


@pytest.mark.parametrize("rows", [5, 33])
def test_one_member_is_the_single_model_call(rows):
    m, _, _ = build(DEEP, seed=55)
    one = m.decoder
    arguments = loop_table(DEEP[0])
    brackets = BracketTable(arguments.classes, END)
    enc = encs_of("b", rows)[1]
    sample = (0.9, 5, 0.9, 4711)
    for rule in RULES:
        dec = EnsembleDecoder([one], [3.0], rule)
        for table in (None, brackets, arguments):
            for stop in (_lib.STOP_NONE, _lib.STOP_STICKY):
                kw = dict(stop=stop, end_id=END, select=_lib.SELECT_SOFTMAX, temperature=0.8, want_logits=True,
                          want_state=True, constraint=table)
                ids, lg, (h, c) = one.run_steps(enc, STEPS, tok0_of(rows), flags=FLAG, **kw)
                e_ids, e_lg, e_state = dec.run_steps([enc], STEPS, tok0_of(rows), **kw)
                assert torch.equal(ids, e_ids), (rule, stop)
                n = steps_run(ids, stop)
                assert same_bits(lg[:, :n], e_lg[:, :n]), (rule, stop)
                if n == STEPS:
                    assert same_bits(h, e_state[0][0]) and same_bits(c, e_state[0][1]), (rule, stop)
                s_ids, s_pr, (sh, sc) = one.sample_steps(enc, STEPS, tok0_of(rows), *sample, stop=stop, end_id=END,
                                                         want_probs=True, flags=FLAG, want_state=True, constraint=table)
                t_ids, t_pr, t_state = dec.sample_steps([enc], STEPS, tok0_of(rows), *sample, stop=stop, end_id=END,
                                                        want_probs=True, want_state=True, constraint=table)
                n = steps_run(s_ids, stop)
                assert torch.equal(s_ids, t_ids) and same_bits(s_pr[:, :n], t_pr[:, :n]), (rule, stop)
                if n == STEPS:
                    assert same_bits(sh, t_state[0][0]) and same_bits(sc, t_state[0][1]), (rule, stop)


# ------------------------------------------------------------------------------------------------ 4. sampling
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("rows", [5, 33])
def test_sampling_vs_float64(rows, rule):
    """helpers.check_sampling, unchanged: EnsembleDecoder.sample_steps has sample_steps' call shape, the float64 ensemble
    is the oracle step."""
    dec = decoder_of("b", rule)
    encs = encs_of("b", rows)
    step = reference("b", rule, rows).oracle_step()
    for top_k, top_p in ((5, 0.0), (0, 0.9), (5, 0.9)):
        check_sampling(dec, encs, step, top_k, top_p, 1.0, seed=2024 + top_k, steps=6,
                       what=f"ensemble b {rule} rows={rows} sampling top_k={top_k} top_p={top_p} probabilities")


# ------------------------------------------------------------------------------------------------ 5. constraints
@pytest.mark.parametrize("kind", ["brackets", "arguments"])
@pytest.mark.parametrize("rule", RULES)
def test_constrained_ensemble(rule, kind):
    dec = decoder_of("b", rule)
    arguments = loop_table(WIDE[0])
    table = arguments if kind == "arguments" else BracketTable(arguments.classes, END)
    good = (lambda r: table.complete(r, END) and table.well_formed(r, END)) if kind == "arguments" else \
        (lambda r: table.well_formed(r, END))
    fresh = C.ArgumentState if kind == "arguments" else C.BracketState
    for rows in (5, 33):
        tag = f"ensemble b {rule} {kind} rows={rows}"
        encs = encs_of("b", rows)
        ref, margins = greedy_reference("b", rule, rows, table)
        if rows == 33:      # the inputs: the constraint has something to do (float64: 6 or 7 of the 33 free rows break it)
            free, _ = greedy_reference("b", rule, rows)
            assert sum(not good(r[1:]) for r in free.tolist()) >= 3, tag
        ids, _, _ = dec.run_steps(encs, STEPS, tok0_of(rows), end_id=END, constraint=table)
        got = ids.cpu().numpy()
        for r in got.tolist():
            assert END in r and good(r), (tag, r)
        left = _margin_guard(got, ref, margins, GUARD[rule])
        near = int((margins.min(axis=1) < GUARD[rule]).sum())
        record(f"{tag} greedy: rows leaving the float64 ids at a near-tie", left)
        assert left <= near and rows - left >= 0.9 * rows, (tag, left, near)
        for stop in (_lib.STOP_NONE, _lib.STOP_STICKY):
            s_ids, probs = dec.sample_steps(encs, STEPS, tok0_of(rows), 0.9, 5, 0.9, 4711, stop=stop, end_id=END,
                                            want_probs=True, constraint=table)
            again, _ = dec.sample_steps(encs, STEPS, tok0_of(rows), 0.9, 5, 0.9, 4711, stop=stop, end_id=END, constraint=table)
            assert torch.equal(s_ids, again)
            probs = probs.cpu().numpy()
            for b, r in enumerate(s_ids.cpu().tolist()):
                assert END in r, (tag, r)
                n = r.index(END)
                assert good(r[:n + 1]), (tag, r)
                if stop == _lib.STOP_STICKY:
                    assert all(i == -1 for i in r[n + 1:]), (tag, r)
                st = fresh()
                for t in range(n + 1):
                    mask = table.allowed(st, END, STEPS - t - 1).astype(bool)
                    assert mask[r[t]] and (probs[b, t][~mask] == 0.0).all(), (tag, b, t)
                    table.advance(st, r[t], END)
    with pytest.raises(RuntimeError):
        dec.run_steps(encs, STEPS, tok0_of(rows), forced=torch.zeros((rows, STEPS), dtype=torch.int32, device=DEV),
                      end_id=END, constraint=table)


# ------------------------------------------------------------------------------------------------ 6. sticky stop
@pytest.mark.parametrize("name,rule", [("a", "logprob"), ("b", "prob"), ("d", "logprob"), ("e", "prob")])
def test_sticky_stop(name, rule):
    dec = decoder_of(name, rule)
    for rows in rows_of(name, rule):
        encs = encs_of(name, rows)
        free, _, _ = dec.run_steps(encs, STEPS, tok0_of(rows))
        sticky, _, _ = dec.run_steps(encs, STEPS, tok0_of(rows), stop=_lib.STOP_STICKY, end_id=END)
        free, sticky = free.cpu().numpy(), sticky.cpu().numpy()
        last = 0
        for b in range(rows):
            ends = np.nonzero(free[b] == END)[0]
            n = int(ends[0]) + 1 if ends.size else STEPS
            last = max(last, n)
            assert np.array_equal(sticky[b, :n], free[b, :n]) and (sticky[b, n:] == -1).all(), (name, rows, b)
        assert (sticky[:, last:] == -1).all(), (name, rows)


# ------------------------------------------------------------------------------------------------ 7. the surface
PT = os.path.join(GOLDEN, "predict_64x800.pt")
PNG = os.path.join(GOLDEN, "predict_page.png")


@pytest.fixture(scope="module")
def second_checkpoint(tmp_path_factory):
    """The fixture checkpoint with seeded noise on its decoder's weights: same vocabulary, another model."""
    ck = torch.load(PT, map_location="cpu", weights_only=False)
    g = torch.Generator().manual_seed(77)
    for k, v in ck["model_state_dict"].items():
        if k.startswith("decoder.") and v.dtype == torch.float32:
            ck["model_state_dict"][k] = v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g)
    path = str(tmp_path_factory.mktemp("ensemble") / "second.pt")
    torch.save(ck, path)
    return path


def test_predictor_from_checkpoints(second_checkpoint):
    from img2latex_amd.training import Predictor
    dev = torch.device(DEV)
    T = 40
    single = Predictor.from_checkpoint(PT, device=dev)
    before = single.predict(PNG, max_length=T)
    ens = Predictor.from_checkpoints([PT, second_checkpoint], weights=[0.6, 0.4], combine="logprob", device=dev)
    assert ens.tokenizer.token_to_id == single.tokenizer.token_to_id and ens.model_type == single.model_type
    text = ens.predict(PNG, max_length=T)
    x = torch.cat([ens._prepare_image(PNG)] * 3)
    tok = ens.tokenizer
    # predict is _greedy_search's loop (arg max of the logits, no sticky stop), predict_batch the sticky softmax arg max:
    # the same tokens up to the first END
    assert ens.predict_batch([PNG, PNG], max_length=T) == [text] * 2
    rows = ens.predict_batch_ids(x, max_length=T)
    assert [tok.decode(r[1:]) for r in rows] == [text] * 3
    for wf in (True, "arguments"):
        formed = ens.predict(PNG, max_length=T, well_formed=wf)
        assert ens.predict_batch([PNG], max_length=T, well_formed=wf) == [formed]
        assert [tok.decode(r[1:]) for r in ens.predict_batch_ids(x, max_length=T, well_formed=wf)] == [formed] * 3
        table = C.as_table(wf, tok)
        ids = tok.encode(formed) + [END]
        assert table.well_formed(ids) and (wf is True or table.complete(ids)), formed
    sampled = ens.predict_batch([PNG, PNG], max_length=T, temperature=0.9, top_k=5, top_p=0.9, seed=5)
    assert sampled == ens.predict_batch([PNG, PNG], max_length=T, temperature=0.9, top_k=5, top_p=0.9, seed=5)
    tgt = torch.tensor([[START, 5, 6, END, 0, 0]] * 3, dtype=torch.int32, device=DEV)
    out = ens.evaluate_batch(x, tgt, max_length=T, return_strings=True, return_statistics=True)
    assert {"bleu", "levenshtein", "batch_size", "pred_ids", "pred_len", "pred_text", "statistics"} <= set(out)
    assert out["pred_text"] == [text] * 3 and out["batch_size"] == 3
    # the prob rule, and one checkpoint through the ensemble constructor: the single predictor's output
    assert isinstance(Predictor.from_checkpoints([PT, second_checkpoint], combine="prob", device=dev).predict(PNG, max_length=T), str)
    alone = Predictor.from_checkpoints([PT], device=dev, decode_flags=FLAG)
    assert alone.predict(PNG, max_length=T) == Predictor.from_checkpoint(PT, device=dev, decode_flags=FLAG).predict(PNG, max_length=T)
    # what has no ensemble form is refused before anything is launched
    for call, said in ((lambda: ens.predict_ids_stream(iter([x])), "predict_ids_stream"),
                       (lambda: ens.predict_strings_stream(iter([x])), "predict_strings_stream"),
                       (lambda: ens.evaluate_stream(iter([(x, tgt)])), "evaluate_stream"),
                       (lambda: ens.predict_nbest(PNG, beam_size=3), "predict_nbest"),
                       (lambda: ens.predict_batch_nbest([PNG], beam_size=3), "predict_batch_nbest")):
        with pytest.raises(RuntimeError, match=said):
            call()
    with torch.no_grad(), pytest.raises(RuntimeError, match="beam_size=3"):
        ens.model.inference(x[:1], START, END, max_length=T, beam_size=3)
    # a single-checkpoint predictor is the parent's
    assert Predictor.from_checkpoint(PT, device=dev).predict(PNG, max_length=T) == before
    assert len(list(single.predict_strings_stream(iter([x]), max_length=T))) == 1


def test_cli_ensemble(second_checkpoint, capsys):
    from img2latex_amd import cli
    from img2latex_amd.training import Predictor
    assert cli.main(["predict", PT, PNG, "--max-length", "40"]) == 0
    alone = capsys.readouterr().out
    assert cli.main(["predict", PT, PNG, "--max-length", "40", "--ensemble", second_checkpoint, "--ensemble-weights", "0.6,0.4",
                     "--ensemble-rule", "prob"]) == 0
    out = capsys.readouterr().out
    assert out.startswith("Generated LaTeX:\n")
    ens = Predictor.from_checkpoints([PT, second_checkpoint], weights=[0.6, 0.4], combine="prob", device=torch.device(DEV))
    assert out.split("\n")[1] == ens.predict(PNG, max_length=40)
    assert alone.split("\n")[1] == Predictor.from_checkpoint(PT, device=torch.device(DEV)).predict(PNG, max_length=40)


def test_cli_evaluate_ensemble(second_checkpoint, tmp_path, capsys):
    import json
    import shutil
    from img2latex_amd import cli
    ck_dir = tmp_path / "outputs" / "tiny_exp" / "checkpoints"
    os.makedirs(ck_dir)
    shutil.copyfile(PT, ck_dir / "ck.pt")
    assert cli.main(["evaluate", str(ck_dir / "ck.pt"), os.path.join(GOLDEN, "dataset_tiny"), "--batch-size", "5", "--device",
                     "cuda", "--output-dir", str(tmp_path / "out"), "--ensemble", second_checkpoint]) == 0
    said = capsys.readouterr().out
    assert "BLEU-4 Score:" in said and "Number of Samples:" in said
    saved = json.loads((tmp_path / "out" / "tiny_exp" / "predictions" / "predictions.json").read_text())
    assert saved and all(set(p) == {"prediction", "reference"} for p in saved)
