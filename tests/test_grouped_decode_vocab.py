"""The grouped decode kernels (decode_group_kernel<4>, <8>, decode_group16_kernel, beam_group_kernel) against the
float64 restatement of test_decoder_shapes.py at vocabularies BELOW their 512 columns (group_shape_ok: L = 1,
H = 256, V <= 512): padding columns with a -inf bias, members that own no valid column (V = 33 leaves 14 of 16
members empty) or fewer than the beam width, the ``tk < V ? tk : 0`` guard, logits written at row stride V, and the
first-index tie-break across lanes, waves and members.

V is the first / last column of a member's slice for 16, 8 and 4 members (32, 64, 128 columns), one partly filled
16-column tile and the minimum; E cycles through 4, 36, 100, 256, 512.  33 rows leave the last group ragged at all
three member counts; 8 steps is the shortest loop on the grouped path, 8 and 9 are the two parities of its double
buffers.  Bounds are the suite's: ids equal the float64 ids up to a row's first float64 top1-top2 margin below 2e-4
(helpers._margin_guard), logits 1e-4 absolute, beam sequences equal unless the float64 ranking has a gap below 1e-4,
winning scores 1e-4.

Conditions on the inputs, asserted on the float64 reference alone before a kernel's output is read (_conditions):
at least 95 % of the (row, step) pairs lie before their row's first margin below 2e-4, at most 2 of the 33 rows are
cut short, and at least 8 compared steps have a margin below 1e-2, so that the guard has something to judge; a beam
case has at most 2 of its 7 searches below the 1e-4 gap and no empty winner.  The first test records the worst counts
per family of inputs, those of the 8- and 9-step prefixes included.  Weight seeds that meet them were picked on the
host (SEEDS; test_decoder_shapes.build's own seed elsewhere).  build's "negative" variant (output weights at
1/sqrt(H)) has margins so small that it keeps only 62 % of the pairs at V = 65, so the all-negative model here keeps
the output scale 12 and lowers the bias by 200 instead (|W_out h| <= 12/16 * 256 = 192): every valid logit is below
-190 and a padding column that read 0 instead of -inf would win every step.

The 8- and 16-member kernels return ids only: on those two this file catches index and padding errors and losses of
bf16 size, not a dropped 2^-16 partial product."""
import warnings

import numpy as np
import pytest
import torch

import img2latex_oracle as O
from conftest import record
from helpers import END, START, _margin_guard, close
from img2latex_amd import _lib, synth
from test_decoder_shapes import build, enc_for, model_from_sd, oracle_greedy, oracle_steps, shape_config, tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 2e-4
ROWS = 33
VS = [3, 17, 31, 33, 64, 65, 127, 129, 255, 257, 300, 383, 511]
ES = [4, 36, 100, 256, 512]
SEEDS = {3: 403, 17: 317}                 # build's own seed leaves fewer than 8 margins below 1e-2 at these two
FLAGS = {4: 0, 8: _lib.FLAG_DECODE_GROUP8, 16: _lib.FLAG_DECODE_GROUP16}
BEAM_CASES = [(6, 6), (7, 2), (130, 5), (258, 5), (258, 6), (386, 3), (300, 4), (511, 6)]     # (V, k)
BEAM_E = {6: 4, 7: 36, 130: 100, 258: 256, 386: 512}


def shape_of(V):
    E = ES[VS.index(V) % len(ES)] if V in VS else BEAM_E[V]
    return (V, E, 256, 1, False)


_SPECIAL = {}


def model(V, kind="plain"):
    """(model, float64 decoder state dict, cfg).  "plain": test_decoder_shapes.build; "negative": every logit below
    -190 (module docstring); "late_end": the END clock at (0.05, 40, 20) instead of (0.05, 12, 6) -- at k = V the
    beam [START, END] completes in the first step and wins unless END is that unlikely there."""
    shape = shape_of(V)
    if kind == "plain":
        return build(shape, seed=SEEDS.get(V))
    if (V, kind) not in _SPECIAL:
        cfg = shape_config(shape)
        if kind == "negative":
            sd = synth.make_state_dict(cfg, seed=121, out_scale=12.0)
            sd["decoder.output_layer.bias"] = sd["decoder.output_layer.bias"] - np.float32(200.0)
        else:
            assert kind == "late_end"
            sd = synth.make_state_dict(cfg, seed=306, out_scale=12.0, end_clock=(0.05, 40.0, 20.0))
        _SPECIAL[(V, kind)] = model_from_sd(cfg, sd) + (cfg,)
    return _SPECIAL[(V, kind)]


def _counts(margins, steps):
    """From float64 margins (rows, >= steps): (share of the (row, step) pairs before their row's first margin below
    MARGIN, rows cut short, compared pairs with a margin below 1e-2)."""
    mg = margins[:, :steps]
    below = mg < MARGIN
    cut = np.where(below.any(1), below.argmax(1), steps)
    near = sum(int((mg[b, :cut[b]] < 1e-2).sum()) for b in range(mg.shape[0]))
    return float(cut.sum()) / mg.size, int((cut < steps).sum()), near


def _conditions(margins, tag):
    """The module docstring's conditions on float64 margins of 40 steps."""
    share, cut, near = _counts(margins, 40)
    assert share >= 0.95 and cut <= 2 and near >= 8, (tag, share, cut, near)


_REFS = {}


def reference(V, kind, temperature=1.0):
    """float64 greedy ids (ROWS, 41) and margins (ROWS, 40) of model(V, kind) on enc_for(seed 9); the conditions hold
    for the margins as the run under test sees them (divided by its temperature)."""
    key = (V, kind)
    if key not in _REFS:
        _, sd64, cfg = model(V, kind)
        _REFS[key] = oracle_greedy(sd64, cfg, enc_for(shape_of(V), ROWS, seed=9), 40)
    ids, margins = _REFS[key]
    _conditions(margins / temperature, f"V{V} {kind} at temperature {temperature}")
    return ids, margins / temperature


def decode(m, enc, steps, members, **kw):
    """Free-running ids (ROWS, steps) of the grouped kernel with ``members`` members -- and the proof that it ran."""
    tok0 = torch.full((enc.shape[0],), START, dtype=torch.int32, device=DEV)
    ids, logits, _ = m.decoder.run_steps(enc, steps, tok0, flags=FLAGS[members], **kw)
    got = _lib.check_ids(ids.cpu()).numpy()            # a timed-out poll shows as -3: never compared
    st = m.decoder.group_status()
    assert st is not None and not st["timed_out"] and st["groups"] == -(-enc.shape[0] // members), (members, st)
    return got, logits


_DIVERGED = {}


def count_divergences(kernel, n):
    _DIVERGED[kernel] = _DIVERGED.get(kernel, 0) + n
    record(f"V < 512, {kernel}: (run, row) pairs leaving the float64 ids at a near-tie", _DIVERGED[kernel])


# ------------------------------------------------------------------------------------------ 0. the inputs
def test_inputs_meet_the_conditions_in_float64():
    """Every greedy and beam input of this file, from float64 alone: the conditions (asserted again wherever a reference
    is used) and, per family of inputs, the worst counts at 40, 8 and 9 steps for the record."""
    families = {}
    for V in VS:
        families.setdefault("plain", []).append(reference(V, "plain")[1])
        families.setdefault("plain at temperature 0.7", []).append(reference(V, "plain", 0.7)[1])
        families.setdefault("all-negative", []).append(reference(V, "negative")[1])
    for V in (300, 511):
        for P in (12, 32):
            families.setdefault("duplicated vocabulary", []).append(dup_model(V, P)[2])
    for family, all_margins in families.items():
        for steps in (40, 8, 9):
            counts = [_counts(mg, steps) for mg in all_margins]
            tag = f"V < 512 inputs, {family}, {steps} steps, float64 alone"
            record(f"{tag}: largest share of (row, step) pairs not compared", 1.0 - min(c[0] for c in counts))
            record(f"{tag}: most rows cut short (of {ROWS})", max(c[1] for c in counts))
            record(f"{tag}: fewest compared steps with a margin below 1e-2", min(c[2] for c in counts))
    gaps = [[gap for _, _, gap in beam_reference(V, k)] for V, k in BEAM_CASES]
    record("V < 512 inputs, beam, float64 alone: most searches of a case with a ranking gap below 1e-4 (of 7)",
           max(sum(g < 1e-4 for g in case) for case in gaps))


# ------------------------------------------------------------------------------------------ 1. free-running ids
@pytest.mark.parametrize("members", [4, 8, 16])
@pytest.mark.parametrize("V", VS)
def test_free_running_ids_vs_float64(V, members):
    """Arg max of the logits, of the softmax, at temperature 0.7, the sticky stop and the all-negative model, at 40, 8
    and 9 steps, on decode_group_kernel<4> / <8> / decode_group16_kernel."""
    enc = enc_for(shape_of(V), ROWS, seed=9)
    kernel = f"{members}-member kernel"
    for kind in ("plain", "negative"):
        m, _, _ = model(V, kind)
        runs = {"logits": dict(select=_lib.SELECT_LOGITS)}
        if kind == "plain":
            runs["softmax"] = dict(select=_lib.SELECT_SOFTMAX)
            runs["temperature 0.7"] = dict(select=_lib.SELECT_LOGITS, temperature=0.7)
        for steps in (40, 8, 9):
            got = {}
            for what, kw in runs.items():
                ref, margins = reference(V, kind, kw.get("temperature", 1.0))
                got[what], _ = decode(m, enc, steps, members, **kw)
                assert got[what].min() >= 0 and got[what].max() < V, (V, members, kind, what, steps)
                count_divergences(kernel, _margin_guard(got[what], ref, margins, MARGIN))
            if kind != "plain":
                continue
            sticky, _ = decode(m, enc, steps, members, stop=_lib.STOP_STICKY, end_id=END)
            for b in range(ROWS):
                ends = np.nonzero(got["logits"][b] == END)[0]
                n = int(ends[0]) + 1 if ends.size else steps
                assert np.array_equal(sticky[b, :n], got["logits"][b, :n]) and (sticky[b, n:] == -1).all(), \
                    (V, members, steps, b)


# ------------------------------------------------------------------------------------------ 2. teacher-forced logits
@pytest.mark.parametrize("T", [9, 40])
@pytest.mark.parametrize("V", VS)
def test_teacher_forced_logits_vs_float64(V, T):
    """Forced tokens and logits at row stride V: the 4-member kernel (the only grouped one that writes logits) and the
    row kernels at 1, 2 and 4 rows per workgroup, whose resident H = 256 variants take T >= 8 too."""
    shape = shape_of(V)
    m, sd64, cfg = model(V)
    enc = enc_for(shape, ROWS)
    forced = tokens(shape, ROWS, T).to(torch.int32).contiguous()
    ref, _ = oracle_steps(sd64, cfg, enc, forced)
    ref = ref.cpu().numpy()
    for r in (0, 1, 2, 4):
        ids, lg, _ = m.decoder.run_steps(enc, T, forced[:, 0].contiguous(), forced=forced, want_logits=True,
                                         rows_per_workgroup=r)
        ids, lg = _lib.check_ids(ids.cpu()).numpy(), lg.cpu().numpy()
        if r == 0:
            st = m.decoder.group_status()
            assert not st["timed_out"] and st["groups"] == -(-ROWS // 4), st
        close(lg, ref, 1e-4, f"V{V} teacher-forced logits, " + ("4-member kernel" if r == 0 else "row kernels"),
              absolute=True)
        assert np.array_equal(ids, lg.argmax(-1)), (V, T, r)         # numpy: the first index of a maximum


# ------------------------------------------------------------------------------------------ 3. duplicated vocabulary
_DUP = {}


def dup_model(V, P):
    """model(V)'s weights with W_out[v] = W_out[v % P], b_out[v] = b_out[v % P]; the float64 decoder cut to its first P
    output rows and embeddings.  Fed-back ids stay below P while the first index wins, so the two are one model and no
    float64 tie is ever consulted."""
    if (V, P) not in _DUP:
        cfg = shape_config(shape_of(V))
        sd = synth.make_state_dict(cfg, seed=121, out_scale=12.0, end_clock=(0.05, 12.0, 6.0))
        idx = np.arange(V) % P
        for n in ("decoder.output_layer.weight", "decoder.output_layer.bias"):
            sd[n] = np.ascontiguousarray(sd[n][idx])
        m, sd64 = model_from_sd(cfg, sd)
        for n in ("decoder.output_layer.weight", "decoder.output_layer.bias", "decoder.embedding.weight"):
            sd64[n] = sd64[n][:P].contiguous()
        _DUP[(V, P)] = (m,) + oracle_greedy(sd64, cfg, enc_for(shape_of(V), ROWS, seed=9), 40)
    _conditions(_DUP[(V, P)][2], f"V{V} duplicated from {P} tokens")
    return _DUP[(V, P)]


@pytest.mark.parametrize("P", [12, 32])
@pytest.mark.parametrize("V", [300, 511])
def test_duplicated_vocabulary_first_index_wins(V, P):
    """Every column v >= P repeats column v % P, in every member's slice: the three grouped kernels and the row kernel
    must pick ids below P at every step (and, mod P, the P-token float64 model's ids).  The two kernels that return
    logits return the duplicates bit-equal -- a column's summation tree does not depend on its position (fold_logits4,
    the row kernel's projection pass) -- which makes "below P" a statement about the tie-break alone."""
    m, ref, margins = dup_model(V, P)
    enc = enc_for(shape_of(V), ROWS, seed=9)
    idx = torch.arange(V) % P
    tok0 = torch.full((ROWS,), START, dtype=torch.int32, device=DEV)
    results = {}
    for members in (4, 8, 16):
        results[f"{members}-member kernel"] = decode(m, enc, 40, members, want_logits=members == 4)
    ids, lg, _ = m.decoder.run_steps(enc, 40, tok0, want_logits=True, rows_per_workgroup=1)
    results["row kernel"] = (ids.cpu().numpy(), lg)
    for kernel, (got, lg) in results.items():
        if lg is not None:
            lg = lg.cpu()
            unequal = int((lg != lg[..., idx]).sum())
            record(f"V{V} duplicated from {P} tokens, {kernel}: logits that differ from their duplicate's", unequal)
            assert torch.equal(lg[..., :P], lg[..., P:2 * P]) and unequal == 0, (V, P, kernel, unequal)
        count_divergences(kernel, _margin_guard(got % P, ref, margins, MARGIN))
        assert got.min() >= 0 and got.max() < P, (V, P, kernel, int(got.max()))


# ------------------------------------------------------------------------------------------ 4. grouped beam
_BEAM_REFS = {}


def beam_reference(V, k):
    """float64 O.beam_search of 7 images x 30 steps: [(sequence, score, smallest ranking gap)]."""
    if (V, k) not in _BEAM_REFS:
        _, sd64, cfg = model(V, "late_end" if k == V else "plain")
        enc = enc_for(shape_of(V), 7, seed=13).double()
        out = []
        for j in range(7):
            st = {}
            seq, sc = O.beam_search(sd64, cfg, enc[j:j + 1], START, END, 30, k, return_score=True, stats=st)
            out.append((seq, sc, st["gap"]))
        _BEAM_REFS[(V, k)] = out
    out = _BEAM_REFS[(V, k)]
    # at least 5 of the 7 sequences are compared, and a search that ends at once compares nothing
    assert sum(gap < 1e-4 for _, _, gap in out) <= 2 and all(seq for seq, _, _ in out), (V, k, out)
    return out


@pytest.mark.parametrize("flags", [0, _lib.FLAG_NO_GROUP], ids=["grouped", "workgroup_per_image"])
@pytest.mark.parametrize("V,k", BEAM_CASES)
def test_beam_search_vs_float64(V, k, flags):
    """beam_group_kernel and beam_kernel<K>, 7 images (unused slots in the last group at every k) x 30 steps, under
    test_decoder_shapes.test_beam_search_vs_float64's rule.  V = 130 and 258 leave one member two valid columns, fewer
    than k; at (6, 6) every step's candidates are the whole vocabulary."""
    want = beam_reference(V, k)
    m, _, _ = model(V, "late_end" if k == V else "plain")
    enc = enc_for(shape_of(V), 7, seed=13)
    which = "grouped" if flags == 0 else "workgroup per image"
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")         # a grouped search that timed out would re-run on the other kernel
        got, scores = m.beam_search_batch(enc, START, END, 30, k, return_scores=True, flags=flags)
    near, worst = 0, 0.0
    for j, (seq, sc, gap) in enumerate(want):
        assert all(0 <= t < V for t in got[j]), (V, k, j)
        if got[j] != seq:
            assert gap < 1e-4, (V, k, j, gap, got[j], seq)
            near += 1
            continue
        err = abs(scores[j] - sc) / max(1.0, abs(sc))
        worst = max(worst, err)
        assert err <= 1e-4, (V, k, j, scores[j], sc)
    record(f"V{V} beam k={k} [{which}] winning score vs float64 [rel to max(1,|score|)]", worst)
    count_divergences(f"beam kernel [{which}]", near)
