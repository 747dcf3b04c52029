"""The schedule the headline number rests on: GreedyPipeline exactly as bench.py builds it by default (16-member grouped
decode, three batches in flight, the group region cleared early on the encoder stream, the encoder held behind the
decode's residency word, a separate copy stream) -- its ids against the reference's fixture and bit for bit against the
same kernel run one batch at a time, with a grouped-decode time-out (the pipeline's silent fallback) failing the test;
what close() leaves behind while batches are still in flight; and the residency word, which must never move backwards."""
import gc
import warnings

import numpy as np
import pytest
import torch

from conftest import record
from helpers import END, START, _margin_guard, load, model_for
from img2latex_amd import _lib, synth
from img2latex_amd.pipeline import GreedyPipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
G16 = _lib.FLAG_DECODE_GROUP16

# bench.py's pipelined region with its default arguments (--pipe-depth 3, co-resident with --decode-members 16,
# --decode-priority -1, one encoder stream, neither --pipe-late-clear nor --pipe-no-hold), copied rather than imported
HEADLINE = dict(depth=3, rows_per_workgroup=0, decode_streams=1, decode_flags=G16, decode_priority=-1, encoder_streams=1,
                encoder_priority=0, hold_encoder=None, clear_early=True)
SEEDS = (1234, 77, 78)                       # seed 1234 = the images of the reference's B=256 fixtures
# 12 batches, never the same image set twice in a row; batch j uses decoder slot j % (depth + 1), so each of the four
# slots is reused twice and sees a different image set than the batch before it in that slot
ORDER = [0, 1, 2, 0, 2, 1, 0, 1, 0, 2, 1, 2]


def headline_pipeline(m, steps=150, **override):
    return GreedyPipeline(m, START, END, steps, **{**HEADLINE, **override})


def run(pipe, batches):
    """bench.py's pipe_step for every batch, then its pipe_drain; the ids of every batch in submission order."""
    got = []
    for x in batches:
        if pipe.pending() >= pipe.depth:
            got.append(pipe.collect().numpy().copy())
        pipe.submit(x)
    while pipe.pending():
        got.append(pipe.collect().numpy().copy())
    return got


def serial_ids(m, x, steps=150):
    """The same kernel on the same images, one batch at a time on the caller's stream."""
    with torch.no_grad():
        return _lib.check_ids(m.greedy_ids(m.encoder(x), START, END, steps, flags=G16)[0].cpu()).numpy()


def slot_keys(m):
    return {k for k in m.decoder._ws_by_stream if isinstance(k, tuple) and k[0] == "slot"}


@pytest.mark.parametrize("fname", ["primary_cfg2", "primary_cfg2_clock"])
def test_headline_pipeline_ids_vs_reference(fname):
    """bench.py's default pipeline over 12 batches of three image sets at B=256, 150 steps: every batch bit-equal to the
    serial 16-member decode (the encoder is deterministic and it is the same kernel), no negative id, no time-out, the
    fixture's images within the margin guard of the reference's ids; the residency word counts every batch.  The same with
    the two A/B switches of bench.py (--pipe-late-clear, --pipe-no-hold)."""
    d, cfg, sd_kw = load(fname)
    m, _ = model_for(fname, sd_kw, cfg)
    ref_ids = d["ids"].astype(np.int64)
    steps = ref_ids.shape[1] - 1
    sets = [torch.from_numpy(synth.make_images(256, cfg, seed=s)).to(DEV) for s in SEEDS]
    want = [serial_ids(m, x) for x in sets]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    n_slots = HEADLINE["depth"] + 1
    assert all(a != b for a, b in zip(ORDER, ORDER[1:]))
    assert all(sum(1 for j in range(len(ORDER)) if j % n_slots == s) >= 3 for s in range(n_slots))
    first = None
    for variant in ({}, {"clear_early": False}, {"hold_encoder": False}):
        pipe = headline_pipeline(m, **variant)
        assert pipe.depth == 3 and len(pipe.enc_streams) == 1 and len(pipe.dec_streams) == 1
        assert pipe.copy_stream is not None and pipe.decode_flags == G16 and pipe.encoder_flags == 0
        assert pipe.hold_encoder == variant.get("hold_encoder", True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)          # a grouped decode that timed out fails here
            got = run(pipe, [sets[i] for i in ORDER])
        assert len(got) == len(ORDER)
        for j, (i, g) in enumerate(zip(ORDER, got)):
            _lib.check_ids(torch.from_numpy(g))
            assert int(g.min()) >= 0, (variant, j)
            assert np.array_equal(g, want[i]), (variant, j, i, int((g != want[i]).any(axis=1).sum()))
            if i == 0:
                diverged = _margin_guard(g[:, :steps], ref_ids, d["margins"], tol=2e-4)
                record(f"{fname} headline pipeline (group16, depth 3): rows that leave the reference at a near-tie", diverged)
                assert diverged <= 0.05 * 256
        if pipe.hold_encoder:
            assert int(pipe._resident.item()) == len(ORDER)
        if first is None:
            first = got
        else:
            assert all(np.array_equal(a, b) for a, b in zip(first, got)), variant
        pipe.close()


def test_pipeline_close_drains_in_flight_batches():
    """close() with `depth` batches still in flight returns only once their work has ended on every stream of the
    pipeline: the slot workspaces it gives back are no longer read or written by a decode, so memory the allocator hands
    out again keeps what is written to it.  A fresh pipeline on the same model then gives the serial ids."""
    d, cfg, sd_kw = load("primary_cfg2")
    m, _ = model_for("primary_cfg2", sd_kw, cfg)
    x = torch.from_numpy(synth.make_images(256, cfg, seed=1234)).to(DEV)
    want = serial_ids(m, x)
    before = slot_keys(m)
    pipe = headline_pipeline(m)
    for _ in range(pipe.depth):
        pipe.submit(x)
    mine = slot_keys(m) - before
    sizes = [m.decoder._ws_by_stream[k][0].numel() for k in mine]
    assert len(sizes) == pipe.depth
    pipe.close()
    assert pipe.pending() == 0
    streams = {"encoder": pipe.enc_streams, "decode": pipe.dec_streams, "copy": [pipe.copy_stream]}
    busy = [f"{kind} stream {i}" for kind, ss in streams.items() for i, s in enumerate(ss) if not s.query()]
    assert not busy, f"close() returned with work still queued on the {busy}"
    assert not (slot_keys(m) & mine)
    pipe.close()                                                      # a second close does nothing
    # the released workspaces came from the encoder stream's pool: take blocks at least that large from it again
    with torch.cuda.stream(pipe.enc_streams[0]):
        bufs = [torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV) for n in sizes]
    torch.cuda.synchronize()
    assert all(bool((b == 0xA5).all()) for b in bufs)
    del bufs
    fresh = headline_pipeline(m)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = run(fresh, [x, x])
    assert all(np.array_equal(g, want) for g in got)
    fresh.close()


def test_abandoned_predict_ids_stream_is_safe():
    """A consumer that stops reading Predictor.predict_ids_stream after one batch (its pipeline closes with batches in
    flight) leaves no slot workspace on the decoder, and the next stream still equals predict_batch_ids; a pipeline
    dropped with batches in flight (garbage collection) leaves the serial decode unchanged."""
    from img2latex_amd.training import Predictor, TokenTable
    d, cfg, sd_kw = load("primary_cfg2_clock")
    m, _ = model_for("primary_cfg2_clock", sd_kw, cfg)
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, cfg["vocab_size"])})
    pred = Predictor(m, TokenTable(vocab, max_sequence_length=150), device=torch.device(DEV))
    x = torch.from_numpy(synth.make_images(6 * 64, cfg, seed=1234)).to(DEV)
    batches = [x[i:i + 64] for i in range(0, 6 * 64, 64)]
    T = 60
    before = slot_keys(m)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        gen = pred.predict_ids_stream(iter(batches), max_length=T)
        head = next(gen)
        gen.close()                                                   # two batches still in flight
        assert not (slot_keys(m) - before)
        want = [pred.predict_batch_ids(b, max_length=T) for b in batches]
        got = list(pred.predict_ids_stream(iter(batches), max_length=T))
    assert head == got[0]                                             # same pipeline kernel, same images
    assert [len(g) for g in got] == [len(w) for w in want]
    differ = sum(1 for g, w in zip(got, want) for a, b in zip(g, w) if a != b)
    assert differ <= 2, differ                                        # the other kernel's sums: near-ties only
    # garbage collection of a pipeline with batches in flight
    x256 = torch.from_numpy(synth.make_images(256, cfg, seed=1234)).to(DEV)
    want256 = serial_ids(m, x256)
    pipe = headline_pipeline(m)
    for _ in range(pipe.depth):
        pipe.submit(x256)
    del pipe
    gc.collect()
    assert not (slot_keys(m) - before)
    assert np.array_equal(serial_ids(m, x256), want256)


def test_residency_word_never_moves_backwards():
    """The residency word is a wrapping sequence: every kind of decode launch (ungrouped, 4-, 8- and 16-member groups)
    stores its value only if it is ahead of the word, also across the wrap.  A 16-member pipeline with two decode streams
    (launches of consecutive batches publishing in either order) ends with the word at its last batch, without a time-out,
    ids equal to the serial decode."""
    d, cfg, sd_kw = load("primary_cfg2_clock")
    m, _ = model_for("primary_cfg2_clock", sd_kw, cfg)
    x = torch.from_numpy(synth.make_images(64, cfg, seed=1234)).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    tok0 = torch.full((64,), START, dtype=torch.int32, device=DEV)
    launches = [("ungrouped", 0, 1, 0), ("group4", 0, 0, 0), ("group8", _lib.FLAG_DECODE_GROUP8, 0, 8), ("group16", G16, 0, 16)]
    # (word before, value launched, word after); 0xFFFFFFF0 = int32 -16, and 5 is 21 steps ahead of it
    cases = [(200, 150, 200), (200, 201, 201), (0xFFFFFFF0 - (1 << 32), 5, 5)]
    with torch.no_grad():
        enc = m.encoder(x)
        for what, fl, rows_per_wg, members in launches:
            for start, value, after in cases:
                flag.fill_(start)
                ids, _, _ = m.decoder.run_steps(enc, 40, tok0, flags=fl, rows_per_workgroup=rows_per_wg,
                                                resident=(flag, value))
                torch.cuda.synchronize()
                assert int(flag.item()) == after, (what, start, value, int(flag.item()))
                assert int(ids.min()) >= 0, what
                if members:
                    st = m.decoder.group_status()
                    assert st["groups"] == 64 // members and not st["timed_out"], (what, st)     # it WAS that kernel
    sets = [torch.from_numpy(synth.make_images(64, cfg, seed=s)).to(DEV) for s in SEEDS]
    want = [serial_ids(m, s) for s in sets]
    pipe = headline_pipeline(m, decode_streams=2)
    assert len(pipe.dec_streams) == 2 and pipe.hold_encoder
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        got = run(pipe, [sets[i] for i in ORDER])
    assert len(got) == len(ORDER)
    for j, (i, g) in enumerate(zip(ORDER, got)):
        assert np.array_equal(g, want[i]), (j, i)
    assert int(pipe._resident.item()) == len(ORDER)
    pipe.close()
