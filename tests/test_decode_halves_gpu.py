"""Two batches per 16-member grouped launch, half the steps of each (i2l_greedy_decode_halves, GreedyPipeline's split
decode): a batch decoded as two ranges of steps, with another batch in the other row tile each time, gives the ids of the
one-batch 16-member launch bit for bit -- ragged rows, odd step counts, an absent tile --; the headline pipeline with the
split on equals the serial decode and the pipeline with the split off, through a batch-size change and as strings; a
launch that fails takes both of its batches to the fallback and leaves the next launch clean."""
import warnings

import numpy as np
import pytest
import torch

from helpers import END, START, load, model_for
from img2latex_amd import _lib, synth
from img2latex_amd.model.lstm_decoder import DecodeHalf
from img2latex_amd.pipeline import GreedyPipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
G16 = _lib.FLAG_DECODE_GROUP16
FIXTURE = "primary_cfg2_clock"
OWNER = "test-decode-halves"
# bench.py's pipelined region with its default arguments, as tests/test_pipeline_headline.py states them (copied)
HEADLINE = dict(depth=3, rows_per_workgroup=0, decode_streams=1, decode_flags=G16, decode_priority=-1, encoder_streams=1,
                encoder_priority=0, hold_encoder=None, clear_early=True)
SEEDS = (1234, 77, 78)
_CACHE = {}


def fixture():
    """The model, three sets of 64 images and their encoder rows: built once for the module."""
    if "m" not in _CACHE:
        d, cfg, sd_kw = load(FIXTURE)
        m, _ = model_for(FIXTURE, sd_kw, cfg)
        sets = [torch.from_numpy(synth.make_images(64, cfg, seed=s)).to(DEV) for s in SEEDS]
        with torch.no_grad():
            encs = [m.encoder(x).clone() for x in sets]
        _CACHE.update(m=m, cfg=cfg, sets=sets, encs=encs)
    return _CACHE["m"], _CACHE["sets"], _CACHE["encs"]


def serial(which, rows, T):
    """run_steps(flags=FLAG_DECODE_GROUP16) on the first `rows` rows of image set `which`: the reference of every test here."""
    key = ("serial", which, rows, T)
    if key not in _CACHE:
        m, _, encs = fixture()
        tok0 = torch.full((rows,), START, dtype=torch.int32, device=DEV)
        with torch.no_grad():
            ids, _, _ = m.decoder.run_steps(encs[which][:rows].contiguous(), T, tok0, flags=G16, end_id=END)
        _CACHE[key] = _lib.check_ids(ids.cpu()).numpy()
    return _CACHE[key]


def status_of(dec, ws, rows):
    off = _lib.lib().i2l_decoder_group_status_offset(rows, dec.vocab_size, dec.embedding_dim, dec.hidden_dim, dec.lstm_layers)
    st = ws[off:off + 16].view(torch.int32).cpu().tolist()
    return {"timed_out": bool(st[0]), "groups": st[1]}


# (rows of the older tile, rows of the newer tile) of the launch in the middle of a chain of two batches; None: the chain is
# one batch, whose launches have the other tile absent -- (24, None) runs its last steps alone, (None, 24) its first
CASES = [(32, 32), (16, 16), (40, 24), (24, None), (None, 24)]


@pytest.mark.parametrize("T", [1, 2, 7, 40])
@pytest.mark.parametrize("rows", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_halves_equal_the_one_batch_launch(rows, T):
    """A chain of launches (absent, X first half), (X second half, Y first half), (Y second half, absent) -- first half =
    ceil(T / 2) steps -- over two different image sets: the ids of X and of Y equal the 16-member launch of that batch
    alone, no launch timed out, every group of the larger tile took part.  With one tile None the chain is a single batch,
    placed so that the named tile is the one that runs beside nothing."""
    m, _, encs = fixture()
    dec = m.decoder
    if rows[1] is None:
        chain = [(0, rows[0])]
    elif rows[0] is None:
        chain = [(1, rows[1])]
    else:
        chain = [(0, rows[0]), (1, rows[1])]
    first = (T + 1) // 2
    batches = []
    with torch.no_grad():
        for i, (which, r) in enumerate(chain):
            enc = encs[which][:r].contiguous()
            dec.prepare(enc, slot=("halves", OWNER, i))
            batches.append(dict(ws=dec._ws, version=dec._ws_key[2], rows=r, which=which,
                                tok0=torch.full((r,), START, dtype=torch.int32, device=DEV),
                                ids=torch.full((r, T), -7, dtype=torch.int32, device=DEV)))
        half = lambda b, t0, n: DecodeHalf(b["ws"], b["version"], b["rows"], T, t0, n, b["tok0"], b["ids"])
        for i in range(len(batches) + 1):
            older = half(batches[i - 1], first, T - first) if i > 0 else None
            newer = half(batches[i], 0, first) if i < len(batches) else None
            if older is not None and older.n_steps == 0 and newer is None:
                continue                                                # T = 1: nothing left to run
            dec.decode_halves(older, newer, end_id=END)
            home = newer if newer is not None else older
            st = status_of(dec, home.ws, home.rows)
            assert not st["timed_out"], (i, st)
            live = [h.rows for h in (older, newer) if h is not None and h.n_steps > 0]
            assert st["groups"] == -(-max(live) // 16), (i, st)
    for b in batches:
        got = b["ids"].cpu().numpy()
        assert int(got.min()) >= 0, (b["rows"], int(got.min()))
        want = serial(b["which"], b["rows"], T)
        assert np.array_equal(got, want), (b["rows"], T, int((got != want).any(axis=1).sum()))
    dec.release_slots(OWNER)


def test_halves_refuse_workspaces_of_different_weights():
    m, _, encs = fixture()
    dec = m.decoder
    enc = encs[0][:16].contiguous()
    with torch.no_grad():
        dec.prepare(enc, slot=("halves", OWNER, 0))
    tok0 = torch.full((16,), START, dtype=torch.int32, device=DEV)
    ids = torch.empty((16, 8), dtype=torch.int32, device=DEV)
    good = DecodeHalf(dec._ws, dec._ws_key[2], 16, 8, 0, 4, tok0, ids)
    stale = good._replace(version=good.version + (("other",),), first_step=4)
    with pytest.raises(RuntimeError, match="different weights"):
        dec.decode_halves(stale, good, end_id=END)
    dec.release_slots(OWNER)


def run(pipe, batches, strings=False):
    got = []
    take = (lambda: pipe.collect_strings()) if strings else (lambda: pipe.collect().numpy().copy())
    for x in batches:
        if pipe.pending() >= pipe.depth:
            got.append(take())
        pipe.submit(x)
    while pipe.pending():
        got.append(take())
    return got


def pipeline_serial(which, rows, T):
    key = ("pipe-serial", which, rows, T)
    if key not in _CACHE:
        m, sets, _ = fixture()
        with torch.no_grad():
            ids = m.greedy_ids(m.encoder(sets[which][:rows]), START, END, T, flags=G16)[0]
        _CACHE[key] = _lib.check_ids(ids.cpu()).numpy()
    return _CACHE[key]


def test_split_pipeline_equals_the_serial_decode():
    """The headline pipeline at B = 64, T = 41 (halves of 21 and 20 steps) over 7 batches of three image sets, never the
    same set twice running; 7 is odd, so the last batch ends in a launch of its own.  Every batch equals the serial
    16-member decode, the residency word counts every batch, a time-out warning is an error; the same run with the split
    off gives the same ids."""
    m, sets, _ = fixture()
    order = [0, 1, 2, 0, 2, 1, 0]
    want = [pipeline_serial(i, 64, 41) for i in range(3)]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    runs = {}
    for split in (None, False):
        pipe = GreedyPipeline(m, START, END, 41, **HEADLINE, split_decode=split)
        assert pipe.split_decode == (split is None)
        assert pipe.depth == 3 and len(pipe.enc_streams) == 1 and len(pipe.dec_streams) == 1 and pipe.copy_stream is not None
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            got = run(pipe, [sets[i] for i in order])
        assert len(got) == len(order)
        for j, (i, g) in enumerate(zip(order, got)):
            assert int(g.min()) >= 0, (split, j)
            assert np.array_equal(g, want[i]), (split, j, i, int((g != want[i]).any(axis=1).sum()))
        assert int(pipe._resident.item()) == len(order)
        pipe.close()
        runs[split] = got
    assert all(np.array_equal(a, b) for a, b in zip(runs[None], runs[False]))


def test_split_pipeline_through_a_batch_size_change_and_as_strings():
    """Batches of 64, 48 and 64 rows (the launch in the middle pairs 64 rows with 48, the next one 48 with 64): ids equal to
    the serial decode, and the strings of collect_strings() equal to those of the pipeline with the split off."""
    from img2latex_amd.training import DetokenizeTable, TokenTable
    m, sets, _ = fixture()
    cfg = _CACHE["cfg"]
    vocab = {"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3}
    vocab.update({f"t{i}": i for i in range(4, cfg["vocab_size"])})
    table = DetokenizeTable(TokenTable(vocab, max_sequence_length=150), DEV)
    plan = [(0, 64), (1, 48), (2, 64)]
    batches = [sets[i][:r] for i, r in plan]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        pipe = GreedyPipeline(m, START, END, 41, **HEADLINE)
        assert pipe.split_decode
        got = run(pipe, batches)
        pipe.close()
        for (i, r), g in zip(plan, got):
            assert np.array_equal(g, pipeline_serial(i, r, 41)), (i, r)
        texts = {}
        for split in (None, False):
            pipe = GreedyPipeline(m, START, END, 41, **HEADLINE, detokenize=table, split_decode=split)
            texts[split] = run(pipe, batches, strings=True)
            pipe.close()
    assert [len(t) for t in texts[None]] == [64, 48, 64] and any(s for t in texts[None] for s in t)
    assert texts[None] == texts[False]


def test_a_failed_launch_takes_both_batches_to_the_fallback():
    """Batches a, b, c; the launch of submit(b) -- second half of a, first half of b -- is made to time out the way
    test_pipeline_falls_back_when_the_grouped_decode_times_out does (silent member, 2 ms limits), the others are clean.
    a and b come back through collect()'s fallback, one warning each, with the row-per-workgroup kernel's ids; the launch
    of submit(c) marks b's rows instead of resuming them and decodes c, which equals the serial 16-member decode."""
    m, sets, _ = fixture()
    T = 41
    with torch.no_grad():
        rowwise = [_lib.check_ids(m.greedy_ids(m.encoder(sets[i]), START, END, T, rows_per_workgroup=1)[0].cpu()).numpy()
                   for i in (0, 1)]
    pipe = GreedyPipeline(m, START, END, T, **HEADLINE)
    assert pipe.split_decode
    pipe.submit(sets[0])
    pipe.decode_flags = G16 | _lib.FLAG_TEST_DROP_MEMBER | _lib.FLAG_TEST_SHORT_TIMEOUT
    pipe.submit(sets[1])
    pipe.decode_flags = G16
    pipe.submit(sets[2])
    with pytest.warns(RuntimeWarning):
        a = pipe.collect().numpy().copy()
    with pytest.warns(RuntimeWarning):
        b = pipe.collect().numpy().copy()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        c = pipe.collect().numpy().copy()
    pipe.close()
    assert np.array_equal(a, rowwise[0]) and np.array_equal(b, rowwise[1])
    assert np.array_equal(c, pipeline_serial(2, 64, T))
