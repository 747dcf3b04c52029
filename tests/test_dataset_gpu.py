"""The device-resident data set on the GPU: the three kernels through the C ABI (i2l_tokenize_packed, i2l_collate_ids,
i2l_gather_ragged_u8) against the Python rule / numpy, ``preprocess_resident`` bit for bit against ``preprocess_batch``,
the loaders batch for batch against what the REFERENCE's ``create_data_loaders`` yielded on tests/golden/dataset_tiny
(tests/golden/dataset.npz, written by make_golden_dataset.py), and the ``evaluate`` / ``train --data native`` commands.
Integer and byte comparisons are exact; images are ``torch.equal`` with ``tables="host"`` (Pillow's own arithmetic)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd import data as D
from img2latex_amd.data.dataset import decode_page
from img2latex_amd.training import Predictor, TokenTable, pack_texts, tokenize_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = os.path.join(GOLDEN, "dataset_tiny")
CKPT = os.path.join(GOLDEN, "predict_64x800.pt")
PAD, START, END, UNK = 0, 1, 2, 3
GUARD = -77
_CACHE = {}


def golden_tokenize():
    if "tok" not in _CACHE:
        d = np.load(os.path.join(GOLDEN, "tokenize.npz"))
        raw, off = d["text_bytes"].tobytes(), d["text_off"]
        texts = [raw[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
        vocab = {str(t): int(i) for t, i in zip(d["tokens"], d["token_ids"])}
        _CACHE["tok"] = (TokenTable(vocab, max_sequence_length=150), texts)
    return _CACHE["tok"]


def host_rows(tok, texts, add_special):
    rows = [[tok.token_to_id.get(w, UNK) for w in t.split()] for t in texts]
    return [[START] + r + [END] for r in rows] if add_special else rows


def run_packed(tok, data, off, add_special, capacity=None, rows=None, slack=4):
    """The C call -> (rc, ids with `slack` guard words behind the capacity, out_off, status)."""
    t = tokenize_table(tok, DEV)
    rows = off.size - 1 if rows is None else rows
    if capacity is None:
        capacity = int(data.size) + 2 * rows + 1
    text = torch.from_numpy(np.concatenate([np.asarray(data, np.uint8), np.zeros(1, np.uint8)])).to(DEV)
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int32)).to(DEV)
    ids = torch.full((capacity + slack,), GUARD, dtype=torch.int32, device=DEV)
    out_off = torch.full((rows + 2,), GUARD, dtype=torch.int64, device=DEV)
    status = torch.full((1,), GUARD, dtype=torch.int32, device=DEV)
    L = _lib.lib()
    ws = torch.empty((L.i2l_tokenize_packed_workspace_bytes(rows),), dtype=torch.uint8, device=DEV)
    rc = L.i2l_tokenize_packed(text.data_ptr(), int(data.size), d_off.data_ptr(), rows, t.image.data_ptr(), t.image.numel(),
                               t.unk_id, t.start_id, t.end_id, int(add_special), ids.data_ptr(), capacity, out_off.data_ptr(),
                               status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy(), out_off.cpu().numpy(), int(status.item())


def check_packed(tok, texts, add_special, what=None):
    data, off = pack_texts(texts)
    want = host_rows(tok, texts, add_special)
    rc, ids, out_off, status = run_packed(tok, data, off, add_special)
    assert rc == 0 and status == 0, (what, rc, status)
    n = len(texts)
    want_off = np.concatenate([[0], np.cumsum([len(r) for r in want])]).astype(np.int64)
    assert np.array_equal(out_off[:n + 1], want_off), what
    assert out_off[n + 1] == GUARD
    flat = np.array([v for r in want for v in r], np.int32)
    assert np.array_equal(ids[:flat.size], flat), what
    assert bool((ids[flat.size:] == GUARD).all()), what                 # packed without gaps, nothing behind the total
    return want, ids, out_off


# ------------------------------------------------------------------------------------------------ i2l_tokenize_packed
@pytest.mark.parametrize("add_special", [0, 1])
def test_tokenize_packed_equals_the_host_rule_and_i2l_tokenize(add_special):
    tok, texts = golden_tokenize()
    want, ids, out_off = check_packed(tok, texts, add_special, "golden texts")
    # i2l_tokenize's uncut rows: a width no row reaches
    t = tokenize_table(tok, DEV)
    text, row_off = t.upload(texts)
    width = max(len(r) for r in want) + 1
    padded, out_len, _, status = t.launch(text, row_off, width, bool(add_special))
    assert int(status.item()) == 0
    padded, out_len = padded.cpu().numpy(), out_len.cpu().numpy()
    for r in range(len(texts)):
        assert np.array_equal(padded[r, :out_len[r]], ids[out_off[r]:out_off[r + 1]]), r


def test_tokenize_packed_row_counts_and_chunk_boundaries():
    tok, texts = golden_tokenize()
    words = [w for w in tok.token_to_id if not w.startswith("<")]
    for add_special in (0, 1):
        # 0 rows: only the scan runs
        rc, ids, out_off, status = run_packed(tok, np.zeros(0, np.uint8), np.zeros(1, np.int32), add_special)
        assert rc == 0 and status == 0 and out_off[0] == 0 and out_off[1] == GUARD and bool((ids == GUARD).all())
        check_packed(tok, texts[40:41], add_special, "1 row")
        check_packed(tok, texts[30:35], add_special, "5 rows")          # not a multiple of the four rows per workgroup
    # rows whose length crosses the 64-byte chunk at 63, 64 and 65 bytes, with the last token on either side of it
    edge = []
    for n in (63, 64, 65, 127, 128, 129):
        edge += ["x " * ((n - 1) // 2) + "y" * (n - 2 * ((n - 1) // 2)), " " * (n - 2) + "xy", "z" * n, ("x" * 61 + " yz zz")[:n].ljust(n)]
    assert {63, 64, 65} <= {len(e.encode()) for e in edge}
    check_packed(tok, edge, 1, "chunk edges")
    # about 3000 short rows (three passes of the scan's 1024 threads), a 400-token row, empty and blank rows between them
    many = [" ".join(words[(7 * r + k) % len(words)] for k in range(r % 5)) for r in range(3001)]
    many[17], many[1023], many[1024], many[2500] = " ".join(["x"] * 400), "", "   \t ", "　 "
    want, _, out_off = check_packed(tok, many, 1, "3001 rows")
    assert out_off[3001] == sum(len(r) for r in want) and len(want[17]) == 402


def test_tokenize_packed_capacity_and_bad_offsets():
    tok, texts = golden_tokenize()
    data, off = pack_texts(texts)
    want = host_rows(tok, texts, 1)
    total = sum(len(r) for r in want)
    flat = np.array([v for r in want for v in r], np.int32)
    rc, ids, out_off, status = run_packed(tok, data, off, 1, capacity=total - 1)
    assert rc == 0 and status == 1                                      # I2L_TOKENIZE_PACKED_OVERFLOW
    assert out_off[len(texts)] == total and np.array_equal(np.diff(out_off[:len(texts) + 1]), [len(r) for r in want])
    assert np.array_equal(ids[:total - 1], flat[:total - 1]) and bool((ids[total - 1:] == GUARD).all())
    rc, ids, out_off, status = run_packed(tok, data, off, 1, capacity=total)
    assert rc == 0 and status == 0 and np.array_equal(ids[:total], flat)
    # one bad row offset: its bit, that row is empty, the others are untouched by it
    some = ["x y", "x y z", "y", "z z"]
    data, off = pack_texts(some)
    bad = off.copy()
    bad[2] = off[1] - 2                                                 # row 1 ends in front of its start; row 2 starts earlier
    rc, ids, out_off, status = run_packed(tok, data, bad, 0)
    assert rc == 0 and status == 2
    lens = np.diff(out_off[:5])
    assert lens[1] == 0 and lens[0] == 2 and lens[3] == 2
    rc, ids, out_off, status = run_packed(tok, data, bad, 1)
    assert status == 2 and np.array_equal(ids[out_off[1]:out_off[2]], [START, END])
    # refusals before any launch
    L = _lib.lib()
    assert L.i2l_tokenize_packed(None, 2 ** 31, None, 1, None, 0, 3, 1, 2, 1, None, 0, None, None, None, 0, None) != 0
    assert L.i2l_tokenize_packed_workspace_bytes(0) > 0


# ---------------------------------------------------------------------------------------------------- i2l_collate_ids
def run_collate(rows, index, width, stride=None, pad=PAD):
    lens = [len(r) for r in rows]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.array([v for r in rows for v in r] + [GUARD] * 8, np.int32)  # words behind the store: never to be read as a row
    d_ids, d_off = torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV)
    d_idx = torch.from_numpy(np.asarray(index, np.int64)).to(DEV)
    B = len(index)
    stride = width + 3 if stride is None else stride
    out = torch.full((B, stride), GUARD, dtype=torch.int32, device=DEV)
    status = torch.full((1,), GUARD, dtype=torch.int32, device=DEV)
    rc = _lib.lib().i2l_collate_ids(d_ids.data_ptr(), int(off[-1]), d_off.data_ptr(), len(rows), d_idx.data_ptr(), B, width, pad,
                                    out.data_ptr(), stride, status.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), int(status.item())


def test_collate_ids_equals_the_collator_rule():
    rng = np.random.default_rng(5)
    rows = [list(rng.integers(4, 500, size=int(n))) for n in list(rng.integers(0, 90, size=37)) + [1, 150, 64, 65, 63]]
    for B in (1, 5, 64):
        index = rng.integers(0, len(rows), size=B).tolist()
        if B > 1:
            index[1] = index[0]                                         # a repeated index
        if B == 64:
            index[7] = 38                                               # the 150-id row
        longest = max(len(rows[i]) for i in index)
        for width in (longest, longest + 1):
            rc, out, status = run_collate(rows, index, width)
            assert rc == 0 and status == 0, (B, width)
            want = np.full((B, width), PAD, np.int32)
            for b, i in enumerate(index):
                want[b, :len(rows[i])] = rows[i]
            assert np.array_equal(out[:, :width], want), (B, width)
            assert bool((out[:, width:] == GUARD).all())
    # an index outside the store and a row longer than the width: their bits, PAD rows, the other rows unharmed
    index = [2, -1, len(rows), 38, 3]
    width = max(len(rows[2]), len(rows[3]), 1)
    rc, out, status = run_collate(rows, index, width, pad=9)
    assert rc == 0 and status == 3
    for b in (1, 2, 3):
        assert bool((out[b, :width] == 9).all())
    assert out[0, :len(rows[2])].tolist() == rows[2] and out[4, :len(rows[3])].tolist() == rows[3]
    assert bool((out[:, width:] == GUARD).all())
    assert run_collate(rows, [38], 149)[2] == 1 and run_collate(rows, [len(rows)], 5)[2] == 2
    assert _lib.lib().i2l_collate_ids(None, 0, None, 0, None, 1, 0, 0, None, 0, None, None) != 0     # width 0


def test_formula_store_collate_equals_tokenize_table_collate():
    tok = eval_tokenizer()
    store = D.FormulaStore(os.path.join(TINY, "im2latex_formulas.norm.lst"), tok, DEV)
    t = tokenize_table(tok, DEV)
    for idx in ([0], [8, 1, 9, 1], list(range(len(store))), [5, 5, 5]):
        got = store.collate(idx)
        want = t.collate([store.raw_formula(i) for i in idx])
        assert got.dtype == want.dtype == torch.int32 and got.is_cuda and got.is_contiguous()
        assert got.shape == want.shape and torch.equal(got, want), idx
    assert store.collate([8]).shape[1] == 157 and tuple(store.collate([1]).cpu().tolist()[0]) == (START, END)
    assert tuple(store.collate([]).shape) == (0, 0)
    with pytest.raises(IndexError):
        store.collate([len(store)])


# ----------------------------------------------------------------------------------------------- i2l_gather_ragged_u8
SIZES = [0, 1, 3, 15, 16, 17, 63, 64, 65, 4097, 300001]


def test_gather_ragged_u8_is_byte_exact_at_every_alignment():
    rng = np.random.default_rng(11)
    pages = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in SIZES]
    L = _lib.lib()
    for src_mis in (0, 5):
        # the store: every page at a multiple of 256 plus src_mis, 0xAB between them
        s_off, cur = [], 0
        for p in pages:
            s_off.append(cur + src_mis)
            cur += (p.size + src_mis + 255) // 256 * 256 + 256
        src = np.full(cur, 0xAB, np.uint8)
        for o, p in zip(s_off, pages):
            src[o:o + p.size] = p
        d_src = torch.from_numpy(src).to(DEV)
        for dst_mis in range(16):
            order = rng.permutation(len(pages)).tolist()
            order.insert(3, order[-1])                                  # one page taken twice
            d_off, cur = [], 64
            for i in order:
                d_off.append(cur + dst_mis)
                cur = (cur + dst_mis + pages[i].size + 31) // 32 * 32 + 32   # guard bytes between the destinations
            want = np.full(cur + 64, 0xEE, np.uint8)
            for i, o in zip(order, d_off):
                want[o:o + pages[i].size] = pages[i]
            lists = np.concatenate([[s_off[i] for i in order], [pages[i].size for i in order], d_off]).astype(np.int64)
            d_lists = torch.from_numpy(lists).to(DEV)
            dst = torch.full((want.size,), 0xEE, dtype=torch.uint8, device=DEV)
            status = torch.full((1,), GUARD, dtype=torch.int32, device=DEV)
            n = len(order)
            rc = L.i2l_gather_ragged_u8(d_src.data_ptr(), src.size, d_lists.data_ptr(), d_lists.data_ptr() + 8 * n, n,
                                        max(SIZES), dst.data_ptr(), want.size, d_lists.data_ptr() + 16 * n, status.data_ptr(),
                                        _lib.stream_ptr())
            assert rc == 0
            got = dst.cpu().numpy()
            assert int(status.item()) == 0
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (src_mis, dst_mis, int(bad[0]), bad.size)
    # a range that leaves a buffer is not copied and reports it; max_size too small still copies whole ranges
    lists = np.array([s_off[10], s_off[9], 300001, src.size, 0, 400000], np.int64)
    d_lists = torch.from_numpy(lists).to(DEV)
    dst = torch.full((700000,), 0xEE, dtype=torch.uint8, device=DEV)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    rc = L.i2l_gather_ragged_u8(d_src.data_ptr(), src.size, d_lists.data_ptr(), d_lists.data_ptr() + 16, 2, 100,
                                dst.data_ptr(), dst.numel(), d_lists.data_ptr() + 32, status.data_ptr(), _lib.stream_ptr())
    got = dst.cpu().numpy()
    assert rc == 0 and int(status.item()) == 1
    assert np.array_equal(got[:300001], pages[10]) and bool((got[300001:] == 0xEE).all())


# ------------------------------------------------------------------------------------------------ preprocess_resident
def tiny_paths():
    return [os.path.join(TINY, "img", f"p{k:02d}.png") for k in range(12)] + [os.path.join(TINY, "img", "missing_a.png")]


@pytest.mark.parametrize("channels", [1, 3])
def test_preprocess_resident_is_bit_identical_to_preprocess_batch(channels):
    paths = tiny_paths()
    store = D.PageStore(paths, channels, DEV, decode_threads=3, chunk_bytes=20000)      # several upload chunks
    assert len(store) == 13 and store.failed.tolist() == [False] * 12 + [True]
    assert bool((store.offsets % 256 == 0).all()) and {1, 3} == set(store.shapes[:12, 2].tolist())
    pages = [decode_page(p, channels) for p in paths[:12]]
    for r, a in enumerate(pages):
        got = store.pixels[store.offsets[r]:store.offsets[r] + a.size].cpu().numpy()
        assert np.array_equal(got, a.reshape(-1)), r
    index = [3, 0, 3, 7, 11, 5, 2, 10, 6, 1, 9, 8, 4, 3]                 # mixed L / RGB, a page three times
    ids = np.arange(100, 100 + len(index))
    for tables in ("device", "host"):
        for augment in (None, D.Augment(seed=3)):
            kw = dict(img_size=(32, 128), channels=channels, tables=tables, augment=augment, sample_ids=ids, epoch=2)
            got = D.preprocess_resident(store, index, **kw)
            want = D.preprocess_batch([pages[i] for i in index], **kw)
            assert got.shape == (len(index), channels, 32, 128) and torch.equal(got, want), (tables, augment is not None)
    with pytest.raises(IndexError):
        D.preprocess_resident(store, [12])                              # the failed page has no pixels
    assert tuple(D.preprocess_resident(store, [], img_size=(32, 128), channels=channels).shape) == (0, channels, 32, 128)


# ----------------------------------------------------------------------------------- loaders vs the reference fixture
def eval_tokenizer():
    if "eval_tok" not in _CACHE:
        tk = torch.load(CKPT, map_location="cpu", weights_only=False)["tokenizer_config"]
        _CACHE["eval_tok"] = TokenTable(tk["token_to_id"], tk["special_tokens"], tk["max_sequence_length"])
    return _CACHE["eval_tok"]


def fixture():
    if "npz" not in _CACHE:
        _CACHE["npz"] = np.load(os.path.join(GOLDEN, "dataset.npz"))
    return _CACHE["npz"]


def fixture_batches(d, key):
    k = 0
    while f"{key}_{k}_ids" in d:
        yield (json.loads(str(d[f"{key}_{k}_names"])), d[f"{key}_{k}_idx"].tolist(), d[f"{key}_{k}_ids"], d[f"{key}_{k}_images"],
               json.loads(str(d[f"{key}_{k}_raw"])))
        k += 1


@pytest.mark.parametrize("channels", [1, 3])
def test_loaders_give_the_references_batches(channels):
    d = fixture()
    runs = {}
    for resident in (True, False):
        cfg = json.loads(str(d[f"config_c{channels}"]))
        cfg["data"].update(data_dir=TINY, load_in_memory=resident)
        torch.manual_seed(1234)                                         # make_golden_dataset.py SEED
        loaders = D.create_data_loaders(cfg, eval_tokenizer(), device=DEV, tables="host")
        assert loaders["train"].dataset.resident is resident
        got = runs[resident] = []
        zero_rows = 0
        for key, split in (("train0", "train"), ("train1", "train"), ("val", "val"), ("test", "test")):
            mine = list(loaders[split])
            want = list(fixture_batches(d, f"c{channels}_{key}"))
            assert len(mine) == len(want) == len(loaders[split]) and len(want) > 0, key
            for b, (batch, (names, idx, ids, images, raw)) in enumerate(zip(mine, want)):
                assert batch["image_paths"] == names and batch["formula_idxs"] == idx and batch["raw_formulas"] == raw, (key, b)
                assert batch["formulas"].dtype == torch.int32 and batch["formulas"].is_cuda
                assert tuple(batch["formulas"].shape) == ids.shape and np.array_equal(batch["formulas"].cpu().numpy(), ids), (key, b)
                x = batch["images"]
                assert x.dtype == torch.float32 and x.is_cuda and tuple(x.shape) == images.shape == (len(names), channels, 32, 128)
                assert torch.equal(x.cpu(), torch.from_numpy(images)), (key, b, float((x.cpu() - torch.from_numpy(images)).abs().max()))
                for r, name in enumerate(names):
                    if name.startswith("missing"):
                        assert bool((x[r] == 0).all())                  # the reference's zero image, not normalised
                        zero_rows += 1
                got.append(batch)
        assert zero_rows >= 1                                           # test holds one; train's is there when it is drawn
    for a, b in zip(runs[True], runs[False]):                           # resident and streaming: identical batches
        assert torch.equal(a["images"], b["images"]) and torch.equal(a["formulas"], b["formulas"])
        assert a["image_paths"] == b["image_paths"]


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_evaluate_equals_the_references_loop(tmp_path, capsys):
    from img2latex_amd import cli
    d = fixture()
    ck_dir = tmp_path / "outputs" / "tiny_exp" / "checkpoints"
    os.makedirs(ck_dir)
    shutil.copyfile(CKPT, ck_dir / "ck.pt")
    out = cli.evaluate(str(ck_dir / "ck.pt"), TINY, split="test", batch_size=5, device="cuda", output_dir=str(tmp_path / "results"))
    want = json.loads(str(d["eval_results"]))
    saved = json.loads((tmp_path / "results" / "tiny_exp" / "predictions" / "predictions.json").read_text())
    print("bleu", out["bleu"], float(d["eval_bleu"]), "levenshtein", out["levenshtein"], float(d["eval_levenshtein"]))
    assert saved == want                                                # predictions and references, string for string
    assert out["batch_size"] == int(d["eval_count"]) == len(want)
    assert abs(out["bleu"] - float(d["eval_bleu"])) <= 1e-12 and abs(out["levenshtein"] - float(d["eval_levenshtein"])) <= 1e-12
    text = capsys.readouterr().out
    assert "BLEU-4 Score:" in text and "Levenshtein Similarity:" in text and f"Number of Samples: {len(want)}" in text
    # --num-samples truncates the split; a beam size is clamped to greedy with a warning
    with pytest.warns(UserWarning, match="greedy"):
        few = cli.evaluate(str(ck_dir / "ck.pt"), TINY, num_samples=3, beam_size=4, device="cuda", output_dir=str(tmp_path / "few"))
    assert few["batch_size"] == 3
    assert json.loads((tmp_path / "few" / "tiny_exp" / "predictions" / "predictions.json").read_text()) == want[:3]


def _train_config(tmp_path):
    config = {
        "model": {"name": "cnn_lstm", "embedding_dim": 32,
                  "encoder": {"cnn": {"img_height": 16, "img_width": 32, "channels": 1, "conv_filters": [4, 8, 16],
                                      "kernel_size": 3, "pool_size": 2, "padding": "same"}},
                  "decoder": {"hidden_dim": 64, "lstm_layers": 1, "dropout": 0.0, "attention": False, "max_seq_length": 160}},
        "data": {"data_dir": TINY, "batch_size": 4, "max_seq_length": 160},
        "training": {"device": "cuda", "epochs": 2, "early_stopping_patience": 5, "learning_rate": 1e-3, "weight_decay": 0.0,
                     "accumulation_steps": 1},
        "evaluation": {"bleu_batches": 1},
    }
    path = tmp_path / "config.yaml"
    path.write_text(yaml.safe_dump(config))
    return str(path)


def _train_twice(tmp_path):
    from img2latex_amd import cli
    cfg = _train_config(tmp_path)
    return [cli.train(cfg, f"run{k}", None, None, "cuda", 7, output_dir=str(tmp_path / "outputs"), augment=True, data="native")
            for k in range(2)]


def test_cli_train_native_runs(tmp_path):
    """``train --data native`` on dataset_tiny: the vocabulary fitted on the device, two steps per epoch (11 samples, batch
    4, drop_last) for two epochs with the raw-page warp, a finite loss, validation on the 5 val samples, and a checkpoint
    that Predictor.from_checkpoint loads."""
    import math
    from img2latex_amd import cli
    out = cli.train(_train_config(tmp_path), "run", None, None, "cuda", 7, output_dir=str(tmp_path / "outputs"), augment=True,
                    data="native")
    assert out["steps"] == 4 and out["global_step"] == 4 and math.isfinite(out["loss"])
    assert math.isfinite(out["val_metrics"]["val_loss"]) and out["val_metrics"]["val_samples"] == 5
    ck = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    vocab = ck["tokenizer_config"]["token_to_id"]
    assert len(vocab) > 40 and vocab["<PAD>"] == 0 and "t4" in vocab and "α" in vocab
    p = Predictor.from_checkpoint(out["checkpoint"], device=torch.device("cuda"))
    assert p.tokenizer.vocab_size == len(vocab)
    with pytest.raises(SystemExit):
        cli.train(_train_config(tmp_path), "bad", None, None, "cuda", 7, output_dir=str(tmp_path / "outputs"), data="elsewhere")


def test_cli_train_native_twice_gives_bit_identical_parameters(tmp_path):
    """The same seed, ``--data native`` run twice: bit-identical parameters.  The two runs see the same batches (the
    loader's order and its warp are functions of the seed alone), and every sum of the training step has a fixed order:
    the embedding gradient, once a scatter of fp32 atomics whose order varied from launch to launch (1 or 2 of the 1760
    embedding weights then differed in about every second pair of runs), is a gather in ascending token position
    (train_decoder.hip, ``emb_gather_kernel``)."""
    outs = _train_twice(tmp_path)
    cks = [torch.load(o["checkpoint"], map_location="cpu", weights_only=False) for o in outs]
    assert cks[0]["tokenizer_config"]["token_to_id"] == cks[1]["tokenizer_config"]["token_to_id"]
    differing = {}
    for k, v in cks[0]["model_state_dict"].items():
        w = cks[1]["model_state_dict"][k]
        if not torch.equal(v, w):
            differing[k] = (float((v - w).abs().max()), int((v != w).sum()), v.numel(), float(v.abs().max()))
    print("parameters that differ between two runs (max |diff|, elements, of, max |w|):", differing)
    assert not differing, differing
