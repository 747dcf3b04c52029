"""The host half of the device-resident data set (img2latex_amd/data/dataset.py): everything that decides WHICH samples
form a batch needs no GPU -- split-file parsing (reference dataset.py:233-269) against the samples the reference itself
read from tests/golden/dataset_tiny (tests/golden/dataset.npz), the index order against torch's own DataLoader, the
batch-size rule and the config defaults of create_data_loaders -- plus the presence of the new exports and the
``evaluate`` command's options."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd import data as D
from img2latex_amd.training import TokenTable

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TINY = os.path.join(GOLDEN, "dataset_tiny")
SPLIT_FILES = {"train": "im2latex_train_filter.lst", "val": "im2latex_validate_filter.lst", "test": "im2latex_test_filter.lst"}
FORMULAS = "im2latex_formulas.norm.lst"
TOK = TokenTable({"<PAD>": 0, "<START>": 1, "<END>": 2, "<UNK>": 3, "t4": 4})


def fixture():
    return np.load(os.path.join(GOLDEN, "dataset.npz"))


def dataset(split, **kw):
    return D.DeviceDataset(TINY, SPLIT_FILES[split], FORMULAS, TOK, **kw)


def test_split_files_yield_the_references_samples():
    d = fixture()
    for split in ("train", "val", "test"):
        want = json.loads(str(d[f"c1_samples_{split}"]))
        ds = dataset(split)
        assert len(ds) == len(want)
        assert [[n, int(k)] for n, k in zip(ds.image_names, ds.formula_idxs)] == want
    # what the split files hold on purpose: 17 / 14 lines, of which these are skipped
    names = dataset("train").image_names
    assert len(names) == 11 and "only_one_field" not in names and "three" not in names
    assert "p03.png" not in names                                   # index 99 is out of range
    assert "p05.png" not in names                                   # index "x7" is no int
    assert names.count("p09.png") == 1                              # "-1" is skipped, "11" is kept
    assert names.count("p00.png") == 2 and "missing_a.png" in names  # a repeated page, a name with no file
    assert "p09.png" not in dataset("test").image_names             # "1.5" is no int
    assert len(dataset("test")) == 12


def test_the_formulas_file_is_cut_as_text_mode_cuts_it():
    ds = dataset("train")
    with open(os.path.join(TINY, FORMULAS), "r", encoding="utf-8") as f:
        want = [line.strip() for line in f]
    assert len(ds.formulas) == len(want)
    assert [ds.formulas.raw_formula(r) for r in range(len(want))] == want
    assert "" in want and any(len(w.split()) > 150 for w in want)


def test_max_samples_truncates_afterwards():
    full = dataset("train")
    cut = dataset("train", max_samples=3)
    assert cut.image_names == full.image_names[:3] and np.array_equal(cut.formula_idxs, full.formula_idxs[:3])
    assert len(dataset("train", max_samples=0)) == len(full)        # the reference ignores 0
    assert len(dataset("train", max_samples=1000)) == len(full)
    # a page several samples name is stored once
    assert len(full.page_paths) == len(set(full.image_names)) and full.page_rows[0] == full.page_rows[full.image_names.index("p00.png", 1)]


def test_the_three_missing_paths_raise(tmp_path):
    with pytest.raises(FileNotFoundError, match="Split file"):
        D.DeviceDataset(TINY, "no_such.lst", FORMULAS, TOK)
    with pytest.raises(FileNotFoundError, match="Formulas file"):
        D.DeviceDataset(TINY, SPLIT_FILES["train"], "no_such.lst", TOK)
    with pytest.raises(FileNotFoundError, match="Image directory"):
        D.DeviceDataset(TINY, SPLIT_FILES["train"], FORMULAS, TOK, img_dir="no_such_dir")


class Numbers:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("n,batch", [(11, 4), (10, 3), (8, 4), (3, 4)])
def test_index_order_is_the_dataloaders(n, batch):
    """Two consecutive epochs under one torch.manual_seed, shuffled with drop_last and plain, against
    torch.utils.data.DataLoader itself (num_workers = 0); the generator is left in the same state."""
    from torch.utils.data import DataLoader
    for shuffle, drop_last in ((True, True), (True, False), (False, False)):
        torch.manual_seed(77)
        ref = DataLoader(range(n), batch_size=batch, shuffle=shuffle, drop_last=drop_last)
        want = [[b.tolist() for b in ref] for _ in range(2)]
        want_next = torch.rand(1).item()
        torch.manual_seed(77)
        mine = D.DeviceLoader(Numbers(n), batch, shuffle=shuffle, drop_last=drop_last)
        got = [[list(b) for b in mine.index_batches()] for _ in range(2)]
        assert got == want, (shuffle, drop_last)
        assert torch.rand(1).item() == want_next
        assert len(mine) == len(ref) == len(want[0])
        if shuffle and n > 4:
            assert want[0] != want[1]


def test_len_for_both_drop_last_settings():
    assert len(D.DeviceLoader(Numbers(11), 4, drop_last=True)) == 2
    assert len(D.DeviceLoader(Numbers(11), 4, drop_last=False)) == 3
    assert len(D.DeviceLoader(Numbers(12), 4, drop_last=False)) == 3
    assert len(D.DeviceLoader(Numbers(0), 4)) == 0 and list(D.DeviceLoader(Numbers(0), 4, shuffle=True).index_batches()) == []
    with pytest.raises(ValueError):
        D.DeviceLoader(Numbers(3), 0)


def test_create_data_loaders_reads_the_references_keys_and_defaults(tmp_path):
    s = D.loader_settings({"model": {"name": "cnn_lstm", "encoder": {"cnn": {}}}})
    assert s["split_files"] == SPLIT_FILES and s["formulas_file"] == FORMULAS and s["img_dir"] == "img"
    assert s["img_size"] == (64, 800) and s["channels"] == 1 and s["batch_size"] == 128 and s["eval_batch_size"] == 256
    assert s["resident"] is True                                    # the one deliberate difference: the reference's is False
    s = D.loader_settings({"model": {"name": "resnet_lstm", "encoder": {"resnet": {"img_height": 32}}},
                           "data": {"batch_size": 24, "load_in_memory": False, "train_file": "a.lst", "img_dir": "pages"}})
    assert s["channels"] == 3 and s["img_size"] == (32, 800) and s["eval_batch_size"] == 48 and s["resident"] is False
    assert s["split_files"]["train"] == "a.lst" and s["img_dir"] == "pages"
    for bs, mult, cap, want in ((4, 2, 256, 8), (200, 2, 256, 256), (16, 3, 40, 40), (16, 1, 256, 16)):
        s = D.loader_settings({"model": {"encoder": {"cnn": {}}}, "data": {"batch_size": bs, "eval_batch_size_multiplier": mult,
                                                                            "max_eval_batch_size": cap}})
        assert s["eval_batch_size"] == want
    with pytest.raises(ValueError):
        D.loader_settings({"model": {"encoder": {"cnn": {}}}, "data": {"batch_size": 0}})
    # the loaders themselves: no device is touched before the first batch
    cfg = json.loads(str(fixture()["config_c1"]))
    cfg["data"]["data_dir"] = TINY
    loaders = D.create_data_loaders(cfg, TOK, max_samples={"val": 2})
    assert sorted(loaders) == ["test", "train", "val"]
    tr, va, te = loaders["train"], loaders["val"], loaders["test"]
    assert (tr.batch_size, tr.shuffle, tr.drop_last) == (4, True, True)
    assert (va.batch_size, va.shuffle, va.drop_last) == (8, False, False) and (te.batch_size, te.shuffle, te.drop_last) == (8, False, False)
    assert len(va.dataset) == 2 and len(tr) == 2 and len(te) == 2
    assert tr.dataset.formulas is va.dataset.formulas is te.dataset.formulas      # one corpus for the three splits
    assert tr.dataset.img_size == (32, 128) and tr.dataset.channels == 1 and tr.dataset.resident
    assert tr.augment is None
    assert D.create_data_loaders(cfg, TOK, max_samples=None) != {}
    # all splits empty: {}
    os.makedirs(tmp_path / "img")
    for name in list(SPLIT_FILES.values()):
        open(tmp_path / name, "w").close()
    with open(tmp_path / FORMULAS, "w") as f:
        f.write("t4 t4\n")
    assert D.create_data_loaders(dict(cfg, data=dict(cfg["data"], data_dir=str(tmp_path))), TOK) == {}


def test_new_exports_are_declared_bound_and_built():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for sym in ("i2l_tokenize_packed", "i2l_tokenize_packed_workspace_bytes", "i2l_collate_ids", "i2l_gather_ragged_u8"):
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), sym)
    assert _lib.lib().i2l_tokenize_packed_workspace_bytes(1000) >= 4000
    assert _lib.lib().i2l_version() >= 103


def test_evaluate_help_lists_the_options():
    env = dict(os.environ, PYTHONPATH=os.path.join(REPO, "hmer-img2latex_amd"))
    out = subprocess.run([sys.executable, "-m", "img2latex_amd", "evaluate", "--help"], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    for opt in ("checkpoint_path", "data_dir", "--split", "--batch-size", "--num-samples", "--beam-size", "--device", "--output-dir"):
        assert opt in out.stdout
    out = subprocess.run([sys.executable, "-m", "img2latex_amd", "train", "--help"], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and "--data" in out.stdout and "native" in out.stdout
