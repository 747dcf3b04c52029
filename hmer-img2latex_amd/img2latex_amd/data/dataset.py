"""The data set on the device, with the reference's batches (img2latex/data/dataset.py): the formulas file is uploaded
and tokenized ONCE into a ragged id store (i2l_tokenize_packed), the pages of a split are decoded (PIL, a small thread
pool) and uploaded ONCE into one resident uint8 buffer, and a batch then costs one small upload -- its indices, plans and
table requests -- and three launches in front of the unchanged preprocessing chain: i2l_collate_ids (the padded id
matrix), i2l_gather_ragged_u8 (the batch's pages, packed as ``preprocess_batch`` packs them) and the chain itself.

What the batches share with the reference's ``create_data_loaders`` (``num_workers = 0``): the samples a split file
yields (dataset.py:233-269), their order under the same ``torch.manual_seed`` (``DataLoader(shuffle=True)``'s draws from
the default CPU generator, epoch after epoch), the padded id matrix (START formula END, never cut, PAD to the longest
row: dataset.py:333-335, collator :59-66), the images bit for bit (``load_image`` with ``tables="host"``; to fp32
rounding with the default device tables) and the all-zero image of a file that cannot be read (data/utils.py:84-90).
What differs: ``images`` and ``formulas`` are device tensors (``formulas`` int32, the project's id type; the reference
hands out int64 on the CPU), and ``load_in_memory`` -- here ``resident`` -- defaults to true when the key is absent (the
reference's default is false): a data set of im2latex size is a few GB of uint8 pages and fits in HBM many times over.
``resident=False`` is the streaming mode: pages decoded per batch, ``preprocess_batch`` from the host.

Everything that decides WHICH samples form a batch (split parsing, samplers, batch sizes) is host code and needs no GPU;
the device is first touched when a store is built, i.e. by the first batch or by ``DeviceDataset.build()``.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .preprocess import preprocess_batch, preprocess_resident

PAGE_ALIGN = 256                                                     # store pages begin at multiples of this
STATUS_OVERFLOW, STATUS_BAD_OFFSETS, STATUS_BAD_TABLE = 1, 2, 4      # i2l_tokenize_packed's *status bits
COLLATE_ROW_TOO_LONG, COLLATE_BAD_INDEX = 1, 2                       # i2l_collate_ids' *status bits


def _cuda_device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("img2latex_amd: the data set kernels need the ROCm device; there is no CPU fallback")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"img2latex_amd: the data set lives on a ROCm device, not on {dev}")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def read_split(split_path: str, n_formulas: int, max_samples: Optional[int] = None) -> Tuple[List[str], np.ndarray]:
    """dataset.py:233-269: ``(image names, formula indices int64)`` of a split file.  A line counts when it has exactly
    two whitespace-separated fields and the second is an ``int`` in ``[0, n_formulas)``; anything else is skipped.
    ``max_samples`` (positive) truncates afterwards."""
    names, idx = [], []
    with open(split_path, "r", encoding="utf-8") as f:
        for line in f:
            parts = line.strip().split()
            if len(parts) != 2:
                continue
            try:
                k = int(parts[1])
            except ValueError:
                continue
            if 0 <= k < n_formulas:
                names.append(parts[0])
                idx.append(k)
    if max_samples is not None and max_samples > 0:
        names, idx = names[:max_samples], idx[:max_samples]
    return names, np.asarray(idx, dtype=np.int64)


class FormulaStore:
    """The formulas file as ragged token ids on the device.  ``__init__`` reads the file on the host (``vocab.split_lines``:
    text mode's line rule, as ``fit_formulas_file`` cuts it); the first use uploads it once and runs i2l_tokenize_packed
    with START / END (dataset.py:333-335) -- row r of the store is what ``tokenizer.encode(f"{START} {formula_r} {END}")``
    gives.  The offsets come to the host once, so a batch's width needs no device read."""

    def __init__(self, formulas_file: str, tokenizer, device=None):
        from ..training.vocab import split_lines
        self.path, self.tokenizer, self._device = formulas_file, tokenizer, device
        self.raw = np.fromfile(formulas_file, dtype=np.uint8)
        self.raw.tobytes().decode("utf-8")                           # a malformed file raises, as the reference's open() does
        self.line_off = split_lines(self.raw)
        self.ids = None                                              # built by the first use

    def __len__(self) -> int:
        return self.line_off.size - 1

    def raw_formula(self, r: int) -> str:
        """``line.strip()`` of line r (dataset.py:225)."""
        return self.raw[self.line_off[r]:self.line_off[r + 1]].tobytes().decode("utf-8").strip()

    def build(self) -> "FormulaStore":
        if self.ids is not None:
            return self
        from ..training.tokenizer import tokenize_table, upload_packed
        dev = self.device = _cuda_device(self._device)
        table = self.table = tokenize_table(self.tokenizer, dev)
        if table is None:
            raise ValueError("img2latex_amd: this tokenizer has no device vocabulary table (see tokenize_image)")
        rows = len(self)
        lens = np.diff(self.line_off.astype(np.int64))
        bound = int(((lens + 1) // 2).sum()) + 2 * rows              # b bytes hold at most (b + 1) // 2 tokens
        L = _lib.lib()
        with torch.cuda.device(dev):
            text, row_off = upload_packed(self.raw, self.line_off, dev)
            ids = torch.empty((max(bound, 1),), dtype=torch.int32, device=dev)
            meta = torch.empty((2 * (rows + 1) + 2,), dtype=torch.int32, device=dev)     # offsets (int64), then the status
            ws = torch.empty((L.i2l_tokenize_packed_workspace_bytes(rows),), dtype=torch.uint8, device=dev)
            off = meta[:2 * (rows + 1)].view(torch.int64)
            status = meta[2 * (rows + 1):]
            _lib.check(L.i2l_tokenize_packed(text.data_ptr() if text.numel() else None, self.raw.size, row_off.data_ptr(), rows,
                                             table.image.data_ptr(), table.image.numel(), table.unk_id, table.start_id,
                                             table.end_id, 1, ids.data_ptr(), ids.numel(), off.data_ptr(), status.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "tokenize_packed")
            host = meta.cpu()
        st = int(host[-2])
        if st:
            raise RuntimeError(f"img2latex_amd: tokenize_packed reported status {st} on {self.path}")
        self.off_host = host[:2 * (rows + 1)].view(torch.int64).numpy().copy()
        self.lengths = np.diff(self.off_host)
        total = int(self.off_host[-1])
        self.ids = ids[:max(total, 1)].clone()                       # the bound's slack goes back to the allocator
        self.n_ids = total
        self.off = off.clone()
        return self

    def collate(self, indices: Sequence[int]) -> torch.Tensor:
        """Im2LatexCollator's id matrix of the store rows ``indices``: (B, longest) int32 on the device, as
        ``TokenizeTable.collate`` of the same strings returns it.  One index upload, one launch, no device read."""
        self.build()
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size == 0:
            return torch.empty((0, 0), dtype=torch.int32, device=self.device)
        if int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise IndexError("FormulaStore.collate: a formula index outside the file")
        return self.launch(torch.from_numpy(idx).to(self.device), int(self.lengths[idx].max()))[0]

    def launch(self, index: torch.Tensor, width: int, out: Optional[torch.Tensor] = None):
        """i2l_collate_ids on the current stream, no host wait: ``index`` (B int64 on the device) -> ``(ids (B, width)
        int32, status (1))``.  ``out``: a (B, >= width) int32 matrix to write into."""
        self.build()
        B = index.numel()
        if out is None:
            out = torch.empty((B, width), dtype=torch.int32, device=self.device)
        status = torch.zeros((1,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().i2l_collate_ids(self.ids.data_ptr(), self.n_ids, self.off.data_ptr(), len(self),
                                                  index.data_ptr(), B, width, self.table.pad_id, out.data_ptr(), out.stride(0),
                                                  status.data_ptr(), _lib.stream_ptr()), "collate_ids")
        return out[:, :width], status


def decode_page(path: str, channels: int) -> Optional[np.ndarray]:
    """``Image.open`` + the mode rule of ``data.load_image``: ``L`` and ``RGB`` pages are kept as they are (the kernel
    converts), anything else is converted for ``channels``.  None for a file that cannot be opened or decoded."""
    try:
        from PIL import Image
        with Image.open(path) as img:
            if img.mode not in ("L", "RGB"):
                img = img.convert("L" if channels == 1 else "RGB")
            arr = np.array(img)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or arr.size == 0:
            return None
        return np.ascontiguousarray(arr)
    except Exception:                                                # utils.py:84-90: any failure is the zero image
        return None


class PageStore:
    """Decoded pages resident on the device: one uint8 buffer ``pixels``, page r the interleaved (h, w, c) image at
    ``offsets[r]`` (a multiple of 256), ``shapes[r] = (h, w, c)``; ``failed[r]`` marks a file that could not be read (it
    takes no room).  Every path is decoded once, on ``decode_threads`` host threads, and uploaded in chunks of about
    ``chunk_bytes`` through one pinned block, so the host never holds more than a chunk of decoded pages."""

    def __init__(self, paths: Sequence[str], channels: int = 1, device=None, decode_threads: int = 8,
                 chunk_bytes: int = 64 << 20):
        self.device = dev = _cuda_device(device)
        self.paths, self.channels = list(paths), channels
        n = len(self.paths)
        self.shapes = np.ones((n, 3), dtype=np.int64)
        self.offsets = np.zeros(n, dtype=np.int64)
        self.failed = np.zeros(n, dtype=bool)
        self.decode_seconds = self.upload_seconds = 0.0
        import time
        threads = max(1, int(decode_threads))
        group = max(threads * 8, 64)                                 # files handed to the pool at a time
        parts: List[torch.Tensor] = []                               # one device tensor per uploaded chunk
        pinned, used, base, pending = None, 0, 0, []

        def flush():
            nonlocal used, base, pending
            if used == 0:
                return
            t0 = time.perf_counter()
            host = pinned.numpy()
            for r, rel, arr in pending:
                host[rel:rel + arr.size] = arr.reshape(-1)
            with torch.cuda.device(dev):
                part = torch.empty((used,), dtype=torch.uint8, device=dev)
                part.copy_(pinned[:used], non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()         # the pinned block is filled again right away
            parts.append(part)
            base += used
            used, pending = 0, []
            self.upload_seconds += time.perf_counter() - t0

        with ThreadPoolExecutor(max_workers=threads) as pool:
            for g0 in range(0, n, group):
                t0 = time.perf_counter()
                arrays = list(pool.map(lambda p: decode_page(p, channels), self.paths[g0:g0 + group]))
                self.decode_seconds += time.perf_counter() - t0
                for r, arr in enumerate(arrays, start=g0):
                    if arr is None:
                        self.failed[r] = True
                        continue
                    size = (arr.size + PAGE_ALIGN - 1) // PAGE_ALIGN * PAGE_ALIGN
                    if used and used + size > chunk_bytes:
                        flush()
                    if pinned is None or pinned.numel() < max(chunk_bytes, size):
                        pinned = torch.empty((max(chunk_bytes, size),), dtype=torch.uint8).pin_memory()
                    self.shapes[r] = arr.shape if arr.ndim == 3 else arr.shape + (1,)
                    self.offsets[r] = base + used
                    pending.append((r, used, arr))
                    used += size
            flush()
        with torch.cuda.device(dev):
            self.pixels = parts[0] if len(parts) == 1 else (torch.cat(parts) if parts else
                                                             torch.zeros((PAGE_ALIGN,), dtype=torch.uint8, device=dev))

    def __len__(self) -> int:
        return len(self.paths)


class DeviceDataset:
    """One split, Im2LatexDataset's samples (dataset.py:94-343).  ``samples`` of the reference are ``image_names`` /
    ``formula_idxs`` here.  ``resident``: pages decoded and uploaded once (``PageStore``); otherwise decoded per batch.
    ``formula_store``: a ``FormulaStore`` of the same formulas file shared between splits (one corpus upload);
    ``tables``: ``preprocess_batch``'s option (``"host"`` is the Pillow-exact arithmetic)."""

    def __init__(self, data_dir: str, split_file: str, formulas_file: str, tokenizer, img_dir: str = "img",
                 img_size: Tuple[int, int] = (64, 800), channels: int = 1, max_samples: Optional[int] = None,
                 resident: bool = True, device=None, formula_store: Optional[FormulaStore] = None, tables: str = "device",
                 decode_threads: int = 8):
        self.data_dir = str(data_dir)
        self.img_base_dir = os.path.join(self.data_dir, img_dir or "img")
        split_path = os.path.join(self.data_dir, split_file)
        formulas_path = os.path.join(self.data_dir, formulas_file)
        if not os.path.exists(split_path):
            raise FileNotFoundError(f"Split file not found: {split_path}")
        if not os.path.exists(formulas_path):
            raise FileNotFoundError(f"Formulas file not found: {formulas_path}")
        if not os.path.exists(self.img_base_dir):
            raise FileNotFoundError(f"Image directory not found: {self.img_base_dir}")
        self.tokenizer, self.img_size, self.channels = tokenizer, (int(img_size[0]), int(img_size[1])), int(channels)
        self.resident, self.device, self.tables, self.decode_threads = bool(resident), device, tables, int(decode_threads)
        self.formulas = formula_store if formula_store is not None else FormulaStore(formulas_path, tokenizer, device)
        self.image_names, self.formula_idxs = read_split(split_path, len(self.formulas), max_samples)
        # a page that several samples name is stored once
        self.page_paths = list(dict.fromkeys(self.image_names))
        row = {name: r for r, name in enumerate(self.page_paths)}
        self.page_rows = np.fromiter((row[name] for name in self.image_names), dtype=np.int64, count=len(self.image_names))
        self.pages: Optional[PageStore] = None

    def __len__(self) -> int:
        return len(self.image_names)

    def build(self) -> "DeviceDataset":
        """Builds the stores (the first batch does it otherwise)."""
        self.formulas.build()
        self.device = self.formulas.device
        if self.resident and self.pages is None:
            self.pages = PageStore([os.path.join(self.img_base_dir, p) for p in self.page_paths], self.channels, self.device,
                                   self.decode_threads)
        return self

    def batch(self, indices: Sequence[int], augment=None, first_position: int = 0, epoch: int = 0) -> Dict:
        """The collated batch of the samples ``indices`` with Im2LatexCollator's keys.  ``augment``: an ``Augment``,
        applied to the raw pages (the reference's order), keyed by ``first_position + b`` and ``epoch``."""
        self.build()
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        B, (H, W) = idx.size, self.img_size
        rows = self.page_rows[idx]
        positions = first_position + np.arange(B)
        kw = dict(img_size=self.img_size, channels=self.channels, normalize=True, tables=self.tables, augment=augment,
                  epoch=epoch)
        with torch.cuda.device(self.device):
            if self.resident:
                good = np.flatnonzero(~self.pages.failed[rows])
                part = preprocess_resident(self.pages, rows[good], sample_ids=positions[good], **kw)
            else:
                paths = [os.path.join(self.img_base_dir, self.page_paths[r]) for r in rows.tolist()]
                with ThreadPoolExecutor(max_workers=max(1, self.decode_threads)) as pool:
                    arrays = list(pool.map(lambda p: decode_page(p, self.channels), paths))
                good = np.array([b for b, a in enumerate(arrays) if a is not None], dtype=np.int64)
                part = preprocess_batch([arrays[b] for b in good.tolist()], device=self.device, sample_ids=positions[good], **kw)
            if good.size == B:
                images = part
            else:                                                    # utils.py:84-90: the zero image, not normalised
                images = torch.zeros((B, self.channels, H, W), dtype=torch.float32, device=self.device)
                if good.size:
                    images[torch.from_numpy(good).to(self.device)] = part
            fidx = self.formula_idxs[idx]
            formulas = self.formulas.collate(fidx)
        return {"images": images, "formulas": formulas,
                "raw_formulas": [self.formulas.raw_formula(int(k)) for k in fidx],
                "image_paths": [self.image_names[int(i)] for i in idx],
                "formula_idxs": [int(k) for k in fidx]}


class DeviceLoader:
    """``DataLoader(dataset, batch_size, shuffle, drop_last, collate_fn=Im2LatexCollator, num_workers=0)`` over a
    ``DeviceDataset``.  The index order is torch's own: every new iteration first draws DataLoader's base seed from the
    default CPU generator, then -- with ``shuffle`` -- ``RandomSampler`` draws its seed and its permutation, so the same
    ``torch.manual_seed`` gives the reference's batches epoch after epoch.  ``index_batches`` is that order alone and
    needs nothing of the dataset but its length.  ``augment``: see ``DeviceDataset.batch``; the epoch number counts the
    iterations from 0 unless ``set_epoch`` says otherwise."""

    def __init__(self, dataset, batch_size: int, shuffle: bool = False, drop_last: bool = False, augment=None):
        if int(batch_size) <= 0:
            raise ValueError(f"Batch size must be positive, got {batch_size}")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.augment, self.epoch = augment, 0

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def index_batches(self):
        """The batches' sample indices (lists of int), drawing from torch's default generator as DataLoader does."""
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        torch.empty((), dtype=torch.int64).random_()                 # _BaseDataLoaderIter's base seed: drawn, never used
        n = len(self.dataset)
        if n == 0:
            return
        sampler = RandomSampler(range(n)) if self.shuffle else SequentialSampler(range(n))
        yield from BatchSampler(sampler, self.batch_size, self.drop_last)

    def __iter__(self):
        epoch, seen = self.epoch, 0
        self.epoch += 1
        for idx in self.index_batches():
            yield self.dataset.batch(idx, self.augment, seen, epoch)
            seen += len(idx)


def loader_settings(config: Dict) -> Dict:
    """The keys and defaults ``create_data_loaders`` reads (dataset.py:415-557), as one dict: file names, ``img_dir``,
    ``img_size`` and ``channels`` by model type, ``batch_size``, ``eval_batch_size`` = min(batch_size *
    eval_batch_size_multiplier, max_eval_batch_size), ``resident`` (``load_in_memory``; true when absent -- the one
    deliberate difference from the reference, whose default is false)."""
    data, model = config.get("data", {}) or {}, config.get("model", {}) or {}
    name = model.get("name", "cnn_lstm")
    enc = model.get("encoder", {})
    if name == "cnn_lstm" or name.startswith("cnn"):
        e, default_channels = enc["cnn"], 1
    else:
        e, default_channels = enc["resnet"], 3
    batch_size = data.get("batch_size", 128)
    if batch_size <= 0:
        raise ValueError(f"Batch size must be positive, got {batch_size}")
    return {"data_dir": data.get("data_dir"),
            "split_files": {"train": data.get("train_file", "im2latex_train_filter.lst"),
                            "val": data.get("validate_file", "im2latex_validate_filter.lst"),
                            "test": data.get("test_file", "im2latex_test_filter.lst")},
            "formulas_file": data.get("formulas_file", "im2latex_formulas.norm.lst"),
            "img_dir": data.get("img_dir", "img"),
            "img_size": (e.get("img_height", 64), e.get("img_width", 800)),
            "channels": e.get("channels", default_channels),
            "batch_size": batch_size,
            "eval_batch_size": min(batch_size * data.get("eval_batch_size_multiplier", 2), data.get("max_eval_batch_size", 256)),
            "resident": bool(data.get("load_in_memory", True))}


def create_data_loaders(config: Dict, tokenizer, max_samples: Optional[Dict[str, Optional[int]]] = None, device=None,
                        tables: str = "device", augment=None) -> Dict[str, DeviceLoader]:
    """dataset.py:367-557 on the device stores: ``{"train", "val", "test"}`` loaders (``{}`` when all splits are empty),
    ``train`` shuffled with ``drop_last``, the other two at the evaluation batch size.  The three splits share one
    ``FormulaStore``.  No train-time transform unless ``augment`` (an ``Augment``) is given: the reference applies its
    transform to preloaded images only.  Nothing touches the device before the first batch."""
    s = loader_settings(config)
    max_samples = max_samples or {}
    store = FormulaStore(os.path.join(str(s["data_dir"]), s["formulas_file"]), tokenizer, device) \
        if os.path.exists(os.path.join(str(s["data_dir"]), s["formulas_file"])) else None
    datasets = {split: DeviceDataset(s["data_dir"], s["split_files"][split], s["formulas_file"], tokenizer, s["img_dir"],
                                     s["img_size"], s["channels"], max_samples.get(split), s["resident"], device, store, tables)
                for split in ("train", "val", "test")}
    if all(len(ds) == 0 for ds in datasets.values()):
        return {}
    return {split: DeviceLoader(ds, s["batch_size"] if split == "train" else s["eval_batch_size"], shuffle=split == "train",
                                drop_last=split == "train", augment=augment if split == "train" else None)
            for split, ds in datasets.items()}
