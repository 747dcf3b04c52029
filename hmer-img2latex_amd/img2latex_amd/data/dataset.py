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


class _PinnedUploader:
    """Host pages -> device parts through one pinned block of about ``chunk_bytes``: ``add`` places a page at the next
    multiple of PAGE_ALIGN and returns its offset in the concatenation of ``parts``; the block is uploaded when the next
    page would not fit.  ``append`` takes a part that is on the device already (pages decoded there)."""

    def __init__(self, dev: torch.device, chunk_bytes: int):
        self.dev, self.chunk_bytes = dev, chunk_bytes
        self.parts: List[torch.Tensor] = []                          # one device tensor per uploaded chunk
        self.pinned, self.used, self.base, self.pending = None, 0, 0, []
        self.seconds = 0.0

    def add(self, arr: np.ndarray) -> int:
        size = (arr.size + PAGE_ALIGN - 1) // PAGE_ALIGN * PAGE_ALIGN
        if self.used and self.used + size > self.chunk_bytes:
            self.flush()
        if self.pinned is None or self.pinned.numel() < max(self.chunk_bytes, size):
            self.pinned = torch.empty((max(self.chunk_bytes, size),), dtype=torch.uint8).pin_memory()
        offset = self.base + self.used
        self.pending.append((self.used, arr))
        self.used += size
        return offset

    def flush(self) -> None:
        if self.used == 0:
            return
        import time
        t0 = time.perf_counter()
        host = self.pinned.numpy()
        for rel, arr in self.pending:
            host[rel:rel + arr.size] = arr.reshape(-1)
        with torch.cuda.device(self.dev):
            part = torch.empty((self.used,), dtype=torch.uint8, device=self.dev)
            part.copy_(self.pinned[:self.used], non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()        # the pinned block is filled again right away
        self.parts.append(part)
        self.base += self.used
        self.used, self.pending = 0, []
        self.seconds += time.perf_counter() - t0

    def append(self, part: torch.Tensor) -> int:
        """-> the offset of ``part`` (its size a multiple of PAGE_ALIGN) in the concatenation."""
        self.flush()
        offset = self.base
        self.parts.append(part)
        self.base += part.numel()
        return offset

    def pixels(self) -> torch.Tensor:
        self.flush()
        with torch.cuda.device(self.dev):
            if len(self.parts) == 1:
                return self.parts[0]
            return torch.cat(self.parts) if self.parts else torch.zeros((PAGE_ALIGN,), dtype=torch.uint8, device=self.dev)


_PNG_IMAGE = np.dtype([("z_off", "<i8"), ("z_len", "<i8"), ("pal_off", "<i8"), ("out_off", "<i8"), ("width", "<i4"),
                       ("height", "<i4"), ("colour_type", "<i4"), ("pal_n", "<i4"), ("channels", "<i4"), ("reserved", "<i4")])


def _read_png(path: str):
    """The file's ``PngInfo`` when the device may decode it, else None (unreadable, not a PNG, not eligible)."""
    from .png import parse_png
    try:
        with open(path, "rb") as f:
            return parse_png(f.read())
    except OSError:
        return None


def _png_launch(infos, channels: int, dev: torch.device, seconds: Dict[str, float]):
    """One i2l_png_decode launch over the parsed files ``infos``: ``(part, offsets within part, status)``.  The streams
    and palettes go up compressed in one block; the pages are laid out at multiples of PAGE_ALIGN from their IHDR."""
    import time
    t0 = time.perf_counter()
    n = len(infos)
    blobs, cols, z_at, out_at, filtered = [], [], 0, 0, 0
    for info in infos:
        z_off, pal_off, pal_n = z_at, -1, 0
        blobs.append(info.idat)
        z_at += len(info.idat)
        if info.colour_type == 3:
            pal_off, pal_n = z_at, len(info.palette) // 3
            blobs.append(info.palette)
            z_at += len(info.palette)
        oc = info.out_channels(channels)
        cols.append((z_off, len(info.idat), pal_off, out_at, info.width, info.height, info.colour_type, pal_n, oc, 0))
        out_at += (info.width * info.height * oc + PAGE_ALIGN - 1) // PAGE_ALIGN * PAGE_ALIGN
        filtered += info.filtered_bytes
    desc = np.array(cols, dtype=_PNG_IMAGE)                          # struct i2l_png_image, field for field
    z_host = torch.frombuffer(bytearray(b"".join(blobs)) or bytearray(1), dtype=torch.uint8)
    L = _lib.lib()
    with torch.cuda.device(dev):
        z = z_host.to(dev)
        torch.cuda.current_stream(dev).synchronize()
        t1 = time.perf_counter()
        part = torch.empty((out_at,), dtype=torch.uint8, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        ws = torch.empty((L.i2l_png_decode_workspace_bytes(n, filtered),), dtype=torch.uint8, device=dev)
        _lib.check(L.i2l_png_decode(z.data_ptr(), z_at, desc.ctypes.data, n, part.data_ptr(), out_at, status.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "png_decode")
        status_host = status.cpu().numpy()                           # waits for the launch
    t2 = time.perf_counter()
    seconds["upload"] += t1 - t0
    seconds["launch"] += t2 - t1
    return part, desc["out_off"].astype(np.int64), status_host


def decode_pages_device(paths: Sequence[str], channels: int = 1, device=None, decode_threads: int = 8,
                        chunk_bytes: int = 64 << 20, seconds: Optional[Dict[str, float]] = None):
    """The pages of ``paths`` decoded ON THE DEVICE: ``(pixels, offsets, shapes, failed)`` with ``PageStore``'s meaning.
    The files are read and parsed on ``decode_threads`` host threads (``png.parse_png``); the eligible ones go up
    compressed and are inflated, unfiltered and converted by i2l_png_decode, one launch per about ``chunk_bytes`` of
    pages.  Every other file -- and every file whose device status is not 0 -- takes ``decode_page`` and the pinned
    upload, so ``failed`` is decided by ``decode_page`` alone and every page holds the bytes it returns.
    ``seconds``: a dict that receives the time spent in "read_parse", "upload", "launch" and "fallback"."""
    import time
    dev = _cuda_device(device)
    paths = list(paths)
    n = len(paths)
    shapes = np.ones((n, 3), dtype=np.int64)
    offsets = np.zeros(n, dtype=np.int64)
    failed = np.zeros(n, dtype=bool)
    seconds = seconds if seconds is not None else {}
    for key in ("read_parse", "upload", "launch", "fallback"):
        seconds.setdefault(key, 0.0)
    threads = max(1, int(decode_threads))
    group = max(threads * 64, 1024)                                  # files read and parsed at a time
    up = _PinnedUploader(dev, chunk_bytes)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for g0 in range(0, n, group):
            t0 = time.perf_counter()
            infos = list(pool.map(_read_png, paths[g0:g0 + group]))
            seconds["read_parse"] += time.perf_counter() - t0
            rows = [g0 + k for k, info in enumerate(infos) if info is not None]
            fallback = [g0 + k for k, info in enumerate(infos) if info is None]
            k0 = 0
            while k0 < len(rows):                                    # launches of about chunk_bytes of pages
                k1, size = k0, 0
                while k1 < len(rows) and (k1 == k0 or size < chunk_bytes):
                    info = infos[rows[k1] - g0]
                    size += info.width * info.height * info.out_channels(channels)
                    k1 += 1
                chunk = [infos[r - g0] for r in rows[k0:k1]]
                part, rel, status = _png_launch(chunk, channels, dev, seconds)
                base = up.append(part)
                for r, info, o, st in zip(rows[k0:k1], chunk, rel, status):
                    if st:
                        fallback.append(r)                           # its room in the part stays unused
                    else:
                        shapes[r] = (info.height, info.width, info.out_channels(channels))
                        offsets[r] = base + int(o)
                k0 = k1
            if fallback:
                fallback.sort()
                t0 = time.perf_counter()
                arrays = list(pool.map(lambda r: decode_page(paths[r], channels), fallback))
                for r, arr in zip(fallback, arrays):
                    if arr is None:
                        failed[r] = True
                        continue
                    shapes[r] = arr.shape if arr.ndim == 3 else arr.shape + (1,)
                    offsets[r] = up.add(arr)
                up.flush()
                seconds["fallback"] += time.perf_counter() - t0     # PIL and the pinned upload
    return up.pixels(), offsets, shapes, failed


class PageStore:
    """Decoded pages resident on the device: one uint8 buffer ``pixels``, page r the interleaved (h, w, c) image at
    ``offsets[r]`` (a multiple of 256), ``shapes[r] = (h, w, c)``; ``failed[r]`` marks a file that could not be read (it
    takes no room).  ``decode="host"``: every path is decoded once, on ``decode_threads`` host threads, and uploaded in
    chunks of about ``chunk_bytes`` through one pinned block, so the host never holds more than a chunk of decoded
    pages.  ``decode="device"``: ``decode_pages_device`` -- the files go up compressed and i2l_png_decode writes the
    pages; same ``shapes``, ``failed`` and page bytes, while the offsets may differ."""

    def __init__(self, paths: Sequence[str], channels: int = 1, device=None, decode_threads: int = 8,
                 chunk_bytes: int = 64 << 20, decode: str = "host"):
        if decode not in ("host", "device"):
            raise ValueError(f"PageStore: decode={decode!r}: expected \"host\" or \"device\"")
        self.device = dev = _cuda_device(device)
        self.paths, self.channels, self.decode = list(paths), channels, decode
        n = len(self.paths)
        self.decode_seconds = self.upload_seconds = 0.0
        if decode == "device":
            self.seconds: Dict[str, float] = {}
            self.pixels, self.offsets, self.shapes, self.failed = decode_pages_device(
                self.paths, channels, dev, decode_threads, chunk_bytes, self.seconds)
            self.decode_seconds = self.seconds["read_parse"] + self.seconds["launch"] + self.seconds["fallback"]
            self.upload_seconds = self.seconds["upload"]
            return
        self.shapes = np.ones((n, 3), dtype=np.int64)
        self.offsets = np.zeros(n, dtype=np.int64)
        self.failed = np.zeros(n, dtype=bool)
        import time
        threads = max(1, int(decode_threads))
        group = max(threads * 8, 64)                                 # files handed to the pool at a time
        up = _PinnedUploader(dev, chunk_bytes)
        with ThreadPoolExecutor(max_workers=threads) as pool:
            for g0 in range(0, n, group):
                t0 = time.perf_counter()
                arrays = list(pool.map(lambda p: decode_page(p, channels), self.paths[g0:g0 + group]))
                self.decode_seconds += time.perf_counter() - t0
                for r, arr in enumerate(arrays, start=g0):
                    if arr is None:
                        self.failed[r] = True
                        continue
                    self.shapes[r] = arr.shape if arr.ndim == 3 else arr.shape + (1,)
                    self.offsets[r] = up.add(arr)
        self.pixels = up.pixels()
        self.upload_seconds = up.seconds

    def __len__(self) -> int:
        return len(self.paths)


class DeviceDataset:
    """One split, Im2LatexDataset's samples (dataset.py:94-343).  ``samples`` of the reference are ``image_names`` /
    ``formula_idxs`` here.  ``resident``: pages decoded and uploaded once (``PageStore``); otherwise decoded per batch.
    ``formula_store``: a ``FormulaStore`` of the same formulas file shared between splits (one corpus upload);
    ``tables``: ``preprocess_batch``'s option (``"host"`` is the Pillow-exact arithmetic).  ``decode``: where the page
    files are decoded, ``"host"`` (PIL) or ``"device"`` (``decode_pages_device``), for the resident store and for the
    per-batch route alike."""

    def __init__(self, data_dir: str, split_file: str, formulas_file: str, tokenizer, img_dir: str = "img",
                 img_size: Tuple[int, int] = (64, 800), channels: int = 1, max_samples: Optional[int] = None,
                 resident: bool = True, device=None, formula_store: Optional[FormulaStore] = None, tables: str = "device",
                 decode_threads: int = 8, decode: str = "host"):
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
        if decode not in ("host", "device"):
            raise ValueError(f"DeviceDataset: decode={decode!r}: expected \"host\" or \"device\"")
        self.decode = decode
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
                                   self.decode_threads, decode=self.decode)
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
            elif self.decode == "device":                             # the batch's files decoded on the device, then as resident
                paths = [os.path.join(self.img_base_dir, self.page_paths[r]) for r in rows.tolist()]
                pages = PageStore(paths, self.channels, self.device, self.decode_threads, decode="device")
                good = np.flatnonzero(~pages.failed)
                part = preprocess_resident(pages, good, sample_ids=positions[good], **kw)
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
    deliberate difference from the reference, whose default is false), ``decode`` (this package's key ``data.decode``:
    "host" or "device", see ``PageStore``)."""
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
            "resident": bool(data.get("load_in_memory", True)),
            "decode": data.get("decode", "host")}


def create_data_loaders(config: Dict, tokenizer, max_samples: Optional[Dict[str, Optional[int]]] = None, device=None,
                        tables: str = "device", augment=None, decode: Optional[str] = None) -> Dict[str, DeviceLoader]:
    """dataset.py:367-557 on the device stores: ``{"train", "val", "test"}`` loaders (``{}`` when all splits are empty),
    ``train`` shuffled with ``drop_last``, the other two at the evaluation batch size.  The three splits share one
    ``FormulaStore``.  No train-time transform unless ``augment`` (an ``Augment``) is given: the reference applies its
    transform to preloaded images only.  ``decode``: "host" or "device" (``PageStore``); None reads the config key
    ``data.decode`` (default "host").  Nothing touches the device before the first batch."""
    s = loader_settings(config)
    decode = s["decode"] if decode is None else decode
    max_samples = max_samples or {}
    store = FormulaStore(os.path.join(str(s["data_dir"]), s["formulas_file"]), tokenizer, device) \
        if os.path.exists(os.path.join(str(s["data_dir"]), s["formulas_file"])) else None
    datasets = {split: DeviceDataset(s["data_dir"], s["split_files"][split], s["formulas_file"], tokenizer, s["img_dir"],
                                     s["img_size"], s["channels"], max_samples.get(split), s["resident"], device, store, tables,
                                     decode=decode)
                for split in ("train", "val", "test")}
    if all(len(ds) == 0 for ds in datasets.values()):
        return {}
    return {split: DeviceLoader(ds, s["batch_size"] if split == "train" else s["eval_batch_size"], shuffle=split == "train",
                                drop_last=split == "train", augment=augment if split == "train" else None)
            for split, ds in datasets.items()}
