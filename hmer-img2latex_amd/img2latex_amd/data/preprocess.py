"""Image preprocessing on the device with the reference's results (img2latex/data/utils.py:18-110,
data/transforms.py:26-56): mode conversion, aspect-preserving LANCZOS resize to the target height, right-pad /
centre-crop to the target width, /255 and normalisation -- for a whole ragged batch in one pair of kernel launches,
bit-identical to `load_image` (Pillow 12.2 semantics; golden vectors in tests/golden/preprocess.npz).

File decoding stays with PIL on the host (it is I/O + entropy decoding, not part of the hot path); everything after
`Image.open` runs in HIP.  Since r04 that includes the resampling tables: `i2l_resample_coeffs_device` builds the
Lanczos / bicubic weights of a whole batch on the device from its size list (the host's double-precision arithmetic
repeated operation by operation; `tables="host"` keeps the library's host helper -- libm, the arithmetic Pillow itself
runs -- with its device-resident cache), and the ragged pages are gathered into the pinned upload block by
`i2l_pack_host` on several host threads.  Per batch the host now walks the shapes, fills one record array and uploads.
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import _lib


# struct i2l_resize_plan (include/img2latex_hip.h) as a numpy record: a whole batch of plans is ONE array
PLAN_DTYPE = np.dtype([("src_offset", "<i8"), ("tmp_offset", "<i8"), ("bh_offset", "<i8"), ("kh_offset", "<i8"),
                       ("bv_offset", "<i8"), ("kv_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("src_c", "<i4"),
                       ("new_w", "<i4"), ("ybox_first", "<i4"), ("tmp_rows", "<i4"), ("need_h", "<i4"), ("need_v", "<i4"),
                       ("kh_ksize", "<i4"), ("kv_ksize", "<i4")])
assert PLAN_DTYPE.itemsize == 88

# How far an axis may shrink.  Output sample x sums up to 2 * support * in / out source samples ("taps"), held in a table
# row of ksize = 2 * ceil(support * in / out) + 1 weights (support 3 for LANCZOS, 2 for BICUBIC).  The host builder
# (i2l_resample_coeffs) keeps one sample's weights in 512 doubles on its stack and returns I2L_ERR_UNSUPPORTED for more
# (LANCZOS past ~85x, BICUBIC past ~128x); the device builder has no such buffer and is held to rows of 1024 weights
# (LANCZOS ~170x, BICUBIC ~255x).  Between the two, ``tables="device"`` resamples and ``tables="host"`` refuses.
HOST_MAX_TAPS = 512
DEVICE_MAX_KSIZE = 1024


class _TablePool:
    """Resampling tables resident on the device, one per (source size, target size, filter), shared by every image
    and every batch that needs them: a batch only pays (threaded, in the library's host helper) for sizes it has not
    seen before, and uploads nothing else but its pixels and plans.  Grow-only up to `capacity` int32 elements, then
    reset.  One pool per device."""

    def __init__(self, device: torch.device, capacity: int = 16 << 20):
        self.device, self.capacity = device, capacity
        self.tables = torch.empty((capacity,), dtype=torch.int32, device=device)
        self.used = 0
        self.index = {}            # (in, out, filter) -> (bounds offset, weights offset, ksize, first, last)

    def lookup(self, keys):
        """Makes every key resident; returns nothing (read self.index)."""
        missing = [k for k in dict.fromkeys(keys) if k not in self.index]
        if not missing:
            return
        L = _lib.lib()
        ks = [L.i2l_resample_ksize(f, a, b) for (a, b, f) in missing]
        if min(ks) <= 0:
            raise ValueError("cannot resample an empty axis")
        sizes = [b * (2 + k) for (a, b, f), k in zip(missing, ks)]
        total = int(sum(sizes))
        if total > self.capacity:
            raise ValueError("resampling tables of one batch exceed the table pool")
        if self.used + total > self.capacity:                     # full: start over (tables of earlier batches are
            torch.cuda.current_stream(self.device).synchronize()  # dropped once nothing in flight reads them)
            self.index.clear()
            self.used = 0
            return self.lookup(keys)
        offs = np.zeros(len(missing), np.int64)
        offs[1:] = np.cumsum(sizes[:-1])
        host = torch.empty((total,), dtype=torch.int32).pin_memory()
        for flt in sorted({f for (_, _, f) in missing}):
            sel = [i for i, (_, _, f) in enumerate(missing) if f == flt]
            ins = np.array([missing[i][0] for i in sel], np.int32)
            outs = np.array([missing[i][1] for i in sel], np.int32)
            o = np.ascontiguousarray(offs[sel])
            rc = L.i2l_resample_coeffs_batch(flt, len(sel), ins.ctypes.data, outs.ctypes.data, o.ctypes.data,
                                             host.data_ptr(), min(16, os.cpu_count() or 1))
            if rc == _lib.ERR_UNSUPPORTED:                        # nothing of this request has entered the pool
                raise ValueError(f"tables=\"host\" builds at most {HOST_MAX_TAPS} taps per output sample and an axis of "
                                 f"this batch shrinks by more than that allows; tables=\"device\" takes table rows of "
                                 f"up to {DEVICE_MAX_KSIZE} weights")
            _lib.check(rc, "resample_coeffs_batch")
        hv = host.numpy()
        for (key, k, off) in zip(missing, ks, offs.tolist()):
            b = key[1]
            first = int(hv[off])
            last = int(hv[off + 2 * (b - 1)] + hv[off + 2 * (b - 1) + 1])
            self.index[key] = (self.used + off, self.used + off + 2 * b, k, first, last)
        self.tables[self.used:self.used + total].copy_(host, non_blocking=True)
        # the pinned staging block must outlive the asynchronous copy
        torch.cuda.current_stream(self.device).synchronize()
        self.used += total


_POOLS = {}
_STAGING = {}


def _pool(dev: torch.device) -> _TablePool:
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _POOLS:
        _POOLS[key] = _TablePool(dev)
    return _POOLS[key]


def _staging(dev: torch.device, nbytes: int):
    """Two pinned uint8 blocks per device, used alternately; a block is reused only after the copy that last read it
    has finished (its event)."""
    key = (dev.type, dev.index)
    st = _STAGING.setdefault(key, {"bufs": [None, None], "events": [None, None], "next": 0})
    i = st["next"]
    st["next"] = i ^ 1
    if st["events"][i] is not None:
        st["events"][i].synchronize()
    if st["bufs"][i] is None or st["bufs"][i].numel() < nbytes:
        st["bufs"][i] = torch.empty((max(nbytes, 1 << 20) * 5 // 4,), dtype=torch.uint8).pin_memory()
    return st, i, st["bufs"][i]


def _ksizes(flt: int, ins: np.ndarray, outs: np.ndarray) -> np.ndarray:
    """i2l_resample_ksize for arrays (preprocess.hip: (int)ceil(support * max(1, (double)(float)in / out)) * 2 + 1)."""
    fs = np.maximum(ins.astype(np.float32).astype(np.float64) / outs, 1.0)
    return np.ceil((2.0 if flt == _lib.FILTER_BICUBIC else 3.0) * fs).astype(np.int64) * 2 + 1


def _extents(flt: int, ins: np.ndarray, outs: np.ndarray):
    """First source sample of output 0 and one past the last source sample of output out - 1 (what the vertical pass
    needs of the horizontal one): the bounds arithmetic of i2l_resample_coeffs for those two outputs, in the same doubles."""
    scale = ins.astype(np.float32).astype(np.float64) / outs
    support = (2.0 if flt == _lib.FILTER_BICUBIC else 3.0) * np.maximum(scale, 1.0)
    c0 = (0 + 0.5) * scale
    first = np.maximum(np.trunc(c0 - support + 0.5), 0.0)
    cl = (outs - 1 + 0.5) * scale
    last = np.minimum(np.trunc(cl + support + 0.5), ins.astype(np.float64))
    return first.astype(np.int64), last.astype(np.int64)


def _check_options(channels: int, resample: str, normalize, tables: str, device):
    """The options preprocess_batch and preprocess_resident share: (filter, normalize code, device)."""
    if tables not in ("device", "host"):
        raise ValueError("tables must be 'device' or 'host'")
    flt = {"lanczos": _lib.FILTER_LANCZOS, "bicubic": _lib.FILTER_BICUBIC}[resample]
    normalize = 2 if normalize == "symmetric" else int(bool(normalize))
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    if not torch.cuda.is_available():
        raise RuntimeError("img2latex_amd: the preprocessing kernels need the ROCm device; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return flt, normalize, dev


class _BatchPlan:
    """What the planning part hands to the uploading and the launching part: the shapes (h, w, c), the plan records, the
    table request (None with ``tables="host"``: the plans then point into the device's table pool ``pool``), the page
    sizes and their packed offsets, and the temporary rows."""
    __slots__ = ("n", "h", "w", "c", "new_w", "plans", "tab_req", "pool", "sizes", "src_off", "tmp_rows", "tmp_bytes")


def _plan_batch(shapes: np.ndarray, out_h: int, channels: int, keep_aspect: bool, out_w: int, flt: int, tables: str,
                dev: torch.device) -> _BatchPlan:
    """The part that plans: (n, 3) int64 shapes (h, w, c) -> plans and table requests.  Touches the device only with
    ``tables="host"`` (new sizes enter the table pool).  Call under ``torch.cuda.device(dev)``."""
    P = _BatchPlan()
    n = P.n = shapes.shape[0]
    h, w, c = shapes[:, 0], shapes[:, 1], shapes[:, 2]
    P.h, P.w, P.c = h, w, c
    if int(h.min()) == 0 or int(w.min()) == 0:
        raise ValueError("empty image")
    # transforms.py:33-36: int(round(target_h * (w / h))) -- Python's round() and numpy's both round half to even
    new_w = np.round(out_h * (w / h)).astype(np.int64) if keep_aspect else np.full(n, out_w, np.int64)
    if int(new_w.min()) <= 0:
        bad = int(np.argmin(new_w))
        raise ValueError(f"image {bad} ({int(h[bad])}x{int(w[bad])}) collapses to zero width at height {out_h}")
    P.new_w, P.pool = new_w, None
    if tables == "host":
        pool = P.pool = _pool(dev)
        hkeys = [(int(a), int(b), flt) for a, b in zip(w, new_w)]
        vkeys = [(int(a), out_h, flt) for a in h]
        pool.lookup(hkeys + vkeys)
        ent_h = np.array([pool.index[k] for k in hkeys], np.int64)
        ent_v = np.array([pool.index[k] for k in vkeys], np.int64)
        P.tab_req = None
    else:
        # 2n tables (n horizontal w -> new_w, n vertical h -> out_h) laid out back to back in one per-batch buffer
        t_in = np.concatenate([w, h]).astype(np.int32)
        t_out = np.concatenate([new_w, np.full(n, out_h, np.int64)]).astype(np.int32)
        ks = _ksizes(flt, t_in, t_out)
        if int(ks.max()) > DEVICE_MAX_KSIZE:
            raise ValueError(f"an axis of this batch shrinks by more than table rows of {DEVICE_MAX_KSIZE} weights allow "
                             f"(it needs {int(ks.max())})")
        t_size = t_out.astype(np.int64) * (2 + ks)
        t_off = np.zeros(2 * n, np.int64)
        t_off[1:] = np.cumsum(t_size[:-1])
        first, last = _extents(flt, t_in[n:], t_out[n:])
        ent_h = np.stack([t_off[:n], t_off[:n] + 2 * t_out[:n], ks[:n]], axis=1)
        ent_v = np.stack([t_off[n:], t_off[n:] + 2 * t_out[n:], ks[n:], first, last], axis=1)
        P.tab_req = (t_in, t_out, t_off, int(t_size.sum()), int(t_out.max()))
    plans = P.plans = np.zeros(n, PLAN_DTYPE)
    sizes = P.sizes = h * w * c
    src_off = P.src_off = np.zeros(n, np.int64)
    src_off[1:] = np.cumsum(sizes[:-1])
    need_h = new_w != w
    tmp_rows = P.tmp_rows = np.where(need_h, ent_v[:, 4] - ent_v[:, 3], 0)
    tmp_bytes = P.tmp_bytes = (tmp_rows * new_w * channels + 255) // 256 * 256
    tmp_off = np.zeros(n, np.int64)
    tmp_off[1:] = np.cumsum(tmp_bytes[:-1])
    plans["src_offset"], plans["tmp_offset"] = src_off, tmp_off
    plans["bh_offset"], plans["kh_offset"], plans["kh_ksize"] = ent_h[:, 0], ent_h[:, 1], ent_h[:, 2]
    plans["bv_offset"], plans["kv_offset"], plans["kv_ksize"] = ent_v[:, 0], ent_v[:, 1], ent_v[:, 2]
    plans["src_h"], plans["src_w"], plans["src_c"], plans["new_w"] = h, w, c, new_w
    plans["ybox_first"] = np.where(need_h, ent_v[:, 3], 0)
    plans["tmp_rows"] = tmp_rows
    plans["need_h"], plans["need_v"] = need_h, h != out_h
    return P


def _upload_batch(dev: torch.device, P: _BatchPlan, flats, warp, upload_stream, tail: np.ndarray = None):
    """The part that uploads: ONE pinned block -> ONE device block ``d_all``, laid out as [pixels | plans | table
    requests | warp parameters | tail], every part at a multiple of 256 bytes.  ``flats``: the host pages, packed into the
    pixel region (i2l_pack_host); None: the pixel region is left for the device to fill and only what lies behind it is
    uploaded.  ``tail``: any further uint8 block (the resident path's gather list).  Returns ``(d_all, p0, p1, p2, p3)``:
    the byte offsets of the plans, the table requests, the warp parameters and the tail."""
    n = P.n
    total_px = int(P.sizes.sum())
    plan_bytes = n * PLAN_DTYPE.itemsize
    req_bytes = 0 if P.tab_req is None else 2 * n * (4 + 4 + 8)
    p0 = (total_px + 255) // 256 * 256
    p1 = (p0 + plan_bytes + 255) // 256 * 256
    p2 = p3 = None
    if warp is not None:                                          # the warp parameters: behind everything else
        p2 = (p1 + req_bytes + 255) // 256 * 256
        req_bytes = p2 - p1 + warp.nbytes
    if tail is not None:
        p3 = (p1 + req_bytes + 255) // 256 * 256
        req_bytes = p3 - p1 + tail.nbytes
    first = 0 if flats is not None else p0                        # the first byte that is uploaded
    st, slot, pinned = _staging(dev, p1 + req_bytes + 256)
    host = pinned.numpy()
    if flats is not None:
        # the pages -> one pinned block, on several host threads (one thread copies 16 MB in ~3 ms)
        ptrs = np.fromiter((a.__array_interface__["data"][0] for a in flats), dtype=np.uint64, count=n)
        _lib.check(_lib.lib().i2l_pack_host(ptrs.ctypes.data, P.sizes.ctypes.data, P.src_off.ctypes.data, n, pinned.data_ptr(),
                                            min(4, os.cpu_count() or 1)), "pack_host")      # 16 MB: 0.39 / 0.18 / 0.25 ms on 1 / 4 / 8 threads
    host[p0:p0 + plan_bytes] = P.plans.view(np.uint8)
    if P.tab_req is not None:
        t_in, t_out, t_off, t_total, t_max_out = P.tab_req
        host[p1:p1 + 8 * n] = t_in.view(np.uint8)
        host[p1 + 8 * n:p1 + 16 * n] = t_out.view(np.uint8)
        host[p1 + 16 * n:p1 + 32 * n] = t_off.view(np.uint8)
    if warp is not None:
        host[p2:p2 + warp.nbytes] = warp.view(np.uint8)
    if tail is not None:
        host[p3:p3 + tail.nbytes] = tail
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.stream(upload_stream if upload_stream is not None else cur):
        # allocated under the uploading stream: memory the caching allocator hands out there has no pending work
        # of the compute stream on it, so the copy need not wait for the previous batch's kernels
        d_all = torch.empty((p1 + req_bytes,), dtype=torch.uint8, device=dev)
        d_all[first:].copy_(pinned[first:p1 + req_bytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
    st["events"][slot] = ev
    if upload_stream is not None:
        cur.wait_event(ev)
        d_all.record_stream(cur)
    return d_all, p0, p1, p2, p3


def _launch_batch(dev: torch.device, P: _BatchPlan, d_all: torch.Tensor, p0: int, p1: int, p2, flt: int, channels: int,
                  out_h: int, out_w: int, normalize: int, augment) -> torch.Tensor:
    """The part that launches, on the current stream: the tables (``tables="device"``), the optional warp, then
    i2l_preprocess_images on the pixel region of ``d_all``."""
    n = P.n
    max_tmp_px = int((P.tmp_rows * P.new_w).max())
    ws = torch.empty((max(int(P.tmp_bytes.sum()), 16),), dtype=torch.uint8, device=dev)
    out = torch.empty((n, channels, out_h, out_w), dtype=torch.float32, device=dev)
    if P.tab_req is None:
        tab = P.pool.tables
    else:
        t_total, t_max_out = P.tab_req[3], P.tab_req[4]
        tab = torch.empty((max(t_total, 4),), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().i2l_resample_coeffs_device(flt, 2 * n, d_all.data_ptr() + p1, d_all.data_ptr() + p1 + 8 * n,
                                                         d_all.data_ptr() + p1 + 16 * n, tab.data_ptr(), t_max_out,
                                                         _lib.stream_ptr()), "resample_coeffs_device")
    pages = d_all
    if augment is not None:
        pages = augment.pages(d_all[:p0], d_all.data_ptr() + p0, d_all.data_ptr() + p2, n, int(max(P.h.max(), P.w.max())),
                              int(P.sizes.max()))
    _lib.check(_lib.lib().i2l_preprocess_images(pages.data_ptr(), d_all.data_ptr() + p0, tab.data_ptr(), n,
                                                max_tmp_px, channels, out_h, out_w, normalize,
                                                ws.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "preprocess_images")
    return out


def _warp_params(augment, P: _BatchPlan, sample_ids, epoch: int):
    if augment is None:
        return None
    return augment.params(list(zip(P.h.tolist(), P.w.tolist())), np.arange(P.n) if sample_ids is None else sample_ids, epoch)


def preprocess_batch(images: Sequence[np.ndarray], img_size: Tuple[int, int] = (64, 800), channels: int = 1,
                     normalize=True, device=None, keep_aspect: bool = True, resample: str = "lanczos",
                     upload_stream=None, tables: str = "device", augment=None, sample_ids=None,
                     epoch: int = 0) -> torch.Tensor:
    """`load_image` for already decoded images: uint8 arrays (H, W) ["L"] or (H, W, 3) ["RGB"], any sizes.
    Returns (n, channels, img_size[0], img_size[1]) float32 on the device.

    ``keep_aspect=False, resample="bicubic", normalize="symmetric"`` is the PIL.Image branch of the reference's
    ``Predictor._prepare_image`` instead (predictor.py:432-451): ``image.resize((W, H))`` with Pillow's default filter
    straight to the target size, then ``x / 255 * 2 - 1`` on every channel.

    Host work per batch: one pass over the shapes, one record array of plans, ONE packed copy of the pixels into pinned
    memory (i2l_pack_host, several threads) and one asynchronous upload (pixels + plans + size list); the resampling
    tables are built on the device (``tables="device"``, i2l_resample_coeffs_device).  ``tables="host"``: the library's
    host helper (libm: Pillow's own arithmetic) with look-ups in a device-resident pool, new sizes computed on the host's
    cores.  ``upload_stream``: run the upload on a side stream (the kernels, on the current stream, wait for it) so that
    it overlaps whatever the current stream is still doing.

    ``augment``: an ``Augment`` (data/augment.py) warps every page first, as the reference's training split does
    (dataset.py:486-492: rotation, then shift, NEAREST, white fill), keyed by ``sample_ids`` (default 0 .. n-1) and
    ``epoch``.  Its parameter block rides in the same upload and ONE more launch (i2l_affine_nearest_u8) writes the
    warped pages to a second pixel buffer, on which the unchanged plans and tables then run.  ``None``: nothing changes."""
    flt, normalize, dev = _check_options(channels, resample, normalize, tables, device)
    out_h, out_w = int(img_size[0]), int(img_size[1])
    n = len(images)
    if n == 0:
        return torch.empty((0, channels, out_h, out_w), dtype=torch.float32, device=dev)
    # one pass over the Python objects, as little per image as the interpreter allows (256 pages: ~0.15 ms)
    u8 = np.dtype(np.uint8)
    try:
        ok = all(a.dtype is u8 or a.dtype == u8 for a in images)
        dims = [a.shape if a.ndim == 3 else a.shape + (1,) for a in images]
    except AttributeError:
        ok = False
    if not ok or any(len(d) != 3 or (d[2] != 3 and d[2] != 1) for d in dims) or any(a.ndim == 3 and a.shape[2] == 1 for a in images):
        raise TypeError("images must be uint8 arrays of shape (H, W) or (H, W, 3)")
    flats = [a if a.flags.c_contiguous else np.ascontiguousarray(a) for a in images]
    shapes = np.array(dims, np.int64).reshape(n, 3)
    with torch.cuda.device(dev):
        P = _plan_batch(shapes, out_h, channels, keep_aspect, out_w, flt, tables, dev)
        d_all, p0, p1, p2, _ = _upload_batch(dev, P, flats, _warp_params(augment, P, sample_ids, epoch), upload_stream)
        return _launch_batch(dev, P, d_all, p0, p1, p2, flt, channels, out_h, out_w, normalize, augment)


def preprocess_resident(store, indices, img_size: Tuple[int, int] = (64, 800), channels: int = 1, normalize=True,
                        keep_aspect: bool = True, resample: str = "lanczos", upload_stream=None, tables: str = "device",
                        augment=None, sample_ids=None, epoch: int = 0) -> torch.Tensor:
    """``preprocess_batch`` for pages that already live on the device: ``store`` is a ``PageStore`` (data/dataset.py),
    ``indices`` the batch's store rows (repeats allowed, none of a failed page).  The planning and the launches are
    ``preprocess_batch``'s own; what differs is the upload: only the small block -- plans, table requests, warp
    parameters and the gather list (three int64 per page) -- crosses the bus, and ONE more launch (i2l_gather_ragged_u8)
    copies the pages from the store into the batch's pixel region, at the offsets the plans already name.  The result
    is bit-identical to ``preprocess_batch`` on the same pages."""
    dev = store.device
    flt, normalize, dev = _check_options(channels, resample, normalize, tables, dev)
    out_h, out_w = int(img_size[0]), int(img_size[1])
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    n = idx.size
    if n == 0:
        return torch.empty((0, channels, out_h, out_w), dtype=torch.float32, device=dev)
    if int(idx.min()) < 0 or int(idx.max()) >= len(store) or bool(store.failed[idx].any()):
        raise IndexError("preprocess_resident: an index outside the store, or of a page that failed to decode")
    shapes = np.ascontiguousarray(store.shapes[idx])
    with torch.cuda.device(dev):
        P = _plan_batch(shapes, out_h, channels, keep_aspect, out_w, flt, tables, dev)
        gather = np.concatenate([store.offsets[idx], P.sizes, P.src_off]).astype(np.int64)
        d_all, p0, p1, p2, p3 = _upload_batch(dev, P, None, _warp_params(augment, P, sample_ids, epoch), upload_stream,
                                              gather.view(np.uint8))
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        g = d_all.data_ptr() + p3
        _lib.check(_lib.lib().i2l_gather_ragged_u8(store.pixels.data_ptr(), store.pixels.numel(), g, g + 8 * n, n,
                                                   int(P.sizes.max()), d_all.data_ptr(), p0, g + 16 * n, status.data_ptr(),
                                                   _lib.stream_ptr()), "gather_ragged_u8")
        return _launch_batch(dev, P, d_all, p0, p1, p2, flt, channels, out_h, out_w, normalize, augment)


def load_image(image_path: str, img_size: Tuple[int, int] = (64, 800), channels: int = 1,
               normalize: bool = True) -> torch.Tensor:
    """utils.py:18-90 with the reference's signature and defaults.  PIL only opens / decodes the file; the tensor
    (channels, H, W) is produced on the device (the reference returns the same values on the CPU).  Like the
    reference, any failure yields a zero image."""
    try:
        from PIL import Image
        img = Image.open(image_path)
        if channels == 1:
            arr = np.array(img if img.mode in ("L", "RGB") else img.convert("L"))
        else:
            arr = np.array(img if img.mode in ("L", "RGB") else img.convert("RGB"))
        return preprocess_batch([arr], img_size, channels, normalize)[0]
    except Exception:                                             # utils.py:84-90
        dev = torch.device("cuda", torch.cuda.current_device())
        return torch.zeros((channels, img_size[0], img_size[1]), device=dev)


def resize_bilinear(t: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """``torch.nn.functional.interpolate(t, size, mode="bilinear", align_corners=False)`` of a (..., H, W) fp32 device
    tensor on the HIP kernel (the tensor branch of Predictor._prepare_image, predictor.py:483-491)."""
    if not t.is_cuda:
        raise RuntimeError("img2latex_amd: resize_bilinear needs a tensor on the ROCm device; there is no CPU fallback")
    t = t.to(torch.float32).contiguous()
    out = torch.empty(t.shape[:-2] + (int(size[0]), int(size[1])), dtype=torch.float32, device=t.device)
    planes = int(np.prod(t.shape[:-2])) if t.dim() > 2 else 1
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().i2l_resize_bilinear_f32(t.data_ptr(), out.data_ptr(), planes, t.shape[-2], t.shape[-1],
                                                      int(size[0]), int(size[1]), _lib.stream_ptr()), "resize_bilinear_f32")
    return out


def batch_convert_for_resnet(batch_tensor: torch.Tensor) -> torch.Tensor:
    """utils.py:93-110: gray -> RGB by repeating the channel."""
    if batch_tensor.shape[1] == 3:
        return batch_tensor
    return batch_tensor.repeat(1, 3, 1, 1)
