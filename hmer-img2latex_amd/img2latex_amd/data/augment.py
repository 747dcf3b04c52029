"""Train-time augmentation on the device with the reference's results (img2latex/data/dataset.py:486-492):
``RandomRotation(degrees=5, fill=(255,))`` then ``RandomAffine(degrees=0, translate=(0.02, 0.02), fill=(255,))`` on
the decoded page, before ``load_image``'s chain.  On PIL images both resample NEAREST and end in two Pillow calls,

    rot = page.rotate(angle, resample=NEAREST, expand=False, center=None, fillcolor=white)
    out = rot.transform(rot.size, AFFINE, (1, 0, -tx, 0, 1, -ty), resample=NEAREST, fillcolor=white)

whose 16.16 fixed-point arithmetic (include/img2latex_hip.h, i2l_affine_params) composes into one gather per output
pixel.  The host draws ``angle, tx, ty`` per sample and turns them into Pillow's six coefficients in Python doubles --
``Image.rotate``'s own arithmetic, ``round`` included -- and the HIP kernel (csrc/augment.hip) does the integer rest, so
the warped bytes are Pillow's exactly (tests/golden/augment_pillow.npz).

``preprocess_batch(pages, augment=Augment(), sample_ids=ids, epoch=e)`` is the reference-order path: raw page -> warp ->
convert / LANCZOS resize / pad / normalise, the shift a fraction of the RAW page's size.  ``Augment.tensor`` warps a
batch that is already preprocessed (what the reference's data loaders hand out), the shift then a fraction of the
tensor's size.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib, synth

# struct i2l_affine_params (include/img2latex_hip.h)
PARAMS_DTYPE = np.dtype([("a0", "<i4"), ("a1", "<i4"), ("a2", "<i4"), ("a3", "<i4"), ("a4", "<i4"), ("a5", "<i4"),
                         ("tx", "<i4"), ("ty", "<i4")])
assert PARAMS_DTYPE.itemsize == 32
MAX_SIDE = 16384                     # csrc/augment.hip AFF_MAX_SIDE

_IMAGENET_MEAN, _IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def white_fill(channels: int, normalize=True) -> Tuple[float, ...]:
    """The value of a white (255) pixel per channel after ``preprocess_batch(..., normalize=normalize)``: what the
    reference's fill colour has become in a preprocessed batch.  1.0 for /255 only, for grayscale in [-1, 1] and for
    ``"symmetric"``; ``(1 - mean) / std`` in the kernel's fp32 operations for ImageNet RGB (data/utils.py:77-79)."""
    if channels == 3 and normalize and normalize != "symmetric":
        one = np.float32(1.0)
        return tuple(float((one - np.float32(m)) / np.float32(s)) for m, s in zip(_IMAGENET_MEAN, _IMAGENET_STD))
    return (1.0,) * channels


def coefficients_batch(angles: Sequence[float], sizes: Sequence[Tuple[int, int]]) -> np.ndarray:
    """``Image.rotate(angle, NEAREST, expand=False, center=None)``'s matrix per (h, w) page (PIL/Image.py, the same
    doubles operation by operation) as the six 16.16 coefficients of Pillow's nearest affine: (n, 6) int64.  sin / cos /
    ``round(x, 15)`` run per sample in Python (libm and Python's decimal rounding are what Pillow runs); the products,
    sums and FIX (libImaging/Geometry.c: floor(v * 65536 + 0.5)) are numpy doubles, IEEE operations one by one."""
    m0, m1, m3 = [], [], []
    for a in (np.asarray(angles, np.float64) % 360.0).tolist():
        if a in (90.0, 180.0, 270.0):
            raise ValueError("Pillow rotates by 90 / 180 / 270 degrees with a transpose, not this arithmetic")
        a = -math.radians(a)
        cs, sn = math.cos(a), math.sin(a)
        m0.append(round(cs, 15)), m1.append(round(sn, 15)), m3.append(round(-sn, 15))
    m0, m1, m3 = np.array(m0), np.array(m1), np.array(m3)
    m4 = m0
    hw = np.asarray(sizes, np.float64).reshape(len(m0), 2)
    cx, cy = hw[:, 1] / 2, hw[:, 0] / 2
    m2 = (m0 * -cx + m1 * -cy + 0.0) + cx
    m5 = (m3 * -cx + m4 * -cy + 0.0) + cy
    m = np.stack([m0, m1, m2 + m0 * 0.5 + m1 * 0.5, m3, m4, m5 + m3 * 0.5 + m4 * 0.5], axis=1)
    return np.floor(m * 65536.0 + 0.5).astype(np.int64)


def coefficients(angle: float, w: int, h: int) -> Tuple[int, ...]:
    """``coefficients_batch`` for one (w, h) page, as a tuple of Python ints."""
    return tuple(coefficients_batch([angle], [(h, w)])[0].tolist())


class Augment:
    """The reference's train-time warp: a rotation by an angle uniform in ``[-degrees, degrees]`` about the page's
    centre, then a shift by ``(tx, ty)`` whole pixels, ``tx = int(round(u))`` for ``u`` uniform in
    ``[-translate[0] * W, translate[0] * W]`` and ``ty`` likewise from ``translate[1] * H``; white where the page ends.

    The random stream CANNOT be torch's: torchvision draws from the global torch generator in whatever order the data
    loader's workers reach the samples.  Here every draw comes from ``synth``'s counter-based generator keyed by
    ``(seed, epoch, sample id)``: a sample gets the same warp whatever batch, position or worker it lands in, and a
    run is reproducible from its seed alone.  The distributions are the reference's, the numbers are not."""

    def __init__(self, degrees: float = 5.0, translate: Tuple[float, float] = (0.02, 0.02), seed: int = 0):
        if not 0.0 <= float(degrees) < 90.0:
            raise ValueError("degrees must be in [0, 90)")
        if not all(0.0 <= float(t) <= 1.0 for t in translate) or len(translate) != 2:
            raise ValueError("translate must be two fractions in [0, 1]")
        self.degrees, self.translate, self.seed = float(degrees), (float(translate[0]), float(translate[1])), int(seed)

    def draw(self, sizes: Sequence[Tuple[int, int]], sample_ids: Sequence[int], epoch: int = 0):
        """(angle, tx, ty) per sample: float64, int, int arrays.  ``sizes``: (h, w) per sample."""
        ids = np.asarray(sample_ids, dtype=np.int64)
        if ids.ndim != 1 or len(ids) != len(sizes) or (len(ids) and int(ids.min()) < 0) or epoch < 0:
            raise ValueError("one non-negative sample id per page and a non-negative epoch")
        u = [(synth.keyed_bits(self.seed, "augment", ids, lane=3 * int(epoch) + k) >> np.uint64(11)).astype(np.float64)
             / float(1 << 53) for k in range(3)]                          # [0, 1), exact
        angles = -self.degrees + (2.0 * self.degrees) * u[0]
        mx, my = self.translate
        u1, u2 = u[1].tolist(), u[2].tolist()                     # Python floats: round() below is Python's (half to even)
        tx = [int(round(-mx * w + (2.0 * (mx * w)) * a)) for (h, w), a in zip(sizes, u1)]
        ty = [int(round(-my * h + (2.0 * (my * h)) * a)) for (h, w), a in zip(sizes, u2)]
        return angles, np.array(tx, np.int64), np.array(ty, np.int64)

    def params(self, sizes: Sequence[Tuple[int, int]], sample_ids: Sequence[int], epoch: int = 0) -> np.ndarray:
        """The batch's parameter block, one ``i2l_affine_params`` record per sample (``PARAMS_DTYPE``)."""
        if len(sizes) and max(max(int(h), int(w)) for h, w in sizes) > MAX_SIDE:
            raise ValueError(f"a page side above {MAX_SIDE} is not supported")
        angles, tx, ty = self.draw(sizes, sample_ids, epoch)
        out = np.zeros(len(sizes), PARAMS_DTYPE)
        if len(sizes):
            coef = coefficients_batch(angles, sizes)
            for k in range(6):
                out[f"a{k}"] = coef[:, k]
            out["tx"], out["ty"] = tx, ty
        return out

    @staticmethod
    def pages(pixels: torch.Tensor, plans_ptr: int, params_ptr: int, n: int, max_side: int, max_page_bytes: int) -> torch.Tensor:
        """The warp launch of ``preprocess_batch``: ``pixels`` is the uploaded device block that starts with the ragged
        pages, ``plans_ptr`` / ``params_ptr`` device addresses of the n plans and parameter records.  Returns a second
        pixel buffer with the warped pages at the same offsets."""
        out = torch.empty_like(pixels)
        _lib.check(_lib.lib().i2l_affine_nearest_u8(pixels.data_ptr(), out.data_ptr(), plans_ptr, params_ptr, n, max_side,
                                                    max_page_bytes, _lib.stream_ptr()), "affine_nearest_u8")
        return out

    def tensor(self, x: torch.Tensor, fill: Sequence[float], sample_ids: Optional[Sequence[int]] = None,
               epoch: int = 0) -> torch.Tensor:
        """The same warp of a preprocessed (B, C, H, W) fp32 device batch, ``fill[c]`` (see ``white_fill``) where the
        look-up leaves the image; the shift is a fraction of (H, W).  ``sample_ids`` default to 0 .. B-1."""
        x = _lib.require_gpu(x, "x")
        if x.dim() != 4:
            raise ValueError("x must be (B, C, H, W)")
        b, c, h, w = (int(d) for d in x.shape)
        if len(fill) != c:
            raise ValueError(f"fill needs {c} values, one per channel")
        if b == 0:
            return x.clone()
        ids = np.arange(b) if sample_ids is None else sample_ids
        params = torch.from_numpy(self.params([(h, w)] * b, ids, epoch).view(np.uint8).copy()).to(x.device)
        fill_arr = np.asarray(fill, np.float32)
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().i2l_affine_nearest_f32(x.data_ptr(), out.data_ptr(), params.data_ptr(), fill_arr.ctypes.data,
                                                         b, c, h, w, _lib.stream_ptr()), "affine_nearest_f32")
        return out
