"""A numpy restatement of the train-time warp, independent of the package (shared by the augmentation tests):
Pillow's ``rotate(angle, NEAREST, expand=False, fillcolor=white)`` followed by ``transform(size, AFFINE,
(1, 0, -tx, 0, 1, -ty), NEAREST, fillcolor=white)`` as ONE gather, in Pillow's 16.16 fixed point.  Checked byte for
byte against tests/golden/augment_pillow.npz (and against the installed Pillow when there is one)."""
import math

import numpy as np

from img2latex_amd import synth

# the fixture's cases (tests/golden/make_golden_augment.py draws its pages from the same lists)
SIZES = [(1, 9), (33, 2), (7, 13), (51, 403), (64, 320)]             # (h, w)
ANGLES = [0.0, 5.0, -5.0, 1.2345, -3.999, 0.0001]
SHIFTS = [(0, 0), (3, -1), (-6, 1)]                                  # (tx, ty)
MODES = [1, 3]                                                       # bands: "L", "RGB"


def make_page(seed, h, w, c):
    """Formula-like content, as make_golden_preprocess.py's pages: light page, dark strokes, noise on every pixel."""
    base = synth.uniform(seed, "img", (h, w, c), 0.0, 1.0)
    strokes = synth.uniform(seed + 1, "mask", (h, w, 1), 0.0, 1.0) < 0.18
    img = np.where(strokes, base * 90.0, 200.0 + base * 55.0)
    return np.clip(np.round(img), 0, 255).astype(np.uint8).reshape((h, w) if c == 1 else (h, w, 3))


def fixture_page(c, size_index):
    h, w = SIZES[size_index]
    return make_page(5000 + 100 * c + 10 * size_index, h, w, c)


def fixture_cases():
    """(band count, size index, angle, tx, ty) in the fixture's order."""
    return [(c, si, a, tx, ty) for c in MODES for si in range(len(SIZES)) for a in ANGLES for (tx, ty) in SHIFTS]


def fix(v):
    return math.floor(v * 65536.0 + 0.5)


def coefficients(angle, w, h):
    """PIL/Image.py Image.rotate's matrix in doubles -> Geometry.c's fixed-point coefficients."""
    angle = angle % 360.0
    a = -math.radians(angle)
    m0, m1 = round(math.cos(a), 15), round(math.sin(a), 15)
    m3, m4 = round(-math.sin(a), 15), round(math.cos(a), 15)
    m2 = m0 * (-w / 2) + m1 * (-h / 2) + 0.0
    m5 = m3 * (-w / 2) + m4 * (-h / 2) + 0.0
    m2 += w / 2
    m5 += h / 2
    return (fix(m0), fix(m1), fix(m2 + m0 * 0.5 + m1 * 0.5), fix(m3), fix(m4), fix(m5 + m3 * 0.5 + m4 * 0.5))


def source_index(h, w, coef, tx, ty):
    """(H, W) int64 array: the source pixel y*w + x each output pixel copies, -1 where it takes the fill."""
    a0, a1, a2, a3, a4, a5 = (int(v) for v in coef)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    xs, ys = xs - int(tx), ys - int(ty)
    on = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    xin = (a2 + a0 * xs + a1 * ys) >> 16
    yin = (a5 + a3 * xs + a4 * ys) >> 16
    ok = on & (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    return np.where(ok, yin * w + xin, -1)


def warp_pages(img, coef, tx, ty, fill=255):
    """Interleaved (H, W) or (H, W, C) array; the same fill on every band."""
    h, w = img.shape[:2]
    idx = source_index(h, w, coef, tx, ty)
    flat = img.reshape(h * w, -1)
    out = np.where((idx >= 0).reshape(-1, 1), flat[np.maximum(idx, 0).reshape(-1)], np.asarray(fill, img.dtype))
    return out.reshape(img.shape)


def warp_planes(x, coef, tx, ty, fill):
    """Planar (C, H, W) array, fill[c] per plane."""
    c, h, w = x.shape
    idx = source_index(h, w, coef, tx, ty).reshape(-1)
    out = np.empty_like(x)
    for ch in range(c):
        out[ch] = np.where(idx >= 0, x[ch].reshape(-1)[np.maximum(idx, 0)], np.asarray(fill[ch], x.dtype)).reshape(h, w)
    return out


def pillow_warp(img, angle, tx, ty):
    """The two Pillow calls torchvision makes for a PIL image (needs Pillow)."""
    from PIL import Image
    page = Image.fromarray(img, "L" if img.ndim == 2 else "RGB")
    white = 255 if img.ndim == 2 else (255, 255, 255)
    rot = page.rotate(angle, resample=Image.NEAREST, expand=False, center=None, fillcolor=white)
    out = rot.transform(rot.size, Image.AFFINE, (1, 0, -tx, 0, 1, -ty), resample=Image.NEAREST, fillcolor=white)
    return np.array(out)
