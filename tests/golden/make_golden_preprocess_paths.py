#!/usr/bin/env python3
"""Golden vectors for every path of the preprocessing kernels (csrc/preprocess.hip), beside preprocess.npz's twelve pages.

Aspect-keeping path: generated pages are written as lossless PNG files and pushed through the REAL
`img2latex.data.utils.load_image` (reference, imported unmodified; make_golden_preprocess puts it on the path behind the
inert torchvision shim).  Fixed-size path (the PIL.Image branch of the reference's Predictor._prepare_image,
predictor.py:427-447): Pillow itself, `Image.fromarray(page).convert(mode).resize((W, H), filter)` -- the call that branch
makes -- and the uint8 result is stored; the `/255`, `*2-1` step is float32 arithmetic the test applies.

tests/golden/preprocess_paths.npz stores the generator arguments of every page and the outputs, and the Pillow version:
    aspect_cases  (n, 8) int32: seed, h, w, source channels, target H, target W, output channels, normalize
    aspect{i}     float32 (output channels, H, W): what load_image returned (the zero image where the width collapses)
    fixed_cases   (m, 8) int32: seed, h, w, source channels, target H, target W, output channels, filter
                  (PIL.Image.Resampling: 1 LANCZOS, 3 BICUBIC)
    fixed{i}      uint8 (H, W) or (H, W, 3): the resized image

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_preprocess_paths.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_preprocess as G  # noqa: E402  (the reference on the path, its load_image, the page generator)

import numpy as np  # noqa: E402
import PIL  # noqa: E402
from PIL import Image  # noqa: E402

MODES = [(1, 1), (3, 3), (3, 1), (1, 3)]                   # (source channels, output channels)
TARGET = (24, 56)
LANCZOS, BICUBIC = int(Image.Resampling.LANCZOS), int(Image.Resampling.BICUBIC)

# aspect-keeping path, LANCZOS, neighbours differ in the passes they need: no resampling (exact, pad, even crop of 34, odd
# crop of 35), vertical pass only (new width = width), both passes (up + pad, down + pad, odd crop of 47), half-to-even
# widths (1.5 -> 2, 2.5 -> 2, 3.5 -> 4) and the width that collapses (0.5 -> 0)
ASPECT_RAW = [(24, 56), (24, 13)]                          # also stored with normalize=False
ASPECT = [(24, 56), (25, 3), (11, 20), (24, 13), (23, 5), (70, 150), (24, 90), (48, 3), (70, 300), (24, 91), (48, 5),
          (48, 7), (48, 1)]
# fixed-size path: neither pass, vertical only, horizontal only, both (down one way and up the other), one-pixel axes
FIXED = [(24, 56), (37, 56), (24, 90), (70, 13), (11, 56), (24, 13), (5, 300), (1, 1), (1, 9), (9, 1), (2, 3)]
TINY_TARGETS = [(1, 1), (7, 5)]
TINY_SOURCES = [(5, 7), (9, 1)]
# more taps per output sample (600 -> 5: 600) than the host table builder takes; (h, w, source channels, output channels)
LIMIT_TARGET = (5, 8)
LIMIT = [(600, 8, 1, 1), (600, 9, 3, 1)]
SEED0 = 20000


def aspect_cases():
    rows = [(h, w, sc, TARGET, oc, 1) for (h, w) in ASPECT for (sc, oc) in MODES]
    rows += [(h, w, sc, TARGET, oc, 0) for (h, w) in ASPECT_RAW for (sc, oc) in MODES]
    return [(SEED0 + 10 * i,) + r for i, r in enumerate(rows)]


def fixed_cases():
    rows = [(h, w, sc, TARGET, oc, f) for f in (LANCZOS, BICUBIC) for (h, w) in FIXED for (sc, oc) in MODES]
    rows += [(h, w, sc, t, oc, f) for f in (LANCZOS, BICUBIC) for t in TINY_TARGETS for (h, w) in TINY_SOURCES
             for (sc, oc) in MODES]
    rows += [(h, w, sc, LIMIT_TARGET, oc, f) for f in (LANCZOS, BICUBIC) for (h, w, sc, oc) in LIMIT]
    return [(SEED0 + 5000 + 10 * i,) + r for i, r in enumerate(rows)]


def flat(cases):
    return np.array([[s, h, w, sc, th, tw, oc, last] for (s, h, w, sc, (th, tw), oc, last) in cases], np.int32)


def main():
    a_cases, f_cases = aspect_cases(), fixed_cases()
    out = {"aspect_cases": flat(a_cases), "fixed_cases": flat(f_cases), "pillow": np.array(PIL.__version__)}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (seed, h, w, sc, size, oc, norm) in enumerate(a_cases):
            path = os.path.join(tmp, f"im{i}.png")
            Image.fromarray(G.make_image(seed, h, w, sc)).save(path)
            out[f"aspect{i}"] = G.load_image(path, img_size=size, channels=oc, normalize=bool(norm)).numpy().astype(np.float32)
    for i, (seed, h, w, sc, (th, tw), oc, flt) in enumerate(f_cases):
        img = Image.fromarray(G.make_image(seed, h, w, sc)).convert("L" if oc == 1 else "RGB")
        out[f"fixed{i}"] = np.array(img.resize((tw, th), Image.Resampling(flt)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "preprocess_paths.npz")
    np.savez_compressed(path, **out)
    print("aspect", len(a_cases), "fixed", len(f_cases), "pillow", PIL.__version__, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
