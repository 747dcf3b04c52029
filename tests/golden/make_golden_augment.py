#!/usr/bin/env python3
"""Golden vectors for the train-time augmentation (reference img2latex/data/dataset.py:486-492).  torchvision's
RandomRotation + RandomAffine on a PIL image end in two Pillow calls (tests/augment_ref.py `pillow_warp`); this script
makes exactly those two calls with the INSTALLED Pillow on pages drawn from `synth` and stores the parameters and
Pillow's output bytes in tests/golden/augment_pillow.npz.  The pages themselves are not stored: the tests redraw them.

All outputs of one (mode, size) sit in one array and the archive is LZMA-compressed (numpy reads it like any .npz):
the 18 warps of a page are rearrangements of the same bytes, which a long-window coder stores once.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py
"""
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(REPO, "hmer-img2latex_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import PIL  # noqa: E402

import augment_ref as R  # noqa: E402


def main():
    cases = R.fixture_cases()
    out = {"pillow": np.array(PIL.__version__),
           "cases": np.array([[c, si, R.SIZES[si][0], R.SIZES[si][1], tx, ty] for (c, si, a, tx, ty) in cases], np.int32),
           "angles": np.array([a for (_, _, a, _, _) in cases], np.float64)}
    groups = {}
    for (c, si, a, tx, ty) in cases:
        groups.setdefault((c, si), []).append(R.pillow_warp(R.fixture_page(c, si), a, tx, ty))
    for (c, si), outs in groups.items():
        out[f"out_c{c}_s{si}"] = np.stack(outs)                   # (angles x shifts, H, W[, 3]) in case order
    path = os.path.join(HERE, "augment_pillow.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as zf:
        for name, arr in out.items():
            with zf.open(name + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asarray(arr), allow_pickle=False)
    print("cases", len(cases), "pillow", PIL.__version__, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
