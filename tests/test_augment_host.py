"""Train-time augmentation, host side (reference data/dataset.py:486-492; Pillow 12.2 NEAREST rotate + shift).

The numpy restatement of the one-gather warp (tests/augment_ref.py) against Pillow's recorded bytes and, when Pillow is
importable, against the live library; `Augment.params` against the fixture's parameters; the C ABI's new symbols."""
import math
import os
import re

import numpy as np
import pytest

import augment_ref as R
from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd.data import Augment, white_fill
from img2latex_amd.data import augment as A

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def golden():
    d = np.load(f"{GOLDEN}/augment_pillow.npz")
    seen, outs = {}, []
    for (c, si, *_rest) in R.fixture_cases():
        j = seen.get((c, si), 0)
        seen[(c, si)] = j + 1
        outs.append(d[f"out_c{c}_s{si}"][j])
    return d, outs


def test_fixture_covers_the_cases(golden):
    d, outs = golden
    cases = R.fixture_cases()
    assert len(cases) == len(outs) == 2 * 5 * 6 * 3
    assert d["cases"].tolist() == [[c, si, R.SIZES[si][0], R.SIZES[si][1], tx, ty] for (c, si, a, tx, ty) in cases]
    assert d["angles"].tolist() == [a for (_, _, a, _, _) in cases]
    assert str(d["pillow"])
    for (c, si, *_), o in zip(cases, outs):
        assert o.dtype == np.uint8 and o.shape == R.SIZES[si] + ((3,) if c == 3 else ())


def test_restatement_equals_pillow_fixture(golden):
    _, outs = golden
    for (c, si, a, tx, ty), want in zip(R.fixture_cases(), outs):
        h, w = R.SIZES[si]
        got = R.warp_pages(R.fixture_page(c, si), R.coefficients(a, w, h), tx, ty)
        assert np.array_equal(got, want), (c, si, a, tx, ty)


def test_restatement_equals_live_pillow():
    """Freshly drawn pages and parameters, when Pillow is importable (the fixture covers the case that it is not)."""
    pytest.importorskip("PIL")
    aug = Augment(seed=11)
    sizes = [(1, 9), (33, 2), (7, 13), (40, 150), (64, 321), (90, 77)]
    angles, txs, tys = aug.draw(sizes, np.arange(len(sizes)) + 1000, epoch=2)
    for i, (h, w) in enumerate(sizes):
        for c in (1, 3):
            page = R.make_page(700 + 10 * i + c, h, w, c)
            for angle, tx, ty in ((float(angles[i]), int(txs[i]), int(tys[i])), (-4.25, 2, 1), (0.0, -1, 0)):
                got = R.warp_pages(page, R.coefficients(angle, w, h), tx, ty)
                assert np.array_equal(got, R.pillow_warp(page, angle, tx, ty)), (h, w, c, angle, tx, ty)


def test_planar_restatement_is_the_same_gather():
    page = R.make_page(31, 7, 13, 3)
    coef = R.coefficients(-3.999, 13, 7)
    got = R.warp_planes(page.transpose(2, 0, 1).astype(np.float32), coef, 3, -1, (255.0, 255.0, 255.0))
    assert np.array_equal(got.transpose(1, 2, 0), R.warp_pages(page, coef, 3, -1).astype(np.float32))


def test_params_reproduce_the_fixture_coefficients():
    """Pillow's matrix from the fixture's angles: the package's coefficients equal the restatement the fixture pins."""
    for (c, si, a, tx, ty) in R.fixture_cases():
        h, w = R.SIZES[si]
        assert A.coefficients(a, w, h) == R.coefficients(a, w, h), (si, a)
    assert A.coefficients(0.0, 320, 64) == (65536, 0, 32768, 0, 65536, 32768)          # the identity
    assert A.coefficients(-5.0, 9, 1) == A.coefficients(355.0, 9, 1)
    with pytest.raises(ValueError):
        A.coefficients(180.0, 9, 1)

    class Fixed(Augment):                       # the fixture's parameters in place of the random draw
        def draw(self, sizes, sample_ids, epoch=0):
            return np.array([5.0, -3.999]), np.array([3, -6]), np.array([-1, 1])
    cases = R.fixture_cases()

    class All(Augment):                         # every fixture case as one batch: the batched arithmetic is the scalar one
        def draw(self, sizes, sample_ids, epoch=0):
            return (np.array([k[2] for k in cases]), np.array([k[3] for k in cases]), np.array([k[4] for k in cases]))
    p = All().params([R.SIZES[k[1]] for k in cases], np.arange(len(cases)))
    assert [tuple(r) for r in p.tolist()] == [R.coefficients(a, *R.SIZES[si][::-1]) + (tx, ty) for (_, si, a, tx, ty) in cases]
    sizes = [(30 + (7 * k) % 90, 80 + (53 * k) % 700) for k in range(300)]
    drawn = Augment(seed=8)
    angles, tx, ty = drawn.draw(sizes, np.arange(300), 4)
    p = drawn.params(sizes, np.arange(300), 4)
    assert [tuple(r)[:6] for r in p.tolist()] == [R.coefficients(float(a), w, h) for a, (h, w) in zip(angles, sizes)]
    assert p["tx"].tolist() == tx.tolist() and p["ty"].tolist() == ty.tolist()
    p = Fixed().params([(51, 403), (64, 320)], [0, 1])
    assert p.dtype == A.PARAMS_DTYPE and p.dtype.itemsize == 32
    assert tuple(p[0]) == R.coefficients(5.0, 403, 51) + (3, -1)
    assert tuple(p[1]) == R.coefficients(-3.999, 320, 64) + (-6, 1)


def test_params_are_deterministic_and_keyed_by_sample():
    aug = Augment(seed=3)
    sizes = [(51, 403), (64, 320), (33, 2), (128, 800), (64, 320)]
    ids = [7, 1000000007, 3, 42, 8]
    p = aug.params(sizes, ids, epoch=1)
    assert np.array_equal(p, Augment(seed=3).params(sizes, ids, epoch=1))
    # the same sample in another batch, at another position, beside other samples: the same warp
    order = [3, 0, 4]
    q = aug.params([sizes[i] for i in order] + [(9, 9)], [ids[i] for i in order] + [5], epoch=1)
    assert np.array_equal(q[:3], p[order])
    # other epoch, other seed, other sample: other draws
    a0, _, _ = aug.draw(sizes, ids, epoch=1)
    assert not np.array_equal(a0, aug.draw(sizes, ids, epoch=2)[0])
    assert not np.array_equal(a0, Augment(seed=4).draw(sizes, ids, epoch=1)[0])
    assert len(set(a0.tolist())) == len(ids)
    with pytest.raises(ValueError):
        aug.params(sizes, ids[:-1])
    with pytest.raises(ValueError):
        aug.params([(16385, 4)], [0])
    with pytest.raises(ValueError):
        Augment(degrees=90.0)


def test_draws_stay_in_range():
    """|angle| <= degrees; tx = int(round(u)) with |u| <= translate * W, so |tx| <= translate * W wherever rounding cannot
    carry u past it (the fraction of translate * W below one half) and |tx| <= translate * W + 1/2 always.  The draws
    also have to use their range: a generator stuck near 0 would pass the bounds."""
    n = 4000
    for degrees, translate, (h, w) in ((5.0, (0.02, 0.02), (64, 320)), (5.0, (0.02, 0.02), (51, 403)),
                                       (2.5, (0.1, 0.05), (33, 2)), (0.0, (0.0, 0.0), (7, 13))):
        aug = Augment(degrees, translate, seed=5)
        angles, tx, ty = aug.draw([(h, w)] * n, np.arange(n), epoch=0)
        assert float(np.abs(angles).max()) <= degrees
        for t, lim in ((tx, translate[0] * w), (ty, translate[1] * h)):
            assert int(np.abs(t).max()) <= lim + 0.5
            if lim - math.floor(lim) < 0.5:
                assert int(np.abs(t).max()) <= lim
            assert int(t.max()) == -int(t.min()) == int(round(lim)) or lim - math.floor(lim) == 0.5
        if degrees:
            assert angles.min() < -0.99 * degrees and angles.max() > 0.99 * degrees and abs(angles.mean()) < 0.05 * degrees


def test_white_fill():
    assert white_fill(1, True) == (1.0,) and white_fill(1, False) == (1.0,) and white_fill(3, "symmetric") == (1.0, 1.0, 1.0)
    assert white_fill(3, False) == (1.0, 1.0, 1.0)
    one = np.float32(1.0)
    want = tuple(float((one - np.float32(m)) / np.float32(s)) for m, s in ((0.485, 0.229), (0.456, 0.224), (0.406, 0.225)))
    assert white_fill(3, True) == want and all(2.2 < v < 2.7 for v in want)


def test_symbols_declared_and_exported():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for name in ("i2l_affine_nearest_u8", "i2l_affine_nearest_f32"):
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert "typedef struct i2l_affine_params" in header and "dataset.py:486-492" in header
    fields = re.search(r"typedef struct i2l_affine_params \{(.*?)\} i2l_affine_params;", header, flags=re.S).group(1)
    assert re.findall(r"\b(a[0-5]|tx|ty)\b(?=[,;])", fields) == list(A.PARAMS_DTYPE.names)


def test_entry_points_refuse_before_any_launch():
    """Argument checks are host code: they answer without a device (nothing is dereferenced, nothing launched)."""
    L = _lib.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert L.i2l_affine_nearest_u8(p, p + 32, p, p, 1, 16385, 16385, None) == _lib.ERR_UNSUPPORTED
    assert L.i2l_affine_nearest_f32(p, p + 32, p, p, 1, 1, 16385, 4, None) == _lib.ERR_UNSUPPORTED
    assert L.i2l_affine_nearest_f32(p, p + 32, p, p, 1, 1, 4, 16385, None) == _lib.ERR_UNSUPPORTED
    assert L.i2l_affine_nearest_f32(p, p + 32, p, p, 1, 5, 4, 4, None) == _lib.ERR_UNSUPPORTED
    assert L.i2l_affine_nearest_u8(p, p, p, p, 1, 8, 64, None) == _lib.ERR_ARG            # in place
    assert L.i2l_affine_nearest_u8(None, p, p, p, 1, 8, 64, None) == _lib.ERR_ARG
    assert L.i2l_affine_nearest_u8(p, p + 32, p, p, 0, 8, 64, None) == _lib.ERR_ARG
    assert L.i2l_affine_nearest_f32(p, p + 32, p, None, 1, 1, 4, 4, None) == _lib.ERR_ARG
