"""Every path of the preprocessing kernels (csrc/preprocess.hip) against Pillow (reference data/utils.py:18-90,
data/transforms.py:26-56, training/predictor.py:427-447; Pillow 12.2), beside test_preprocess.py's page-like cases.

tests/golden/preprocess_paths.npz (make_golden_preprocess_paths.py) holds what the reference's `load_image` and Pillow's own
`convert(mode).resize((W, H), filter)` returned for small pages chosen by the branch they take: which of the two passes
run, the four mode conversions, pad / exact / crop, the three normalisations, both filters, one- to seven-pixel axes,
half-to-even widths, and a kernel longer than the host table builder takes.  DESIGN.md ("What pins preprocessing") maps
the branches to the tests below.

CPU: the oracle restatement against the fixture and against live Pillow, the entries' argument checks.
GPU: ragged batches in both orders with device- and host-built tables, the device table builder at 1 .. 7 samples and
past its grid, a second trip of every grid-stride loop.  Every comparison is `np.array_equal`."""
import functools

import numpy as np
import pytest
import torch

from helpers import GOLDEN
import preprocess_oracle as PO
from img2latex_amd import _lib
from test_preprocess import make_image

MODES = [(1, 1), (3, 3), (3, 1), (1, 3)]                   # (source channels, output channels)
TARGET = (24, 56)
LANCZOS, BICUBIC = 1, 3                                    # _lib.FILTER_* = PIL.Image.Resampling
FILTER_NAME = {LANCZOS: "lanczos", BICUBIC: "bicubic"}
# aspect-keeping path (h, w) -> (24, 56), in the fixture's order: neighbours need different passes
ASPECT = [(24, 56), (25, 3), (11, 20), (24, 13), (23, 5), (70, 150), (24, 90), (48, 3), (70, 300), (24, 91), (48, 5),
          (48, 7), (48, 1)]
ASPECT_NEW_W = [56, 3, 44, 13, 5, 51, 90, 2, 103, 91, 2, 4, 0]     # int(round(24 * (w / h))): half to even
ASPECT_RAW = [(24, 56), (24, 13)]                          # also with normalize=False
# fixed-size path (h, w) -> (24, 56): neither pass, vertical, horizontal, both, ..., one-pixel axes
FIXED = [(24, 56), (37, 56), (24, 90), (70, 13), (11, 56), (24, 13), (5, 300), (1, 1), (1, 9), (9, 1), (2, 3)]
TINY_TARGETS = [(1, 1), (7, 5)]
TINY_SOURCES = [(5, 7), (9, 1)]
LIMIT_TARGET = (5, 8)
LIMIT = [(600, 8, 1, 1), (600, 9, 3, 1)]                   # 600 -> 5 LANCZOS: 600 taps, the host builder stops at 512
# a second trip of the pixel kernels' grid-stride loops (1024 blocks of 256 threads = 262 144 elements per trip):
# (h, w, c) -> target, fixed-size.  330 * 800 = 264 000 intermediate pixels; 336 * 784 = 263 424 output pixels
TRIPS = [((330, 50, 3), (64, 800), 3), ((20, 30, 1), (336, 784), 1)]
GRID_ELEMS = 1024 * 256
SENTINEL = -2 ** 31 + 7                                    # no bound (>= 0) and no 22-bit weight


@functools.lru_cache(maxsize=None)
def page(seed, h, w, c):
    a = make_image(seed, h, w, c)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def golden():
    """(aspect rows, fixed rows): (seed, h, w, source channels, (H, W), output channels, normalize | filter, output)."""
    d = np.load(f"{GOLDEN}/preprocess_paths.npz")
    rows = lambda key: [(s, h, w, sc, (th, tw), oc, last, d[f"{key}{i}"])
                        for i, (s, h, w, sc, th, tw, oc, last) in enumerate(d[f"{key}_cases"].tolist())]
    return rows("aspect"), rows("fixed"), str(d["pillow"])


def symmetric(u8):
    """predictor.py:439-447 on the resized uint8 image: (C, H, W) float32, x / 255 * 2 - 1 on every channel."""
    t = (u8[None] if u8.ndim == 2 else np.transpose(u8, (2, 0, 1))).astype(np.float32)
    return t / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)


def oracle_fixed(img, size, oc, flt):
    return PO.resize_lanczos_u8(PO.convert_mode(img, oc), size[1], size[0], FILTER_NAME[flt])


@functools.lru_cache(maxsize=None)
def trip_expected(k, flt):
    """The oracle's result for loop-trip page k, computed once and shared by the CPU and the GPU test."""
    (h, w, c), size, oc = TRIPS[k]
    out = oracle_fixed(page(30000 + k, h, w, c), size, oc, flt)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_holds_the_branch_matrix(golden):
    aspect, fixed, pillow = golden
    assert pillow
    want = [(h, w, sc, TARGET, oc, 1) for (h, w) in ASPECT for (sc, oc) in MODES]
    want += [(h, w, sc, TARGET, oc, 0) for (h, w) in ASPECT_RAW for (sc, oc) in MODES]
    assert [r[1:7] for r in aspect] == want
    want = [(h, w, sc, TARGET, oc, f) for f in (LANCZOS, BICUBIC) for (h, w) in FIXED for (sc, oc) in MODES]
    want += [(h, w, sc, t, oc, f) for f in (LANCZOS, BICUBIC) for t in TINY_TARGETS for (h, w) in TINY_SOURCES
             for (sc, oc) in MODES]
    want += [(h, w, sc, LIMIT_TARGET, oc, f) for f in (LANCZOS, BICUBIC) for (h, w, sc, oc) in LIMIT]
    assert [r[1:7] for r in fixed] == want
    assert len({r[0] for r in aspect + fixed}) == len(aspect) + len(fixed) == 184
    for (_, h, w, sc, (th, tw), oc, _, out) in aspect:
        assert out.dtype == np.float32 and out.shape == (oc, th, tw)
    for (_, h, w, sc, (th, tw), oc, _, out) in fixed:
        assert out.dtype == np.uint8 and out.shape == ((th, tw) if oc == 1 else (th, tw, 3))
    # the widths the aspect rule gives, the passes they ask for, and what is left of the page: nothing drifts unnoticed
    assert [int(round(TARGET[0] * (w / h))) for (h, w) in ASPECT] == ASPECT_NEW_W
    passes = {(nw != w, h != TARGET[0]) for (h, w), nw in zip(ASPECT, ASPECT_NEW_W) if nw}
    assert passes == {(False, False), (False, True), (True, True)}       # a horizontal pass alone cannot keep the aspect
    assert {(w != TARGET[1], h != TARGET[0]) for (h, w) in FIXED} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {np.sign(nw - TARGET[1]) for nw in ASPECT_NEW_W} == {-1, 0, 1}
    assert sorted((nw - TARGET[1]) for nw in ASPECT_NEW_W if nw > TARGET[1]) == [34, 35, 47]
    for (seed, h, w, sc, *_rest) in aspect + fixed:                     # the conversions are under test: bands differ
        if sc == 3 and h * w > 1:
            img = page(seed, h, w, sc)
            assert not np.array_equal(img[..., 0], img[..., 1]) and not np.array_equal(img[..., 1], img[..., 2])


def test_oracle_equals_the_fixture(golden):
    """The restatement of Pillow (oracle/preprocess_oracle.py) on all 184 entries, bit for bit: it is then the expected
    value wherever an output is too large to store."""
    aspect, fixed, _ = golden
    for (seed, h, w, sc, size, oc, norm, want) in aspect:
        if int(round(size[0] * (w / h))) == 0:                          # the reference's resize raises: the zero image
            assert not want.any(), (h, w)
            continue
        got = PO.load_image_from_array(page(seed, h, w, sc), size, oc, bool(norm))
        assert got.dtype == np.float32 and np.array_equal(got, want), (h, w, sc, oc, norm)
    for (seed, h, w, sc, size, oc, flt, want) in fixed:
        assert np.array_equal(oracle_fixed(page(seed, h, w, sc), size, oc, flt), want), (h, w, sc, size, oc, flt)


def test_oracle_equals_live_pillow_at_the_loop_trip_pages():
    """The two pages whose outputs are not stored: `convert(mode).resize((W, H), filter)` of the installed Pillow."""
    Image = pytest.importorskip("PIL.Image")
    for k, ((h, w, c), size, oc) in enumerate(TRIPS):
        for flt in (LANCZOS, BICUBIC):
            img = Image.fromarray(page(30000 + k, h, w, c)).convert("L" if oc == 1 else "RGB")
            want = np.array(img.resize((size[1], size[0]), Image.Resampling(flt)))
            assert np.array_equal(trip_expected(k, flt), want), (k, flt)


def test_loop_trip_pages_pass_one_grid():
    """What makes TRIPS a second trip, from the launch arithmetic of i2l_preprocess_images."""
    from img2latex_amd.data.preprocess import _extents
    (h, w, _), (th, tw), _ = TRIPS[0]
    for flt in (LANCZOS, BICUBIC):
        first, last = _extents(flt, np.array([h]), np.array([th]))
        assert GRID_ELEMS < int(last[0] - first[0]) * tw == 264000
    (_, _, _), (th, tw), _ = TRIPS[1]
    assert GRID_ELEMS < th * tw == 263424


def test_host_builder_refuses_past_its_limit():
    """i2l_resample_coeffs keeps at most 512 taps per output sample: 600 -> 5 LANCZOS needs 600 and is refused (its first and
    last output samples, 420 taps each, are within the limit: the middle ones decide); the same axis with BICUBIC (481) is built, equal to the oracle's."""
    L = _lib.lib()
    ks = L.i2l_resample_ksize(LANCZOS, 600, 5)
    assert ks == 721
    bounds, kk = np.zeros((5, 2), np.int32), np.zeros((5, ks), np.int32)
    assert L.i2l_resample_coeffs(LANCZOS, 600, 5, bounds.ctypes.data, kk.ctypes.data) == _lib.ERR_UNSUPPORTED
    ks, bo, ko = PO.precompute_coeffs(600, 0.0, 600.0, 5, "bicubic")
    assert L.i2l_resample_ksize(BICUBIC, 600, 5) == ks == 481 and int(bo[:, 1].max()) == 480
    bounds, kk = np.zeros((5, 2), np.int32), np.zeros((5, ks), np.int32)
    assert L.i2l_resample_coeffs(BICUBIC, 600, 5, bounds.ctypes.data, kk.ctypes.data) == 0
    assert np.array_equal(bounds, bo) and np.array_equal(kk, ko)
    from img2latex_amd.data.preprocess import HOST_MAX_TAPS              # the documented number is the library's
    for in_size, rc in ((HOST_MAX_TAPS, 0), (HOST_MAX_TAPS + 1, _lib.ERR_UNSUPPORTED)):
        ks = L.i2l_resample_ksize(BICUBIC, in_size, 1)                  # one output sample sums the whole axis
        bounds, kk = np.zeros((1, 2), np.int32), np.zeros((1, ks), np.int32)
        assert L.i2l_resample_coeffs(BICUBIC, in_size, 1, bounds.ctypes.data, kk.ctypes.data) == rc
        assert rc or bounds.tolist() == [[0, in_size]]


def test_entries_refuse_before_any_launch():
    """Argument checks are host code: they answer without a device (nothing is dereferenced, nothing launched)."""
    L = _lib.lib()
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data

    def images(pixels=p, plans=p, tables=p, n=1, max_tmp_px=0, out_c=1, out_h=4, out_w=4, workspace=p, out=p):
        return L.i2l_preprocess_images(pixels, plans, tables, n, max_tmp_px, out_c, out_h, out_w, 1, workspace, out, None)
    for null in ("pixels", "plans", "tables", "out"):
        assert images(**{null: None}) == _lib.ERR_ARG, null
    for bad in (dict(n=0), dict(n=-1), dict(n=65536), dict(out_c=2), dict(out_c=0), dict(out_c=4), dict(out_h=0),
                dict(out_h=-3), dict(out_w=0), dict(out_w=-3)):
        assert images(**bad) == _lib.ERR_ARG, bad
    assert images(max_tmp_px=1, workspace=None) == _lib.ERR_WORKSPACE
    assert images(max_tmp_px=1, workspace=None, out_c=2) == _lib.ERR_ARG            # the arguments are judged first

    def tables(flt=LANCZOS, n=1, ins=p, outs=p, offs=p, tab=p, max_out=8):
        return L.i2l_resample_coeffs_device(flt, n, ins, outs, offs, tab, max_out, None)
    for bad in (dict(n=0), dict(n=-1), dict(n=65536), dict(max_out=0), dict(max_out=-1), dict(ins=None), dict(outs=None),
                dict(offs=None), dict(tab=None)):
        assert tables(**bad) == _lib.ERR_ARG, bad
    for flt in (0, 2, 9, -1):
        assert tables(flt=flt) == _lib.ERR_UNSUPPORTED, flt


# ------------------------------------------------------------------------------------------------------------ GPU
def run_batch(rows, wants, tables=("device", "host"), **kw):
    """One ragged batch of fixture rows, as listed and reversed, per table builder: every image equals its `wants`."""
    from img2latex_amd.data import preprocess_batch
    size, oc = rows[0][4], rows[0][5]
    for tab in tables:
        for order in (range(len(rows)), range(len(rows) - 1, -1, -1)):
            imgs = [page(*rows[i][:4]) for i in order]
            out = preprocess_batch(imgs, size, oc, tables=tab, **kw)
            assert tuple(out.shape) == (len(rows), oc) + tuple(size) and out.dtype == torch.float32
            got = out.cpu().numpy()
            for j, i in enumerate(order):
                assert np.array_equal(got[j], wants[i]), (tab, order[0] == 0, rows[i][1:7])


def fixed_group(fixed, size, oc, flt):
    rows = [r for r in fixed if r[4] == size and r[5] == oc and r[6] == flt]
    return rows, [symmetric(r[7]) for r in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("oc", [1, 3])
@pytest.mark.parametrize("normalize", [True, False])
def test_aspect_path_batches(golden, oc, normalize):
    """`load_image`'s path: both source modes of every page side by side, neighbours needing different passes; pad (white
    / Pillow's red), exact width, even and odd crops; normalize 0 and 1 at one and three channels."""
    rows = [r for r in golden[0] if r[5] == oc and bool(r[6]) == normalize and int(round(r[4][0] * (r[2] / r[1]))) > 0]
    assert len(rows) == (24 if normalize else 4) and {r[3] for r in rows} == {1, 3}
    run_batch(rows, [r[7] for r in rows], normalize=normalize)


@pytest.mark.gpu
@pytest.mark.parametrize("oc", [1, 3])
@pytest.mark.parametrize("flt", [LANCZOS, BICUBIC])
@pytest.mark.parametrize("size", [TARGET] + TINY_TARGETS)
def test_fixed_path_batches(golden, size, flt, oc):
    """The PIL.Image branch of Predictor._prepare_image: straight to the target size, x / 255 * 2 - 1 on every band.  The
    vertical pass reading the source (with its conversions), the horizontal pass alone, both, neither; 1 .. 9-pixel axes."""
    rows, wants = fixed_group(golden[1], size, oc, flt)
    assert len(rows) == (2 * len(FIXED) if size == TARGET else 2 * len(TINY_SOURCES)) and {r[3] for r in rows} == {1, 3}
    run_batch(rows, wants, normalize="symmetric", keep_aspect=False, resample=FILTER_NAME[flt])


@pytest.mark.gpu
def test_beyond_the_host_builders_limit(golden):
    """600 -> 5: LANCZOS needs 600 taps per output sample.  The device builder computes them and the result is Pillow's;
    the host builder stops at 512 and the call says so instead of returning an image.  BICUBIC (480 taps) passes on both."""
    from img2latex_amd.data import preprocess_batch
    kw = dict(normalize="symmetric", keep_aspect=False)
    rows, wants = fixed_group(golden[1], LIMIT_TARGET, 1, LANCZOS)
    assert [r[1:4] for r in rows] == [(600, 8, 1), (600, 9, 3)]
    run_batch(rows, wants, tables=("device",), resample="lanczos", **kw)
    for sel in ([0, 1], [0], [1]):
        with pytest.raises(ValueError, match="512"):
            preprocess_batch([page(*rows[i][:4]) for i in sel], LIMIT_TARGET, 1, tables="host", resample="lanczos", **kw)
    rows, wants = fixed_group(golden[1], LIMIT_TARGET, 1, BICUBIC)
    run_batch(rows, wants, resample="bicubic", **kw)                   # the host pool serves on after the refusal


@pytest.mark.gpu
def test_width_collapsing_to_zero(golden, tmp_path):
    """(48, 1) at height 24: round(0.5) = 0.  The batch call refuses, naming the page; `load_image` answers with the zero
    image, as the reference does (utils.py:84-90)."""
    from PIL import Image
    from img2latex_amd.data import load_image, preprocess_batch
    rows = [r for r in golden[0] if (r[1], r[2]) == (48, 1)]
    assert len(rows) == 4
    for (seed, h, w, sc, size, oc, norm, want) in rows:
        for imgs, bad in (([page(seed, h, w, sc)], 0), ([page(20000, 24, 56, 1), page(seed, h, w, sc)], 1)):
            for tab in ("device", "host"):
                with pytest.raises(ValueError, match=f"image {bad} .48x1. collapses to zero width"):
                    preprocess_batch(imgs, size, oc, bool(norm), tables=tab)
        path = str(tmp_path / f"thin{sc}{oc}.png")
        Image.fromarray(page(seed, h, w, sc)).save(path)
        got = load_image(path, size, oc, bool(norm))
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want) and not want.any()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1])
def test_second_trip_of_the_pixel_loops(k):
    """One page whose intermediate image (k = 0, resize_h_kernel) or output (k = 1, resize_v_norm_kernel) is larger than
    one pass of the 1024-block grid: the elements of the second trip equal the oracle's too."""
    from img2latex_amd.data import preprocess_batch
    (h, w, c), size, oc = TRIPS[k]
    for flt in (LANCZOS, BICUBIC):
        want = symmetric(trip_expected(k, flt))
        for tab in ("device", "host"):
            out = preprocess_batch([page(30000 + k, h, w, c)], size, oc, "symmetric", keep_aspect=False,
                                   resample=FILTER_NAME[flt], tables=tab)
            assert np.array_equal(out.cpu().numpy()[0], want), (flt, tab)


@pytest.mark.gpu
def test_resident_pages_take_the_same_paths(golden, tmp_path):
    """`preprocess_resident` (pages gathered from a PageStore at 256-byte offsets) on the fixed-size and on the
    aspect-keeping batch: the fixture's values."""
    from PIL import Image
    from img2latex_amd import data as D
    aspect, fixed, _ = golden
    frows, fwants = fixed_group(fixed, TARGET, 3, BICUBIC)
    arows = [r for r in aspect if r[5] == 1 and r[6] == 1 and (r[1], r[2]) != (48, 1)]
    paths = []
    for r in frows + arows:
        paths.append(str(tmp_path / f"p{len(paths)}.png"))
        Image.fromarray(page(*r[:4])).save(paths[-1])
    store = D.PageStore(paths, 3, "cuda", decode_threads=2)
    assert not store.failed.any() and store.shapes[:, 2].tolist() == [r[3] for r in frows + arows]
    for tab in ("device", "host"):
        for order in (list(range(len(frows))), list(range(len(frows) - 1, -1, -1))):
            got = D.preprocess_resident(store, order, TARGET, 3, "symmetric", keep_aspect=False, resample="bicubic",
                                        tables=tab).cpu().numpy()
            for j, i in enumerate(order):
                assert np.array_equal(got[j], fwants[i]), (tab, frows[i][1:7])
        index = [len(frows) + i for i in range(len(arows))]
        got = D.preprocess_resident(store, index, TARGET, 1, True, tables=tab).cpu().numpy()
        for j, r in enumerate(arows):
            assert np.array_equal(got[j], r[7]), (tab, r[1:7])


@pytest.mark.gpu
@pytest.mark.parametrize("flt", [LANCZOS, BICUBIC])
def test_device_tables_at_short_axes_and_past_the_grid(flt):
    """i2l_resample_coeffs_device against i2l_resample_coeffs (host, libm = Pillow's arithmetic) in ONE launch: every axis
    of 1 .. 7 samples (both bounds of every output sample clip) to 1, 2, 7 and 24; 4100 outputs (the 64-block grid covers
    4096: a second trip) up- and down-scaling, with a one-output entry of 1801 taps between them in the same grid.  Every
    bound and weight is equal, and the gaps between the tables and the guards around them keep their sentinel."""
    L = _lib.lib()
    pairs = [(a, b) for a in range(1, 8) for b in (1, 2, 7, 24)] + [(5000, 4100), (300, 1), (3, 4100)]
    ins, outs = (np.array(v, np.int32) for v in zip(*pairs))
    ks = np.array([L.i2l_resample_ksize(flt, a, b) for a, b in pairs], np.int64)
    assert int(ks.min()) >= 5 and int(ks[-2]) == (1801 if flt == LANCZOS else 1201)
    sizes = outs.astype(np.int64) * (2 + ks)
    gap, guard = 5, 64
    offs = guard + np.concatenate([[0], np.cumsum(sizes[:-1] + gap)]).astype(np.int64)
    total = int(offs[-1] + sizes[-1]) + guard
    want = np.full(total, SENTINEL, np.int32)
    assert L.i2l_resample_coeffs_batch(flt, len(pairs), ins.ctypes.data, outs.ctypes.data, offs.ctypes.data,
                                       want.ctypes.data, 4) == 0
    written = np.zeros(total, bool)
    for o, s in zip(offs.tolist(), sizes.tolist()):
        written[o:o + s] = True
    assert bool((want[~written] == SENTINEL).all()) and int((~written).sum()) == 2 * guard + gap * (len(pairs) - 1)
    assert bool((np.abs(want[written].astype(np.int64)) <= 1 << 23).all())
    d_in, d_out, d_off = (torch.from_numpy(a).cuda() for a in (ins, outs, offs))
    got = torch.full((total,), SENTINEL, dtype=torch.int32, device="cuda")
    assert L.i2l_resample_coeffs_device(flt, len(pairs), d_in.data_ptr(), d_out.data_ptr(), d_off.data_ptr(),
                                        got.data_ptr(), 4100, _lib.stream_ptr()) == 0
    got = got.cpu().numpy()
    assert bool((got[~written] == SENTINEL).all()), np.nonzero(got[~written] != SENTINEL)[0][:5]
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (flt, diff[:5], got[diff[:5]], want[diff[:5]])
