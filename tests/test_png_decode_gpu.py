"""PNG pages decoded on the device (csrc/png.hip, data.decode_pages_device) against PIL: every comparison is exact and
against ``decode_page`` on the same file.  The hand-written cases of tests/png_cases.py (colour types x block types x
filters x sizes, a match at distance 32258, a constant page, multi-block streams) and the twelve pages of
tests/golden/dataset_tiny go through ONE launch per channel count into a sentinel-filled buffer; the streams the decoder
must refuse run on the GPU only after the sanitized host program has passed them, between good neighbours; then the
data set routes (PageStore, the per-batch route, the loaders against tests/golden/dataset.npz) and ``evaluate --decode
device``."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import png_cases as C
from helpers import GOLDEN
from img2latex_amd import _lib
from img2latex_amd import data as D
from img2latex_amd.data.dataset import _PNG_IMAGE, decode_page
from img2latex_amd.training import TokenTable

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = os.path.join(GOLDEN, "dataset_tiny")
CKPT = os.path.join(GOLDEN, "predict_64x800.pt")
SENTINEL = 0xA5
_CACHE = {}


def launch(pngs, channels, gap=37):
    """i2l_png_decode through the C ABI on the files ``pngs`` (bytes): the pages at odd offsets with ``gap`` sentinel
    bytes in front of each -> (rc, status, the whole pixel buffer, page offsets, page sizes)."""
    infos = [D.parse_png(p) for p in pngs]
    assert all(i is not None for i in infos)
    n = len(infos)
    desc = np.zeros(n, dtype=_PNG_IMAGE)
    blobs, z_at, out_at, filtered = [], 0, 0, 0
    for k, info in enumerate(infos):
        d = desc[k]
        d["z_off"], d["z_len"], d["pal_off"] = z_at, len(info.idat), -1
        blobs.append(info.idat)
        z_at += len(info.idat)
        if info.colour_type == 3:
            d["pal_off"], d["pal_n"] = z_at, len(info.palette) // 3
            blobs.append(info.palette)
            z_at += len(info.palette)
        oc = info.out_channels(channels)
        out_at += gap
        d["width"], d["height"], d["colour_type"], d["channels"], d["out_off"] = info.width, info.height, info.colour_type, oc, out_at
        out_at += info.width * info.height * oc
        filtered += info.filtered_bytes
    out_at += gap
    z = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(DEV)
    pixels = torch.full((out_at,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), -77, dtype=torch.int32, device=DEV)
    L = _lib.lib()
    ws = torch.empty((L.i2l_png_decode_workspace_bytes(n, filtered),), dtype=torch.uint8, device=DEV)
    rc = L.i2l_png_decode(z.data_ptr(), z_at, desc.ctypes.data, n, pixels.data_ptr(), out_at, status.data_ptr(), ws.data_ptr(),
                          ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    sizes = desc["width"].astype(np.int64) * desc["height"] * desc["channels"]
    return rc, status.cpu().numpy(), pixels.cpu().numpy(), desc["out_off"].astype(np.int64), sizes


def outside_is_sentinel(buf, offsets, sizes):
    mask = np.ones(buf.size, bool)
    for o, s in zip(offsets, sizes):
        mask[o:o + s] = False
    return bool((buf[mask] == SENTINEL).all()) and int(mask.sum()) > 0


def good_files(tmp_path_factory):
    """The good cases and the dataset_tiny pages as files, with what ``decode_page`` makes of them, once."""
    if "files" not in _CACHE:
        root = tmp_path_factory.mktemp("png_cases")
        names, pngs = [], []
        for c in C.good_cases():
            names.append(c.name)
            pngs.append(c.png)
        for k in range(12):
            names.append(f"tiny_p{k:02d}")
            pngs.append(open(os.path.join(TINY, "img", f"p{k:02d}.png"), "rb").read())
        paths = []
        for name, png in zip(names, pngs):
            paths.append(str(root / (name + ".png")))
            with open(paths[-1], "wb") as f:
                f.write(png)
        want = {ch: [decode_page(p, ch) for p in paths] for ch in (1, 3)}
        _CACHE["files"] = (names, pngs, paths, want)
    return _CACHE["files"]


def batch(tmp_path_factory, channels):
    """ONE launch over all good files."""
    if ("batch", channels) not in _CACHE:
        names, pngs, paths, want = good_files(tmp_path_factory)
        _CACHE[("batch", channels)] = launch(pngs, channels)
    return _CACHE[("batch", channels)]


N_GOOD = 60 + 12                                                    # png_cases.good_cases() and the dataset_tiny pages


# -------------------------------------------------------------------------------------------------- matrix and batch
@pytest.mark.parametrize("channels", [1, 3])
def test_batch_of_all_cases_in_one_launch_leaves_the_sentinel(tmp_path_factory, channels):
    names, pngs, paths, want = good_files(tmp_path_factory)
    assert len(names) == N_GOOD
    rc, status, buf, offsets, sizes = batch(tmp_path_factory, channels)
    assert rc == 0 and status.tolist() == [0] * len(names), dict(zip(names, status.tolist()))
    assert outside_is_sentinel(buf, offsets, sizes)
    for k in range(len(names) - 12, len(names)):                        # the dataset_tiny pages
        assert np.array_equal(buf[offsets[k]:offsets[k] + sizes[k]], want[channels][k].reshape(-1)), names[k]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("k", range(N_GOOD - 12))
def test_case_equals_decode_page(tmp_path_factory, k, channels):
    names, pngs, paths, want = good_files(tmp_path_factory)
    rc, status, buf, offsets, sizes = batch(tmp_path_factory, channels)
    page = want[channels][k]
    assert page is not None and page.size == sizes[k], names[k]
    assert status[k] == 0, (names[k], int(status[k]))
    got = buf[offsets[k]:offsets[k] + sizes[k]]
    bad = np.flatnonzero(got != page.reshape(-1))
    assert bad.size == 0, (names[k], channels, int(bad[0]), bad.size)


def test_single_image_launches_and_argument_refusals(tmp_path_factory):
    names, pngs, paths, want = good_files(tmp_path_factory)
    for k in (0, names.index("ct6_33x100_dynamic"), names.index("ct3_9x13_fixed")):       # n = 1, 2 and 5: partly filled workgroups
        for n in (1, 2, 5):
            rc, status, buf, offsets, sizes = launch([pngs[k]] * n, 3)
            assert rc == 0 and status.tolist() == [0] * n and outside_is_sentinel(buf, offsets, sizes)
            for j in range(n):
                assert np.array_equal(buf[offsets[j]:offsets[j] + sizes[j]], want[3][k].reshape(-1)), (names[k], n, j)
    # descriptors that do not fit: refused before any launch, nothing written
    info = D.parse_png(pngs[0])
    L = _lib.lib()
    z = torch.from_numpy(np.frombuffer(info.idat, np.uint8).copy()).to(DEV)
    size = info.width * info.height
    pixels = torch.full((2 * size + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((2,), -77, dtype=torch.int32, device=DEV)
    ws = torch.empty((L.i2l_png_decode_workspace_bytes(2, 2 * info.filtered_bytes),), dtype=torch.uint8, device=DEV)

    def call(n=1, ws_bytes=None, **fields):
        desc = np.zeros(2, dtype=_PNG_IMAGE)
        desc["z_len"], desc["pal_off"], desc["width"], desc["height"], desc["channels"] = len(info.idat), -1, info.width, info.height, 1
        desc["out_off"] = [0, size + 32]
        for key, v in fields.items():
            desc[key][0] = v
        return L.i2l_png_decode(z.data_ptr(), z.numel(), desc.ctypes.data, n, pixels.data_ptr(), pixels.numel(), status.data_ptr(),
                                ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_ptr())

    for fields in (dict(z_len=len(info.idat) + 1), dict(z_off=-1), dict(out_off=pixels.numel() - size + 1), dict(out_off=-1),
                   dict(width=0), dict(height=-3), dict(colour_type=5), dict(channels=2), dict(channels=3),
                   dict(colour_type=3, pal_n=0, pal_off=0), dict(colour_type=3, pal_n=2, pal_off=len(info.idat) - 5),
                   dict(colour_type=3, pal_n=257, pal_off=0)):
        assert call(**fields) == _lib.ERR_ARG, fields
    assert call(n=2, out_off=size + 32) == _lib.ERR_ARG                 # the two pages overlap
    assert call(ws_bytes=16) == _lib.ERR_WORKSPACE
    assert call(width=1 << 27, height=1, out_off=0) in (_lib.ERR_ARG, _lib.ERR_UNSUPPORTED)
    torch.cuda.synchronize()
    assert bool((pixels == SENTINEL).all()) and status.tolist() == [-77, -77]
    assert call(n=2) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0]


# ----------------------------------------------------------------------------------------------------------- rejection
def rejected(tmp_path_factory):
    """The host program first (sanitized, a process of its own); only then the same files on the GPU, each between two
    good neighbours, all in one launch."""
    if "rejected" not in _CACHE:
        bad = C.rejection_cases()
        work = tmp_path_factory.mktemp("png_host")
        host = C.run_host_program(C.build_host_program(str(work))[0], bad, str(work))    # sanitized or not: test_png_host.py decides
        assert all(status != 0 for status, _ in host), [s for s, _ in host]
        names, pngs, paths, want = good_files(tmp_path_factory)
        neighbours = [names.index("ct2_33x100_dynamic"), names.index("ct0_9x13_fixed")]
        order = []
        for k, c in enumerate(bad):
            order += [("good", neighbours[k % 2]), ("bad", k)]
        order.append(("good", neighbours[0]))
        files = [pngs[i] if kind == "good" else bad[i].png for kind, i in order]
        _CACHE["rejected"] = (bad, [s for s, _ in host], order, launch(files, 1))
    return _CACHE["rejected"]


@pytest.mark.parametrize("k", range(12))
def test_rejected_stream_sets_its_status_and_nothing_else(tmp_path_factory, k):
    names, pngs, paths, want = good_files(tmp_path_factory)
    bad, host_status, order, (rc, status, buf, offsets, sizes) = rejected(tmp_path_factory)
    assert len(bad) == 12 and rc == 0                                   # an ordinary return
    at = order.index(("bad", k))
    assert status[at] != 0 and status[at] == host_status[k], (bad[k].name, int(status[at]), host_status[k])
    for j in (at - 1, at + 1):                                          # intact neighbours
        kind, i = order[j]
        assert kind == "good" and status[j] == 0
        assert np.array_equal(buf[offsets[j]:offsets[j] + sizes[j]], want[1][i].reshape(-1)), (bad[k].name, j)
    assert outside_is_sentinel(buf, offsets, sizes)                     # a refused image may scribble on its own page only


# ------------------------------------------------------------------------------------------------------------ data set
def eval_tokenizer():
    if "tok" not in _CACHE:
        tk = torch.load(CKPT, map_location="cpu", weights_only=False)["tokenizer_config"]
        _CACHE["tok"] = TokenTable(tk["token_to_id"], tk["special_tokens"], tk["max_sequence_length"])
    return _CACHE["tok"]


def extended_tiny(tmp_path_factory):
    """A copy of dataset_tiny whose test split also names: a corrupt PNG, files PIL reads but the device must not
    (interlaced, 16-bit, 1-bit, tRNS), files with a clean stream that PIL refuses for an ancillary chunk, a BMP, a
    palette page, and a missing file."""
    if "extended" not in _CACHE:
        from PIL import Image
        root = str(tmp_path_factory.mktemp("tiny") / "data")
        shutil.copytree(TINY, root)
        img = os.path.join(root, "img")
        rng = np.random.default_rng(3)
        good = C.good_cases()
        by_name = {c.name: c for c in good}
        extra = {}
        c = by_name["ct0_33x100_dynamic"]
        extra["x_wrong_adler.png"] = C.container(c.width, c.height, 0, c.stream[:-1] + bytes([c.stream[-1] ^ 1]))
        extra["x_filter_5.png"] = [r for r in C.rejection_cases() if r.name == "filter_byte_5"][0].png
        px = rng.integers(0, 256, size=(11, 21, 1), dtype=np.uint8)
        extra["x_interlaced.png"] = C.container(21, 11, 0, C.deflate(C.adam7(px), "dynamic"), interlace=1)
        extra["x_palette.png"] = by_name["ct3_33x100_fixed"].png
        extra["x_rgba.png"] = by_name["ct6_33x100_dynamic"].png
        # a clean stream behind an ancillary chunk PIL raises on: PIL's verdict (unreadable) must be the device route's too
        import struct
        import zlib
        anc = {"phys1": C.chunk(b"pHYs", b"\x00"), "gama1": C.chunk(b"gAMA", b"\x00"), "srgb0": C.chunk(b"sRGB", b""),
               "chrm1": C.chunk(b"cHRM", b"\x00"), "iccp_m1": C.chunk(b"iCCP", b"a\x00\x01" + zlib.compress(b"x")),
               "ztxt_2mb": C.chunk(b"zTXt", b"k\x00\x00" + zlib.compress(bytes(2 << 20)))}
        for key, chunk in anc.items():
            extra[f"x_anc_{key}.png"] = C.container(c.width, c.height, 0, c.stream, extra_before_idat=chunk)
        extra["x_anc_ztxt_2mb_behind.png"] = extra["x_rgba.png"][:-12] + anc["ztxt_2mb"] + C.chunk(b"IEND", b"")
        extra["x_anc_fine.png"] = C.container(c.width, c.height, 0, c.stream, extra_before_idat=(
            C.chunk(b"gAMA", b"\x00\x01\x86\xa0") + C.chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)) + C.chunk(b"tEXt", b"Comment\x00v")))
        # tEXt keywords that PIL's decoder takes for its own parameters (Image.info): a clean stream PIL cannot read
        pc = by_name["ct3_33x100_fixed"]
        extra["x_anc_text_interlace.png"] = C.container(c.width, c.height, 0, c.stream, extra_before_idat=C.chunk(b"tEXt", b"interlace\x001"))
        extra["x_anc_text_bbox.png"] = C.container(c.width, c.height, 0, c.stream, extra_before_idat=C.chunk(b"tEXt", b"bbox\x001"))
        extra["x_anc_text_transparency.png"] = pc.png[:-12] + C.chunk(b"tEXt", b"transparency\x001") + C.chunk(b"IEND", b"")
        for name, data in extra.items():
            with open(os.path.join(img, name), "wb") as f:
                f.write(data)
        Image.fromarray(rng.integers(0, 65536, size=(9, 14)).astype(np.uint16)).save(os.path.join(img, "x_16bit.png"))
        Image.fromarray(rng.integers(0, 2, size=(9, 14)).astype(bool)).save(os.path.join(img, "x_1bit.png"))
        pal = Image.new("P", (14, 9))
        pal.putdata(rng.integers(0, 4, size=9 * 14).tolist())
        pal.putpalette(list(range(12)))
        pal.save(os.path.join(img, "x_trns.png"), transparency=0)
        Image.fromarray(rng.integers(0, 256, size=(9, 14, 3), dtype=np.uint8)).save(os.path.join(img, "x_bitmap.bmp"))
        extras = list(extra) + ["x_16bit.png", "x_1bit.png", "x_trns.png", "x_bitmap.bmp", "x_missing.png"]
        for name in extras[:-1]:
            data = open(os.path.join(img, name), "rb").read()
            eligible = name in ("x_wrong_adler.png", "x_filter_5.png", "x_palette.png", "x_rgba.png", "x_anc_fine.png")
            assert (D.parse_png(data) is not None) == eligible, name
        with open(os.path.join(root, "im2latex_test_filter.lst"), "a") as f:
            for k, name in enumerate(extras):
                f.write(f"{name} {k % 16}\n")
        _CACHE["extended"] = (root, extras)
    return _CACHE["extended"]


@pytest.mark.parametrize("channels", [1, 3])
def test_page_store_device_equals_host(tmp_path_factory, channels):
    root, extras = extended_tiny(tmp_path_factory)
    names = [f"p{k:02d}.png" for k in range(12)] + extras + ["p03.png"]
    paths = [os.path.join(root, "img", n) for n in names]
    host = D.PageStore(paths, channels, DEV, decode_threads=3, chunk_bytes=20000)
    for chunk_bytes in (20000, 64 << 20):                               # several launches and uploads, and one
        dev = D.PageStore(paths, channels, DEV, decode_threads=3, chunk_bytes=chunk_bytes, decode="device")
        assert np.array_equal(dev.failed, host.failed) and np.array_equal(dev.shapes, host.shapes)
        assert bool((dev.offsets % D.dataset.PAGE_ALIGN == 0).all())
        for r, name in enumerate(names):
            if host.failed[r]:
                continue
            size = int(np.prod(host.shapes[r]))
            a = host.pixels[host.offsets[r]:host.offsets[r] + size]
            b = dev.pixels[dev.offsets[r]:dev.offsets[r] + size]
            assert torch.equal(a, b), (name, chunk_bytes)
    failed = dict(zip(names, host.failed.tolist()))
    assert failed["x_missing.png"] and failed["x_wrong_adler.png"] and not failed["x_interlaced.png"] and not failed["x_trns.png"]
    assert not failed["x_palette.png"] and not failed["x_bitmap.bmp"] and not failed["x_16bit.png"] and not failed["x_anc_fine.png"]
    bad_anc = [n for n in names if n.startswith("x_anc_") and n != "x_anc_fine.png"]
    assert len(bad_anc) == 10 and all(failed[n] for n in bad_anc), failed      # PIL refuses them, so both stores do
    pixels, offsets, shapes, bad = D.decode_pages_device(paths, channels, DEV)
    assert np.array_equal(bad, host.failed) and np.array_equal(shapes, host.shapes) and pixels.dtype == torch.uint8
    with pytest.raises(ValueError):
        D.PageStore(paths[:1], channels, DEV, decode="gpu")


@pytest.mark.parametrize("channels", [1, 3])
def test_per_batch_route_device_equals_host(tmp_path_factory, channels):
    root, extras = extended_tiny(tmp_path_factory)
    kw = dict(img_size=(32, 128), channels=channels, resident=False, device=DEV, tables="host")
    args = (root, "im2latex_test_filter.lst", "im2latex_formulas.norm.lst", eval_tokenizer())
    host = D.DeviceDataset(*args, **kw)
    dev = D.DeviceDataset(*args, decode="device", **kw)
    assert len(host) == len(dev) >= 12 + len(extras)
    index = list(range(len(host)))
    for idx in (index, index[::-3], index[-len(extras):]):
        a, b = host.batch(idx, first_position=5, epoch=1), dev.batch(idx, first_position=5, epoch=1)
        assert torch.equal(a["images"], b["images"]) and torch.equal(a["formulas"], b["formulas"])
        assert a["image_paths"] == b["image_paths"] and a["raw_formulas"] == b["raw_formulas"]
    zero = [i for i, n in enumerate(host.image_names) if n in ("x_missing.png", "x_wrong_adler.png")]
    assert len(zero) == 2 and bool((dev.batch(zero)["images"] == 0).all())
    with pytest.raises(ValueError):
        D.DeviceDataset(*args, decode="pil", **kw)


def fixture_batches(d, key):
    k = 0
    while f"{key}_{k}_ids" in d:
        yield (json.loads(str(d[f"{key}_{k}_names"])), d[f"{key}_{k}_ids"], d[f"{key}_{k}_images"])
        k += 1


@pytest.mark.parametrize("channels", [1, 3])
def test_loaders_with_decode_device_give_the_golden_batches(channels):
    d = np.load(os.path.join(GOLDEN, "dataset.npz"))
    for resident in (True, False):
        cfg = json.loads(str(d[f"config_c{channels}"]))
        cfg["data"].update(data_dir=TINY, load_in_memory=resident, decode="device")
        torch.manual_seed(1234)                                         # make_golden_dataset.py SEED
        loaders = D.create_data_loaders(cfg, eval_tokenizer(), device=DEV, tables="host")
        assert loaders["train"].dataset.decode == "device" and loaders["train"].dataset.resident is resident
        for key, split in (("train0", "train"), ("train1", "train"), ("val", "val"), ("test", "test")):
            mine = list(loaders[split])
            want = list(fixture_batches(d, f"c{channels}_{key}"))
            assert len(mine) == len(want) > 0, key
            for b, (batch_, (names, ids, images)) in enumerate(zip(mine, want)):
                assert batch_["image_paths"] == names and np.array_equal(batch_["formulas"].cpu().numpy(), ids), (key, b)
                assert torch.equal(batch_["images"].cpu(), torch.from_numpy(images)), (key, b)
        if resident:
            assert loaders["test"].dataset.pages.decode == "device"
    assert D.loader_settings(cfg)["decode"] == "device" and D.loader_settings({"model": {"encoder": {"cnn": {}}}})["decode"] == "host"


# ----------------------------------------------------------------------------------------------------------------- CLI
def test_cli_evaluate_decode_device_prints_and_writes_the_same(tmp_path, capsys):
    from img2latex_amd import cli
    ck_dir = tmp_path / "outputs" / "tiny_exp" / "checkpoints"
    os.makedirs(ck_dir)
    shutil.copyfile(CKPT, ck_dir / "ck.pt")
    texts, saved = [], []
    for extra, out in (([], "host"), (["--decode", "device"], "device")):
        assert cli.main(["evaluate", str(ck_dir / "ck.pt"), TINY, "--batch-size", "5", "--device", "cuda", "--output-dir",
                         str(tmp_path / out)] + extra) == 0
        lines = [ln.strip() for ln in capsys.readouterr().out.splitlines()
                 if ln.strip().startswith(("BLEU-4 Score:", "Levenshtein Similarity:", "Number of Samples:"))]
        assert len(lines) == 3, lines
        texts.append(lines)
        saved.append(json.loads((tmp_path / out / "tiny_exp" / "predictions" / "predictions.json").read_text()))
    assert texts[0] == texts[1] and saved[0] == saved[1] and len(saved[0]) > 0
    with pytest.raises(SystemExit):
        cli.main(["evaluate", str(ck_dir / "ck.pt"), TINY, "--decode", "elsewhere"])
