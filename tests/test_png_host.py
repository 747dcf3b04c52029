"""The host side of the device PNG decoder, no GPU: ``data.png.parse_png`` on every hand-written case (tests/png_cases.py)
and on every kind of file it must refuse, and the shared decode core (csrc/png_core.inc.h) as a stand-alone program built
with -fsanitize=address,undefined -- it must reproduce ``zlib.decompress`` plus the numpy unfilter on every good case
and report a status, with no sanitizer report, on every stream the decoder has to reject."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import png_cases as C
from img2latex_amd import _lib
from img2latex_amd.data import png as P

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_CACHE = {}


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = (C.good_cases(), C.rejection_cases())
    return _CACHE["cases"]


def test_every_case_contains_what_it_claims():
    good, bad = cases()
    names = [c.name for c in good + bad]
    assert len(set(names)) == len(names)
    kinds = {(c.colour_type, tuple(sorted(set(c.walk.block_types)))) for c in good}
    for colour in C.COLOUR_TYPES:
        assert {(colour, (0,)), (colour, (1,)), (colour, (2,))} <= kinds, colour
    sizes = {(c.height, c.width) for c in good}
    assert set(C.SMALL_SIZES) | {C.STROKE_SIZE, (129, 253)} <= sizes
    assert max(c.walk.max_distance for c in good) == 32258
    for c in bad:                                                    # zlib refuses them too, or gives another size
        expect = c.height * (1 + c.width * C.BPP[c.colour_type])
        try:
            ok = len(zlib.decompress(c.stream)) == expect and c.name not in ("filter_byte_5", "palette_index_beyond_plte")
        except zlib.error:
            ok = False
        assert not ok, c.name


def test_parse_png_returns_the_fields_and_the_idat_concatenation():
    good, bad = cases()
    for c in good + bad:
        for split in (None, 7):
            png = C.container(c.width, c.height, c.colour_type, c.stream, c.palette, idat_split=split)
            if split == 7 and len(c.stream) > 7:
                assert png.count(b"IDAT") >= len(c.stream) // 7
            info = P.parse_png(png)
            assert info is not None, c.name
            assert (info.width, info.height, info.bit_depth, info.colour_type) == (c.width, c.height, 8, c.colour_type), c.name
            assert info.palette == c.palette and info.idat == c.stream, c.name
            assert info.bytes_per_pixel == C.BPP[c.colour_type]
            assert info.filtered_bytes == c.height * (1 + c.width * C.BPP[c.colour_type])
    assert P.parse_png(good[0].png) == P.parse_png(bytearray(good[0].png))
    info = P.parse_png(C.container(3, 2, 6, b"\x78\x9c", extra_before_idat=C.chunk(b"gAMA", b"\x00\x01\x86\xa0")))
    assert info is not None and info.out_channels(1) == 1 and info.out_channels(3) == 3      # ancillary chunks are skipped
    assert P.parse_png(C.container(3, 2, 0, b"x")).out_channels(3) == 1 and P.parse_png(C.container(3, 2, 2, b"x")).out_channels(1) == 3


def _with_bad_crc(png: bytes, ctype: bytes) -> bytes:
    at = png.index(ctype) - 4
    (length,) = struct.unpack(">I", png[at:at + 4])
    end = at + 12 + length
    return png[:end - 1] + bytes([png[end - 1] ^ 1]) + png[end:]


def test_parse_png_refuses_what_is_not_for_the_device():
    w, h = 5, 3
    stream = C.deflate(C.filter_rows(np.zeros((h, w), np.uint8), 1, [0] * h), "fixed")
    good = C.container(w, h, 0, stream)
    assert P.parse_png(good) is not None
    iend, plte = C.chunk(b"IEND", b""), C.chunk(b"PLTE", C.PALETTE)
    refused = {
        "empty": b"",
        "not a png": b"BM" + good[2:],
        "signature": good[:7] + b"\x0b" + good[8:],
        "ihdr not first": C.SIGNATURE + C.chunk(b"gAMA", b"\x00\x01\x86\xa0") + good[8:],
        "ihdr twice": good[:33] + good[8:],
        "ihdr crc": _with_bad_crc(good, b"IHDR"),
        "idat crc": _with_bad_crc(good, b"IDAT"),
        "iend crc": _with_bad_crc(good, b"IEND"),
        "idat not consecutive": C.SIGNATURE + C.ihdr(w, h) + C.chunk(b"IDAT", stream[:5]) + C.chunk(b"tEXt", b"Comment\x00b") +
                                C.chunk(b"IDAT", stream[5:]) + iend,
        "no iend": good[:-12],
        "no idat": C.SIGNATURE + C.ihdr(w, h) + iend,
        "cut inside a chunk": good[:-15],
        "bytes behind iend": good + b"\x00",
        "compression method": C.SIGNATURE + C.ihdr(w, h, compression=1) + C.chunk(b"IDAT", stream) + iend,
        "filter method": C.SIGNATURE + C.ihdr(w, h, flt=1) + C.chunk(b"IDAT", stream) + iend,
        "interlaced": C.container(w, h, 0, stream, interlace=1),
        "16 bit": C.container(w, h, 0, stream, depth=16),
        "1 bit": C.container(w, h, 0, stream, depth=1),
        "colour type 5": C.container(w, h, 5, stream),
        "palette image without plte": C.container(w, h, 3, stream),
        "plte of 0 entries": C.container(w, h, 3, stream, b""),
        "plte of 257 entries": C.container(w, h, 3, stream, bytes(771)),
        "plte not a multiple of 3": C.container(w, h, 3, stream, bytes(7)),
        "plte twice": C.container(w, h, 3, stream, C.PALETTE, extra_before_idat=plte),
        "plte behind idat": C.SIGNATURE + C.ihdr(w, h, colour=3) + C.chunk(b"IDAT", stream) + plte + iend,
        "trns": C.container(w, h, 3, stream, C.PALETTE, extra_before_idat=C.chunk(b"tRNS", b"\x00")),
        "trns gray": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tRNS", b"\x00\x00")),
        "unknown critical chunk": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"ABCD", b"")),
        "animated": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"acTL", bytes(8))),
        "zero width": C.container(0, h, 0, stream),
        "zero height": C.container(w, 0, 0, stream),
        "beyond the size limit": C.container(1 << 14, 1 << 13, 2, stream),
        # ancillary chunks PIL raises on (checked against Pillow 12.2: decode_page gives None for each) or may raise on
        "phys of 1 byte": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"pHYs", b"\x00")),
        "gama of 1 byte": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"gAMA", b"\x00")),
        "gama of 5 bytes": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"gAMA", bytes(5))),
        "empty srgb": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"sRGB", b"")),
        "chrm of 1 byte": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"cHRM", b"\x00")),
        "iccp, compression method 1": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"iCCP", b"a\x00\x01" + zlib.compress(b"x"))),
        "iccp": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"iCCP", b"a\x00\x00" + zlib.compress(b"x"))),
        "ztxt of 2 MB": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"zTXt", b"k\x00\x00" + zlib.compress(bytes(2 << 20)))),
        "ztxt of 2 MB behind idat": good[:-12] + C.chunk(b"zTXt", b"k\x00\x00" + zlib.compress(bytes(2 << 20))) + iend,
        "phys of 1 byte behind idat": good[:-12] + C.chunk(b"pHYs", b"\x00") + iend,
        "itxt": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"iTXt", b"k\x00\x00\x00\x00\x00v")),
        "exif": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"eXIf", b"MM\x00*")),
        "private ancillary chunk": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"prVt", b"abc")),
        "text beyond the limit": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", b"Comment\x00" + bytes(P.MAX_TEXT_BYTES - 7))),
        # tEXt keywords: PIL puts them into Image.info, where its decoder looks its own parameters up (decode_page gives
        # None for these three in front of IDAT, and for "transparency" on a palette image behind it as well)
        "text named interlace": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", b"interlace\x001")),
        "text named bbox": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", b"bbox\x001")),
        "text named transparency": C.container(w, h, 3, stream, C.PALETTE, extra_before_idat=C.chunk(b"tEXt", b"transparency\x001")),
        "text named transparency behind idat": C.container(w, h, 3, stream, C.PALETTE)[:-12] + C.chunk(b"tEXt", b"transparency") + iend,
        "text with a keyword of its own": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", b"k\x00v")),
        "text without a keyword": C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", b"\x00v")),
        "ihdr length": C.SIGNATURE + C.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0) + b"\x00") + good[33:],
    }
    for name, data in refused.items():
        assert P.parse_png(data) is None, name
    # what PIL reads without a chance to raise, or does not read at all, stays eligible
    import struct as st
    kept = (C.chunk(b"gAMA", b"\x00\x01\x86\xa0") + C.chunk(b"cHRM", bytes(32)) + C.chunk(b"sRGB", b"\x00") +
            C.chunk(b"pHYs", st.pack(">IIB", 2835, 2835, 1)) + C.chunk(b"bKGD", b"\x00\x00") + C.chunk(b"tIME", bytes(7)) +
            C.chunk(b"tEXt", b"Software\x00x"))
    assert P.parse_png(C.container(w, h, 0, stream, extra_before_idat=kept)) is not None
    assert P.parse_png(good[:-12] + C.chunk(b"tEXt", b"Comment\x00v") + C.chunk(b"tIME", bytes(7)) + iend) is not None
    for key in P.TEXT_KEYWORDS:
        assert P.parse_png(C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", key + b"\x00v"))) is not None, key
    assert P.parse_png(C.container(w, h, 0, stream, extra_before_idat=C.chunk(b"tEXt", b"Comment\x00" + bytes(P.MAX_TEXT_BYTES - 8)))) is not None
    assert (1 << 14) * (1 << 13) * 3 > P.MAX_FILTERED_BYTES >= 64 * 800 * 4 * 100
    assert P.parse_png(C.container(4000, 4000, 6, stream)) is not None                      # 64 MB of RGBA still goes


def test_shared_core_as_a_sanitized_host_program(tmp_path):
    """The stand-alone program, a process of its own: every good case byte for byte, every rejection case a status."""
    good, bad = cases()
    exe, sanitized = C.build_host_program(str(tmp_path))
    print("png_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of png_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    results = C.run_host_program(exe, good + bad, str(tmp_path))
    for c, (status, data) in zip(good, results):
        filtered = zlib.decompress(c.stream)
        want = C.unfilter_rows(filtered, c.height, c.width * C.BPP[c.colour_type], C.BPP[c.colour_type])
        assert np.array_equal(want, c.raw), c.name                   # the builder's filter and this unfilter agree
        assert status == 0 and data == want.tobytes(), (c.name, status)
    want_status = {"wrong_adler": 11, "cut_mid_block": 2, "one_byte_too_many": 8, "one_byte_too_few": 9, "filter_byte_5": 12,
                   "stored_len_nlen_mismatch": 4, "over_subscribed_lengths": 5, "incomplete_lengths": 5, "litlen_symbol_286": 6,
                   "distance_code_30": 6, "distance_before_start": 7, "palette_index_beyond_plte": 13}
    assert {c.name for c in bad} == set(want_status)
    for c, (status, data) in zip(bad, results[len(good):]):
        assert status == want_status[c.name] and data == b"", (c.name, status)


def test_png_symbols_are_bound_and_declared():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    for sym in ("i2l_png_decode", "i2l_png_decode_workspace_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and re.search(rf"\b{sym}\s*\(", header)
    assert "i2l_png_image" in header
    L = _lib.lib()
    assert L.i2l_version() >= 104
    assert L.i2l_png_decode_workspace_bytes(3, 1000) >= 1000 and L.i2l_png_decode_workspace_bytes(-1, 0) == 0
    # refusals that need no device: nothing to do, and arguments that do not fit
    assert L.i2l_png_decode(None, 0, None, 0, None, 0, None, None, 0, None) == 0
    assert L.i2l_png_decode(None, 10, None, 1, None, 10, None, None, 0, None) == _lib.ERR_ARG
    assert L.i2l_png_decode(None, -1, None, 1, None, 10, None, None, 0, None) == _lib.ERR_ARG
