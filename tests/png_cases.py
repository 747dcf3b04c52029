"""PNG files written by hand for the device decoder's tests: chunks via ``struct``, filtering in numpy, the stream from
``zlib.compressobj`` (or bit by bit for streams zlib would never write).  ``walk_inflate`` is a small pure-Python inflate
that lists what a stream contains -- block types, the largest match distance, whether a match overlaps its own output --
and every case asserts that it contains what it claims to.  No GPU, no PIL."""
import struct
import zlib
from typing import List, NamedTuple, Optional

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
COLOUR_TYPES = (0, 2, 3, 4, 6)
SMALL_SIZES = ((1, 1), (1, 67), (9, 13), (3, 300))                   # (height, width)
STROKE_SIZE = (33, 100)


# ------------------------------------------------------------------------------------------------------- the container
def chunk(ctype: bytes, body: bytes, crc: Optional[int] = None) -> bytes:
    crc = zlib.crc32(ctype + body) if crc is None else crc
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", crc & 0xffffffff)


def ihdr(w, h, depth=8, colour=0, compression=0, flt=0, interlace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, compression, flt, interlace))


def container(w, h, colour, stream: bytes, palette: Optional[bytes] = None, idat_split: Optional[int] = None,
              extra_before_idat: bytes = b"", depth=8, interlace=0) -> bytes:
    parts = [SIGNATURE, ihdr(w, h, depth, colour, interlace=interlace)]
    if palette is not None:
        parts.append(chunk(b"PLTE", palette))
    parts.append(extra_before_idat)
    step = idat_split or max(len(stream), 1)
    for k in range(0, max(len(stream), 1), step):
        parts.append(chunk(b"IDAT", stream[k:k + step]))
    parts.append(chunk(b"IEND", b""))
    return b"".join(parts)


# ------------------------------------------------------------------------------------------------------------- filters
def _paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw: np.ndarray, bpp: int, filters) -> bytes:
    """raw: (h, row bytes) uint8 -> the filtered byte string, row y with filter type filters[y] (PNG spec 9.2).  A type
    above 4 is written as it is, with the row unfiltered (for the rejection case)."""
    h, rb = raw.shape
    out = bytearray()
    zero = np.zeros(rb, np.uint8)
    for y in range(h):
        x = raw[y]
        b = raw[y - 1] if y else zero
        a = np.concatenate([np.zeros(bpp, np.uint8), x[:-bpp]]) if rb > bpp else np.zeros(rb, np.uint8)
        c = np.concatenate([np.zeros(bpp, np.uint8), b[:-bpp]]) if rb > bpp else np.zeros(rb, np.uint8)
        ft = int(filters[y])
        if ft == 1:
            pred = a.astype(np.int32)
        elif ft == 2:
            pred = b.astype(np.int32)
        elif ft == 3:
            pred = (a.astype(np.int32) + b.astype(np.int32)) >> 1
        elif ft == 4:
            pred = _paeth(a, b, c)
        else:
            pred = np.zeros(rb, np.int32)
        out.append(ft)
        out += ((x.astype(np.int32) - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def unfilter_rows(filtered: bytes, h: int, rb: int, bpp: int) -> np.ndarray:
    """The inverse, written separately: None / Up whole rows, Sub as a running sum per channel, Average / Paeth byte
    by byte."""
    f = np.frombuffer(filtered, np.uint8).reshape(h, rb + 1)
    out = np.zeros((h, rb), np.uint8)
    for y in range(h):
        ft, x = int(f[y, 0]), f[y, 1:]
        b = out[y - 1] if y else np.zeros(rb, np.uint8)
        if ft == 0:
            out[y] = x
        elif ft == 2:
            out[y] = x + b
        elif ft == 1:
            for ch in range(bpp):
                out[y, ch::bpp] = np.cumsum(x[ch::bpp].astype(np.int64)) & 255
        elif ft in (3, 4):
            row = [0] * rb
            xs, bs = x.tolist(), b.tolist()
            for i in range(rb):
                a = row[i - bpp] if i >= bpp else 0
                c = bs[i - bpp] if i >= bpp else 0
                if ft == 3:
                    pred = (a + bs[i]) >> 1
                else:
                    p = a + bs[i] - c
                    pa, pb, pc = abs(p - a), abs(p - bs[i]), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (bs[i] if pb <= pc else c)
                row[i] = (xs[i] + pred) & 255
            out[y] = row
        else:
            raise ValueError(f"filter type {ft}")
    return out


# ------------------------------------------------------------------------------------------------------------- streams
def deflate(data: bytes, mode: str, level: int = 6, flush_every: Optional[int] = None) -> bytes:
    """A zlib stream of `data`: mode "stored" (level 0), "fixed" (Z_FIXED) or "dynamic" (the default strategy).
    ``flush_every``: a Z_FULL_FLUSH after every that many bytes (many blocks in one stream)."""
    if mode == "stored":
        co = zlib.compressobj(0)
    elif mode == "fixed":
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    else:
        co = zlib.compressobj(level)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = b""
    for k in range(0, len(data), flush_every):
        out += co.compress(data[k:k + flush_every]) + co.flush(zlib.Z_FULL_FLUSH)
    return out + co.flush()


class BitWriter:
    """Deflate's bit order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.bits: List[int] = []

    def value(self, v: int, n: int) -> "BitWriter":
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, c: int, n: int) -> "BitWriter":
        self.bits += [(c >> k) & 1 for k in range(n - 1, -1, -1)]
        return self

    def fixed_litlen(self, s: int) -> "BitWriter":
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xc0 + s - 280, 8)

    def bytes(self) -> bytes:
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(bits[k + j] << j for j in range(8)) for k in range(0, len(bits), 8))


def zlib_wrap(raw_deflate: bytes, data_for_adler: bytes = b"") -> bytes:
    return b"\x78\x9c" + raw_deflate + struct.pack(">I", zlib.adler32(data_for_adler))


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Walk(NamedTuple):
    block_types: List[int]
    max_distance: int
    overlap: bool                    # some match had distance < length
    output: bytes


def walk_inflate(stream: bytes) -> Walk:
    """Inflates a VALID zlib stream bit by bit and reports what it is made of.  Raises ValueError on anything else."""
    data = stream[2:]
    pos = 0                                                          # in bits

    def take(n):
        nonlocal pos
        v = 0
        for k in range(n):
            if (pos >> 3) >= len(data):
                raise ValueError("stream ends")
            v |= ((data[pos >> 3] >> (pos & 7)) & 1) << k
            pos += 1
        return v

    def table(lengths):
        codes, code = {}, 0
        for ln in range(1, 16):
            for s, v in enumerate(lengths):
                if v == ln:
                    codes[(ln, code)] = s
                    code += 1
            code <<= 1
        return codes

    def symbol(codes):
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | take(1)
            if (ln, code) in codes:
                return codes[(ln, code)]
        raise ValueError("no such code")

    out = bytearray()
    types, max_dist, overlap = [], 0, False
    while True:
        final, btype = take(1), take(2)
        types.append(btype)
        if btype == 0:
            pos = (pos + 7) & ~7
            ln, nl = take(16), take(16)
            if ln ^ nl != 0xffff:
                raise ValueError("LEN / NLEN")
            out += data[pos >> 3:(pos >> 3) + ln]
            pos += 8 * ln
        elif btype in (1, 2):
            if btype == 1:
                lit = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
                dist = table([5] * 32)
            else:
                nlit, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for k in range(ncode):
                    cl[_ORDER[k]] = take(3)
                clt, lens = table(cl), []
                while len(lens) < nlit + ndist:
                    s = symbol(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    elif s == 17:
                        lens += [0] * (3 + take(3))
                    else:
                        lens += [0] * (11 + take(7))
                lit, dist = table(lens[:nlit]), table(lens[nlit:nlit + ndist])
            while True:
                s = symbol(lit)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    ln = _LEN_BASE[s - 257] + take(_LEN_EXTRA[s - 257])
                    d = symbol(dist)
                    d = _DIST_BASE[d] + take(_DIST_EXTRA[d])
                    if d > len(out):
                        raise ValueError("distance")
                    max_dist, overlap = max(max_dist, d), overlap or d < ln
                    for _ in range(ln):
                        out.append(out[-d])
        else:
            raise ValueError("block type 3")
        if final:
            break
    return Walk(types, max_dist, overlap, bytes(out))


# --------------------------------------------------------------------------------------------------------------- cases
class Case(NamedTuple):
    name: str
    png: bytes                       # the file
    width: int
    height: int
    colour_type: int
    palette: Optional[bytes]
    stream: bytes                    # the zlib stream (= the concatenated IDAT payloads)
    raw: Optional[np.ndarray]        # (h, w * bpp) the unfiltered rows; None for a rejection case
    walk: Optional[Walk]


def _pixels(rng, h, w, colour, kind="noise"):
    bpp = BPP[colour]
    if kind == "stroke":                                             # a white page with 8 % dark pixels
        dark = rng.random((h, w)) < 0.08
        px = np.full((h, w, bpp), 255, np.uint8)
        px[dark] = rng.integers(0, 90, size=(int(dark.sum()), bpp), dtype=np.uint8)
        if colour == 3:
            px = np.where(dark, rng.integers(1, 7, size=(h, w)), 0).astype(np.uint8)[:, :, None]
    else:
        # four levels: random, yet with enough repeats that Z_FIXED does not fall back to stored blocks
        px = (rng.integers(0, 4, size=(h, w, bpp)) * (1 if colour == 3 else 64)).astype(np.uint8)
    return px.reshape(h, w * bpp)


PALETTE = bytes(v for k in range(7) for v in ((255, 255, 255) if k == 0 else (37 * k % 256, 91 * k % 256, 200 - 23 * k)))


def good_case(name, raw, h, w, colour, mode, first_filter=0, level=6, flush_every=None, filters=None,
              idat_split=None) -> Case:
    bpp = BPP[colour]
    filters = [(first_filter + y) % 5 for y in range(h)] if filters is None else filters
    filtered = filter_rows(raw, bpp, filters)
    stream = deflate(filtered, mode, level, flush_every)
    walk = walk_inflate(stream)
    assert walk.output == filtered and zlib.decompress(stream) == filtered, name
    want = {"stored": {0}, "fixed": {1}, "dynamic": {2}}[mode]
    assert set(walk.block_types) == want or (flush_every and 0 in walk.block_types), (name, walk.block_types)
    palette = PALETTE if colour == 3 else None
    return Case(name, container(w, h, colour, stream, palette, idat_split), w, h, colour, palette, stream, raw, walk)


def matrix_cases() -> List[Case]:
    """Colour types x {stored, fixed, dynamic} with the row filters cycling 0 .. 4 (starting one later in every case, so
    that one-row images meet them all).  The small sizes carry stored and fixed streams only: zlib picks fixed codes
    for so little data whatever it is asked, so a "dynamic" case there would not contain what it claims; dynamic
    blocks come with the 33 x 100 stroke page."""
    rng = np.random.default_rng(20240607)
    cases, k = [], 0
    for colour in COLOUR_TYPES:
        for (h, w) in SMALL_SIZES:
            raw = _pixels(rng, h, w, colour)
            for mode in ("stored", "fixed"):
                cases.append(good_case(f"ct{colour}_{h}x{w}_{mode}", raw, h, w, colour, mode, first_filter=k))
                k += 1
        h, w = STROKE_SIZE
        raw = _pixels(rng, h, w, colour, "stroke")
        for mode in ("stored", "fixed", "dynamic"):
            cases.append(good_case(f"ct{colour}_{h}x{w}_{mode}", raw, h, w, colour, mode, first_filter=k))
            k += 1
    return cases


def special_cases() -> List[Case]:
    rng = np.random.default_rng(7)
    out = []
    # 129 x 253 gray, the last two rows repeat the first two: a match 127 * 254 = 32258 bytes back
    h, w = 129, 253
    raw = (rng.integers(0, 16, size=(h, w)) * 16).astype(np.uint8)      # 16 gray levels: compressible, so no stored blocks
    raw[127:] = raw[:2]
    c = good_case("far_match_129x253", raw, h, w, 0, "dynamic", level=9, filters=[0] * h)
    assert c.walk.max_distance == 127 * 254, c.walk.max_distance
    out.append(c)
    # a constant page: distance 1, length 258 runs
    h, w = 40, 120
    c = good_case("constant_40x120", np.zeros((h, w), np.uint8), h, w, 0, "fixed", filters=[0] * h)   # the filter bytes are 0 too
    assert c.walk.overlap and c.walk.max_distance == 1
    out.append(c)
    # Z_FULL_FLUSH between the rows: many blocks in one stream -- a coded block and the flush's empty stored block per row
    # (fixed codes: a row is too little for zlib to send a code); flushed every 33 rows of a 99 x 100 gray page the coded blocks are dynamic
    h, w = STROKE_SIZE
    raw = _pixels(rng, h, w, 2, "stroke")
    c = good_case("full_flush_33x100", raw, h, w, 2, "dynamic", flush_every=1 + 3 * w)
    assert len(c.walk.block_types) > 2 * h and {0, 1} <= set(c.walk.block_types), c.walk.block_types
    out.append(c)
    h, w = 99, 100
    raw = _pixels(rng, h, w, 0, "stroke")
    c = good_case("full_flush_33_rows_99x100", raw, h, w, 0, "dynamic", first_filter=2, flush_every=33 * (1 + w))
    assert len(c.walk.block_types) >= 6 and {0, 2} <= set(c.walk.block_types), c.walk.block_types
    out.append(c)
    # a dynamic block for a 1 x 1 image, bit by bit (zlib itself codes so little with fixed tables): literal/length
    # lengths {0: 1 bit, 200: 2, 256: 2}, one distance code of one bit, sent with the code-length code {18: 1 bit, 1: 2, 2: 2}
    b = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(14, 4)
    for sym in _ORDER[:18]:
        b.value({18: 1, 1: 2, 2: 2}.get(sym, 0), 3)
    b.code(2, 2)                                                     # length 1 for literal 0
    b.code(0, 1).value(127, 7).code(0, 1).value(50, 7)               # 138 + 61 zero lengths: literals 1 .. 199
    b.code(3, 2)                                                     # length 2 for literal 200
    b.code(0, 1).value(44, 7)                                        # 55 zero lengths: 201 .. 255
    b.code(3, 2).code(2, 2)                                          # length 2 for the end code, 1 for the distance code
    b.code(0, 1).code(2, 2).code(3, 2)                               # the data: 0 (the filter byte), 200, end
    filtered = bytes([0, 200])
    stream = zlib_wrap(b.bytes(), filtered)
    walk = walk_inflate(stream)
    assert zlib.decompress(stream) == filtered and walk.output == filtered and walk.block_types == [2]
    out.append(Case("handmade_dynamic_1x1", container(1, 1, 0, stream), 1, 1, 0, None, stream,
                    np.array([[200]], np.uint8), walk))
    return out


def good_cases() -> List[Case]:
    return matrix_cases() + special_cases()


def _rejection(name, w, h, colour, stream, palette=None) -> Case:
    return Case(name, container(w, h, colour, stream, palette), w, h, colour, palette, stream, None, None)


def rejection_cases() -> List[Case]:
    """Streams the decoder must refuse, each with the reason in its name.  All are gray 4 x 6 unless they need more."""
    rng = np.random.default_rng(11)
    h, w = 4, 6
    raw = _pixels(rng, h, w, 0)
    filtered = filter_rows(raw, 1, [0, 1, 2, 3])
    good = deflate(filtered, "fixed")
    cases = [_rejection("wrong_adler", w, h, 0, good[:-1] + bytes([good[-1] ^ 1]))]
    big = _pixels(rng, 33, 100, 0, "stroke")
    big_stream = deflate(filter_rows(big, 1, [y % 5 for y in range(33)]), "dynamic")
    assert set(walk_inflate(big_stream).block_types) == {2}
    cases.append(_rejection("cut_mid_block", 100, 33, 0, big_stream[:len(big_stream) // 2]))
    cases.append(_rejection("one_byte_too_many", w, h, 0, deflate(filtered + b"\x00", "fixed")))
    cases.append(_rejection("one_byte_too_few", w, h, 0, deflate(filtered[:-1], "fixed")))
    cases.append(_rejection("filter_byte_5", w, h, 0, deflate(filter_rows(raw, 1, [0, 5, 2, 3]), "fixed")))
    stored = bytearray(deflate(filtered, "stored"))
    assert stored[2] == 1 and stored[3] == len(filtered)             # one final stored block: header, LEN, NLEN
    stored[5] ^= 0x10
    cases.append(_rejection("stored_len_nlen_mismatch", w, h, 0, bytes(stored)))
    # dynamic headers zlib never writes.  Code-length code {0: 1 bit, 1: 1 bit}: 257 literal/length codes of one bit
    b = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(15, 4)
    for sym in _ORDER:
        b.value(1 if sym in (0, 1) else 0, 3)
    for _ in range(258):
        b.code(1, 1)
    cases.append(_rejection("over_subscribed_lengths", w, h, 0, zlib_wrap(b.bytes() + b"\x00" * 8)))
    # code-length code {0: 1 bit, 2: 1 bit}: literal 0 and the end code with two bits each, nothing else: incomplete
    b = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(0, 5).value(12, 4)
    for sym in _ORDER[:16]:
        b.value(1 if sym in (0, 2) else 0, 3)
    b.code(1, 1)
    for _ in range(255):
        b.code(0, 1)
    b.code(1, 1).code(0, 1)
    cases.append(_rejection("incomplete_lengths", w, h, 0, zlib_wrap(b.bytes() + b"\x00" * 8)))
    b = BitWriter().value(1, 1).value(1, 2).fixed_litlen(65).fixed_litlen(286).fixed_litlen(256)
    cases.append(_rejection("litlen_symbol_286", w, h, 0, zlib_wrap(b.bytes())))
    b = BitWriter().value(1, 1).value(1, 2).fixed_litlen(65).fixed_litlen(257).code(30, 5).fixed_litlen(256)
    cases.append(_rejection("distance_code_30", w, h, 0, zlib_wrap(b.bytes())))
    b = BitWriter().value(1, 1).value(1, 2).fixed_litlen(65).fixed_litlen(257).code(1, 5).fixed_litlen(256)
    cases.append(_rejection("distance_before_start", w, h, 0, zlib_wrap(b.bytes())))      # distance 2 after one byte
    idx = np.zeros((h, w), np.uint8)
    idx[2, 3] = 2
    cases.append(_rejection("palette_index_beyond_plte", w, h, 3, deflate(filter_rows(idx, 1, [0] * h), "fixed"), PALETTE[:6]))
    return cases


def write_case_file(path, cases) -> None:
    """The host program's input (csrc/png_host_main.cpp)."""
    with open(path, "wb") as f:
        f.write(b"PNGC" + struct.pack("<i", len(cases)))
        for c in cases:
            pal = c.palette or b""
            f.write(struct.pack("<iiiiq", c.width, c.height, c.colour_type, len(pal) // 3, len(c.stream)) + c.stream + pal)


def read_result_file(path, n):
    """[(status, bytes)] as the host program wrote them."""
    data, pos, out = open(path, "rb").read(), 0, []
    for _ in range(n):
        status, size = struct.unpack_from("<iq", data, pos)
        pos += 12
        out.append((status, data[pos:pos + size]))
        pos += size
    assert pos == len(data)
    return out


# ---------------------------------------------------------------------------------------------------- the host program
def adam7(px: np.ndarray) -> bytes:
    """(h, w, bpp) pixels -> the filtered bytes of an INTERLACED image (seven passes, filter 0 in every row)."""
    out = bytearray()
    for xs, ys, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = px[ys::dy, xs::dx]
        if sub.size:
            for row in sub:
                out += b"\x00" + row.tobytes()
    return bytes(out)


def build_host_program(out_dir: str, name: str = "png_host_main") -> str:
    """Compiles csrc/<name>.cpp (png_host_main: the shared decode core with a ``main``) with the host compiler that comes with
    hipcc and ``-fsanitize=address,undefined`` -> ``(the program's path, sanitized)``.  Where the sanitizer runtime cannot
    be linked the program is built plain and ``sanitized`` is False: the caller decides whether that is acceptable."""
    import os
    import shutil
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hmer-img2latex_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = clang if os.path.exists(clang) else (shutil.which("clang++") or shutil.which("g++") or "c++")
    exe = os.path.join(out_dir, name)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", csrc, os.path.join(csrc, name + ".cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        print(name + ": the sanitizer build failed, building plain:\n" + r.stderr[-800:])
        subprocess.run(base, check=True)
    return exe, sanitized


def run_host_program(exe: str, cases, work_dir: str):
    """-> [(status, bytes)] per case; asserts an ordinary exit and no sanitizer report."""
    import os
    import subprocess
    src, dst = os.path.join(work_dir, "cases.bin"), os.path.join(work_dir, "results.bin")
    write_case_file(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    return read_result_file(dst, len(cases))
