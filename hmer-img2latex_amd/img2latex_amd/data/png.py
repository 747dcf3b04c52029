"""The PNG container on the host: ``parse_png`` walks the chunks of a file and hands back what the device decoder
(i2l_png_decode, csrc/png.hip) needs -- the IHDR fields, the PLTE bytes and the concatenated IDAT payload, which is the
zlib stream and stays compressed.  Pure Python (``struct`` and ``zlib.crc32``), no GPU, no PIL.

The rule is: the device decodes only files this parser has validated end to end; everything else -- not a PNG, another
bit depth, interlaced, transparency, a chunk layout with anything odd in it -- returns ``None`` and takes the PIL route
(``data.dataset.decode_page``), which alone decides whether a file can be read.  So the parser errs on the strict side:
a file it refuses costs a host decode, a file it wrongly accepted could give pixels PIL would not.

That holds for the chunks the pixels do not depend on as well: PIL interprets some of them while it opens or loads a
file and raises on a malformed one (a gAMA of one byte, an iCCP with another compression method, a zTXt that inflates
beyond its text limit), and the file then counts as unreadable.  An ancillary chunk is therefore accepted only when PIL
cannot raise on it: the fixed-size ones PIL unpacks, at exactly their size (``_FIXED_SIZE``), and the standard ones PIL
has no handler for (``_IGNORED``: it checks their CRC and skips them).  tEXt is kept only with a keyword from
``TEXT_KEYWORDS`` and within a small total: PIL stores every keyword in ``Image.info``, the dict its own decoder reads
its parameters from, so a tEXt chunk named ``interlace``, ``bbox`` or ``transparency`` makes a clean file unreadable for
it; the list holds the PNG specification's registered keywords and ImageMagick's two date stamps, none of which PIL
reads.  Anything else -- iCCP, zTXt, iTXt, eXIf, private chunks, other keywords -- sends the file to PIL.

Limits: width, height >= 1 and height * (1 + width * bytes per pixel) <= ``MAX_FILTERED_BYTES`` = 2^26 (64 MiB of
filtered rows; the kernel's own ceiling is 2^27).  A larger page goes to PIL.
"""
from __future__ import annotations

import struct
import zlib
from typing import NamedTuple, Optional

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BYTES_PER_PIXEL = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}                     # colour type -> bytes per pixel at bit depth 8
MAX_FILTERED_BYTES = 1 << 26
_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")
_FIXED_SIZE = {b"gAMA": 4, b"cHRM": 32, b"sRGB": 1, b"pHYs": 9}       # PIL unpacks these: another size can raise
_IGNORED = (b"bKGD", b"tIME", b"sBIT", b"hIST", b"sPLT")             # PIL has no handler: CRC check, then skipped
TEXT_KEYWORDS = frozenset((b"Title", b"Author", b"Description", b"Copyright", b"Creation Time", b"Software", b"Disclaimer",
                           b"Warning", b"Source", b"Comment", b"date:create", b"date:modify"))
MAX_TEXT_BYTES = 1 << 16                                             # all tEXt chunks of a file (PIL: 1 MB a chunk, 64 MB a file)


class PngInfo(NamedTuple):
    width: int
    height: int
    bit_depth: int
    colour_type: int
    palette: Optional[bytes]          # the PLTE bytes (3 per entry), None without a PLTE chunk
    idat: bytes                       # the IDAT payloads, concatenated: one zlib stream

    @property
    def bytes_per_pixel(self) -> int:
        return BYTES_PER_PIXEL[self.colour_type]

    @property
    def filtered_bytes(self) -> int:
        return self.height * (1 + self.width * self.bytes_per_pixel)

    def out_channels(self, channels: int) -> int:
        """Channels of the page ``decode_page(path, channels)`` returns: L and RGB files are kept as they are."""
        return 1 if self.colour_type == 0 else 3 if self.colour_type == 2 else channels


def parse_png(data: bytes) -> Optional[PngInfo]:
    """``PngInfo`` of an 8-bit, non-interlaced PNG of colour type 0, 2, 3, 4 or 6 whose every chunk checks out, else
    ``None`` ("not for the device")."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        return None
    view = memoryview(data)                                          # chunk bodies are sliced, not copied
    pos, n = 8, len(data)
    header = palette = None
    idat, idat_open, idat_done, ended, text = [], False, False, False, 0
    while pos < n:
        if ended or n - pos < 12:                                    # bytes behind IEND, or no room for a chunk
            return None
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        ctype = data[pos + 4:pos + 8]
        if length > n - pos - 12:
            return None
        body = view[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        if zlib.crc32(body, zlib.crc32(ctype)) != crc:
            return None
        pos += 12 + length
        if header is None:
            if ctype != b"IHDR" or length != 13:
                return None
            header = struct.unpack(">IIBBBBB", body)
            continue
        if ctype == b"IHDR":
            return None
        if ctype not in _CRITICAL:                                   # ancillary: only what PIL cannot raise on
            if ctype == b"tEXt":
                text += length
                if text > MAX_TEXT_BYTES or bytes(body).split(b"\x00", 1)[0] not in TEXT_KEYWORDS:
                    return None
            elif ctype in _FIXED_SIZE:
                if length != _FIXED_SIZE[ctype]:
                    return None
            elif ctype not in _IGNORED:                              # tRNS, animation, iCCP, zTXt, iTXt, eXIf, unknown ones
                return None
        if ctype == b"IDAT":
            if idat_done:                                            # IDAT chunks must be consecutive
                return None
            idat_open = True
            idat.append(body)
            continue
        if idat_open:
            idat_open, idat_done = False, True
        if ctype == b"PLTE":
            if palette is not None or idat_done or length % 3 or not 3 <= length <= 768:
                return None
            palette = bytes(body)
        elif ctype == b"IEND":
            if length:
                return None
            ended = True
    if header is None or not ended or not idat:
        return None
    width, height, depth, colour, compression, flt, interlace = header
    if depth != 8 or colour not in BYTES_PER_PIXEL or compression or flt or interlace:
        return None
    if width < 1 or height < 1 or width > MAX_FILTERED_BYTES or height > MAX_FILTERED_BYTES:
        return None
    if colour == 3 and palette is None:
        return None
    info = PngInfo(width, height, depth, colour, palette, b"".join(idat))
    if info.filtered_bytes > MAX_FILTERED_BYTES:
        return None
    return info
