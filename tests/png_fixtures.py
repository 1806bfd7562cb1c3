"""PNG fixtures for tests/test_png_cpu.py and tests/test_gpu_png.py, built at run time from seeded numpy content.  Two sources:
Pillow's writer at compress_level 0 / 1 / 6 / 9, and a writer of the tests' own (stdlib zlib + struct) that takes what Pillow's does
not offer - a filter type per row, the zlib level, strategy and window, flush points, IDAT split positions - and that also wraps
arbitrary random bytes as scanlines under random filter types: a valid PNG that reaches every wrap-around, every 9-bit Average sum and
every Paeth tie.  Two files carry a hand-assembled deflate stream for what zlib never emits: distance 32768 and a one-code distance tree."""
import io
import struct
import zlib

import numpy as np

import png_ref as PR

FORMATS = {"rgb8": (2, 8, 3), "g8": (0, 8, 1), "g16": (0, 16, 2)}      # name -> (colour type, bit depth, bytes per pixel)
WIDTHS = [1, 2, 3, 5, 17, 64, 65]
HEIGHTS = [1, 2, 63, 64, 65]                                    # 63 / 64 / 65: both sides of a wave of rows
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY}
_CACHE = {}


def chunk(ctype, payload):
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload))


def wrap(w, h, colour, depth, stream, splits=None, interlace=0, extra=()):
    """A PNG file around a finished zlib stream.  ``splits``: the IDAT payload sizes in order (0 = an empty IDAT); what they leave
    goes into a last IDAT."""
    out = [PR.SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))]
    out += [chunk(t, p) for t, p in extra]
    pos = 0
    for n in splits or ():
        out.append(chunk(b"IDAT", stream[pos:pos + n]))
        pos += n
    if pos < len(stream) or not splits:
        out.append(chunk(b"IDAT", stream[pos:]))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def deflate(raw, level=6, strategy="default", wbits=15, flush_at=()):
    """zlib stream of ``raw``; a Z_SYNC_FLUSH after each position in ``flush_at`` (it leaves an empty stored block)."""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, STRATEGIES[strategy])
    out, pos = [], 0
    for at in list(flush_at) + [len(raw)]:
        out.append(co.compress(raw[pos:at]))
        if at < len(raw):
            out.append(co.flush(zlib.Z_SYNC_FLUSH))
        pos = at
    out.append(co.flush())
    return b"".join(out)


def write(fmt, pixels, filters, splits=None, **zargs):
    """``pixels``: the reconstructed bytes uint8 [H, W * bpp]; ``filters``: one type per row."""
    colour, depth, bpp = FORMATS[fmt]
    rows = PR.refilter(pixels, bpp, filters)
    return wrap(pixels.shape[1] // bpp, pixels.shape[0], colour, depth, deflate(rows.tobytes(), **zargs), splits)


def write_scanlines(fmt, rows, splits=None, **zargs):
    """``rows``: the FILTERED bytes uint8 [H, 1 + W * bpp], column 0 the filter types."""
    colour, depth, bpp = FORMATS[fmt]
    return wrap((rows.shape[1] - 1) // bpp, rows.shape[0], colour, depth, deflate(rows.tobytes(), **zargs), splits)


def random_scanlines(rng, w, h, bpp, first=None):
    rows = rng.integers(0, 256, (h, 1 + w * bpp), dtype=np.uint8)
    rows[:, 0] = rng.integers(0, 5, h)
    if first is not None:
        rows[0, 0] = first
    return rows


def content(kind, w, h, bpp, rng):
    """Reconstructed bytes uint8 [h, w * bpp]."""
    y, x = np.mgrid[0:h, 0:w * bpp]
    if kind == "ramp":
        return ((x * 7 + y * 13) & 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w * bpp), dtype=np.uint8)
    if kind == "texture":                                        # compressible and not flat: what a dynamic block is for
        return ((x // bpp * 3 + y * 5 + rng.integers(0, 24, (h, w * bpp))) & 255).astype(np.uint8)
    return ((((x // bpp + y) & 1) * 255)).astype(np.uint8)       # checker


def pillow_write(fmt, pixels, level):
    from PIL import Image
    bpp = FORMATS[fmt][2]
    h, w = pixels.shape[0], pixels.shape[1] // bpp
    if fmt == "rgb8":
        im = Image.fromarray(pixels.reshape(h, w, 3))
    elif fmt == "g8":
        im = Image.fromarray(pixels)
    else:
        im = Image.fromarray(pixels.reshape(h, w, 2).astype(np.uint16) @ np.array([256, 1], np.uint16))
    buf = io.BytesIO()
    im.save(buf, "PNG", compress_level=level)
    return buf.getvalue()


# ---- a deflate assembler for the two streams zlib does not emit -------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, count):                                 # least significant bit first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):                                # a Huffman code goes out most significant bit first
        self.put(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def canonical(lengths):
    """symbol -> (code, length) of the canonical Huffman code."""
    code, out = 0, {}
    for length in range(1, 16):
        for sym, n in enumerate(lengths):
            if n == length:
                out[sym] = (code, length)
                code += 1
        code <<= 1
    return out


def far_match_stream(literals, dynamic):
    """zlib stream: ``literals`` (32768 bytes) in a stored block, then 1024 more bytes as matches of length 258, 258, 258, 250 at
    distance 32768 - in a fixed block, or in a dynamic block whose distance tree is ONE code of length 1."""
    assert len(literals) == 32768
    b = Bits()
    b.put(0x78, 8)
    b.put(0x01, 8)
    b.put(0, 1)
    b.put(0, 2)
    b.align()
    b.put(32768, 16)
    b.put(32768 ^ 0xFFFF, 16)
    b.out += literals
    b.put(1, 1)
    if dynamic:
        b.put(2, 2)
        lit = [0] * 286
        lit[256], lit[284], lit[285] = 1, 2, 2
        dist = [0] * 30
        dist[29] = 1
        b.put(286 - 257, 5)
        b.put(30 - 1, 5)
        b.put(19 - 4, 4)
        cl = [4 if s < 16 else 0 for s in range(19)]             # sixteen 4-bit codes: every length goes out as itself
        for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
            b.put(cl[s], 3)
        for n in lit + dist:
            b.code(n, 4)
        lcode, dcode = canonical(lit), {29: (0, 1)}
    else:
        b.put(1, 2)
        lcode = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
        dcode = {s: (s, 5) for s in range(30)}
    for length in (258, 258, 258, 250):
        if length == 258:
            b.code(*lcode[285])
        else:
            b.code(*lcode[284])
            b.put(250 - 227, 5)
        b.code(*dcode[29])
        b.put(32768 - 24577, 13)
    b.code(*lcode[256])
    b.align()
    raw = bytes(literals) + bytes(literals[:1024])
    b.out += struct.pack(">I", zlib.adler32(raw))
    assert zlib.decompress(bytes(b.out)) == raw
    return bytes(b.out)


def fixtures():
    """[(name, bytes)], all inside the covered set; a name starts with its format (rgb8, g8, g16)."""
    if "all" in _CACHE:
        return _CACHE["all"]
    from fusiondepth_amd import image_codecs
    band = image_codecs.PNG_BAND_ROWS                           # held to fd_png_band_rows() by tests/test_png_cpu.py
    rng = np.random.default_rng(2025)
    out = []
    # Pillow's writer
    kinds = ("ramp", "noise", "checker", "texture")
    k = 0
    for fmt, sizes in (("rgb8", [(1, 1), (3, 2), (17, 9), (64, 24), (65, 63)]), ("g8", [(5, 3), (65, 64)]), ("g16", [(5, 3), (64, 65)])):
        for w, h in sizes:
            for level in (0, 1, 6, 9):
                kind = kinds[k % 4]
                k += 1
                out.append(("%s-pillow-%dx%d-%s-l%d" % (fmt, w, h, kind, level), pillow_write(fmt, content(kind, w, h, FORMATS[fmt][2], rng), level)))
    # random bytes as scanlines: every width x every height for RGB, a rotation of them for the grey formats
    for fi, fmt in enumerate(FORMATS):
        bpp = FORMATS[fmt][2]
        for wi, w in enumerate(WIDTHS):
            for hi, h in enumerate(HEIGHTS):
                if fmt == "rgb8" or (wi + fi) % 5 == hi:
                    out.append(("%s-random-%dx%d" % (fmt, w, h), write_scanlines(fmt, random_scanlines(rng, w, h, bpp), level=1)))
        for h in (band - 1, band, band + 1):                     # the rows one workgroup holds at a time
            out.append(("%s-band-3x%d" % (fmt, h), write_scanlines(fmt, random_scanlines(rng, 3, h, bpp), level=1)))
        for ft in range(5):                                      # every filter on the first row, and so at the first pixel
            out.append(("%s-first%d-5x3" % (fmt, ft), write_scanlines(fmt, random_scanlines(rng, 5, 3, bpp, first=ft), level=6)))
    # real pictures under a filter list, through every zlib setting
    tex = content("texture", 50, 40, 3, rng)
    five = [y % 5 for y in range(40)]
    for name in STRATEGIES:
        out.append(("rgb8-strategy-%s" % name, write("rgb8", tex, five, strategy=name)))
    for wbits in range(9, 16):
        out.append(("rgb8-wbits%d" % wbits, write("rgb8", tex, five[::-1], wbits=wbits, level=9)))
    for ft in range(5):
        out.append(("g16-texture-filter%d" % ft, write("g16", content("texture", 33, 31, 2, rng), [ft] * 31)))
    out.append(("g8-checker-rle", write("g8", content("checker", 64, 24, 1, rng), [0] * 24, strategy="rle")))       # distance 1
    out.append(("g8-flat-l9", write("g8", np.full((65, 300), 7, np.uint8), [0] * 65, level=9)))                       # length 258
    rows = PR.refilter(tex, 3, five)
    out.append(("rgb8-syncflush", write("rgb8", tex, five, flush_at=(0, 1, 151, 152, 3000))))                          # empty stored blocks
    stream = deflate(rows.tobytes(), level=6)
    out.append(("rgb8-idat-every-byte", wrap(50, 40, 2, 8, stream, [1] * len(stream))))
    out.append(("rgb8-idat-empty", wrap(50, 40, 2, 8, stream, [0, 2, 0, 0, 5, 0])))
    stored = deflate(rows.tobytes(), level=0)
    out.append(("rgb8-stored-split-in-len", wrap(50, 40, 2, 8, stored, [3, 1, 1, 1, 1, 7])))                           # zlib header, block header, LEN | NLEN
    out.append(("rgb8-texture-300x200", write("rgb8", content("texture", 300, 200, 3, rng), [y % 5 for y in range(200)], level=6)))
    far = random_scanlines(rng, 1023, 32, 1)                     # pitch 1024: row 32 repeats row 0 at distance 32768
    for dynamic in (False, True):
        out.append(("g8-far-match-%s" % ("one-code-tree" if dynamic else "fixed"),
                    wrap(1023, 33, 0, 8, far_match_stream(far.tobytes(), dynamic), [20000])))        # split inside the stored block
    _CACHE["all"] = out
    return out


def uncovered():
    """[(name, bytes)]: palette, RGBA, interlaced, 1-bit, 16-bit RGB, grey + tRNS - all 5 x 3 except the interlaced one (1 x 1, whose
    Adam7 data is its one scanline).  All valid files: Pillow decodes them."""
    from PIL import Image
    rng = np.random.default_rng(11)

    def save(im, **params):
        buf = io.BytesIO()
        im.save(buf, "PNG", **params)
        return buf.getvalue()

    rgb = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    return [("palette", save(Image.fromarray(rgb).convert("P"))),
            ("rgba", save(Image.fromarray(np.concatenate([rgb, rgb[:, :, :1]], 2), "RGBA"))),
            ("interlaced", wrap(1, 1, 2, 8, deflate(bytes([0, 10, 20, 30])), interlace=1)),
            ("1bit", save(Image.fromarray(grey > 127))),
            ("rgb16", wrap(5, 3, 2, 16, deflate(b"".join(b"\x00" + rng.integers(0, 256, 30, dtype=np.uint8).tobytes() for _ in range(3))))),
            ("grey-trns", save(Image.fromarray(grey), transparency=3))]


def pillow(data):
    """What the loaders got from Pillow: ``convert("RGB")`` of an 8-bit file, ``np.asarray`` of a 16-bit grey one."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im) if im.mode.startswith("I") else np.asarray(im.convert("RGB"))


def pillow_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def corruptions(data, count=200, seed=99):
    """``count`` seeded single-byte corruptions of ``data``."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(data)
        i = int(rng.integers(0, len(b)))
        b[i] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out
