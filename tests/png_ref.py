"""numpy restatement of the PNG rules of include/fdhip.h ("PNG frames"): the chunk walk, the five scanline filters (both directions)
and the two output layouts.  ``zlib.decompress`` restates the inflate.  Used by tests/test_png_cpu.py, tests/test_gpu_png.py and the
writer of tests/png_fixtures.py."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {(2, 8): 3, (0, 8): 1, (0, 16): 2}                       # (colour type, bit depth) of the covered files


def chunks(data):
    """[(type, payload)] up to and including IEND."""
    assert data[:8] == SIGNATURE
    out, pos = [], 8
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        out.append((data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]))
        pos += 12 + n
        if out[-1][0] == b"IEND":
            break
    return out


def header(data):
    cs = chunks(data)
    assert cs[0][0] == b"IHDR"
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    return {"width": w, "height": h, "depth": depth, "colour": colour, "interlace": interlace, "bpp": BPP.get((colour, depth), 0),
            "trns": any(t == b"tRNS" for t, _ in cs)}


def idat(data):
    """The joined IDAT payloads: one zlib stream."""
    return b"".join(p for t, p in chunks(data) if t == b"IDAT")


def scanlines(data):
    """-> (header, the filtered bytes uint8 [H, 1 + row_bytes])."""
    h = header(data)
    raw = np.frombuffer(zlib.decompress(idat(data)), np.uint8)
    return h, raw.reshape(h["height"], 1 + h["width"] * h["bpp"])


def paeth(a, b, c):
    """int arrays -> the predictor; ties resolve a, then b, then c."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(rows, bpp):
    """Filtered [H, 1 + row_bytes] -> reconstructed uint8 [H, row_bytes]."""
    H, rb = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((H, rb), np.int64)
    above = np.zeros(rb, np.int64)
    for y in range(H):
        ft, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        cur = out[y]
        if ft == 0:
            cur[:] = x
        elif ft == 2:
            cur[:] = (x + above) & 255
        elif ft == 1:
            for k in range(min(bpp, rb)):                        # a running sum per byte lane
                cur[k::bpp] = np.cumsum(x[k::bpp]) & 255
        else:
            assert ft in (3, 4), ft
            for i in range(0, rb, bpp):
                j = min(i + bpp, rb)
                a = cur[i - bpp:i][:j - i] if i >= bpp else np.zeros(j - i, np.int64)
                b = above[i:j]
                c = above[i - bpp:i][:j - i] if i >= bpp else np.zeros(j - i, np.int64)
                pred = (a + b) >> 1 if ft == 3 else paeth(a, b, c)
                cur[i:j] = (x[i:j] + pred) & 255
        above = cur
    return out.astype(np.uint8)


def refilter(pixels, bpp, filters):
    """Reconstructed uint8 [H, row_bytes] + one filter type per row -> the filtered [H, 1 + row_bytes]."""
    H, rb = pixels.shape
    p = pixels.astype(np.int64)
    left = np.zeros_like(p)
    left[:, bpp:] = p[:, :-bpp] if rb > bpp else 0
    up = np.zeros_like(p)
    up[1:] = p[:-1]
    upleft = np.zeros_like(p)
    upleft[1:, bpp:] = p[:-1, :-bpp] if rb > bpp else 0
    out = np.zeros((H, rb + 1), np.uint8)
    for y in range(H):
        ft = int(filters[y])
        pred = [0, left[y], up[y], (left[y] + up[y]) >> 1, paeth(left[y], up[y], upleft[y])][ft]
        out[y, 0] = ft
        out[y, 1:] = (p[y] - pred) & 255
    return out


def rgb(h, recon):
    """Pillow's ``convert("RGB")`` of an 8-bit file: uint8 [H, W, 3]."""
    if h["bpp"] == 3:
        return recon.reshape(h["height"], h["width"], 3)
    assert h["bpp"] == 1
    return np.repeat(recon.reshape(h["height"], h["width"], 1), 3, 2)


def gray16(h, recon):
    """``np.asarray(Image.open(f))`` of a 16-bit grey file: host-order uint16 [H, W]."""
    assert h["bpp"] == 2
    return recon.reshape(h["height"], h["width"], 2).astype(np.uint16) @ np.array([256, 1], np.uint16)


def decode(data):
    """The whole restatement -> the array Pillow gives (``rgb`` for 8 bits, ``gray16`` for 16)."""
    h, rows = scanlines(data)
    recon = unfilter(rows, h["bpp"])
    return gray16(h, recon) if h["bpp"] == 2 else rgb(h, recon)
