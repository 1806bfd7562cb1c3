"""JPEG fixtures for tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py, encoded at run time with Pillow from seeded numpy content:
a smooth ramp, noise, and a black / white checkerboard at quality 100 (it drives the range limit)."""
import io

import numpy as np

SIZES = [(1, 1), (3, 2), (4, 4), (5, 3), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (50, 40), (64, 24)]      # (w, h)
SUBSAMPLING = {0: "444", 1: "422", 2: "420"}
_CACHE = {}


def content(kind, w, h, rng):
    """uint8 [h, w, 3]."""
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], 2).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)


def encode(img, mode="RGB", **params):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(img[:, :, 0])) if mode == "L" else Image.fromarray(img)
    if mode == "CMYK":
        im = im.convert("CMYK")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **params)
    return buf.getvalue()


def fixtures():
    """[(name, bytes)]: every size x 4:4:4 / 4:2:2 / 4:2:0 x (ramp at quality 30, noise at 92, checkerboard at 100), greyscale, custom
    Huffman tables (optimize=True) and restart intervals (restart_marker_blocks=3).  All inside the covered set."""
    if "all" in _CACHE:
        return _CACHE["all"]
    rng = np.random.default_rng(2024)
    out = []
    for w, h in SIZES:
        for sub, tag in SUBSAMPLING.items():
            for kind, q in (("ramp", 30), ("noise", 92), ("checker", 100)):
                out.append(("%dx%d-%s-%s-q%d" % (w, h, tag, kind, q), encode(content(kind, w, h, rng), quality=q, subsampling=sub)))
        out.append(("%dx%d-grey-noise-q92" % (w, h), encode(content("noise", w, h, rng), "L", quality=92)))
    for w, h in ((17, 9), (50, 40), (64, 24)):
        for sub, tag in SUBSAMPLING.items():
            img = content("noise", w, h, rng)
            out.append(("%dx%d-%s-optimize" % (w, h, tag), encode(img, quality=92, subsampling=sub, optimize=True)))
            out.append(("%dx%d-%s-restart3" % (w, h, tag), encode(img, quality=92, subsampling=sub, restart_marker_blocks=3)))
        out.append(("%dx%d-grey-restart3" % (w, h), encode(content("ramp", w, h, rng), "L", quality=30, restart_marker_blocks=3)))
    _CACHE["all"] = out
    return out


def uncovered():
    """[(name, bytes)]: a progressive file and a CMYK file."""
    rng = np.random.default_rng(7)
    img = content("noise", 33, 31, rng)
    return [("progressive", encode(img, quality=92, progressive=True)), ("cmyk", encode(img, "CMYK", quality=92))]


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
