"""The images the PNG encoder is held to (tests/test_png_enc_cpu.py, tests/test_gpu_png_enc.py): the smallest shapes at which a rule
of the stream can go wrong, in the three covered pixel kinds, and the restatement's file of each (computed once per process).

Heights 1 / 63 / 64 / 65 / 129 sit around the 64-row block; widths 1 / 2 / 3 / 85 / 86 / 87 / 259 and one row of 600 put scanline
lengths around the 3 / 258 / 259 / 261 / 517 run boundaries (a scanline of a constant image is ONE run of 1 + W * bpp bytes, or a
filter byte and a run).  Content: zero, constant maximum, a ramp, random bytes; one image per filter type on which that filter wins
the rows it can win; one on which two filters tie."""
import functools

import numpy as np

import png_enc_ref as ER

HEIGHTS = (1, 63, 64, 65, 129)
WIDTHS = (1, 2, 3, 85, 86, 87, 259)
KINDS = {"rgb8": (np.uint8, 3), "g8": (np.uint8, 1), "g16": (np.uint16, 2)}
CONTENTS = ("zero", "max", "ramp", "random")
FILTER_NAMES = ("none", "sub", "up", "average", "paeth")


def _shape(kind, h, w):
    return (h, w, 3) if kind == "rgb8" else (h, w)


def _content(kind, content, h, w, seed):
    dt, _ = KINDS[kind]
    shape, top = _shape(kind, h, w), int(np.iinfo(dt).max)
    if content == "zero":
        return np.zeros(shape, dt)
    if content == "max":
        return np.full(shape, top, dt)
    if content == "ramp":                                        # slow enough for runs, fast enough to wrap in the wider images
        return ((np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape) // 5 * 3) % (top + 1)).astype(dt)
    return np.random.default_rng(seed).integers(0, top + 1, shape).astype(dt)


def _from_raw(kind, raw, h, w):
    """The image whose unfiltered scanline bytes are ``raw`` (uint8 [H, W * bpp])."""
    if kind == "g16":
        return np.ascontiguousarray(raw).view(">u2").astype(np.uint16).reshape(h, w)
    return np.ascontiguousarray(raw).reshape(_shape(kind, h, w))


def filter_winner(kind, ft, h=9, w=85, seed=0):
    """An image on which filter ``ft`` wins: byte by byte, the filter's own prediction plus a sparse strong noise d (0 three times out
    of five, else +-90), so that its cost is about 36 a byte while every other filter's residual is close to uniform (about 64 a
    byte)."""
    _, bpp = KINDS[kind]
    rng = np.random.default_rng(1000 + 10 * seed + ft)
    rb = w * bpp
    d = rng.choice(np.array([0, 0, 0, 90, -90]), size=(h, rb))
    raw = np.zeros((h, rb), np.int64)
    for y in range(h):
        for i in range(rb):
            a = raw[y, i - bpp] if i >= bpp else 0
            b = raw[y - 1, i] if y else 0
            c = raw[y - 1, i - bpp] if y and i >= bpp else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            raw[y, i] = (int(d[y, i]) + (0, a, b, (a + b) >> 1, paeth)[ft]) & 255
    return _from_raw(kind, raw.astype(np.uint8), h, w)


@functools.lru_cache(maxsize=None)
def images():
    """[(name, array)] - every fixture."""
    out, seed = [], 0
    for kind in KINDS:
        shapes = [(h, w) for h in HEIGHTS for w in WIDTHS] + [(1, 600)]
        for h, w in shapes:
            for content in CONTENTS:
                seed += 1
                out.append(("%s-%dx%d-%s" % (kind, h, w, content), _content(kind, content, h, w, seed)))
        for ft, name in enumerate(FILTER_NAMES):
            out.append(("%s-9x85-wins-%s" % (kind, name), filter_winner(kind, ft)))
        # rows 1 .. of a constant non-zero image: Up and Paeth both leave zeros, Sub and Average do not: a tie, to the lower type
        out.append(("%s-5x7-tie" % kind, _content(kind, "max", 5, 7, 0)))
    return out


@functools.lru_cache(maxsize=None)
def encoded():
    """{name: the restatement's file} - the reference every test shares; computed once and never changed."""
    return {name: ER.encode(a) for name, a in images()}


def batches(size=66):
    """The fixtures in batches that mix sizes and kinds: every ``size``-th one of the list, which runs kind after kind."""
    items = images()
    stride = (len(items) + size - 1) // size
    return [items[k::stride] for k in range(stride)]


def write_histograms(path):
    """The fixtures' block histograms as tests/png_enc_host_main.cpp reads them: uint32 n, then n x HIST uint32."""
    hists = np.concatenate([ER.histograms(ER.filter_rows(a)[0]) for _, a in images()]).astype("<u4")
    with open(path, "wb") as fh:
        fh.write(np.array([len(hists)], "<u4").tobytes())
        fh.write(hists.tobytes())
    return len(hists)


if __name__ == "__main__":
    import sys
    print("%d histograms -> %s" % (write_histograms(sys.argv[1]), sys.argv[1]))
