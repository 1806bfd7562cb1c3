"""The images the JPEG encoder is held to (tests/test_jpeg_enc_cpu.py, tests/test_gpu_jpeg_enc.py), built from seeds: the smallest sizes
that reach each rule of include/fdhip.h ("JPEG outputs"), and the contents that reach each branch of the entropy coder."""
import io

import numpy as np

# (H, W): smallest image; one luma block; pad on both sides; even H that is no multiple of 16 (twice) and 4x8, 20x23; odd H; right-edge
# dummy blocks; a bottom dummy row under a right-edge dummy; one KITTI frame (odd H, W = 77 * 16 + 10)
SIZES = ((1, 1), (8, 8), (7, 9), (4, 8), (24, 40), (12, 9), (20, 23), (31, 16), (64, 65), (17, 33))
FRAME = (375, 1242)
QUALITIES = (10, 30, 75, 92, 100)
SAMPLINGS = ("1x1", "2x1", "2x2")
SUBSAMPLING = {"1x1": 0, "2x1": 1, "2x2": 2}


def content(kind, h, w, seed=0):
    rng = np.random.RandomState(1000 * h + w + seed)
    if kind == "noise":                                          # long codes, many FF bytes to stuff
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "checker":                                        # alternating 8x8 blocks: DC differences of category 11 at quality 100
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == "sparks":                                         # single bright pixels on black: long runs of zeros at low quality
        a = np.zeros((h, w, 3), np.uint8)
        n = max(1, h * w // 150)
        a[rng.randint(0, h, n), rng.randint(0, w, n)] = 255
        return a
    if kind == "fine":                                           # alternating pixels: one high coefficient behind a run of 16 and more zeros
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == "gradient":
        row = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)
        return np.ascontiguousarray(np.stack([np.tile(row, (h, 1)), np.tile(row[::-1], (h, 1)), np.full((h, w), 90, np.uint8)], 2))
    if kind == "texture":                                        # a smooth scene plus fine noise, as a photograph has
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([128 + 90 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0 - c) for c in range(3)], 2)
        return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
    raise ValueError(kind)


CONTENTS = ("noise", "white", "black", "checker", "sparks", "fine", "gradient")


def pillow(rgb, quality, sampling):
    from PIL import Image
    f = io.BytesIO()
    if rgb.ndim == 2:
        Image.fromarray(rgb).save(f, "JPEG", quality=quality)
    else:
        Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=SUBSAMPLING[sampling])
    return f.getvalue()


def cases(qualities=QUALITIES, sizes=SIZES, contents=CONTENTS):
    """[(name, rgb, quality, sampling)]: every size x sampling, the contents and qualities going round so that each content meets each
    quality and each sampling; plus the pairs the rules name (checker at 100, sparks and fine at 10)."""
    out, k = [], 0
    for h, w in sizes:
        for s in SAMPLINGS:
            for c in contents:
                q = qualities[k % len(qualities)]
                k += 1
                out.append(("%s-%dx%d-q%d-%s" % (c, h, w, q, s), content(c, h, w), q, s))
            k += 1
            for c, q in (("checker", 100), ("sparks", 10), ("fine", 10)):
                name = "%s-%dx%d-q%d-%s" % (c, h, w, q, s)
                if name not in [n for n, _, _, _ in out]:
                    out.append((name, content(c, h, w), q, s))
    return out


def frame_cases(qualities=(10, 92, 100)):
    """The KITTI frame at all three samplings and at each quality: [(name, rgb, quality, sampling)] - texture, and noise at quality 100
    (the densest stream there is: 21 996 blocks at 1x1)."""
    h, w = FRAME
    return [("%s-%dx%d-q%d-%s" % (c, h, w, q, s), content(c, h, w), q, s)
            for q in qualities for c in ("noise" if q == 100 else "texture",) for s in SAMPLINGS]
