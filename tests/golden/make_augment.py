"""Generator of tests/golden/augment_*.npz: what PIL itself computes for the image half of a KITTI training item
(datasets/mono_dataset.py:85-104 through the published torchvision -> PIL mapping: ``Resize`` = ``Image.resize``,
``ColorJitter`` = ``ImageEnhance.Brightness / Contrast / Color`` + an HSV round trip with a uint8 hue offset,
``ToTensor`` = uint8 / 255 in float32).  Calls PIL and numpy only.

    python tests/golden/make_augment.py        # rewrites the files next to this script

The source frame is not stored (a 375x1242 noise frame does not compress below the 1 MiB per-file limit): ``frame()``
regenerates it from a seed.  Expected outputs are stored as uint8; the float32 planes for the two smallest scales only.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20260
HEIGHT, WIDTH, NUM_SCALES = 192, 640, 4
# (brightness, contrast, saturation, hue), order of the four operations (0 b, 1 c, 2 s, 3 h)
JITTER_SETS = (
    ((1.2, 0.8, 1.13, 0.1), (0, 1, 2, 3)),
    ((0.8, 1.2, 0.87, -0.05), (3, 2, 1, 0)),
    ((0.93, 1.07, 1.2, -0.1), (1, 3, 0, 2)),
)
PLANE_SCALES = (2, 3)


def frame(seed=SEED, height=375, width=1242):
    """Seeded uint8 frame: 8x8 colour blocks (flat areas, hard edges, saturated colours) plus +-24 of noise."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (height // 8 + 1, width // 8 + 1, 3))
    base = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)[:height, :width]
    noise = rng.integers(-24, 25, (height, width, 3))
    return np.clip(base + noise, 0, 255).astype(np.uint8)


def pil_pyramid(img, height=HEIGHT, width=WIDTH, num_scales=NUM_SCALES, mirror=False):
    from PIL import Image
    cur = Image.fromarray(img)
    if mirror:
        cur = cur.transpose(Image.FLIP_LEFT_RIGHT)
    out = []
    for s in range(num_scales):
        cur = cur.resize((width // 2 ** s, height // 2 ** s), Image.LANCZOS)
        out.append(np.asarray(cur).copy())
    return out


def pil_hue(pil_img, h):
    from PIL import Image
    hh, ss, vv = pil_img.convert("HSV").split()
    arr = np.array(hh, dtype=np.uint8)
    arr = (arr.astype(np.int32) + int(np.trunc(h * 255.0)) % 256).astype(np.uint8)      # uint8 wrap-around
    return Image.merge("HSV", (Image.fromarray(arr, "L"), ss, vv)).convert("RGB")


def pil_jitter(img, factors, order):
    from PIL import Image, ImageEnhance
    cur = Image.fromarray(img)
    for op in order:
        if op == 0:
            cur = ImageEnhance.Brightness(cur).enhance(factors[0])
        elif op == 1:
            cur = ImageEnhance.Contrast(cur).enhance(factors[1])
        elif op == 2:
            cur = ImageEnhance.Color(cur).enhance(factors[2])
        else:
            cur = pil_hue(cur, factors[3])
    return np.asarray(cur).copy()


def pil_planes(img):
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def build():
    """{file stem: {key: array}}."""
    src = frame()
    pyr = pil_pyramid(src)
    sets = {"augment_pyramid": {"seed": np.int64(SEED)}}
    for s, lvl in enumerate(pyr):
        sets["augment_pyramid"]["color_%d" % s] = lvl
    for s in PLANE_SCALES:
        sets["augment_pyramid"]["planes_%d" % s] = pil_planes(pyr[s])
    sets["augment_pyramid"]["mirror_3"] = pil_pyramid(src, mirror=True)[3]
    for j, (factors, order) in enumerate(JITTER_SETS):
        d = {"factors": np.asarray(factors, np.float64), "order": np.asarray(order, np.int32)}
        for s, lvl in enumerate(pyr):
            d["aug_%d" % s] = pil_jitter(lvl, factors, order)
        for s in PLANE_SCALES:
            d["aug_planes_%d" % s] = pil_planes(d["aug_%d" % s])
        sets["augment_jitter%d" % j] = d
    return sets


if __name__ == "__main__":
    for stem, arrays in build().items():
        path = os.path.join(HERE, stem + ".npz")
        np.savez_compressed(path, **arrays)
        print("%s: %d bytes" % (path, os.path.getsize(path)))
