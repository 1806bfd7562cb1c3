"""numpy restatement of the image half of the reference data loader (datasets/mono_dataset.py:85-104): Pillow's 8-bit
antialiased Lanczos resample, the four torchvision ``ColorJitter`` operations on a PIL image and ``ToTensor``.

This is the arithmetic csrc/augment.hip is pinned to.  tests/test_augment_cpu.py checks every function here against PIL
itself (torchvision's PIL branch is a thin mapping onto PIL calls; torchvision is not installed, so that mapping is
second-hand - DESIGN.md section 2); tests/test_gpu_augment.py checks the kernels against these functions bit for bit.
Test helper: not imported by the package.
"""
import numpy as np

PRECISION_BITS = 22          # Pillow Resample.c: 32 - 8 - 2
OPS = ("brightness", "contrast", "saturation", "hue")


# ---------------------------------------------------------------------------------------------- Lanczos resample
def _lanczos(t):
    """sinc(t) * sinc(t / 3) on [-3, 3), 0 outside; sinc(0) = 1."""
    def sinc(x):
        xp = x * np.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(x == 0.0, 1.0, np.sin(xp) / xp)
    return np.where((t >= -3.0) & (t < 3.0), sinc(t) * sinc(t / 3.0), 0.0)


def lanczos_coeffs(in_size, out_size):
    """Per output index: first tap, tap count, int32 coefficients [out_size, ksize] (zero beyond the count)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    xmin = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        x0 = max(int(center - support + 0.5), 0)
        x1 = min(int(center + support + 0.5), in_size)
        n = x1 - x0
        w = _lanczos(((np.arange(n) + x0) - center + 0.5) * ss)
        ww = 0.0
        for v in w:                       # sequential float64 sum, as the C loop
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        k = np.where(w < 0, w * (1 << PRECISION_BITS) - 0.5, w * (1 << PRECISION_BITS) + 0.5)
        xmin[xx], count[xx] = x0, n
        coef[xx, :n] = np.trunc(k).astype(np.int32)
    return xmin, count, coef, ksize


def _resample_axis1(img, out_size):
    """img [A, in, C] uint8 -> [A, out, C] uint8 along axis 1."""
    xmin, count, coef, _ = lanczos_coeffs(img.shape[1], out_size)
    out = np.empty((img.shape[0], out_size, img.shape[2]), np.uint8)
    wide = img.astype(np.int64)
    for xx in range(out_size):
        x0, n = int(xmin[xx]), int(count[xx])
        acc = np.tensordot(wide[:, x0:x0 + n, :], coef[xx, :n].astype(np.int64), axes=([1], [0]))
        out[:, xx, :] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def resize_lanczos(img, out_h, out_w, mirror=False):
    """``img.resize((out_w, out_h), Image.LANCZOS)`` for an [H, W, 3] uint8 array: horizontal pass, uint8 intermediate,
    vertical pass.  ``mirror``: the source is flipped left-right first (kitti_dataset.py:56-62)."""
    img = np.ascontiguousarray(img[:, ::-1] if mirror else img)
    tmp = _resample_axis1(img, out_w) if out_w != img.shape[1] else img
    if out_h == tmp.shape[0]:
        return tmp
    return np.ascontiguousarray(_resample_axis1(tmp.transpose(1, 0, 2), out_h).transpose(1, 0, 2))


def pyramid(img, height, width, num_scales, mirror=False):
    """mono_dataset.py:96-97: scale s is resampled from scale s - 1."""
    out, cur = [], img
    for s in range(num_scales):
        cur = resize_lanczos(cur, height // 2 ** s, width // 2 ** s, mirror and s == 0)
        out.append(cur)
    return out


# ---------------------------------------------------------------------------------------------- ColorJitter
def luma(img):
    """PIL ``convert("L")``: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    w = img.astype(np.int64)
    return ((19595 * w[..., 0] + 38470 * w[..., 1] + 7471 * w[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, img, factor):
    """PIL ``Image.blend(degenerate, img, factor)`` in float32: truncated for 0 <= factor <= 1, else clipped, then truncated."""
    f = np.float32(factor)
    d = degenerate.astype(np.int32)
    t = d.astype(np.float32) + f * (img.astype(np.int32) - d).astype(np.float32)
    if not (0.0 <= f <= 1.0):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def contrast_mean(img):
    """int(mean(L) + 0.5) with the mean = exact integer sum / pixel count in float64."""
    lum = luma(img)
    return int(int(lum.astype(np.int64).sum()) / lum.size + 0.5)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)


def rgb_to_hsv(img):
    """PIL ``convert("HSV")`` (Convert.c rgb2hsv_row), with its mix of float32 and double."""
    f32, f64 = np.float32, np.float64
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    mx = np.where(maxc == 0, 1, maxc).astype(f32)
    s = cr / mx
    rc = (maxc - r).astype(f32) / cr
    gc = (maxc - g).astype(f32) / cr
    bc = (maxc - b).astype(f32) / cr
    h_r = bc - gc                                                           # float32
    h_g = ((2.0 + rc.astype(f64)) - bc.astype(f64)).astype(f32)             # double, then rounded to float32
    h_b = ((4.0 + gc.astype(f64)) - rc.astype(f64)).astype(f32)
    h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    uh, us = np.where(grey, 0, uh), np.where(grey, 0, us)
    return np.stack([uh, us, maxc], -1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def hsv_to_rgb(hsv):
    """PIL ``convert("RGB")`` of an HSV image (Convert.c hsv2rgb)."""
    f32, f64 = np.float32, np.float64
    h, s, v = (hsv[..., c].astype(np.int32) for c in range(3))
    h6 = h.astype(f64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vf = v.astype(f32).astype(f64)
    fs64, f64_ = fs.astype(f64), f.astype(f64)
    p = _round_half_away(vf * (1.0 - fs64))
    q = _round_half_away(vf * (1.0 - (fs * f).astype(f64)))                 # fs * f is a float32 product
    t = _round_half_away(vf * (1.0 - fs64 * (1.0 - f64_)))                  # fs * (1.0 - f) is a double product
    p, q, t = (np.clip(a, 0, 255).astype(np.int32) for a in (p, q, t))
    sel = i.astype(np.int32) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.empty(hsv.shape, np.uint8)
    for c in range(3):
        ch = np.select([sel == k for k in range(6)], [table[k][c] for k in range(6)])
        out[..., c] = np.where(s == 0, v, ch)
    return out


def hue_shift(h):
    """uint8 amount added to H: trunc(h * 255) mod 256 (h = -0.05 adds 244)."""
    return int(np.trunc(h * 255.0)) % 256


def hue(img, h):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(h)).astype(np.uint8)
    return hsv_to_rgb(hsv)


_OP_FN = (brightness, contrast, saturation, hue)


def color_jitter(img, factors, order):
    """The four operations with ``factors`` = (b, c, s, h), applied in ``order`` (a sequence of op ids 0..3)."""
    for op in order:
        img = _OP_FN[op](img, factors[op])
    return img


# ---------------------------------------------------------------------------------------------- ToTensor
def to_planes(img):
    """[H, W, 3] uint8 -> [3, H, W] float32, v / 255 correctly rounded."""
    return np.ascontiguousarray((img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
