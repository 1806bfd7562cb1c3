"""Data preparation on the GPU, no autograd: the LiDAR scatter and rasterisation, scan sparsification, the batched bilinear resize
and the uint8 image pipeline (Lanczos resample, colour jitter, ``image_pyramid``) that build a training batch."""
import ctypes

import torch

from . import _lib
from ._lib import _empty, _need_cuda, call, f32, ptr, query, stream


# ------------------------------------------------------------------------------------ LiDAR -------
def scatter_2channel(beam, roi=(76, 190, 2, 638), expand=2):
    """gen2channel.py:60-117 on the GPU.  beam [B,1,H,W] (or [H,W]) -> [B,2,H,W]."""
    squeeze = beam.dim() == 2
    if squeeze:
        beam = beam[None, None]
    beam = f32(beam)
    _need_cuda(beam)
    B, _, H, W = beam.shape
    out = _empty((B, 2, H, W), beam)
    call("fd_scatter_2channel", ptr(beam), ptr(out), B, H, W, roi[0], roi[1], roi[2], roi[3], expand, stream())
    return out[0] if squeeze else out


def padded_rows(im_h, target_h):
    """Rows of generate_depth_map(shape=[target_h, .]) (kitti_utils.py:88-101): top padding, 2 rows cropped if shorter."""
    return im_h + abs(target_h - im_h) - (2 if target_h < im_h else 0)


def velo_rasterize(points, P_velo2im, im_h, im_w, shape=(384, 1280), return_full=False, vel_depth=False, beam=True):
    """Velodyne scan -> "4beam" network input (kitti_utils.py:40-102 + kitti_dataset.py:93-117 + mono_dataset.py:193-198).
    ``points``: [N,4] float32 CUDA; ``P_velo2im``: 3x4 (numpy / tensor, float64); ``shape``: the reference's ``shape`` argument
    (None: no padding).  Returns the pooled float32 map (metres / 100) and / or, with ``return_full``, the float64 image
    ``generate_depth_map`` returns."""
    points = f32(points)
    _need_cuda(points)
    P = torch.as_tensor(P_velo2im, dtype=torch.float64).reshape(12).to(points.device).contiguous()
    n = points.shape[0]
    th, tw = (int(shape[0]), int(shape[1])) if shape is not None else (im_h, im_w)
    ph = padded_rows(im_h, th)
    out = torch.empty(((ph + 1) // 2, (tw + 1) // 2), device=points.device, dtype=torch.float32) if beam else None
    full = torch.empty((ph, tw), device=points.device, dtype=torch.float64) if return_full else None
    if out is None and full is None:
        raise ValueError("velo_rasterize: nothing to return")
    ws = torch.empty((query("fd_velo_rasterize_ws_bytes", n, im_h, im_w),), device=points.device, dtype=torch.uint8)
    call("fd_velo_rasterize", points.data_ptr(), n, P.data_ptr(), im_h, im_w, 1 if vel_depth else 0, th, tw,
         out.data_ptr() if out is not None else None, full.data_ptr() if full is not None else None, ws.data_ptr(), stream())
    if out is not None and full is not None:
        return out, full
    return out if out is not None else full


def scaled_roi(H, W):
    """ROI of gen2channel.py:64-65 (rows 76..189, cols 2..637 of 192x640) scaled to another size."""
    return (max(int(round(76 * H / 192)), 2), min(int(round(190 * H / 192)), H - 2), 2, W - 2)


# sparsify/sparsify.py on the GPU ------------------------------------------------------------------
SPARSIFY_BOX = (0.0, 120.0, -50.0, 50.0, -2.5, 1.5)          # sparsify.py:98-103: x, y, z half-open ranges
SPARSIFY_LINE_SPEC = {1: (9,), 2: (9, 11), 3: (7, 9, 11), 4: (2, 7, 12, 16)}     # prepare_{n}beam_data_for_prediction.sh --line_spec


def sparsify_rows(H=64, line_spec=None, slice=1):
    """The rows ``pto_ang_map`` keeps, in output order: ``line_spec`` as given, else ``0::slice``."""
    return [int(r) for r in line_spec] if line_spec is not None else list(range(0, int(H), int(slice)))


def as_int64(v):
    """The 64 bits of an integer as a signed value (how a uint64 key travels in an int64 tensor)."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _device_table(values, dtype, device):
    return torch.tensor(values, dtype=dtype).to(device)


def sparsify_scans(points, H=64, W=1024, line_spec=None, slice=1, random_sample=0, uniforms=None, seed=0, keys=None, offsets=None,
                   box=SPARSIFY_BOX, return_cells=False):
    """``gen_sparse_points`` (sparsify/sparsify.py:32-136) for S raw Velodyne scans in one call (fd_sparsify_scans).
    ``points``: a list of [n,4] float32 CUDA tensors, or one packed [sum n,4] tensor with ``offsets`` (int32 CUDA, [S+1]).
    ``random_sample`` = N > 0 keeps about N * 1.8 of the points: with ``uniforms`` (a float64 CUDA [S, cap] tensor, or a list of 1-D
    arrays, one draw per compacted point - ``np.random.uniform(0, 1, m)`` of the reference) or, without, with the library's
    generator keyed by (``seed``, ``keys[s]``, slot); ``keys``: S integers or an int64 CUDA tensor (default 0 .. S-1).
    Returns ``(slab, counts)``: slab [S, cap, 4] with cap = rows * W, scan s's points in ``slab[s, :counts[s]]`` in the reference's
    order and ``(-1, 0, 0, 0)`` after them; counts int32 CUDA [S].  ``return_cells`` adds int32 [sum n]: row * W + column per point
    (-1: filtered out).  numpy 2 semantics (the angle arithmetic after arcsin is float64)."""
    if isinstance(points, (list, tuple)):
        scans = [f32(p).reshape(-1, 4) for p in points]
        if not scans:
            raise ValueError("sparsify_scans: no scans")
        _need_cuda(*scans)
        ends, total = [0], 0
        for p in scans:
            total += p.shape[0]
            ends.append(total)
        packed = torch.cat(scans) if len(scans) > 1 else scans[0]
        offsets = _device_table(ends, torch.int32, packed.device)
    else:
        packed = f32(points).reshape(-1, 4)
        _need_cuda(packed)
        if offsets is None or offsets.dtype != torch.int32 or not offsets.is_cuda or not offsets.is_contiguous():
            raise ValueError("sparsify_scans: a packed tensor needs offsets: a contiguous int32 CUDA tensor [S + 1]")
    if not packed.is_contiguous():
        packed = packed.contiguous()
    S = offsets.numel() - 1
    rows = sparsify_rows(H, line_spec, slice)
    if not 1 <= len(rows) <= 64:
        raise ValueError("sparsify_scans: %d rows selected; the kernel takes 1 .. 64" % len(rows))
    cfg = _lib.SparsifyCfg()
    cfg.S, cfg.H, cfg.W, cfg.n_rows = S, int(H), int(W), len(rows)
    for k, r in enumerate(rows):
        cfg.rows[k] = r
    cfg.x_lo, cfg.x_hi, cfg.y_lo, cfg.y_hi, cfg.z_lo, cfg.z_hi = [float(v) for v in box]
    cfg.random_sample, cfg.seed = int(random_sample), int(seed) & 0xFFFFFFFFFFFFFFFF
    cap = len(rows) * int(W)
    dev = packed.device
    if cfg.random_sample > 0:
        if uniforms is not None:
            if not torch.is_tensor(uniforms):
                import numpy as np
                host = np.ones((S, cap), dtype=np.float64)
                for s_, u in enumerate(uniforms):
                    u = np.asarray(u, dtype=np.float64).reshape(-1)
                    host[s_, :u.size] = u
                uniforms = torch.from_numpy(host).to(dev)
            if uniforms.dtype != torch.float64 or tuple(uniforms.shape) != (S, cap) or not uniforms.is_cuda or not uniforms.is_contiguous():
                raise ValueError("sparsify_scans: uniforms must be a contiguous float64 CUDA tensor [%d, %d]" % (S, cap))
        elif keys is None:
            keys = list(range(S))
        if keys is not None and not torch.is_tensor(keys):
            keys = _device_table([as_int64(k) for k in keys], torch.int64, dev)
        if keys is not None and (keys.dtype != torch.int64 or keys.numel() != S or not keys.is_cuda or not keys.is_contiguous()):
            raise ValueError("sparsify_scans: keys must be %d integers or a contiguous int64 CUDA tensor" % S)
    else:
        uniforms = keys = None
    nbytes = query("fd_sparsify_ws_bytes", ctypes.byref(cfg))
    if nbytes <= 0:
        raise RuntimeError("fd_sparsify_ws_bytes: %s" % _lib.last_error())
    ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    slab = torch.empty((S, cap, 4), device=dev, dtype=torch.float32)
    counts = torch.empty((S,), device=dev, dtype=torch.int32)
    cells = torch.empty((packed.shape[0],), device=dev, dtype=torch.int32) if return_cells else None
    call("fd_sparsify_scans", packed.data_ptr() if packed.shape[0] else None, offsets.data_ptr(), packed.shape[0], ctypes.byref(cfg),
         uniforms.data_ptr() if uniforms is not None else None, keys.data_ptr() if keys is not None else None, slab.data_ptr(),
         counts.data_ptr(), cells.data_ptr() if cells is not None and cells.numel() else None, ws.data_ptr(), stream())
    return (slab, counts, cells) if return_cells else (slab, counts)


def raster_desc_table(descs):
    """Host image of the ``fd_raster_desc`` table for ``descs`` = [(P_velo2im 3x4, im_h, im_w, flip)]: a ctypes array."""
    import numpy as np
    table = (_lib.RasterDesc * len(descs))()
    for d, (P, im_h, im_w, flip) in zip(table, descs):
        P = np.asarray(P.cpu() if torch.is_tensor(P) else P, dtype=np.float64).reshape(12)
        for k in range(12):
            d.P[k] = P[k]
        d.im_h, d.im_w, d.flip = int(im_h), int(im_w), 1 if flip else 0
    return table


def velo_rasterize_batch(points, descs, shape=(384, 1280), return_full=False, vel_depth=False, beam=True, offsets=None, n_max=None,
                         desc_table=None):
    """``velo_rasterize`` for S scans in one call (fd_velo_rasterize_batch), each already flipped left-right where asked.
    ``points``: a slab [S, cap, 4] (rows with x < 0, such as ``sparsify_scans``' padding, are dropped), or a packed [N, 4] tensor
    with ``offsets`` (int32 CUDA [S+1]) and ``n_max`` >= the longest scan.  ``descs``: [(P_velo2im, im_h, im_w, flip)] per scan (sizes
    may differ; all must pad to the same number of rows for ``shape``); ``desc_table``: the same table already on the device (a uint8
    CUDA tensor holding ``raster_desc_table(descs)``), else it is uploaded here.  Returns [S, h, w] float32 and / or, with
    ``return_full``, [S, H, W] float64."""
    points = f32(points)
    _need_cuda(points)
    if not points.is_contiguous():
        points = points.contiguous()
    S = len(descs)
    if offsets is None:
        if points.dim() != 3 or points.shape[0] != S or points.shape[2] != 4:
            raise ValueError("velo_rasterize_batch: expected a slab [%d, cap, 4], got %s" % (S, tuple(points.shape)))
        n_max = points.shape[1]
    else:
        if offsets.dtype != torch.int32 or not offsets.is_cuda or offsets.numel() != S + 1 or not offsets.is_contiguous() or n_max is None:
            raise ValueError("velo_rasterize_batch: packed points need int32 CUDA offsets [S + 1] and n_max")
    th, tw = int(shape[0]), int(shape[1])
    rows = {padded_rows(int(d[1]), th) for d in descs}
    if len(rows) != 1:
        raise ValueError("velo_rasterize_batch: the scans pad to different heights %s for target %d rows" % (sorted(rows), th))
    ph = rows.pop()
    max_h, max_w = max(int(d[1]) for d in descs), max(int(d[2]) for d in descs)
    if desc_table is None:
        table = raster_desc_table(descs)
        desc_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(points.device)
    elif desc_table.dtype != torch.uint8 or not desc_table.is_cuda or desc_table.numel() != S * ctypes.sizeof(_lib.RasterDesc):
        raise ValueError("velo_rasterize_batch: desc_table must be a uint8 CUDA tensor of %d bytes" % (S * ctypes.sizeof(_lib.RasterDesc)))
    out = torch.empty((S, (ph + 1) // 2, (tw + 1) // 2), device=points.device, dtype=torch.float32) if beam else None
    full = torch.empty((S, ph, tw), device=points.device, dtype=torch.float64) if return_full else None
    if out is None and full is None:
        raise ValueError("velo_rasterize_batch: nothing to return")
    ws = torch.empty((query("fd_velo_rasterize_batch_ws_bytes", S, max_h, max_w),), device=points.device, dtype=torch.uint8)
    call("fd_velo_rasterize_batch", points.data_ptr() if points.numel() else None, offsets.data_ptr() if offsets is not None else None,
         int(n_max), S, desc_table.data_ptr(), max_h, max_w, 1 if vel_depth else 0, th, tw, ph,
         out.data_ptr() if out is not None else None, full.data_ptr() if full is not None else None, ws.data_ptr(), stream())
    if out is not None and full is not None:
        return out, full
    return out if out is not None else full


def resize_desc_table(descs):
    """Host image of the ``fd_resize_desc`` table for ``descs`` = [(offset in floats, h_in, w_in, mirror)]: a ctypes array."""
    table = (_lib.ResizeDesc * len(descs))()
    for d, (offset, h_in, w_in, mirror) in zip(table, descs):
        d.offset, d.h_in, d.w_in, d.mirror = int(offset), int(h_in), int(w_in), 1 if mirror else 0
    return table


def resize_bilinear_batch(packed, descs, size, desc_table=None):
    """``F.interpolate(plane[None, None], size, mode="bilinear", align_corners=False)`` - ATen's CPU result, bit for bit - for B
    planes of different sizes in one call (fd_resize_bilinear_batch), each mirrored left-right AFTER the resize where asked
    (kitti_dataset.py:163-171).  ``packed``: a 1-D float32 CUDA tensor holding the planes; ``descs``: [(offset in floats, h_in, w_in,
    mirror)] per plane; ``desc_table``: the same table already on the device (a uint8 CUDA tensor holding
    ``resize_desc_table(descs)``), else it is uploaded here.  Returns [B, size[0], size[1]] float32."""
    _need_cuda(packed)
    if packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous() or not packed.numel():
        raise ValueError("resize_bilinear_batch: packed must be a non-empty contiguous 1-D float32 CUDA tensor")
    B = len(descs)
    oh, ow = int(size[0]), int(size[1])
    if B < 1 or oh < 1 or ow < 1:
        raise ValueError("resize_bilinear_batch: nothing to do (%d planes -> %d x %d)" % (B, oh, ow))
    for offset, h_in, w_in, _ in descs:
        if h_in < 1 or w_in < 1 or offset < 0 or offset + h_in * w_in > packed.numel():
            raise ValueError("resize_bilinear_batch: a %d x %d plane at float %d leaves the packed buffer of %d floats"
                             % (h_in, w_in, offset, packed.numel()))
    nbytes = B * ctypes.sizeof(_lib.ResizeDesc)
    if desc_table is None:
        desc_table = torch.frombuffer(bytearray(bytes(resize_desc_table(descs))), dtype=torch.uint8).to(packed.device)
    elif desc_table.dtype != torch.uint8 or not desc_table.is_cuda or desc_table.numel() != nbytes or not desc_table.is_contiguous() \
            or desc_table.data_ptr() % 8:
        raise ValueError("resize_bilinear_batch: desc_table must be an 8-byte aligned contiguous uint8 CUDA tensor of %d bytes" % nbytes)
    out = torch.empty((B, oh, ow), device=packed.device, dtype=torch.float32)
    call("fd_resize_bilinear_batch", packed.data_ptr(), packed.numel(), desc_table.data_ptr(), B, oh, ow, out.data_ptr(), stream())
    return out


def depth_png_desc_table(descs):
    """Host image of the ``fd_depth_png_desc`` table for ``descs`` = [(offset in uint16 elements, h, w, mirror, src_y, src_x, win_y,
    win_x, win_h, win_w)]: a ctypes array."""
    table = (_lib.DepthPngDesc * len(descs))()
    for d, (offset, h, w, mirror, src_y, src_x, win_y, win_x, win_h, win_w) in zip(table, descs):
        d.offset, d.h, d.w, d.mirror = int(offset), int(h), int(w), 1 if mirror else 0
        d.src_y, d.src_x, d.win_y, d.win_x, d.win_h, d.win_w = int(src_y), int(src_x), int(win_y), int(win_x), int(win_h), int(win_w)
    return table


def depth_png_keys(packed_u16, descs, canvas, pool=1, channels=1, div0=256.0, div1=1.0, desc_table=None):
    """``get_depth`` of datasets/kitti_completion.py:51-80 for S decoded 16-bit depth PNGs of different sizes in one call
    (fd_depth_png_keys): ``/ div0``, mirror, crop and / or zero pad, ``F.max_pool2d(2, ceil_mode=True)`` with ``pool`` = 2, ``/ div1``.
    ``packed_u16``: a 1-D CUDA tensor holding the planes as uint16 (dtype uint16, or int16 carrying the same bits); ``descs``:
    [(offset, h, w, mirror, src_y, src_x, win_y, win_x, win_h, win_w)] per plane - the window of the ``canvas`` = (H, W) that the
    plane fills, everything outside it is 0, and the source pixel (in mirrored coordinates) of the window's first pixel;
    ``desc_table``: the same table already on the device (a uint8 CUDA tensor holding ``depth_png_desc_table(descs)``), else it is
    uploaded here.  Returns [S, channels, ceil(H / pool), ceil(W / pool)] float32, the map written ``channels`` times."""
    _need_cuda(packed_u16)
    if packed_u16.dtype not in (torch.uint16, torch.int16) or packed_u16.dim() != 1 or not packed_u16.is_contiguous() or not packed_u16.numel() \
            or packed_u16.data_ptr() % 8:
        raise ValueError("depth_png_keys: packed must be a non-empty contiguous 8-byte aligned 1-D uint16 (or int16) CUDA tensor")
    S = len(descs)
    ch, cw = int(canvas[0]), int(canvas[1])
    pool, channels = int(pool), int(channels)
    if S < 1 or ch < 1 or cw < 1 or pool not in (1, 2) or channels not in (1, 2):
        raise ValueError("depth_png_keys: nothing to do (%d planes -> %d x %d, pool %d, %d channels)" % (S, ch, cw, pool, channels))
    for offset, h, w, _, src_y, src_x, win_y, win_x, win_h, win_w in descs:
        if h < 1 or w < 1 or offset < 0 or offset + h * w > packed_u16.numel():
            raise ValueError("depth_png_keys: a %d x %d plane at element %d leaves the packed buffer of %d elements"
                             % (h, w, offset, packed_u16.numel()))
        if min(win_y, win_x, win_h, win_w, src_y, src_x) < 0 or win_y + win_h > ch or win_x + win_w > cw or src_y + win_h > h or src_x + win_w > w:
            raise ValueError("depth_png_keys: window (%d, %d, %d, %d) from source (%d, %d) does not fit a %d x %d plane and a %d x %d canvas"
                             % (win_y, win_x, win_h, win_w, src_y, src_x, h, w, ch, cw))
    nbytes = S * ctypes.sizeof(_lib.DepthPngDesc)
    if desc_table is None:
        desc_table = torch.frombuffer(bytearray(bytes(depth_png_desc_table(descs))), dtype=torch.uint8).to(packed_u16.device)
    elif desc_table.dtype != torch.uint8 or not desc_table.is_cuda or desc_table.numel() != nbytes or not desc_table.is_contiguous() \
            or desc_table.data_ptr() % 8:
        raise ValueError("depth_png_keys: desc_table must be an 8-byte aligned contiguous uint8 CUDA tensor of %d bytes" % nbytes)
    out = torch.empty((S, channels, (ch + pool - 1) // pool, (cw + pool - 1) // pool), device=packed_u16.device, dtype=torch.float32)
    call("fd_depth_png_keys", packed_u16.data_ptr(), packed_u16.numel(), desc_table.data_ptr(), S, ch, cw, pool, channels, float(div0),
         float(div1), out.data_ptr(), stream())
    return out


# ------------------------------------------------------------------------------------ training images (uint8) ---
# datasets/mono_dataset.py:85-104 on the device: Pillow's antialiased Lanczos resample, ColorJitter and ToTensor, bit for bit
# (csrc/augment.hip; the arithmetic is restated in tests/augment_ref.py).  uint8 images are [N,H,W,3].
_LANCZOS_TABLES = {}
_LANCZOS_DEVICE_TABLES = {}
JITTER_OPS = ("brightness", "contrast", "saturation", "hue")


def lanczos_table(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the Lanczos filter, in float64 on the host: int32
    [out_size, 2 + k] rows of (first tap, tap count, k coefficients) and k = 2 * ceil(3 * max(in, out) / out) + 1.  Cached."""
    import math
    import numpy as np
    key = (int(in_size), int(out_size))
    if key in _LANCZOS_TABLES:
        return _LANCZOS_TABLES[key]
    n_in, n_out = key
    if n_in <= 0 or n_out <= 0:
        raise ValueError("lanczos_table: sizes must be positive, got %r" % (key,))
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    k = 2 * ((3 * max(n_in, n_out) + n_out - 1) // n_out) + 1
    inv = 1.0 / filterscale
    tab = np.zeros((n_out, 2 + k), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - first
        ws, total = [], 0.0
        for x in range(count):
            t = (x + first - center + 0.5) * inv
            if -3.0 <= t < 3.0:
                a, b = t * math.pi, t / 3.0 * math.pi
                w = (1.0 if t == 0.0 else math.sin(a) / a) * (1.0 if t == 0.0 else math.sin(b) / b)
            else:
                w = 0.0
            ws.append(w)
            total += w
        tab[xx, 0], tab[xx, 1] = first, count
        for x, w in enumerate(ws):
            if total != 0.0:
                w = w / total
            tab[xx, 2 + x] = int(w * (1 << 22) - 0.5) if w < 0 else int(w * (1 << 22) + 0.5)
    _LANCZOS_TABLES[key] = (tab, k)
    return tab, k


def _lanczos_table_on(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    if key not in _LANCZOS_DEVICE_TABLES:
        tab, k = lanczos_table(in_size, out_size)
        _LANCZOS_DEVICE_TABLES[key] = (torch.from_numpy(tab).to(device), k)
    return _LANCZOS_DEVICE_TABLES[key]


def _need_u8_images(x, what):
    _need_cuda(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
        raise RuntimeError("%s: images must be uint8 [N,H,W,3], got %s %s" % (what, x.dtype, tuple(x.shape)))
    return x.contiguous()


def _mirror_table(mirror, n, device):
    if mirror is None or mirror is False:
        return None
    if torch.is_tensor(mirror):
        if mirror.dtype != torch.int32 or mirror.numel() != n:
            raise RuntimeError("mirror: expected %d int32 flags" % n)
        _need_cuda(mirror)
        return mirror.contiguous()
    flags = [bool(mirror)] * n if isinstance(mirror, bool) else [bool(m) for m in mirror]
    if len(flags) != n:
        raise RuntimeError("mirror: %d flags for %d images" % (len(flags), n))
    return torch.tensor(flags, dtype=torch.int32).to(device) if any(flags) else None


def resize_lanczos_u8(x, size, mirror=None, out=None):
    """``Image.resize((size[1], size[0]), LANCZOS)`` of every image of ``x`` [N,H,W,3] uint8 -> [N,size[0],size[1],3].
    ``mirror``: bool, N bools or an int32 device tensor - those frames are flipped left-right first (kitti_dataset.py:59-60)."""
    x = _need_u8_images(x, "resize_lanczos_u8")
    N, Hin, Win, _ = x.shape
    Hout, Wout = int(size[0]), int(size[1])
    xtab, kx = _lanczos_table_on(Win, Wout, x.device)
    ytab, ky = _lanczos_table_on(Hin, Hout, x.device)
    mir = _mirror_table(mirror, N, x.device)
    if out is None:
        out = torch.empty((N, Hout, Wout, 3), device=x.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, Hout, Wout, 3) or not out.is_contiguous() or out.device != x.device:
        raise RuntimeError("resize_lanczos_u8: out must be a contiguous uint8 [%d,%d,%d,3] tensor on %s" % (N, Hout, Wout, x.device))
    ws = torch.empty((max(query("fd_resize_lanczos_u8_ws_bytes", N, Hin, Win, Hout, Wout), 16),), device=x.device, dtype=torch.uint8)
    call("fd_resize_lanczos_u8", ptr(x), ptr(out), N, Hin, Win, Hout, Wout, xtab.data_ptr(), kx, ytab.data_ptr(), ky,
         mir.data_ptr() if mir is not None else None, ptr(ws), stream())
    return out


def u8_to_planes(x, out=None):
    """``ToTensor``: [N,H,W,3] uint8 -> [N,3,H,W] float32 = v / 255.  ``out``: a batch slot, i.e. a float32 tensor [N,3,H,W] whose
    images are dense (it may be a slice of a larger batch along dim 0, or strided along dim 0)."""
    x = _need_u8_images(x, "u8_to_planes")
    N, H, W, _ = x.shape
    if out is None:
        out = torch.empty((N, 3, H, W), device=x.device, dtype=torch.float32)
    elif (out.dtype != torch.float32 or tuple(out.shape) != (N, 3, H, W) or out.device != x.device or
          tuple(out.stride()[1:]) != (H * W, W, 1) or (N > 1 and out.stride(0) < 3 * H * W)):
        raise RuntimeError("u8_to_planes: out must be float32 [%d,3,%d,%d] with dense images on %s" % (N, H, W, x.device))
    call("fd_u8_to_planes", ptr(x), out.data_ptr(), N, H, W, out.stride(0) if N > 1 else 3 * H * W, stream())
    return out


def _jitter_ops(entry):
    """(factors, order) -> (4 floats, list of distinct op ids); None -> no operation."""
    if entry is None:
        return (1.0, 1.0, 1.0, 0.0), []
    factors, order = entry
    factors, order = [float(f) for f in factors], [int(o) for o in order]
    if len(factors) != 4 or any(o not in (0, 1, 2, 3) for o in order) or len(set(order)) != len(order):
        raise ValueError("jitter: expected ((brightness, contrast, saturation, hue), order of distinct op ids 0..3), got %r" % (entry,))
    return factors, order


def _run_jitter(src, descs, dst_u8, dst_planes, max_pixels):
    """descs: list of (src_off, u8_off, planes_off, plain_off, H, W, factors, order).  The hue offset is formed here, from the Python
    double: trunc(h * 255) mod 256 (the kernel's float32 copy of h could land on the other side of an integer)."""
    n = len(descs)
    table = (_lib.JitterDesc * n)()
    for d, (src_off, u8_off, planes_off, plain_off, H, W, factors, order) in zip(table, descs):
        d.src_off, d.u8_off, d.planes_off, d.plain_off, d.H, d.W, d.n_ops = src_off, u8_off, planes_off, plain_off, H, W, len(order)
        d.factor[:] = list(factors[:3]) + [0.0]
        d.order[:] = list(order) + [0] * (4 - len(order))
        d.hue_shift = int(factors[3] * 255.0) % 256
    dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(src.device)
    ws = torch.empty((query("fd_color_jitter_u8_ws_bytes", n),), device=src.device, dtype=torch.uint8)
    call("fd_color_jitter_u8", ptr(src), src.numel(), ptr(dst_u8), dst_u8.numel() if dst_u8 is not None else 0,
         ptr(dst_planes), dst_planes.numel() if dst_planes is not None else 0, dev_table.data_ptr(), n, int(max_pixels), ptr(ws),
         stream())
    off = query("fd_color_jitter_u8_means_offset", n)
    return ws[off:off + 4 * n].view(torch.int32)


def color_jitter_u8(x, params, planes=False, return_means=False):
    """torchvision ``ColorJitter`` on PIL images, for every image of ``x`` [N,H,W,3] uint8 in one launch sequence.  ``params``: one
    entry per image, ``((brightness, contrast, saturation, hue), order)`` with ``order`` the op ids (0 brightness, 1 contrast,
    2 saturation, 3 hue) in application order, or None to copy the image.  Returns uint8 [N,H,W,3], or with ``planes`` the float32
    [N,3,H,W] ``ToTensor`` of it; with ``return_means`` also the int32 grey level each contrast operation blended towards (-1: none)."""
    x = _need_u8_images(x, "color_jitter_u8")
    N, H, W, _ = x.shape
    if len(params) != N:
        raise ValueError("color_jitter_u8: %d parameter sets for %d images" % (len(params), N))
    out = torch.empty((N, 3, H, W), device=x.device, dtype=torch.float32) if planes else torch.empty_like(x)
    per = 3 * H * W
    descs = []
    for i, entry in enumerate(params):
        factors, order = _jitter_ops(entry)
        descs.append((i * per, -1 if planes else i * per, i * per if planes else -1, -1, H, W, factors, order))
    means = _run_jitter(x.view(-1), descs, None if planes else out.view(-1), out.view(-1) if planes else None, H * W)
    return (out, means) if return_means else out


def image_pyramid(frames_u8, height, width, num_scales, flip=None, jitter=None):
    """The colour keys of a batch (mono_dataset.py:85-104): ``frames_u8`` [N,H,W,3] uint8 decoded frames ->
    ``{("color", s): [N,3,height >> s,width >> s], ("color_aug", s): ...}`` float32.  Scale s is resampled from scale s - 1 (Lanczos,
    chained as the reference does); ``flip``: per-frame left-right mirror of the source.  ``jitter``: None (``color_aug`` is
    ``color``), or one entry per frame: None, a ``(factors, order)`` pair applied at every scale, or a list of ``num_scales`` such
    pairs (a fresh draw per image).  Ten launches whatever N: two resample passes per scale, then the contrast statistics, their
    final pass and one apply pass that reads every level once and writes every plane of ``color`` and ``color_aug`` once."""
    frames_u8 = _need_u8_images(frames_u8, "image_pyramid")
    N = frames_u8.shape[0]
    dev = frames_u8.device
    if jitter is not None and len(jitter) != N:
        raise ValueError("image_pyramid: %d jitter entries for %d frames" % (len(jitter), N))
    sizes = [(int(height) // 2 ** s, int(width) // 2 ** s) for s in range(int(num_scales))]
    if not sizes or min(min(hw) for hw in sizes) < 1:
        raise ValueError("image_pyramid: %dx%d has no %d-level pyramid" % (height, width, num_scales))
    r16 = lambda v: (v + 15) // 16 * 16
    u8_off, pl_off, u8_total, pl_total = [], [], 0, 0
    variants = 2 if jitter is not None else 1
    for h, w in sizes:
        u8_off.append(u8_total)
        pl_off.append(pl_total)
        u8_total += r16(N * h * w * 3)
        pl_total += r16(variants * N * h * w * 3)
    arena = torch.empty((u8_total,), device=dev, dtype=torch.uint8)
    planes = torch.empty((pl_total,), device=dev, dtype=torch.float32)
    levels, cur = [], frames_u8
    for s, (h, w) in enumerate(sizes):
        lvl = arena[u8_off[s]:u8_off[s] + N * h * w * 3].view(N, h, w, 3)
        resize_lanczos_u8(cur, (h, w), mirror=flip if s == 0 else None, out=lvl)
        levels.append(lvl)
        cur = lvl
    descs, out = [], {}
    for s, (h, w) in enumerate(sizes):
        per = 3 * h * w
        out[("color", s)] = planes[pl_off[s]:pl_off[s] + N * per].view(N, 3, h, w)
        if jitter is not None:
            out[("color_aug", s)] = planes[pl_off[s] + N * per:pl_off[s] + 2 * N * per].view(N, 3, h, w)
        else:
            out[("color_aug", s)] = out[("color", s)]
        for n in range(N):
            if jitter is None:
                descs.append((u8_off[s] + n * per, -1, pl_off[s] + n * per, -1, h, w, (1.0, 1.0, 1.0, 0.0), []))
                continue
            entry = jitter[n]
            if isinstance(entry, list):
                if len(entry) != len(sizes):
                    raise ValueError("image_pyramid: a per-image jitter list needs one entry per scale")
                entry = entry[s]
            factors, order = _jitter_ops(entry)
            # one table entry per image: the level is read once, `color` is written from it as read and `color_aug` after the operations
            descs.append((u8_off[s] + n * per, -1, pl_off[s] + (N + n) * per, pl_off[s] + n * per, h, w, factors, order))
    _run_jitter(arena, descs, None, planes, sizes[0][0] * sizes[0][1])
    return out


# ------------------------------------------------------------------------------------ baseline JPEG frames -------
# Pillow's decode of a baseline JPEG, split as include/fdhip.h ("baseline JPEG frames") describes: Huffman decoding on a host pool
# behind the C ABI (ctypes releases the interpreter lock), everything after it in csrc/jpeg.hip.  tests/jpeg_ref.py restates it.
_JPEG_POOL = []


def _round16(n):
    return (n + 15) // 16 * 16


def jpeg_pool():
    """The 16-thread pool ``decode_jpeg_batch`` uses when the caller brings none."""
    if not _JPEG_POOL:
        import concurrent.futures
        _JPEG_POOL.append(concurrent.futures.ThreadPoolExecutor(max_workers=16))
    return _JPEG_POOL[0]


def jpeg_probe(data):
    """``fd_jpeg_probe`` of a bytes-like object -> (status, JpegInfo).  Host only."""
    info = _lib.JpegInfo()
    buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data) if not isinstance(data, bytes) else data
    return _lib.load().fd_jpeg_probe(buf, len(data), ctypes.byref(info)), info


def jpeg_entropy_decode(data, coef, qt):
    """``fd_jpeg_entropy_decode`` into ``coef`` (a contiguous int16 numpy array; its size is ``coef_cap``) and ``qt`` (uint16, 192
    values) -> (status, JpegInfo).  Host only; the reason of a non-zero status is ``_lib.last_error()`` on the calling thread."""
    info = _lib.JpegInfo()
    buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data) if not isinstance(data, bytes) else data
    st = _lib.load().fd_jpeg_entropy_decode(buf, len(data), coef.ctypes.data, coef.size, qt.ctypes.data, ctypes.byref(info))
    return st, info


def _pil_rgb(data):
    import io
    import numpy as np
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img.convert("RGB"))


class JpegBatchJob:
    """The host side of ``decode_jpeg_batch``, started on ``pool`` without blocking the caller: every file is read and probed; the
    worker that finishes the last probe lays out ONE pinned staging buffer (descriptors, then per frame its tables and coefficients
    or, for a frame Pillow decodes, its RGB bytes) and submits the entropy decoders, each writing straight into its slice.
    ``finish(device)`` waits, uploads the buffer once and calls ``fd_jpeg_reconstruct`` once."""
    NAME = "decode_jpeg_batch"

    def __init__(self, files, pool=None):
        import threading
        self.files = list(files)
        if not self.files:
            raise ValueError("%s: no files" % self.NAME)
        if len(self.files) > 65535:
            raise ValueError("%s: %d files in one call; the kernel takes 65535" % (self.NAME, len(self.files)))
        self.pool = pool if pool is not None else jpeg_pool()
        self._lock, self._ready, self._error = threading.Lock(), threading.Event(), None
        self._left = len(self.files)
        self._probed = [None] * len(self.files)
        self._futures = []
        for i, f in enumerate(self.files):
            self.pool.submit(self._probe, i, f)

    # ---- pool side --------------------------------------------------------------------------------------------------------------
    def _probe(self, i, f):
        try:
            if isinstance(f, (bytes, bytearray, memoryview)):
                data = bytes(f)
            else:
                with open(f, "rb") as fh:
                    data = fh.read()
            self._probed[i] = self._probe_one(data)
        except BaseException as e:                               # noqa: B902 - handed to finish()
            with self._lock:
                self._error = self._error or e
        with self._lock:
            self._left -= 1
            last = self._left == 0
        if last:
            self._plan()

    def _probe_one(self, data):
        """-> (data, info of a frame the device half takes, or None with the frame Pillow decoded)."""
        st, info = jpeg_probe(data)
        if st == 0 and info.covered:
            return data, info, None
        return data, None, _pil_rgb(data)                        # not covered, or not a JPEG at all: Pillow decides

    def _plan(self):
        try:
            if self._error is not None:
                return
            n = len(self.files)
            at = _round16(n * ctypes.sizeof(_lib.JpegDesc))
            self._slots, planes = [], 0
            for data, info, rgb in self._probed:
                if info is not None:
                    h, w, need = info.height, info.width, 384 + 2 * info.coef_count
                    planes += _round16(info.coef_count)
                else:
                    h, w, need = rgb.shape[0], rgb.shape[1], 0
                size = _round16(max(need, 3 * h * w))            # a frame whose entropy decoding fails gets Pillow's bytes instead
                self._slots.append((at, size, h, w))
                at += size
            self._upload_bytes, self._plane_bytes = at, planes
            self._staging = torch.empty((at,), dtype=torch.uint8, pin_memory=True)
            self._host = self._staging.numpy()
            self._kinds = [1] * n
            self._futures = [self.pool.submit(self._decode, i) for i in range(n)]
        except BaseException as e:                               # noqa: B902
            self._error = e
        finally:
            self._ready.set()

    def _decode(self, i):
        import numpy as np
        data, info, rgb = self._probed[i]
        at, size, h, w = self._slots[i]
        if info is not None:
            qt = self._host[at:at + 384].view(np.uint16)
            coef = self._host[at + 384:at + 384 + 2 * info.coef_count].view(np.int16)
            st, _ = jpeg_entropy_decode(data, coef, qt)
            if st == 0:
                self._kinds[i] = 0
                return
            rgb = _pil_rgb(data)                                 # a damaged stream: as tolerant, or as strict, as Pillow is
            if rgb.shape[:2] != (h, w):
                raise RuntimeError("decode_jpeg_batch: Pillow decoded %s, the frame header says %s" % (rgb.shape[:2], (h, w)))
        self._host[at:at + 3 * h * w] = rgb.reshape(-1)

    # ---- caller side ------------------------------------------------------------------------------------------------------------
    def wait_host(self):
        """Block until the host phase (read, probe, Huffman decoding or Pillow) is done; raise what it raised.  Returns the layout:
        ``{"staging": the pinned uint8 buffer, "upload_bytes": its size, "plane_bytes": the device-only room behind it,
        "total_bytes": their sum}`` - the descriptor table at the start of the buffer is written by ``finish``."""
        self._ready.wait()
        if self._error is not None:
            raise self._error
        for f in self._futures:
            f.result()
        return {"staging": self._staging, "upload_bytes": self._upload_bytes, "plane_bytes": self._plane_bytes,
                "total_bytes": self._upload_bytes + self._plane_bytes}

    def descriptors(self):
        """A copy of the ``fd_jpeg_desc`` table ``finish`` wrote (a ctypes array of ``_lib.JpegDesc``)."""
        n = len(self.files)
        return (_lib.JpegDesc * n).from_buffer_copy(self._host[:n * ctypes.sizeof(_lib.JpegDesc)].tobytes())

    def finish(self, device="cuda"):
        """-> (groups, stats): ``groups`` = {(H, W): (uint8 [n, H, W, 3] device tensor, input indices)} in order of first
        appearance, all views of one buffer.  Runs on ``device``'s current stream, whichever device is current."""
        self.wait_host()
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("%s runs on the GPU only (got %s); there is no CPU path" % (self.NAME, device))
        with torch.cuda.device(device):
            return self._finish_on(device)

    def _finish_on(self, device):
        n = len(self.files)
        members = {}
        for i, (_, _, h, w) in enumerate(self._slots):
            members.setdefault((h, w), []).append(i)
        out_off, at = [0] * n, 0
        spans = {}
        for (h, w), idx in members.items():
            spans[(h, w)] = at
            for i in idx:
                out_off[i] = at
                at += 3 * h * w
            at = _round16(at)
        out_bytes = max(at, 16)
        table = (_lib.JpegDesc * n)()
        plane_at = self._upload_bytes
        for i, (d, (slot, _, h, w)) in enumerate(zip(table, self._slots)):
            info = self._probed[i][1]
            d.kind, d.width, d.height, d.out_off = self._kinds[i], w, h, out_off[i]
            if self._kinds[i] == 0:
                d.qt_off, d.coef_off, d.plane_off = slot, slot + 384, plane_at
                d.components, d.h_samp, d.v_samp = info.components, info.h_samp, info.v_samp
                plane_at += _round16(info.coef_count)
            else:
                d.coef_off = slot
        nbytes = n * ctypes.sizeof(_lib.JpegDesc)
        import numpy as np
        self._host[:nbytes] = np.frombuffer(table, dtype=np.uint8)
        total = self._upload_bytes + self._plane_bytes
        dev = torch.empty((total,), dtype=torch.uint8, device=device)
        dev[:self._upload_bytes].copy_(self._staging, non_blocking=True)       # the batch's one host-to-device copy
        out = torch.empty((out_bytes,), dtype=torch.uint8, device=device)
        call("fd_jpeg_reconstruct", dev.data_ptr(), total, dev.data_ptr(), n, out.data_ptr(), out_bytes, stream())
        groups = {(h, w): (out[spans[(h, w)]:spans[(h, w)] + len(idx) * 3 * h * w].view(len(idx), h, w, 3), idx)
                  for (h, w), idx in members.items()}
        device_n = sum(1 for k in self._kinds if k == 0)
        return groups, {"device": device_n, "fallback": n - device_n}


def decode_jpeg_batch(files, device="cuda", pool=None):
    """``np.asarray(Image.open(f).convert("RGB"))`` of every file, byte for byte, on the device.  ``files``: paths or ``bytes``.
    Returns ``(frames, stats)``: a list of uint8 [H, W, 3] device tensors - views into one buffer, same-size frames contiguous - and
    ``{"device": n, "fallback": n}``.  Covered baseline streams (include/fdhip.h) are Huffman-decoded on the host pool and finished
    by ``fd_jpeg_reconstruct``; everything else - progressive, CMYK, a PNG, a damaged stream - is decoded by Pillow into the same
    staging buffer and copied by the same call.  One host-to-device copy and one library call whatever the number of files."""
    groups, stats = JpegBatchJob(files, pool).finish(device)
    frames = [None] * len(files)
    for stack, idx in groups.values():
        for k, i in enumerate(idx):
            frames[i] = stack[k]
    return frames, stats


# ------------------------------------------------------------------------------------------------ PNG frames -------
# Pillow's decode of a PNG, split as include/fdhip.h ("PNG frames") describes: the chunk walk and the inflate on a host pool behind
# the C ABI (ctypes releases the interpreter lock), the scanline filters in csrc/png.hip.  tests/png_ref.py restates it.
PNG_BAND_ROWS = 512          # FD_PNG_BAND_ROWS: the rows one workgroup of k_png_unfilter holds at a time
PNG_MODES = {"rgb": 0, "gray16": 1}


def png_probe(data):
    """``fd_png_probe`` of a bytes-like object -> (status, PngInfo).  Host only."""
    info = _lib.PngInfo()
    buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data) if not isinstance(data, bytes) else data
    return _lib.load().fd_png_probe(buf, len(data), ctypes.byref(info)), info


def png_inflate(data, dst):
    """``fd_png_inflate`` into ``dst`` (a contiguous uint8 numpy array; its size is ``dst_cap``) -> (status, PngInfo).  Host only; the
    reason of a non-zero status is ``_lib.last_error()`` on the calling thread."""
    info = _lib.PngInfo()
    buf = (ctypes.c_ubyte * len(data)).from_buffer_copy(data) if not isinstance(data, bytes) else data
    return _lib.load().fd_png_inflate(buf, len(data), dst.ctypes.data, dst.size, ctypes.byref(info)), info


def _pil_gray16(data, name="<bytes>"):
    """``np.asarray(Image.open(f))`` as uint16, with the completion loader's single-channel-integer check."""
    import io
    import numpy as np
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        a = np.asarray(img)
    if a.ndim != 2 or a.dtype.kind not in "ui":
        raise RuntimeError("decode_png_batch: %s decoded to %s %s, expected a single-channel integer depth map" % (name, a.dtype, a.shape))
    if a.size and (int(a.max()) > 65535 or int(a.min()) < 0):
        raise RuntimeError("decode_png_batch: %s holds values outside 16 bits" % name)
    return a.astype(np.uint16)


class PngBatchJob(JpegBatchJob):
    """The host side of ``decode_png_batch``; ``JpegBatchJob``'s structure: every file is read and probed on ``pool``; the worker
    that finishes the last probe lays out ONE pinned staging buffer (descriptors, then per frame its filtered scanlines or, for a frame
    Pillow decodes, its finished bytes) and submits the inflates, each writing straight into its slice with the interpreter lock
    released.  ``finish(device)`` waits, uploads the buffer once and calls ``fd_png_unfilter`` once.  ``mode``: ``"rgb"`` (8-bit RGB
    and grey files on the device, uint8 [H, W, 3] frames) or ``"gray16"`` (16-bit grey files on the device, uint16 [H, W] frames);
    every other file is Pillow's."""
    NAME = "decode_png_batch"

    def __init__(self, files, pool=None, mode="rgb"):
        if mode not in PNG_MODES:
            raise ValueError("decode_png_batch: mode must be 'rgb' or 'gray16', got %r" % (mode,))
        self.mode = mode
        self._elem = 2 if mode == "gray16" else 3                # output bytes per pixel
        super().__init__(files, pool)

    def _pil(self, data, i):
        name = self.files[i] if isinstance(self.files[i], str) else "<bytes %d>" % i
        return _pil_gray16(data, name) if self.mode == "gray16" else _pil_rgb(data)

    def _probe_one(self, data):
        st, info = png_probe(data)
        if st == 0 and info.covered and (info.bpp == 2) == (self.mode == "gray16"):
            return data, info, None
        return data, None, False                                 # Pillow decodes it in _decode, straight into the buffer

    def _plan(self):
        try:
            if self._error is not None:
                return
            import io
            from PIL import Image
            n = len(self.files)
            at = _round16(n * ctypes.sizeof(_lib.PngDesc))
            self._slots = []
            for data, info, _ in self._probed:
                if info is not None:
                    h, w, need = info.height, info.width, info.raw_bytes
                else:                                            # the size from the header alone; Pillow raises for what it cannot open
                    with Image.open(io.BytesIO(data)) as img:
                        w, h = img.size
                    need = 0
                size = _round16(max(need, self._elem * h * w))   # a frame whose inflate fails gets Pillow's bytes instead
                self._slots.append((at, size, h, w))
                at += size
            self._upload_bytes, self._plane_bytes = at, 0
            self._staging = torch.empty((at,), dtype=torch.uint8, pin_memory=True)
            self._host = self._staging.numpy()
            self._kinds = [1] * n
            self._futures = [self.pool.submit(self._decode, i) for i in range(n)]
        except BaseException as e:                               # noqa: B902
            self._error = e
        finally:
            self._ready.set()

    def _decode(self, i):
        import numpy as np
        data, info, _ = self._probed[i]
        at, size, h, w = self._slots[i]
        if info is not None:
            st, _ = png_inflate(data, self._host[at:at + info.raw_bytes])
            if st == 0:
                self._kinds[i] = 0
                return
        px = self._pil(data, i)                                  # not covered, or damaged: as tolerant, or as strict, as Pillow is
        if px.shape[:2] != (h, w):
            raise RuntimeError("decode_png_batch: Pillow decoded %s, the header says %s" % (px.shape[:2], (h, w)))
        self._host[at:at + self._elem * h * w] = np.ascontiguousarray(px).reshape(-1).view(np.uint8)

    def descriptors(self):
        """A copy of the ``fd_png_desc`` table ``finish`` wrote (a ctypes array of ``_lib.PngDesc``)."""
        n = len(self.files)
        return (_lib.PngDesc * n).from_buffer_copy(self._host[:n * ctypes.sizeof(_lib.PngDesc)].tobytes())

    def layout(self, out_base=0):
        """-> (table, out_off per frame, {(h, w): first byte}, {(h, w): indices}, out bytes): same-size frames contiguous, in order of
        first appearance, the groups 16-byte aligned from ``out_base`` on."""
        n = len(self.files)
        members = {}
        for i, (_, _, h, w) in enumerate(self._slots):
            members.setdefault((h, w), []).append(i)
        out_off, at, spans = [0] * n, out_base, {}
        for (h, w), idx in members.items():
            spans[(h, w)] = at
            for i in idx:
                out_off[i] = at
                at += self._elem * h * w
            at = _round16(at)
        table = (_lib.PngDesc * n)()
        for i, (d, (slot, _, h, w)) in enumerate(zip(table, self._slots)):
            info = self._probed[i][1]
            d.kind, d.width, d.height, d.raw_off, d.out_off, d.mode = self._kinds[i], w, h, slot, out_off[i], PNG_MODES[self.mode]
            d.bpp = info.bpp if self._kinds[i] == 0 else 0
        return table, out_off, spans, members, max(at, 16)

    def run(self, device, out, table):
        """Upload the staging buffer (with ``table`` at its head) and make the one library call into ``out``, a uint8 device tensor."""
        import numpy as np
        n = len(self.files)
        self._host[:n * ctypes.sizeof(_lib.PngDesc)] = np.frombuffer(table, dtype=np.uint8)
        dev = torch.empty((self._upload_bytes,), dtype=torch.uint8, device=device)
        dev.copy_(self._staging, non_blocking=True)              # the batch's one host-to-device copy
        call("fd_png_unfilter", dev.data_ptr(), self._upload_bytes, ctypes.addressof(table), n, out.data_ptr(), out.numel(), stream())
        device_n = sum(1 for k in self._kinds if k == 0)
        return {"device": device_n, "fallback": n - device_n}

    def _finish_on(self, device):
        table, _, spans, members, out_bytes = self.layout()
        out = torch.empty((out_bytes,), dtype=torch.uint8, device=device)
        stats = self.run(device, out, table)
        groups = {}
        for (h, w), idx in members.items():
            flat = out[spans[(h, w)]:spans[(h, w)] + len(idx) * self._elem * h * w]
            groups[(h, w)] = (flat.view(torch.uint16).view(len(idx), h, w) if self.mode == "gray16" else flat.view(len(idx), h, w, 3), idx)
        return groups, stats


def decode_png_batch(files, device="cuda", pool=None, mode="rgb"):
    """``np.asarray(Image.open(f).convert("RGB"))`` of every file (``mode="rgb"``: uint8 [H, W, 3]) or ``np.asarray(Image.open(f))`` of
    every 16-bit depth map (``mode="gray16"``: uint16 [H, W]), value for value, on the device.  ``files``: paths or ``bytes``.
    Returns ``(frames, stats)``: a list of device tensors - views into one buffer, same-size frames contiguous - and ``{"device": n,
    "fallback": n}``.  Covered files (include/fdhip.h: non-interlaced 8-bit RGB and 8-bit grey in ``rgb`` mode, 16-bit grey in
    ``gray16`` mode) are inflated on the host pool and unfiltered by ``fd_png_unfilter``; everything else - palette, alpha, tRNS,
    Adam7, other depths, a damaged file, a JPEG - is decoded by Pillow into the same staging buffer and copied by the same call.
    One host-to-device copy and one library call whatever the number of files."""
    groups, stats = PngBatchJob(files, pool, mode).finish(device)
    frames = [None] * len(files)
    for stack, idx in groups.values():
        for k, i in enumerate(idx):
            frames[i] = stack[k]
    return frames, stats


# ------------------------------------------------------------------------------------------------ PNG outputs ------
# The encoder of include/fdhip.h ("PNG outputs"): filter, token counts, bit placement and the file's bytes in csrc/png_enc.hip, the
# Huffman plan and the CRC-32s on the host behind the C ABI (csrc/png_deflate.h).  tests/png_enc_ref.py restates the stream.
PNG_ENC_BLOCK_ROWS = 64      # FD_PNG_ENC_BLOCK_ROWS
PNG_ENCODERS = ("pil", "device")


def check_png_encoder(name, who="png_encoder"):
    if name not in PNG_ENCODERS:
        raise ValueError("%s must be 'pil' or 'device', got %r" % (who, name))
    return name


def png_enc_layout(shapes):
    """``fd_png_enc_layout`` of [(width, height, bpp)] -> (a ctypes array of ``_lib.PngEncDesc``, ``_lib.PngEncSizes``).  Host only;
    a shape the encoder does not cover is a ValueError."""
    table = (_lib.PngEncDesc * max(len(shapes), 1))()
    for d, (w, h, bpp) in zip(table, shapes):
        d.width, d.height, d.bpp = min(int(w), 1 << 30), min(int(h), 1 << 30), int(bpp)      # the library refuses what is too large
    sizes = _lib.PngEncSizes()
    if _lib.load().fd_png_enc_layout(table, len(shapes), ctypes.byref(sizes)) != 0:
        raise ValueError(_lib.last_error())
    return table, sizes


def png_enc_plan(table, n, stats, blocks=None):
    """``fd_png_enc_plan``: ``stats`` = the contiguous uint32 numpy array launch A leaves (histograms, then Adler pairs) -> (blocks, total
    bytes); ``table`` gets every file's offset, size and Adler-32.  ``blocks``: the address of room for the batch's ``_lib.PngEncBlock``
    table, else one is allocated.  Host only."""
    keep = None
    if blocks is None:
        keep = (_lib.PngEncBlock * int(table[n - 1].first_block + (table[n - 1].height + PNG_ENC_BLOCK_ROWS - 1) // PNG_ENC_BLOCK_ROWS))()
        blocks = ctypes.addressof(keep)
    total = ctypes.c_long(0)
    if _lib.load().fd_png_enc_plan(table, n, stats.ctypes.data, blocks, ctypes.byref(total)) != 0:
        raise RuntimeError("fd_png_enc_plan failed: %s" % _lib.last_error())
    return keep, total.value


def png_enc_finish(files, desc):
    """``fd_png_enc_finish``: the three CRC-32s of ``desc``'s file inside ``files`` (a contiguous uint8 numpy array), in place.  Host
    only; the interpreter lock is released while it runs."""
    if _lib.load().fd_png_enc_finish(files.ctypes.data, files.size, ctypes.byref(desc)) != 0:
        raise RuntimeError("fd_png_enc_finish failed: %s" % _lib.last_error())


def _png_enc_kind(x, i):
    """-> (height, width, bpp) of one image of ``encode_png_batch``; ValueError for a dtype or rank the encoder does not cover."""
    import numpy as np
    shape, dt = tuple(x.shape), x.dtype
    u8 = dt in (torch.uint8, np.dtype(np.uint8))
    u16 = dt in (torch.uint16, np.dtype(np.uint16))
    if u8 and len(shape) == 3 and shape[2] == 3:
        bpp = 3
    elif u8 and len(shape) == 2:
        bpp = 1
    elif u16 and len(shape) == 2:
        bpp = 2
    else:
        raise ValueError("encode_png_batch: image %d is %s %s, none of uint8 [H,W,3], uint8 [H,W], uint16 [H,W]" % (i, dt, list(shape)))
    h, w = shape[0], shape[1]                                    # their limits are fd_png_enc_layout's to check
    return h, w, bpp


class PngEncodeJob:
    """``encode_png_batch`` in its two halves, so that a caller can put work between them: the constructor checks the images, uploads
    the host ones in one copy and issues launch A and the download of its statistics; ``finish()`` waits for them, plans, issues
    launches B and C and the download of the files, waits, and fills the CRC-32s on ``pool``."""

    def __init__(self, images, pool=None, device=None):
        import numpy as np
        images = list(images)
        if not images:
            raise ValueError("encode_png_batch: no images")
        kinds = []
        for i, x in enumerate(images):
            if not isinstance(x, (torch.Tensor, np.ndarray)):
                raise ValueError("encode_png_batch: image %d is a %s, not a tensor or an array" % (i, type(x).__name__))
            kinds.append(_png_enc_kind(x, i))
        self.pool = pool if pool is not None else jpeg_pool()
        self.n = n = len(images)
        self.table, self.sizes = png_enc_layout([(w, h, bpp) for h, w, bpp in kinds])
        dev = [x.device for x in images if isinstance(x, torch.Tensor) and x.is_cuda]
        self.device = torch.device(device) if device is not None else (dev[0] if dev else torch.device("cuda", torch.cuda.current_device()))
        if self.device.type != "cuda":
            raise RuntimeError("encode_png_batch runs on the GPU only (got %s); there is no CPU path" % self.device)
        host = [(i, x.numpy() if isinstance(x, torch.Tensor) else x) for i, x in enumerate(images)
                if not (isinstance(x, torch.Tensor) and x.is_cuda)]
        self._keep = []
        with torch.cuda.device(self.device):
            src = [None] * n
            if host:                                             # the host images: one pinned buffer, one upload
                at, slots = 0, []
                for i, a in host:
                    slots.append(at)
                    at += _round16(a.nbytes)
                pinned = torch.empty((at,), dtype=torch.uint8, pin_memory=True)
                flat = pinned.numpy()
                for (i, a), s in zip(host, slots):
                    flat[s:s + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
                up = torch.empty((at,), dtype=torch.uint8, device=self.device)
                up.copy_(pinned, non_blocking=True)
                self._keep += [pinned, up]
                for (i, _), s in zip(host, slots):
                    src[i] = up.data_ptr() + s
            for i, x in enumerate(images):
                if src[i] is None:
                    if x.device != self.device:
                        raise ValueError("encode_png_batch: image %d lives on %s, the batch on %s" % (i, x.device, self.device))
                    x = x.contiguous()
                    self._keep.append(x)
                    src[i] = x.data_ptr()
            for d, p in zip(self.table, src):
                d.src = p
            sz = self.sizes
            self.work = torch.empty((sz.work_bytes,), dtype=torch.uint8, device=self.device)
            call("fd_png_enc_filter", self.work.data_ptr(), sz.work_bytes, ctypes.addressof(self.table), n, stream())
            self._stats = torch.empty((sz.stat_bytes,), dtype=torch.uint8, pin_memory=True)
            self._stats.copy_(self.work[sz.stat_off:sz.stat_off + sz.stat_bytes], non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()

    def finish(self):
        """-> (files, stats) of ``encode_png_batch``."""
        import numpy as np
        sz, n = self.sizes, self.n
        with torch.cuda.device(self.device):
            self._event.synchronize()
            blocks = torch.empty((sz.blocks * ctypes.sizeof(_lib.PngEncBlock),), dtype=torch.uint8, pin_memory=True)
            _, total = png_enc_plan(self.table, n, self._stats.numpy().view(np.uint32), blocks.data_ptr())
            room = (total + 3) // 4 * 4 + 4
            out = torch.empty((room,), dtype=torch.uint8, device=self.device)
            call("fd_png_enc_emit", self.work.data_ptr(), sz.work_bytes, ctypes.addressof(self.table), n, blocks.data_ptr(),
                 out.data_ptr(), room, stream())
            pinned = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
            pinned.copy_(out[:total], non_blocking=True)         # exactly the sum of the file sizes
            torch.cuda.current_stream().synchronize()
        flat = pinned.numpy()
        for f in [self.pool.submit(png_enc_finish, flat, self.table[i]) for i in range(n)]:
            f.result()
        view = memoryview(flat)
        files = [view[d.out_off:d.out_off + d.out_bytes] for d in list(self.table)[:n]]
        self._keep = self.work = None
        return files, {"bytes": int(total), "raw_bytes": int(sz.raw_bytes)}


def encode_png_batch(images, pool=None):
    """PNG files of ``images`` - device tensors, or host tensors / numpy arrays (uploaded in one copy), each uint8 [H, W, 3], uint8
    [H, W] or uint16 [H, W]; sizes and kinds may differ - that decode to the input value for value.  Returns ``(files, stats)``: one
    ``memoryview`` per image into ONE pinned buffer, complete files ready to be written, and ``{"bytes": their total size,
    "raw_bytes": the scanline bytes they hold}``.  Three launches, three small uploads and two downloads whatever the number of images;
    anything else is a ValueError before the GPU is touched."""
    return PngEncodeJob(images, pool).finish()


# ------------------------------------------------------------------------------------------------ JPEG outputs -----
# The encoder of include/fdhip.h ("JPEG outputs"): pixels to stuffed entropy-coded bytes in csrc/jpeg_enc.hip, the tables, the layout
# and the header bytes on the host behind the C ABI (csrc/jpeg_enc_host.h).  tests/jpeg_enc_ref.py restates the stream.
JPEG_ENC_HEADER_BYTES = 623  # FD_JPEG_ENC_HEADER_BYTES
JPEG_SAMPLINGS = {"1x1": (1, 1), "2x1": (2, 1), "2x2": (2, 2)}
JPEG_SUBSAMPLING = {"1x1": 0, "2x1": 1, "2x2": 2}                # Pillow's name for the same three
JPEG_ENCODERS = ("pil", "device")


def jpeg_enc_quant_tables(quality):
    """``fd_jpeg_enc_quant_tables`` -> uint16 [2, 64] numpy array in zigzag order.  Host only."""
    import numpy as np
    zz = np.zeros((2, 64), np.uint16)
    if _lib.load().fd_jpeg_enc_quant_tables(int(quality), zz.ctypes.data) != 0:
        raise ValueError(_lib.last_error())
    return zz


def jpeg_enc_header(width, height, sampling, quality, dst=None):
    """``fd_jpeg_enc_header`` -> the header bytes of a file (or written at the start of ``dst``, a contiguous uint8 numpy array).  Host only."""
    import numpy as np
    hs, vs = JPEG_SAMPLINGS[sampling] if isinstance(sampling, str) else sampling
    buf = np.zeros((JPEG_ENC_HEADER_BYTES,), np.uint8) if dst is None else dst
    if _lib.load().fd_jpeg_enc_header(int(width), int(height), int(hs), int(vs), int(quality), buf.ctypes.data, buf.size) != 0:
        raise ValueError(_lib.last_error())
    return buf.tobytes() if dst is None else None


def jpeg_enc_layout(shapes):
    """``fd_jpeg_enc_layout`` of [(width, height, hs, vs)] -> (a ctypes array of ``_lib.JpegEncDesc``, ``_lib.JpegEncSizes``).  Host only;
    a shape the encoder does not cover is a ValueError."""
    table = (_lib.JpegEncDesc * max(len(shapes), 1))()
    for d, (w, h, hs, vs) in zip(table, shapes):
        d.width, d.height, d.hs, d.vs = min(int(w), 1 << 30), min(int(h), 1 << 30), int(hs), int(vs)
    sizes = _lib.JpegEncSizes()
    if _lib.load().fd_jpeg_enc_layout(table, len(shapes), ctypes.byref(sizes)) != 0:
        raise ValueError(_lib.last_error())
    return table, sizes


def _pil_jpeg(a, quality, sampling=None):
    """The file Pillow writes for a uint8 [H, W] (mode L) or [H, W, 3] array."""
    import io
    from PIL import Image
    f = io.BytesIO()
    if a.ndim == 2:
        Image.fromarray(a).save(f, "JPEG", quality=quality)
    else:
        Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=JPEG_SUBSAMPLING[sampling])
    return f.getvalue()


def check_jpeg_params(quality, sampling, n, who="encode_jpeg_batch"):
    """-> the per-image list of sampling names; ValueError for a bad ``quality`` or ``sampling``."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("%s: quality must be an int in 1 .. 100, got %r" % (who, quality))
    names = [sampling] * n if isinstance(sampling, str) else (list(sampling) if isinstance(sampling, (list, tuple)) else [None])
    if len(names) != n or any(not isinstance(s, str) or s not in JPEG_SAMPLINGS for s in names):
        raise ValueError("%s: sampling must be '1x1', '2x1' or '2x2' (or one of them per image), got %r" % (who, sampling))
    return names


def encode_jpeg_batch(images, quality=92, sampling="2x2", pool=None):
    """The JPEG files Pillow writes for ``Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=...)``, byte for byte, of
    ``images`` - device tensors, or host tensors / numpy arrays (uploaded in one copy), uint8 [H, W, 3] of any mix of sizes.
    ``sampling``: '1x1', '2x1' or '2x2' (Pillow's subsampling 0, 1, 2), or a list with one per image.  Returns ``(files, stats)``: one
    ``memoryview`` per image into ONE pinned buffer, complete files ready to be written, and ``{"device": n, "fallback": n, "bytes":
    their total size}``.  A uint8 [H, W] image is outside the covered set: Pillow encodes it (mode L) into the same buffer and it is
    counted as ``fallback``.  One library call of seven launches whatever the number of images; any other dtype or rank, a zero or
    over-large side, a bad ``quality`` or ``sampling`` is a ValueError before the GPU is touched."""
    import numpy as np
    images = list(images)
    if not images:
        raise ValueError("encode_jpeg_batch: no images")
    names = check_jpeg_params(quality, sampling, len(images))
    colour, grey = [], []
    for i, x in enumerate(images):
        if not isinstance(x, (torch.Tensor, np.ndarray)):
            raise ValueError("encode_jpeg_batch: image %d is a %s, not a tensor or an array" % (i, type(x).__name__))
        shape = tuple(x.shape)
        if x.dtype not in (torch.uint8, np.dtype(np.uint8)) or not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
            raise ValueError("encode_jpeg_batch: image %d is %s %s, neither uint8 [H,W,3] nor uint8 [H,W]" % (i, x.dtype, list(shape)))
        if not (1 <= shape[0] <= 65535 and 1 <= shape[1] <= 65535):
            raise ValueError("encode_jpeg_batch: image %d is %d x %d, a side outside 1 .. 65535" % (i, shape[0], shape[1]))
        (colour if len(shape) == 3 else grey).append(i)
    on = [(i, images[i].device) for i in colour if isinstance(images[i], torch.Tensor) and images[i].is_cuda]
    for i, dv in on:                                             # one device per batch: the first device image's
        if dv != on[0][1]:
            raise ValueError("encode_jpeg_batch: image %d lives on %s, the batch on %s" % (i, dv, on[0][1]))
    pool = pool if pool is not None else jpeg_pool()
    grey_jobs = {i: pool.submit(_pil_jpeg, images[i].cpu().numpy() if isinstance(images[i], torch.Tensor) else np.ascontiguousarray(images[i]),
                                quality) for i in grey}
    results, out, device = None, None, None
    if colour:
        table, sizes = jpeg_enc_layout([(images[i].shape[1], images[i].shape[0]) + JPEG_SAMPLINGS[names[i]] for i in colour])
        dev = [images[i].device for i in colour if isinstance(images[i], torch.Tensor) and images[i].is_cuda]
        device = dev[0] if dev else torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(device):
            keep, src = [], {}
            host = [(i, images[i].numpy() if isinstance(images[i], torch.Tensor) else images[i]) for i in colour
                    if not (isinstance(images[i], torch.Tensor) and images[i].is_cuda)]
            if host:                                             # the host images: one pinned buffer, one upload
                at, slots = 0, []
                for i, a in host:
                    slots.append(at)
                    at += _round16(a.nbytes)
                pinned = torch.empty((at,), dtype=torch.uint8, pin_memory=True)
                flat = pinned.numpy()
                for (i, a), s in zip(host, slots):
                    flat[s:s + a.nbytes] = np.ascontiguousarray(a).reshape(-1)
                up = torch.empty((at,), dtype=torch.uint8, device=device)
                up.copy_(pinned, non_blocking=True)
                keep += [pinned, up]
                for (i, _), s in zip(host, slots):
                    src[i] = up.data_ptr() + s
            for i in colour:
                if i not in src:
                    x = images[i].contiguous()
                    keep.append(x)
                    src[i] = x.data_ptr()
            for d, i in zip(table, colour):
                d.src = src[i]
            n = len(colour)
            work = torch.empty((sizes.work_bytes,), dtype=torch.uint8, device=device)
            out = torch.empty((sizes.out_bytes,), dtype=torch.uint8, device=device)
            call("fd_jpeg_enc_encode", work.data_ptr(), sizes.work_bytes, ctypes.addressof(table), n, quality, out.data_ptr(), sizes.out_bytes,
                 stream())
            rows = torch.empty((sizes.result_bytes,), dtype=torch.uint8, pin_memory=True)
            rows.copy_(work[sizes.result_off:sizes.result_off + sizes.result_bytes], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            results = (_lib.JpegEncResult * n).from_buffer_copy(rows.numpy().tobytes())
    grey_files = {i: f.result() for i, f in grey_jobs.items()}
    device_bytes = sum(r.out_bytes for r in results) if results is not None else 0
    total = device_bytes + sum(len(f) for f in grey_files.values())
    pinned = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    flat = pinned.numpy()
    if colour:
        if results[len(colour) - 1].out_off + results[len(colour) - 1].out_bytes != device_bytes or device_bytes > sizes.out_bytes:
            raise RuntimeError("encode_jpeg_batch: the files' sizes do not add up")
        with torch.cuda.device(device):
            pinned[:device_bytes].copy_(out[:device_bytes], non_blocking=True)     # exactly the sum of the file sizes
            torch.cuda.current_stream().synchronize()
    view, files, at = memoryview(flat), [None] * len(images), device_bytes
    for k, i in enumerate(colour):
        r, d = results[k], table[k]
        jpeg_enc_header(d.width, d.height, (d.hs, d.vs), quality, flat[r.out_off:r.out_off + JPEG_ENC_HEADER_BYTES])
        files[i] = view[r.out_off:r.out_off + r.out_bytes]
    for i in grey:
        data = grey_files[i]
        flat[at:at + len(data)] = np.frombuffer(data, np.uint8)
        files[i] = view[at:at + len(data)]
        at += len(data)
    return files, {"device": len(colour), "fallback": len(grey), "bytes": int(total)}
