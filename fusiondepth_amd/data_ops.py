"""Data preparation on the GPU, no autograd: the LiDAR scatter and rasterisation, scan sparsification, the batched bilinear resize
and the uint8 image pipeline (Lanczos resample, colour jitter, ``image_pyramid``) that build a training batch."""
import ctypes

import torch

from . import _lib
from ._lib import _empty, _need_cuda, call, f32, ptr, query, round16, stream


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
    u8_off, pl_off, u8_total, pl_total = [], [], 0, 0
    variants = 2 if jitter is not None else 1
    for h, w in sizes:
        u8_off.append(u8_total)
        pl_off.append(pl_total)
        u8_total += round16(N * h * w * 3)
        pl_total += round16(variants * N * h * w * 3)
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
