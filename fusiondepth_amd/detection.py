"""The KITTI 3-D object detection side of the reference: its ``KITTIDetecDataset`` (datasets/kitti_dataset.py:13-25, 176-239), the
``detec`` / ``detec4beam`` ground-truth exports (export_gt_depth.py:13-25, 71-75, 81-85) and the dense part of ``export_detection.py``
(:317-392) - the depth maps, at each image's own size, as the 16-bit PNG payload the monocular 3-D detector is trained on.

  * ``detec_calib_date(height, width)`` / ``image_size(path)``   the object set has no per-date folders: the reference picks the raw
    recording date whose rectified image size the frame has (``get_detec_calib``).  It decodes the image with OpenCV for that;
    only the size is needed, and PIL reads it from the file header.
  * ``KITTIDetecBatches``           ``KITTIRAWBatches`` over the object layout: 6-digit frame names, calibration chosen by image size.
  * ``export_gt_depths_detec`` / ``detec_output_name``   ``gt_depths.npz`` / ``4beam.npz`` of ``splits/detection``.
  * ``depth_export``                ``fd_depth_export`` (csrc/detection.hip): resize, invert, scale and quantise N maps of different
    sizes in one library call per chunk; ``quantize_u16``: the same quantiser on the float64 map GDC produces.
  * ``points_export``               ``fd_points_export`` (csrc/pseudo_lidar.hip): pseudo-LiDAR clouds, the other half of the
    Pseudo-LiDAR family this project's LiDAR pipeline comes from (``project_depth_to_points``) - N float32 maps of different sizes
    back-projected into the Velodyne frame, filtered and compacted in three launches per chunk, one download of the kept points.

The point rule.  For pixel column ``u``, row ``v`` (integers) and ``z = float64(depth[v, u])``, with ``Calibration``'s camera-2 scalars and
``(A, t) = kitti_utils.rect_to_velo(date folder)``, all in float64, each operation rounded once, no contraction, in this order:
    x = ((u - c_u) * z) / f_u + b_x
    y = ((v - c_v) * z) / f_v + b_y
    X = ((A00*x + A01*y) + A02*z) + t0                  # Y, Z likewise with rows 1, 2
    keep = (X >= 0) & (Z < max_high)                    # max_high defaults to 1.0 m; NaN falls out through the comparisons
    point = float32(X), float32(Y), float32(Z), 1.0f
Kept points follow in row-major pixel order (numpy's boolean indexing), images back to back; there are no other filters
(tests/pseudo_lidar_ref.py restates it in numpy).

Deviations from the reference, on purpose
  * an image size outside ``get_detec_calib``'s table raises ``ValueError`` naming it (the reference returns ``None`` and fails later).
  * ``batch["date"]`` of ``KITTIDetecBatches`` is the calibration date chosen from the image size, where the reference gives the first
    path component of the line (``training``): ``--eval_gdc`` needs the date to find ``calib_cam_to_cam.txt``.
  * the calibration lives under ``<data_path>/<date>`` (the reference hardcodes ``kitti_data/<date>`` relative to the working directory).
  * out of the ``uint16`` range numpy's ``astype`` is undefined; the quantiser defines it: NaN and negative -> 0, ``>= 65535`` -> 65535.
  * the pseudo-LiDAR calibration is the recording DATE's (``calib_cam_to_cam.txt`` / ``calib_velo_to_cam.txt``, chosen from the image
    size like everything else here), not the object set's per-frame ``calib/*.txt`` that Pseudo-LiDAR reads.
  * the matrix products of the point rule are written out in this project's order, so a cloud agrees with Pseudo-LiDAR's ``np.dot``
    chain to float64 rounding (far below the float32 it is stored in), not to the bit.
No CPU fallback: ``depth_export``, ``points_export`` and the loader need the GPU; the path rules and the table do not.
"""
import ctypes
import os
import threading

import numpy as np
import torch

from . import _lib
from .datasets import SIDE_MAP, KITTIRAWBatches

# datasets/kitti_dataset.py:13-25 (the same table in export_gt_depth.py, export_detection.py and gen2channel_detec.py)
DETEC_CALIB_DATES = {(375, 1242): "2011_09_26", (370, 1224): "2011_09_28", (374, 1238): "2011_09_29", (370, 1226): "2011_09_30",
                     (376, 1241): "2011_10_03"}
# numpy mirror of ``fd_export_desc`` (24 bytes, as ``_lib.ExportDesc``)
EXPORT_DESC = np.dtype([("offset", np.int64), ("H", np.int32), ("W", np.int32), ("pred", np.int32), ("reserved", np.int32)])
assert EXPORT_DESC.itemsize == ctypes.sizeof(_lib.ExportDesc)


def detec_calib_date(height, width):
    """``get_detec_calib``: the raw recording date whose rectified images are ``height`` x ``width``."""
    key = (int(height), int(width))
    if key not in DETEC_CALIB_DATES:
        raise ValueError("detec_calib_date: no KITTI recording date has %d x %d images (known sizes: %s)"
                         % (key[0], key[1], ", ".join("%dx%d" % k for k in sorted(DETEC_CALIB_DATES))))
    return DETEC_CALIB_DATES[key]


def image_size(path):
    """(height, width) of an image file, from its header: PIL opens lazily, no pixel is decoded."""
    from PIL import Image
    with Image.open(path) as img:
        width, height = img.size
    return int(height), int(width)


class KITTIDetecBatches(KITTIRAWBatches):
    """``KITTIRAWBatches`` over the KITTI object layout (``KITTIDetecDataset``): frames are ``{:06d}`` names under
    ``<folder>/image_0{2,3}/data``, ``<folder>/velodyne_points/data`` and the beam folder - ``4beam``, or ``random{N}`` when
    ``opt.random_sample != -1`` (this class's rule in the reference; the raw class tests ``> 0``).  The calibration folder of a line
    is ``<data_path>/<detec_calib_date(size of its image_02 frame)>`` - always ``image_02``, whatever the side, as in the reference -
    cached per (folder, frame).  ``batch["date"]`` is that date, NOT the line's first path component as in the reference (module
    docstring).  Same arguments and every other key as the parent; the ``2channel`` maps are computed online as there.
    ``lidar_source="raw"`` is refused: the sparsifier has no key for this layout."""

    def __init__(self, *args, **kwargs):
        self._dates = {}
        super().__init__(*args, **kwargs)
        if self.lidar_source == "raw":
            raise NotImplementedError("KITTIDetecBatches: lidar_source='raw' is not covered (no sparsifier key for the object layout); "
                                      "write the 4beam / random{N} scans offline")

    # ---- paths (kitti_dataset.py:183-225) ---------------------------------------------------------------------------------------
    def get_image_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, folder, "image_0{}/data".format(SIDE_MAP[side]), "{:06d}{}".format(frame_index, self.img_ext))

    def get_velo_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "velodyne_points/data/{:06d}.bin".format(int(frame_index)))

    def beam_folder(self):
        random_sample = self._opt("random_sample", -1)
        return "random{}".format(random_sample) if random_sample != -1 else "4beam"

    def get_beam_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "{}/{:06d}.bin".format(self.beam_folder(), int(frame_index)))

    def calib_date(self, folder, frame_index):
        key = (folder, int(frame_index))
        if key not in self._dates:
            path = os.path.join(self.data_path, folder, "image_02/data/{:06d}.png".format(int(frame_index)))
            self._dates[key] = detec_calib_date(*image_size(path))
        return self._dates[key]

    def plan_batch(self, epoch, indices):
        items = super().plan_batch(epoch, indices)
        for it in items:                                         # the date selects the projection and becomes batch["date"]
            it["date"] = self.calib_date(it["folder"], it["frame_index"])
        return items


# ---------------------------------------------------------------------------------------------------------------- ground truth
_DETEC_SCAN_DIR = {"detec": "velodyne_points/data", "detec4beam": "4beam"}


def detec_output_name(split):
    """export_gt_depth.py:116-127 for the two detection splits."""
    if split not in _DETEC_SCAN_DIR:
        raise ValueError("detec_output_name: split must be 'detec' or 'detec4beam', got %r" % (split,))
    return "4beam.npz" if split == "detec4beam" else "gt_depths.npz"


def export_gt_depths_detec(data_path, lines, split, output_path=None, device="cuda"):
    """export_gt_depth.py:71-75 (``detec``: scans from ``velodyne_points/data``) and :81-85 (``detec4beam``: from ``4beam``): one
    ``generate_depth_map(calib_dir, scan, 2, True)`` per split line ``"<folder> <frame> <side>"``, float32, with the calibration
    folder chosen from the size of the line's ``image_02`` frame.  Saved like ``kitti_utils.export_gt_depths`` saves (an object array
    when the sizes differ).  Returns the list of maps."""
    from . import kitti_utils
    if split not in _DETEC_SCAN_DIR:
        raise ValueError("export_gt_depths_detec: split must be 'detec' or 'detec4beam', got %r" % (split,))
    gt_depths = []
    for line in lines:
        folder, frame_id, _ = line.split()
        frame_id = int(frame_id)
        date = detec_calib_date(*image_size(os.path.join(data_path, folder, "image_02/data/{:06d}.png".format(frame_id))))
        velo_filename = os.path.join(data_path, folder, _DETEC_SCAN_DIR[split], "{:06d}.bin".format(frame_id))
        gt_depths.append(kitti_utils.generate_depth_map(os.path.join(data_path, date), velo_filename, 2, True, device=device).astype(np.float32))
    if output_path is not None:
        same = all(g.shape == gt_depths[0].shape for g in gt_depths)
        data = np.array(gt_depths) if same else np.array(gt_depths, dtype=object)       # the dates differ in image size
        np.savez_compressed(output_path, data=data)
    return gt_depths


# ---------------------------------------------------------------------------------------------------------------- the exporter
def pack_export_sizes(sizes):
    """N ``(H, W)`` pairs -> (``EXPORT_DESC`` array: the maps back to back, map i computed from prediction i; total elements)."""
    desc = np.zeros(len(sizes), dtype=EXPORT_DESC)
    at = 0
    for i, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError("depth_export: size %d is %d x %d, expected positive" % (i, H, W))
        desc[i] = (at, H, W, i, 0)
        at += H * W
    return desc, at


def depth_export(pred_disps, sizes, ratios=None, pred_depth_scale_factor=1.0, want_depth=False, chunk=64, want_packed=False,
                 want_device=False):
    """export_detection.py:322-325, 344-348, 388 for N images, ``chunk`` of them per ``fd_depth_export`` call: the disparity resized to
    ``sizes[i] = (H_i, W_i)`` by OpenCV's float32 INTER_LINEAR rule, ``1 / .``, ``* pred_depth_scale_factor``, ``* ratios[i]`` (when
    given), ``* 256`` and the cast to ``uint16`` - each step one float32 rounding, the cast as the module docstring defines it.
    ``pred_disps``: [N,h,w] device tensor or host array (float64 is rounded to float32 once, as ``eigen_scores`` does).
    Returns a list of N ``uint16`` [H_i,W_i] arrays, views into one pinned download per chunk; with ``want_depth`` also the float32
    maps before the ``* 256`` (what the scorer clamps and scores) as device tensors: ``(u16 list, depth list)``.  ``want_packed``
    (with ``want_depth``) adds a third element: per chunk, ``(packed float32 device tensor, EXPORT_DESC array)`` - what the depth list
    is made of views of, in the form ``points_export(packed=...)`` takes without another launch or copy.  ``want_device``: the uint16
    maps stay on the device - N ``torch.uint16`` [H_i,W_i] tensors, views into one buffer per chunk, and no download - for
    ``image_codecs.encode_png_batch``."""
    if want_packed and not want_depth:
        raise ValueError("depth_export: want_packed needs want_depth")
    if not torch.cuda.is_available():
        raise RuntimeError("fusiondepth_amd.detection.depth_export needs an MI355X: there is no CPU path (tests/detection_ref.py restates it)")
    from . import functional as FD
    N = len(sizes)
    if len(pred_disps) != N:
        raise ValueError("depth_export: %d predictions for %d sizes" % (len(pred_disps), N))
    if chunk < 1 or chunk > 4096:
        raise ValueError("depth_export: chunk must be 1 .. 4096")
    if ratios is not None:
        ratios = np.ascontiguousarray(np.asarray(ratios, dtype=np.float32).reshape(-1))
        if ratios.size != N:
            raise ValueError("depth_export: %d ratios for %d maps" % (ratios.size, N))
    maps, depths, packs = [], [], []
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        disp = pred_disps[a:b]
        disp = disp if torch.is_tensor(disp) else torch.as_tensor(np.asarray(disp))
        disp = FD.f32(disp).cuda()
        if disp.dim() != 3:
            raise ValueError("depth_export: pred_disps must be [N,h,w], got %s" % (tuple(disp.shape),))
        dev = disp.device
        desc, total = pack_export_sizes(sizes[a:b])
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        ratio_d = None if ratios is None else torch.from_numpy(ratios[a:b].copy()).to(dev)
        out = torch.empty((total,), device=dev, dtype=torch.int16)          # the bits of uint16
        depth = torch.empty((total,), device=dev, dtype=torch.float32) if want_depth else None
        _lib.call("fd_depth_export", disp.data_ptr(), disp.shape[0], disp.shape[1], disp.shape[2], desc_d.data_ptr(), b - a, total,
                  int(desc["H"].max()), int(desc["W"].max()), float(pred_depth_scale_factor),
                  None if ratio_d is None else ratio_d.data_ptr(), None if depth is None else depth.data_ptr(), out.data_ptr(), _lib.stream())
        if want_device:                                          # desc_d and ratio_d go back to the allocator in stream order
            flat = out.view(torch.uint16)
        else:
            host = torch.empty((total,), dtype=torch.int16, pin_memory=True)
            host.copy_(out)                                      # synchronises: desc_d and ratio_d are free to go afterwards
            flat = host.numpy().view(np.uint16)                  # keeps the pinned tensor alive
        for d in desc:
            o, n = int(d["offset"]), int(d["H"]) * int(d["W"])
            maps.append(flat[o:o + n].reshape(int(d["H"]), int(d["W"])))
            if want_depth:
                depths.append(depth[o:o + n].view(int(d["H"]), int(d["W"])))
        if want_packed:
            packs.append((depth, desc))
    if want_packed:
        return maps, depths, packs
    return (maps, depths) if want_depth else maps


# ---------------------------------------------------------------------------------------------------------------- pseudo-LiDAR
# numpy mirror of ``fd_points_calib`` (144 bytes, as ``_lib.PointsCalib``): c_u, c_v, f_u, f_v, b_x, b_y, A[9], t[3]
POINTS_CALIB_DOUBLES = 18
assert POINTS_CALIB_DOUBLES * 8 == ctypes.sizeof(_lib.PointsCalib)
_POINTS_STAGE = [None]                                           # the pinned staging buffer, reused across chunks and calls
_POINTS_LOCK = threading.Lock()                                  # one chunk at a time owns it, from its download to its copy-out
_COPY_POOL = [None]                                              # host threads that copy the clouds out of it
_COPY_POOL_MIN_POINTS = 1 << 18                                  # 4 MiB of points: below it one thread is as quick


def _copy_pool():
    if _COPY_POOL[0] is None:
        import concurrent.futures
        _COPY_POOL[0] = concurrent.futures.ThreadPoolExecutor(max_workers=min(8, max(1, os.cpu_count() or 1)),
                                                              thread_name_prefix="fd_points_copy")
    return _COPY_POOL[0]


def points_calib_row(calibration, A, t):
    """One ``fd_points_calib`` as 18 float64: ``kitti_utils.Calibration``'s camera-2 scalars, then ``rect_to_velo``'s A and t."""
    A, t = np.asarray(A, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if A.shape != (3, 3) or t.shape != (3,):
        raise ValueError("points_export: A must be [3,3] and t [3], got %s and %s" % (A.shape, t.shape))
    c = calibration
    return np.concatenate([np.array([c.c_u, c.c_v, c.f_u, c.f_v, c.b_x, c.b_y], dtype=np.float64), A.reshape(9), t])


def _stage(floats):
    """A pinned float32 buffer of at least ``floats`` elements; grown by doubling, kept for the next chunk."""
    cur = _POINTS_STAGE[0]
    if cur is None or cur.numel() < floats:
        cur = torch.empty((max(floats, 2 * (cur.numel() if cur is not None else 0), 1 << 16),), dtype=torch.float32, pin_memory=True)
        _POINTS_STAGE[0] = cur
    return cur


def _points_chunk(depth, desc, calibs, max_high):
    """One ``fd_points_export`` call on a packed float32 device tensor: one table upload (descriptors and calibrations in one buffer),
    the call, the read-back of ``starts``, one pinned download of exactly 16 bytes per kept point."""
    n = len(desc)
    total_px = int(depth.numel())
    dev = depth.device
    table = np.concatenate([np.ascontiguousarray(desc).view(np.uint8).reshape(-1),
                            np.stack([points_calib_row(*c) for c in calibs]).view(np.uint8).reshape(-1)])
    table_d = torch.from_numpy(table).to(dev)                    # 24 n bytes of descriptors, then 144 n of calibrations: both 8-aligned
    max_H, max_W = int(desc["H"].max()), int(desc["W"].max())
    ws_bytes = _lib.query("fd_points_export_ws_bytes", n, max_H)
    if ws_bytes <= 0:
        raise ValueError("points_export: %d maps of up to %d rows are out of range" % (n, max_H))
    ws = torch.empty((ws_bytes,), device=dev, dtype=torch.uint8)
    points = torch.empty((4 * total_px,), device=dev, dtype=torch.float32)
    starts = torch.empty((n + 1,), device=dev, dtype=torch.int64)
    _lib.call("fd_points_export", depth.data_ptr(), table_d.data_ptr(), table_d.data_ptr() + desc.nbytes, n, total_px, max_H, max_W,
              float(max_high), ws.data_ptr(), points.data_ptr(), starts.data_ptr(), _lib.stream())
    starts_h = starts.cpu().numpy()                              # synchronises: table_d and ws are free to go afterwards
    total = int(starts_h[-1])
    if total > total_px:
        raise ValueError("points_export: descriptors overlap (%d points for %d pixels)" % (total, total_px))
    if not total:
        return [np.empty((0, 4), dtype=np.float32) for _ in range(n)]
    with _POINTS_LOCK:                                           # two threads in points_export take turns at the staging buffer
        stage = _stage(4 * total)[:4 * total]
        stage.copy_(points[:4 * total])                          # 16 * total bytes, nothing more
        staged = stage.numpy().reshape(total, 4)
        views = [staged[int(starts_h[i]):int(starts_h[i + 1])] for i in range(n)]
        # out of the staging buffer, which the next chunk reuses: a copy per cloud - for more than a few MB on host threads (numpy
        # releases the GIL in a copy; on one thread this copy, not the download, is what a chunk of 16 KITTI-sized maps waits for)
        if n == 1 or total < _COPY_POOL_MIN_POINTS:
            return [v.copy() for v in views]
        return list(_copy_pool().map(np.copy, views))


def points_export(depth_maps, calibs, max_high=1.0, chunk=16, packed=None):
    """Pseudo-LiDAR clouds by the point rule of the module docstring (``fd_points_export``).  ``depth_maps``: a list of 2-D float32
    device tensors of different sizes, such as the maps ``depth_export(want_depth=True)`` returns; ``calibs``: one
    ``(kitti_utils.Calibration, A, t)`` per map, ``(A, t) = kitti_utils.rect_to_velo(...)``.  Returns a list of float32 ``[M_i, 4]`` host
    arrays (x, y, z, 1): the layout of a KITTI ``.bin``.  ``chunk`` maps share one library call.
    ``packed=(tensor, EXPORT_DESC array)`` instead of ``depth_maps`` (pass ``None``): the maps already lie packed on the device, as one
    element of ``depth_export(want_depth=True, want_packed=True)[2]`` - one call for all of them, no per-image launch or copy.
    The pinned staging buffer and the copy threads are module state (``_POINTS_STAGE``, ``_COPY_POOL``: idle worker threads that the
    interpreter joins at exit); a lock serialises the download and copy-out of concurrent callers, everything else may overlap."""
    if not torch.cuda.is_available():
        raise RuntimeError("fusiondepth_amd.detection.points_export needs an MI355X GPU: there is no CPU path "
                           "(tests/pseudo_lidar_ref.py restates it)")
    if chunk < 1 or chunk > 4096:
        raise ValueError("points_export: chunk must be 1 .. 4096")
    if packed is not None:
        if depth_maps is not None:
            raise ValueError("points_export: give depth_maps or packed, not both")
        depth, desc = packed
        if not (torch.is_tensor(depth) and depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 1 and depth.is_contiguous()):
            raise ValueError("points_export: packed[0] must be a contiguous 1-D float32 device tensor")
        if len(desc) != len(calibs):
            raise ValueError("points_export: %d calibrations for %d maps" % (len(calibs), len(desc)))
        return _points_chunk(depth, desc, calibs, max_high) if len(desc) else []
    N = len(depth_maps)
    if len(calibs) != N:
        raise ValueError("points_export: %d calibrations for %d maps" % (len(calibs), N))
    clouds = []
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        part = depth_maps[a:b]
        for i, m in enumerate(part):
            if not (torch.is_tensor(m) and m.is_cuda and m.dtype == torch.float32 and m.dim() == 2):
                raise ValueError("points_export: map %d must be a 2-D float32 device tensor" % (a + i))
        desc, _ = pack_export_sizes([tuple(m.shape) for m in part])
        depth = part[0].reshape(-1).contiguous() if b - a == 1 else torch.cat([m.reshape(-1) for m in part])
        clouds += _points_chunk(depth, desc, calibs[a:b], max_high)
    return clouds


def quantize_u16(depth, want_device=False):
    """``(depth * 256.0).astype(np.uint16)`` of export_detection.py:388 for one dense device map (the one GDC returns), with the
    product in float64 as numpy computes it for the reference's float64 map and the out-of-range rule of the module docstring
    (``fd_depth_quantize_u16``) -> ``uint16`` host array of the same shape; with ``want_device`` a ``torch.uint16`` device tensor and
    no download."""
    _lib._need_cuda(depth)
    x = depth.detach().to(torch.float64).contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=torch.int16)
    if x.numel():
        _lib.call("fd_depth_quantize_u16", x.data_ptr(), out.data_ptr(), x.numel(), _lib.stream())
    if want_device:
        return out.view(torch.uint16)
    return out.cpu().numpy().view(np.uint16)
