"""The trainer's image summaries on the device (trainer.py:656-681): for the first J items of a batch one uint8 RGB contact sheet per
item - the input colours per frame and scale, the warped colour predictions of scale 0, the normalised disparities and the automask
(or the predictive masks) - rendered by ONE ``fd_log_sheets`` call (csrc/log_images.hip: two launches and a memset whatever J, the
scales and the frames are) and brought back by one pinned download.

  * ``layout(...)``   on the host: the sheet's size and the tag and ``(y, x, h, w, channels)`` of every tile.  The tags are the
    reference's strings with the item index: ``"color_-1_0/2"``, ``"color_pred_s_0/0"``, ``"disp_3/1"``, ``"automask_0/0"``.
  * ``render(...)``   -> the downloaded sheets ``[J, Hs, Ws, 3]`` and ``{tag: numpy view into its sheet}``.  No CPU fallback: it needs
    the GPU (tests/log_images_ref.py restates everything but the warp in numpy).
  * ``write_png`` / ``PngSink``   the default ``Trainer.image_sink``: ``<log_path>/<mode>/images/{step:07d}_{j}.png``, one sheet per
    item, encoded with PIL on one background thread.

The sheet.  One row block per scale ``s``, in the order of ``scales``; inside a block the tiles stand side by side with their top edges
on the block's, no gaps, no resizing, in this order:
    ``color_{f}_{s}`` for every frame id ``f``; at ``s == 0`` ``color_pred_{f}_0`` for every ``f != 0``; ``disp_{s}``; then
    ``automask_{s}``, or ``predictive_mask_{f}_{s}`` per source frame with ``predictive_mask`` - neither with automasking off alone, and
    neither for a validation event (trainer.py:671-681).
``Ws`` is the widest block, ``Hs`` the sum of the block heights, bytes outside every tile are 0, a single-channel tile fills the three
channels alike.  A tile has the size of the tensor the reference hands to ``add_image``: ``h_s x w_s`` for the colours, the disparity
and the predictive masks.  THE AUTOMASK IS THE EXCEPTION: the loss forms the reprojection minimum at full resolution for every scale
(trainer.py:434-435 upsamples the disparity first), so ``identity_selection/{s}`` has the size of scale 0 unless ``--v1_multiscale``;
that tile is drawn at its own size and its block is as tall as it (``mask_size``).  With ``--v1_multiscale``, with predictive masks,
with automasking off and for validation events every block has its scale's height ``h_s``.

What is pinned and what is not
  * ``normalize_image`` (``ma``, ``mi`` the tile's float32 maximum and minimum, ``d = float32(float64(ma) - float64(mi))``, ``1e5`` where
    they are equal, ``(x - mi) / d`` with an IEEE division) equals the reference's torch expression bit for bit
    (tests/test_log_images_cpu.py holds the restatement against torch, tests/test_gpu_log_images.py the kernels against the restatement).
  * THE QUANTISATION IS A SPECIFICATION, NOT A PINNED RESULT.  Every float becomes a byte by ``trunc(min(max(x * 255, 0), 255))`` in
    float32, NaN becomes 0 - the rule ``torch.utils.tensorboard.summary.image`` applies to float input.  tensorboard is not available
    to this project's build and tests, so the rule cannot be held against it; this text is the specification.
  * the colour predictions restate the loss kernels' warp (csrc/photometric.hip: ``project`` / ``gather3``) and are held to
    ``FD.photo_loss(..., materialize=True)`` within one level per byte.

Plugging in tensorboard or wandb: ``Trainer.image_sink`` is any callable ``(mode, step, sheets, tiles)``; with a
``torch.utils.tensorboard.SummaryWriter`` per mode it is ``for tag, tile in tiles.items(): writers[mode].add_image(tag, tile, step,
dataformats="HWC")``.  Neither package is imported here.
"""
import collections
import ctypes
import os
import queue
import threading

import numpy as np
import torch

from . import _lib

MAX_ITEMS = 64                                                    # fd_log_sheets' limits
MAX_TILES = 64
MAX_ROWS = 8
PROJECT_EPS = 1e-7                                                # loss_ops.PROJECT_EPS: Project3D's eps
KIND_COLOR, KIND_PRED, KIND_DISP, KIND_AUTOMASK, KIND_MASK = range(5)

Tile = collections.namedtuple("Tile", "tag item y x h w channels kind frame scale")
Layout = collections.namedtuple("Layout", "Hs Ws tiles rows")    # rows: (y, height, first tile of an item, tile count) per scale


def layout(frame_ids, scales, height, width, J=1, automask=True, predictive_mask=False, val=False, mask_size=None):
    """The contact sheet of one log event (module docstring) -> ``Layout(Hs, Ws, tiles, rows)``.  ``tiles``: for every item ``j < J``
    and every tile, ``Tile(tag, item, y, x, h, w, channels, kind, frame, scale)`` - ``(y, x, h, w)`` inside sheet ``item``,
    ``channels`` 3 or 1 (what the reference hands to ``add_image``; the sheet holds three either way).  ``height`` / ``width``: the
    size of scale 0; scale ``s`` is ``height // 2 ** s`` by ``width // 2 ** s``.  ``val``: a validation event - pass ``frame_ids=[0]``
    as the reference does; the mask tiles are left out.  ``mask_size``: the size of the automask planes (default: scale 0's, as the
    loss leaves them; ``"scale"`` for ``--v1_multiscale``, where they have their scale's size)."""
    frame_ids, scales = list(frame_ids), list(scales)
    if not frame_ids or not scales or len(scales) > MAX_ROWS:
        raise ValueError("layout: needs at least one frame id and 1 .. %d scales" % MAX_ROWS)
    if J < 1:
        raise ValueError("layout: J must be at least 1, got %d" % J)
    rows, per_item, y = [], [], 0
    for s in scales:
        h, w = int(height) // (2 ** s), int(width) // (2 ** s)
        if h < 1 or w < 1:
            raise ValueError("layout: scale %d of a %d x %d image is empty" % (s, height, width))
        row = [("color_{}_{}".format(f, s), h, w, 3, KIND_COLOR, f) for f in frame_ids]
        if s == 0:
            row += [("color_pred_{}_{}".format(f, s), h, w, 3, KIND_PRED, f) for f in frame_ids if f != 0]
        row.append(("disp_{}".format(s), h, w, 1, KIND_DISP, None))
        if predictive_mask:
            if not val:
                row += [("predictive_mask_{}_{}".format(f, s), h, w, 1, KIND_MASK, f) for f in frame_ids[1:]]
        elif automask and not val:
            mh, mw = (h, w) if mask_size == "scale" else ((int(height), int(width)) if mask_size is None else mask_size)
            row.append(("automask_{}".format(s), int(mh), int(mw), 1, KIND_AUTOMASK, None))
        x, block = 0, max(t[1] for t in row)
        rows.append((y, block, len(per_item), len(row)))
        for tag, th, tw, ch, kind, f in row:
            per_item.append((tag, y, x, th, tw, ch, kind, f, s))
            x += tw
        y += block
    Ws = max(t[2] + t[4] for t in per_item)
    tiles = [Tile("%s/%d" % (tag, j), j, ty, tx, th, tw, ch, kind, f, s) for j in range(J) for tag, ty, tx, th, tw, ch, kind, f, s in per_item]
    return Layout(y, Ws, tiles, rows)


_PLANS = {}                                                       # configuration -> (Layout, LogCfg, the tile table with its geometry filled in)


def _plan(key, min_depth, max_depth):
    """The layout, the ``fd_log_cfg`` and the geometry half of the tile table: built once per distinct configuration."""
    plan = _PLANS.get(key + (min_depth, max_depth))
    if plan is not None:
        return plan
    frame_ids, scales, height, width, J, automask, predictive_mask, val, mask_size = key
    lay = layout(frame_ids, scales, height, width, J, automask, predictive_mask, val, mask_size)
    NT = len(lay.tiles) // J
    if NT > MAX_TILES:
        raise ValueError("render: %d tiles per item, fd_log_sheets takes %d" % (NT, MAX_TILES))
    cfg = _lib.LogCfg()
    cfg.Hs, cfg.Ws, cfg.n_rows = lay.Hs, lay.Ws, len(lay.rows)
    for r, (y, h, first, count) in enumerate(lay.rows):
        cfg.row_y[r], cfg.row_h[r], cfg.row_first[r], cfg.row_count[r] = y, h, first, count
    cfg.lo, cfg.span, cfg.eps = 1.0 / max_depth, 1.0 / min_depth - 1.0 / max_depth, PROJECT_EPS
    table = (_lib.LogTile * (J * NT))()
    n_disp = 0
    for i, t in enumerate(lay.tiles):
        e = table[i]
        e.kind, e.y, e.x, e.h, e.w = t.kind, t.y, t.x, t.h, t.w
        if t.kind == KIND_DISP:
            e.slot = sum(1 for u in lay.tiles[t.item * NT:i] if u.kind == KIND_DISP)
            if t.item == 0:
                cfg.disp_tile[e.slot] = i
                n_disp += 1
    cfg.n_disp = n_disp
    plan = (lay, cfg, table, NT)
    _PLANS[key + (min_depth, max_depth)] = plan
    return plan


def _plane(t, shape, what, dtype=torch.float32):
    """A contiguous device tensor of ``dtype`` whose trailing dimensions are ``shape``; a ValueError names what is wrong."""
    if not torch.is_tensor(t):
        raise ValueError("render: %s is not a tensor" % what)
    if tuple(t.shape[1:]) != tuple(shape):
        raise ValueError("render: %s has shape %s, expected [B, %s]" % (what, tuple(t.shape), ", ".join(str(v) for v in shape)))
    if not t.is_cuda:
        raise ValueError("render: %s lives on %s; the renderer runs on the GPU only" % (what, t.device))
    t = t.detach()
    if dtype == torch.float32:
        return _lib.f32(t)
    if t.dtype != dtype:
        raise ValueError("render: %s must be %s, got %s" % (what, dtype, t.dtype))
    return t.contiguous()


def render(inputs, outputs, frame_ids, scales, J, Ts=None, first=0, automask=True, predictive_mask=False, val=False, min_depth=0.1,
           max_depth=100.0, v1_multiscale=False, want_stats=False, encode=False):
    """trainer.py:656-681 for the items ``first .. first + J - 1`` of a batch: one ``fd_log_sheets`` call, one pinned download.
    ``inputs`` / ``outputs``: the reference's dicts on the device - ``("color", f, s)`` [B,3,h_s,w_s] for every frame id and scale,
    ``("K", 0)`` / ``("inv_K", 0)`` [B,4,4], ``("disp", s)`` [B,1,h_s,w_s], ``("sel", s)`` (the pair the loss leaves: the uint8 argmin
    index [B,H,W] and the number of identity losses) for the automask, ``outputs["predictive_mask"][("disp", s)]`` [B,NF,h_s,w_s].
    ``Ts``: ``{f: T}`` for every source frame ``f != 0``, ``T`` [B,4,4] (or [1,4,4], shared by the items): ``("cam_T_cam", 0, f)``,
    ``stereo_T`` for ``"s"``, or the matrix ``Trainer.generate_images_pred`` forms for scale 0 with ``--pose_model_type posecnn``.
    ``val``: a validation event (``frame_ids=[0]``, no mask tiles).  Nothing is launched before every key, shape and ``J`` has been
    checked: a missing key, a mismatched size or ``J < 1`` is a ValueError.
    Returns ``(sheets, tiles)``: the uint8 array [J,Hs,Ws,3] (a view of the pinned download) and ``{tag: view into its sheet}``, [h,w,3]
    each; with ``want_stats`` also ``{disparity tag: (mi, ma)}`` as float32, the minimum and maximum the call used (NaN, NaN where
    the tile holds a NaN).  ``encode`` (not with ``want_stats``): the sheets are encoded on the device
    (``image_codecs.encode_png_batch``) and what comes down is their PNG files - ``(files, None)``, one ``memoryview`` per sheet into one
    pinned buffer, each decoding to the sheet the call without ``encode`` returns."""
    if encode and want_stats:
        raise ValueError("render: encode and want_stats cannot be combined")
    if not torch.cuda.is_available():
        raise RuntimeError("fusiondepth_amd.log_images.render needs an MI355X: there is no CPU path (tests/log_images_ref.py restates it)")
    frame_ids, scales, J, first = list(frame_ids), list(scales), int(J), int(first)
    if J < 1 or J > MAX_ITEMS:
        raise ValueError("render: J must be 1 .. %d, got %d" % (MAX_ITEMS, J))
    Ts = Ts or {}

    def need(d, key, name):
        if not hasattr(d, "get") or d.get(key) is None:
            raise ValueError("render: %s[%r] is missing" % (name, key))
        return d.get(key)

    color0 = need(inputs, ("color", frame_ids[0], scales[0]), "inputs")
    if not torch.is_tensor(color0) or color0.dim() != 4:
        raise ValueError("render: inputs[%r] must be [B,3,h,w]" % (("color", frame_ids[0], scales[0]),))
    B = color0.shape[0]
    height, width = color0.shape[2] * 2 ** scales[0], color0.shape[3] * 2 ** scales[0]
    if first < 0 or first + J > B:
        raise ValueError("render: items %d .. %d of a batch of %d" % (first, first + J - 1, B))
    draw_auto = automask and not predictive_mask and not val
    mask_size = None
    if draw_auto:
        pair = need(outputs, ("sel", scales[0]), "outputs")
        mask_size = "scale" if v1_multiscale else tuple(pair[0].shape[1:])
    key = (tuple(frame_ids), tuple(scales), height, width, J, bool(automask), bool(predictive_mask), bool(val), mask_size)
    lay, cfg, template, NT = _plan(key, float(min_depth), float(max_depth))

    # ---- every source, checked, before anything is launched
    keep, src = [], {}                                            # the tensors the call reads stay alive until the download has synchronised
    def batch_of(t, what):
        if t.shape[0] != B:
            raise ValueError("render: %s holds %d items, the batch has %d" % (what, t.shape[0], B))
        keep.append(t)
        return t
    item0 = lay.tiles[:NT]
    for t in item0:
        if t.kind in (KIND_COLOR, KIND_PRED):
            k = ("color", t.frame, t.scale)
            c = batch_of(_plane(need(inputs, k, "inputs"), (3, t.h, t.w), "inputs[%r]" % (k,)), "inputs[%r]" % (k,))
            src[t.tag] = (c, 3 * t.h * t.w * 4)
        if t.kind == KIND_PRED:
            h0, w0 = t.h, t.w
            d = batch_of(_plane(need(outputs, ("disp", 0), "outputs"), (1, h0, w0), "outputs[('disp', 0)]"), "outputs[('disp', 0)]")
            K = batch_of(_plane(need(inputs, ("K", 0), "inputs"), (4, 4), "inputs[('K', 0)]"), "inputs[('K', 0)]")
            iK = batch_of(_plane(need(inputs, ("inv_K", 0), "inputs"), (4, 4), "inputs[('inv_K', 0)]"), "inputs[('inv_K', 0)]")
            T = _plane(need(Ts, t.frame, "Ts"), (4, 4), "Ts[%r]" % (t.frame,))
            if T.shape[0] not in (1, B):
                raise ValueError("render: Ts[%r] holds %d matrices, the batch has %d" % (t.frame, T.shape[0], B))
            if h0 < 2 or w0 < 2:
                raise ValueError("render: a colour prediction needs at least 2 x 2 pixels")
            keep.append(T)
            src[t.tag] += (d, h0 * w0 * 4, K, iK, T, 64 if T.shape[0] == B else 0)
        elif t.kind == KIND_DISP:
            k = ("disp", t.scale)
            d = batch_of(_plane(need(outputs, k, "outputs"), (1, t.h, t.w), "outputs[%r]" % (k,)), "outputs[%r]" % (k,))
            src[t.tag] = (d, t.h * t.w * 4)
        elif t.kind == KIND_AUTOMASK:
            k = ("sel", t.scale)
            pair = need(outputs, k, "outputs")
            sel = batch_of(_plane(pair[0], (t.h, t.w), "outputs[%r][0]" % (k,), torch.uint8), "outputs[%r][0]" % (k,))
            src[t.tag] = (sel, t.h * t.w, int(pair[1]))
        elif t.kind == KIND_MASK:
            masks = need(need(outputs, "predictive_mask", "outputs"), ("disp", t.scale), "outputs['predictive_mask']")
            nf = len(frame_ids) - 1
            m = batch_of(_plane(masks, (nf, t.h, t.w), "outputs['predictive_mask'][%r]" % (("disp", t.scale),)), "the predictive mask")
            src[t.tag] = (m, nf * t.h * t.w * 4, frame_ids[1:].index(t.frame) * t.h * t.w * 4)
    dev = color0.device
    for t in keep:
        if t.device != dev:
            raise ValueError("render: the tensors live on different devices (%s, %s)" % (dev, t.device))

    # ---- the tile table: the cached geometry, this call's pointers
    table = (_lib.LogTile * (J * NT))()
    ctypes.memmove(table, template, ctypes.sizeof(table))
    for j in range(J):
        b = first + j
        for i, t in enumerate(item0):
            e, s = table[j * NT + i], src[t.tag]
            if t.kind == KIND_MASK:
                e.p0 = s[0].data_ptr() + b * s[1] + s[2]
                continue
            e.p0 = s[0].data_ptr() + b * s[1]
            if t.kind == KIND_PRED:
                e.p1 = s[2].data_ptr() + b * s[3]
                e.p2, e.p3, e.p4 = s[4].data_ptr() + b * 64, s[5].data_ptr() + b * 64, s[6].data_ptr() + b * s[7]
            elif t.kind == KIND_AUTOMASK:
                e.aux = s[2]
    raw = np.frombuffer(table, dtype=np.uint8)
    table_d = torch.from_numpy(raw.copy()).to(dev)               # the one upload
    ws = torch.empty((max(_lib.query("fd_log_sheets_ws_bytes", J, cfg.n_disp), 16),), device=dev, dtype=torch.uint8)
    sheets = torch.empty((J, lay.Hs, lay.Ws, 3), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.call("fd_log_sheets", ctypes.addressof(table), table_d.data_ptr(), J, NT, ctypes.addressof(cfg), sheets.data_ptr(),
                  ws.data_ptr(), _lib.stream())
        if encode:                                               # the sheets leave the device as PNG files: no pixel download
            from . import image_codecs
            files, _ = image_codecs.encode_png_batch([sheets[j] for j in range(J)])
            return files, None
        host = torch.empty(sheets.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(sheets)                                       # the one download; synchronises, the sources are free to go afterwards
    arr = host.numpy()                                           # keeps the pinned tensor alive
    tiles = {t.tag: arr[t.item, t.y:t.y + t.h, t.x:t.x + t.w] for t in lay.tiles}
    if not want_stats:
        return arr, tiles
    words = ws.cpu().numpy().view(np.uint32)[:4 * J * cfg.n_disp].reshape(J, cfg.n_disp, 4) if cfg.n_disp else np.zeros((J, 0, 4), np.uint32)
    stats = {}
    for i, t in enumerate(lay.tiles):
        if t.kind == KIND_DISP:
            ma_key, mi_key, nan = (int(v) for v in words[t.item, table[i].slot][:3])
            mi, ma = _value_of_key(~mi_key & 0xffffffff), _value_of_key(ma_key)
            stats[t.tag] = (np.float32(np.nan), np.float32(np.nan)) if nan else (mi, ma)
    return arr, tiles, stats


def _value_of_key(k):
    """The float32 behind the order-preserving key of csrc/log_images.hip."""
    u = (k & 0x7fffffff) if k & 0x80000000 else (~k & 0xffffffff)
    return np.array([u], np.uint32).view(np.float32)[0]


# ------------------------------------------------------------------------------------------------ the default sink
def write_png(path, sheet):
    """One [H,W,3] uint8 sheet as a PNG (PIL), written under a temporary name and moved into place."""
    from PIL import Image
    sheet = np.ascontiguousarray(sheet)
    if sheet.dtype != np.uint8 or sheet.ndim != 3 or sheet.shape[2] != 3:
        raise ValueError("write_png: expected a [H,W,3] uint8 array, got %s %s" % (sheet.dtype, sheet.shape))
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        Image.fromarray(sheet, "RGB").save(fh, format="PNG")
    os.replace(tmp, path)


def write_file(path, data):
    """An already encoded PNG (``render(encode=True)``), written under the same temporary name and moved into place."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(data)
    os.replace(tmp, path)


class PngSink:
    """The default ``Trainer.image_sink``: ``sink(mode, step, sheets, tiles)`` writes ``<log_path>/<mode>/images/{step:07d}_{j}.png``,
    one sheet per item; a sheet that arrives as encoded bytes (``Trainer.png_encoder = "device"``) is written as it is.
    The encoding and writing run on ONE background thread, started with the first event after a ``join`` and gone after the next: ``join()`` waits until everything handed in is on disk and re-raises what the thread ran into; ``close`` is ``join``."""

    def __init__(self, log_path):
        self.log_path = log_path
        self._queue = queue.Queue()
        self._thread = None
        self._error = None

    @staticmethod
    def path(log_path, mode, step, item):
        return os.path.join(log_path, mode, "images", "%07d_%d.png" % (step, item))

    def __call__(self, mode, step, sheets, tiles=None):
        if self._thread is None:
            self._thread = threading.Thread(target=self._work, name="fd-log-images", daemon=True)
            self._thread.start()
        self._queue.put((mode, int(step), sheets))

    def _work(self):
        while True:
            job = self._queue.get()
            if job is None:
                return
            try:
                mode, step, sheets = job
                os.makedirs(os.path.join(self.log_path, mode, "images"), exist_ok=True)
                for j in range(len(sheets)):
                    write = write_file if isinstance(sheets[j], (bytes, bytearray, memoryview)) else write_png
                    write(self.path(self.log_path, mode, step, j), sheets[j])
            except Exception as e:                                # handed to the caller of join
                self._error = self._error or e

    def join(self):
        if self._thread is not None:
            self._queue.put(None)
            self._thread.join()
            self._thread = None
        err, self._error = self._error, None
        if err is not None:
            raise err

    close = join
