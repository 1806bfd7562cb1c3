"""The image codecs of the loaders and the exporters, host side: baseline JPEG and PNG frames decoded on the device, PNG and baseline
JPEG files written on it.  Each is Pillow's result byte for byte; the split between the host pool and the kernels is the one
include/fdhip.h describes.  No autograd, and nothing of ``functional``."""
import ctypes
import io
import threading

import numpy as np
import torch

from . import _lib
from ._lib import call, round16, stream

_HOST_POOL = []


def host_pool():
    """The 16-thread pool the codecs use when the caller brings none."""
    if not _HOST_POOL:
        import concurrent.futures
        _HOST_POOL.append(concurrent.futures.ThreadPoolExecutor(max_workers=16))
    return _HOST_POOL[0]


def _c_bytes(data):
    """A bytes-like object as a ctypes argument: ``bytes`` as it is, anything else copied once."""
    return data if isinstance(data, bytes) else (ctypes.c_ubyte * len(data)).from_buffer_copy(data)


def _pil_rgb(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img.convert("RGB"))


# ------------------------------------------------------------------------------------------ the decode job -------
def group_layout(sizes, elem, out_base=0):
    """Where the frames of a batch go in the output: ``sizes`` = [(h, w)] per frame, ``elem`` bytes per pixel -> (out_off per frame,
    {(h, w): first byte}, {(h, w): indices}, out bytes).  Same-size frames are contiguous, the groups in order of first appearance
    and 16-byte aligned from ``out_base`` on.  Pure: neither torch nor the GPU."""
    members = {}
    for i, (h, w) in enumerate(sizes):
        members.setdefault((h, w), []).append(i)
    out_off, at, spans = [0] * len(sizes), out_base, {}
    for (h, w), idx in members.items():
        spans[(h, w)] = at
        for i in idx:
            out_off[i] = at
            at += elem * h * w
        at = round16(at)
    return out_off, spans, members, max(at, 16)


def _in_input_order(groups, n):
    """The ``groups`` of ``BatchDecodeJob.finish`` -> one frame per file, in input order."""
    frames = [None] * n
    for stack, idx in groups.values():
        for k, i in enumerate(idx):
            frames[i] = stack[k]
    return frames


class BatchDecodeJob:
    """The host side of a batch decode, started on ``pool`` without blocking the caller: every file is read and probed; the worker
    that finishes the last probe lays out ONE pinned staging buffer (the descriptor table, then one slot per frame: what the device
    half reads or, for a frame Pillow decodes, its finished bytes) and submits the per-frame decoders, each writing straight into its
    slot with the interpreter lock released.  ``finish(device)`` waits, uploads the buffer once and makes the one library call.

    A subclass names its descriptor struct (``DESC``), its output bytes per pixel (``_elem``; 2 is a uint16 [H, W] frame, 3 a uint8
    [H, W, 3] one) and supplies ``_probe_one``, ``_slot_need``, ``_device_only``, ``_decode``, ``_fill`` and ``_launch``.  An entry
    of ``_probed`` is ``(data, info, pixels)``: the file's bytes, the probe's info of a frame the device half takes (else None), and
    what Pillow has decoded of it already (else None)."""
    NAME = DESC = None
    _elem = 3

    def __init__(self, files, pool=None):
        self.files = list(files)
        if not self.files:
            raise ValueError("%s: no files" % self.NAME)
        if len(self.files) > 65535:
            raise ValueError("%s: %d files in one call; the kernel takes 65535" % (self.NAME, len(self.files)))
        self.pool = pool if pool is not None else host_pool()
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
            self._probed[i] = (data,) + self._probe_one(data)
        except BaseException as e:                               # noqa: B902 - handed to finish()
            with self._lock:
                self._error = self._error or e
        with self._lock:
            self._left -= 1
            last = self._left == 0
        if last:
            self._plan()

    def _plan(self):
        try:
            if self._error is not None:
                return
            n = len(self.files)
            at = round16(n * ctypes.sizeof(self.DESC))
            self._slots, planes = [], 0
            for data, info, pixels in self._probed:
                h, w, need = self._slot_need(data, info, pixels)
                if info is not None:
                    planes += self._device_only(info)
                size = round16(max(need, self._elem * h * w))    # a frame whose host decoding fails gets Pillow's bytes instead
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

    # ---- caller side ------------------------------------------------------------------------------------------------------------
    def wait_host(self):
        """Block until the host phase (read, probe, Huffman decoding / inflate or Pillow) is done; raise what it raised.  Returns the
        layout: ``{"staging": the pinned uint8 buffer, "upload_bytes": its size, "plane_bytes": the device-only room behind it,
        "total_bytes": their sum}`` - the descriptor table at the start of the buffer is written by ``run``."""
        self._ready.wait()
        if self._error is not None:
            raise self._error
        for f in self._futures:
            f.result()
        return {"staging": self._staging, "upload_bytes": self._upload_bytes, "plane_bytes": self._plane_bytes,
                "total_bytes": self._upload_bytes + self._plane_bytes}

    def sizes(self):
        """[(h, w)] per file, once ``wait_host`` has returned."""
        return [(h, w) for _, _, h, w in self._slots]

    def descriptors(self):
        """A copy of the descriptor table ``run`` wrote at the head of the staging buffer (a ctypes array of ``DESC``)."""
        n = len(self.files)
        return (self.DESC * n).from_buffer_copy(self._host[:n * ctypes.sizeof(self.DESC)].tobytes())

    def layout(self, out_base=0):
        """-> (table, out_off per frame, {(h, w): first byte}, {(h, w): indices}, out bytes): ``group_layout`` of the batch and the
        descriptor table that goes with it."""
        out_off, spans, members, out_bytes = group_layout(self.sizes(), self._elem, out_base)
        table = (self.DESC * len(self.files))()
        plane_at = self._upload_bytes
        for i, (d, (slot, _, h, w)) in enumerate(zip(table, self._slots)):
            info = self._probed[i][1]
            d.kind, d.width, d.height, d.out_off = self._kinds[i], w, h, out_off[i]
            self._fill(d, slot, info, plane_at)
            if d.kind == 0:
                plane_at += self._device_only(info)
        return table, out_off, spans, members, out_bytes

    def run(self, device, out, table):
        """Upload the staging buffer (with ``table`` at its head) and make the one library call into ``out``, a uint8 device tensor."""
        n = len(self.files)
        self._host[:n * ctypes.sizeof(self.DESC)] = np.frombuffer(table, dtype=np.uint8)
        total = self._upload_bytes + self._plane_bytes
        dev = torch.empty((total,), dtype=torch.uint8, device=device)
        dev[:self._upload_bytes].copy_(self._staging, non_blocking=True)       # the batch's one host-to-device copy
        self._launch(dev, total, table, n, out)
        device_n = sum(1 for k in self._kinds if k == 0)
        return {"device": device_n, "fallback": n - device_n}

    def finish(self, device="cuda"):
        """-> (groups, stats): ``groups`` = {(H, W): (device tensor of the n frames of that size, input indices)} in order of first
        appearance, all views of one buffer; ``stats`` = {"device": n, "fallback": n}.  Runs on ``device``'s current stream,
        whichever device is current."""
        self.wait_host()
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("%s runs on the GPU only (got %s); there is no CPU path" % (self.NAME, device))
        with torch.cuda.device(device):
            table, _, spans, members, out_bytes = self.layout()
            out = torch.empty((out_bytes,), dtype=torch.uint8, device=device)
            stats = self.run(device, out, table)
        groups = {}
        for (h, w), idx in members.items():
            flat = out[spans[(h, w)]:spans[(h, w)] + len(idx) * self._elem * h * w]
            groups[(h, w)] = (flat.view(torch.uint16).view(len(idx), h, w) if self._elem == 2 else flat.view(len(idx), h, w, 3), idx)
        return groups, stats


# ------------------------------------------------------------------------------------ baseline JPEG frames -------
# Pillow's decode of a baseline JPEG, split as include/fdhip.h ("baseline JPEG frames") describes: Huffman decoding on a host pool
# behind the C ABI (ctypes releases the interpreter lock), everything after it in csrc/jpeg.hip.  tests/jpeg_ref.py restates it.
def jpeg_probe(data):
    """``fd_jpeg_probe`` of a bytes-like object -> (status, JpegInfo).  Host only."""
    info = _lib.JpegInfo()
    return _lib.load().fd_jpeg_probe(_c_bytes(data), len(data), ctypes.byref(info)), info


def jpeg_entropy_decode(data, coef, qt):
    """``fd_jpeg_entropy_decode`` into ``coef`` (a contiguous int16 numpy array; its size is ``coef_cap``) and ``qt`` (uint16, 192
    values) -> (status, JpegInfo).  Host only; the reason of a non-zero status is ``_lib.last_error()`` on the calling thread."""
    info = _lib.JpegInfo()
    st = _lib.load().fd_jpeg_entropy_decode(_c_bytes(data), len(data), coef.ctypes.data, coef.size, qt.ctypes.data, ctypes.byref(info))
    return st, info


class JpegBatchJob(BatchDecodeJob):
    """The host side of ``decode_jpeg_batch``: a covered frame's slot holds its quantisation tables (384 bytes) and its coefficients,
    written by the entropy decoder on the pool; its coefficient planes are device-only room behind the upload.  A frame that is
    not covered is decoded by Pillow in the probe."""
    NAME, DESC = "decode_jpeg_batch", _lib.JpegDesc

    def _probe_one(self, data):
        st, info = jpeg_probe(data)
        if st == 0 and info.covered:
            return info, None
        return None, _pil_rgb(data)                              # not covered, or not a JPEG at all: Pillow decides

    def _slot_need(self, data, info, rgb):
        if info is not None:
            return info.height, info.width, 384 + 2 * info.coef_count
        return rgb.shape[0], rgb.shape[1], 0

    def _device_only(self, info):
        return round16(info.coef_count)

    def _decode(self, i):
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

    def _fill(self, d, slot, info, plane_at):
        if d.kind == 0:
            d.qt_off, d.coef_off, d.plane_off = slot, slot + 384, plane_at
            d.components, d.h_samp, d.v_samp = info.components, info.h_samp, info.v_samp
        else:
            d.coef_off = slot

    def _launch(self, dev, total, table, n, out):                # the kernels read the table from the head of ``dev``
        call("fd_jpeg_reconstruct", dev.data_ptr(), total, dev.data_ptr(), n, out.data_ptr(), out.numel(), stream())


def decode_jpeg_batch(files, device="cuda", pool=None):
    """``np.asarray(Image.open(f).convert("RGB"))`` of every file, byte for byte, on the device.  ``files``: paths or ``bytes``.
    Returns ``(frames, stats)``: a list of uint8 [H, W, 3] device tensors - views into one buffer, same-size frames contiguous - and
    ``{"device": n, "fallback": n}``.  Covered baseline streams (include/fdhip.h) are Huffman-decoded on the host pool and finished
    by ``fd_jpeg_reconstruct``; everything else - progressive, CMYK, a PNG, a damaged stream - is decoded by Pillow into the same
    staging buffer and copied by the same call.  One host-to-device copy and one library call whatever the number of files."""
    groups, stats = JpegBatchJob(files, pool).finish(device)
    return _in_input_order(groups, len(files)), stats


# ------------------------------------------------------------------------------------------------ PNG frames -------
# Pillow's decode of a PNG, split as include/fdhip.h ("PNG frames") describes: the chunk walk and the inflate on a host pool behind
# the C ABI (ctypes releases the interpreter lock), the scanline filters in csrc/png.hip.  tests/png_ref.py restates it.
PNG_BAND_ROWS = 512          # FD_PNG_BAND_ROWS: the rows one workgroup of k_png_unfilter holds at a time
PNG_MODES = {"rgb": 0, "gray16": 1}


def png_probe(data):
    """``fd_png_probe`` of a bytes-like object -> (status, PngInfo).  Host only."""
    info = _lib.PngInfo()
    return _lib.load().fd_png_probe(_c_bytes(data), len(data), ctypes.byref(info)), info


def png_inflate(data, dst):
    """``fd_png_inflate`` into ``dst`` (a contiguous uint8 numpy array; its size is ``dst_cap``) -> (status, PngInfo).  Host only; the
    reason of a non-zero status is ``_lib.last_error()`` on the calling thread."""
    info = _lib.PngInfo()
    return _lib.load().fd_png_inflate(_c_bytes(data), len(data), dst.ctypes.data, dst.size, ctypes.byref(info)), info


def _pil_gray16(data, name="<bytes>"):
    """``np.asarray(Image.open(f))`` as uint16, with the completion loader's single-channel-integer check."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        a = np.asarray(img)
    if a.ndim != 2 or a.dtype.kind not in "ui":
        raise RuntimeError("decode_png_batch: %s decoded to %s %s, expected a single-channel integer depth map" % (name, a.dtype, a.shape))
    if a.size and (int(a.max()) > 65535 or int(a.min()) < 0):
        raise RuntimeError("decode_png_batch: %s holds values outside 16 bits" % name)
    return a.astype(np.uint16)


class PngBatchJob(BatchDecodeJob):
    """The host side of ``decode_png_batch``: a covered frame's slot holds its filtered scanlines, inflated on the pool; nothing is
    device-only.  A frame that is not covered only has its header read by the planner and is decoded by Pillow on the pool, straight
    into its slot.  ``mode``: ``"rgb"`` (8-bit RGB and grey files on the device, uint8 [H, W, 3] frames) or ``"gray16"`` (16-bit
    grey files on the device, uint16 [H, W] frames); every other file is Pillow's."""
    NAME, DESC = "decode_png_batch", _lib.PngDesc

    def __init__(self, files, pool=None, mode="rgb"):
        if mode not in PNG_MODES:
            raise ValueError("decode_png_batch: mode must be 'rgb' or 'gray16', got %r" % (mode,))
        self.mode = mode
        self._elem = 2 if mode == "gray16" else 3
        super().__init__(files, pool)

    def _probe_one(self, data):
        st, info = png_probe(data)
        if st == 0 and info.covered and (info.bpp == 2) == (self.mode == "gray16"):
            return info, None
        return None, None                                        # Pillow decodes it in _decode, straight into the buffer

    def _slot_need(self, data, info, _):
        if info is not None:
            return info.height, info.width, info.raw_bytes
        from PIL import Image
        with Image.open(io.BytesIO(data)) as img:                # the size from the header alone; Pillow raises for what it cannot open
            w, h = img.size
        return h, w, 0

    def _device_only(self, info):
        return 0

    def _decode(self, i):
        data, info, _ = self._probed[i]
        at, size, h, w = self._slots[i]
        if info is not None:
            st, _ = png_inflate(data, self._host[at:at + info.raw_bytes])
            if st == 0:
                self._kinds[i] = 0
                return
        name = self.files[i] if isinstance(self.files[i], str) else "<bytes %d>" % i
        px = _pil_gray16(data, name) if self.mode == "gray16" else _pil_rgb(data)     # not covered, or damaged: Pillow decides
        if px.shape[:2] != (h, w):
            raise RuntimeError("decode_png_batch: Pillow decoded %s, the header says %s" % (px.shape[:2], (h, w)))
        self._host[at:at + self._elem * h * w] = np.ascontiguousarray(px).reshape(-1).view(np.uint8)

    def _fill(self, d, slot, info, plane_at):
        d.raw_off, d.mode, d.bpp = slot, PNG_MODES[self.mode], info.bpp if d.kind == 0 else 0

    def _launch(self, dev, total, table, n, out):                # the library reads the table on the host
        call("fd_png_unfilter", dev.data_ptr(), total, ctypes.addressof(table), n, out.data_ptr(), out.numel(), stream())


def decode_png_batch(files, device="cuda", pool=None, mode="rgb"):
    """``np.asarray(Image.open(f).convert("RGB"))`` of every file (``mode="rgb"``: uint8 [H, W, 3]) or ``np.asarray(Image.open(f))`` of
    every 16-bit depth map (``mode="gray16"``: uint16 [H, W]), value for value, on the device.  ``files``: paths or ``bytes``.
    Returns ``(frames, stats)``: a list of device tensors - views into one buffer, same-size frames contiguous - and ``{"device": n,
    "fallback": n}``.  Covered files (include/fdhip.h: non-interlaced 8-bit RGB and 8-bit grey in ``rgb`` mode, 16-bit grey in
    ``gray16`` mode) are inflated on the host pool and unfiltered by ``fd_png_unfilter``; everything else - palette, alpha, tRNS,
    Adam7, other depths, a damaged file, a JPEG - is decoded by Pillow into the same staging buffer and copied by the same call.
    One host-to-device copy and one library call whatever the number of files."""
    groups, stats = PngBatchJob(files, pool, mode).finish(device)
    return _in_input_order(groups, len(files)), stats


# ------------------------------------------------------------------------------------- what the encoders share -------
_PNG_KINDS = ((3, 1, 2), "none of uint8 [H,W,3], uint8 [H,W], uint16 [H,W]")
_JPEG_KINDS = ((3, 1), "neither uint8 [H,W,3] nor uint8 [H,W]")


def _image_kind(x, i, kinds, who):
    """-> (height, width, bytes per pixel) of image ``i`` of an encoder's batch: 3 is uint8 [H, W, 3], 1 uint8 [H, W], 2 uint16
    [H, W].  ``kinds`` = (those ``who`` takes, how its message lists them); ValueError for anything else."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise ValueError("%s: image %d is a %s, not a tensor or an array" % (who, i, type(x).__name__))
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
        bpp = 0
    if bpp not in kinds[0]:
        raise ValueError("%s: image %d is %s %s, %s" % (who, i, dt, list(shape), kinds[1]))
    return shape[0], shape[1], bpp                               # their limits are the caller's to check


def _on_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _stage_images(images, table, who, device=None):
    """The sources of an encoder's batch -> (device, what keeps the sources alive); ``table[i].src`` gets image ``i``'s device
    address.  The device is ``device``, else the first device image's, else the current one; the host images are packed into one
    pinned buffer at 16-byte slots and uploaded in one copy; the device images are used where they are, made contiguous."""
    dev = [x.device for x in images if _on_device(x)]
    device = torch.device(device) if device is not None else (dev[0] if dev else torch.device("cuda", torch.cuda.current_device()))
    if device.type != "cuda":
        raise RuntimeError("%s runs on the GPU only (got %s); there is no CPU path" % (who, device))
    host = [(i, x.numpy() if isinstance(x, torch.Tensor) else x) for i, x in enumerate(images) if not _on_device(x)]
    keep = []
    with torch.cuda.device(device):
        if host:
            at, slots = 0, []
            for i, a in host:
                slots.append(at)
                at += round16(a.nbytes)
            pinned = torch.empty((at,), dtype=torch.uint8, pin_memory=True)
            flat = pinned.numpy()
            for (i, a), s in zip(host, slots):
                flat[s:s + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            up = torch.empty((at,), dtype=torch.uint8, device=device)
            up.copy_(pinned, non_blocking=True)
            keep += [pinned, up]
            for (i, _), s in zip(host, slots):
                table[i].src = up.data_ptr() + s
        for i, x in enumerate(images):
            if _on_device(x):
                if x.device != device:
                    raise ValueError("%s: image %d lives on %s, the batch on %s" % (who, i, x.device, device))
                x = x.contiguous()
                keep.append(x)
                table[i].src = x.data_ptr()
    return device, keep


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


class PngEncodeJob:
    """``encode_png_batch`` in its two halves, so that a caller can put work between them: the constructor checks the images, uploads
    the host ones in one copy and issues launch A and the download of its statistics; ``finish()`` waits for them, plans, issues
    launches B and C and the download of the files, waits, and fills the CRC-32s on ``pool``."""

    def __init__(self, images, pool=None, device=None):
        images = list(images)
        if not images:
            raise ValueError("encode_png_batch: no images")
        kinds = [_image_kind(x, i, _PNG_KINDS, "encode_png_batch") for i, x in enumerate(images)]
        self.pool = pool if pool is not None else host_pool()
        self.n = n = len(images)
        self.table, self.sizes = png_enc_layout([(w, h, bpp) for h, w, bpp in kinds])       # the sides' limits are the library's to check
        self.device, self._keep = _stage_images(images, self.table, "encode_png_batch", device)
        sz = self.sizes
        with torch.cuda.device(self.device):
            self.work = torch.empty((sz.work_bytes,), dtype=torch.uint8, device=self.device)
            call("fd_png_enc_filter", self.work.data_ptr(), sz.work_bytes, ctypes.addressof(self.table), n, stream())
            self._stats = torch.empty((sz.stat_bytes,), dtype=torch.uint8, pin_memory=True)
            self._stats.copy_(self.work[sz.stat_off:sz.stat_off + sz.stat_bytes], non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()

    def stats_words(self):
        """Launch A's statistics (histograms, then Adler pairs) as a uint32 numpy array, once their download has arrived."""
        self._event.synchronize()
        return self._stats.numpy().view(np.uint32)

    def finish(self):
        """-> (files, stats) of ``encode_png_batch``."""
        sz, n = self.sizes, self.n
        with torch.cuda.device(self.device):
            words = self.stats_words()
            blocks = torch.empty((sz.blocks * ctypes.sizeof(_lib.PngEncBlock),), dtype=torch.uint8, pin_memory=True)
            _, total = png_enc_plan(self.table, n, words, blocks.data_ptr())
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
    zz = np.zeros((2, 64), np.uint16)
    if _lib.load().fd_jpeg_enc_quant_tables(int(quality), zz.ctypes.data) != 0:
        raise ValueError(_lib.last_error())
    return zz


def jpeg_enc_header(width, height, sampling, quality, dst=None):
    """``fd_jpeg_enc_header`` -> the header bytes of a file (or written at the start of ``dst``, a contiguous uint8 numpy array).  Host only."""
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


def pil_jpeg(a, quality, sampling=None):
    """The file Pillow writes for a uint8 [H, W] (mode L) or [H, W, 3] array."""
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


def _jpeg_enc_check(images, quality, sampling):
    """-> (sampling name per image, indices of the colour images, indices of the grey ones); every ValueError of ``encode_jpeg_batch``."""
    if not images:
        raise ValueError("encode_jpeg_batch: no images")
    names = check_jpeg_params(quality, sampling, len(images))
    colour, grey = [], []
    for i, x in enumerate(images):
        h, w, bpp = _image_kind(x, i, _JPEG_KINDS, "encode_jpeg_batch")
        if not (1 <= h <= 65535 and 1 <= w <= 65535):
            raise ValueError("encode_jpeg_batch: image %d is %d x %d, a side outside 1 .. 65535" % (i, h, w))
        (colour if bpp == 3 else grey).append(i)
    on = [(i, images[i].device) for i in colour if _on_device(images[i])]
    for i, dv in on:                                             # one device per batch: the first device image's
        if dv != on[0][1]:
            raise ValueError("encode_jpeg_batch: image %d lives on %s, the batch on %s" % (i, dv, on[0][1]))
    return names, colour, grey


def _jpeg_enc_start_grey(images, grey, quality, pool):
    """Pillow's mode-L files of the grey images, started on ``pool`` -> {index: future}."""
    return {i: pool.submit(pil_jpeg, images[i].cpu().numpy() if isinstance(images[i], torch.Tensor) else np.ascontiguousarray(images[i]),
                           quality) for i in grey}


def _jpeg_enc_launch(images, names, quality):
    """Stage the colour ``images`` and make the one library call -> (device, table, sizes, work, out, what keeps the sources alive)."""
    table, sizes = jpeg_enc_layout([(x.shape[1], x.shape[0]) + JPEG_SAMPLINGS[s] for x, s in zip(images, names)])
    device, keep = _stage_images(images, table, "encode_jpeg_batch")
    with torch.cuda.device(device):
        work = torch.empty((sizes.work_bytes,), dtype=torch.uint8, device=device)
        out = torch.empty((sizes.out_bytes,), dtype=torch.uint8, device=device)
        call("fd_jpeg_enc_encode", work.data_ptr(), sizes.work_bytes, ctypes.addressof(table), len(images), quality, out.data_ptr(),
             sizes.out_bytes, stream())
    return device, table, sizes, work, out, keep


def _jpeg_enc_results(launched, n):
    """Download the library call's result rows and wait for them -> a ctypes array of ``_lib.JpegEncResult``."""
    device, _, sizes, work, _, _ = launched
    with torch.cuda.device(device):
        rows = torch.empty((sizes.result_bytes,), dtype=torch.uint8, pin_memory=True)
        rows.copy_(work[sizes.result_off:sizes.result_off + sizes.result_bytes], non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return (_lib.JpegEncResult * n).from_buffer_copy(rows.numpy().tobytes())


def _jpeg_enc_assemble(n, colour, grey, launched, results, grey_files, quality):
    """One pinned buffer of every file: the device's streams downloaded in one copy, their headers written in front of them, Pillow's
    grey files behind.  ``launched``: what ``_jpeg_enc_launch`` returned, None without a colour image -> (one ``memoryview`` per
    image, the buffer's size)."""
    device_bytes = sum(r.out_bytes for r in results) if colour else 0
    total = device_bytes + sum(len(f) for f in grey_files.values())
    pinned = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    flat = pinned.numpy()
    view, files, at = memoryview(flat), [None] * n, device_bytes
    if colour:
        device, table, sizes, _, out, _ = launched
        if results[len(colour) - 1].out_off + results[len(colour) - 1].out_bytes != device_bytes or device_bytes > sizes.out_bytes:
            raise RuntimeError("encode_jpeg_batch: the files' sizes do not add up")
        with torch.cuda.device(device):
            pinned[:device_bytes].copy_(out[:device_bytes], non_blocking=True)     # exactly the sum of the file sizes
            torch.cuda.current_stream().synchronize()
        for i, r, d in zip(colour, results, table):
            jpeg_enc_header(d.width, d.height, (d.hs, d.vs), quality, flat[r.out_off:r.out_off + JPEG_ENC_HEADER_BYTES])
            files[i] = view[r.out_off:r.out_off + r.out_bytes]
    for i in grey:
        data = grey_files[i]
        flat[at:at + len(data)] = np.frombuffer(data, np.uint8)
        files[i] = view[at:at + len(data)]
        at += len(data)
    return files, total


def encode_jpeg_batch(images, quality=92, sampling="2x2", pool=None):
    """The JPEG files Pillow writes for ``Image.fromarray(a).save(f, "JPEG", quality=quality, subsampling=...)``, byte for byte, of
    ``images`` - device tensors, or host tensors / numpy arrays (uploaded in one copy), uint8 [H, W, 3] of any mix of sizes.
    ``sampling``: '1x1', '2x1' or '2x2' (Pillow's subsampling 0, 1, 2), or a list with one per image.  Returns ``(files, stats)``: one
    ``memoryview`` per image into ONE pinned buffer, complete files ready to be written, and ``{"device": n, "fallback": n, "bytes":
    their total size}``.  A uint8 [H, W] image is outside the covered set: Pillow encodes it (mode L) into the same buffer and it is
    counted as ``fallback``.  One library call of seven launches whatever the number of images; any other dtype or rank, a zero or
    over-large side, a bad ``quality`` or ``sampling`` is a ValueError before the GPU is touched."""
    images = list(images)
    names, colour, grey = _jpeg_enc_check(images, quality, sampling)
    grey_jobs = _jpeg_enc_start_grey(images, grey, quality, pool if pool is not None else host_pool())
    launched = results = None
    if colour:
        launched = _jpeg_enc_launch([images[i] for i in colour], [names[i] for i in colour], quality)
        results = _jpeg_enc_results(launched, len(colour))
    grey_files = {i: f.result() for i, f in grey_jobs.items()}
    files, total = _jpeg_enc_assemble(len(images), colour, grey, launched, results, grey_files, quality)
    return files, {"device": len(colour), "fallback": len(grey), "bytes": int(total)}
