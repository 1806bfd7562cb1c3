"""KITTI raw training batches, built on the GPU: the reference's ``KITTIRAWDataset`` (datasets/mono_dataset.py:33-228,
datasets/kitti_dataset.py:28-117) plus the ``DataLoader`` around it (trainer.py:155-171), as one iterable that yields
collated batches on the device in the reference's schema.

    loader = KITTIRAWBatches(data_path, filenames, 192, 640, [0, -1, 1], 4, is_train=True, img_ext=".jpg", opt=opts,
                             batch_size=12, shuffle=True, seed=0)
    Trainer(opts).train(loader)

What runs where
  * host, on a thread pool of at most 16 workers: ``PIL.Image.open(path).convert("RGB")`` per frame and ``np.fromfile`` per
    LiDAR scan (PIL is imported here, lazily, and nowhere else in the package);
  * device: the frames are uploaded as uint8 and everything after the decoder runs in HIP kernels - the four-level Lanczos
    pyramid, colour jitter and ``ToTensor`` (``data_ops.image_pyramid``), the ``4beam`` rasterisation, the ``2channel`` scatter
    (computed online from the beam map: no ``.npy`` files are read) and ``depth_gt``.
  * the builder issues batch i + 1 on its own stream before it hands batch i to the consumer; the hand-over is an event the
    consumer's stream waits on (the pattern of ``refiner.prefetch_frozen``).  All device work is issued from the calling thread.

Colour jitter policy.  The reference's docstring (mono_dataset.py:88-90) promises that "the same augmentation" reaches all
images of an item.  That was true of its monodepth2 ancestor, which called ``ColorJitter.get_params(...)`` once per item and got
back one fixed transform (torchvision < 0.9; from 0.9 on ``get_params`` returns the raw draw instead).  The reference itself
builds a ``ColorJitter`` OBJECT per item (mono_dataset.py:178) and calls it on every frame and scale, and in the torchvision
sources known to us (0.9 and later) ``ColorJitter.forward`` draws the order and the four factors afresh on every call - so
there every image gets its own draw.  Default here: what the docstring promises, ONE draw per item shared by all of its frames
and scales; ``jitter_per_image=True`` gives one draw per (frame, scale), the behaviour of the object under torchvision >= 0.9.
torchvision is not installed where this package is built, so both statements are second-hand (read from its published source),
like the ResNet trunk's layout.

Deviation from the reference, on purpose: it rasterises ``4beam`` at the fixed ``[384, 1280]`` (a ``[192, 640]`` map) whatever
``height`` / ``width`` are, and its ``2channel`` files are made for that size.  Here the map is rasterised at ``[2 height, 2 width]``
and scattered with the ROI scaled to match - identical at the reference's 192x640, and usable by the trainer at other sizes, where
the reference's fixed-size map does not fit the network's input.  As in the reference, ``("2channel", f, 0)`` exists whenever
``need_2_channel`` is set; ``"4beam"`` and ``"2channel"`` only with ``need_4beam``.

LiDAR source.  ``lidar_source="files"`` (the default) reads the ``{n}beam/`` / ``random{N}/`` scans an offline sparsifier wrote
(the reference's ``sparsify/sparsify.py`` or ``python -m fusiondepth_amd.sparsify``).  ``lidar_source="raw"`` needs none of them: it reads
``velodyne_points/data/*.bin`` and sparsifies on the device.  That path is batched from the start - whatever the batch size, the LiDAR
keys of a batch cost ONE host-to-device copy (the worker threads read the files straight into one pinned staging buffer that also
carries the offsets, the random keys and the cameras) and four library calls: ``fd_sparsify_scans``, ``fd_velo_rasterize_batch`` for
the beam maps, ``fd_velo_rasterize_batch`` for ``depth_gt`` (frame 0's scan serves both, read and uploaded once) and
``fd_scatter_2channel``.  Rows: ``line_spec``, default the reference's list for ``opt.nbeams``; ``opt.random_sample > 0`` samples
instead, with the generator keyed by (``seed``, folder, frame index) - a frame's sparse scan is the same in every epoch, batch and
worker order, and the same as the offline tool writes with ``--seed``.  The two sources give bit-identical batches.

The Refiner's loader.  ``KITTIRefinerBatches`` is ``KITTIRAWBatches`` plus the ``"inf_gdc"`` key (mono_dataset.py:224-226,
kitti_dataset.py:154-173): the dense GDC-corrected depth ``python -m fusiondepth_amd.inf_gdc`` wrote per frame, resized to
``(height, width)`` with ATen's CPU bilinear rule and mirrored after the resize where the item is flipped - bit-identical to the
reference's ``F.interpolate`` + ``fliplr`` on the host.  The maps of a batch differ in size with the date; the worker threads load
them straight into one pinned staging buffer that also carries the descriptor table, so the key costs ONE host-to-device copy and
ONE library call (``fd_resize_bilinear_batch``) per batch.  Shape ``[B, height, width]``, the reference's squeezed shape (it
hardcodes ``[192, 640]``: the same deviation as ``4beam``, identical at the default size).  Every other key is the parent's.

The stereo loader.  ``KITTIStereoBatches`` is ``KITTIRAWBatches`` plus the stereo partner ``"s"`` of ``--use_stereo``
(mono_dataset.py:156-163, 216-222): ``("color" | "color_aug", "s", scale)`` = the other camera's image at the item's own frame index,
with the item's flip and jitter draw, and ``"stereo_T"`` [B,4,4], built on the host for the batch and sent with one upload.  ``"s"``
has no LiDAR scan and no ``("2channel", "s", 0)``.  Every other key is the parent's.

Rank sharding.  ``rank`` / ``world_size`` (inherited by every builder below and by the completion and detection loaders) give each
process of a data-parallel job its own batches.  The global order of an epoch stays ``default_rng([seed, epoch]).permutation(n)``, the
same on every rank; it is cut into global batches of ``batch_size``, of which only the first ``(n // (batch_size * world_size)) *
world_size`` are used, and global batch k goes to rank ``k % world_size``.  Every rank therefore yields the same number of batches
(``len(loader)``) - an unequal count would leave a rank alone in the gradient all-reduce - which is also why ``world_size > 1`` with
``drop_last=False`` raises.  ``item_draws`` stays keyed by (seed, epoch, index): an item gets the same flip and jitter on whichever
rank it lands.  With the defaults (rank 0 of 1) the order and every batch are what they were.

Not covered (each raises): ``need_full_res_4beam`` (needs cv2; ``4beam_full`` / ``2channel_full`` are read by nothing in the
reference); the stereo frame ``"s"`` everywhere but in ``KITTIStereoBatches``; in ``KITTIRAWBatches`` itself also ``need_inf_gdc`` /
``clone_gdc`` - those are ``KITTIRefinerBatches``'.
"""
import concurrent.futures
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import data_ops
from . import image_codecs
from . import kitti_utils
from . import sparsify as SP
from . import synthetic
from ._lib import round16

SIDE_MAP = {"2": 2, "3": 3, "l": 2, "r": 3}                  # kitti_dataset.py:42
JITTER_RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))     # mono_dataset.py:65-68


def pil_loader(path):
    """mono_dataset.py:14-17 -> [H,W,3] uint8."""
    from PIL import Image
    with open(path, "rb") as f:
        with Image.open(f) as img:
            return np.asarray(img.convert("RGB"))


def _read_into(path, dst):
    """Fill the uint8 array ``dst`` (a slice of the staging buffer) from the start of a file."""
    with open(path, "rb") as f:
        got = f.readinto(memoryview(dst))
    if got != dst.size:
        raise RuntimeError("KITTIRAWBatches: %s changed size while it was read (%d of %d bytes)" % (path, got, dst.size))


def _upload(staging, device):
    """The one host-to-device copy of a raw-mode batch's LiDAR data."""
    return staging.to(device, non_blocking=True)


def parse_line(line):
    """One split-file line ``"<folder> <frame> <side>"`` -> (folder, frame_index, side); a bare folder gives (folder, 0, None)
    (mono_dataset.py:138-154)."""
    parts = line.split()
    if len(parts) == 3:
        return parts[0], int(parts[1]), parts[2]
    return parts[0], 0, None


class KITTIRAWBatches:
    """See the module docstring.  The first nine arguments are ``KITTIRAWDataset``'s; ``batch_size`` / ``shuffle`` are the
    ``DataLoader``'s, ``drop_last`` too (default True; False also yields the trailing partial batch).  ``seed`` seeds the epoch
    order and the per-item draws, ``workers`` sizes the decode pool (at most 16), ``draws`` = callable ``(epoch, index) -> dict``
    that replaces ``item_draws`` (tests inject flags and jitter parameters through it), ``loader`` = callable ``path -> [H,W,3]
    uint8`` instead of the PIL decoder (pre-decoded frames), ``prefetch`` = issue the next batch on a side stream before handing
    out the current one, ``lidar_source`` = ``"files"`` (sparse scans written offline) or ``"raw"`` (sparsified here from
    ``velodyne_points``), ``line_spec`` = the rows raw mode keeps (default: the reference's list for ``opt.nbeams``),
    ``sparsify_grid`` = (H, W) of its angular grid, ``rank`` / ``world_size`` = this process's shard of every epoch (data-parallel
    training; the defaults give the whole epoch, exactly as before), ``decoder`` = ``"pil"`` (Pillow on the pool, the default) or
    ``"device"`` (``image_codecs.JpegBatchJob``: Huffman decoding on the pool, the rest in HIP, byte for byte Pillow's frames;
    ``decode_stats`` counts the frames each way; it is for JPEG frames and changes nothing for a ``.png`` tree, ``loader=`` with it
    raises), ``png_decoder`` = the same choice for a ``.png`` tree (``image_codecs.PngBatchJob``: the inflate on the pool, the scanline
    filters in HIP, byte for byte Pillow's frames, counted in ``decode_stats`` too; it changes nothing for a JPEG tree, ``loader=``
    with it raises)."""

    def __init__(self, data_path, filenames, height, width, frame_idxs, num_scales, is_train=False, img_ext=".jpg", opt=None,
                 batch_size=1, shuffle=False, seed=0, device="cuda", workers=8, jitter_per_image=False, draws=None, loader=None,
                 prefetch=True, lidar_source="files", line_spec=None, sparsify_grid=(64, 1024), drop_last=True, rank=0, world_size=1,
                 decoder="pil", png_decoder="pil"):
        self.data_path, self.filenames = data_path, list(filenames)
        self.height, self.width, self.num_scales = int(height), int(width), int(num_scales)
        self.frame_idxs = list(frame_idxs)
        self.is_train, self.img_ext, self.opt = bool(is_train), img_ext, opt
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.drop_last = bool(drop_last)
        self.device = torch.device(device)
        self.workers = max(1, min(int(workers), 16))
        self.jitter_per_image = bool(jitter_per_image)
        self.draws, self.loader, self.prefetch = draws, loader or pil_loader, bool(prefetch)
        if decoder not in ("pil", "device"):
            raise ValueError("KITTIRAWBatches: decoder must be 'pil' or 'device', got %r" % (decoder,))
        if decoder == "device" and loader is not None:
            raise ValueError("KITTIRAWBatches: decoder='device' decodes the files itself; it cannot be combined with loader=")
        if png_decoder not in ("pil", "device"):
            raise ValueError("KITTIRAWBatches: png_decoder must be 'pil' or 'device', got %r" % (png_decoder,))
        if png_decoder == "device" and loader is not None:
            raise ValueError("KITTIRAWBatches: png_decoder='device' decodes the files itself; it cannot be combined with loader=")
        # each argument speaks for its own kind of tree: decoder= for JPEG frames, png_decoder= for PNG frames
        self.decoder = decoder if str(img_ext).lower() in (".jpg", ".jpeg") else "pil"
        self.png_decoder = png_decoder if str(img_ext).lower() == ".png" else "pil"
        self.decode_stats = {"device": 0, "fallback": 0}
        if self.batch_size < 1:
            raise ValueError("KITTIRAWBatches: batch_size must be positive")
        self.rank, self.world_size = int(rank), int(world_size)
        if self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError("KITTIRAWBatches: rank %d is not in [0, world_size = %d)" % (self.rank, self.world_size))
        if self.world_size > 1 and not self.drop_last:
            raise ValueError("KITTIRAWBatches: world_size > 1 needs drop_last=True (a trailing partial batch would leave one rank "
                             "alone in the gradient all-reduce)")
        self.served = []                                         # (epoch, item indices) of every epoch handed out, in order
        self._check_covered()
        if 0 not in self.frame_idxs:
            raise ValueError("KITTIRAWBatches: frame_idxs must contain 0 (the frame every network and the LiDAR keys refer to)")
        self.need_4beam = bool(self._opt("need_4beam"))
        self.need_2_channel = bool(self._opt("need_2_channel"))
        self.load_depth = self.check_depth()
        if lidar_source not in ("files", "raw"):
            raise ValueError("KITTIRAWBatches: lidar_source must be 'files' or 'raw', got %r" % (lidar_source,))
        self.lidar_source = lidar_source
        self.sparsify_grid = (int(sparsify_grid[0]), int(sparsify_grid[1]))
        self.random_sample = max(int(self._opt("random_sample", -1)), 0)
        if line_spec is None and not self.random_sample:
            nbeams = int(self._opt("nbeams", 4))
            if lidar_source == "raw" and nbeams not in data_ops.SPARSIFY_LINE_SPEC:
                raise ValueError("KITTIRAWBatches: no default row list for nbeams = %d; pass line_spec" % nbeams)
            line_spec = data_ops.SPARSIFY_LINE_SPEC.get(nbeams)
        self.line_spec = None if line_spec is None else [int(r) for r in line_spec]
        self._epoch = 0
        self._open = 0                                           # iterations begun and not yet finished or dropped
        self._pool = None
        self._stream = None
        self._K = {}
        self._calib = {}

    def _opt(self, name, default=False):
        return getattr(self.opt, name, default) if self.opt is not None else default

    def _check_covered(self):
        """Refuse what this class does not build (module docstring, "Not covered"); a subclass that builds more overrides it."""
        if "s" in self.frame_idxs:
            raise NotImplementedError("KITTIRAWBatches: the stereo frame 's' is not covered (temporal frames only)")
        if self._opt("need_full_res_4beam"):
            raise NotImplementedError("KITTIRAWBatches: need_full_res_4beam is not covered (the reference resizes with cv2)")
        if self._opt("need_inf_gdc") or self._opt("clone_gdc"):
            raise NotImplementedError("KITTIRAWBatches: need_inf_gdc / clone_gdc are not covered (no inf_gdc maps are loaded); "
                                      "KITTIRefinerBatches loads them")

    # ---- paths (kitti_dataset.py:44-54, 72-76, 93-103) --------------------------------------------------------------------------
    def get_image_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, folder, "image_0{}/data".format(SIDE_MAP[side]), "{:010d}{}".format(frame_index, self.img_ext))

    def get_velo_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "velodyne_points/data/{:010d}.bin".format(int(frame_index)))

    def frame_image_path(self, folder, frame_index, side, f):
        """The image of frame slot ``f`` of an item (mono_dataset.py:156-161)."""
        return self.get_image_path(folder, frame_index + f, side)

    def lidar_frames(self):
        """The frame slots that have a LiDAR scan of their own, in the order of the per-frame LiDAR keys."""
        return self.frame_idxs

    def beam_folder(self):
        random_sample = self._opt("random_sample", -1)
        return "random{}".format(random_sample) if random_sample > 0 else "{}beam".format(self._opt("nbeams", 4))

    def get_beam_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "{}/{:010d}.bin".format(self.beam_folder(), int(frame_index)))

    def check_depth(self):
        if not self.filenames:
            return False
        folder, frame_index, _ = parse_line(self.filenames[0])
        return os.path.isfile(self.get_velo_path(folder, frame_index))

    def close(self):
        """Stop the decode pool (idle threads otherwise live as long as the object)."""
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- order and draws --------------------------------------------------------------------------------------------------------
    def __len__(self):
        """Batches per epoch on THIS rank (the same number on every rank)."""
        n, B = len(self.filenames), self.batch_size
        if self.world_size > 1:
            return n // (B * self.world_size)
        return n // B if self.drop_last else (n + B - 1) // B

    def epoch_order(self, epoch):
        """Item indices of one epoch on this rank, in batch order (with ``drop_last`` the trailing partial batch is dropped).  The
        global order is the same on every rank; it is cut into global batches of ``batch_size``, the first ``len(self) * world_size``
        of them are used and global batch k goes to rank ``k % world_size`` (module docstring, "Rank sharding")."""
        n = len(self.filenames)
        order = np.random.default_rng([self.seed, int(epoch)]).permutation(n) if self.shuffle else np.arange(n)
        if self.world_size > 1:
            B, W = self.batch_size, self.world_size
            return [int(i) for k in range(self.rank, len(self) * W, W) for i in order[k * B:(k + 1) * B]]
        return [int(i) for i in order[:len(self) * self.batch_size if self.drop_last else n]]

    def item_draws(self, epoch, index):
        """The random part of one item, a function of (seed, epoch, index) alone: ``do_color_aug`` and ``do_flip`` (``random() > 0.5``
        each, training only) and ``jitter``: one ``((brightness, contrast, saturation, hue), order)`` draw, or with
        ``jitter_per_image`` a list ``[frame][scale]`` of them; None without colour augmentation."""
        if self.draws is not None:
            return self.draws(epoch, index)
        rng = np.random.default_rng([self.seed, int(epoch), int(index), 1])
        do_color_aug = self.is_train and rng.random() > 0.5
        do_flip = self.is_train and rng.random() > 0.5

        def one():
            order = [int(o) for o in rng.permutation(4)]
            return tuple(float(rng.uniform(lo, hi)) for lo, hi in JITTER_RANGES), order

        jitter = None
        if do_color_aug:
            jitter = [[one() for _ in range(self.num_scales)] for _ in self.frame_idxs] if self.jitter_per_image else one()
        return {"do_color_aug": bool(do_color_aug), "do_flip": bool(do_flip), "jitter": jitter}

    # ---- host side of a batch ---------------------------------------------------------------------------------------------------
    def _workers(self):
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers)
        return self._pool

    def plan_batch(self, epoch, indices):
        """Everything about a batch that needs no device: per item (folder, frame, side, draws) and the files to read."""
        items = []
        for index in indices:
            folder, frame_index, side = parse_line(self.filenames[index])
            d = self.item_draws(epoch, index)
            item = {"index": index, "folder": folder, "frame_index": frame_index, "side": side, "date": folder.split("/")[0],
                    "do_flip": bool(d["do_flip"]), "jitter": d["jitter"] if d["do_color_aug"] else None,
                    "images": [self.frame_image_path(folder, frame_index, side, f) for f in self.frame_idxs],
                    "beams": [], "velo": None}
            if self.need_4beam or self.need_2_channel:
                frames = self.lidar_frames() if self.need_2_channel else [0]
                item["beams"] = [self.get_beam_path(folder, frame_index + f) for f in frames]
            if self.load_depth:
                item["velo"] = self.get_velo_path(folder, frame_index)
            if self.lidar_source == "raw":                       # the raw scans of the frames whose beam maps are needed
                item["frames"] = [frame_index + f for f in frames] if item["beams"] else []
                item["beams"] = [self.get_velo_path(folder, i) for i in item["frames"]]
            items.append(item)
        return items

    def _plan_staging(self, items):
        """Raw mode: the layout of the batch's staging buffer.  Scans are frame-major like every other key; with ``depth_gt`` alone
        (no beam keys) the scans are the items' own frames.  Frame 0's scan serves ``depth_gt`` too, so it appears once."""
        per_item = len(items[0]["beams"])
        if per_item:
            scans = [(it, it["beams"][k], it["frames"][k]) for k in range(per_item) for it in items]
        else:
            scans = [(it, it["velo"], it["frame_index"]) for it in items if it["velo"]]
        S = len(scans)
        lengths = [os.path.getsize(path) // 16 for _, path, _ in scans]
        plan = {"S": S, "lengths": lengths, "sparse": bool(per_item), "scans": scans}
        at = 0
        for name, nbytes in (("offsets", 4 * (S + 1)), ("keys", 8 * S), ("descs", ctypes.sizeof(_lib.RasterDesc) * S)):
            plan[name] = (at, at + nbytes)
            at = round16(at + nbytes)
        plan["points"] = (at, at + 16 * sum(lengths))
        plan["bytes"] = max(plan["points"][1], 16)
        return plan

    def _start_raw(self, items, pool):
        """Raw mode: one pinned staging buffer per batch, filled by the pool - the files are read straight into it."""
        plan = self._plan_staging(items)
        if not plan["S"]:
            return None
        staging = torch.empty((plan["bytes"],), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        ends = np.cumsum([0] + plan["lengths"])
        if ends[-1] >= 2 ** 31:
            raise RuntimeError("KITTIRAWBatches: %d points in one batch" % ends[-1])
        host[plan["offsets"][0]:plan["offsets"][1]].view(np.int32)[:] = ends
        host[plan["keys"][0]:plan["keys"][1]].view(np.uint64)[:] = np.array([SP.scan_key(it["folder"], frame) for it, _, frame in plan["scans"]],
                                                                              dtype=np.uint64)
        descs = []
        for it, _, _ in plan["scans"]:
            P, (im_h, im_w) = self._projection(it["date"], SIDE_MAP[it["side"]])
            descs.append((P, im_h, im_w, it["do_flip"]))
        table = data_ops.raster_desc_table(descs)
        host[plan["descs"][0]:plan["descs"][1]] = np.frombuffer(table, dtype=np.uint8)
        base = plan["points"][0]
        plan["futures"] = [pool.submit(_read_into, path, host[base + 16 * int(ends[k]):base + 16 * int(ends[k + 1])])
                           for k, (_, path, _) in enumerate(plan["scans"])]
        plan["staging"], plan["desc_list"] = staging, descs
        return plan

    def _start_host(self, epoch, indices):
        """Submit the file work of a batch to the pool."""
        items = self.plan_batch(epoch, indices)
        pool = self._workers()
        on_device = self.decoder == "device" or self.png_decoder == "device"
        if on_device:                                            # frame-major, the order of every colour key
            job = image_codecs.JpegBatchJob if self.decoder == "device" else image_codecs.PngBatchJob
            items[0]["decode_job"] = job([it["images"][fi] for fi in range(len(self.frame_idxs)) for it in items], pool)
        for it in items:
            if not on_device:
                it["image_futures"] = [pool.submit(self.loader, p) for p in it["images"]]
            if self.lidar_source == "raw":
                continue
            it["beam_futures"] = [pool.submit(kitti_utils.load_velodyne_points, p) for p in it["beams"]]
            it["velo_future"] = pool.submit(kitti_utils.load_velodyne_points, it["velo"]) if it["velo"] else None
        if self.lidar_source == "raw":
            items[0]["raw_plan"] = self._start_raw(items, pool)
        return items

    def _projection(self, date, cam):
        key = (date, cam)
        if key not in self._calib:
            self._calib[key] = kitti_utils.velo_to_image(os.path.join(self.data_path, date), cam)
        return self._calib[key]

    # ---- device side of a batch -------------------------------------------------------------------------------------------------
    def _colour_keys(self, items, batch):
        B, F = len(items), len(self.frame_idxs)
        groups, stacks = {}, {}                                  # native size -> [(frame slot, item)]: drives differ in size
        if "decode_job" in items[0]:                             # decoded on the device: the stacks are views of one buffer
            decoded, stats = items[0]["decode_job"].finish(self.device)
            for name in stats:
                self.decode_stats[name] += stats[name]
            for (h, w), (stack, idx) in decoded.items():
                groups[(h, w, 3)], stacks[(h, w, 3)] = [(i // B, i % B) for i in idx], stack
        else:
            frames = [[f.result() for f in it["image_futures"]] for it in items]
            for fi in range(F):                                  # frame-major: with one native size every key is a contiguous slice
                for b in range(B):
                    groups.setdefault(frames[b][fi].shape, []).append((fi, b))
        sizes = [(self.height // 2 ** s, self.width // 2 ** s) for s in range(self.num_scales)]
        whole = {}
        for shape, members in groups.items():
            if len(shape) != 3 or shape[2] != 3:
                raise RuntimeError("KITTIRAWBatches: a decoded frame has shape %s, expected [H,W,3]" % (shape,))
            if shape in stacks:
                stack = stacks[shape]
            else:
                stack = torch.from_numpy(np.stack([frames[b][fi] for fi, b in members])).to(self.device, non_blocking=True)
            flip = [items[b]["do_flip"] for _, b in members]
            jitter = None
            if any(it["jitter"] is not None for it in items):
                jitter = []
                for fi, b in members:
                    j = items[b]["jitter"]
                    jitter.append(j[fi] if isinstance(j, list) else j)
            pyr = data_ops.image_pyramid(stack, self.height, self.width, self.num_scales, flip, jitter)
            if len(groups) == 1:
                whole = pyr
                break
            slots = torch.tensor([fi * B + b for fi, b in members], device=self.device)
            for s, (h, w) in enumerate(sizes):
                for name in ("color", "color_aug"):
                    if (name, s) not in whole:
                        whole[(name, s)] = torch.empty((F * B, 3, h, w), device=self.device)
                    whole[(name, s)][slots] = pyr[(name, s)]
        for fi, f in enumerate(self.frame_idxs):
            for s in range(self.num_scales):
                for name in ("color", "color_aug"):
                    batch[(name, f, s)] = whole[(name, s)][fi * B:(fi + 1) * B]

    def _lidar_keys_raw(self, items, batch):
        """The LiDAR keys from raw scans: one upload and four library calls whatever the batch size (module docstring)."""
        plan = items[0]["raw_plan"]
        if plan is None:
            return
        for f in plan["futures"]:
            f.result()
        dev = _upload(plan["staging"], self.device)
        S, B, descs = plan["S"], len(items), plan["desc_list"]
        part = lambda name: dev[plan[name][0]:plan[name][1]]
        offsets, keys, table = part("offsets").view(torch.int32), part("keys").view(torch.int64), part("descs")
        points = part("points").view(torch.float32).view(-1, 4)
        zero = 0
        if plan["sparse"]:
            H, W = self.sparsify_grid
            slab, _ = data_ops.sparsify_scans(points, H, W, None if self.random_sample else self.line_spec, 1, self.random_sample, None,
                                        self.seed, keys, offsets=offsets)
            beams = data_ops.velo_rasterize_batch(slab, descs, (2 * self.height, 2 * self.width), desc_table=table).unsqueeze(1)
            zero = self.lidar_frames().index(0) if self.need_2_channel else 0
            if self.need_2_channel:
                two = data_ops.scatter_2channel(beams, data_ops.scaled_roi(self.height, self.width))
                for fi, f in enumerate(self.lidar_frames()):
                    batch[("2channel", f, 0)] = two[fi * B:(fi + 1) * B]
            if self.need_4beam:
                batch["4beam"] = beams[zero * B:(zero + 1) * B]
                if self.need_2_channel:
                    batch["2channel"] = two[zero * B:(zero + 1) * B]
        if self.load_depth:                                      # frame 0's scans are B consecutive entries of the same tables
            size = ctypes.sizeof(_lib.RasterDesc)
            full = data_ops.velo_rasterize_batch(points, descs[zero * B:(zero + 1) * B], (375, 1242), return_full=True, beam=False,
                                           offsets=offsets[zero * B:(zero + 1) * B + 1], n_max=max(plan["lengths"][zero * B:(zero + 1) * B]),
                                           desc_table=table[zero * B * size:(zero + 1) * B * size])
            batch["depth_gt"] = full.float().unsqueeze(1)

    def _lidar_keys(self, items, batch):
        if self.lidar_source == "raw":
            return self._lidar_keys_raw(items, batch)
        if self.need_4beam or self.need_2_channel:
            per_item = len(items[0]["beams"])
            beams = []
            for k in range(per_item):                            # frame-major, like the colour keys
                for it in items:
                    P, (im_h, im_w) = self._projection(it["date"], SIDE_MAP[it["side"]])
                    pts = torch.from_numpy(it["beam_futures"][k].result()).to(self.device, non_blocking=True)
                    beam = data_ops.velo_rasterize(pts, P, im_h, im_w, (2 * self.height, 2 * self.width))     # [384, 1280] at 192x640
                    beams.append(torch.flip(beam, dims=[1]) if it["do_flip"] else beam)
            beams = torch.stack(beams).unsqueeze(1).contiguous()
            B = len(items)
            zero = self.lidar_frames().index(0) if self.need_2_channel else 0
            if self.need_2_channel:                              # mono_dataset.py:162-163: one per frame, with or without need_4beam
                two = data_ops.scatter_2channel(beams, data_ops.scaled_roi(self.height, self.width))
                for fi, f in enumerate(self.lidar_frames()):
                    batch[("2channel", f, 0)] = two[fi * B:(fi + 1) * B]
            if self.need_4beam:                                  # mono_dataset.py:193-206
                batch["4beam"] = beams[zero * B:(zero + 1) * B]
                if self.need_2_channel:
                    batch["2channel"] = two[zero * B:(zero + 1) * B]
        if self.load_depth:
            maps = []
            for it in items:
                P, (im_h, im_w) = self._projection(it["date"], SIDE_MAP[it["side"]])
                pts = torch.from_numpy(it["velo_future"].result()).to(self.device, non_blocking=True)
                full = data_ops.velo_rasterize(pts, P, im_h, im_w, (375, 1242), return_full=True, beam=False)
                maps.append((torch.flip(full, dims=[1]) if it["do_flip"] else full).float())
            batch["depth_gt"] = torch.stack(maps).unsqueeze(1).contiguous()

    def _finish_batch(self, items):
        """The device work of one batch, on the current stream."""
        batch = {}
        if self.opt is not None:
            batch["date"] = [it["date"] for it in items]
            if self._opt("need_path"):
                batch["path"] = [self.filenames[it["index"]] for it in items]
        self._colour_keys(items, batch)
        if len(items) not in self._K:                            # by batch size: the trailing partial batch has its own
            self._K[len(items)] = synthetic.intrinsics(len(items), self.height, self.width, self.num_scales, self.device)
        batch.update(self._K[len(items)])
        self._lidar_keys(items, batch)
        return batch

    def build_batch(self, epoch, indices):
        """One batch, start to finish, on the current stream (no prefetch)."""
        return self._finish_batch(self._start_host(epoch, indices))

    def _issue(self, items):
        """Device work of a batch on the builder's stream -> (batch, event)."""
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self._stream):
            batch = self._finish_batch(items)
            done = torch.cuda.Event()
            done.record(self._stream)
        return batch, done

    @staticmethod
    def _tensors(batch):
        return [v for v in batch.values() if torch.is_tensor(v)]

    def set_epoch(self, n):
        """The next ``__iter__`` serves ``epoch_order(n)`` with the draws of epoch ``n`` (a continued run, ``Trainer.resume``).
        Refused while an iteration is open: its batches are being built ahead from the epoch it started with."""
        if self._open:
            raise RuntimeError("%s.set_epoch: an iteration is open; finish or drop it first" % type(self).__name__)
        if int(n) < 0:
            raise ValueError("%s.set_epoch: the epoch must not be negative, got %r" % (type(self).__name__, n))
        self._epoch = int(n)

    def __iter__(self):
        epoch = self._epoch
        self._epoch += 1
        order = self.epoch_order(epoch)
        self.served.append((epoch, order))
        self._open += 1
        try:
            yield from self._batches(epoch, order)
        finally:
            self._open -= 1

    def _batches(self, epoch, order):
        """The batches of one epoch, in ``order``."""
        B = self.batch_size
        chunks = [order[i * B:(i + 1) * B] for i in range(len(self))]
        if not chunks:
            return
        if not (self.prefetch and self.device.type == "cuda"):
            host = self._start_host(epoch, chunks[0])
            for i in range(len(chunks)):
                nxt = self._start_host(epoch, chunks[i + 1]) if i + 1 < len(chunks) else None    # files of the next batch meanwhile
                yield self._finish_batch(host)
                host = nxt
            return
        with torch.cuda.device(self.device):
            host = [self._start_host(epoch, c) for c in chunks[:2]]                # file work runs up to two batches ahead
            pending = self._issue(host.pop(0))
            for i in range(len(chunks)):
                if i + 2 < len(chunks):
                    host.append(self._start_host(epoch, chunks[i + 2]))
                batch, done = pending
                pending = self._issue(host.pop(0)) if i + 1 < len(chunks) else None    # batch i + 1 goes out before batch i is consumed
                cur = torch.cuda.current_stream()
                cur.wait_event(done)
                for t in self._tensors(batch):
                    t.record_stream(cur)
                yield batch


OTHER_SIDE = {"l": "r", "r": "l"}                             # mono_dataset.py:157


def stereo_T(side, do_flip):
    """mono_dataset.py:216-222: the pose of the stereo partner, a 0.1 baseline along x whose sign depends on the side and the flip."""
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = (-1 if side == "l" else 1) * (-1 if do_flip else 1) * 0.1
    return T


class KITTIStereoBatches(KITTIRAWBatches):
    """``KITTIRAWBatches`` for ``--use_stereo``: accepts the stereo partner ``"s"`` in ``frame_idxs`` (``[0, "s"]``, ``[0, -1, 1,
    "s"]``) and adds ``("color" | "color_aug", "s", scale)`` and ``"stereo_T"``; see the module docstring.  Same arguments; every
    other key is the parent's, and both ``lidar_source`` modes work.  With ``jitter_per_image`` the slot of ``"s"`` has its own
    ``[scale]`` list of draws like every other frame slot.

    ``"s"`` gets no ``("2channel", "s", 0)``: the dataset makes none (mono_dataset.py:156-163), and ``Trainer.predict_poses`` reads
    that key for the temporal frames only.  The reference itself reads it for every frame id, so with stereo + temporal frames and
    its default pose network it dies with a ``KeyError`` at trainer.py:334; this port does not."""

    def _check_covered(self):
        if self._opt("need_full_res_4beam"):
            raise NotImplementedError("KITTIStereoBatches: need_full_res_4beam is not covered (the reference resizes with cv2)")
        if self._opt("need_inf_gdc") or self._opt("clone_gdc"):
            raise NotImplementedError("KITTIStereoBatches: need_inf_gdc / clone_gdc are not covered (no inf_gdc maps are loaded); "
                                      "KITTIRefinerBatches loads them")
        for f in self.frame_idxs:
            if f != "s" and not isinstance(f, (int, np.integer)):
                raise ValueError("KITTIStereoBatches: frame id %r is neither an integer nor 's'" % (f,))

    def frame_image_path(self, folder, frame_index, side, f):
        if f == "s":
            return self.get_image_path(folder, frame_index, OTHER_SIDE[side])
        return super().frame_image_path(folder, frame_index, side, f)

    def lidar_frames(self):
        return [f for f in self.frame_idxs if f != "s"]

    def plan_batch(self, epoch, indices):
        if "s" in self.frame_idxs:
            for index in indices:
                if parse_line(self.filenames[index])[2] not in OTHER_SIDE:
                    raise ValueError("KITTIStereoBatches: the split line %r names no side ('l' or 'r'), so it has no stereo partner"
                                     % (self.filenames[index],))
        return super().plan_batch(epoch, indices)

    def _finish_batch(self, items):
        batch = super()._finish_batch(items)
        if "s" in self.frame_idxs:
            host = np.stack([stereo_T(it["side"], it["do_flip"]) for it in items])
            batch["stereo_T"] = torch.from_numpy(host).to(self.device, non_blocking=True)
        return batch


def _load_map_into(path, dst):
    """``np.load(path).astype(np.float32)`` (kitti_dataset.py:166-167) straight into ``dst``, a 2-D float32 view of the staging
    buffer planned from the date's image size."""
    a = np.load(path)
    if a.shape != dst.shape:
        raise RuntimeError("KITTIRefinerBatches: %s holds a map of shape %s; the calibration of its date says %s"
                           % (path, a.shape, dst.shape))
    np.copyto(dst, a, casting="unsafe")


class KITTIRefinerBatches(KITTIRAWBatches):
    """``KITTIRAWBatches`` for the Refiner: accepts ``opt.need_inf_gdc`` / ``opt.clone_gdc`` and adds ``batch["inf_gdc"]``
    ([B, height, width] float32) whenever ``(opt.clone_gdc and is_train) or opt.need_inf_gdc`` (mono_dataset.py:224); see the
    module docstring.  Same arguments; every other key is the parent's."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.need_gdc = bool((self._opt("clone_gdc") and self.is_train) or self._opt("need_inf_gdc"))

    def _check_covered(self):
        if "s" in self.frame_idxs:
            raise NotImplementedError("KITTIRefinerBatches: the stereo frame 's' is not covered (temporal frames only)")
        if self._opt("need_full_res_4beam"):
            raise NotImplementedError("KITTIRefinerBatches: need_full_res_4beam is not covered (the reference resizes with cv2)")

    # ---- paths (kitti_dataset.py:154-161) ---------------------------------------------------------------------------------------
    def gdc_folder(self):
        random_sample = self._opt("random_sample", -1)
        return "inf_gdc_r{}".format(random_sample) if random_sample > 0 else "inf_gdc_{}beam".format(self._opt("nbeams", 4))

    def get_gdc_path(self, folder, frame_index, side):
        return os.path.join(self.data_path, folder, "{}/{}_{}.npy".format(self.gdc_folder(), int(frame_index), side))

    # ---- host side --------------------------------------------------------------------------------------------------------------
    def plan_batch(self, epoch, indices):
        items = super().plan_batch(epoch, indices)
        if self.need_gdc:
            for it in items:
                it["gdc"] = self.get_gdc_path(it["folder"], it["frame_index"], it["side"])
        return items

    def _plan_gdc(self, items):
        """Layout of the key's staging buffer, before any map is read: the descriptor table, then the planes, each of its date's
        image size (``inf_gdc`` writes its maps at the size of camera 2's rectified image, whatever the side)."""
        B = len(items)
        table_bytes = ctypes.sizeof(_lib.ResizeDesc) * B
        base = round16(table_bytes)
        descs, at = [], 0
        for it in items:
            _, (im_h, im_w) = self._projection(it["date"], 2)
            descs.append((at, int(im_h), int(im_w), it["do_flip"]))
            at += int(im_h) * int(im_w)
        return {"descs": descs, "table": (0, table_bytes), "planes": (base, base + 4 * at), "bytes": base + 4 * at}

    def _start_gdc(self, items, pool):
        """One pinned staging buffer per batch; the pool loads every map straight into its slice."""
        for it in items:
            if not os.path.isfile(it["gdc"]):
                raise FileNotFoundError("KITTIRefinerBatches: %s is missing; `python -m fusiondepth_amd.inf_gdc` writes the inf_gdc maps "
                                        "(from the inf_depth maps of `python -m fusiondepth_amd.inf_depth_map`)" % it["gdc"])
        plan = self._plan_gdc(items)
        staging = torch.empty((plan["bytes"],), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        host[plan["table"][0]:plan["table"][1]] = np.frombuffer(data_ops.resize_desc_table(plan["descs"]), dtype=np.uint8)
        planes = host[plan["planes"][0]:plan["planes"][1]].view(np.float32)
        plan["futures"] = [pool.submit(_load_map_into, it["gdc"], planes[at:at + h * w].reshape(h, w))
                           for it, (at, h, w, _) in zip(items, plan["descs"])]
        plan["staging"] = staging
        return plan

    def _start_host(self, epoch, indices):
        items = super()._start_host(epoch, indices)
        if self.need_gdc:
            items[0]["gdc_plan"] = self._start_gdc(items, self._workers())
        return items

    # ---- device side ------------------------------------------------------------------------------------------------------------
    def _finish_batch(self, items):
        batch = super()._finish_batch(items)
        if self.need_gdc:
            plan = items[0]["gdc_plan"]
            for f in plan["futures"]:
                f.result()                                       # a size mismatch raises here, with the path
            dev = _upload(plan["staging"], self.device)
            table = dev[plan["table"][0]:plan["table"][1]]
            planes = dev[plan["planes"][0]:plan["planes"][1]].view(torch.float32)
            batch["inf_gdc"] = data_ops.resize_bilinear_batch(planes, plan["descs"], (self.height, self.width), desc_table=table)
        return batch
