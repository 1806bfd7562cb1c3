"""KITTI depth-completion batches, built on the GPU: the reference's ``KITTICompletion`` (datasets/completion_dataset.py:142-369,
datasets/kitti_completion.py:13-80) plus the ``DataLoader`` around it (completor.py:131-146, evaluate_completion.py:94-98), as one
iterable of collated device batches in the reference's schema.

    loader = KITTICompletionBatches(data_path + "/completion", 352, 1216, [0, -1, 1], 4, is_train=True, opt=opts, batch_size=4,
                                    shuffle=True)
    Completor(opts).train(loader)

``completion_paths`` restates ``get_paths_and_transform`` (completion_dataset.py:22-139).  ``KITTICompletionBatches`` subclasses
``KITTIRAWBatches`` and keeps its machinery: the epoch order, ``item_draws``, the decode pool, file work two batches ahead, the
builder stream and the hand-over event.

What runs where
  * host, in the pool: every colour PNG is decoded and bottom-cropped to 352x1216 (full-res mode) or zero-padded to 384x1280
    (``--completion_not_full_res``) with a slice copy into the batch's pinned stack; every 16-bit depth PNG is decoded (PIL
    returns a fresh array) and copied into its uint16 slice of one pinned staging buffer that also carries the descriptor tables.
    The reference's ``max > 255`` assertion runs there and names the file.  The buffer's layout needs every plane's size first: the
    PNG headers are read (nothing decoded) on the calling thread when the batch's file work is submitted, one open per file.
  * device: one upload of the stack and ``data_ops.image_pyramid`` for the colour keys (the mirror stays on the device: cropping
    at the mirrored offset and mirroring afterwards equals the reference's mirror-then-crop); one upload of the staging buffer and at
    most four library calls for the depth keys whatever the batch size - ``fd_depth_png_keys`` for all beam planes (frame-major;
    frame 0's slice serves ``"4beam"``), for ``depth_gt`` and, when asked, for ``full_res_4beam``, then at most one
    ``fd_scatter_2channel``.

Geometry (kitti_completion.py:29-80).  The mirror acts on the source.  ``bottom_crop`` keeps rows ``h - 352 .. h`` and columns from
``j = int(round((w - 1216) / 2.))`` - Python's round-half-even: 1241 gives 12.  The pad fills zeros to 384x1280, ``384 - h`` rows on
top and ``(1280 - w) // 2`` columns on the left.  ``get_depth``: ``/ 256``, mirror, crop (full-res mode), pad (``padding``), 2x2
ceil-mode max-pool (``pool``), and ``/ 100`` for the sparse input.  ``depth_gt`` is never pooled; ``full_res_4beam`` is padded and not
pooled in both modes (crop-then-pad in full-res mode).

Deviations from the reference, on purpose
  * ``load_4beam_2channel`` mirrors its ``[2,H,W]`` array with ``np.fliplr``, which flips axis 1: a VERTICAL flip.  Here a flipped
    item's 2-channel map is the scatter of the horizontally mirrored beam map, like every other key of the item and like
    ``KITTIRAWBatches``.
  * with ``completion_not_full_res`` the same function calls ``np.pad`` on the 3-D array with two pad pairs, which raises
    ``ValueError`` under numpy 2: ``completion_need2channel == "true"`` together with ``completion_not_full_res`` raises
    ``NotImplementedError`` here.
  * ``2cha/*.npy`` files are neither read nor needed: with ``completion_need2channel == "true"`` the map is computed online with
    gen2cha_completion.py's window (rows [110, 350), columns [2, 1214), expand 2) from the mirrored, cropped map / 100.
Not covered (raises): the stereo frame ``"s"``; the reference's ``inf`` demo paths.
"""
import ctypes
import glob
import os

import numpy as np
import torch

from . import _lib
from . import data_ops
from . import image_codecs
from . import synthetic
from ._lib import round16
from .datasets import KITTIRAWBatches, _upload, pil_loader

CROP = (352, 1216)                                           # bottom_crop, completion_dataset.py:230-244
PAD = (384, 1280)                                            # kitti_completion.py:35-40, 71-75
SCATTER_ROI = (110, 350, 2, 1214)                            # gen2cha_completion.py: rows [110, 350), columns [2, 1214) of 352x1216
SPLITS = ("train", "val", "test_completion", "test_prediction")


def completion_paths(data_folder, split, val_split="select", verify=True):
    """``get_paths_and_transform`` (completion_dataset.py:22-139) -> ``{"rgb": [...], "d": [...], "gt": [...]}``."""
    use_d = use_rgb = split in ("train", "val")
    glob_d = glob_gt = glob_rgb = get_rgb = None
    if split == "train":
        glob_d = os.path.join(data_folder, "data_depth_velodyne/train/*_sync/proj_depth/velodyne_raw/image_0[2,3]/*.png")
        glob_gt = os.path.join(data_folder, "data_depth_annotated/train/*_sync/proj_depth/groundtruth/image_0[2,3]/*.png")

        def get_rgb(p):
            ps = p.split("/")
            return "/".join([data_folder] + ["data_rgb"] + ps[-6:-4] + ps[-2:-1] + ["data"] + ps[-1:])
    elif split == "val":
        if val_split == "full":
            glob_d = os.path.join(data_folder, "data_depth_velodyne/val/*_sync/proj_depth/velodyne_raw/image_0[2,3]/*.png")
            glob_gt = os.path.join(data_folder, "data_depth_annotated/val/*_sync/proj_depth/groundtruth/image_0[2,3]/*.png")

            def get_rgb(p):
                ps = p.split("/")
                return "/".join(ps[:-7] + ["data_rgb"] + ps[-6:-4] + ps[-2:-1] + ["data"] + ps[-1:])
        elif val_split == "select":
            glob_d = os.path.join(data_folder, "depth_selection/val_selection_cropped/velodyne_raw/*.png")
            glob_gt = os.path.join(data_folder, "depth_selection/val_selection_cropped/groundtruth_depth/*.png")

            def get_rgb(p):
                return p.replace("groundtruth_depth", "image")
        else:                                                    # the reference leaves glob_gt unbound here: UnboundLocalError
            raise ValueError("Unrecognized val_split " + str(val_split))
    elif split == "test_completion":
        glob_d = os.path.join(data_folder, "depth_selection/test_depth_completion_anonymous/velodyne_raw/*.png")
        glob_rgb = os.path.join(data_folder, "depth_selection/test_depth_completion_anonymous/image/*.png")
    elif split == "test_prediction":
        glob_rgb = os.path.join(data_folder, "depth_selection/test_depth_prediction_anonymous/image/*.png")
    else:
        raise ValueError("Unrecognized split " + str(split))

    if glob_gt is not None:
        paths_d = sorted(glob.glob(glob_d))
        paths_gt = sorted(glob.glob(glob_gt))
        paths_rgb = [get_rgb(p) for p in paths_gt]
    else:
        paths_rgb = sorted(glob.glob(glob_rgb))
        paths_gt = [None] * len(paths_rgb)
        paths_d = [None] * len(paths_rgb) if split == "test_prediction" else sorted(glob.glob(glob_d))

    if verify and split == "train":                          # keep the items whose sparse file has both temporal neighbours on disk
        def has_frame(path, step):
            folder, name = os.path.split(path)
            return os.path.isfile(os.path.join(folder, "%010d.png" % (int(name[:name.find(".")]) + step)))

        keep = [k for k, p in enumerate(paths_d) if has_frame(p, -1) and has_frame(p, 1)]
        if keep and (keep[-1] >= len(paths_rgb) or keep[-1] >= len(paths_gt)):
            raise IndexError("completion_paths: fewer ground-truth than sparse files under %s" % data_folder)
        paths_d, paths_rgb, paths_gt = ([ps[k] for k in keep] for ps in (paths_d, paths_rgb, paths_gt))

    if len(paths_d) == 0 and len(paths_rgb) == 0 and len(paths_gt) == 0:
        raise RuntimeError("Found 0 images under {}".format(glob_gt))
    if len(paths_d) == 0 and use_d:
        raise RuntimeError("completion_paths: the %s split needs sparse depth maps and none matched %s" % (split, glob_d))
    if len(paths_rgb) == 0 and use_rgb:
        raise RuntimeError("completion_paths: the %s split needs colour images and none was found" % split)
    if len(paths_rgb) != len(paths_d) or len(paths_rgb) != len(paths_gt):
        raise RuntimeError("Produced different sizes for datasets")
    return {"rgb": paths_rgb, "d": paths_d, "gt": paths_gt}


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def crop_origin(h, w):
    """``bottom_crop`` (completion_dataset.py:230-244): first row and column kept.  round() is Python's, half to even."""
    return h - CROP[0], int(round((w - CROP[1]) / 2.))


def pad_origin(h, w):
    """The zero pad (kitti_completion.py:71-75): rows on top, columns on the left."""
    return PAD[0] - h, (PAD[1] - w) // 2


def colour_placement(h, w, do_flip, full_res):
    """Where a decoded [h,w,3] frame goes so that mirroring the result on the device equals the reference's mirror-then-crop (or
    mirror-then-pad): ``(canvas, (src_y, src_x), (dst_y, dst_x), (rows, cols))``."""
    if full_res:
        i, j = crop_origin(h, w)
        return CROP, (i, w - CROP[1] - j if do_flip else j), (0, 0), CROP
    y, x = pad_origin(h, w)
    return PAD, (0, 0), (y, PAD[1] - w - x if do_flip else x), (h, w)


def depth_desc(offset, h, w, do_flip, full_res, padding):
    """One ``fd_depth_png_desc`` tuple and its canvas for ``get_depth(path, do_flip, padding)`` in full-res or not-full-res mode
    (the pool and the divisors are the call's).  (offset, h, w, mirror, src_y, src_x, win_y, win_x, win_h, win_w), (H, W)."""
    if full_res:
        i, j = crop_origin(h, w)
        if padding:                                              # crop, then pad the 352x1216 map
            y, x = pad_origin(*CROP)
            return (offset, h, w, do_flip, i, j, y, x, CROP[0], CROP[1]), PAD
        return (offset, h, w, do_flip, i, j, 0, 0, CROP[0], CROP[1]), CROP
    if not padding:
        raise ValueError("depth_desc: not-full-res maps are always padded (their sizes differ)")
    y, x = pad_origin(h, w)
    return (offset, h, w, do_flip, 0, 0, y, x, h, w), PAD


def _check_size(path, h, w, full_res):
    if full_res and (h < CROP[0] or w < CROP[1]):
        raise RuntimeError("KITTICompletionBatches: %s is %d x %d, smaller than the %d x %d crop" % (path, h, w, CROP[0], CROP[1]))
    if not full_res and (h > PAD[0] or w > PAD[1]):
        raise RuntimeError("KITTICompletionBatches: %s is %d x %d, larger than the %d x %d pad" % (path, h, w, PAD[0], PAD[1]))


def png_size(path):
    """(h, w) from the header; nothing is decoded."""
    from PIL import Image
    with Image.open(path) as img:
        return img.size[1], img.size[0]


def _colour_into(loader, path, dst, do_flip, full_res):
    """Decode one frame and crop / pad it into ``dst``, its [Hc,Wc,3] slot of the batch's stack (zero-filled for the pad)."""
    a = loader(path)
    if a.ndim != 3 or a.shape[2] != 3:
        raise RuntimeError("KITTICompletionBatches: %s decoded to shape %s, expected [H,W,3]" % (path, a.shape))
    h, w = a.shape[:2]
    _check_size(path, h, w, full_res)
    canvas, (sy, sx), (dy, dx), (rows, cols) = colour_placement(h, w, do_flip, full_res)
    if tuple(dst.shape[:2]) != canvas:
        raise RuntimeError("KITTICompletionBatches: stack slot %s for canvas %s" % (tuple(dst.shape), canvas))
    dst[dy:dy + rows, dx:dx + cols] = a[sy:sy + rows, sx:sx + cols]


def _depth_into(path, dst):
    """``np.array(Image.open(path), dtype=int)`` (kitti_completion.py:53-58), copied into ``dst``, a 2-D uint16 view of the
    staging buffer planned from the file's header, with the reference's 16-bit assertion."""
    from PIL import Image
    if not os.path.exists(path):
        raise AssertionError("file not found: {}".format(path))
    with Image.open(path) as img:
        a = np.asarray(img)
    if a.ndim != 2 or a.dtype.kind not in "ui":
        raise RuntimeError("KITTICompletionBatches: %s decoded to %s %s, expected a single-channel integer depth map" % (path, a.dtype, a.shape))
    if a.shape != dst.shape:
        raise RuntimeError("KITTICompletionBatches: %s changed size while it was read (%s, planned %s)" % (path, a.shape, dst.shape))
    top = int(a.max())
    if not top > 255:                                            # make sure we have a proper 16bit depth map here.. not 8bit!
        raise AssertionError("np.max(depth_png)={}, path={}".format(top, path))
    if top > 65535 or int(a.min()) < 0:
        raise RuntimeError("KITTICompletionBatches: %s holds values outside 16 bits" % path)
    np.copyto(dst, a, casting="unsafe")


class KITTICompletionBatches(KITTIRAWBatches):
    """See the module docstring.  The first eight arguments are ``KITTICompletion``'s (``data_path`` is the completion tree);
    the others are ``KITTIRAWBatches``'.  The split is ``train`` if ``is_train`` else ``val`` (``val_split`` = "select" / "full"), and
    ``test_completion`` when ``opt.completion_test``.  ``decoder="device"`` is accepted and changes nothing: the colour frames of
    the completion tree are PNG files.  ``png_decoder="device"`` moves the 16-bit depth PNGs of every batch (beam planes, ``depth_gt``,
    ``full_res_4beam``) to ``image_codecs.PngBatchJob``: inflated on the pool, unfiltered by ``fd_png_unfilter`` straight into the planes
    ``fd_depth_png_keys`` reads, every key bit for bit the ``pil`` route's; the reference's 16-bit assertion then costs one small
    download per batch.  The colour frames stay with Pillow either way: their crop, pad and mirror run on the host threads."""

    def __init__(self, data_path, height, width, frame_idxs, num_scales, is_train=False, val_split="select", opt=None, batch_size=1,
                 shuffle=False, seed=0, device="cuda", workers=8, draws=None, loader=None, prefetch=True, drop_last=True,
                 rank=0, world_size=1, decoder="pil", png_decoder="pil"):
        if opt is None:
            raise ValueError("KITTICompletionBatches: opt is required (completion_not_full_res, completion_test, ...)")
        self.full_res = not getattr(opt, "completion_not_full_res", False)
        self.completion_test = bool(getattr(opt, "completion_test", False))
        self.need2channel = getattr(opt, "completion_need2channel", "false") == "true"
        if self.need2channel and not self.full_res:
            raise NotImplementedError("KITTICompletionBatches: completion_need2channel with completion_not_full_res is not covered "
                                      "(the reference's load_4beam_2channel raises there: np.pad of a 3-D array with two pad pairs)")
        self.val_split = val_split
        self.split = "test_completion" if self.completion_test else ("train" if is_train else "val")
        self.paths = completion_paths(data_path, self.split, val_split)
        super().__init__(data_path, self.paths["rgb"], height, width, frame_idxs, num_scales, is_train=is_train, img_ext=".png", opt=opt,
                         batch_size=batch_size, shuffle=shuffle, seed=seed, device=device, workers=workers, draws=draws, loader=loader,
                         prefetch=prefetch, drop_last=drop_last, rank=rank, world_size=world_size, decoder=decoder,
                         png_decoder=png_decoder)
        self.frames = list(self.frame_idxs) if self.is_train else [0]
        self.eval_gdc = bool(self._opt("eval_gdc"))

    def _check_covered(self):
        if "s" in self.frame_idxs:
            raise NotImplementedError("KITTICompletionBatches: the stereo frame 's' is not covered (temporal frames only)")
        if self._opt("inf"):
            raise NotImplementedError("KITTICompletionBatches: the reference's hard-coded --inf demo paths are not covered")

    def check_depth(self):
        return not self.completion_test                          # completion_dataset.py:206

    # ---- host side --------------------------------------------------------------------------------------------------------------
    def plan_batch(self, epoch, indices):
        items = []
        for index in indices:
            rgb, d, gt = self.paths["rgb"][index], self.paths["d"][index], self.paths["gt"][index]
            dr = self.item_draws(epoch, index)
            item = {"index": index, "do_flip": bool(dr["do_flip"]), "jitter": dr["jitter"] if dr["do_color_aug"] else None,
                    "rgb": rgb, "gt": gt if self.load_depth else None, "beams": []}
            if self.is_train:                                    # completion_dataset.py:310-325
                head, tail = os.path.split(rgb)
                frame_index = int(tail[0:tail.find(".")])
                head_d, _ = os.path.split(d)
                item["images"] = [os.path.join(head, "%010d.png" % (frame_index + f)) for f in self.frames]
                item["beams"] = [os.path.join(head_d, "%010d.png" % (frame_index + f)) for f in self.frames]
            else:
                item["images"] = [rgb]
                if self.need_4beam:
                    item["beams"] = [d]
            if self.eval_gdc:                                    # completion_dataset.py:301-306
                item["date"] = rgb.split("/")[-4][:10] if self.is_train else rgb.split("/")[-1][:10]
            items.append(item)
        return items

    def _plan_depth(self, items):
        """Layout of the batch's staging buffer, from the PNG headers alone: the descriptor tables (beam planes frame-major,
        ``depth_gt``, ``full_res_4beam``), then the uint16 planes.  Frame 0's sparse plane serves every key made from it."""
        B = len(items)
        planes, at = {}, 0                                       # path -> (offset in uint16 elements, h, w)

        def plane(path):
            nonlocal at
            if path not in planes:
                if not os.path.exists(path):
                    raise AssertionError("file not found: {}".format(path))
                h, w = png_size(path)
                _check_size(path, h, w, self.full_res)
                planes[path] = (at, h, w)
                at += (h * w + 3) // 4 * 4                       # planes start 8-byte aligned
            return planes[path]

        tables, canvases = {}, {}
        per_item = len(items[0]["beams"])
        if per_item:
            tables["beam"] = []
            for k in range(per_item):                            # frame-major, like the colour keys
                for it in items:
                    off, h, w = plane(it["beams"][k])
                    d, canvases["beam"] = depth_desc(off, h, w, it["do_flip"], self.full_res, not self.full_res)
                    tables["beam"].append(d)
        if self.load_depth:
            tables["gt"] = []
            for it in items:
                off, h, w = plane(it["gt"])
                d, canvases["gt"] = depth_desc(off, h, w, it["do_flip"], self.full_res, not self.full_res)
                tables["gt"].append(d)
        if self.need_4beam and self.eval_gdc:                    # get_depth(paths_d[index], do_flip, pool=False): padding=True
            zero = self.frames.index(0)
            tables["full"] = []
            for it in items:
                off, h, w = plane(it["beams"][zero])
                d, canvases["full"] = depth_desc(off, h, w, it["do_flip"], self.full_res, True)
                tables["full"].append(d)
        plan = {"tables": tables, "canvases": canvases, "planes": planes, "B": B}
        size = ctypes.sizeof(_lib.DepthPngDesc)
        pos = 0
        for name, descs in tables.items():
            plan[name] = (pos, pos + size * len(descs))
            pos = round16(pos + size * len(descs))
        plan["data"] = (pos, pos + 2 * at)
        plan["bytes"] = max(pos + 2 * at, 16)
        return plan

    def _start_depth(self, items, pool):
        plan = self._plan_depth(items)
        if not plan["tables"]:
            return None
        on_device = self.png_decoder == "device"
        size = plan["data"][0] if on_device else plan["bytes"]   # the device route uploads the tables alone from here
        staging = torch.empty((max(size, 16),), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        host = staging.numpy()
        for name, descs in plan["tables"].items():
            host[plan[name][0]:plan[name][1]] = np.frombuffer(data_ops.depth_png_desc_table(descs), dtype=np.uint8)
        plan["staging"] = staging
        if on_device:
            plan["paths"] = list(plan["planes"])
            plan["job"] = image_codecs.PngBatchJob(plan["paths"], pool, mode="gray16")
            plan["futures"] = []
            return plan
        data = host[plan["data"][0]:plan["data"][1]].view(np.uint16)
        plan["futures"] = [pool.submit(_depth_into, path, data[off:off + h * w].reshape(h, w)) for path, (off, h, w) in plan["planes"].items()]
        return plan

    def __iter__(self):
        if self.device.type == "cuda" and not torch.cuda.is_available():
            raise RuntimeError("KITTICompletionBatches builds its batches on the GPU and none is available: there is no CPU path")
        return super().__iter__()

    def _start_host(self, epoch, indices):
        items = self.plan_batch(epoch, indices)
        pool = self._workers()
        canvas = CROP if self.full_res else PAD
        n = len(self.frames) * len(items)
        stack = torch.empty((n, canvas[0], canvas[1], 3), dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        if not self.full_res:
            stack.zero_()
        host = stack.numpy()
        futures = []
        for fi in range(len(self.frames)):                       # frame-major: every key is a contiguous slice of the pyramid
            for b, it in enumerate(items):
                futures.append(pool.submit(_colour_into, self.loader, it["images"][fi], host[fi * len(items) + b], it["do_flip"], self.full_res))
        items[0]["colour_plan"] = {"stack": stack, "futures": futures}
        items[0]["depth_plan"] = self._start_depth(items, pool)
        return items

    # ---- device side ------------------------------------------------------------------------------------------------------------
    def _colour_keys(self, items, batch):
        B = len(items)
        plan = items[0]["colour_plan"]
        for f in plan["futures"]:
            f.result()
        stack = _upload(plan["stack"], self.device)
        flip = [it["do_flip"] for _ in self.frames for it in items]
        jitter = None
        if any(it["jitter"] is not None for it in items):
            jitter = []
            for fi in range(len(self.frames)):
                for it in items:
                    j = it["jitter"]
                    jitter.append(j[fi] if isinstance(j, list) else j)
        pyr = data_ops.image_pyramid(stack, self.height, self.width, self.num_scales, flip, jitter)
        for fi, f in enumerate(self.frames):
            for s in range(self.num_scales):
                for name in ("color", "color_aug"):
                    batch[(name, f, s)] = pyr[(name, s)][fi * B:(fi + 1) * B]

    def _unfilter_depth(self, plan):
        """The device route of the depth planes: the tables are uploaded, ``fd_png_unfilter`` writes the host-order uint16 planes
        at the offsets ``_plan_depth`` chose, and the reference's 16-bit assertion reads one byte per plane back."""
        job = plan["job"]
        job.wait_host()
        table = job.layout()[0]
        for d, path, (h, w) in zip(table, plan["paths"], job.sizes()):
            off, ph, pw = plan["planes"][path]
            if (h, w) != (ph, pw):
                raise RuntimeError("KITTICompletionBatches: %s changed size while it was read (%s, planned %s)" % (path, (h, w), (ph, pw)))
            d.out_off = 2 * off
        lo, hi = plan["data"]
        dev = torch.empty((max(plan["bytes"], 16),), dtype=torch.uint8, device=self.device)
        dev[:lo].copy_(plan["staging"][:lo], non_blocking=True)
        with torch.cuda.device(self.device):
            stats = job.run(self.device, dev[lo:hi], table)
        for name in stats:
            self.decode_stats[name] += stats[name]
        planes = [dev[lo + 2 * off:lo + 2 * (off + h * w)] for off, h, w in (plan["planes"][p] for p in plan["paths"])]
        high = torch.stack([p[1::2].amax() for p in planes]).cpu()              # a 16-bit map has a value above 255
        for path, p, top in zip(plan["paths"], planes, high.tolist()):
            if not top > 0:                                      # make sure we have a proper 16bit depth map here.. not 8bit!
                raise AssertionError("np.max(depth_png)={}, path={}".format(int(p[0::2].amax()), path))
        return dev

    def _depth_keys(self, items, batch):
        """One upload, then ``fd_depth_png_keys`` per key and at most one scatter (module docstring)."""
        plan = items[0]["depth_plan"]
        if plan is None:
            return
        for f in plan["futures"]:
            f.result()                                           # the 16-bit assertion raises here, with the path
        dev = self._unfilter_depth(plan) if "job" in plan else _upload(plan["staging"], self.device)
        B = len(items)
        packed = dev[plan["data"][0]:plan["data"][1]].view(torch.int16)
        pool = 1 if self.full_res else 2

        def keys(name, pool, channels, div1):
            table = dev[plan[name][0]:plan[name][1]]
            return data_ops.depth_png_keys(packed, plan["tables"][name], plan["canvases"][name], pool, channels, 256.0, div1, desc_table=table)

        if "beam" in plan["tables"]:
            zero = self.frames.index(0)
            if self.need2channel:                                # computed online from the mirrored, cropped map / 100
                beams = keys("beam", pool, 1, 100.0)
                two = data_ops.scatter_2channel(beams, SCATTER_ROI, 2)
            else:                                                # torch.stack([d, d]): the kernel writes the map twice
                two = keys("beam", pool, 2, 100.0)
                beams = None
            if self.is_train:
                for fi, f in enumerate(self.frames):
                    batch[("2channel", f, 0)] = two[fi * B:(fi + 1) * B]
            if self.need_4beam:
                z = slice(zero * B, (zero + 1) * B)
                batch["4beam"] = beams[z] if beams is not None else two[z, :1].contiguous()
                batch["2channel"] = two[z]
        if "gt" in plan["tables"]:
            batch["depth_gt"] = keys("gt", 1, 1, 1.0)
        if "full" in plan["tables"]:
            batch["full_res_4beam"] = keys("full", 1, 1, 1.0)

    def _finish_batch(self, items):
        batch = {}
        if self.eval_gdc:
            batch["date"] = [it["date"] for it in items]
        if self._opt("need_path"):
            batch["path"] = [it["rgb"] for it in items]
        self._colour_keys(items, batch)
        if len(items) not in self._K:
            self._K[len(items)] = synthetic.intrinsics(len(items), self.height, self.width, self.num_scales, self.device)
        batch.update(self._K[len(items)])
        self._depth_keys(items, batch)
        return batch
