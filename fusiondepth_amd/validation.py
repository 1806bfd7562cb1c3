"""The trainer's in-training validation metrics on the device: ``compute_depth_losses`` (trainer.py:598-630) plus
``compute_depth_errors`` (layers.py:284-302), per image, against ground-truth maps whose sizes differ from image to image - the
``gt_depths.npz`` of the Eigen split, which the reference's ``val`` indexes per batch (trainer.py:404-405).

  * ``ValGroundTruth(gt_depths)``  packs the maps once, uploads them once and keeps the packed buffer, the descriptor table, the
    workspace and the result buffer on the device for as long as it lives; ``score(depths)`` is then one ``fd_val_scores`` call per
    chunk of 64 images with NOTHING uploaded and nothing read back.
  * ``val_scores(depths, gt)``     the same with one download: ``(per_image[N,7] float64, ratios[N] float32, counts[N] int64)``.
  * ``CompletionGroundTruth`` / ``completion_val_scores`` / ``CompletionValScorer``  the same chain under the Completor's rule
    (``fd_completion_val_scores``; the block at the end of this module).

The rule (include/fdhip.h, fd_val_scores; restated in tests/val_ref.py): mask ``gt > 0`` inside the Garg crop ``153:371, 44:1197``
clipped to the map as slicing clips it; ATen's CPU bilinear rule (``align_corners=False``) resamples the predicted DEPTH to the map's
size at the selected pixels only; clamp to [1e-3, 80]; torch's LOWER medians; ``pred *= med(gt) / med(pred)``; clamp again; the seven
metrics from float32 terms summed in float64 in a fixed order (bitwise reproducible).  Not the rule of ``evaluate_depth.py``
(``evaluate_depth.eigen_scores``): that one resizes the disparity with OpenCV's rule and takes numpy's medians.
No CPU fallback: tensors must live on the GPU.
"""
import numpy as np
import torch

from ._lib import call, query, stream
from .evaluate_depth import EIGEN_DESC

MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0     # trainer.py:607, 622
VAL_CROP = (153, 371, 44, 1197)       # trainer.py:615: the Garg / Eigen crop as fixed indices
CHUNK = 64                            # images per fd_val_scores call


def val_window(H, W, window=None):
    """``[y0:y1, x0:x1]`` of an H x W map as Python slicing clips it -> (y0, y1, x0, x1) with 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W
    (a 128 x 192 map leaves ``153:371`` empty)."""
    y0, y1, x0, x1 = VAL_CROP if window is None else (int(v) for v in window)
    y1, x1 = min(max(y1, 0), H), min(max(x1, 0), W)
    return min(max(y0, 0), y1), y1, min(max(x0, 0), x1), x1


class ValGroundTruth:
    """Ground-truth maps resident on the device for the life of the object: one packed float32 buffer (the maps back to back, each
    behind ``gap`` unused floats - one number, or one per map -), one ``fd_eigen_desc`` table (plane offset, size, prediction index = position in ``gt_depths``, mask
    window), one workspace sized for the largest chunk and one ``[N, 9]`` float64 result buffer.  The 697 maps of the Eigen split
    (375 x 1242 and smaller) are about 1.3 GB of device memory; they are staged through ordinary host memory once, nothing is pinned.
    ``window``: (y0, y1, x0, x1) instead of the Garg crop, clipped to each map the same way.  ``chunk``: images per library call
    (<= 4096); it bounds the workspace (two float32 lists of at most chunk x window area)."""

    ENTRY = "fd_val_scores"                # the entry point and the arguments between list_cap and out: (lo, hi)
    RULE_ARGS = (MIN_DEPTH, MAX_DEPTH)

    def __init__(self, gt_depths, window=None, chunk=CHUNK, device="cuda", gap=0):
        if not torch.cuda.is_available():
            raise RuntimeError("fusiondepth_amd.validation.ValGroundTruth needs an MI355X: there is no CPU path (tests/val_ref.py restates "
                               "the rule for CPU checks)")
        if chunk < 1 or chunk > 4096:
            raise ValueError("ValGroundTruth: chunk must be 1 .. 4096")
        self.desc, total = plan_gt(gt_depths, window, gap)
        self.N, self.chunk = len(self.desc), int(chunk)
        host = np.zeros((max(total, 2),), dtype=np.float32)
        for d, g in zip(self.desc, gt_depths):
            host[d["offset"]:d["offset"] + d["H"] * d["W"]] = np.asarray(g, dtype=np.float32).reshape(-1)
        self.device = torch.device(device)
        self.packed = torch.from_numpy(host).to(self.device)
        self.desc_dev = torch.from_numpy(self.desc.view(np.uint8).copy()).to(self.device)
        rows = (self.desc["y1"] - self.desc["y0"]).astype(np.int64)
        area = rows * (self.desc["x1"] - self.desc["x0"])
        self.chunks, ws_bytes = [], 8
        for a in range(0, self.N, self.chunk):                   # (first, last + 1, max_rows, list_cap) of every call
            b = min(a + self.chunk, self.N)
            c = (a, b, int(rows[a:b].max()), int(area[a:b].sum()))
            self.chunks.append(c)
            ws_bytes = max(ws_bytes, query(self.ENTRY + "_ws_bytes", b - a, c[2], c[3]))
        self.ws = torch.empty((ws_bytes,), device=self.device, dtype=torch.uint8)
        self.out = torch.empty((self.N, 9), device=self.device, dtype=torch.float64)

    def __len__(self):
        return self.N

    def score(self, depths):
        """``depths``: [N,h,w] (or [N,1,h,w]) contiguous float32 device tensor, image i scored against map i.  Returns the resident
        ``[N, 9]`` float64 device tensor ``{abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio, count}``, valid in stream order; it
        is overwritten by the next call.  No host synchronisation, no upload."""
        if depths.dim() == 4 and depths.shape[1] == 1:
            depths = depths[:, 0]
        if not (depths.is_cuda and depths.dtype == torch.float32 and depths.is_contiguous() and depths.dim() == 3):
            raise ValueError("ValGroundTruth.score: depths must be a contiguous float32 [N,h,w] device tensor")
        if depths.shape[0] != self.N:
            raise ValueError("ValGroundTruth.score: %d predictions for %d ground-truth maps" % (depths.shape[0], self.N))
        size = EIGEN_DESC.itemsize
        for a, b, max_rows, cap in self.chunks:                  # the chunks share one workspace: they run in stream order
            call(self.ENTRY, depths.data_ptr(), self.N, depths.shape[1], depths.shape[2], self.packed.data_ptr(), self.packed.numel(),
                 self.desc_dev.data_ptr() + a * size, b - a, max_rows, cap, *self.RULE_ARGS, self.out.data_ptr() + a * 9 * 8,
                 self.ws.data_ptr(), stream())
        return self.out


def plan_gt(gt_depths, window=None, gap=0):
    """The descriptor table of ``ValGroundTruth`` and the packed buffer's length in floats.  ``window``: one (y0, y1, x0, x1) for all
    maps, or one per map.  Pure host code."""
    desc = np.zeros(len(gt_depths), dtype=EIGEN_DESC)
    gaps = [int(gap)] * len(gt_depths) if np.ndim(gap) == 0 else [int(v) for v in gap]
    at = 0
    for i, g in enumerate(gt_depths):
        shape = np.shape(g)
        if len(shape) != 2 or not shape[0] or not shape[1]:
            raise ValueError("ValGroundTruth: ground truth %d has shape %s, expected a non-empty [H,W] map" % (i, shape))
        H, W = int(shape[0]), int(shape[1])
        at += gaps[i]
        desc[i] = (at, H, W, i) + val_window(H, W, window[i] if np.ndim(window) == 2 else window) + (0,)
        at += H * W
    return desc, at


def val_scores(depths, gt, window=None, chunk=CHUNK):
    """trainer.py:598-630 + layers.py:284-302 per image, ``chunk`` images per ``fd_val_scores`` call.  ``depths``: [N,h,w] device
    tensor of predicted depths; ``gt``: a ``ValGroundTruth`` (nothing is uploaded) or N [H_i,W_i] maps (packed and uploaded here).
    Returns ``(per_image[N,7] float64, ratios[N] float32, counts[N] int64)`` after ONE download; a count of -1 marks a descriptor
    that left the buffers."""
    if not isinstance(gt, ValGroundTruth):
        gt = ValGroundTruth(gt, window=window, chunk=chunk, device=depths.device)
    out = gt.score(depths).cpu().numpy()
    return out[:, :7].copy(), out[:, 7].astype(np.float32), out[:, 8].astype(np.int64)



# ---------------------------------------------------------------------------------------------- the Completor's rule
# completor.py:728-762 + layers.py:284-302 (include/fdhip.h, fd_completion_val_scores; restated in tests/completion_val_ref.py): mask
# ``gt > 0.1`` - float32 against float32(0.1), as torch compares a float32 tensor with a Python scalar - over the whole map, or with
# ``--completion_eigen_crop`` inside ``153:371, 44:1197`` clipped as slicing clips it; ATen's CPU bilinear rule on the predicted DEPTH
# at the selected pixels only; clamp to [1e-3, 80]; torch's LOWER medians; ``pred *= med(gt) / med(pred)``; clamp again; both sides
# ``* 1000.0`` (millimetres, one float32 rounding each); the seven metrics from float32 terms summed in float64 in a fixed order.
COMPLETION_GT_MIN = 0.1               # completor.py:741; handed over as a C float: float32(0.1)
WHOLE_MAP = (0, 1 << 30, 0, 1 << 30)  # a window that ``val_window`` clips to every map


def completion_window(eigen_crop):
    return VAL_CROP if eigen_crop else WHOLE_MAP


class CompletionGroundTruth(ValGroundTruth):
    """``ValGroundTruth`` under the Completor's rule (``fd_completion_val_scores``): maps of any sizes, resident, scored in chunks.
    ``window`` overrides the choice ``eigen_crop`` makes."""
    ENTRY = "fd_completion_val_scores"
    RULE_ARGS = (COMPLETION_GT_MIN, MIN_DEPTH, MAX_DEPTH)

    def __init__(self, gt_depths, eigen_crop=False, window=None, chunk=CHUNK, device="cuda", gap=0):
        super().__init__(gt_depths, window=completion_window(eigen_crop) if window is None else window, chunk=chunk, device=device, gap=gap)


def completion_val_scores(depths, gt, eigen_crop=False, window=None, chunk=CHUNK):
    """``val_scores`` under the Completor's rule.  ``gt``: a ``CompletionGroundTruth`` or N [H_i,W_i] maps."""
    if not isinstance(gt, CompletionGroundTruth):
        gt = CompletionGroundTruth(gt, eigen_crop=eigen_crop, window=window, chunk=chunk, device=depths.device)
    out = gt.score(depths).cpu().numpy()
    return out[:, :7].copy(), out[:, 7].astype(np.float32), out[:, 8].astype(np.int64)


class CompletionValScorer:
    """The resident scorer of ``Completor.val_metrics`` for a validation set of ``n_images`` whose maps all have one size: ground
    truth ``gt_size`` = (H, W), predictions ``pred_size`` = (h, w) (equal in full-resolution mode, 192 x 640 against 384 x 1280 with
    ``--completion_not_full_res``).  For the life of the object it holds one staging pair ``[chunk, h, w]`` / ``[chunk, H, W]``, the
    descriptor table of one chunk (uploaded once), one workspace and one ``[n_images, 9]`` float64 result buffer; device memory is
    bounded by the chunk, not by the split (chunk 64 at 352 x 1216: 2 x 64 x 1.7 MB = 220 MB of staging, as much again of workspace).

        scorer.begin()
        for batch: scorer.add(depth[B,1,h,w], depth_gt[B,1,H,W])     # device-to-device copies; ONE library call per full chunk
        rows = scorer.finish()                                       # one more call for the remainder; the [N, 9] device tensor

    Nothing is read back by any of the three: no host synchronisation until the caller downloads ``rows``."""

    def __init__(self, n_images, gt_size, pred_size, eigen_crop=False, chunk=CHUNK, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("fusiondepth_amd.validation.CompletionValScorer needs an MI355X: there is no CPU path "
                               "(tests/completion_val_ref.py restates the rule for CPU checks)")
        if n_images < 1 or chunk < 1 or chunk > 4096:
            raise ValueError("CompletionValScorer: n_images must be positive and chunk 1 .. 4096")
        self.N, self.chunk = int(n_images), min(int(chunk), int(n_images))
        (H, W), (h, w) = (int(v) for v in gt_size), (int(v) for v in pred_size)
        self.gt_size, self.pred_size, self.eigen_crop = (H, W), (h, w), bool(eigen_crop)
        self.desc = plan_gt([np.broadcast_to(np.float32(0), (H, W))] * self.chunk, completion_window(eigen_crop))[0]
        self.max_rows = int(self.desc["y1"][0] - self.desc["y0"][0])
        self.area = self.max_rows * int(self.desc["x1"][0] - self.desc["x0"][0])
        self.device = torch.device(device)
        self.gt = torch.zeros((self.chunk, H, W), device=self.device, dtype=torch.float32)
        self.pred = torch.zeros((self.chunk, h, w), device=self.device, dtype=torch.float32)
        self.desc_dev = torch.from_numpy(self.desc.view(np.uint8).copy()).to(self.device)
        ws_bytes = max(8, query("fd_completion_val_scores_ws_bytes", self.chunk, self.max_rows, self.chunk * self.area))
        self.ws = torch.empty((ws_bytes,), device=self.device, dtype=torch.uint8)
        self.out = torch.empty((self.N, 9), device=self.device, dtype=torch.float64)
        self.calls = 0                                           # library calls since ``begin``
        self.begin()

    def __len__(self):
        return self.N

    def begin(self):
        self.seen, self.filled, self.calls = 0, 0, 0

    def _flush(self):
        k = self.filled
        if not k:
            return
        call("fd_completion_val_scores", self.pred.data_ptr(), self.chunk, self.pred_size[0], self.pred_size[1], self.gt.data_ptr(),
             self.gt.numel(), self.desc_dev.data_ptr(), k, self.max_rows, k * self.area, COMPLETION_GT_MIN, MIN_DEPTH, MAX_DEPTH,
             self.out.data_ptr() + (self.seen - k) * 9 * 8, self.ws.data_ptr(), stream())
        self.filled = 0
        self.calls += 1

    def add(self, depth, depth_gt):
        """``depth`` [B,1,h,w] (or [B,h,w]) and ``depth_gt`` [B,1,H,W] (or [B,H,W]): float32 device tensors of one batch."""
        if depth.dim() == 4:
            depth = depth[:, 0]
        if depth_gt.dim() == 4:
            depth_gt = depth_gt[:, 0]
        if tuple(depth.shape[1:]) != self.pred_size or tuple(depth_gt.shape[1:]) != self.gt_size or depth.shape[0] != depth_gt.shape[0]:
            raise ValueError("CompletionValScorer.add: depth %s / depth_gt %s for a scorer of %s / %s" %
                             (tuple(depth.shape), tuple(depth_gt.shape), self.pred_size, self.gt_size))
        if not (depth.is_cuda and depth_gt.is_cuda and depth.dtype == torch.float32 and depth_gt.dtype == torch.float32):
            raise ValueError("CompletionValScorer.add: float32 device tensors only")
        B, at = depth.shape[0], 0
        if self.seen + B > self.N:
            raise ValueError("CompletionValScorer.add: the loader yields more images than the scorer was built for (%d)" % self.N)
        while at < B:
            k = min(B - at, self.chunk - self.filled)
            self.pred[self.filled:self.filled + k].copy_(depth[at:at + k])
            self.gt[self.filled:self.filled + k].copy_(depth_gt[at:at + k])
            self.filled, self.seen, at = self.filled + k, self.seen + k, at + k
            if self.filled == self.chunk:
                self._flush()

    def finish(self):
        """The remainder's call -> the resident ``[N, 9]`` float64 device tensor ``{abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, ratio,
        count}``, valid in stream order and overwritten by the next round."""
        self._flush()
        if self.seen != self.N:
            raise ValueError("CompletionValScorer.finish: %d images were added for the %d the scorer was built for" % (self.seen, self.N))
        return self.out
