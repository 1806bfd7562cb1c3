"""``evaluate_depth.py --visualize`` on the device (evaluate_depth.py:407-449): the two pictures the reference writes per test image.

  * the disparity picture: ``d' = 1 / pred_depth`` normalised from its minimum to its 95th percentile (``np.percentile`` as numpy 2
    computes it for float32 input, ``mpl.colors.Normalize``) through matplotlib's ``magma`` table;
  * the error picture: ``|pred_depth - gt|`` up to 2 m through a hue ramp at the evaluation mask, 2x2 max-reduced
    (``skimage.measure.block_reduce``), grey 220 where nothing was scored.

``render`` produces both for N maps of different sizes, ``chunk`` of them per ``fd_vis_render`` call (csrc/visualize.hip; at most nine
launches per call whatever the chunk holds); ``colorize_disparity`` is the colour picture alone for a batch of same-size maps, the way
to look at a ``Predictor`` output.  ``magma_lut`` / ``hue_lut`` are the two default tables.

What is pinned and what is not
  * the percentile, the normalisation and the lookup equal numpy 2.2 and matplotlib 3.10 bit for bit (tests/test_visualize_cpu.py
    checks the restatement against both, tests/test_gpu_visualize.py the kernels against the restatement);
  * ``magma_lut()`` is ``trunc(magma(k) * 255)`` of matplotlib, committed below as data: matplotlib is not needed at run time;
  * the DEFAULT ERROR COLOURS ARE NOT OpenCV's BIT FOR BIT.  The reference uses ``cv2.applyColorMap(.., cv2.COLORMAP_HSV)``, a
    64-entry table that OpenCV interpolates to 256; cv2 is not available to this project's build and tests, so that table cannot be
    pinned.  ``hue_lut()`` is the analytic ramp ``round(255 * hsv_to_rgb(k / 256, 1, 1))``.  For the reference's exact colours pass
    ``lut_err=cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_HSV)[:, 0, ::-1]`` (the table, channels reversed from
    OpenCV's BGR to RGB).
No CPU fallback: ``render`` and ``colorize_disparity`` need the GPU; the tables do not.
"""
import colorsys

import numpy as np
import torch

from . import _lib

MAX_CHUNK = 64                                                    # fd_vis_render's limit on N

# (matplotlib.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8), row-major, as hex
_MAGMA_HEX = (
    "00000300000400000601000701010901010b02020d02020f03031104031304041505041706051907051b08061d09071f0a07220b08240c09260d0a280e0a2a0f"
    "0b2c100c2f110c31120d33140d35150e38160e3a170f3c180f3f1a10411b10441c10461e10491f114b20114d2211502311522511552611572811592a115c2b11"
    "5e2d10602f1062301065321067341068350f6a370f6c390f6e3b0f6f3c0f713e0f72400f73420f74430f75450f76470f774810784a10794b10794d117a4f117b"
    "50127b52127c53137c55137d57147d58157e5a157e5b167e5d177e5e177f60187f61187f63197f651a80661a80681b80691c806b1c806c1d806e1e816f1e8171"
    "1f81731f817420817621817721817922817a22817c23817e24817f24818125818225818426818526818727818928818a28818c29808d29808f2a80912a80922b"
    "80942b80952c80972c7f992d7f9a2d7f9c2e7f9e2e7e9f2f7ea12f7ea3307ea4307da6317da7317da9327cab337cac337bae347bb0347bb1357ab3357ab53679"
    "b63679b83778b93778bb3877bd3977be3976c03a75c23a75c33b74c53c74c63c73c83d72ca3e72cb3e71cd3f70ce4070d0416fd1426ed3426dd4436dd6446cd7"
    "456bd9466ada4769dc4869dd4968de4a67e04b66e14c66e24d65e44e64e55063e65162e75262e85461ea5560eb5660ec585fed595fee5b5eee5d5def5e5df060"
    "5df1615cf2635cf3655cf3675bf4685bf56a5bf56c5bf66e5bf6705bf7715bf7735cf8755cf8775cf9795cf97b5df97d5dfa7f5efa805efa825ffb8460fb8660"
    "fb8861fb8a62fc8c63fc8e63fc9064fc9265fc9366fd9567fd9768fd9969fd9b6afd9d6bfd9f6cfda16efda26ffda470fea671fea873feaa74feac75feae76fe"
    "af78feb179feb37bfeb57cfeb77dfeb97ffebb80febc82febe83fec085fec286fec488fec689fec78bfec98dfecb8efdcd90fdcf92fdd193fdd295fdd497fdd6"
    "98fdd89afdda9cfddc9dfddd9ffddfa1fde1a3fce3a5fce5a6fce6a8fce8aafceaacfcecaefceeb0fcf0b1fcf1b3fcf3b5fcf5b7fbf7b9fbf9bbfbfabdfbfcbf")


def magma_lut():
    """matplotlib's ``magma`` as the reference's ``(rgba * 255).astype(np.uint8)`` turns it into bytes -> [256,3] uint8, RGB."""
    return np.frombuffer(bytes.fromhex(_MAGMA_HEX), dtype=np.uint8).reshape(256, 3).copy()


def hue_lut():
    """The default error table: ``round(255 * hsv_to_rgb(k / 256, 1, 1))`` -> [256,3] uint8, RGB (red at 0, through yellow, green at
    about 85: entries 0 .. 80 are the ones the error picture uses).  NOT OpenCV's ``COLORMAP_HSV`` bit for bit (module docstring)."""
    return np.rint(255.0 * np.array([colorsys.hsv_to_rgb(k / 256.0, 1.0, 1.0) for k in range(256)])).astype(np.uint8)


def _table(lut, default, name, who):
    t = default() if lut is None else np.asarray(lut)
    if t.shape != (256, 3) or t.dtype != np.uint8:
        raise ValueError("%s: %s must be a [256,3] uint8 table, got %s %s" % (who, name, t.dtype, t.shape))
    return np.ascontiguousarray(t)


def err_size(H, W):
    """The size of the error picture of an H x W map: ``block_reduce`` pads an odd edge."""
    return (int(H) + 1) // 2, (int(W) + 1) // 2


def _call(disp, ratio_d, depth_in, packed_d, desc_d, desc, total, gt_lo, gt_hi, scale, lut_disp_d, lut_err_d, color, err, err_pixels,
          stats, depth_out):
    """One ``fd_vis_render`` call; every tensor lives on the device, an absent one is None."""
    n = len(desc)
    dev = desc_d.device
    ws = torch.empty((max(_lib.query("fd_vis_render_ws_bytes", n, total), 16),), device=dev, dtype=torch.uint8)
    p = lambda t: None if t is None else t.data_ptr()
    M, h, w = (0, 0, 0) if disp is None else disp.shape
    _lib.call("fd_vis_render", p(disp), M, h, w, float(scale), p(ratio_d), p(depth_in), p(packed_d), total, desc_d.data_ptr(), n,
              int((desc["H"].astype(np.int64) * desc["W"]).max()), float(gt_lo), float(gt_hi), p(lut_disp_d), p(lut_err_d), p(color), p(err),
              int(err_pixels), p(stats), p(depth_out), ws.data_ptr(), _lib.stream())


def render(pred_disps, gt_depths, ratios=None, eval_split="eigen", pred_depth_scale_factor=1.0, depths=None, lut_disp=None, lut_err=None,
           want_stats=False, want_depth=False, chunk=64):
    """evaluate_depth.py:407-449 for N images, ``chunk`` (<= 64) of them per ``fd_vis_render`` call.
    ``pred_disps``: [N,h,w] device tensor or host array (float64 is rounded to float32 once); the depth of image i is formed as
    ``depth_export`` forms it: resized to the size of ``gt_depths[i]`` by OpenCV's float32 INTER_LINEAR rule, ``1 / .``,
    ``* pred_depth_scale_factor``, ``* ratios[i]`` (the scorer's ratios, when given).  ``depths``: instead of ``pred_disps`` (pass None
    for it), N dense [H_i,W_i] maps that are drawn as they are - the maps GDC returns, rounded to float32 once.  ``gt_depths``: N
    [H_i,W_i] ground-truth maps; the error picture is drawn at the pixels ``eval_split`` scores (``split_window`` / ``split_bounds``).
    ``lut_disp`` / ``lut_err``: [256,3] uint8 RGB tables, default ``magma_lut()`` / ``hue_lut()`` (the latter is not OpenCV's
    ``COLORMAP_HSV`` bit for bit; build that one with ``cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_HSV)`` and
    reverse its channels to RGB).
    Returns ``(colors, errors)``: lists of N uint8 arrays [H_i,W_i,3] and [ceil(H_i/2),ceil(W_i/2),3], views into one pinned download
    per chunk; then, with ``want_stats``, a float32 [N,2] array of (vmin, vmax) and, with ``want_depth``, the list of N float32 depth
    maps as device tensors."""
    from .evaluate_depth import pack_gt_depths, split_bounds
    who = "render"
    if not torch.cuda.is_available():
        raise RuntimeError("fusiondepth_amd.visualize.render needs an MI355X: there is no CPU path (tests/visualize_ref.py restates it)")
    N = len(gt_depths)
    if (pred_disps is None) == (depths is None):
        raise ValueError("render: give pred_disps or depths, not both")
    source = pred_disps if depths is None else depths
    if len(source) != N:
        raise ValueError("render: %d maps for %d ground-truth maps" % (len(source), N))
    if chunk < 1 or chunk > MAX_CHUNK:
        raise ValueError("render: chunk must be 1 .. %d" % MAX_CHUNK)
    if ratios is not None:
        ratios = np.ascontiguousarray(np.asarray(ratios, dtype=np.float32).reshape(-1))
        if depths is not None:
            raise ValueError("render: ratios go with pred_disps; depths are drawn as they are")
        if ratios.size != N:
            raise ValueError("render: %d ratios for %d maps" % (ratios.size, N))
    lut_disp, lut_err = _table(lut_disp, magma_lut, "lut_disp", who), _table(lut_err, hue_lut, "lut_err", who)
    gt_lo, gt_hi = split_bounds(eval_split)
    colors, errors, stats_rows, depth_maps = [], [], [], []
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        packed, desc = pack_gt_depths(gt_depths[a:b], eval_split)  # refuses an empty or non-2-D map
        total = int(packed.numel())
        disp = depth_in = None
        if depths is None:
            disp = pred_disps[a:b]
            disp = disp if torch.is_tensor(disp) else torch.as_tensor(np.asarray(disp))
            disp = _lib.f32(disp).cuda()
            if disp.dim() != 3:
                raise ValueError("render: pred_disps must be [N,h,w], got %s" % (tuple(disp.shape),))
            dev = disp.device
        else:
            planes = []
            for i, (m, d) in enumerate(zip(depths[a:b], desc)):
                m = m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m))
                if tuple(m.shape) != (int(d["H"]), int(d["W"])):
                    raise ValueError("render: depth map %d has shape %s, its ground truth is %s" % (a + i, tuple(m.shape), (int(d["H"]), int(d["W"]))))
                planes.append(m.detach().to(device="cuda", dtype=torch.float32).reshape(-1))
            depth_in = torch.cat(planes)
            dev = depth_in.device
        packed_d = packed.to(dev, non_blocking=True)
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        ratio_d = None if ratios is None else torch.from_numpy(ratios[a:b].copy()).to(dev)
        luts = torch.from_numpy(np.concatenate([lut_disp, lut_err])).to(dev)
        sizes = [err_size(d["H"], d["W"]) for d in desc]
        err_pixels = sum(h2 * w2 for h2, w2 in sizes)
        out = torch.empty((3 * total + 3 * err_pixels,), device=dev, dtype=torch.uint8)       # colour, then error: one download
        stats = torch.empty((b - a, 2), device=dev, dtype=torch.float32) if want_stats else None
        depth = torch.empty((total,), device=dev, dtype=torch.float32) if want_depth else None
        _call(disp, ratio_d, depth_in, packed_d, desc_d, desc, total, gt_lo, gt_hi, pred_depth_scale_factor, luts[:256], luts[256:],
              out[:3 * total], out[3 * total:], err_pixels, stats, depth)
        host = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(out)                                          # synchronises: the uploads are free to go afterwards
        flat = host.numpy()                                      # keeps the pinned tensor alive
        at = 3 * total
        for d, (h2, w2) in zip(desc, sizes):
            o, H, W = 3 * int(d["offset"]), int(d["H"]), int(d["W"])
            colors.append(flat[o:o + 3 * H * W].reshape(H, W, 3))
            errors.append(flat[at:at + 3 * h2 * w2].reshape(h2, w2, 3))
            at += 3 * h2 * w2
            if want_depth:
                depth_maps.append(depth[int(d["offset"]):int(d["offset"]) + H * W].view(H, W))
        if want_stats:
            stats_rows.append(stats.cpu().numpy())
    result = (colors, errors)
    if want_stats:
        result += (np.concatenate(stats_rows) if stats_rows else np.zeros((0, 2), np.float32),)
    if want_depth:
        result += (depth_maps,)
    return result


def colorize_disparity(disp, lut=None):
    """The colour picture of ``render`` for a batch of same-size maps, on the device: [B,H,W] or [B,1,H,W] disparities (a ``Predictor``
    output) -> uint8 [B,H,W,3], every map normalised from its own minimum to its own 95th percentile through ``lut`` (default
    ``magma_lut()``).  The same kernels as ``render`` with the colour output alone, at the map's own size (the resize is then the
    identity); the value drawn is ``1 / (1 / disp)`` in float32, as in the script's pictures."""
    _lib._need_cuda(disp)
    if disp.dim() == 4 and disp.shape[1] == 1:
        disp = disp[:, 0]
    if disp.dim() != 3 or not disp.numel():
        raise ValueError("colorize_disparity: expected non-empty [B,H,W] or [B,1,H,W] disparities, got %s" % (tuple(disp.shape),))
    from .evaluate_depth import EIGEN_DESC
    disp = _lib.f32(disp.detach())
    B, H, W = disp.shape
    lut_d = torch.from_numpy(_table(lut, magma_lut, "lut", "colorize_disparity")).to(disp.device)
    out = torch.empty((B, H, W, 3), device=disp.device, dtype=torch.uint8)
    for a in range(0, B, MAX_CHUNK):
        n = min(MAX_CHUNK, B - a)
        desc = np.zeros(n, dtype=EIGEN_DESC)
        for i in range(n):
            desc[i] = (i * H * W, H, W, i, 0, H, 0, W, 0)
        desc_d = torch.from_numpy(desc.view(np.uint8).copy()).to(disp.device)
        _call(disp[a:a + n], None, None, None, desc_d, desc, n * H * W, 0.0, float("inf"), 1.0, lut_d, None, out[a:a + n], None, 0, None,
              None)
    return out
