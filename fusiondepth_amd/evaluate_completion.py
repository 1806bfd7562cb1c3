"""The reference's ``evaluate_completion.py`` on the device: RMSE / MAE in mm and iRMSE / iMAE in 1/km of predicted depth maps
against KITTI depth-completion ground truth.

  * ``compute_errors(gt, pred)``                 evaluate_completion.py:31-48 (fd_completion_errors)
  * ``evaluate_completion_predictions(...)``     the per-image loop of ``evaluate`` (:297-355): ``pred_depth_scale_factor``, median
    scaling with numpy's median (fd_completion_medians: radix select per image, no sort), optional GDC (--eval_gdc, gdc.py) between the
    two kernels, clamp to [1e-3, 80], the four metrics per image (float32 element arithmetic as numpy does it, float64 sums in a fixed
    order: bitwise reproducible) and their mean.
  * ``predict_depths(predictor, batch, opt)``    :141-224: disparity -> depth, bilinear to 352x1216 (384x1280 with
    ``--completion_not_full_res``), clamp, ``--post_process``.
  * ``evaluate(opt)`` / ``python -m fusiondepth_amd.evaluate_completion``: the script, on ``Predictor`` and ``KITTICompletionBatches``.

Deviations from the reference, on purpose
  * its ``evaluate`` pairs prediction i with ``gt_depths[i][0][0]``, the first item of BATCH i - right only at ``--eval_batch_size 1``.
    Here every image meets its own ground truth.
  * with ``--completion_test`` it writes ``(pred * 256).astype(uint16)`` PNGs with cv2 to a fixed relative folder; here with PIL to
    ``--eval_out_dir`` (default ``<data_path>/completion/test_result``).  It then scores against ``4beam * 100``; so does this.
  * with ``--completion_test`` and ``--completion_not_full_res`` its ``4beam * 100`` is the pooled 192x640 map while the predictions are
    384x1280, and its boolean indexing fails; here the score is taken against ``full_res_4beam``, the same sparse map at 384x1280.
  * ``--post_process`` feeds the mirrored colour image next to the UNMIRRORED 2-channel map to the beam encoder (and a batch of B maps
    next to 2 B images); here the second pass gets the mirrored map.
  * configurations ``Predictor`` does not cover raise: ``--refine_2d``, a model without the beam encoder.
No CPU fallback: tensors must live on the GPU.
"""
import os
import sys

import numpy as np
import torch

from ._lib import _need_cuda, call, f32, query, stream

MIN_DEPTH = 1e-3          # evaluate_completion.py:65-66
MAX_DEPTH = 80
GT_MIN = 0.1              # :305
GDC_ARGS = dict(W_tol=3e-5, recon_tol=5e-4, consider_range=(-3, 9), k=10, method="cg")      # :331-332


def _planes(pred, gt, who):
    pred, gt = torch.as_tensor(pred), torch.as_tensor(gt)
    _need_cuda(pred, gt)
    pred, gt = f32(pred), f32(gt)
    if pred.dim() == 2:
        pred, gt = pred[None], gt[None]
    if pred.dim() != 3 or pred.shape != gt.shape or not pred.numel():
        raise ValueError("%s: pred %s and gt %s must be matching non-empty [N,H,W] maps" % (who, tuple(pred.shape), tuple(gt.shape)))
    return pred, gt


def completion_medians(pred, gt, gt_min=GT_MIN, pred_scale=1.0):
    """Per image of ``pred`` / ``gt`` [N,H,W], over ``gt > gt_min``: float32 [N,4] = (median(gt) / median(pred * pred_scale),
    median(gt), median(pred * pred_scale), count) with numpy's medians (fd_completion_medians)."""
    pred, gt = _planes(pred, gt, "completion_medians")
    N, H, W = pred.shape
    out = torch.empty((N, 4), device=pred.device, dtype=torch.float32)
    call("fd_completion_medians", pred.data_ptr(), gt.data_ptr(), N, H, W, float(gt_min), float(pred_scale), out.data_ptr(), None, stream())
    return out


def completion_errors(pred, gt, ratio=None, gt_min=GT_MIN, pred_scale=1.0, lo=MIN_DEPTH, hi=MAX_DEPTH):
    """Per image, over ``gt > gt_min``: float64 [N,5] = (rmse, mae, irmse, imae, count) of clamp(pred * pred_scale * ratio[n], lo, hi)
    against gt (fd_completion_errors).  ``ratio``: float32 [N] device tensor or None."""
    pred, gt = _planes(pred, gt, "completion_errors")
    N, H, W = pred.shape
    if ratio is not None:
        _need_cuda(ratio)
        if ratio.dtype != torch.float32 or ratio.numel() != N or not ratio.is_contiguous():
            raise ValueError("completion_errors: ratio must be a contiguous float32 tensor of %d values" % N)
    ws = torch.empty((max(query("fd_completion_ws_bytes", N, H, W), 8),), device=pred.device, dtype=torch.uint8)
    out = torch.empty((N, 5), device=pred.device, dtype=torch.float64)
    call("fd_completion_errors", pred.data_ptr(), gt.data_ptr(), ratio.data_ptr() if ratio is not None else None, N, H, W, float(gt_min),
         float(pred_scale), float(lo), float(hi), out.data_ptr(), ws.data_ptr(), stream())
    return out


def compute_errors(gt, pred):
    """evaluate_completion.py:31-48 on matched (already selected and clamped) device tensors -> (rmse, mae, irmse, imae) as floats."""
    gt, pred = torch.as_tensor(gt), torch.as_tensor(pred)
    _need_cuda(gt, pred)
    inf = float("inf")
    out = completion_errors(pred.reshape(1, 1, -1), gt.reshape(1, 1, -1), None, -inf, 1.0, -inf, inf)
    return tuple(float(v) for v in out[0, :4].cpu())


def evaluate_completion_predictions(pred_depths, gt_depths, pred_depth_scale_factor=1.0, disable_median_scaling=False, eval_gdc=False,
                                    beam_depths=None, calibs=None, return_maps=False):
    """evaluate_completion.py:297-362.  ``pred_depths`` / ``gt_depths``: [N,H,W] (or [N,1,H,W]) device tensors, metres.  Returns
    ``(mean[4], ratios[N], per_image[N,4])`` as numpy arrays: (rmse, mae, irmse, imae), the median-scaling ratios (empty when
    ``disable_median_scaling``).  ``eval_gdc``: after scaling, each prediction is corrected with GDC against ``beam_depths[i]`` (the
    sparse map at the same size in metres, 0 = no point) and ``calibs[i]`` with the reference's arguments here (``GDC_ARGS``); an
    image whose correction raises is scored uncorrected after a "GDC failed" line, as the reference does.  ``return_maps`` adds a fourth
    value: the [N,H,W] float32 device tensor that was scored, before the clamp - scaled, and corrected where ``eval_gdc`` (what
    ``--completion_test`` writes to disk)."""
    squeeze = lambda t: t[:, 0] if torch.is_tensor(t) and t.dim() == 4 else t
    pred, gt = _planes(squeeze(pred_depths), squeeze(gt_depths), "evaluate_completion_predictions")
    N = pred.shape[0]
    scale = float(pred_depth_scale_factor)
    ratio = None
    if not disable_median_scaling:
        ratio = completion_medians(pred, gt, GT_MIN, scale)[:, 0].contiguous()
    if eval_gdc and (beam_depths is None or calibs is None):
        raise ValueError("evaluate_completion_predictions: eval_gdc needs beam_depths and calibs")
    maps = None
    if eval_gdc or return_maps:
        maps = pred * np.float32(scale)                          # the reference's two in-place float32 products, in its order
        if ratio is not None:
            maps = maps * ratio[:, None, None]
    if eval_gdc:
        from .gdc import GDC
        beams = squeeze(beam_depths)
        corrected = []
        for i in range(N):
            try:
                gtd = torch.as_tensor(beams[i], dtype=torch.float64).to(pred.device).clone()
                gtd[gtd == 0] = -1
                corrected.append(GDC(maps[i], gtd, calibs[i], idx=i, **GDC_ARGS))
            except Exception:                                    # evaluate_completion.py:334-335
                print("GDC failed")
                corrected.append(maps[i])
        maps = torch.stack(corrected)
        out = completion_errors(maps, gt, None, GT_MIN, 1.0)
    else:
        out = completion_errors(pred, gt, ratio, GT_MIN, scale)
    per_image = out[:, :4].cpu().numpy()
    ratios = ratio.cpu().numpy() if ratio is not None else np.zeros((0,), np.float32)
    result = (per_image.mean(0), ratios, per_image)
    return result + (maps,) if return_maps else result


def canvas_size(opt):
    return (384, 1280) if getattr(opt, "completion_not_full_res", False) else (352, 1216)


def predict_depths(predictor, batch, opt):
    """evaluate_completion.py:154-222 for one batch -> [B,H,W] float32 device tensor of depths at the ground-truth size."""
    from . import functional as FD
    from .evaluate_depth import batch_post_process_disparity
    B = batch["color", 0, 0].shape[0]
    if getattr(opt, "post_process", False):                      # two passes per image, the second mirrored
        batch = {("color_aug", 0, 0): torch.cat((batch["color", 0, 0], torch.flip(batch["color", 0, 0], [3])), 0),
                 "2channel": torch.cat((batch["2channel"], torch.flip(batch["2channel"], [3])), 0)}
    else:
        batch = {("color_aug", 0, 0): batch["color", 0, 0], "2channel": batch["2channel"]}
    disp = predictor.predict(batch)[("disp", 0)]
    _, depth = FD.disp_to_depth(disp, opt.min_depth, opt.max_depth)
    H, W = canvas_size(opt)
    if tuple(depth.shape[2:]) != (H, W):
        depth = FD.bilinear_upsample(depth, (H, W)) if H >= depth.shape[2] and W >= depth.shape[3] else \
            torch.nn.functional.interpolate(depth, [H, W], mode="bilinear", align_corners=False)
    depth = torch.clamp(depth, MIN_DEPTH, MAX_DEPTH)[:, 0]
    if getattr(opt, "post_process", False):
        pred_disp = 1 / depth
        pred_disp = batch_post_process_disparity(pred_disp[:B].contiguous(), torch.flip(pred_disp[B:], [2]).contiguous())
        depth = (1 / pred_disp).float()
    return depth


def _calibration(data_path, date):
    from . import kitti_utils
    return kitti_utils.Calibration(os.path.join(data_path, date, "calib_cam_to_cam.txt"))


def evaluate(opt):
    """evaluate_completion.py:62-366: predictions of a saved model over the completion validation (or, ``--completion_test``, test)
    split, scored.  Returns ``(mean[4], ratios, per_image)``."""
    from .completion_data import KITTICompletionBatches
    from .predict import Predictor
    if not opt.completion_not_full_res:
        opt.height, opt.width = 352, 1216
    if sum((bool(opt.eval_mono), bool(opt.eval_stereo))) != 1:
        raise ValueError("Please choose mono or stereo evaluation by setting either --eval_mono or --eval_stereo")
    if opt.ext_disp_to_eval is not None:
        raise NotImplementedError("evaluate_completion: --ext_disp_to_eval is not covered (the reference leaves pred_depths undefined there)")
    if opt.refine_2d:
        raise NotImplementedError("evaluate_completion: --refine_2d is not covered (Predictor runs encoder, beam encoder and depth decoder)")
    if not opt.beam_encoder:
        raise NotImplementedError("evaluate_completion: a model without the beam encoder is not covered (Predictor always runs it)")
    if opt.load_weights_folder is None:
        raise ValueError("evaluate_completion: --load_weights_folder is required")
    folder = os.path.expanduser(opt.load_weights_folder)
    print("-> Loading weights from {}".format(folder))
    predictor = Predictor(folder, num_layers=opt.num_layers, scales=tuple(opt.scales), cat_4beam_to_color=opt.cat_4beam_to_color,
                          cat2start=opt.cat2start, cat2end=opt.cat2end)
    enc = torch.load(os.path.join(folder, "encoder.pth"), map_location="cpu")
    height, width = int(enc.get("height", opt.height)), int(enc.get("width", opt.width))
    if opt.eval_gdc:
        opt.eval_batch_size = 1
    opt.need_4beam = True                                        # the model input; the reference's script needs the flag set too
    # --completion_test with --completion_not_full_res: "4beam" is the pooled 192x640 map there, the predictions are 384x1280, so the
    # sparse map is asked for at full size too (the key the loader otherwise builds for --eval_gdc only)
    test_full = bool(opt.completion_test and opt.completion_not_full_res)
    loader_opt = opt
    if test_full and not opt.eval_gdc:
        import copy
        loader_opt = copy.copy(opt)
        loader_opt.eval_gdc = True
    loader = KITTICompletionBatches(os.path.join(opt.data_path, "completion"), height, width, [0], 4, is_train=False,
                                    val_split=opt.completion_val_split, opt=loader_opt, batch_size=opt.eval_batch_size, drop_last=False)
    print("-> Computing predictions with size {}x{}".format(width, height))
    preds, gts, beams, dates = [], [], [], []
    for batch in loader:
        preds.append(predict_depths(predictor, batch, opt))
        if opt.completion_test:
            gts.append(batch["full_res_4beam"][:, 0] if test_full else batch["4beam"][:, 0] * 100.0)
        else:
            gts.append(batch["depth_gt"][:, 0])
        if opt.eval_gdc:
            dates += batch["date"]
            beams.append(batch["full_res_4beam"][:, 0] if opt.completion_not_full_res else batch["4beam"][:, 0] * 100.0)
    loader.close()
    pred, gt = torch.cat(preds), torch.cat(gts)
    print("-> Evaluating")
    if opt.eval_stereo:
        print("   Stereo evaluation - disabling median scaling, scaling by 5.4")
        opt.disable_median_scaling = True
        opt.pred_depth_scale_factor = 5.4
    else:
        print("   Mono evaluation - using median scaling")
    calibs = [_calibration(opt.data_path, d) for d in dates] if opt.eval_gdc else None
    mean, ratios, per_image, maps = evaluate_completion_predictions(pred, gt, opt.pred_depth_scale_factor, opt.disable_median_scaling,
                                                                    opt.eval_gdc, torch.cat(beams) if opt.eval_gdc else None, calibs,
                                                                    return_maps=True)
    if opt.completion_test:                                      # :340-345: the maps as scored - scaled, GDC-corrected - before the clamp
        from PIL import Image
        out_dir = opt.eval_out_dir or os.path.join(opt.data_path, "completion", "test_result")
        os.makedirs(out_dir, exist_ok=True)
        for i, p in enumerate((maps * 256.0).cpu().numpy().astype(np.uint16)):
            Image.fromarray(p).save(os.path.join(out_dir, "{:010d}.png".format(i)))
        print("-> Saved {} predictions to {}".format(len(maps), out_dir))
    if not opt.disable_median_scaling:
        med = np.median(ratios)
        print(" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)))
    print("\n  " + ("{:>8} | " * 4).format("rmse", "mae", "irmse", "imae"))
    print(("&{: 8.3f}  " * 4).format(*mean.tolist()) + "\\\\")
    print("\n-> Done!")
    return mean, ratios, per_image


def main(argv=None):
    from .options import MonodepthOptions
    options = MonodepthOptions()
    evaluate(options.parse(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
