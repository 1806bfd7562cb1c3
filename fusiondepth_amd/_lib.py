"""ctypes binding of ``libfdhip.so`` (C ABI declared in ``include/fdhip.h``).

There is no CPU fallback: every op in this package goes through this library and raises if it is not
built (``python -m fusiondepth_amd.build``) or if a tensor is not a contiguous float32 CUDA tensor.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FD_LIBFDHIP") or os.path.join(_HERE, "libfdhip.so")   # FD_LIBFDHIP: another build of the library, for a same-box A/B
ABI_VERSION = 8
PHOTO_OUT_FLOATS = 96        # FD_PHOTO_OUT_FLOATS

_P, _I, _L, _F, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double
_KIND = {"p": _P, "i": _I, "l": _L, "f": _F, "d": _D}


class PhotoCfg(ctypes.Structure):
    """Mirror of ``fd_photo_cfg``."""
    _fields_ = [("min_depth", _D), ("max_depth", _D),
                ("B", _I), ("H", _I), ("W", _I), ("Hs", _I), ("Ws", _I), ("NF", _I),
                ("use_ssim", _I), ("avg_reprojection", _I),
                ("si_depth_scale", _F), ("si_beam_scale", _F), ("si_threshold", _F), ("si_var", _F), ("eps", _F),
                ("groups", _I), ("si_lo", _F), ("si_mode", _I)]


class PhotoMsCfg(ctypes.Structure):
    """Mirror of ``fd_photo_ms_cfg``."""
    _fields_ = [("base", PhotoCfg), ("n_scales", _I), ("Hs", _I * 4), ("Ws", _I * 4), ("beam_mask", ctypes.c_uint),
                ("rows_per_strip", _I)]


class RefineCfg(ctypes.Structure):
    """Mirror of ``fd_refine_cfg``."""
    _fields_ = [("B", _I), ("H", _I), ("W", _I), ("n_scales", _I), ("Hs", _I * 4), ("Ws", _I * 4),
                ("crop_y0", _I), ("crop_y1", _I), ("crop_x0", _I), ("crop_x1", _I), ("min_depth", _D), ("max_depth", _D),
                ("catxy", _I), ("pool_disp0", _I)]


class ConvDesc(ctypes.Structure):
    """Mirror of ``fd_conv_desc``."""
    _fields_ = [(n, _I) for n in ("N", "Cin", "H", "W", "Cout", "KH", "KW", "stride", "pad", "pad_mode", "act", "in_norm")]


class JitterDesc(ctypes.Structure):
    """Mirror of ``fd_jitter_desc``."""
    _fields_ = [("src_off", _L), ("u8_off", _L), ("planes_off", _L), ("plain_off", _L), ("H", _I), ("W", _I), ("factor", _F * 4),
                ("order", _I * 4), ("n_ops", _I), ("hue_shift", _I)]


class SparsifyCfg(ctypes.Structure):
    """Mirror of ``fd_sparsify_cfg``."""
    _fields_ = [("S", _I), ("H", _I), ("W", _I), ("n_rows", _I), ("rows", _I * 64),
                ("x_lo", _F), ("x_hi", _F), ("y_lo", _F), ("y_hi", _F), ("z_lo", _F), ("z_hi", _F),
                ("random_sample", _I), ("reserved", _I), ("seed", ctypes.c_ulonglong)]


class RasterDesc(ctypes.Structure):
    """Mirror of ``fd_raster_desc``."""
    _fields_ = [("P", _D * 12), ("im_h", _I), ("im_w", _I), ("flip", _I), ("reserved", _I)]


class ResizeDesc(ctypes.Structure):
    """Mirror of ``fd_resize_desc``."""
    _fields_ = [("offset", _L), ("h_in", _I), ("w_in", _I), ("mirror", _I), ("reserved", _I)]


class DepthPngDesc(ctypes.Structure):
    """Mirror of ``fd_depth_png_desc``."""
    _fields_ = [("offset", _L)] + [(n, _I) for n in ("h", "w", "mirror", "src_y", "src_x", "win_y", "win_x", "win_h", "win_w", "reserved")]


class EigenDesc(ctypes.Structure):
    """Mirror of ``fd_eigen_desc``."""
    _fields_ = [("offset", _L)] + [(n, _I) for n in ("H", "W", "pred", "y0", "y1", "x0", "x1", "reserved")]


class ExportDesc(ctypes.Structure):
    """Mirror of ``fd_export_desc``."""
    _fields_ = [("offset", _L), ("H", _I), ("W", _I), ("pred", _I), ("reserved", _I)]


class PointsCalib(ctypes.Structure):
    """Mirror of ``fd_points_calib``."""
    _fields_ = [(n, _D) for n in ("c_u", "c_v", "f_u", "f_v", "b_x", "b_y")] + [("A", _D * 9), ("t", _D * 3)]


assert ctypes.sizeof(PointsCalib) == 144


class RelayoutJob(ctypes.Structure):
    """Mirror of ``fd_relayout_job``."""
    _fields_ = ([("w", ctypes.c_void_p), ("dst", ctypes.c_void_p)] +
                [(n, _I) for n in ("Co", "Ci", "KH", "KW", "TA", "TB", "kh0", "dkh", "kw0", "dkw", "mode", "reserved")] +
                [("n", ctypes.c_long), ("first_block", ctypes.c_long)])


class LogTile(ctypes.Structure):
    """Mirror of ``fd_log_tile``."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("p0", "p1", "p2", "p3", "p4")] + \
               [(n, _I) for n in ("kind", "y", "x", "h", "w", "aux", "slot", "reserved")]


class JpegInfo(ctypes.Structure):
    """Mirror of ``fd_jpeg_info``."""
    _fields_ = [(n, _I) for n in ("width", "height", "components", "h_samp", "v_samp", "covered")] + \
               [("blocks_w", _I * 3), ("blocks_h", _I * 3), ("restart_interval", _I), ("reserved", _I), ("coef_count", _L)]


class JpegDesc(ctypes.Structure):
    """Mirror of ``fd_jpeg_desc``."""
    _fields_ = [(n, _L) for n in ("coef_off", "qt_off", "plane_off", "out_off")] + \
               [(n, _I) for n in ("kind", "width", "height", "components", "h_samp", "v_samp")] + [("reserved", _I * 2)]


assert ctypes.sizeof(JpegInfo) == 64 and ctypes.sizeof(JpegDesc) == 64


class PngInfo(ctypes.Structure):
    """Mirror of ``fd_png_info``."""
    _fields_ = [(n, _I) for n in ("width", "height", "bit_depth", "colour_type", "interlace", "covered", "bpp", "reserved")] + \
               [("row_bytes", _L), ("raw_bytes", _L), ("reserved2", _L * 2)]


class PngDesc(ctypes.Structure):
    """Mirror of ``fd_png_desc``."""
    _fields_ = [("raw_off", _L), ("out_off", _L)] + [(n, _I) for n in ("kind", "width", "height", "bpp", "mode")] + [("reserved", _I * 3)]


assert ctypes.sizeof(PngInfo) == 64 and ctypes.sizeof(PngDesc) == 48


class PngEncDesc(ctypes.Structure):
    """Mirror of ``fd_png_enc_desc``."""
    _fields_ = [("src", ctypes.c_void_p)] + [(n, _L) for n in ("ws_off", "out_off", "out_bytes", "stream_bits")] + \
               [(n, _I) for n in ("width", "height", "bpp", "first_row", "first_block", "first_group")] + \
               [("adler", ctypes.c_uint), ("reserved", _I * 3)]


class PngEncSizes(ctypes.Structure):
    """Mirror of ``fd_png_enc_sizes``."""
    _fields_ = [(n, _L) for n in ("rows", "blocks", "groups", "raw_bytes", "stat_off", "stat_bytes", "rowbits_off", "table_off", "ws_off",
                                  "work_bytes")]


class PngEncBlock(ctypes.Structure):
    """Mirror of ``fd_png_enc_block``."""
    _fields_ = [("bit_off", ctypes.c_ulonglong), ("bits", ctypes.c_ulonglong), ("header_bits", ctypes.c_uint), ("dist_len", ctypes.c_uint),
                ("header", ctypes.c_uint * 128), ("code", ctypes.c_ushort * 288), ("len", ctypes.c_ubyte * 288), ("reserved", ctypes.c_uint * 2)]


assert ctypes.sizeof(PngEncDesc) == 80 and ctypes.sizeof(PngEncSizes) == 80 and ctypes.sizeof(PngEncBlock) == 1408


class JpegEncDesc(ctypes.Structure):
    """Mirror of ``fd_jpeg_enc_desc``."""
    _fields_ = [("src", ctypes.c_void_p)] + [(n, _L) for n in ("first_block", "blocks", "raw_off", "raw_cap", "first_tile", "out_cap")] + \
               [(n, _I) for n in ("width", "height", "hs", "vs", "mcus_w", "mcus_h")] + [("reserved", _I * 4)]


class JpegEncSizes(ctypes.Structure):
    """Mirror of ``fd_jpeg_enc_sizes``."""
    _fields_ = [(n, _L) for n in ("blocks", "tiles", "tab_off", "coef_off", "bits_off", "pos_off", "tile_off", "tilepos_off", "total_off",
                                  "result_off", "result_bytes", "raw_off", "raw_bytes", "work_bytes", "out_bytes", "reserved")]


class JpegEncResult(ctypes.Structure):
    """Mirror of ``fd_jpeg_enc_result``."""
    _fields_ = [(n, _L) for n in ("out_off", "out_bytes", "stream_bits", "stuffed")]


assert ctypes.sizeof(JpegEncDesc) == 96 and ctypes.sizeof(JpegEncSizes) == 128 and ctypes.sizeof(JpegEncResult) == 32


class LogCfg(ctypes.Structure):
    """Mirror of ``fd_log_cfg``."""
    _fields_ = [("Hs", _I), ("Ws", _I), ("n_rows", _I), ("n_disp", _I), ("row_y", _I * 8), ("row_h", _I * 8), ("row_first", _I * 8),
                ("row_count", _I * 8), ("disp_tile", _I * 8), ("lo", _F), ("span", _F), ("eps", _F), ("reserved", _I)]


# name -> (argument kinds, restype kind)  ('p' pointer, 'i' int, 'l' long, 'f' float, 'd' double)
SIGNATURES = {
    "fd_abi_version": ("", "i"),
    "fd_supported_arch": ("", "s"),
    "fd_last_error": ("", "s"),
    "fd_tuning_defaults": ("p", "v"),
    "fd_set_tuning": ("p", "i"),
    "fd_get_tuning": ("p", "v"),
    "fd_tuning_generation": ("", "l"),
    "fd_disp_to_depth_fwd": ("ppplddp", "i"),
    "fd_disp_to_depth_bwd": ("pppplddp", "i"),
    "fd_pose_matrix_fwd": ("pppiip", "i"),
    "fd_pose_matrix_bwd": ("pppppiip", "i"),
    "fd_pose_head_fwd": ("ppppiiiiip", "i"),
    "fd_pose_head_bwd": ("pppiiiiip", "i"),
    "fd_proj_matrix_fwd": ("ppplip", "i"),
    "fd_proj_matrix_bwd": ("pplpip", "i"),
    "fd_backproject_fwd": ("pppiiip", "i"),
    "fd_backproject_bwd": ("pppiiip", "i"),
    "fd_project3d_fwd": ("ppppiiifp", "i"),
    "fd_project3d_bwd_ws_floats": ("iii", "l"),
    "fd_project3d_bwd": ("pppppppiiifp", "i"),
    "fd_cat_xy_fwd": ("pppiiip", "i"),
    "fd_bilinear_up_fwd": ("ppiiiiip", "i"),
    "fd_bilinear_up_bwd": ("ppiiiiip", "i"),
    "fd_ssim_fwd": ("pppiiiip", "i"),
    "fd_ssim_bwd": ("pppppiiiip", "i"),
    "fd_reproj_loss_map": ("pppliiiip", "i"),
    "fd_photo_ws_floats": ("iii", "l"),
    "fd_photo_fwd": ("p" * 16, "i"),
    "fd_photo_bwd_ws_floats": ("iii", "l"),
    "fd_photo_bwd": ("pppppppp" "i" "pppppp", "i"),
    "fd_photo_fwd_ex": ("p" * 18, "i"),
    "fd_photo_bwd_ex": ("ppppppppp" "i" "pppppp", "i"),
    "fd_photo_ms_ws_floats": ("p", "l"),
    "fd_photo_ms_fwd": ("p" * 14, "i"),
    "fd_photo_ms_bwd": ("p" * 11, "i"),
    "fd_smooth_ws_floats": ("iii", "l"),
    "fd_smooth_fwd": ("ppppiiiip", "i"),
    "fd_smooth_bwd": ("pppppiiiip", "i"),
    "fd_scatter_2channel": ("ppiiiiiiiip", "i"),
    "fd_conv2d_fwd_wt_floats": ("p", "l"),
    "fd_conv2d_fwd_ws_floats": ("p", "l"),
    "fd_conv2d_fwd": ("pppppp" "i" "pp", "i"),
    "fd_conv2d_fwd_stat_slots": ("p", "l"),
    "fd_conv2d_fwd_stats": ("pppppp" "i" "ppp", "i"),
    "fd_conv2d_fwd_bn_ok": ("pi", "i"),
    "fd_conv2d_fwd_bn": ("pppppip" "pppppppp" "iffip", "i"),
    "fd_bn_train_fwd_parts": ("pppppppppp" "iiiiii" "ff" "ip", "i"),
    "fd_conv2d_bwd_data_wt_floats": ("p", "l"),
    "fd_conv2d_bwd_data_ws_floats": ("p", "l"),
    "fd_conv2d_bwd_data": ("ppppp" "i" "pp", "i"),
    "fd_conv2d_bwd_data_add": ("pppppp" "i" "pp", "i"),
    "fd_conv2d_bwd_data_inact": ("pppp" "i" "pp" "i" "pp", "i"),
    "fd_conv3x3_wino_wt_floats": ("p", "l"),
    "fd_conv3x3_wino_ws_floats": ("p", "l"),
    "fd_conv3x3_wino_fwd": ("pppppp" "i" "pp", "i"),
    "fd_velo_rasterize_ws_bytes": ("iii", "l"),
    "fd_velo_rasterize": ("pipiiiiipppp", "i"),
    "fd_resize_linear_cv": ("ppliiiip", "i"),
    "fd_masked_median_ws_bytes": ("iii", "l"),
    "fd_masked_median": ("ppfiiiiiiippp", "i"),
    "fd_refine_inputs_ws_bytes": ("p", "l"),
    "fd_refine_inputs": ("ppppppppp", "i"),
    "fd_conv2d_relayout_jobs": ("pippp", "i"),
    "fd_relayout_plan": ("pi", "l"),
    "fd_relayout_batch": ("pilp", "i"),
    "fd_conv2d_bwd_weight_ws_floats": ("p", "l"),
    "fd_conv2d_bwd_weight": ("pppppp" "i" "p", "i"),
    "fd_act_bwd": ("ppplip", "i"),
    "fd_bn_ws_floats": ("iiiii", "l"),
    "fd_bn_train_fwd": ("pppppppppp" "iiiii" "ff" "ip", "i"),
    "fd_bn_eval_fwd": ("ppppppp" "iiii" "f" "ip", "i"),
    "fd_bn_train_bwd": ("ppppppppppp" "iiiii" "iip", "i"),
    "fd_bn_train_bwd_remask": ("pppppppppp" "iiiii" "ip", "i"),
    "fd_bn_relu_maxpool_fwd": ("ppppppppppp" "iiiii" "ffp", "i"),
    "fd_bn_relu_maxpool_bwd": ("pppppppppppp" "iiiii" "ip", "i"),
    "fd_maxpool3x3s2_fwd": ("pppiiiip", "i"),
    "fd_maxpool3x3s2_bwd": ("pppiiiip", "i"),
    "fd_upcat_fwd": ("ppppp" "iiiiii" "p", "i"),
    "fd_upcat_bwd": ("pppp" "iiiiii" "p", "i"),
    "fd_upcat_bwd_act": ("pp" "i" "ppp" "iiiiii" "p", "i"),
    "fd_upsample2x_fwd": ("ppliip", "i"),
    "fd_upsample2x_bwd": ("ppliip", "i"),
    "fd_axpby": ("ppplffp", "i"),
    "fd_input_normalize": ("pplffp", "i"),
    "fd_stack_normalize": ("pppiiiiiipiffp", "i"),
    "fd_combine_losses_fwd": ("pppifpp", "i"),
    "fd_combine_losses_bwd": ("pifpp", "i"),
    "fd_spatial_mean_fwd": ("ppllfp", "i"),
    "fd_spatial_mean_bwd": ("ppllfp", "i"),
    "fd_depth_errors": ("pplppp", "i"),
    "fd_post_process_disparity": ("ppplii" "p", "i"),
    "fd_adam_step": ("ppppl" "fffffff" "p", "i"),
    "fd_adam_step_dev": ("ppppl" "p" "ffff" "p", "i"),
    "fd_adam_step_dev_zero": ("ppppl" "p" "ffff" "p", "i"),
    "fd_grad_stats_ws_bytes": ("li", "l"),
    "fd_grad_stats": ("plpi" "ffi" "pppp" "p", "i"),
    "fd_adam_step_guarded": ("ppppl" "p" "ffff" "pi" "p", "i"),
    "fd_replay_function_count": ("", "i"),
    "fd_replay_function_name": ("i", "s"),
    "fd_replay_function_signature": ("i", "s"),
    "fd_replay": ("pippip", "i"),
    "fd_gdc_prepare_ws_bytes": ("ii", "l"),
    "fd_gdc_prepare": ("ppii" "dddddddd" "pppp", "i"),
    "fd_gdc_ws_bytes": ("iii", "l"),
    "fd_gdc_build": ("ppp" "iiiii" "ddddddd" "pp", "i"),
    "fd_gdc_cg_iters": ("piiiip", "i"),
    "fd_gdc_finish": ("ppp" "iiiii" "ppp", "i"),
    "fd_resize_lanczos_u8_ws_bytes": ("iiiii", "l"),
    "fd_resize_lanczos_u8": ("pp" "iiiii" "pipi" "ppp", "i"),
    "fd_color_jitter_u8_ws_bytes": ("i", "l"),
    "fd_color_jitter_u8_means_offset": ("i", "l"),
    "fd_color_jitter_u8": ("plplpl" "pil" "pp", "i"),
    "fd_u8_to_planes": ("pp" "iii" "l" "p", "i"),
    "fd_sparsify_ws_bytes": ("p", "l"),
    "fd_sparsify_scans": ("pp" "l" "ppppppp" "p", "i"),
    "fd_velo_rasterize_batch_ws_bytes": ("iii", "l"),
    "fd_velo_rasterize_batch": ("pp" "ii" "p" "iiiiii" "ppp" "p", "i"),
    "fd_resize_bilinear_batch": ("pl" "p" "iii" "p" "p", "i"),
    "fd_depth_png_keys": ("pl" "p" "iiiii" "ff" "p" "p", "i"),
    "fd_completion_ws_bytes": ("iii", "l"),
    "fd_completion_medians": ("pp" "iii" "ff" "p" "pp", "i"),
    "fd_completion_errors": ("ppp" "iii" "ffff" "p" "pp", "i"),
    "fd_eigen_scores_ws_bytes": ("iil", "l"),
    "fd_eigen_scores": ("piii" "pl" "pi" "il" "fff" "i" "ff" "p" "pp", "i"),
    "fd_eigen_class_scores_ws_bytes": ("iili", "l"),
    "fd_eigen_class_scores": ("piii" "pl" "pi" "il" "fff" "i" "ff" "pi" "pp" "pp", "i"),
    "fd_class_errors": ("ppp" "li" "ff" "p" "p", "i"),
    "fd_val_scores_ws_bytes": ("iil", "l"),
    "fd_val_scores": ("piii" "pl" "pi" "il" "ff" "p" "pp", "i"),
    "fd_completion_val_scores_ws_bytes": ("iil", "l"),
    "fd_completion_val_scores": ("piii" "pl" "pi" "il" "fff" "p" "pp", "i"),
    "fd_depth_export": ("piii" "pi" "lii" "f" "ppp" "p", "i"),
    "fd_depth_quantize_u16": ("pplp", "i"),
    "fd_points_export_ws_bytes": ("ii", "l"),
    "fd_points_export": ("ppp" "il" "ii" "d" "p" "pp" "p", "i"),
    "fd_vis_render_ws_bytes": ("il", "l"),
    "fd_vis_render": ("piii" "fp" "p" "pl" "pi" "l" "ff" "pp" "pp" "l" "pp" "pp", "i"),
    "fd_log_sheets_ws_bytes": ("ii", "l"),
    "fd_log_sheets": ("pp" "ii" "p" "pp" "p", "i"),
    "fd_jpeg_probe": ("plp", "i"),
    "fd_jpeg_entropy_decode": ("pl" "pl" "pp", "i"),
    "fd_jpeg_reconstruct": ("pl" "pi" "pl" "p", "i"),
    "fd_png_probe": ("plp", "i"),
    "fd_png_inflate": ("pl" "pl" "p", "i"),
    "fd_png_band_rows": ("", "i"),
    "fd_png_unfilter": ("pl" "pi" "pl" "p", "i"),
    "fd_png_enc_block_rows": ("", "i"),
    "fd_png_enc_layout": ("pip", "i"),
    "fd_png_enc_filter": ("pl" "pi" "p", "i"),
    "fd_png_enc_plan": ("pi" "pp" "p", "i"),
    "fd_png_enc_emit": ("pl" "pi" "p" "pl" "p", "i"),
    "fd_png_enc_finish": ("pl" "p", "i"),
    "fd_jpeg_enc_quant_tables": ("ip", "i"),
    "fd_jpeg_enc_header": ("iiiii" "pl", "i"),
    "fd_jpeg_enc_layout": ("pip", "i"),
    "fd_jpeg_enc_encode": ("pl" "pi" "i" "pl" "p", "i"),
}

_lock = threading.Lock()
_lib = None


def load():
    """Load (once) and return the ctypes handle; raise if the library is missing or mismatched."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libfdhip.so is not built (%s missing). Run `python -m fusiondepth_amd.build` "
                               "(or __graft_entry__.build()). There is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in SIGNATURES.items():
            fn = getattr(lib, name)           # AttributeError if the symbol is not exported
            fn.argtypes = [_KIND[k] for k in args]
            fn.restype = ctypes.c_char_p if res == "s" else (None if res == "v" else _KIND[res])
        if lib.fd_abi_version() != ABI_VERSION:
            raise RuntimeError("libfdhip ABI %d != expected %d; rebuild" % (lib.fd_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def last_error():
    return load().fd_last_error().decode()


# tuning.host.host_delay_us = x: busy-wait x microseconds before every entry-point call - the experiment behind DESIGN.md's "the
# step is GPU-bound": up to 16 us per call (about +11 ms of host work per step) leaves ms_per_step unchanged (profiles/README.md,
# round 3).  Set by fusiondepth_amd/tuning.py.
HOST_DELAY_US = 0.0


# replay.py: while a region is being recorded, every entry-point call and every tensor handed to ``ptr`` is reported to the recorder
# (one list lookup per call otherwise); HOST_PERSISTENT = host addresses that may appear as literal pointer arguments of a recorded
# call (the shape-keyed convolution descriptors, kept alive by functional._CONV_PLANS and by the plans that reference them)
RECORDER = [None]
HOST_PERSISTENT = set()


def call(name, *args):
    """Invoke an ``int``-returning entry point and raise RuntimeError on a non-zero status."""
    lib = load()
    if RECORDER[0] is not None and name != "fd_replay":
        RECORDER[0].saw_call(name, args)
    if HOST_DELAY_US:
        import time
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e6 < HOST_DELAY_US:
            pass
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed (status %d): %s" % (name, rc, lib.fd_last_error().decode()))


def query(name, *args):
    """Invoke a size-query entry point."""
    return getattr(load(), name)(*args)


def ptr(t):
    """Device pointer of a contiguous float32 (or uint8) CUDA tensor; ``None`` -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("fusiondepth_amd ops run on the GPU only (got a %s tensor); there is no CPU path" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    if t.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError("tensor must be float32 (or uint8 for masks), got %s" % t.dtype)
    if RECORDER[0] is not None:
        RECORDER[0].saw_tensor(t)
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """hipStream_t of the current PyTorch stream on the current device.  Called once per kernel launch (~1 400 times per
    training step): torch.cuda.current_stream() builds a Python Stream object (~10 us); the raw getters are plain C calls."""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def round16(n):
    """``n`` rounded up to the 16-byte alignment of the staging, arena and output layouts."""
    return (n + 15) // 16 * 16


def f32(t):
    """Contiguous float32 view/copy (plumbing only)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fusiondepth_amd: tensors must live on the GPU (no CPU fallback); got %s" % t.device)
