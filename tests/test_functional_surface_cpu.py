"""fusiondepth_amd.functional after its split into loss_ops / data_ops / pass_state: every public name it had is still there and is
the object its new module defines, the flop tally is still the module global the benchmark assigns, and none of the new modules
imports functional back."""
import os
import subprocess
import sys
import types

from fusiondepth_amd import data_ops, functional, loss_ops, pass_state, weight_layouts

# [n for n in dir(functional) if not n.startswith('_')] without submodules, before the split
PUBLIC = [
    'ACT', 'CONV_FLOP_TALLY', 'JITTER_OPS', 'PAD_MODE', 'PROJECT_EPS', 'PhotoOptions', 'SPARSIFY_BOX', 'SPARSIFY_LINE_SPEC', 'adam_step',
    'adam_step_dev', 'add', 'add_grad_ready_callback', 'as_int64', 'backproject_depth', 'batch_norm', 'begin_forward_pass',
    'bilinear_upsample', 'bn_groups', 'bn_relu_maxpool', 'build_weight_plan', 'bump_bn_counter', 'bump_weights_epoch', 'call', 'cat_xy',
    'color_jitter_u8', 'combine_losses', 'conv2d', 'conv2d_stats', 'conv2d_tap', 'conv_bn', 'conv_bn_frozen', 'defer_bn_counters',
    'depth_errors', 'disp_to_depth', 'enable_direct_grad', 'enable_side_wgrad', 'enable_weight_cache', 'evict_dead_weight_layouts', 'f32',
    'folded_tensors', 'frozen_epoch', 'get_smooth_loss', 'image_pyramid', 'input_normalize', 'invalidate_frozen_layouts',
    'join_wgrad_streams', 'lanczos_table', 'mark_single_consumer', 'masked_median', 'max_pool3x3s2', 'normalized_smooth_loss', 'padded_rows',
    'param_uses', 'photo_loss', 'photo_loss_ms', 'photo_ms_supported', 'pose_head', 'project_3d', 'ptr', 'query', 'raster_desc_table',
    'refine_inputs', 'refresh_weight_layouts', 'release_retired_layouts', 'reprojection_loss_map', 'resize_bilinear_batch',
    'resize_desc_table', 'resize_lanczos_u8', 'resize_linear_cv', 'scaled_roi', 'scatter_2channel', 'sparsify_rows', 'sparsify_scans',
    'spatial_mean', 'ssim', 'stack_normalize', 'stream', 'sync_late_layouts', 'transformation_from_parameters', 'u8_to_planes', 'unfreeze',
    'upsample_concat', 'upsample_nearest2x', 'velo_rasterize', 'velo_rasterize_batch', 'weight_layout', 'weight_plan_needs_rebuild']

MOVED = {
    loss_ops: ['PROJECT_EPS', 'PhotoOptions', 'backproject_depth', 'bilinear_upsample', 'cat_xy', 'combine_losses', 'disp_to_depth',
               'get_smooth_loss', 'normalized_smooth_loss', 'photo_loss', 'photo_loss_ms', 'photo_ms_supported', 'pose_head', 'project_3d',
               'reprojection_loss_map', 'ssim', 'transformation_from_parameters'],
    data_ops: ['JITTER_OPS', 'SPARSIFY_BOX', 'SPARSIFY_LINE_SPEC', 'as_int64', 'color_jitter_u8', 'image_pyramid', 'lanczos_table',
               'padded_rows', 'raster_desc_table', 'resize_bilinear_batch', 'resize_desc_table', 'resize_lanczos_u8', 'scaled_roi',
               'scatter_2channel', 'sparsify_rows', 'sparsify_scans', 'u8_to_planes', 'velo_rasterize', 'velo_rasterize_batch'],
    pass_state: ['add_grad_ready_callback', 'begin_forward_pass', 'bn_groups', 'bump_bn_counter', 'defer_bn_counters', 'enable_direct_grad',
                 'enable_side_wgrad', 'join_wgrad_streams', 'param_uses'],
    weight_layouts: ['build_weight_plan', 'bump_weights_epoch', 'enable_weight_cache', 'evict_dead_weight_layouts', 'frozen_epoch',
                     'invalidate_frozen_layouts', 'refresh_weight_layouts', 'release_retired_layouts', 'sync_late_layouts', 'unfreeze',
                     'weight_layout', 'weight_plan_needs_rebuild'],
}


def test_every_public_name_still_resolves():
    assert len(PUBLIC) == len(set(PUBLIC)) == 87
    missing = [n for n in PUBLIC if not hasattr(functional, n)]
    assert not missing, missing
    assert not [n for n in PUBLIC if isinstance(getattr(functional, n), types.ModuleType)]


def test_moved_names_are_the_objects_of_their_new_module():
    for mod, names in MOVED.items():
        for n in names:
            assert n in PUBLIC, n
            assert getattr(functional, n) is getattr(mod, n), (mod.__name__, n)
    # what is left is defined in functional itself (or is one of the _lib helpers it always carried)
    moved = {n for names in MOVED.values() for n in names}
    for n in set(PUBLIC) - moved - {'CONV_FLOP_TALLY', 'ACT', 'PAD_MODE', 'call', 'f32', 'ptr', 'query', 'stream'}:
        assert getattr(functional, n).__module__ == functional.__name__, n


class _Desc:
    N, Cout, Cin, KH, KW = 2, 3, 5, 3, 3


def test_flop_tally_is_the_module_global_the_benchmark_assigns():
    before = functional.CONV_FLOP_TALLY
    try:
        functional.CONV_FLOP_TALLY = [0.0]
        functional._tally(_Desc, 4, 6, passes=2)
        assert functional.CONV_FLOP_TALLY[0] == 25920.0          # 2 * 2 * 2 * 3 * 4 * 6 * 5 * 9
        functional.CONV_FLOP_TALLY = None
        functional._tally(_Desc, 4, 6, passes=2)                 # switched off: counts nothing, raises nothing
        assert functional.CONV_FLOP_TALLY is None
    finally:
        functional.CONV_FLOP_TALLY = before


def test_the_new_modules_do_not_import_functional():
    code = ("import sys; import fusiondepth_amd.pass_state, fusiondepth_amd.loss_ops, fusiondepth_amd.data_ops; "
            "assert 'fusiondepth_amd.functional' not in sys.modules, 'functional imported'")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
