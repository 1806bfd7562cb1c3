// F.interpolate(x, size, mode="bilinear", align_corners=False) on the CPU, float32: ATen's source-index rule, shared by the kernels
// that restate it bit for bit (k_resize_bilinear_batch in resize.hip, the training-time scorer in val_scores.hip) so that the two
// cannot drift.  include/fdhip.h spells the rule out (fd_resize_bilinear_batch).
#pragma once
#include <hip/hip_runtime.h>

// area_pixel_compute_source_index(align_corners=False) + the index / weight step of upsample_bilinear2d, float32.
// scale = (float)n_in / (float)n_out;  l0 weighs tap i0, l1 tap i1.
__device__ __forceinline__ void aten_src(int dst, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);      // ONE rounding
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i0 = i0 > n_in - 1 ? n_in - 1 : i0;                               // never taken for a valid size; keeps the loads in the plane
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}
