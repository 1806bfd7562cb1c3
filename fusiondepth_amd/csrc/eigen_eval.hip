// The Eigen-split scorer ("fd_eigen_scores"; include/fdhip.h): the per-image loop of evaluate_depth.py:344-478, without GDC, for N
// images of different ground-truth sizes in one call.  6 launches (5 without median scaling), whatever N is.  The kernels are
// score_lists.h's, instantiated with RULE_EIGEN: the mask  gt > gt_lo && gt < gt_hi, OpenCV's float32 INTER_LINEAR resize of the
// disparity from its four taps (k_resize_linear_cv's arithmetic: horizontal pass first, separate multiplies and adds), 1 / disp (IEEE
// division), * pred_scale, numpy's medians (an even count takes the float32 mean of the two middle values) and the terms of
// compute_errors (evaluate_depth.py:42-60).  fd_val_scores (val_scores.hip) is the same chain under the trainer's rules.
// Every float32 step is one rounding, as numpy does it: contraction is off for the whole file.
#include "score_lists.h"

#pragma clang fp contract(off)

extern "C" long fd_eigen_scores_ws_bytes(int N, int max_rows, long list_cap) {
    if (!sizes_ok(N, max_rows, list_cap)) return 0;
    return layout(N, max_rows, list_cap).total;
}

extern "C" int fd_eigen_scores(const float* disp, int M, int h, int w, const float* packed, long packed_floats, const fd_eigen_desc* desc,
                               int N, int max_rows, long list_cap, float gt_lo, float gt_hi, float pred_scale, int median_scaling, float lo,
                               float hi, double* out, void* ws, void* stream) {
    FD_REQUIRE(disp && packed && desc && out && ws && M > 0 && h > 0 && w > 0 && packed_floats > 0, "fd_eigen_scores: bad args");
    FD_REQUIRE(sizes_ok(N, max_rows, list_cap), "fd_eigen_scores: N must be 1 .. 4096, max_rows and list_cap non-negative");
    FD_REQUIRE((long)M * h * w < (1L << 40) && (long)h * w < (1L << 30), "fd_eigen_scores: disparities too large");
    FD_REQUIRE((((uintptr_t)ws | (uintptr_t)out | (uintptr_t)desc | (uintptr_t)packed) & 7) == 0,
               "fd_eigen_scores: packed, desc, out and ws must be 8-byte aligned");
    Args a;
    a.disp = disp; a.M = M; a.h = h; a.w = w; a.packed = packed; a.packed_floats = packed_floats; a.desc = desc; a.N = N;
    a.max_rows = max_rows; a.list_cap = list_cap; a.gt_lo = gt_lo; a.gt_hi = gt_hi; a.pred_scale = pred_scale; a.lo = lo; a.hi = hi;
    a.median_scaling = median_scaling;
    a.out = out;
    place(a, ws);
    static const char* const names[6] = {"fd_eigen_scores (count)",   "fd_eigen_scores (scan)",   "fd_eigen_scores (compact)",
                                         "fd_eigen_scores (medians)", "fd_eigen_scores (errors)", "fd_eigen_scores (finish)"};
    return launch_scores<RULE_EIGEN>(a, (hipStream_t)stream, names);
}
