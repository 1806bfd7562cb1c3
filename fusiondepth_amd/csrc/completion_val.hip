// The Completor's training-time scorer ("fd_completion_val_scores"; include/fdhip.h): compute_depth_losses (completor.py:728-762) plus
// compute_depth_errors (layers.py:284-302), per image, for N images in one call of 6 launches, whatever N is.  The kernels are
// score_lists.h's, instantiated with RULE_COMPLETION: the mask  gt > gt_min  (float32 against float32) inside the window, ATen's CPU
// bilinear rule (align_corners=False) on the DEPTH at the selected pixels only, the clamp to [lo, hi] BEFORE the medians, torch's lower
// median, ratio = med(gt) / med(pred), the clamp again, both sides * 1000.0f (millimetres) and the seven terms on the scaled values.
// fd_val_scores (val_scores.hip) is the same chain under the trainer's rule: gt > 0, metres.
// Every float32 step is one rounding: contraction is off for the whole file, the fused multiply-adds of ATen's rule are explicit.
#include "score_lists.h"

#pragma clang fp contract(off)

extern "C" long fd_completion_val_scores_ws_bytes(int N, int max_rows, long list_cap) {
    if (!sizes_ok(N, max_rows, list_cap)) return 0;
    return layout(N, max_rows, list_cap).total;
}

extern "C" int fd_completion_val_scores(const float* depth, int M, int h, int w, const float* packed, long packed_floats,
                                        const fd_eigen_desc* desc, int N, int max_rows, long list_cap, float gt_min, float lo, float hi,
                                        double* out, void* ws, void* stream) {
    FD_REQUIRE(depth && packed && desc && out && ws && M > 0 && h > 0 && w > 0 && packed_floats > 0, "fd_completion_val_scores: bad args");
    FD_REQUIRE(sizes_ok(N, max_rows, list_cap), "fd_completion_val_scores: N must be 1 .. 4096, max_rows and list_cap non-negative");
    FD_REQUIRE((long)M * h * w < (1L << 40) && (long)h * w < (1L << 30), "fd_completion_val_scores: depths too large");
    FD_REQUIRE((((uintptr_t)ws | (uintptr_t)out | (uintptr_t)desc | (uintptr_t)packed) & 7) == 0,
               "fd_completion_val_scores: packed, desc, out and ws must be 8-byte aligned");
    Args a;
    a.disp = depth; a.M = M; a.h = h; a.w = w; a.packed = packed; a.packed_floats = packed_floats; a.desc = desc; a.N = N;
    a.max_rows = max_rows; a.list_cap = list_cap;
    a.gt_lo = gt_min; a.gt_hi = __builtin_inff();                 // depth_gt > 0.1
    a.pred_scale = 1.f; a.lo = lo; a.hi = hi;
    a.median_scaling = 1;
    a.out = out;
    place(a, ws);
    static const char* const names[6] = {"fd_completion_val_scores (count)",   "fd_completion_val_scores (scan)",
                                         "fd_completion_val_scores (compact)", "fd_completion_val_scores (medians)",
                                         "fd_completion_val_scores (errors)",  "fd_completion_val_scores (finish)"};
    return launch_scores<RULE_COMPLETION>(a, (hipStream_t)stream, names);
}
