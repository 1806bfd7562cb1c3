// Per-class Eigen-split scores ("fd_eigen_class_scores", "fd_class_errors"; include/fdhip.h): evaluate_depth.py's --per_semantic loop
// (:451-467), 34 boolean selections and compute_errors calls per image, as one call for N images.  fd_eigen_class_scores makes
// fd_eigen_scores' six launches under RULE_EIGEN (score_lists.h) with the compact launch instantiated to write each selected pixel's
// label beside its pair, then ONE more launch: k_class_errors, a workgroup per (class, image) that walks the image's compact list -
// a few times 10^4 pairs, not the plane - keeps the pairs of its class, forms k_score_errors' terms from the same ratio and clamps
// (score_terms) and writes class_out[n][c] itself.  No partials, no finish launch, no float atomics: two calls give the same bits.
// fd_class_errors is that class kernel alone on matched lists (the --eval_gdc path, where the dense map exists on the device): the
// same workgroup shape, thread stride and tree, so the same pairs give the same bits by either entry.
#include "score_lists.h"

#pragma clang fp contract(off)

namespace {

inline bool classes_ok(int K) { return K >= 1 && K <= 256; }

// fd_eigen_scores' workspace, then the label list: the three scorers' layout and sizes stay as they are
inline long label_list_at(int N, int max_rows, long list_cap) { return layout(N, max_rows, list_cap).total; }

}  // namespace

extern "C" long fd_eigen_class_scores_ws_bytes(int N, int max_rows, long list_cap, int K) {
    if (!sizes_ok(N, max_rows, list_cap) || !classes_ok(K)) return 0;
    return label_list_at(N, max_rows, list_cap) + align8(list_cap);
}

extern "C" int fd_eigen_class_scores(const float* disp, int M, int h, int w, const float* packed, long packed_floats,
                                     const fd_eigen_desc* desc, int N, int max_rows, long list_cap, float gt_lo, float gt_hi,
                                     float pred_scale, int median_scaling, float lo, float hi, const unsigned char* labels, int K,
                                     double* out, double* class_out, void* ws, void* stream) {
    FD_REQUIRE(disp && packed && desc && labels && out && class_out && ws && M > 0 && h > 0 && w > 0 && packed_floats > 0,
               "fd_eigen_class_scores: bad args");
    FD_REQUIRE(classes_ok(K), "fd_eigen_class_scores: K must be 1 .. 256");
    FD_REQUIRE(sizes_ok(N, max_rows, list_cap), "fd_eigen_class_scores: N must be 1 .. 4096, max_rows and list_cap non-negative");
    FD_REQUIRE((long)M * h * w < (1L << 40) && (long)h * w < (1L << 30), "fd_eigen_class_scores: disparities too large");
    FD_REQUIRE((((uintptr_t)ws | (uintptr_t)out | (uintptr_t)class_out | (uintptr_t)desc | (uintptr_t)packed) & 7) == 0,
               "fd_eigen_class_scores: packed, desc, out, class_out and ws must be 8-byte aligned");
    Args a;
    a.disp = disp; a.M = M; a.h = h; a.w = w; a.packed = packed; a.packed_floats = packed_floats; a.desc = desc; a.N = N;
    a.max_rows = max_rows; a.list_cap = list_cap; a.gt_lo = gt_lo; a.gt_hi = gt_hi; a.pred_scale = pred_scale; a.lo = lo; a.hi = hi;
    a.median_scaling = median_scaling;
    a.out = out;
    place(a, ws);
    a.labels = labels; a.K = K; a.class_out = class_out;
    a.label_list = (unsigned char*)ws + label_list_at(N, max_rows, list_cap);
    static const char* const names[7] = {"fd_eigen_class_scores (count)",   "fd_eigen_class_scores (scan)",   "fd_eigen_class_scores (compact)",
                                         "fd_eigen_class_scores (medians)", "fd_eigen_class_scores (errors)", "fd_eigen_class_scores (finish)",
                                         "fd_eigen_class_scores (classes)"};
    return launch_scores<RULE_EIGEN, true>(a, (hipStream_t)stream, names);
}

extern "C" int fd_class_errors(const float* gt, const float* pred, const unsigned char* labels, long n, int K, float lo, float hi,
                               double* class_out, void* stream) {
    FD_REQUIRE(class_out && n >= 0 && (n == 0 || (gt && pred && labels)), "fd_class_errors: bad args");
    FD_REQUIRE(classes_ok(K), "fd_class_errors: K must be 1 .. 256");
    FD_REQUIRE(((uintptr_t)class_out & 7) == 0, "fd_class_errors: class_out must be 8-byte aligned");
    hipLaunchKernelGGL(k_class_errors_lists, dim3(K), dim3(CLASS_THREADS), 0, (hipStream_t)stream, gt, pred, labels, n, lo, hi, class_out);
    FD_LAUNCH_CHECK("fd_class_errors");
    return 0;
}
