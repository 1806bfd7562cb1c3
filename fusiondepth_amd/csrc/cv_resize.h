// cv2.resize(img, (Wout, Hout)) with INTER_LINEAR on a float32 image: OpenCV's coefficient rule, shared by every kernel that restates
// it (k_resize_linear_cv in geometry.hip, the scorer in eigen_eval.hip, the exporter in detection.hip) so that the three cannot drift.
#pragma once
#include <hip/hip_runtime.h>

// resize.cpp: scale in double, source coordinate rounded to float, floor, edge rule; weights (1.f - fx, fx) as floats.
// Not ATen's rule (k_bilinear_fwd computes the coordinate in float32 throughout): at x ~ 600 the two differ by ~6e-5 in the weight.
__device__ __forceinline__ void cv_linear_coeff(int d, double scale, int n_in, int& s0, int& s1, float& w0, float& w1) {
#pragma clang fp contract(off)     // no FMA contraction (HIP's __fmul_rn / __dmul_rn are plain operators): OpenCV's scalar arithmetic
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
    s0 = s; s1 = s + 1 < n_in ? s + 1 : n_in - 1;
    w0 = 1.0f - f; w1 = f;
}

// One output pixel from its four taps: the horizontal pass first, separate multiplies and adds (the arithmetic of the numpy
// restatement in oracle/evaluate.py).  `row0` / `row1` point at source rows y0 / y1.
__device__ __forceinline__ float cv_linear_pixel(const float* __restrict__ row0, const float* __restrict__ row1, int x0, int x1, float a0,
                                                 float a1, float b0, float b1) {
#pragma clang fp contract(off)
    const float r0 = row0[x0] * a0 + row0[x1] * a1;
    const float r1 = row1[x0] * a0 + row1[x1] * a1;
    return r0 * b0 + r1 * b1;
}
