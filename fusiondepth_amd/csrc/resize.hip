// Batched bilinear resize of planes of DIFFERENT sizes to one output size, with an optional left-right mirror of the result: the
// "inf_gdc" training key (kitti_dataset.py:154-173: np.load -> F.interpolate(mode="bilinear", align_corners=False) -> fliplr), one
// launch per batch.  The arithmetic is ATen's CPU rule for float32, restated operation by operation so that the output is
// bit-identical to torch on the host (include/fdhip.h spells it out).  Every fused multiply-add of that rule is written as an
// explicit fmaf and contraction is off for the rest of the file, so the compiler fuses nothing else.
//
// One thread per output pixel, grid (ceil(Hout * Wout / 256), B): the descriptor is uniform per block (plain loads, served from
// the scalar / L2 path), stores are coalesced, and the four taps of neighbouring threads fall into the same two source rows.  A
// gather bound by those rows: no LDS.
#include "../../include/fdhip.h"
#include "fd_common.h"
#include "aten_resize.h"                                        // ATen's source-index rule (aten_src)

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(256) k_resize_bilinear_batch(const float* __restrict__ packed, long packed_floats,
                                                               const fd_resize_desc* __restrict__ desc, int out_h, int out_w,
                                                               float* __restrict__ out) {
    const int b = blockIdx.y;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= out_h * out_w) return;
    const fd_resize_desc d = desc[b];
    float* dst = out + (long)b * out_h * out_w + o;
    // a descriptor that leaves the packed buffer gives a NaN plane, never a read outside it
    if (d.h_in <= 0 || d.w_in <= 0 || d.offset < 0 || d.offset > packed_floats ||
        (long)d.h_in * d.w_in > packed_floats - d.offset) {
        *dst = __builtin_nanf("");
        return;
    }
    const int oy = o / out_w, ox = o - oy * out_w;
    const int rx = d.mirror ? out_w - 1 - ox : ox;                    // the mirror acts on the RESIZED plane
    const float sy = (float)d.h_in / (float)out_h, sx = (float)d.w_in / (float)out_w;
    int y0, y1, x0, x1;
    float hy, ly, hx, lx;
    aten_src(oy, sy, d.h_in, y0, y1, hy, ly);
    aten_src(rx, sx, d.w_in, x0, x1, hx, lx);
    const float* r0 = packed + d.offset + (long)y0 * d.w_in;
    const float* r1 = packed + d.offset + (long)y1 * d.w_in;
    const float top = __builtin_fmaf(hx, r0[x0], lx * r0[x1]);
    const float bot = __builtin_fmaf(hx, r1[x0], lx * r1[x1]);
    *dst = __builtin_fmaf(hy, top, ly * bot);
}

}  // namespace

extern "C" int fd_resize_bilinear_batch(const float* packed, long packed_floats, const fd_resize_desc* desc, int B, int out_h,
                                        int out_w, float* out, void* stream) {
    FD_REQUIRE(packed && desc && out && packed_floats > 0 && B > 0 && B <= 65535 && out_h > 0 && out_w > 0 &&
                   (long)out_h * out_w < (1l << 31) - 256,
               "fd_resize_bilinear_batch: bad args");
    hipLaunchKernelGGL(k_resize_bilinear_batch, dim3(fd_cdiv((long)out_h * out_w, 256), B), dim3(256), 0, (hipStream_t)stream, packed,
                       packed_floats, desc, out_h, out_w, out);
    FD_LAUNCH_CHECK("fd_resize_bilinear_batch");
    return 0;
}
