// The dense part of the KITTI 3-D detection export ("fd_depth_export", "fd_depth_quantize_u16"; include/fdhip.h): the loop of
// export_detection.py:317-392 without its scoring, for N maps of different sizes packed back to back, in ONE launch.
//
// Store-bound streaming: 2 B (+ 4 B with the float map) written per pixel; the 192x640 source is 0.5 MB per map and stays in cache.
//   * grid (row jobs, column chunks, maps), sized by the chunk's largest map; a wave whose job lies outside its own map exits at once.
//   * a wave owns 512 columns and up to `rows` rows.  Planes start at arbitrary element offsets, so the 16-byte phase of a row start
//     changes from row to row by W mod 8 - but rows y and y + k, k = 8 / gcd(W, 8), share it.  A wave therefore takes rows
//     c, c + k, c + 2k, ... of one class: its head length s (elements up to the first 16-byte boundary of the row, from the ADDRESS)
//     is the same for all of them, a lane's eight body columns s + 8 g .. s + 8 g + 7 are fixed, and their horizontal taps and weights
//     are computed once and reused down the rows.
//   * per row: lanes < s of column chunk 0 store the head pixels one by one, every lane whose eight columns are inside the row stores
//     one uint4 of eight uint16 (and two float4), the lane that holds the row's end stores its pixels one by one.
// Every float32 step is one rounding, as numpy does it: contraction is off for the whole file.
#include "../../include/fdhip.h"
#include "fd_common.h"
#include "cv_resize.h"

#pragma clang fp contract(off)

namespace {

constexpr int EXP_WAVES = 4;                                      // row jobs per workgroup
constexpr int EXP_COLS = 8;                                       // body columns per lane: one 16-byte store of uint16

struct ExportArgs {
    const float* disp; int M, h, w;
    const fd_export_desc* desc; int N; long packed_elems;
    float pred_scale; const float* ratio;
    float* depth_out; uint16_t* u16_out;
    int rows;                                                     // rows per wave
};

// numpy's astype(np.uint16) in range (truncation toward zero); out of range as include/fdhip.h defines it
template <class T>
__device__ __forceinline__ unsigned quantize_u16(T q) {
    if (!(q > (T)0)) return 0u;                                   // NaN, negative, zero
    if (q >= (T)65535) return 65535u;                             // +inf included
    return (unsigned)(int)q;
}

struct Taps { int x0, x1; float a0, a1; };

__global__ void __launch_bounds__(EXP_WAVES * 64) k_depth_export(ExportArgs a) {
    const int n = blockIdx.z, lane = threadIdx.x & 63;
    const int job = blockIdx.x * EXP_WAVES + (threadIdx.x >> 6); // wave-uniform
    const fd_export_desc d = a.desc[n];
    if (d.H <= 0 || d.W <= 0 || d.pred < 0 || d.pred >= a.M || d.offset < 0 || d.offset > a.packed_elems ||
        (long)d.H * d.W > a.packed_elems - d.offset)
        return;
    const int W = d.W, H = d.H;
    const int chunk0 = blockIdx.y * 64 * EXP_COLS;                // first body group's column, before the head shift
    if (chunk0 >= W) return;
    const int k = 8 / (((W & 7) == 0) ? 8 : (W & -W & 7));        // 8 / gcd(W, 8): rows y and y + k start at the same 16-byte phase
    const int c = job % k, band = job / k;
    const int y_first = band * (k * a.rows) + c;
    if (y_first >= H) return;
    // the head length of this wave's rows, from the address of the narrowest output that is written
    const long first = d.offset + (long)y_first * W;
    const unsigned long long elem = a.u16_out ? ((unsigned long long)(uintptr_t)a.u16_out >> 1) + (unsigned long long)first
                                              : ((unsigned long long)(uintptr_t)a.depth_out >> 2) + (unsigned long long)first;
    const int s = (int)((8ull - (elem & 7ull)) & 7ull);
    const bool f_vec = a.depth_out && ((((unsigned long long)(uintptr_t)a.depth_out >> 2) + (unsigned long long)first + s) & 3ull) == 0 &&
                       ((uintptr_t)a.depth_out & 3) == 0;
    const bool u_vec = a.u16_out && ((uintptr_t)a.u16_out & 1) == 0;          // the phase above is exact only for an even address

    const float* src = a.disp + (long)d.pred * a.h * a.w;
    const double sx = (double)a.w / (double)W, sy = (double)a.h / (double)H;
    const float ratio = a.ratio ? a.ratio[n] : 1.0f;
    const bool scaled = a.ratio != nullptr;

    const int xb = chunk0 + s + lane * EXP_COLS;                  // this lane's first body column
    Taps t[EXP_COLS];
#pragma unroll
    for (int j = 0; j < EXP_COLS; ++j) {
        const int x = xb + j < W ? xb + j : W - 1;               // past the row: any valid column, never stored
        cv_linear_coeff(x, sx, a.w, t[j].x0, t[j].x1, t[j].a0, t[j].a1);
    }
    const bool has_head = blockIdx.y == 0 && lane < s && lane < W;
    Taps th = {0, 0, 0.f, 0.f};
    if (has_head) cv_linear_coeff(lane, sx, a.w, th.x0, th.x1, th.a0, th.a1);
    const bool full = xb + EXP_COLS <= W;

    for (int i = 0; i < a.rows; ++i) {
        const int y = y_first + i * k;
        if (y >= H) break;
        int y0, y1;
        float b0, b1;
        cv_linear_coeff(y, sy, a.h, y0, y1, b0, b1);
        const float* row0 = src + (long)y0 * a.w;
        const float* row1 = src + (long)y1 * a.w;
        const long at = d.offset + (long)y * W;
        auto pixel = [&](const Taps& tp, float& p, unsigned& q) {
            const float dv = cv_linear_pixel(row0, row1, tp.x0, tp.x1, tp.a0, tp.a1, b0, b1);
            p = (1.0f / dv) * a.pred_scale;
            if (scaled) p = p * ratio;
            q = quantize_u16(p * 256.0f);
        };
        if (has_head) {
            float p;
            unsigned q;
            pixel(th, p, q);
            if (a.depth_out) a.depth_out[at + lane] = p;
            if (a.u16_out) a.u16_out[at + lane] = (uint16_t)q;
        }
        if (xb < W) {
            float p[EXP_COLS];
            unsigned q[EXP_COLS];
#pragma unroll
            for (int j = 0; j < EXP_COLS; ++j) pixel(t[j], p[j], q[j]);
            if (a.u16_out) {
                uint16_t* o = a.u16_out + at + xb;
                if (full && u_vec) {
                    *reinterpret_cast<uint4*>(o) = make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
                } else {
#pragma unroll
                    for (int j = 0; j < EXP_COLS; ++j)
                        if (xb + j < W) o[j] = (uint16_t)q[j];
                }
            }
            if (a.depth_out) {
                float* o = a.depth_out + at + xb;
                if (full && f_vec) {
                    *reinterpret_cast<float4*>(o) = make_float4(p[0], p[1], p[2], p[3]);
                    *reinterpret_cast<float4*>(o + 4) = make_float4(p[4], p[5], p[6], p[7]);
                } else {
#pragma unroll
                    for (int j = 0; j < EXP_COLS; ++j)
                        if (xb + j < W) o[j] = p[j];
                }
            }
        }
    }
}

constexpr int Q_PER = 8;                                          // values per thread: one 16-byte store

__global__ void __launch_bounds__(256) k_depth_quantize_u16(const double* __restrict__ x, uint16_t* __restrict__ out, long n, int head) {
    // [0, head): up to the first 16-byte boundary of `out`, one value per thread of the first workgroup; then groups of eight
    if (blockIdx.x == 0 && threadIdx.x < head) out[threadIdx.x] = (uint16_t)quantize_u16(x[threadIdx.x] * 256.0);
    const long groups = (n - head + Q_PER - 1) / Q_PER;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        const long at = head + g * Q_PER;
        if (at + Q_PER <= n) {
            unsigned q[Q_PER];
#pragma unroll
            for (int j = 0; j < Q_PER; ++j) q[j] = quantize_u16(x[at + j] * 256.0);
            *reinterpret_cast<uint4*>(out + at) = make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
        } else {
            for (long j = at; j < n; ++j) out[j] = (uint16_t)quantize_u16(x[j] * 256.0);
        }
    }
}

}  // namespace

extern "C" int fd_depth_export(const float* disp, int M, int h, int w, const fd_export_desc* desc, int N, long packed_elems, int max_H,
                               int max_W, float pred_scale, const float* ratio, float* depth_out, uint16_t* u16_out, void* stream) {
    FD_REQUIRE(disp && desc && (depth_out || u16_out) && M > 0 && h > 0 && w > 0 && packed_elems > 0, "fd_depth_export: bad args");
    FD_REQUIRE(N > 0 && N <= 65535 && max_H > 0 && max_W > 0, "fd_depth_export: N must be 1 .. 65535, max_H and max_W positive");
    FD_REQUIRE((long)M * h * w < (1L << 40) && (long)h * w < (1L << 30), "fd_depth_export: disparities too large");
    FD_REQUIRE(((uintptr_t)desc & 7) == 0 && ((uintptr_t)depth_out & 3) == 0 && ((uintptr_t)u16_out & 1) == 0,
               "fd_depth_export: desc must be 8-byte aligned, the outputs aligned to their element");
    ExportArgs a;
    a.disp = disp; a.M = M; a.h = h; a.w = w;
    a.desc = desc; a.N = N; a.packed_elems = packed_elems;
    a.pred_scale = pred_scale; a.ratio = ratio;
    a.depth_out = depth_out; a.u16_out = u16_out;
    // rows per wave: 8 where the chunk fills the device anyway, fewer for a few small maps (more waves, the taps still reused)
    const int chunks = fd_cdiv(max_W, 64 * EXP_COLS);
    const long waves8 = (long)N * chunks * fd_cdiv(max_H, 8);
    a.rows = waves8 >= 8192 ? 8 : (waves8 >= 2048 ? 4 : 2);
    const int jobs = fd_cdiv(max_H, a.rows) + 8;                  // k * ceil(H / (k rows)) <= H / rows + k, k <= 8
    FD_REQUIRE(chunks <= 65535, "fd_depth_export: max_W too large");
    hipLaunchKernelGGL(k_depth_export, dim3(fd_cdiv(jobs, EXP_WAVES), chunks, N), dim3(EXP_WAVES * 64), 0, (hipStream_t)stream, a);
    FD_LAUNCH_CHECK("fd_depth_export");
    return 0;
}

extern "C" int fd_depth_quantize_u16(const double* x, uint16_t* out, long n, void* stream) {
    FD_REQUIRE(x && out && n > 0, "fd_depth_quantize_u16: bad args");
    FD_REQUIRE(((uintptr_t)x & 7) == 0 && ((uintptr_t)out & 1) == 0, "fd_depth_quantize_u16: x and out must be aligned to their element");
    long head = (long)(((16 - ((uintptr_t)out & 15)) & 15) >> 1);
    if (head > n) head = n;
    const long groups = (n - head + Q_PER - 1) / Q_PER;
    long blocks = (groups + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(k_depth_quantize_u16, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, out, n, (int)head);
    FD_LAUNCH_CHECK("fd_depth_quantize_u16");
    return 0;
}
