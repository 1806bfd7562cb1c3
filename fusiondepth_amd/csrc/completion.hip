// KITTI depth completion: the depth keys of a batch from packed 16-bit PNG planes ("fd_depth_png_keys") and the scorer of
// evaluate_completion.py ("fd_completion_medians", "fd_completion_errors"; include/fdhip.h).
//
//   k_depth_png_keys    datasets/kitti_completion.py:51-80 (get_depth) for S planes of different sizes in one launch: uint16 ->
//                       float32 / div0, mirror, crop / pad (a window of the canvas, zero outside), ceil-mode max-pool, / div1.
//                       Element-wise and memory-bound: one thread makes 4 adjacent outputs, reads the 4 * pool source columns of
//                       each pooled row with 8- or 4-byte loads where the run lies inside the window (2-byte loads at the window's
//                       border) and stores float4 (float2 / single floats only where a plane of odd size breaks the alignment).
//   k_completion_median one workgroup per (image, quantity): numpy's median of gt[m] and of pred[m] * scale, m = gt > gt_min, by
//                       radix select (4 passes of 8 bits, LDS histograms with integer atomics) over order-preserving keys that are
//                       formed from the planes in every pass (float4 loads where the plane allows) - no compaction list, no sort; a fifth pass finds the upper middle
//                       element for an even count (the count of keys <= the lower one, else the smallest key above it).
//   k_completion_ratio  ratio = median(gt) / median(pred), one thread per image.
//   k_completion_errors evaluate_completion.py:31-48 per element in float32, summed in float64: a fixed grid of workgroups per
//                       image, a fixed shuffle tree inside each, partials to the workspace;
//   k_completion_finish sums an image's partials in index order.  No float atomics anywhere: run-to-run identical.
// Every float32 step below is one rounding, as numpy does it: contraction is off for the whole file.
#include "../../include/fdhip.h"
#include "fd_common.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------- fd_depth_png_keys
__device__ __forceinline__ bool desc_ok(const fd_depth_png_desc& d, long packed_elems, int ch, int cw) {
    return d.h > 0 && d.w > 0 && d.offset >= 0 && d.offset <= packed_elems && (long)d.h * d.w <= packed_elems - d.offset &&
           d.win_h >= 0 && d.win_w >= 0 && d.win_y >= 0 && d.win_x >= 0 && d.win_y <= ch - d.win_h && d.win_x <= cw - d.win_w &&
           d.src_y >= 0 && d.src_x >= 0 && d.src_y <= d.h - d.win_h && d.src_x <= d.w - d.win_w;
}

// NC consecutive uint16 starting at element `first` of `packed` (all inside the buffer), ascending, widest aligned loads first
template <int NC>
__device__ __forceinline__ void load_run(const uint16_t* __restrict__ packed, long packed_elems, long first, unsigned (&v)[NC]) {
    if ((first & 3) == 0) {                                       // 8-byte loads
#pragma unroll
        for (int k = 0; k < NC / 4; ++k) {
            const uint2 q = *reinterpret_cast<const uint2*>(packed + first + 4 * k);
            v[4 * k] = q.x & 0xffffu; v[4 * k + 1] = q.x >> 16; v[4 * k + 2] = q.y & 0xffffu; v[4 * k + 3] = q.y >> 16;
        }
        return;
    }
    const long a0 = first & ~1L;
    const int odd = (int)(first & 1);
    if (a0 + NC + 2 * odd <= packed_elems) {                      // 4-byte loads: NC / 2 words, one more for an odd start
        unsigned t[NC + 2];
#pragma unroll
        for (int k = 0; k < NC / 2; ++k) {
            const unsigned q = *reinterpret_cast<const unsigned*>(packed + a0 + 2 * k);
            t[2 * k] = q & 0xffffu; t[2 * k + 1] = q >> 16;
        }
        unsigned q = 0;
        if (odd) q = *reinterpret_cast<const unsigned*>(packed + a0 + NC);
        t[NC] = q & 0xffffu; t[NC + 1] = q >> 16;
#pragma unroll
        for (int j = 0; j < NC; ++j) v[j] = odd ? t[j + 1] : t[j];
        return;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) v[j] = packed[first + j];       // an odd run that ends with the buffer
}

template <int POOL>
__global__ void __launch_bounds__(256) k_depth_png_keys(const uint16_t* __restrict__ packed, long packed_elems,
                                                        const fd_depth_png_desc* __restrict__ desc, int canvas_h, int canvas_w,
                                                        int out_h, int out_w, int channels, float div0, float div1,
                                                        float* __restrict__ out) {
    constexpr int NC = 4 * POOL;                                  // canvas columns per thread and row
    const int s = blockIdx.y;
    const int P = out_h * out_w;
    const int q0 = (blockIdx.x * 256 + threadIdx.x) * 4;          // 4 adjacent outputs of plane s, row-major (they may wrap a row)
    if (q0 >= P) return;
    const fd_depth_png_desc d = desc[s];
    const bool ok = desc_ok(d, packed_elems, canvas_h, canvas_w);
    float r[4];
    const int oy = q0 / out_w, ox = q0 - oy * out_w;
    if (!ok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = __builtin_nanf("");
    } else if (ox + 4 <= out_w && POOL * ox >= d.win_x && POOL * ox + NC <= d.win_x + d.win_w) {
        // fast path: the four outputs share a row and all their columns lie inside the window (hence inside the canvas)
        unsigned m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int py = 0; py < POOL; ++py) {
            const int cy = POOL * oy + py;
            if (cy < d.win_y || cy >= d.win_y + d.win_h) continue;           // a row outside the window is zero; cy < canvas_h follows
            const int sy = d.src_y + cy - d.win_y;
            const int sx = d.src_x + POOL * ox - d.win_x;                    // first column, in mirrored coordinates
            const long row = d.offset + (long)sy * d.w;
            unsigned v[NC];
            load_run<NC>(packed, packed_elems, row + (d.mirror ? d.w - sx - NC : sx), v);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const unsigned x = d.mirror ? v[NC - 1 - j] : v[j];
                m[j / POOL] = x > m[j / POOL] ? x : m[j / POOL];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = ((float)m[e] / div0) / div1;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = q0 + e;
            unsigned m = 0u;
            if (q < P) {
                const int y = q / out_w, x = q - y * out_w;
                for (int py = 0; py < POOL; ++py) {
                    const int cy = POOL * y + py;
                    if (cy < d.win_y || cy >= d.win_y + d.win_h) continue;
                    for (int px = 0; px < POOL; ++px) {
                        const int cx = POOL * x + px;
                        if (cx < d.win_x || cx >= d.win_x + d.win_w) continue;
                        const int sx = d.src_x + cx - d.win_x;
                        const unsigned v = packed[d.offset + (long)(d.src_y + cy - d.win_y) * d.w + (d.mirror ? d.w - 1 - sx : sx)];
                        m = v > m ? v : m;
                    }
                }
            }
            r[e] = ((float)m / div0) / div1;
        }
    }
    // uint16 -> float32 is exact and x -> x / div0 is monotone, so the largest code of a block gives the block's largest value:
    // max over the block of ((float)v / div0), as F.max_pool2d of the divided map
    for (int c = 0; c < channels; ++c) {
        const long at = ((long)s * channels + c) * P + q0;
        float* dst = out + at;
        if (q0 + 4 <= P && (at & 3) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
        } else if (q0 + 4 <= P && (at & 1) == 0) {
            *reinterpret_cast<float2*>(dst) = make_float2(r[0], r[1]);
            *reinterpret_cast<float2*>(dst + 2) = make_float2(r[2], r[3]);
        } else {
            for (int e = 0; e < 4 && q0 + e < P; ++e) dst[e] = r[e];
        }
    }
}

// ---------------------------------------------------------------------------------------------- medians
__device__ __forceinline__ unsigned key_of(float v) {     // order-preserving: a < b  <=>  key(a) < key(b)  (as in refine.hip)
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}

// f(v) for every selected value of one plane - gt[i] itself (which == 0) or pred[i] * scale where gt[i] > gt_min - over the
// workgroup's 1024 threads.  A pass is a stream of dependent-free loads whose latency is all it costs, so a plane whose size and
// address allow it is read as float4 (a quarter of the trips, four values in flight per load); any other plane element by element.
template <class F>
__device__ __forceinline__ void for_each_selected(const float* __restrict__ gt, const float* __restrict__ pred, int P, int which,
                                                  float gt_min, float scale, F f) {
    const int t = threadIdx.x;
    const bool vec = (P & 3) == 0 && (((uintptr_t)gt | (uintptr_t)pred) & 15) == 0;          // uniform over the workgroup
    if (vec) {
        const float4* g4 = reinterpret_cast<const float4*>(gt);
        const float4* p4 = reinterpret_cast<const float4*>(pred);
#pragma unroll 2
        for (int i = t; i < P / 4; i += 1024) {
            const float4 g = g4[i];
            const float4 p = which ? p4[i] : g;
            if (g.x > gt_min) f(which ? p.x * scale : g.x);
            if (g.y > gt_min) f(which ? p.y * scale : g.y);
            if (g.z > gt_min) f(which ? p.z * scale : g.z);
            if (g.w > gt_min) f(which ? p.w * scale : g.w);
        }
    } else {
        for (int i = t; i < P; i += 1024) {
            const float g = gt[i];
            if (g > gt_min) f(which ? pred[i] * scale : g);
        }
    }
}

struct MedianArgs { const float* pred; const float* gt; int P; float gt_min, pred_scale; float* out; };

// blockIdx.x: 0 = gt[m], 1 = pred[m] * scale; blockIdx.y: image.  out[n][1 + which] = the median, out[n][3] = the count.
__global__ void __launch_bounds__(1024) k_completion_median(MedianArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[4];
    __shared__ int nan_seen;
    const int which = blockIdx.x, n_img = blockIdx.y, t = threadIdx.x;
    const float* gt = a.gt + (long)n_img * a.P;
    const float* pred = a.pred + (long)n_img * a.P;
    float* o = a.out + n_img * 4;
    if (t == 0) nan_seen = 0;
    unsigned prefix = 0, mask = 0;
    int n = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256) hist[t] = 0;
        __syncthreads();
        for_each_selected(gt, pred, a.P, which, a.gt_min, a.pred_scale, [&](float v) {
            if (v != v) nan_seen = 1;
            const unsigned key = key_of(v);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (t == 0) {
            if (shift == 24) {                                    // the first histogram holds every selected element: the count
                unsigned total = 0;
                for (int b = 0; b < 256; ++b) total += hist[b];
                sh[2] = total;
                sh[1] = total ? (total - 1) / 2 : 0;              // rank of the lower middle element
            }
            int left = (int)sh[1];
            unsigned bin = 0;
            for (; bin < 255; ++bin) {
                if (left < (int)hist[bin]) break;
                left -= (int)hist[bin];
            }
            sh[0] = bin; sh[1] = (unsigned)left;
        }
        __syncthreads();
        n = (int)sh[2];
        if (n == 0) {                                             // np.median of an empty selection: NaN (uniform exit)
            if (t == 0) { o[1 + which] = __builtin_nanf(""); if (!which) o[3] = 0.f; }
            return;
        }
        prefix |= sh[0] << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned lower = prefix;
    unsigned upper = lower;
    if ((n & 1) == 0) {                                           // even count: the element of rank n / 2
        if (t == 0) { sh[0] = 0u; sh[1] = 0xffffffffu; }
        __syncthreads();
        unsigned le = 0, above = 0xffffffffu;
        for_each_selected(gt, pred, a.P, which, a.gt_min, a.pred_scale, [&](float v) {
            const unsigned key = key_of(v);
            if (key <= lower) ++le;
            else above = key < above ? key : above;
        });
        atomicAdd(&sh[0], le);
        atomicMin(&sh[1], above);
        __syncthreads();
        upper = (int)sh[0] >= n / 2 + 1 ? lower : sh[1];
    }
    if (t == 0) {
        const float lo = value_of(lower), hi = value_of(upper);
        // np.median: the float32 mean of the middle element(s) - (lo + hi) rounded to float32, then halved
        o[1 + which] = nan_seen ? __builtin_nanf("") : ((n & 1) ? lo : (lo + hi) / 2.0f);
        if (!which) o[3] = (float)n;
    }
}

__global__ void k_completion_ratio(float* out, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) out[4 * i] = out[4 * i + 1] / out[4 * i + 2];
}

// ---------------------------------------------------------------------------------------------- errors
constexpr int ERR_THREADS = 256;
constexpr int ERR_VALUES = 5;                                     // sum of squares, of abs, of inverse squares, of inverse abs, count

inline int error_groups(int P) {
    const int g = fd_cdiv(P, ERR_THREADS * 16);
    return g < 1 ? 1 : (g > 128 ? 128 : g);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, FD_WAVE);
    return v;
}

struct ErrorArgs { const float* pred; const float* gt; const float* ratio; int P, G; float gt_min, pred_scale, lo, hi; double* part; };

__global__ void __launch_bounds__(ERR_THREADS) k_completion_errors(ErrorArgs a) {
    __shared__ double red[ERR_THREADS / 64][ERR_VALUES];
    const int g = blockIdx.x, n_img = blockIdx.y, t = threadIdx.x;
    const float* gt = a.gt + (long)n_img * a.P;
    const float* pred = a.pred + (long)n_img * a.P;
    const bool scaled = a.ratio != nullptr;
    const float ratio = scaled ? a.ratio[n_img] : 1.0f;
    double acc[ERR_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = g * ERR_THREADS + t; i < a.P; i += a.G * ERR_THREADS) {
        const float gv = gt[i];
        if (!(gv > a.gt_min)) continue;
        float p = pred[i] * a.pred_scale;                         // pred_depth *= pred_depth_scale_factor
        if (scaled) p = p * ratio;                                // pred_depth *= ratio
        p = p < a.lo ? a.lo : p;                                  // pred_depth[pred_depth < MIN_DEPTH] = MIN_DEPTH: a NaN stays
        p = p > a.hi ? a.hi : p;
        const float p_mm = p * 1000.0f, g_mm = gv * 1000.0f;
        const float dm = g_mm - p_mm;
        const float ip = 1.0f / (p * 0.001f), ig = 1.0f / (gv * 0.001f);
        const float di = ig - ip;
        acc[0] += (double)(dm * dm);
        acc[1] += (double)__builtin_fabsf(dm);
        acc[2] += (double)(di * di);
        acc[3] += (double)__builtin_fabsf(di);
        acc[4] += 1.0;
    }
#pragma unroll
    for (int v = 0; v < ERR_VALUES; ++v) {
        const double s = wave_sum_f64(acc[v]);
        if ((t & 63) == 0) red[t >> 6][v] = s;
    }
    __syncthreads();
    if (t < ERR_VALUES) {
        double s = 0.0;
        for (int w = 0; w < ERR_THREADS / 64; ++w) s += red[w][t];
        a.part[((long)n_img * a.G + g) * ERR_VALUES + t] = s;
    }
}

__global__ void k_completion_finish(const double* __restrict__ part, int N, int G, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double s[ERR_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < G; ++g)
        for (int v = 0; v < ERR_VALUES; ++v) s[v] += part[((long)i * G + g) * ERR_VALUES + v];
    double* o = out + (long)i * 5;
    const double n = s[4];                                        // 0 selected pixels: 0 / 0 = NaN, numpy's mean of nothing
    o[0] = sqrt(s[0] / n); o[1] = s[1] / n; o[2] = sqrt(s[2] / n); o[3] = s[3] / n; o[4] = n;
}

int check_planes(const char* who, const float* pred, const float* gt, int N, int H, int W) {
    FD_REQUIRE(pred && gt && N > 0 && N <= 65535 && H > 0 && W > 0, "%s: bad args", who);
    FD_REQUIRE((long)H * W < (1L << 30), "%s: %d x %d is too large for 32-bit pixel indices", who, H, W);
    return 0;
}

}  // namespace

extern "C" int fd_depth_png_keys(const uint16_t* packed, long packed_elems, const fd_depth_png_desc* desc, int S, int canvas_h,
                                 int canvas_w, int pool, int channels, float div0, float div1, float* out, void* stream) {
    FD_REQUIRE(packed && desc && out && packed_elems > 0 && S > 0 && S <= 65535 && canvas_h > 0 && canvas_w > 0, "fd_depth_png_keys: bad args");
    FD_REQUIRE((pool == 1 || pool == 2) && (channels == 1 || channels == 2), "fd_depth_png_keys: pool and channels are 1 or 2");
    FD_REQUIRE(div0 != 0.f && div1 != 0.f, "fd_depth_png_keys: a zero divisor");
    FD_REQUIRE((long)canvas_h * canvas_w < (1L << 30), "fd_depth_png_keys: canvas too large");
    FD_REQUIRE(((uintptr_t)packed & 7) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)desc & 7) == 0,
               "fd_depth_png_keys: packed and desc must be 8-byte aligned, out 16-byte aligned");
    const int oh = (canvas_h + pool - 1) / pool, ow = (canvas_w + pool - 1) / pool;
    const dim3 grid(fd_cdiv((long)oh * ow, 4 * 256), S);
    if (pool == 1)
        hipLaunchKernelGGL(k_depth_png_keys<1>, grid, dim3(256), 0, (hipStream_t)stream, packed, packed_elems, desc, canvas_h, canvas_w, oh,
                           ow, channels, div0, div1, out);
    else
        hipLaunchKernelGGL(k_depth_png_keys<2>, grid, dim3(256), 0, (hipStream_t)stream, packed, packed_elems, desc, canvas_h, canvas_w, oh,
                           ow, channels, div0, div1, out);
    FD_LAUNCH_CHECK("fd_depth_png_keys");
    return 0;
}

extern "C" long fd_completion_ws_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (long)H * W >= (1L << 30)) return 0;
    return (long)N * error_groups(H * W) * ERR_VALUES * (long)sizeof(double);
}

extern "C" int fd_completion_medians(const float* pred, const float* gt, int N, int H, int W, float gt_min, float pred_scale,
                                     float* out, void* ws, void* stream) {
    if (int rc = check_planes("fd_completion_medians", pred, gt, N, H, W)) return rc;
    FD_REQUIRE(out, "fd_completion_medians: out is NULL");
    (void)ws;                                                     // the medians need no scratch; the argument keeps the two calls alike
    MedianArgs a;
    a.pred = pred; a.gt = gt; a.P = H * W; a.gt_min = gt_min; a.pred_scale = pred_scale; a.out = out;
    hipLaunchKernelGGL(k_completion_median, dim3(2, N), dim3(1024), 0, (hipStream_t)stream, a);
    FD_LAUNCH_CHECK("fd_completion_medians");
    hipLaunchKernelGGL(k_completion_ratio, dim3(fd_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, out, N);
    FD_LAUNCH_CHECK("fd_completion_medians (ratio)");
    return 0;
}

extern "C" int fd_completion_errors(const float* pred, const float* gt, const float* ratio, int N, int H, int W, float gt_min,
                                    float pred_scale, float lo, float hi, double* out, void* ws, void* stream) {
    if (int rc = check_planes("fd_completion_errors", pred, gt, N, H, W)) return rc;
    FD_REQUIRE(out && ws && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0, "fd_completion_errors: out / ws missing or not 8-byte aligned");
    ErrorArgs a;
    a.pred = pred; a.gt = gt; a.ratio = ratio; a.P = H * W; a.G = error_groups(H * W);
    a.gt_min = gt_min; a.pred_scale = pred_scale; a.lo = lo; a.hi = hi; a.part = (double*)ws;
    hipLaunchKernelGGL(k_completion_errors, dim3(a.G, N), dim3(ERR_THREADS), 0, (hipStream_t)stream, a);
    FD_LAUNCH_CHECK("fd_completion_errors");
    hipLaunchKernelGGL(k_completion_finish, dim3(fd_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, (const double*)ws, N, a.G, out);
    FD_LAUNCH_CHECK("fd_completion_errors (finish)");
    return 0;
}
