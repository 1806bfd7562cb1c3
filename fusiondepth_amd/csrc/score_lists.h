// The device code the three per-image depth scorers share: fd_eigen_scores (eigen_eval.hip: the rules of evaluate_depth.py),
// fd_val_scores (val_scores.hip: the rules of the trainer's compute_depth_losses) and fd_completion_val_scores (completion_val.hip: the
// rules of the Completor's compute_depth_losses).  All select ground-truth pixels inside a window,
// evaluate a bilinear resample of the prediction at the selected pixels only, compact the (gt, pred) pairs in row-major order, take
// a median of each list by radix select and sum the float32 terms of the seven metrics in float64 over a fixed grid of partials.
// What differs is a compile-time RULE:
//   RULE_EIGEN  OpenCV's INTER_LINEAR resize of the DISPARITY, 1 / that, * pred_scale; numpy's median (an even count takes the
//               float32 mean of the two middle values).
//   RULE_VAL    ATen's CPU bilinear rule (align_corners=False, aten_resize.h) on the DEPTH, clamped to [lo, hi] before the median;
//               torch's median (the lower middle element, rank (n - 1) / 2).
//   RULE_COMPLETION  RULE_VAL's resample and medians; after the second clamp both sides are scaled to millimetres, g' = g * 1000.0f
//               and p' = p * 1000.0f (one float32 rounding each), and the seven terms are formed on g' and p' (completor.py:762).
// Launches, whatever N is:
//   1 k_score_rows<RULE, false>  one wave per window row of every image: how many pixels of the row are selected.
//   2 k_score_scan               one workgroup per image: where its compact lists start (the window areas of the images before it)
//                                and the exclusive scan of its row counts -> the start of every row in the lists, the image's count.
//   3 k_score_rows<RULE, true>   the count kernel's walk again; at each selected pixel, and only there, the RULE's resample from its
//                                four taps.  (gt, pred) go to row start + the number of selected lanes below this one (ballot +
//                                popcount): row-major order, no position depends on arrival.
//   4 k_score_median<RULE>       one workgroup per (image, list): completion.hip's radix select (4 passes of 8 bits, LDS histograms
//                                with integer atomics; RULE_EIGEN adds a fifth pass for the upper middle element of an even count)
//                                over the compact list, a few times 10^4 values, not over the plane.
//   5 k_score_errors<RULE>       ratio = median(gt) / median(pred) in float32, p = clamp(pred * ratio, lo, hi) and the terms of
//                                compute_errors / compute_depth_errors in float32, float64 sums: a fixed grid of workgroups per
//                                image, a fixed shuffle tree inside each, partials to the workspace.
//   6 k_score_finish             sums an image's partials in index order -> out[n][9].  No float atomics anywhere: run-to-run
//                                identical.
// Every float32 step is one rounding: contraction is off here and in the including files; the fused multiply-adds of ATen's rule
// are explicit fmaf calls.
// fd_eigen_class_scores (eigen_class.hip) adds two things to the six launches.  k_score_rows<RULE, true, true> also writes the label of
// each selected pixel to a uint8 list at the pair's index (the three scorers above leave the flag off: their kernels are unchanged).
// k_class_errors, one workgroup per (class, image), then walks the image's compact list, keeps the pairs whose label is its class and
// sums score_terms - the per-pixel arithmetic it shares with k_score_errors - through class_reduce.
#pragma once
#include "../../include/fdhip.h"
#include "fd_common.h"
#include "cv_resize.h"                                          // OpenCV's INTER_LINEAR coefficients (cv_linear_coeff)
#include "aten_resize.h"                                        // ATen's source-index rule (aten_src)

#pragma clang fp contract(off)

namespace {

enum ScoreRule { RULE_EIGEN = 0, RULE_VAL = 1, RULE_COMPLETION = 2 };

constexpr int ROW_WAVES = 4;                                      // window rows per workgroup of the count / compact kernels
constexpr int ERR_THREADS = 256;
constexpr int ERR_GROUPS = 32;                                    // partial sums per image
constexpr int ERR_VALUES = 7;                                     // abs_rel, sq_rel, sq, log sq, three threshold counts

struct ImageInfo { long base; int count; int ok; };               // where the image's lists start, how many pairs they hold

struct Args {
    const float* disp; int M, h, w;                               // the predictions: disparities (RULE_EIGEN) or depths (RULE_VAL)
    const float* packed; long packed_floats;
    const fd_eigen_desc* desc; int N, max_rows; long list_cap;
    float gt_lo, gt_hi, pred_scale, lo, hi; int median_scaling;
    int* rows;                                                    // [N][max_rows]: counts, then row starts
    ImageInfo* info;                                              // [N]
    float* med;                                                   // [N][2]: median(gt), median(pred)
    double* part;                                                 // [N][ERR_GROUPS][ERR_VALUES]
    float* gt_list; float* pred_list;                             // [list_cap] each
    double* out;
    // fd_eigen_class_scores alone (k_score_rows<.., true, true> and k_class_errors; nothing else reads them)
    const unsigned char* labels = nullptr;                        // label plane of image n at BYTE desc[n].offset, H x W, row-major
    unsigned char* label_list = nullptr;                          // [list_cap]: the label of the pair at the same index
    int K = 0;                                                    // classes; a label >= K belongs to none
    double* class_out = nullptr;                                  // [N][K][CLASS_VALUES]
};

__device__ __forceinline__ bool desc_ok(const fd_eigen_desc& d, const Args& a) {
    return d.H > 0 && d.W > 0 && d.offset >= 0 && d.offset <= a.packed_floats && (long)d.H * d.W <= a.packed_floats - d.offset &&
           (long)d.H * d.W < (1L << 30) && d.pred >= 0 && d.pred < a.M && d.y0 >= 0 && d.y0 <= d.y1 && d.y1 <= d.H && d.x0 >= 0 &&
           d.x0 <= d.x1 && d.x1 <= d.W && d.y1 - d.y0 <= a.max_rows;
}
__device__ __forceinline__ long window_area(const fd_eigen_desc& d, const Args& a) {
    return desc_ok(d, a) ? (long)(d.y1 - d.y0) * (d.x1 - d.x0) : 0;
}
__device__ __forceinline__ bool selected(float g, float gt_lo, float gt_hi, bool no_hi) { return g > gt_lo && (no_hi || g < gt_hi); }

// ---------------------------------------------------------------------------------------------- 1, 3: count and compact
template <int RULE, bool WRITE, bool LABELS = false>
__global__ void __launch_bounds__(ROW_WAVES * 64) k_score_rows(Args a) {
    static_assert(WRITE || !LABELS, "labels are written beside the pairs");
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const int r = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);    // wave-uniform
    const fd_eigen_desc d = a.desc[n];
    if (!desc_ok(d, a) || r >= d.y1 - d.y0) return;
    if (WRITE && !a.info[n].ok) return;                           // the lists of this image would leave the workspace
    const int y = d.y0 + r;
    const float* row = a.packed + d.offset + (long)y * d.W;
    const bool no_hi = a.gt_hi == __builtin_inff();
    const unsigned long long below = (1ull << lane) - 1ull;
    long at = 0;
    const float* dp = nullptr;
    const unsigned char* lrow = nullptr;                          // byte loads: a plane starts at any address
    int ya = 0, yb = 0;
    float b0 = 0.f, b1 = 0.f;
    double sx = 0.0;                                              // RULE_EIGEN: OpenCV's scale, a double
    float sxf = 0.f;                                              // RULE_VAL: ATen's scale, a float
    if (WRITE) {
        at = a.info[n].base + a.rows[(long)n * a.max_rows + r];
        dp = a.disp + (long)d.pred * a.h * a.w;
        if (LABELS) lrow = a.labels + d.offset + (long)y * d.W;
        if (RULE == RULE_EIGEN) {
            cv_linear_coeff(y, (double)a.h / (double)d.H, a.h, ya, yb, b0, b1);
            sx = (double)a.w / (double)d.W;
        } else {
            aten_src(y, (float)a.h / (float)d.H, a.h, ya, yb, b0, b1);
            sxf = (float)a.w / (float)d.W;
        }
    }
    int count = 0;
    for (int x0 = d.x0; x0 < d.x1; x0 += 64) {                    // the trip count is wave-uniform: ballots see all 64 lanes
        const int x = x0 + lane;
        const float g = x < d.x1 ? row[x] : 0.f;
        const bool sel = x < d.x1 && selected(g, a.gt_lo, a.gt_hi, no_hi);
        const unsigned long long m = __ballot(sel);
        if (WRITE && sel) {
            int xa, xb;
            float a0, a1;
            float depth;
            if (RULE == RULE_EIGEN) {
                cv_linear_coeff(x, sx, a.w, xa, xb, a0, a1);
                const float r0 = dp[ya * a.w + xa] * a0 + dp[ya * a.w + xb] * a1;
                const float r1 = dp[yb * a.w + xa] * a0 + dp[yb * a.w + xb] * a1;
                const float dv = r0 * b0 + r1 * b1;
                depth = (1.0f / dv) * a.pred_scale;
            } else {
                aten_src(x, sxf, a.w, xa, xb, a0, a1);            // the blend runs width first (fdhip.h, fd_resize_bilinear_batch)
                const float top = __builtin_fmaf(a0, dp[ya * a.w + xa], a1 * dp[ya * a.w + xb]);
                const float bot = __builtin_fmaf(a0, dp[yb * a.w + xa], a1 * dp[yb * a.w + xb]);
                depth = __builtin_fmaf(b0, top, b1 * bot);
                depth = depth < a.lo ? a.lo : depth;              // torch.clamp(.., lo, hi) before the median: a NaN stays
                depth = depth > a.hi ? a.hi : depth;
            }
            const long i = at + count + __popcll(m & below);
            a.gt_list[i] = g;
            a.pred_list[i] = depth;
            if (LABELS) a.label_list[i] = lrow[x];
        }
        count += __popcll(m);
    }
    if (!WRITE && lane == 0) a.rows[(long)n * a.max_rows + r] = count;
}

// ---------------------------------------------------------------------------------------------- 2: scan
__global__ void __launch_bounds__(1024) k_score_scan(Args a) {
    __shared__ long red[1024];
    const int n = blockIdx.x, t = threadIdx.x;
    long mine = 0;
    for (int i = t; i < n; i += 1024) mine += window_area(a.desc[i], a);
    red[t] = mine;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {                           // integer sums: any order gives the same value
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const long base = red[0];
    __syncthreads();
    const fd_eigen_desc d = a.desc[n];
    const bool ok = desc_ok(d, a) && base + window_area(d, a) <= a.list_cap;
    const int R = ok ? d.y1 - d.y0 : 0;
    int* rows = a.rows + (long)n * a.max_rows;
    const int per = (R + 1023) / 1024;                            // consecutive rows per thread
    const int r0 = t * per, r1 = r0 + per < R ? r0 + per : R;
    long sum = 0;
    for (int r = r0; r < r1; ++r) sum += rows[r];
    red[t] = sum;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {                          // inclusive scan over the threads' sums
        const long v = t >= s ? red[t - s] : 0;
        __syncthreads();
        red[t] += v;
        __syncthreads();
    }
    long run = red[t] - sum;
    for (int r = r0; r < r1; ++r) {
        const int c = rows[r];
        rows[r] = (int)run;
        run += c;
    }
    if (t == 1023) {
        ImageInfo o;
        o.base = base; o.count = (int)red[1023]; o.ok = ok ? 1 : 0;
        a.info[n] = o;
    }
}

// ---------------------------------------------------------------------------------------------- 4: medians
__device__ __forceinline__ unsigned key_of(float v) {     // order-preserving: a < b  <=>  key(a) < key(b)  (as in completion.hip)
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}

// blockIdx.x: 0 = the gt list, 1 = the pred list; blockIdx.y: image
template <int RULE>
__global__ void __launch_bounds__(1024) k_score_median(Args a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[2];
    __shared__ int nan_seen;
    const int which = blockIdx.x, n_img = blockIdx.y, t = threadIdx.x;
    const ImageInfo info = a.info[n_img];
    float* o = a.med + 2 * n_img + which;
    const int n = info.ok ? info.count : 0;
    if (n == 0) {                                                 // the median of an empty selection: NaN (uniform exit)
        if (t == 0) *o = __builtin_nanf("");
        return;
    }
    const float* v = (which ? a.pred_list : a.gt_list) + info.base;
    if (t == 0) nan_seen = 0;
    unsigned prefix = 0, mask = 0;
    unsigned rank = (unsigned)(n - 1) / 2;                        // rank of the lower middle element
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256) hist[t] = 0;
        __syncthreads();
        for (int i = t; i < n; i += 1024) {
            const float x = v[i];
            if (x != x) nan_seen = 1;
            const unsigned key = key_of(x);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t == 0) {
            unsigned left = rank, bin = 0;
            for (; bin < 255; ++bin) {
                if (left < hist[bin]) break;
                left -= hist[bin];
            }
            sh[0] = bin; sh[1] = left;
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        mask |= 255u << shift;
        rank = sh[1];
        __syncthreads();
    }
    const unsigned lower = prefix;
    unsigned upper = lower;
    const bool two = RULE == RULE_EIGEN && (n & 1) == 0;          // np.median of an even count; torch.median stays at the lower one
    if (two) {                                                    // the element of rank n / 2
        if (t == 0) { sh[0] = 0u; sh[1] = 0xffffffffu; }
        __syncthreads();
        unsigned le = 0, above = 0xffffffffu;
        for (int i = t; i < n; i += 1024) {
            const unsigned key = key_of(v[i]);
            if (key <= lower) ++le;
            else above = key < above ? key : above;
        }
        atomicAdd(&sh[0], le);
        atomicMin(&sh[1], above);
        __syncthreads();
        upper = (int)sh[0] >= n / 2 + 1 ? lower : sh[1];
    }
    if (t == 0) {
        const float lo = value_of(lower), hi = value_of(upper);
        // np.median: the float32 mean of the middle element(s) - (lo + hi) rounded to float32, then halved
        *o = nan_seen ? __builtin_nanf("") : (two ? (lo + hi) / 2.0f : lo);
    }
}

// ---------------------------------------------------------------------------------------------- 5, 6: errors
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, FD_WAVE);
    return v;
}

// The terms of one (gt, pred) pair, added to acc: the per-pixel arithmetic of k_score_errors and k_class_errors.
template <int RULE>
__device__ __forceinline__ void score_terms(float gv, float p, bool scaled, float ratio, float lo, float hi, double (&acc)[ERR_VALUES]) {
    if (scaled) p = p * ratio;                                    // pred_depth *= ratio
    p = p < lo ? lo : p;                                          // pred_depth[pred_depth < MIN_DEPTH] = MIN_DEPTH: a NaN stays
    p = p > hi ? hi : p;
    if (RULE == RULE_COMPLETION) {                                // compute_depth_errors(gt * 1000.0, pred * 1000.0): millimetres
        gv = gv * 1000.0f;
        p = p * 1000.0f;
    }
    const float q0 = gv / p, q1 = p / gv;
    float th = q0 > q1 ? q0 : q1;                                 // np.maximum / torch.max: a NaN on either side gives NaN
    if (q0 != q0 || q1 != q1) th = __builtin_nanf("");
    const float df = gv - p;
    const float sq = df * df;
    // the logarithms in float64, their difference rounded once; numpy's float32 log is not correctly rounded (fdhip.h)
    const float dl = (float)(log((double)gv) - log((double)p));
    acc[0] += (double)(__builtin_fabsf(df) / gv);
    acc[1] += (double)(sq / gv);
    acc[2] += (double)sq;
    acc[3] += (double)(dl * dl);
    acc[4] += th < 1.25f ? 1.0 : 0.0;
    acc[5] += th < 1.5625f ? 1.0 : 0.0;                           // 1.25 ** 2 and 1.25 ** 3 are exact in float32
    acc[6] += th < 1.953125f ? 1.0 : 0.0;
}

template <int RULE>
__global__ void __launch_bounds__(ERR_THREADS) k_score_errors(Args a) {
    __shared__ double red[ERR_THREADS / 64][ERR_VALUES];
    const int g = blockIdx.x, n_img = blockIdx.y, t = threadIdx.x;
    const ImageInfo info = a.info[n_img];
    const int n = info.ok ? info.count : 0;
    const float* gl = a.gt_list + info.base;
    const float* pl = a.pred_list + info.base;
    const bool scaled = a.median_scaling != 0;
    const float ratio = scaled ? a.med[2 * n_img] / a.med[2 * n_img + 1] : 1.0f;
    double acc[ERR_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = g * ERR_THREADS + t; i < n; i += ERR_GROUPS * ERR_THREADS) score_terms<RULE>(gl[i], pl[i], scaled, ratio, a.lo, a.hi, acc);
#pragma unroll
    for (int v = 0; v < ERR_VALUES; ++v) {
        const double s = wave_sum_f64(acc[v]);
        if ((t & 63) == 0) red[t >> 6][v] = s;
    }
    __syncthreads();
    if (t < ERR_VALUES) {
        double s = 0.0;
        for (int w = 0; w < ERR_THREADS / 64; ++w) s += red[w][t];
        a.part[((long)n_img * ERR_GROUPS + g) * ERR_VALUES + t] = s;
    }
}

__global__ void k_score_finish(Args a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N) return;
    double s[ERR_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < ERR_GROUPS; ++g)
        for (int v = 0; v < ERR_VALUES; ++v) s[v] += a.part[((long)i * ERR_GROUPS + g) * ERR_VALUES + v];
    const ImageInfo info = a.info[i];
    double* o = a.out + (long)i * 9;
    const double n = info.ok ? (double)info.count : 0.0;          // 0 selected pixels: 0 / 0 = NaN, the mean of nothing
    o[0] = s[0] / n; o[1] = s[1] / n; o[2] = sqrt(s[2] / n); o[3] = sqrt(s[3] / n);
    o[4] = s[4] / n; o[5] = s[5] / n; o[6] = s[6] / n;
    o[7] = a.median_scaling ? (double)(a.med[2 * i] / a.med[2 * i + 1]) : (double)__builtin_nanf("");
    o[8] = info.ok ? n : -1.0;
}

// ---------------------------------------------------------------------------------------------- 7: per-class errors
constexpr int CLASS_THREADS = 256;                                // T: thread t takes pairs t, t + T, ...
constexpr int CLASS_VALUES = 8;                                   // abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, count
constexpr int CLASS_AHEAD = 16;                                   // steps whose loads a thread issues together

// One workgroup sums the pairs of gl / pl [0, n) whose label is c and writes o[0 .. 8).  Each thread adds its pairs in index order,
// the lanes of a wave add through wave_sum_f64's tree, thread 0 .. 7 adds the waves in wave order: the result is a function of the
// lists alone, by whichever entry point they arrive.  No pair of class c: eight zeros (the reference's np.zeros(7), count 0).
template <int RULE>
__device__ __forceinline__ void class_reduce(const float* gl, const float* pl, const unsigned char* ll, long n, int c, bool scaled,
                                             float ratio, float lo, float hi, double* o) {
    __shared__ double red[CLASS_THREADS / 64][CLASS_VALUES];
    const int t = threadIdx.x;
    double acc[ERR_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    // One label in K fits, so in a step some lane of a wave nearly always has a pair and a wave that took the steps one by one would
    // pay for a memory round trip and for the terms (two float64 logarithms) in almost every step.  Instead the loads of CLASS_AHEAD
    // steps are issued together - labels, and gt and pred whether or not the label fits: coalesced reads of lists that lie in the
    // L2 - and then each thread takes ITS fitting pairs in index order, all lanes at once: a wave forms the terms as often as its
    // busiest lane has pairs among these steps (2 or 3 times in 16), and every thread still adds pairs t, t + T, ... in that order.
    for (long i = t; i < n; i += CLASS_AHEAD * CLASS_THREADS) {
        float gv[CLASS_AHEAD], pv[CLASS_AHEAD];
        unsigned fits = 0;
#pragma unroll
        for (int k = 0; k < CLASS_AHEAD; ++k) {
            const long at = i + (long)k * CLASS_THREADS;
            const bool in = at < n;
            if (in && (int)ll[at] == c) fits |= 1u << k;
            gv[k] = in ? gl[at] : 0.f;
            pv[k] = in ? pl[at] : 0.f;
        }
        while (fits) {
            const int k = __builtin_ctz(fits);
            fits &= fits - 1;
            float g = gv[0], p = pv[0];
#pragma unroll
            for (int j = 1; j < CLASS_AHEAD; ++j) {               // selects, not an indexed array: the values stay in registers
                g = k == j ? gv[j] : g;
                p = k == j ? pv[j] : p;
            }
            score_terms<RULE>(g, p, scaled, ratio, lo, hi, acc);
            cnt += 1.0;
        }
    }
#pragma unroll
    for (int v = 0; v < ERR_VALUES; ++v) {
        const double s = wave_sum_f64(acc[v]);
        if ((t & 63) == 0) red[t >> 6][v] = s;
    }
    const double s = wave_sum_f64(cnt);
    if ((t & 63) == 0) red[t >> 6][ERR_VALUES] = s;
    __syncthreads();
    if (t < CLASS_VALUES) {
        double v = 0.0, m = 0.0;                                  // m: the class's count, a sum of integers
        for (int w = 0; w < CLASS_THREADS / 64; ++w) {
            v += red[w][t];
            m += red[w][ERR_VALUES];
        }
        if (t < ERR_VALUES) {
            v = m > 0.0 ? v / m : 0.0;
            if (t == 2 || t == 3) v = sqrt(v);
        }
        o[t] = v;
    }
}

// blockIdx.x: class; blockIdx.y: image
template <int RULE>
__global__ void __launch_bounds__(CLASS_THREADS) k_class_errors(Args a) {
    const int c = blockIdx.x, n_img = blockIdx.y;
    const ImageInfo info = a.info[n_img];
    const int n = info.ok ? info.count : 0;                       // a refused image: zero rows
    const bool scaled = a.median_scaling != 0;
    const float ratio = scaled ? a.med[2 * n_img] / a.med[2 * n_img + 1] : 1.0f;
    class_reduce<RULE>(a.gt_list + info.base, a.pred_list + info.base, a.label_list + info.base, n, c, scaled, ratio, a.lo, a.hi,
                       a.class_out + ((long)n_img * a.K + c) * CLASS_VALUES);
}

// The class kernel on lists that are already matched and scaled (fd_class_errors): pred is clamped, nothing else.
__global__ void __launch_bounds__(CLASS_THREADS) k_class_errors_lists(const float* gt, const float* pred, const unsigned char* labels, long n,
                                                                      float lo, float hi, double* class_out) {
    class_reduce<RULE_EIGEN>(gt, pred, labels, n, blockIdx.x, false, 1.0f, lo, hi, class_out + (long)blockIdx.x * CLASS_VALUES);
}

// ---------------------------------------------------------------------------------------------- host side
inline long align8(long v) { return (v + 7) & ~7L; }

struct Layout { long part, info, med, rows, gt_list, pred_list, total; };

inline Layout layout(int N, int max_rows, long list_cap) {
    Layout l;
    l.part = 0;
    l.info = l.part + (long)N * ERR_GROUPS * ERR_VALUES * (long)sizeof(double);
    l.med = l.info + (long)N * (long)sizeof(ImageInfo);
    l.rows = align8(l.med + (long)N * 2 * (long)sizeof(float));
    l.gt_list = align8(l.rows + (long)N * max_rows * (long)sizeof(int));
    l.pred_list = align8(l.gt_list + list_cap * (long)sizeof(float));
    l.total = align8(l.pred_list + list_cap * (long)sizeof(float));
    return l;
}

inline bool sizes_ok(int N, int max_rows, long list_cap) {
    return N >= 1 && N <= 4096 && max_rows >= 0 && max_rows <= (1 << 20) && list_cap >= 0 && list_cap < (1L << 40);
}

// The workspace pointers of `a` from its sizes.
inline void place(Args& a, void* ws) {
    const Layout l = layout(a.N, a.max_rows, a.list_cap);
    char* base = (char*)ws;
    a.part = (double*)(base + l.part); a.info = (ImageInfo*)(base + l.info); a.med = (float*)(base + l.med);
    a.rows = (int*)(base + l.rows); a.gt_list = (float*)(base + l.gt_list); a.pred_list = (float*)(base + l.pred_list);
}

// The launches of one call; `names` = the six texts FD_LAUNCH_CHECK reports (count, scan, compact, medians, errors, finish), and a
// seventh (classes) with LABELS: the compact launch then writes the label list too, and the class kernel follows the finish.
template <int RULE, bool LABELS = false>
inline int launch_scores(const Args& a, hipStream_t st, const char* const* names) {
    const dim3 row_grid(a.max_rows > 0 ? fd_cdiv(a.max_rows, ROW_WAVES) : 1, a.N);
    hipLaunchKernelGGL((k_score_rows<RULE, false>), row_grid, dim3(ROW_WAVES * 64), 0, st, a);
    FD_LAUNCH_CHECK(names[0]);
    hipLaunchKernelGGL(k_score_scan, dim3(a.N), dim3(1024), 0, st, a);
    FD_LAUNCH_CHECK(names[1]);
    hipLaunchKernelGGL((k_score_rows<RULE, true, LABELS>), row_grid, dim3(ROW_WAVES * 64), 0, st, a);
    FD_LAUNCH_CHECK(names[2]);
    if (a.median_scaling) {
        hipLaunchKernelGGL((k_score_median<RULE>), dim3(2, a.N), dim3(1024), 0, st, a);
        FD_LAUNCH_CHECK(names[3]);
    }
    hipLaunchKernelGGL((k_score_errors<RULE>), dim3(ERR_GROUPS, a.N), dim3(ERR_THREADS), 0, st, a);
    FD_LAUNCH_CHECK(names[4]);
    hipLaunchKernelGGL(k_score_finish, dim3(fd_cdiv(a.N, 64)), dim3(64), 0, st, a);
    FD_LAUNCH_CHECK(names[5]);
    if (LABELS) {
        hipLaunchKernelGGL((k_class_errors<RULE>), dim3(a.K, a.N), dim3(CLASS_THREADS), 0, st, a);
        FD_LAUNCH_CHECK(names[6]);
    }
    return 0;
}

}  // namespace
