// The two pictures of evaluate_depth.py --visualize ("fd_vis_render"; include/fdhip.h): lines :407-449 for N maps of different sizes
// packed back to back, in at most NINE launches and one memset whatever N is.
//   1 k_vis_depth    the dense depth map of every image into the staging planes (the caller's depth_out, or the workspace):
//                    fd_depth_export's chain through cv_resize.h - resize, 1 / ., * pred_scale, * ratio[n] - or a copy of depth_in
//                    when the caller asks for it back.  Skipped where depth_in is read in place.
//   2-6 k_vis_select<0 .. 4>  vmin = min d' and vmax = np.percentile(d', 95), d' = 1 / depth, by a radix select over the WHOLE plane
//                    (score_lists.h's select, spread over up to 64 workgroups per image so that one map alone still fills the
//                    device).  Four passes of 8 bits find the order statistic of rank k: every workgroup counts its share in LDS (the
//                    histogram in eight copies: the keys of a depth map share their top byte, and 64 lanes on one LDS counter
//                    serialise) and adds it to the image's global histogram; the next launch reads the finished histogram.  A
//                    fifth pass finds rank k + 1 (the count of keys <= sorted[k], the smallest key above) and the minimum.  Integer
//                    atomics only, so the sums do not depend on the order or on the number of workgroups: two calls give the same bits.
//   7 k_vis_stats    (vmin, vmax) per image: numpy's _lerp.
//   8 k_vis_color    matplotlib's Normalize and colormap lookup per pixel, lut_disp[index] as three bytes.
//   9 k_vis_error    |depth - gt| through lut_err at the scorer's selected() pixels, the 2 x 2 maximum, grey 220 where nothing scored.
// Stores (8, 9): a picture [H, W, 3] of bytes is one contiguous run per image, so a thread owns one 16-byte chunk of it - the six
// pixels that touch it, packed for its phase (chunk start mod 3) - and writes one uint4; the bytes before the first 16-byte boundary
// of the ADDRESS and after the last whole chunk are written one by one by the first workgroup.
// Every float32 step is one rounding, as numpy does it: contraction is off for the whole file.
#include "../../include/fdhip.h"
#include "fd_common.h"
#include "cv_resize.h"

#pragma clang fp contract(off)

namespace {

constexpr int VIS_THREADS = 256;
constexpr int SEL_THREADS = 256;                                   // one thread per histogram bin
constexpr int SEL_PER_GROUP = 8192;                               // values per workgroup of a select pass
constexpr int SEL_MAX_GROUPS = 64;
constexpr int SEL_COPIES = 8;                                     // copies of the 256-bin histogram, chosen by lane & 7
constexpr int VIS_MAX_N = 64;

struct VisArgs {
    const float* disp; int M, h, w;
    float pred_scale; const float* ratio;
    const float* depth_in;
    float* depth;                                                 // staging planes (depth_out or workspace); null: depth_in in place
    const float* gt; long packed_floats;
    const fd_eigen_desc* desc; int N;
    float gt_lo, gt_hi;
    const unsigned char* lut_disp; const unsigned char* lut_err;
    unsigned char* color; unsigned char* err; long err_pixels;
    float* stats;                                                 // [N][2]: vmin, vmax (the caller's, or the workspace)
    unsigned* sel_hist;                                           // [4][N][256]: the global histogram of every select pass
    unsigned* sel_fin;                                            // [N][4]: keys <= sorted[k], ~(smallest key above), ~(smallest key)
    uint2* sel_state;                                             // [5][N]: (prefix, remaining rank) at the start of every pass
};

__device__ __forceinline__ bool vis_desc_ok(const fd_eigen_desc& d, const VisArgs& a) {
    return d.H > 0 && d.W > 0 && d.offset >= 0 && d.offset <= a.packed_floats && (long)d.H * d.W <= a.packed_floats - d.offset &&
           (long)d.H * d.W < (1L << 30) && (a.depth_in || (d.pred >= 0 && d.pred < a.M)) && d.y0 >= 0 && d.y0 <= d.y1 && d.y1 <= d.H &&
           d.x0 >= 0 && d.x0 <= d.x1 && d.x1 <= d.W;
}
__device__ __forceinline__ const float* vis_src(const VisArgs& a) { return a.depth ? a.depth : a.depth_in; }

// ---------------------------------------------------------------------------------------------- 1: the depth maps
__global__ void __launch_bounds__(VIS_THREADS) k_vis_depth(VisArgs a) {
    const int n = blockIdx.y;
    const fd_eigen_desc d = a.desc[n];
    if (!vis_desc_ok(d, a)) return;
    const int P = d.H * d.W;
    float* out = a.depth + d.offset;
    if (a.depth_in) {
        for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < P; p += gridDim.x * VIS_THREADS) out[p] = a.depth_in[d.offset + p];
        return;
    }
    const float* src = a.disp + (long)d.pred * a.h * a.w;
    const double sx = (double)a.w / (double)d.W, sy = (double)a.h / (double)d.H;
    const bool scaled = a.ratio != nullptr;
    const float ratio = scaled ? a.ratio[n] : 1.0f;
    for (int p = blockIdx.x * VIS_THREADS + threadIdx.x; p < P; p += gridDim.x * VIS_THREADS) {
        const int y = p / d.W, x = p - y * d.W;
        int x0, x1, y0, y1;
        float a0, a1, b0, b1;
        cv_linear_coeff(x, sx, a.w, x0, x1, a0, a1);
        cv_linear_coeff(y, sy, a.h, y0, y1, b0, b1);
        const float dv = cv_linear_pixel(src + (long)y0 * a.w, src + (long)y1 * a.w, x0, x1, a0, a1, b0, b1);
        float v = (1.0f / dv) * a.pred_scale;                     // fd_depth_export's steps, one rounding each
        if (scaled) v = v * ratio;
        out[p] = v;
    }
}

// ---------------------------------------------------------------------------------------------- 2: minimum and percentile
__device__ __forceinline__ unsigned vis_key(float v) {            // order-preserving, as score_lists.h's key_of
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vis_value(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}

// The virtual index of numpy 2's percentile for n float32 values: (n - 1) * q with q = float32(0.95), all in float32.
__device__ __forceinline__ void vis_rank(int n, int& k, int& k1, float& g) {
    const float q = 95.0f / 100.0f;
    const float pos = (float)(n - 1) * q;
    const float kf = floorf(pos);
    g = pos - kf;
    k = (int)kf;
    k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
    k1 = k + 1 < n ? k + 1 : n - 1;
}

// One pass of the select, gridDim.x workgroups per image (blockIdx.y).  PASS 0 .. 3: the histogram of byte 3 - PASS of the keys that
// share the prefix found so far, summed in LDS and added to the image's global histogram of this pass.  PASS 4: with the whole key of
// rank k known, how many keys are <= it, the smallest key above it and the smallest key of all.  Every pass begins by deriving its
// prefix and remaining rank from the pass before (its entry state and its finished global histogram: a launch boundary lies between);
// every workgroup derives the same, workgroup 0 records it for the next pass.  Integer atomics only.
template <int PASS>
__global__ void __launch_bounds__(SEL_THREADS) k_vis_select(VisArgs a) {
    __shared__ unsigned hist[SEL_COPIES][256];
    __shared__ unsigned scan[256];
    __shared__ unsigned sh[3];
    const int n_img = blockIdx.y, t = threadIdx.x;
    const fd_eigen_desc d = a.desc[n_img];
    if (!vis_desc_ok(d, a)) return;                               // uniform
    const int n = d.H * d.W;
    const float* v = vis_src(a) + d.offset;
    unsigned prefix = 0, rank = 0;
    if (PASS == 0) {
        int k, k1;
        float g;
        vis_rank(n, k, k1, g);
        rank = (unsigned)k;
    } else {
        const uint2 before = a.sel_state[(PASS - 1) * a.N + n_img];
        const unsigned c = a.sel_hist[((long)(PASS - 1) * a.N + n_img) * 256 + t];
        scan[t] = c;
        if (t == 0) { sh[0] = 255u; sh[1] = 0u; }
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {                       // inclusive scan of the 256 counts
            const unsigned add = t >= s ? scan[t - s] : 0u;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const unsigned incl = scan[t];
        if (incl > before.y && incl - c <= before.y) { sh[0] = (unsigned)t; sh[1] = before.y - (incl - c); }   // one thread: the bin of the rank
        __syncthreads();
        prefix = before.x | (sh[0] << (32 - 8 * PASS));
        rank = sh[1];
        __syncthreads();
    }
    if (blockIdx.x == 0 && t == 0) a.sel_state[PASS * a.N + n_img] = make_uint2(prefix, rank);
    const int stride = gridDim.x * SEL_THREADS;
    if (PASS < 4) {
        constexpr int shift = 24 - 8 * (PASS < 4 ? PASS : 0);
        const unsigned mask = PASS == 0 ? 0u : 0xffffffffu << (32 - 8 * PASS);
        unsigned* mine = hist[t & (SEL_COPIES - 1)];
        for (int i = t; i < SEL_COPIES * 256; i += SEL_THREADS) (&hist[0][0])[i] = 0;
        __syncthreads();
        for (int i = blockIdx.x * SEL_THREADS + t; i < n; i += stride) {
            const unsigned key = vis_key(1.0f / v[i]);
            if ((key & mask) == prefix) atomicAdd(&mine[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned s = 0;                                           // integer sums: any order gives the same value
#pragma unroll
        for (int c = 0; c < SEL_COPIES; ++c) s += hist[c][t];
        if (s) atomicAdd(&a.sel_hist[((long)PASS * a.N + n_img) * 256 + t], s);
    } else {
        const unsigned lower = prefix;                            // the key of sorted[k]
        if (t == 0) { sh[0] = 0u; sh[1] = 0u; sh[2] = 0u; }
        __syncthreads();
        unsigned le = 0, above = 0u, least = 0u;                  // the two minima as maxima of ~key: zero is their neutral start
        for (int i = blockIdx.x * SEL_THREADS + t; i < n; i += stride) {
            const unsigned key = vis_key(1.0f / v[i]);
            if (key <= lower) ++le;
            else above = ~key > above ? ~key : above;
            least = ~key > least ? ~key : least;
        }
        atomicAdd(&sh[0], le);
        atomicMax(&sh[1], above);
        atomicMax(&sh[2], least);
        __syncthreads();
        if (t == 0) {
            unsigned* fin = a.sel_fin + 4 * n_img;
            atomicAdd(&fin[0], sh[0]);
            atomicMax(&fin[1], sh[1]);
            atomicMax(&fin[2], sh[2]);
        }
    }
}

// (vmin, vmax) of every image from the select's results: numpy's _lerp, float32 throughout.
__global__ void k_vis_stats(VisArgs a) {
    const int n_img = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_img >= a.N) return;
    const fd_eigen_desc d = a.desc[n_img];
    if (!vis_desc_ok(d, a)) return;
    int k, k1;
    float g;
    vis_rank(d.H * d.W, k, k1, g);
    const unsigned lower = a.sel_state[4 * a.N + n_img].x;
    const unsigned* fin = a.sel_fin + 4 * n_img;
    const unsigned upper = (k1 == k || fin[0] >= (unsigned)k + 2u) ? lower : ~fin[1];
    const float lo = vis_value(lower), hi = vis_value(upper);
    const float diff = hi - lo;
    float vmax = lo + diff * g;
    if (g >= 0.5f) vmax = hi - diff * (1.0f - g);
    if (lo == hi) vmax = lo;
    a.stats[2 * n_img] = vis_value(~fin[2]);
    a.stats[2 * n_img + 1] = vmax;
}

// ---------------------------------------------------------------------------------------------- 3, 4: the pictures
// Sixteen bytes of a picture whose chunk starts at byte 3 * p0 + R: byte i belongs to pixel (R + i) / 3, channel (R + i) % 3;
// c[j] holds pixel p0 + j as r | g << 8 | b << 16.
template <int R>
__device__ __forceinline__ uint4 vis_pack16(const unsigned (&c)[6]) {
    unsigned wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = (R + i) / 3, ch = (R + i) - 3 * j;
        wd[i >> 2] |= ((c[j] >> (8 * ch)) & 255u) << (8 * (i & 3));
    }
    return make_uint4(wd[0], wd[1], wd[2], wd[3]);
}

// One image's picture of `pixels` pixels at `out`: `colour(p)` gives pixel p as r | g << 8 | b << 16.
template <class F>
__device__ __forceinline__ void vis_write_picture(unsigned char* out, int pixels, F colour) {
    const long total = 3L * pixels;
    long head = (long)((16u - (unsigned)((uintptr_t)out & 15u)) & 15u);
    head = head < total ? head : total;
    const long chunks = (total - head) / 16;
    const long tail = head + 16 * chunks;                         // first byte after the last whole chunk
    if (blockIdx.x == 0 && threadIdx.x < 32) {                    // the head and the tail: fewer than 16 bytes each
        const long b = threadIdx.x < 16 ? (long)threadIdx.x : tail + (threadIdx.x - 16);
        const bool in = threadIdx.x < 16 ? b < head : b < total;
        if (in) {
            const int p = (int)(b / 3), ch = (int)(b - 3L * p);
            out[b] = (unsigned char)((colour(p) >> (8 * ch)) & 255u);
        }
    }
    for (long ck = (long)blockIdx.x * VIS_THREADS + threadIdx.x; ck < chunks; ck += (long)gridDim.x * VIS_THREADS) {
        const long b0 = head + 16 * ck;
        const int p0 = (int)(b0 / 3), r = (int)(b0 - 3L * p0);
        unsigned c[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int p = p0 + j;                                 // pixels 0 .. (r + 15) / 3 = 5 touch the chunk; all lie in the picture
            c[j] = p < pixels ? colour(p) : 0u;
        }
        const uint4 q = r == 0 ? vis_pack16<0>(c) : (r == 1 ? vis_pack16<1>(c) : vis_pack16<2>(c));
        *reinterpret_cast<uint4*>(out + b0) = q;
    }
}

__device__ __forceinline__ void vis_load_lut(unsigned* lut, const unsigned char* src) {
    for (int i = threadIdx.x; i < 256; i += VIS_THREADS)
        lut[i] = (unsigned)src[3 * i] | ((unsigned)src[3 * i + 1] << 8) | ((unsigned)src[3 * i + 2] << 16);
    __syncthreads();
}

__global__ void __launch_bounds__(VIS_THREADS) k_vis_color(VisArgs a) {
    __shared__ unsigned lut[256];
    const int n = blockIdx.y;
    const fd_eigen_desc d = a.desc[n];
    if (!vis_desc_ok(d, a)) return;                               // uniform
    vis_load_lut(lut, a.lut_disp);
    const float* v = vis_src(a) + d.offset;
    const float vmin = a.stats[2 * n], vmax = a.stats[2 * n + 1];
    // matplotlib holds the limits as float64 scalars: the difference d' - vmin is rounded to float32 once (the float64 difference of
    // two float32 values is exact), the quotient is formed in float64 and rounded to float32 once
    const double den = (double)vmax - (double)vmin;
    const bool flat = vmin == vmax;
    vis_write_picture(a.color + 3 * d.offset, d.H * d.W, [&](int p) -> unsigned {
        const float dp = 1.0f / v[p];
        const float xn = flat ? 0.0f : (float)((double)(dp - vmin) / den);
        const float xa = xn * 256.0f;
        int idx = 0;                                              // NaN, negative: under -> entry 0
        if (xa >= 256.0f) idx = 255;                              // xa == N -> N - 1; above: over -> the last entry
        else if (xa > 0.0f) idx = (int)xa;
        if (!(__builtin_fabsf(dp) < __builtin_inff())) idx = 0;   // a non-finite d': in bounds, entry 0
        return lut[idx];
    });
}

__global__ void __launch_bounds__(VIS_THREADS) k_vis_error(VisArgs a) {
    __shared__ unsigned lut[256];
    const int n = blockIdx.y;
    const fd_eigen_desc d = a.desc[n];
    if (!vis_desc_ok(d, a)) return;                               // uniform
    long at = 0;                                                  // the pictures lie back to back: the pixels of those before this one
    for (int i = 0; i < n; ++i) {
        const fd_eigen_desc e = a.desc[i];
        if (vis_desc_ok(e, a)) at += (long)((e.H + 1) / 2) * ((e.W + 1) / 2);
    }
    const int H2 = (d.H + 1) / 2, W2 = (d.W + 1) / 2;
    if (at + (long)H2 * W2 > a.err_pixels) return;
    vis_load_lut(lut, a.lut_err);
    const float* v = vis_src(a) + d.offset;
    const float* gt = a.gt + d.offset;
    const bool no_hi = a.gt_hi == __builtin_inff();
    vis_write_picture(a.err + 3 * at, H2 * W2, [&](int p) -> unsigned {
        const int oy = p / W2, ox = p - oy * W2;
        unsigned m0 = 0u, m1 = 0u, m2 = 0u;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * oy + dy, x = 2 * ox + dx;       // beyond an odd edge: 0, as block_reduce pads
                if (y < d.y0 || y >= d.y1 || x < d.x0 || x >= d.x1) continue;
                const float g = gt[y * d.W + x];
                if (!(g > a.gt_lo && (no_hi || g < a.gt_hi))) continue;       // the scorer's selected()
                float df = __builtin_fabsf(v[y * d.W + x] - g);
                df = df < 0.0f ? 0.0f : df;                       // np.clip(diff, 0, 2): a NaN stays
                df = df > 2.0f ? 2.0f : df;
                const float s = 80.0f - df * 40.0f;
                const int idx = s > 0.0f ? (s >= 255.0f ? 255 : (int)s) : 0;  // astype(np.uint8) in range; NaN -> 0
                const unsigned c = lut[idx];
                const unsigned c0 = c & 255u, c1 = (c >> 8) & 255u, c2 = (c >> 16) & 255u;
                m0 = c0 > m0 ? c0 : m0; m1 = c1 > m1 ? c1 : m1; m2 = c2 > m2 ? c2 : m2;
            }
        }
        return (m0 | m1 | m2) == 0u ? 0x00dcdcdcu : (m0 | (m1 << 8) | (m2 << 16));
    });
}

inline long vis_align16(long v) { return (v + 15) & ~15L; }

// the workspace: stats | sel_hist, sel_fin (zeroed by every call) | sel_state | the staging planes
struct VisLayout { long stats, hist, fin, state, staging, total; };
inline VisLayout vis_layout(int N, long packed_floats) {
    VisLayout l;
    l.stats = 0;
    l.hist = vis_align16((long)N * 2 * (long)sizeof(float));
    l.fin = l.hist + 4L * N * 256 * (long)sizeof(unsigned);
    l.state = l.fin + (long)N * 4 * (long)sizeof(unsigned);
    l.staging = vis_align16(l.state + 5L * N * (long)sizeof(uint2));
    l.total = l.staging + vis_align16(packed_floats * (long)sizeof(float));
    return l;
}

}  // namespace

extern "C" long fd_vis_render_ws_bytes(int N, long packed_floats) {
    if (N < 1 || N > VIS_MAX_N || packed_floats < 1 || packed_floats >= (1L << 40)) return 0;
    return vis_layout(N, packed_floats).total;
}

extern "C" int fd_vis_render(const float* disp, int M, int h, int w, float pred_scale, const float* ratio, const float* depth_in,
                             const float* packed_gt, long packed_floats, const fd_eigen_desc* desc, int N, long max_pixels, float gt_lo,
                             float gt_hi, const unsigned char* lut_disp, const unsigned char* lut_err, unsigned char* color,
                             unsigned char* err, long err_pixels, float* stats, float* depth_out, void* ws, void* stream) {
    FD_REQUIRE(desc && ws && packed_floats > 0 && packed_floats < (1L << 40), "fd_vis_render: bad args");
    FD_REQUIRE(N >= 1 && N <= VIS_MAX_N, "fd_vis_render: N must be 1 .. %d", VIS_MAX_N);
    FD_REQUIRE(max_pixels > 0 && max_pixels < (1L << 30), "fd_vis_render: max_pixels must be 1 .. 2^30 - 1");
    FD_REQUIRE((disp != nullptr) != (depth_in != nullptr), "fd_vis_render: give disp or depth_in, not both");
    FD_REQUIRE(!disp || (M > 0 && h > 0 && w > 0 && (long)M * h * w < (1L << 40) && (long)h * w < (1L << 30)),
               "fd_vis_render: bad disparity shape");
    FD_REQUIRE(color || err || stats || depth_out, "fd_vis_render: no output asked for");
    FD_REQUIRE(!color || lut_disp, "fd_vis_render: color needs lut_disp");
    FD_REQUIRE(!err || (lut_err && packed_gt && err_pixels > 0), "fd_vis_render: err needs lut_err, the ground truth and err_pixels");
    FD_REQUIRE(((uintptr_t)desc & 7) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)stats & 3) == 0 && ((uintptr_t)depth_out & 3) == 0 &&
               ((uintptr_t)depth_in & 3) == 0 && ((uintptr_t)packed_gt & 3) == 0,
               "fd_vis_render: desc must be 8-byte aligned, ws 16-byte, the float buffers 4-byte");
    hipStream_t st = (hipStream_t)stream;
    VisArgs a;
    a.disp = disp; a.M = M; a.h = h; a.w = w;
    a.pred_scale = pred_scale; a.ratio = disp ? ratio : nullptr;
    a.depth_in = depth_in;
    a.gt = packed_gt; a.packed_floats = packed_floats;
    a.desc = desc; a.N = N;
    a.gt_lo = gt_lo; a.gt_hi = gt_hi;
    a.lut_disp = lut_disp; a.lut_err = lut_err;
    a.color = color; a.err = err; a.err_pixels = err_pixels;
    const VisLayout l = vis_layout(N, packed_floats);
    char* base = (char*)ws;
    a.stats = stats ? stats : (float*)(base + l.stats);
    a.sel_hist = (unsigned*)(base + l.hist); a.sel_fin = (unsigned*)(base + l.fin); a.sel_state = (uint2*)(base + l.state);
    float* staging = (float*)(base + l.staging);
    a.depth = depth_out ? depth_out : (disp ? staging : nullptr);

    if (a.depth) {
        hipLaunchKernelGGL(k_vis_depth, dim3(fd_cdiv(max_pixels, VIS_THREADS * 4L), N), dim3(VIS_THREADS), 0, st, a);
        FD_LAUNCH_CHECK("fd_vis_render (depth)");
    }
    if (color || stats) {
        const hipError_t e = hipMemsetAsync(base + l.hist, 0, (size_t)(l.state - l.hist), st);
        FD_REQUIRE(e == hipSuccess, "fd_vis_render: clearing the histograms failed: %s", hipGetErrorString(e));
        int groups = fd_cdiv(max_pixels, SEL_PER_GROUP);         // the result does not depend on it: integer sums
        groups = groups > SEL_MAX_GROUPS ? SEL_MAX_GROUPS : groups;
        const dim3 grid(groups, N), block(SEL_THREADS);
        hipLaunchKernelGGL(k_vis_select<0>, grid, block, 0, st, a);
        hipLaunchKernelGGL(k_vis_select<1>, grid, block, 0, st, a);
        hipLaunchKernelGGL(k_vis_select<2>, grid, block, 0, st, a);
        hipLaunchKernelGGL(k_vis_select<3>, grid, block, 0, st, a);
        hipLaunchKernelGGL(k_vis_select<4>, grid, block, 0, st, a);
        FD_LAUNCH_CHECK("fd_vis_render (select)");
        hipLaunchKernelGGL(k_vis_stats, dim3(1), dim3(VIS_MAX_N), 0, st, a);
        FD_LAUNCH_CHECK("fd_vis_render (stats)");
    }
    if (color) {
        hipLaunchKernelGGL(k_vis_color, dim3(fd_cdiv(3 * max_pixels, 16L * VIS_THREADS * 2), N), dim3(VIS_THREADS), 0, st, a);
        FD_LAUNCH_CHECK("fd_vis_render (color)");
    }
    if (err) {
        const long quarter = (max_pixels + 3) / 4 + 1;           // an estimate sizes the grid: the kernels stride over the chunks
        hipLaunchKernelGGL(k_vis_error, dim3(fd_cdiv(3 * quarter, 16L * VIS_THREADS) + 1, N), dim3(VIS_THREADS), 0, st, a);
        FD_LAUNCH_CHECK("fd_vis_render (error)");
    }
    return 0;
}
