// The image summaries of trainer.py:656-681 ("fd_log_sheets"; include/fdhip.h): for J items of a batch, one uint8 RGB contact sheet
// per item - the input colours per frame and scale, the warped colour predictions of scale 0, the normalised disparities and the
// automask (or the predictive masks) - in TWO launches and one memset whatever J, the number of scales and the number of frames are.
//   0 memset         the minimum / maximum words of the disparity tiles.
//   1 k_log_minmax   the float32 minimum and maximum of every disparity tile (utils.normalize_image), up to 64 workgroups per tile:
//                    a shuffle tree per wave, LDS across the waves, then one integer atomic per workgroup on the order-preserving key
//                    of the value (visualize.hip's key).  Integer atomics only: a maximum does not depend on the order, two calls
//                    give the same bits.  A NaN anywhere in a tile sets the tile's NaN word: torch's max() and min() return NaN then,
//                    and every pixel of the tile becomes NaN, which the quantisation turns into 0.
//   2 k_log_write    every byte of every sheet, the background between the tiles included (so nothing has to be cleared first).
//                    A sheet [Hs, Ws, 3] is one contiguous run of bytes: a thread owns one 16-byte chunk of it - the six pixels that
//                    touch it, packed for its phase (chunk start mod 3) - and writes one uint4; the bytes before the first 16-byte
//                    boundary of the ADDRESS and after the last whole chunk are written one by one by the first workgroup
//                    (visualize.hip's scheme).  Chunking the sheet, not the tile, is what keeps every vector store aligned: a tile row
//                    of 3 * w bytes inside a sheet row of 3 * Ws bytes starts at any phase.
//                    A sheet pixel finds its tile through the item's tile table in LDS: the row block (one per scale) by its y, the
//                    tile inside the block by its x; a pixel in no tile is background, 0.
// The tile kinds (fd_log_tile.kind):
//   0 colour         p0 = [3, h, w] float planes                        -> q(r), q(g), q(b)
//   1 prediction     the warp of trainer.py:425-470 at scale 0 for one source frame, restated here with the conventions of the loss
//                    kernels (photometric.hip's project / gather3, layers.py): depth = 1 / (lo + span * disp), the ray through
//                    inv_K, P = (K @ T)[:3], pix = P X / (P X)_z + eps, grid_sample(bilinear, border, align_corners=False).
//                    p0 = the source colours [3, h, w], p1 = the disparity [h, w], p2 = K, p3 = inv_K, p4 = T (4 x 4 each).
//   2 disparity      p0 = [h, w]; (x - mi) / d with d = float32(float64(ma) - float64(mi)), 1e5 where ma == mi; IEEE division.
//   3 automask       p0 = [h, w] uint8, the loss kernel's argmin index; 255 where index > aux - 1 (aux = the number of identity losses).
//   4 mask           p0 = [h, w] float, quantised like a colour.
// q(x) = trunc(min(max(x * 255, 0), 255)), NaN -> 0.  Every float32 step outside the warp is one rounding: contraction is off for the
// file and switched on inside the warp alone, whose sums the loss kernels form with fused multiply-adds.
#include "../../include/fdhip.h"
#include "fd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LOG_THREADS = 256;
constexpr int LOG_MAX_TILES = 64;                                 // tiles per item
constexpr int LOG_MAX_ROWS = 8;                                   // row blocks (scales) per sheet; also disparity tiles per item
constexpr int LOG_MAX_ITEMS = 64;
constexpr int MM_PER_GROUP = 4096;                                // values per workgroup of the minimum / maximum pass
constexpr int MM_MAX_GROUPS = 64;

enum { KIND_COLOR = 0, KIND_PRED = 1, KIND_DISP = 2, KIND_AUTOMASK = 3, KIND_MASK = 4, KIND_COUNT = 5 };

struct LogArgs {
    const fd_log_tile* tiles;                                     // [J][NT], device
    int J, NT;
    fd_log_cfg cfg;
    unsigned char* sheets;
    unsigned* stats;                                              // [J * n_disp][4]: key of the maximum, ~key of the minimum, NaN seen, unused
};

__device__ __forceinline__ unsigned log_key(float v) {            // order-preserving, as visualize.hip's vis_key
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float log_value(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __builtin_bit_cast(float, u);
}

// ---------------------------------------------------------------------------------------------- 1: minimum and maximum
// gridDim.x workgroups per disparity tile, blockIdx.y = item * n_disp + the tile's rank among the item's disparity tiles.
__global__ void __launch_bounds__(LOG_THREADS) k_log_minmax(LogArgs a) {
    __shared__ unsigned red[3][LOG_THREADS / 64];
    const int nd = a.cfg.n_disp, j = blockIdx.y / nd, k = blockIdx.y - j * nd, t = threadIdx.x;
    const fd_log_tile tile = a.tiles[(long)j * a.NT + a.cfg.disp_tile[k]];
    const int n = tile.h * tile.w;
    if ((long)blockIdx.x * LOG_THREADS >= n) return;              // uniform: a tile smaller than the one that sized the grid
    const float* v = (const float*)tile.p0;
    unsigned hi = 0u, lo = 0u, nan = 0u;                          // the minimum as the maximum of ~key: zero is the neutral start of both
    for (int i = blockIdx.x * LOG_THREADS + t; i < n; i += gridDim.x * LOG_THREADS) {
        const float x = v[i];
        if (x != x) { nan = 1u; continue; }
        const unsigned key = log_key(x);
        hi = key > hi ? key : hi;
        lo = ~key > lo ? ~key : lo;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned h2 = __shfl_xor(hi, off, FD_WAVE), l2 = __shfl_xor(lo, off, FD_WAVE), n2 = __shfl_xor(nan, off, FD_WAVE);
        hi = h2 > hi ? h2 : hi; lo = l2 > lo ? l2 : lo; nan |= n2;
    }
    if ((t & 63) == 0) { red[0][t >> 6] = hi; red[1][t >> 6] = lo; red[2][t >> 6] = nan; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < LOG_THREADS / 64; ++w) {
            hi = red[0][w] > hi ? red[0][w] : hi; lo = red[1][w] > lo ? red[1][w] : lo; nan |= red[2][w];
        }
        unsigned* st = a.stats + 4L * blockIdx.y;
        if (hi) atomicMax(&st[0], hi);                            // a key is never 0: 0 means "no finite value seen"
        if (lo) atomicMax(&st[1], lo);
        if (nan) atomicOr(&st[2], 1u);
    }
}

// ---------------------------------------------------------------------------------------------- 2: the sheets
__device__ __forceinline__ unsigned log_q8(float x) {             // trunc(min(max(x * 255, 0), 255)); NaN -> 0
    const float s = x * 255.0f;
    return s > 0.0f ? (s >= 255.0f ? 255u : (unsigned)(int)s) : 0u;
}

// photometric.hip's division: v_rcp_f32 and one Newton-Markstein correction - the correctly rounded quotient except in rare last-bit cases.
__device__ __forceinline__ float log_fdiv(float a, float b) {
    const float rc = __builtin_amdgcn_rcpf(b);
    const float q0 = a * rc;
    return fmaf(fmaf(-q0, b, a), rc, q0);
}

// The warped colour of pixel (y, x): photometric.hip's project and gather3 at the scale where the disparity has the image's size.
__device__ __forceinline__ unsigned log_warp(const fd_log_tile& t, const float* __restrict__ P, float lo, float span, float eps, int y,
                                             int x) {
#pragma clang fp contract(fast)
    const int H = t.h, W = t.w;
    const float* ik = (const float*)t.p3;
    const float fx = (float)x, fy = (float)y;
    const float dup = ((const float*)t.p1)[(long)y * W + x];
    const float depth = log_fdiv(1.0f, lo + span * dup);                                   // layers.py:18-19
    const float r0 = ik[0] * fx + ik[1] * fy + ik[2];                               // layers.py:158
    const float r1 = ik[4] * fx + ik[5] * fy + ik[6];
    const float r2 = ik[8] * fx + ik[9] * fy + ik[10];
    const float X0 = depth * r0, X1 = depth * r1, X2 = depth * r2;
    const float c0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3];                      // layers.py:219
    const float c1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7];
    const float c2 = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
    const float den = c2 + eps;
    const float u = log_fdiv(c0, den), v = log_fdiv(c1, den);                                         // layers.py:221
    const float gx = (log_fdiv(u, (float)(W - 1)) - 0.5f) * 2.0f;                            // layers.py:224-226
    const float gy = (log_fdiv(v, (float)(H - 1)) - 0.5f) * 2.0f;
    // aten GridSampler.h: unnormalize (align_corners=False), then clip_coordinates (border)
    float ix = ((gx + 1.0f) * (float)W - 1.0f) * 0.5f;
    float iy = ((gy + 1.0f) * (float)H - 1.0f) * 0.5f;
    ix = fminf((float)(W - 1), fmaxf(ix, 0.0f));                                    // a NaN becomes 0, as in aten
    iy = fminf((float)(H - 1), fmaxf(iy, 0.0f));
    const float flx = floorf(ix), fly = floorf(iy);
    const int x0 = (int)flx, y0 = (int)fly;                                         // 0 .. W - 1, 0 .. H - 1 after the clip
    const float wx1 = ix - flx, wx0 = 1.0f - wx1, wy1 = iy - fly, wy0 = 1.0f - wy1;
    const bool xin = x0 + 1 <= W - 1, yin = y0 + 1 <= H - 1;      // a tap outside has weight 0; it is not read
    const long plane = (long)H * W;
    const float* src = (const float*)t.p0 + (long)y0 * W + x0;
    unsigned out = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = src + c * plane;
        const float nw = p[0];
        const float ne = xin ? p[1] : 0.0f;
        const float sw = yin ? p[W] : 0.0f;
        const float se = (xin && yin) ? p[W + 1] : 0.0f;
        const float val = nw * (wy0 * wx0) + ne * (wy0 * wx1) + sw * (wy1 * wx0) + se * (wy1 * wx1);
        out |= log_q8(val) << (8 * c);
    }
    return out;
}

// Sixteen bytes of a sheet whose chunk starts at byte 3 * p0 + R: byte i belongs to pixel (R + i) / 3, channel (R + i) % 3;
// c[j] holds pixel p0 + j as r | g << 8 | b << 16.
template <int R>
__device__ __forceinline__ uint4 log_pack16(const unsigned (&c)[6]) {
    unsigned wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = (R + i) / 3, ch = (R + i) - 3 * j;
        wd[i >> 2] |= ((c[j] >> (8 * ch)) & 255u) << (8 * (i & 3));
    }
    return make_uint4(wd[0], wd[1], wd[2], wd[3]);
}

// blockIdx.y = the item; the workgroups of an item stride over the 16-byte chunks of its sheet.
__global__ void __launch_bounds__(LOG_THREADS) k_log_write(LogArgs a) {
    __shared__ fd_log_tile s_tile[LOG_MAX_TILES];
    __shared__ float s_mi[LOG_MAX_TILES], s_d[LOG_MAX_TILES];      // a disparity tile's minimum and divisor (NaN: a NaN in the tile)
    __shared__ float s_P[LOG_MAX_TILES][12];                       // a prediction tile's (K @ T)[:3]
    __shared__ int s_row[4][LOG_MAX_ROWS];                         // y, height, first tile, tile count of every row block
    const int j = blockIdx.y, t = threadIdx.x, NT = a.NT;
    const fd_log_cfg& cfg = a.cfg;
    if (t < LOG_MAX_ROWS) { s_row[0][t] = cfg.row_y[t]; s_row[1][t] = cfg.row_h[t]; s_row[2][t] = cfg.row_first[t]; s_row[3][t] = cfg.row_count[t]; }
    for (int i = t; i < NT; i += LOG_THREADS) {
        const fd_log_tile tile = a.tiles[(long)j * NT + i];
        s_tile[i] = tile;
        if (tile.kind == KIND_DISP) {
            const unsigned* st = a.stats + 4L * (j * cfg.n_disp + tile.slot);
            const float ma = log_value(st[0]), mi = log_value(~st[1]);
            float d = ma == mi ? 1e5f : (float)((double)ma - (double)mi);
            if (st[2]) d = __builtin_nanf("");
            s_mi[i] = mi; s_d[i] = d;
        }
    }
    __syncthreads();
    for (int i = t; i < NT * 12; i += LOG_THREADS) {              // geometry.hip's k_projmat_fwd
        const int ti = i / 12, e = i - 12 * ti, r = e >> 2, c = e & 3;
        if (s_tile[ti].kind != KIND_PRED) continue;
        const float* k = (const float*)s_tile[ti].p2 + r * 4;
        const float* tm = (const float*)s_tile[ti].p4 + c;
        float acc = 0.0f;
        {
#pragma clang fp contract(fast)
            for (int q = 0; q < 4; ++q) acc += k[q] * tm[q * 4];
        }
        s_P[ti][e] = acc;
    }
    __syncthreads();

    const int Ws = cfg.Ws, pixels = cfg.Hs * cfg.Ws;
    const int n_rows = cfg.n_rows;
    auto colour = [&](int gy, int gx) -> unsigned {               // the pixel (gy, gx) of the sheet as r | g << 8 | b << 16
        int r = 0;
        while (r < n_rows && gy >= s_row[0][r] + s_row[1][r]) ++r;
        if (r >= n_rows || gy < s_row[0][r]) return 0u;
        const int ly = gy - s_row[0][r], last = s_row[2][r] + s_row[3][r];
        for (int i = s_row[2][r]; i < last; ++i) {
            const fd_log_tile& tile = s_tile[i];
            const int lx = gx - tile.x;
            if (lx < 0 || lx >= tile.w) continue;
            if (ly >= tile.h) return 0u;                          // below a tile shorter than its row block
            const long o = (long)ly * tile.w + lx;
            switch (tile.kind) {
                case KIND_COLOR: {
                    const float* s = (const float*)tile.p0 + o;
                    const long plane = (long)tile.h * tile.w;
                    return log_q8(s[0]) | (log_q8(s[plane]) << 8) | (log_q8(s[2 * plane]) << 16);
                }
                case KIND_PRED:
                    return log_warp(tile, s_P[i], cfg.lo, cfg.span, cfg.eps, ly, lx);
                case KIND_DISP: {
                    const float x = ((const float*)tile.p0)[o];
                    return 0x010101u * log_q8((x - s_mi[i]) / s_d[i]);
                }
                case KIND_AUTOMASK:
                    return (int)((const unsigned char*)tile.p0)[o] > tile.aux - 1 ? 0xffffffu : 0u;
                case KIND_MASK:
                    return 0x010101u * log_q8(((const float*)tile.p0)[o]);
                default:
                    return 0u;
            }
        }
        return 0u;
    };

    unsigned char* out = a.sheets + 3L * j * pixels;
    const long total = 3L * pixels;
    long head = (long)((16u - (unsigned)((uintptr_t)out & 15u)) & 15u);
    head = head < total ? head : total;
    const long chunks = (total - head) / 16;
    const long tail = head + 16 * chunks;                         // first byte after the last whole chunk
    if (blockIdx.x == 0 && t < 32) {                              // the head and the tail: fewer than 16 bytes each
        const long b = t < 16 ? (long)t : tail + (t - 16);
        const bool in = t < 16 ? b < head : b < total;
        if (in) {
            const int p = (int)(b / 3), ch = (int)(b - 3L * p);
            out[b] = (unsigned char)((colour(p / Ws, p % Ws) >> (8 * ch)) & 255u);
        }
    }
    for (long ck = (long)blockIdx.x * LOG_THREADS + t; ck < chunks; ck += (long)gridDim.x * LOG_THREADS) {
        const long b0 = head + 16 * ck;
        const int p0 = (int)(b0 / 3), r = (int)(b0 - 3L * p0);
        int gy = p0 / Ws, gx = p0 - gy * Ws;
        unsigned c[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {                             // pixels 0 .. (r + 15) / 3 = 5 touch the chunk; all lie in the sheet
            c[q] = p0 + q < pixels ? colour(gy, gx) : 0u;
            if (++gx == Ws) { gx = 0; ++gy; }
        }
        const uint4 v = r == 0 ? log_pack16<0>(c) : (r == 1 ? log_pack16<1>(c) : log_pack16<2>(c));
        *reinterpret_cast<uint4*>(out + b0) = v;
    }
}

}  // namespace

extern "C" long fd_log_sheets_ws_bytes(int J, int n_disp) {
    if (J < 1 || J > LOG_MAX_ITEMS || n_disp < 0 || n_disp > LOG_MAX_ROWS) return 0;
    const long b = 16L * J * n_disp;
    return b > 16 ? b : 16;
}

extern "C" int fd_log_sheets(const fd_log_tile* tiles_host, const fd_log_tile* tiles_dev, int J, int NT, const fd_log_cfg* cfg,
                             unsigned char* sheets, void* ws, void* stream) {
    FD_REQUIRE(tiles_host && tiles_dev && cfg && sheets && ws, "fd_log_sheets: bad args");
    FD_REQUIRE(J >= 1 && J <= LOG_MAX_ITEMS, "fd_log_sheets: J must be 1 .. %d", LOG_MAX_ITEMS);
    FD_REQUIRE(NT >= 1 && NT <= LOG_MAX_TILES, "fd_log_sheets: 1 .. %d tiles per item", LOG_MAX_TILES);
    const fd_log_cfg& c = *cfg;
    FD_REQUIRE(c.Hs > 0 && c.Ws > 0 && (long)c.Hs * c.Ws < (1L << 30), "fd_log_sheets: the sheet must hold 1 .. 2^30 - 1 pixels");
    FD_REQUIRE(c.n_rows >= 1 && c.n_rows <= LOG_MAX_ROWS && c.n_disp >= 0 && c.n_disp <= LOG_MAX_ROWS,
               "fd_log_sheets: 1 .. %d row blocks, at most %d disparity tiles per item", LOG_MAX_ROWS, LOG_MAX_ROWS);
    FD_REQUIRE(((uintptr_t)tiles_dev & 7) == 0 && ((uintptr_t)ws & 15) == 0, "fd_log_sheets: tiles must be 8-byte aligned, ws 16-byte");
    int next = 0, at = 0;
    for (int r = 0; r < c.n_rows; ++r) {                          // the row blocks tile the tile list and follow each other down the sheet
        FD_REQUIRE(c.row_y[r] >= at && c.row_h[r] > 0 && c.row_y[r] <= c.Hs - c.row_h[r], "fd_log_sheets: row block %d leaves the sheet", r);
        FD_REQUIRE(c.row_first[r] == next && c.row_count[r] >= 1 && c.row_count[r] <= NT - next, "fd_log_sheets: row block %d: bad tile range", r);
        at = c.row_y[r] + c.row_h[r];
        next += c.row_count[r];
    }
    FD_REQUIRE(next == NT, "fd_log_sheets: the row blocks hold %d tiles, NT is %d", next, NT);
    int max_disp = 0, seen_disp = 0;
    for (int j = 0; j < J; ++j) {
        for (int r = 0; r < c.n_rows; ++r) {
            int x = 0;
            for (int i = c.row_first[r]; i < c.row_first[r] + c.row_count[r]; ++i) {
                const fd_log_tile& t = tiles_host[(long)j * NT + i];
                FD_REQUIRE(t.kind >= 0 && t.kind < KIND_COUNT, "fd_log_sheets: tile %d of item %d: unknown kind %d", i, j, t.kind);
                FD_REQUIRE(t.h > 0 && t.w > 0 && t.h <= c.row_h[r] && t.y == c.row_y[r] && t.x >= x && t.x <= c.Ws - t.w,
                           "fd_log_sheets: tile %d of item %d leaves its row block or overlaps its neighbour", i, j);
                x = t.x + t.w;
                FD_REQUIRE(t.p0 && ((uintptr_t)t.p0 & (t.kind == KIND_AUTOMASK ? 0 : 3)) == 0, "fd_log_sheets: tile %d of item %d: bad source", i, j);
                if (t.kind == KIND_PRED) {
                    FD_REQUIRE(t.p1 && t.p2 && t.p3 && t.p4 && (((uintptr_t)t.p1 | (uintptr_t)t.p2 | (uintptr_t)t.p3 | (uintptr_t)t.p4) & 3) == 0,
                               "fd_log_sheets: tile %d of item %d: a prediction needs the disparity, K, inv_K and T", i, j);
                    FD_REQUIRE(t.h >= 2 && t.w >= 2, "fd_log_sheets: tile %d of item %d: a prediction needs at least 2 x 2 pixels", i, j);
                }
                if (t.kind == KIND_DISP) {
                    FD_REQUIRE(t.slot >= 0 && t.slot < c.n_disp && c.disp_tile[t.slot] == i, "fd_log_sheets: tile %d of item %d: bad disparity slot", i, j);
                    max_disp = t.h * t.w > max_disp ? t.h * t.w : max_disp;
                    if (j == 0) ++seen_disp;
                }
            }
        }
    }
    FD_REQUIRE(seen_disp == c.n_disp, "fd_log_sheets: %d disparity tiles per item, n_disp is %d", seen_disp, c.n_disp);
    hipStream_t st = (hipStream_t)stream;
    LogArgs a;
    a.tiles = tiles_dev; a.J = J; a.NT = NT; a.cfg = c; a.sheets = sheets; a.stats = (unsigned*)ws;
    if (c.n_disp > 0) {
        const hipError_t e = hipMemsetAsync(ws, 0, (size_t)(16L * J * c.n_disp), st);
        FD_REQUIRE(e == hipSuccess, "fd_log_sheets: clearing the minimum / maximum words failed: %s", hipGetErrorString(e));
        int groups = fd_cdiv(max_disp, MM_PER_GROUP);            // the result does not depend on it: integer maxima
        groups = groups > MM_MAX_GROUPS ? MM_MAX_GROUPS : groups;
        hipLaunchKernelGGL(k_log_minmax, dim3(groups, J * c.n_disp), dim3(LOG_THREADS), 0, st, a);
        FD_LAUNCH_CHECK("fd_log_sheets (minimum / maximum)");
    }
    const long chunks = 3L * c.Hs * c.Ws / 16 + 1;
    hipLaunchKernelGGL(k_log_write, dim3(fd_cdiv(chunks, 2L * LOG_THREADS), J), dim3(LOG_THREADS), 0, st, a);
    FD_LAUNCH_CHECK("fd_log_sheets (write)");
    return 0;
}
