// The convolution entry points of the C ABI (fd_conv2d_*) and everything that decides for them: the shape checks, the three
// routes (route_fwd / route_dgrad / route_wgrad: which kernel family computes a convolution, with which weight layout and
// workspace), the *_impl functions that follow a route, and the small passes around the kernels - weight re-layouts, the
// reflect-padding folds, the bias gradient.  The kernels live in one unit per family: conv_generic.hip (the implicit GEMM every
// shape can fall back to), conv_fast.hip, conv_limb.hip, conv_wino*.hip, conv_n16.hip, conv_narrow.hip, conv_c1.hip, conv_stem.hip.
#include "../../include/fdhip.h"
#include "fd_common.h"
#include "conv_fast.h"
#include "conv_generic.h"
#include "conv_wino.h"
#include "conv_limb.h"
#include <stdio.h>
#include <algorithm>
#include "conv_narrow.h"

extern "C" int fd_axpby(const float* a, const float* b, float* out, long n, float alpha, float beta, void* stream);   // pool.hip
extern "C" int fd_act_bwd(const float* y, const float* gy, float* gpre, long n, int act, void* stream);   // pool.hip

namespace {

__global__ void k_reduce_slabs(const float* __restrict__ slabs, float* __restrict__ out, long n, int splits, int accumulate) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float s = accumulate ? out[i] : 0.f;
        for (int z = 0; z < splits; ++z) s += slabs[(long)z * n + i];
        out[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// Weight re-layouts for the data gradient (tiny, once per backward):
//   stride 1:  Wt[ci][(co, a, b)] = W[co][ci][KH-1-a][KW-1-b]
//   stride 2:  Wt[ci][(co, a, b)] = W[co][ci][kh0+2a][kw0+2b]   (taps of one output-parity class)
__global__ void k_weight_relayout(const float* __restrict__ W, float* __restrict__ Wt, int Co, int Ci, int KH, int KW,
                                  int TA, int TB, int kh0, int dkh, int kw0, int dkw) {
    const long n = (long)Ci * Co * TA * TB;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i % TB);
        const int a = (int)((i / TB) % TA);
        const int co = (int)((i / ((long)TB * TA)) % Co);
        const int ci = (int)(i / ((long)TB * TA * Co));
        const int kh = kh0 + dkh * a, kw = kw0 + dkw * b;
        Wt[i] = W[(((long)co * Ci + ci) * KH + kh) * KW + kw];
    }
}

// All weight re-layouts of a training step in one launch: workgroup -> (job, unit) by binary search over the jobs'
// first_block prefix.  For kernels up to 3x3 a unit is a 32 (Cout) x 32 (Cin) tile staged through LDS: the source rows
// W[co][ci0..ci0+31][kh][kw] are contiguous (coalesced reads) and every destination layout has a contiguous run of 32
// along Cin (forward) or Cout (data gradient), so both sides move full 128-byte lines (the per-element gather read with a
// 36-byte stride: 9x the L2 traffic).  Larger kernels (5x5 PoseCNN) keep the per-element path, 1024 elements per unit.
constexpr int RL_TILE = 32;
__host__ __device__ inline bool relayout_tiled(int KH, int KW) { return KH * KW <= 9; }
__host__ __device__ inline long relayout_units(const fd_relayout_job& j) {
    if (relayout_tiled(j.KH, j.KW)) return (long)((j.Co + RL_TILE - 1) / RL_TILE) * ((j.Ci + RL_TILE - 1) / RL_TILE);
    return (j.n + 1023) / 1024;
}

__global__ void __launch_bounds__(256) k_relayout_batch(const fd_relayout_job* __restrict__ jobs, int njobs) {
    __shared__ float tile[RL_TILE][RL_TILE * 9 + 1];
    const long b = blockIdx.x;
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {                                   // last job with first_block <= b
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const fd_relayout_job j = jobs[lo];
    const unsigned u = (unsigned)(b - j.first_block);
    const unsigned TA = (unsigned)j.TA, TB = (unsigned)j.TB, Co = (unsigned)j.Co, Ci = (unsigned)j.Ci;
    if (relayout_tiled(j.KH, j.KW)) {
        const unsigned KK = (unsigned)(j.KH * j.KW), T = TA * TB;
        const unsigned tiles_ci = (Ci + RL_TILE - 1) / RL_TILE;
        const unsigned co0 = (u / tiles_ci) * RL_TILE, ci0 = (u % tiles_ci) * RL_TILE;
        const unsigned nco = Co - co0 < RL_TILE ? Co - co0 : RL_TILE, nci = Ci - ci0 < RL_TILE ? Ci - ci0 : RL_TILE;
        const unsigned row = nci * KK;                   // contiguous source floats per output channel
        for (unsigned i = threadIdx.x; i < nco * row; i += 256) {
            const unsigned r = i / row, q = i - r * row;
            tile[r][q] = j.w[((size_t)(co0 + r) * Ci + ci0) * KK + q];
        }
        __syncthreads();
        if (j.mode == 0) {                               // dst[(co * T + t) * Ci + ci], ci fastest
            for (unsigned i = threadIdx.x; i < nco * T * nci; i += 256) {
                const unsigned c = i % nci, q = i / nci, t = q % T, r = q / T;
                const unsigned a = t / TB, bb = t - a * TB;
                const unsigned tap = (unsigned)(j.kh0 + j.dkh * (int)a) * (unsigned)j.KW + (unsigned)(j.kw0 + j.dkw * (int)bb);
                j.dst[((size_t)(co0 + r) * T + t) * Ci + ci0 + c] = tile[r][c * KK + tap];
            }
        } else if (j.mode == 3) {                        // Winograd U[t][co][ky][ci] (conv_wino_route.hip: k_wino_weight), ci fastest
            const size_t n = (size_t)Co * 3 * Ci;
            for (unsigned i = threadIdx.x; i < nco * 3 * nci; i += 256) {
                const unsigned c = i % nci, q = i / nci, ky = q % 3, r = q / 3;
                const float g0 = tile[r][c * 9 + ky * 3], g1 = tile[r][c * 9 + ky * 3 + 1], g2 = tile[r][c * 9 + ky * 3 + 2];
                float* o = j.dst + ((size_t)(co0 + r) * 3 + ky) * Ci + ci0 + c;
                o[0] = g0; o[n] = 0.5f * (g0 + g1 + g2); o[2 * n] = 0.5f * (g0 - g1 + g2); o[3 * n] = g2;
            }
        } else if (j.mode == 4) {                        // Winograd U of the data gradient: [t][ci][ky][co] of the flipped kernel
            const size_t n = (size_t)Ci * 3 * Co;
            for (unsigned i = threadIdx.x; i < nci * 3 * nco; i += 256) {
                const unsigned r = i % nco, q = i / nco, ky = q % 3, c = q / 3;
                const unsigned row = (2 - ky) * 3;
                const float g0 = tile[r][c * 9 + row + 2], g1 = tile[r][c * 9 + row + 1], g2 = tile[r][c * 9 + row];
                float* o = j.dst + ((size_t)(ci0 + c) * 3 + ky) * Co + co0 + r;
                o[0] = g0; o[n] = 0.5f * (g0 + g1 + g2); o[2 * n] = 0.5f * (g0 - g1 + g2); o[3 * n] = g2;
            }
        } else if (j.mode == 5 || j.mode == 6) {         // F(2x2, 3x3): U2[t][co][ri][ci] (5) / [t][ci][ri][co] of the flipped kernel (6)
            const bool dg = j.mode == 6;
            const size_t n = (size_t)Co * 4 * Ci;
            for (unsigned i = threadIdx.x; i < nco * 4 * nci; i += 256) {
                unsigned r, c, ri;
                if (!dg) { c = i % nci; const unsigned q = i / nci; ri = q % 4; r = q / 4; }
                else { r = i % nco; const unsigned q = i / nco; ri = q % 4; c = q / 4; }
                float v[3];
                for (unsigned b = 0; b < 3; ++b) {
                    const unsigned kb = dg ? 2 - b : b;
                    const float g0 = tile[r][c * 9 + (dg ? 6 : 0) + kb], g1 = tile[r][c * 9 + 3 + kb], g2 = tile[r][c * 9 + (dg ? 0 : 6) + kb];
                    v[b] = ri == 0 ? g0 : (ri == 3 ? g2 : (ri == 1 ? 0.5f * (g0 + g1 + g2) : 0.5f * (g0 - g1 + g2)));
                }
                float* o = dg ? j.dst + ((size_t)(ci0 + c) * 4 + ri) * Co + co0 + r : j.dst + ((size_t)(co0 + r) * 4 + ri) * Ci + ci0 + c;
                o[0] = v[0]; o[n] = 0.5f * (v[0] + v[1] + v[2]); o[2 * n] = 0.5f * (v[0] - v[1] + v[2]); o[3 * n] = v[2];
            }
        } else if (j.mode == 11 || j.mode == 12) {       // F(2x2, 3x3): the limb image of U2 (conv_wino_slab.hip: wino_limb_piece); 12: of the flipped kernel, m = ci
            const bool dg = j.mode == 12;
            const unsigned nm = dg ? nci : nco, nk8 = (dg ? nco : nci) / 8;
            const long Mrows = dg ? Ci : Co;
            const int cpt = (int)((dg ? Co : Ci) >> 4);
            uint4* A3 = reinterpret_cast<uint4*>(j.dst);
            for (unsigned i = threadIdx.x; i < nm * 4 * nk8; i += 256) {
                const unsigned k8 = i % nk8, q = i / nk8, ri = q % 4, mm = q / 4;
                float u[4][8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned r = dg ? k8 * 8 + e : mm, c = dg ? mm : k8 * 8 + e;      // tile row = co, tile column block = ci
                    float v[3];
                    for (unsigned b = 0; b < 3; ++b) {
                        const unsigned kb = dg ? 2 - b : b;
                        const float g0 = tile[r][c * 9 + (dg ? 6 : 0) + kb], g1 = tile[r][c * 9 + 3 + kb], g2 = tile[r][c * 9 + (dg ? 0 : 6) + kb];
                        v[b] = ri == 0 ? g0 : (ri == 3 ? g2 : (ri == 1 ? 0.5f * (g0 + g1 + g2) : 0.5f * (g0 - g1 + g2)));
                    }
                    u[0][e] = v[0]; u[1][e] = 0.5f * (v[0] + v[1] + v[2]); u[2][e] = 0.5f * (v[0] - v[1] + v[2]); u[3][e] = v[2];
                }
                const long kk = (long)(dg ? co0 : ci0) + k8 * 8, m = (long)(dg ? ci0 : co0) + mm;
                const long pbase = (long)ri * cpt + (kk >> 4);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    uint4 h, md, l;
                    fdlimb::split8(u[t], h, md, l);
                    const long p0 = (((pbase * 4 + t) * 3) * 2 + ((kk >> 3) & 1)) * Mrows + m;
                    A3[p0] = h; A3[p0 + 2 * Mrows] = md; A3[p0 + 4 * Mrows] = l;
                }
            }
        } else if (j.mode == 7 || j.mode == 8) {         // 1x1 weights pre-split into bf16 limbs (conv_limb.h): 7 A[m = co][k = ci], 8 A[m = ci][k = co]
            const bool tr = j.mode == 8;
            const unsigned nm = tr ? nci : nco, nk8 = (tr ? nco : nci) / 8;
            const long Mrows = tr ? Ci : Co;
            uint4* A3 = reinterpret_cast<uint4*>(j.dst);
            for (unsigned i = threadIdx.x; i < nm * nk8; i += 256) {
                const unsigned k8 = i % nk8, mm = i / nk8;
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = tr ? tile[k8 * 8 + e][mm] : tile[mm][k8 * 8 + e];
                uint4 h, md, l;
                fdlimb::split8(x, h, md, l);
                const long kk = (tr ? co0 : ci0) + k8 * 8, m = (tr ? ci0 : co0) + mm;
                A3[fdlimb::a3_piece(kk, 0, m, Mrows)] = h;
                A3[fdlimb::a3_piece(kk, 1, m, Mrows)] = md;
                A3[fdlimb::a3_piece(kk, 2, m, Mrows)] = l;
            }
        } else if (j.mode == 9 || j.mode == 10) {        // the taps' matrix [m][(t, c)] pre-split into bf16 limbs: 9 m = co, c = ci (forward), 10 m = ci, c = co (data gradient)
            const bool tr = j.mode == 10;
            const unsigned nm = tr ? nci : nco, nk8 = (tr ? nco : nci) / 8;
            const long Mrows = tr ? Ci : Co, Cr = tr ? Co : Ci;
            uint4* A3 = reinterpret_cast<uint4*>(j.dst);
            for (unsigned i = threadIdx.x; i < nm * T * nk8; i += 256) {
                const unsigned k8 = i % nk8, q = i / nk8, t = q % T, mm = q / T;
                const unsigned a = t / TB, bb = t - a * TB;
                const unsigned tap = (unsigned)(j.kh0 + j.dkh * (int)a) * (unsigned)j.KW + (unsigned)(j.kw0 + j.dkw * (int)bb);
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = tr ? tile[k8 * 8 + e][mm * KK + tap] : tile[mm][(k8 * 8 + e) * KK + tap];
                uint4 h, md, l;
                fdlimb::split8(x, h, md, l);
                const long kk = (long)t * Cr + (tr ? co0 : ci0) + k8 * 8, m = (tr ? ci0 : co0) + mm;
                A3[fdlimb::a3_piece(kk, 0, m, Mrows)] = h;
                A3[fdlimb::a3_piece(kk, 1, m, Mrows)] = md;
                A3[fdlimb::a3_piece(kk, 2, m, Mrows)] = l;
            }
        } else if (j.mode == 1) {                        // dst[(ci * T + t) * Co + co], co fastest
            for (unsigned i = threadIdx.x; i < nci * T * nco; i += 256) {
                const unsigned r = i % nco, q = i / nco, t = q % T, c = q / T;
                const unsigned a = t / TB, bb = t - a * TB;
                const unsigned tap = (unsigned)(j.kh0 + j.dkh * (int)a) * (unsigned)j.KW + (unsigned)(j.kw0 + j.dkw * (int)bb);
                j.dst[((size_t)(ci0 + c) * T + t) * Co + co0 + r] = tile[r][c * KK + tap];
            }
        } else {                                         // dst[((ci * Co + co) * TA + a) * TB + b], taps fastest
            for (unsigned i = threadIdx.x; i < nci * nco * T; i += 256) {
                const unsigned t = i % T, q = i / T, r = q % nco, c = q / nco;
                const unsigned a = t / TB, bb = t - a * TB;
                const unsigned tap = (unsigned)(j.kh0 + j.dkh * (int)a) * (unsigned)j.KW + (unsigned)(j.kw0 + j.dkw * (int)bb);
                j.dst[((size_t)(ci0 + c) * Co + co0 + r) * T + t] = tile[r][c * KK + tap];
            }
        }
        return;
    }
    const unsigned base = u * 1024u;                     // a job has < 2^31 elements: 32-bit index math
    const unsigned n = (unsigned)j.n;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned i = base + e * 256u + threadIdx.x;
        if (i >= n) return;
        unsigned co, ci, a, bb;
        if (j.mode == 2) {                              // [ci][co][a][b]
            unsigned q = i / TB; bb = i - q * TB;
            unsigned q2 = q / TA; a = q - q2 * TA;
            ci = q2 / Co; co = q2 - ci * Co;
        } else {                                        // [m][a][b][c]: mode 0 m = co, c = ci; mode 1 m = ci, c = co
            const unsigned Cr = j.mode ? Co : Ci;
            unsigned q = i / Cr; const unsigned c = i - q * Cr;
            unsigned q2 = q / TB; bb = q - q2 * TB;
            const unsigned m = q2 / TA; a = q2 - m * TA;
            co = j.mode ? c : m; ci = j.mode ? m : c;
        }
        j.dst[i] = j.w[((co * Ci + ci) * (unsigned)j.KH + (unsigned)(j.kh0 + j.dkh * (int)a)) * (unsigned)j.KW +
                       (unsigned)(j.kw0 + j.dkw * (int)bb)];
    }
}

// Reflect-padded data gradient without the padded-grid round trip: the interior of the padded grid IS the zero-padded data gradient
// (written straight to gx by the convolution kernel), only the one-pixel ring needs the adjoint of ReflectionPad2d(1).  The ring
// arrives as four strips per (image, channel) - top [W+2], bottom [W+2], left [H], right [H] (padded rows 1 .. H) - and folds as
//   gx[1][x] += top[x+1], gx[H-2][x] += bottom[x+1], gx[y][1] += left[y], gx[y][W-2] += right[y],
// the corners top[0] / top[W+1] / bottom[0] / bottom[W+1] going to (1,1) / (1,W-2) / (H-2,1) / (H-2,W-2).  One thread per target pixel
// (rows 1 / H-2, columns 1 / W-2) sums every strip value that maps to it in a fixed order: deterministic, also when H - 2 == 1.
__global__ void __launch_bounds__(256) k_reflect_ring_fold(const float* __restrict__ ring, float* __restrict__ gx, long planes, int H,
                                                           int W) {
    const int rows2 = (H - 2 != 1) ? 2 : 1, cols2 = (W - 2 != 1) ? 2 : 1;     // distinct target rows / columns
    const int nrow_t = rows2 * W, ncol_t = (H - rows2) * cols2, nt = nrow_t + ncol_t;
    const long ring_plane = 2L * (W + 2) + 2L * H;
    const long total = planes * nt;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long pl = i / nt;
        const int t = (int)(i - pl * nt);
        int y, x;
        if (t < nrow_t) { const int r = t / W; x = t - r * W; y = r == 0 ? 1 : H - 2; }
        else {
            const int q = t - nrow_t, k = q / (H - rows2), j = q - k * (H - rows2);
            x = k == 0 ? 1 : W - 2;
            const int r_lo = (rows2 == 2 && H - 2 < 1) ? H - 2 : 1, r_hi = (rows2 == 2 && H - 2 < 1) ? 1 : H - 2;   // sorted target rows
            y = j;
            if (y >= r_lo) ++y;
            if (rows2 == 2 && y >= r_hi) ++y;
        }
        const float* top = ring + pl * ring_plane;
        const float* bot = top + (W + 2);
        const float* lef = bot + (W + 2);
        const float* rig = lef + H;
        // padded rows {0 if y == 1, H+1 if y == H-2} x padded columns {x+1, 0 if x == 1, W+1 if x == W-2}; padded row y+1 x
        // padded columns {0 if x == 1, W+1 if x == W-2}
        float s = 0.f;
        if (y == 1) { s += top[x + 1]; if (x == 1) s += top[0]; if (x == W - 2) s += top[W + 1]; }
        if (y == H - 2) { s += bot[x + 1]; if (x == 1) s += bot[0]; if (x == W - 2) s += bot[W + 1]; }
        if (x == 1) s += lef[y];
        if (x == W - 2) s += rig[y];
        gx[pl * (long)H * W + (long)y * W + x] += s;
    }
}

// planes of [H][W] -> planes of [H+2][W+2] with a border of zeros (the padded-grid data gradient on the Winograd kernel, below)
__global__ void __launch_bounds__(256) k_zero_border_copy(const float* __restrict__ src, float* __restrict__ dst, long planes, int H, int W) {
    const int Wp = W + 2, np = (H + 2) * Wp;
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y)
        for (int r = blockIdx.x * 256 + threadIdx.x; r < np; r += gridDim.x * 256) {
            const int y = r / Wp - 1, x = r - (y + 1) * Wp - 1;
            dst[pl * np + r] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? src[pl * (long)H * W + y * W + x] : 0.f;
        }
}

// Adjoint of ReflectionPad2d(1): fold the gradient on the padded grid [H+2][W+2] back onto [H][W].
__global__ void k_reflect_fold(const float* __restrict__ gp, float* __restrict__ gx, long planes, int H, int W) {
    const int Wp = W + 2;
    for (long pl = blockIdx.y; pl < planes; pl += gridDim.y)
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < H * W; r += gridDim.x * blockDim.x) {
        const int y = r / W, x = r - y * W;
        const long i = pl * H * W + r;
        const float* g = gp + pl * (long)(H + 2) * Wp;
        // padded rows that map to y: y+1 always; 0 if y == 1; H+1 if y == H-2
        int ys[3], nys = 0, xs[3], nxs = 0;
        ys[nys++] = y + 1; if (y == 1) ys[nys++] = 0; if (y == H - 2) ys[nys++] = H + 1;
        xs[nxs++] = x + 1; if (x == 1) xs[nxs++] = 0; if (x == W - 2) xs[nxs++] = W + 1;
        float s = 0.f;
        for (int a = 0; a < nys; ++a)
            for (int b = 0; b < nxs; ++b) s += g[ys[a] * Wp + xs[b]];
        gx[i] = s;
    }
}

// per-channel sum over (n, y, x) — bias gradient.  Two deterministic stages: (channel, slice) partials, then a
// fixed-order sum over the slices.
constexpr int CS_SPLITS = 32;
// Round 5: one 64-bit division per ELEMENT and scalar loads made this pass run at 0.6 TB/s (150 us for the 94 MB of upconv(0, 1)'s
// gradient); now slice s of every image's plane, float4 loads four at a time, no index arithmetic in the loop.  The summation order
// changed with it (per thread: images in order, its quads in order; then the fixed block tree) - still deterministic.
template <bool VEC>
__global__ void __launch_bounds__(256) k_channel_sum_part(const float* __restrict__ x, float* __restrict__ part, int Nb,
                                                          int C, long plane) {
    __shared__ float red[4];
    const int c = blockIdx.x, s = blockIdx.y;
    float v[1] = {0.f};
    if (VEC) {
        const long q = plane >> 2, per = (q + CS_SPLITS - 1) / CS_SPLITS;
        const long lo = (long)s * per, hi = lo + per < q ? lo + per : q;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int n = 0; n < Nb; ++n) {
            const float4* p = reinterpret_cast<const float4*>(x + ((long)n * C + c) * plane);
            long i = lo + threadIdx.x;
            for (; i + 768 < hi; i += 1024) {                       // four independent loads in flight
                const float4 u0 = p[i], u1 = p[i + 256], u2 = p[i + 512], u3 = p[i + 768];
                a0 += (u0.x + u0.y) + (u0.z + u0.w); a1 += (u1.x + u1.y) + (u1.z + u1.w);
                a2 += (u2.x + u2.y) + (u2.z + u2.w); a3 += (u3.x + u3.y) + (u3.z + u3.w);
            }
            for (; i < hi; i += 256) { const float4 u = p[i]; a0 += (u.x + u.y) + (u.z + u.w); }
        }
        v[0] = (a0 + a1) + (a2 + a3);
    } else {
        const long per = (plane + CS_SPLITS - 1) / CS_SPLITS;
        const long lo = (long)s * per, hi = lo + per < plane ? lo + per : plane;
        for (int n = 0; n < Nb; ++n) {
            const float* p = x + ((long)n * C + c) * plane;
            for (long i = lo + threadIdx.x; i < hi; i += 256) v[0] += p[i];
        }
    }
    const float sum = fd_block_sum_n<1, 4>(v, red);
    if (threadIdx.x == 0) part[(long)c * CS_SPLITS + s] = sum;
}
__global__ void k_channel_sum_fin(const float* __restrict__ part, float* __restrict__ out, int C, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = accumulate ? out[c] : 0.f;
    for (int i = 0; i < CS_SPLITS; ++i) s += part[(long)c * CS_SPLITS + i];
    out[c] = s;
}

struct ConvShape {
    int Ho, Wo;
};
bool conv_out_shape(const fd_conv_desc* d, ConvShape& s) {
    s.Ho = (d->H + 2 * d->pad - d->KH) / d->stride + 1;
    s.Wo = (d->W + 2 * d->pad - d->KW) / d->stride + 1;
    return s.Ho > 0 && s.Wo > 0;
}
int check_desc(const fd_conv_desc* d, const char* who) {
    FD_REQUIRE(d, "%s: desc is NULL", who);
    FD_REQUIRE(d->N > 0 && d->Cin > 0 && d->Cout > 0 && d->H > 0 && d->W > 0, "%s: bad sizes", who);
    FD_REQUIRE(d->KH == d->KW && (d->KH == 1 || d->KH == 3 || d->KH == 5 || d->KH == 7), "%s: kernel %dx%d unsupported", who,
               d->KH, d->KW);
    FD_REQUIRE(d->stride == 1 || d->stride == 2, "%s: stride %d unsupported", who, d->stride);
    FD_REQUIRE(d->pad >= 0 && d->pad <= d->KH / 2 + 1, "%s: pad %d unsupported", who, d->pad);
    FD_REQUIRE(d->pad_mode == 0 || (d->pad_mode == 1 && d->stride == 1 && d->pad == 1 && d->H >= 2 && d->W >= 2),
               "%s: reflect padding needs stride 1, pad 1", who);
    FD_REQUIRE(d->act >= 0 && d->act <= 4, "%s: bad activation", who);
    return 0;
}
inline int ew_blocks(long n) {
    long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

inline long align4(long n) { return (n + 3) / 4 * 4; }
inline bool fast_fwd_ok(const fd_conv_desc* d) { return d->Cin % 16 == 0 && !d->in_norm; }
inline bool fast_dgrad_ok(const fd_conv_desc* d) { return d->Cout % 16 == 0; }
// the stride-2 layers on the split-precision implicit GEMM (conv_limb.hip: k_conv_limb), forward and data gradient
// (3x3 kernels always; the 1x1 stride-2 downsample layers only where the launch fills the chip without split-K - limb_conv_1x1_worth)
inline bool limb_conv_taps_ok(const fd_conv_desc* d, int M) {
    ConvShape s;
    return d->KH * d->KW > 1 || (d->pad == 0 && conv_out_shape(d, s) && limb_conv_1x1_worth(M, (long)d->N * s.Ho * s.Wo));
}
inline bool limb_conv_fwd_ok(const fd_conv_desc* d) {
    return d->stride == 2 && !d->in_norm && limb_conv_problem_ok(d->Cout, d->Cin, d->pad_mode, d->act) && limb_conv_taps_ok(d, d->Cout);
}
inline bool limb_conv_dgrad_ok(const fd_conv_desc* d) {
    return d->stride == 2 && d->pad_mode == 0 && limb_conv_problem_ok(d->Cin, d->Cout, 0, 0) && limb_conv_taps_ok(d, d->Cin);
}
inline bool limb_conv_wgrad_ok(const fd_conv_desc* d, const ConvShape& s) {
    if (!(d->stride == 2 && d->pad_mode == 0 && !d->in_norm && limb_wgrad_s2_shape_ok(d->Cout, d->Cin, d->H, d->W, s.Ho, s.Wo))) return false;
    if (d->KH == 3 && d->KW == 3 && d->pad == 1) return true;
    return d->KH == 1 && d->KW == 1 && d->pad == 0 && d->Cin >= 256;      // (K = pixels here: the short dimension is Cin x Cout tiles)
}
inline bool fast_wgrad_ok(const fd_conv_desc* d) { return d->Cin % 16 == 0 && d->Cin >= 64 && !d->in_norm; }   // narrow layers: a (tap, channel) tile would be mostly padding

// fd_tuning.log: one stderr line per convolution call (which kernel family it was routed to) - a tuning aid
void conv_log(const char* what, const char* path, const fd_conv_desc* d) {
    if (fd_tun().log) fprintf(stderr, "FDCONV %s %s N=%d Cin=%d H=%d W=%d Cout=%d K=%d s=%d pad_mode=%d\n", what, path, d->N, d->Cin, d->H, d->W, d->Cout, d->KH,
                              d->stride, d->pad_mode);
}
// 1-D Winograd F(2,3) path (conv_wino_x.hip): 3x3 stride-1 pad-1 convs with >= 64 output channels (its tile is 64 channels tall).
// layer1's 64x64 weight gradient (3 tiles x 256 pixel-splits) is 10 % slower than the direct kernel when run alone and still the
// better choice inside the step (449.6 vs 442 images/s): what the step is short of is MFMA cycles, not launch latency
inline bool wino_use_wgrad(const fd_conv_desc* d) { return fd_tun().wino_wgrad != 0 && wino_wgrad_ok(d); }
// fd_tuning.wino_fwd = 0: forward and data gradient stay on the direct kernels (A/B runs)
bool wino_fwd_enabled() { return fd_tun().wino_fwd != 0; }
inline bool wino_use_fwd(const fd_conv_desc* d) { return wino_fwd_enabled() && wino_fwd_ok(d) && d->Cout >= fd_tun().wino_min_cout; }
// the data gradient of a zero-padded 3x3 stride-1 conv is the same kind of conv over dY (channels swapped, kernel flipped)
inline bool wino_dgrad_desc(const fd_conv_desc* d, fd_conv_desc& g) {
    if (!(wino_fwd_enabled() && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->pad_mode == 0)) return false;
    g = *d;
    g.Cin = d->Cout; g.Cout = d->Cin; g.act = 0; g.in_norm = 0;
    return wino_fwd_ok(&g) && g.Cout >= fd_tun().wino_min_cout;
}

// The interior of a REFLECT-padded 3x3 data gradient (the padded grid's cells that are real pixels) is the zero-padded data
// gradient: a plain 3x3 convolution over dY with the transposed, flipped kernel - Winograd-eligible like the trunk's.  With the
// padded grid's one-pixel ring as four thin problems on the implicit-GEMM kernel + k_reflect_ring_fold (round 3), the decoder's
// wide blocks (upconv(2..4, *): 64 .. 512 channels) leave the direct kernel's padded-grid pass (46 - 60 TFLOP/s on these shapes)
// and its full fold pass.  `g`: the convolution the interior computes.  fd_tuning.reflect_wino = 0 switches it off; needs reflect_ring != 0.
bool refl_wino_interior(const fd_conv_desc* d, fd_conv_desc& g) {
    if (!(wino_fwd_enabled() && d->pad_mode == 1 && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->H >= 2 && d->W >= 2)) return false;
    const fd_tuning& t = fd_tun();
    if (!t.reflect_wino || !t.reflect_ring) return false;
    if ((long)d->H * d->W < (long)t.reflect_wino_min_pixels) return false;
    if (!fast_dgrad_ok(d)) return false;                     // the ring runs on the implicit-GEMM kernel
    g = *d;
    g.Cin = d->Cout; g.Cout = d->Cin; g.pad_mode = 0; g.act = 0; g.in_norm = 0;
    return wino_fwd_ok(&g) && g.Cout >= fd_tun().wino_min_cout;
}

// ... and on SMALL planes (below 4 096 pixels: upconv(2..4, *) at 6x20 .. 24x80) the ring's four thin problems -
// few pixels against up to 512 output channels, 32 - 96 workgroups with 72 chunks each and no split-K - cost more than the interior
// (189 us against 60 us for upconv(4,1)).  There the whole padded-grid gradient is ONE Winograd convolution over dY embedded in a
// border of zeros ((H+2) x (W+2): 6 - 47 % more pixels), followed by the fold pass.  `gp`: that convolution.
bool refl_wino_padded(const fd_conv_desc* d, fd_conv_desc& gp) {
    fd_conv_desc gz;
    if (!refl_wino_interior(d, gz)) return false;
    const fd_tuning& t = fd_tun();
    long thr = t.reflect_wino_padded_max;                    // measured in the step: 4 096 (planes up to 24x80) 20.35 - 20.43 ms, 16 384 20.44 - 20.51, 65 536 20.54 - 20.59; 0: never
    if (t.reflect_ring > 1 && t.reflect_ring < thr) thr = t.reflect_ring;    // (the tests' "ring from n pixels on")
    if ((long)d->H * d->W >= thr) return false;              // larger planes: interior + ring
    gp = gz;
    gp.H = d->H + 2; gp.W = d->W + 2;
    return wino_fwd_ok(&gp);
}
constexpr long REFLECT_RING_MIN_PIXELS = 16384;   // reflect_ring = 1 (smaller planes, measured up to 48 x 160: four thin launches + their fold cost more than the fold pass)

void fill_fwd_args(const fd_conv_desc* d, const ConvShape& s, FastGemmArgs& f) {
    f = FastGemmArgs{};
    f.M = d->Cout; f.C = d->Cin; f.T = d->KH * d->KW; f.TB = d->KW; f.K = f.T * f.C;
    f.Nb = d->N; f.Hi = d->H; f.Wi = d->W; f.NY = s.Ho; f.NX = s.Wo;
    f.sy = d->stride; f.oy = -d->pad; f.da = 1; f.sx = d->stride; f.ox = -d->pad; f.db = 1;
    f.pad_mode = d->pad_mode;
    f.out_cs = (long)s.Ho * s.Wo; f.out_ns = f.out_cs * d->Cout; f.out_total = f.out_ns * d->N;
    f.slab_stride = f.out_total;
    f.out_w = s.Wo; f.osy = 1; f.ooy = 0; f.osx = 1; f.oox = 0;
    f.act = d->act;
}

int wgrad_splits(const fd_conv_desc* d, const ConvShape& s) {
    const long Np = (long)d->N * s.Ho * s.Wo;
    const long J = (long)d->Cin * d->KH * d->KW;
    const long tiles = J <= 64 ? (long)fd_cdiv(d->Cout, 64) : (long)fd_cdiv(J, 128) * fd_cdiv(d->Cout, d->Cout <= 32 ? 32 : 64);
    long want = (768 + tiles - 1) / tiles;            // ~3 workgroups per CU
    long maxs = (Np + 511) / 512;                     // at least 512 pixels per split
    long sp = want < maxs ? want : maxs;
    if (sp < 1) sp = 1;
    if (sp > 96) sp = 96;
    return (int)sp;
}

// re-layout mode of a Winograd layout: `g` = the convolution the kernel computes (for a data gradient: channels already swapped)
inline int wino_layout_mode(const fd_conv_desc* g, bool dgrad) {
    if (wino_fwd_limb(g)) return dgrad ? 12 : 11;
    if (wino_fwd_2d(g)) return dgrad ? 6 : 5;
    return dgrad ? 4 : 3;
}

// ------------------------------------------------------------------------------------------------
// Routing: the kernel family of a convolution, its weight layouts and its buffer sizes, decided ONCE per (descriptor, direction) by
// route_fwd / route_dgrad / route_wgrad from the descriptor and fd_tuning alone.  The size queries, fd_conv2d_relayout_jobs and the
// launchers all read the route; only pointer-dependent refinements stay at launch (stem7 without a bias, the 16-byte alignment of
// the limb weight gradients, the alignment checks inside wino_conv_launch).
//   C1 one-output-channel stencil (conv_c1.hip), N16 16 / 32-channel 3x3 blocks (conv_n16.hip), STEM7 / STEM_WGRAD 7x7 stems
//   (conv_stem.hip / conv_narrow.hip), NARROW narrow weight gradients (conv_narrow.hip), LIMB_1X1 / LIMB_S2 1x1 stride-1 GEMM and
//   stride-2 implicit GEMM on bf16 limbs (conv_limb.hip), WINO Winograd on `g` (conv_wino*.hip), DIRECT implicit GEMM (conv_fast.hip),
//   GENERIC gather GEMM (this file); reflect-padded data gradients: WINO_PADDED one Winograd convolution over the zero-bordered dY
//   (`g`) + fold, RING_* the interior on the Winograd (`g`) / 16-channel / implicit-GEMM kernel + the ring, DIRECT / GENERIC the
//   padded grid + fold.
enum class Fam { C1, N16, STEM7, STEM_WGRAD, NARROW, LIMB_1X1, LIMB_S2, WINO, WINO_PADDED, RING_WINO, RING_N16, RING_DIRECT, DIRECT, GENERIC };
struct Job { int mode, TA, TB, kh0, dkh, kw0, dkw, ph, pw; long off; };     // fd_relayout_job at wt + off; ph / pw: stride-2 parity class
struct Route {
    Fam fam = Fam::GENERIC, fallback = Fam::GENERIC;     // fallback: the weight gradient's family where a limb kernel's alignment fails
    const char* name = "generic";                        // what fd_tuning.log prints
    const char* fallback_name = "generic";
    fd_conv_desc g = {};            // the Winograd problem: the forward itself, the swapped / flipped data gradient, or its zero-bordered grid
    long wt = 0, ws = 0;            // weight-layout and workspace floats
    int njobs = 0;
    Job job[4];
    bool need_zero = false;         // stride-2 data gradient: parity classes without taps leave pixels of gx unwritten
    int stat_slots = 0;             // forward: BatchNorm statistics epilogue
    bool bn = false;                // forward: fused BatchNorm (fd_conv2d_fwd_bn_ok adds the plane / group test)
    void set(Fam f, const char* n) { fam = f; name = n; }
    void add_job(int mode, int TA, int TB, int kh0, int dkh, int kw0, int dkw, long off = 0, int ph = 0, int pw = 0) {
        job[njobs++] = Job{mode, TA, TB, kh0, dkh, kw0, dkw, ph, pw, off};
    }
};

// Forward, in the order of DESIGN.md section 5.
Route route_fwd(const fd_conv_desc* d) {
    Route r;
    ConvShape s;
    const bool shape_ok = conv_out_shape(d, s), fast = fast_fwd_ok(d);
    const int KH = d->KH, KW = d->KW;
    if (c1_shape_ok(d)) r.set(Fam::C1, "c1 stencil");
    else if (fast && n16_shape_ok(d, d->Cout, d->Cin)) r.set(Fam::N16, "n16");            // reads the weights as they are
    else if (stem7_fwd_ok(d)) r.set(Fam::STEM7, "stem7");
    else if (!fast) r.set(Fam::GENERIC, "generic");                                     // likewise
    else if (limb_fwd_ok(d)) {
        r.set(Fam::LIMB_1X1, "limb 1x1");
        r.wt = align4(limb_wt_floats(d->Cout, d->Cin));
        r.ws = shape_ok ? limb_gemm_ws_floats(d->Cout, d->Cin, d->N, d->H * d->W) : 0;
        r.add_job(7, 1, 1, 0, 1, 0, 1);
    } else if (wino_use_fwd(d)) {
        r.set(Fam::WINO, "wino");
        r.g = *d;
        r.wt = align4(wino_wt_floats(d));
        r.ws = shape_ok ? wino_ws_floats(d) : 0;
        r.add_job(wino_layout_mode(d, false), KH, KW, 0, 1, 0, 1);
        r.stat_slots = wino_stat_slots(d);
        r.bn = d->act == 0 && wino_fwd_slab_route(d);
    } else {
        const bool limb = limb_conv_fwd_ok(d);
        if (limb) r.set(Fam::LIMB_S2, "limb direct");
        else r.set(Fam::DIRECT, "direct");
        r.wt = align4(limb ? limb_wt_floats(d->Cout, (long)KH * KW * d->Cin) : (long)d->Cout * d->Cin * KH * KW);
        r.add_job(limb ? 9 : 0, KH, KW, 0, 1, 0, 1);
        FastGemmArgs f;
        fill_fwd_args(d, s, f);
        r.ws = !shape_ok ? 0 : limb ? limb_conv_ws_floats(f) : fast_splitk_slab_floats(f, nullptr);
    }
    return r;
}

// Data gradient: a convolution over dY with the transposed, flipped kernel (stride 2: one per output-parity class).
Route route_dgrad(const fd_conv_desc* d) {
    Route r;
    ConvShape s;
    const bool shape_ok = conv_out_shape(d, s), fast = fast_dgrad_ok(d);
    const int KH = d->KH, KW = d->KW;
    const long wt_n = align4((long)d->Cin * d->Cout * KH * KW);
    // reflect padding: the padded grid's gradient (or the ring's strips) at the front of the workspace
    const long padded = d->pad_mode == 1 ? align4((long)d->N * d->Cin * (d->H + 2) * (d->W + 2)) : 0;
    fd_conv_desc gz;
    if (c1_shape_ok(d)) r.set(Fam::C1, "c1 stencil");   // the reflect adjoint folded into the stencil: no layouts, no workspace
    else if (limb_dgrad_ok(d)) {                         // 1x1 stride 1: one GEMM with the transposed weights
        r.set(Fam::LIMB_1X1, "limb 1x1");
        r.wt = align4(limb_wt_floats(d->Cin, d->Cout));
        r.ws = shape_ok ? limb_gemm_ws_floats(d->Cin, d->Cout, d->N, d->H * d->W) : 0;
        r.add_job(8, 1, 1, 0, 1, 0, 1);
    } else if (wino_dgrad_desc(d, r.g)) {
        r.set(Fam::WINO, "wino");
        r.wt = align4(wino_wt_floats(&r.g));
        r.ws = shape_ok ? wino_ws_floats(&r.g) : 0;
        r.add_job(wino_layout_mode(&r.g, true), KH, KW, 0, 1, 0, 1);
    } else if (d->stride == 2) {
        const bool limb = fast && limb_conv_dgrad_ok(d);
        if (limb) r.set(Fam::LIMB_S2, "limb direct");
        else r.set(fast ? Fam::DIRECT : Fam::GENERIC, "direct");        // (the log names the gather GEMM "direct" here too)
        r.wt = 4 * wt_n;                                 // one slot per class: [Cin][(tap, Cout)], its limb image, or [Cin][Cout][tap]
        r.ws = shape_ok ? padded : 0;
        for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw) {
                const int kh0 = (ph + d->pad) & 1, kw0 = (pw + d->pad) & 1;
                if (kh0 >= KH || kw0 >= KW) { r.need_zero = true; continue; }
                if ((d->H - ph + 1) / 2 <= 0 || (d->W - pw + 1) / 2 <= 0) continue;
                r.add_job(limb ? 10 : fast ? 1 : 2, (KH - kh0 + 1) / 2, (KW - kw0 + 1) / 2, kh0, 2, kw0, 2, (long)(ph * 2 + pw) * wt_n, ph, pw);
            }
    } else if (refl_wino_padded(d, r.g)) {               // [padded-grid gradient | slabs | dY in its border of zeros]
        r.set(Fam::WINO_PADDED, "wino on the padded grid + fold");
        r.wt = align4(wino_wt_floats(&r.g));
        r.ws = shape_ok ? padded + wino_ws_floats(&r.g) + align4((long)d->N * d->Cout * (d->H + 2) * (d->W + 2)) : 0;
        r.add_job(wino_layout_mode(&r.g, true), KH, KW, 0, 1, 0, 1);
    } else {
        r.set(fast ? Fam::DIRECT : Fam::GENERIC, "direct");
        r.wt = wt_n;
        r.add_job(fast ? 1 : 2, KH, KW, KH - 1, -1, KW - 1, -1);
        long slabs = 0;
        if (fast && shape_ok) {                          // split-K: the workspace covers every reflect candidate below
            FastGemmArgs f = {};
            f.M = d->Cin; f.C = d->Cout; f.T = KH * KW; f.Nb = d->N;
            f.osy = 1; f.osx = 1;
            auto slab_floats = [&](int NY, int NX) {
                f.NY = NY; f.NX = NX;
                f.out_total = (long)d->N * d->Cin * NY * NX;
                return fast_splitk_slab_floats(f, nullptr);
            };
            slabs = slab_floats(d->pad_mode == 1 ? d->H + 2 : d->H, d->pad_mode == 1 ? d->W + 2 : d->W);
            if (d->pad_mode == 1) slabs = std::max(slabs, slab_floats(d->H, d->W));   // the interior-plus-ring path: the H x W problem
        }
        const int ring_on = fd_tun().reflect_ring;
        const bool wino_interior = refl_wino_interior(d, gz);
        if (d->pad_mode == 1 && fast && ring_on && KH == 3 && KW == 3 && d->pad == 1 && d->H >= 2 && d->W >= 2 &&
            (wino_interior || (long)d->H * d->W >= (ring_on > 1 ? ring_on : REFLECT_RING_MIN_PIXELS))) {
            if (wino_interior) {                         // [layout of the ring's implicit GEMM | U of the interior's Winograd kernel]
                r.set(Fam::RING_WINO, "wino + ring");
                r.g = gz;
                r.wt += align4(wino_wt_floats(&gz));
                r.add_job(wino_layout_mode(&gz, true), KH, KW, 0, 1, 0, 1, wt_n);
                slabs = std::max(slabs, wino_ws_floats(&gz));
            } else if (n16_shape_ok(d, d->Cin, d->Cout)) r.set(Fam::RING_N16, "n16 + ring");
            else r.set(Fam::RING_DIRECT, "direct");
        }
        r.ws = shape_ok ? padded + slabs : 0;
    }
    return r;
}

// Weight gradient.  The limb kernels need 16-byte aligned tensors: the family they fall back to is part of the route, and the
// workspace covers both.
Route route_wgrad(const fd_conv_desc* d) {
    Route r;
    ConvShape s;
    if (!conv_out_shape(d, s)) return r;
    const long wsz = (long)d->Cout * d->Cin * d->KH * d->KW;
    long slabs;
    if (narrow_wgrad_ok(d)) { r.set(Fam::NARROW, "narrow"); slabs = narrow_wgrad_ws_floats(d); }
    else if (stem_wgrad_ok(d)) { r.set(Fam::STEM_WGRAD, "stem"); slabs = stem_wgrad_ws_floats(d); }
    else if (wino_use_wgrad(d)) { r.set(Fam::WINO, "wino"); slabs = wino_wgrad_ws_floats(d); }
    else if (fast_wgrad_ok(d)) {
        r.set(Fam::DIRECT, "direct");
        slabs = (long)fast_wgrad_splits(d->Cout, d->Cin, d->KH * d->KW, (long)d->N * s.Ho * s.Wo) * wsz;
    } else {
        r.set(Fam::GENERIC, "generic");
        const int sp = wgrad_splits(d, s);
        slabs = sp > 1 ? (long)sp * wsz : 0;
    }
    r.fallback = r.fam; r.fallback_name = r.name;
    if (limb_wgrad_ok(d)) {
        r.set(Fam::LIMB_1X1, "limb 1x1");
        slabs = std::max(slabs, limb_wgrad_ws_floats(d->Cout, d->Cin, d->N, d->H * d->W));
    } else if (limb_conv_wgrad_ok(d, s)) {
        r.set(Fam::LIMB_S2, "limb direct");
        slabs = std::max(slabs, limb_wgrad_s2_ws_floats(d->Cout, d->Cin, d->N, s.Ho * s.Wo, d->KH * d->KW));
    }
    if (slabs < wsz) slabs = wsz;                        // accumulate mode stages a single slab
    r.ws = std::max(slabs, (long)d->Cout * CS_SPLITS);   // the bias gradient's partials: the two uses are sequential on the stream
    return r;
}

// The stand-alone weight re-layout launches of the route's jobs [first, first + n) (wt_ready == 0).
int relayout_launch(const Route& r, const fd_conv_desc* d, const float* w, float* wt, hipStream_t st, int first = 0, int n = -1) {
    for (int i = first; i < (n < 0 ? r.njobs : first + n); ++i) {
        const Job& j = r.job[i];
        float* dst = wt + j.off;
        int rc = 0;
        if (j.mode <= 1) rc = fast_weight_relayout(w, dst, d->Cout, d->Cin, d->KH, d->KW, j.TA, j.TB, j.kh0, j.dkh, j.kw0, j.dkw, j.mode, st);
        else if (j.mode == 7 || j.mode == 8)
            rc = limb_weight_split_launch(w, dst, j.mode == 7 ? d->Cout : d->Cin, j.mode == 7 ? d->Cin : d->Cout, j.mode - 7, st);
        else if (j.mode == 9 || j.mode == 10)
            rc = limb_conv_weight_split_launch(w, dst, d->Cout, d->Cin, d->KH, d->KW, j.TA, j.TB, j.kh0, j.dkh, j.kw0, j.dkw, j.mode - 9, st);
        else if (j.mode != 2) rc = wino_weight_launch(&r.g, w, dst, j.mode % 2 == 0, st);   // U of r.g: 3 / 5 / 11, flipped 4 / 6 / 12
        else {
            hipLaunchKernelGGL(k_weight_relayout, dim3(ew_blocks((long)d->Cin * d->Cout * j.TA * j.TB)), dim3(256), 0, st, w, dst,
                               d->Cout, d->Cin, d->KH, d->KW, j.TA, j.TB, j.kh0, j.dkh, j.kw0, j.dkw);
            FD_LAUNCH_CHECK("fd_conv2d_bwd_data(relayout)");
        }
        if (rc) return rc;
    }
    return 0;
}

void reflect_fold_launch(const float* gpad, float* gx, const fd_conv_desc* d, hipStream_t st) {
    const long planes = (long)d->N * d->Cin, bx = ((long)d->H * d->W + 255) / 256;
    hipLaunchKernelGGL(k_reflect_fold, dim3((unsigned)(bx > 64 ? 64 : bx), (unsigned)(planes > 32768 ? 32768 : planes)), dim3(256), 0, st,
                       gpad, gx, planes, d->H, d->W);
}

int conv2d_fwd_impl(const fd_conv_desc* d, const Route& r, const float* x, const float* w, const float* bias, float* y, float* wt,
                    int wt_ready, float* ws, float* stat_part, hipStream_t st) {
    FD_REQUIRE(x && w && y, "fd_conv2d_fwd: NULL tensor");
    ConvShape s;
    FD_REQUIRE(conv_out_shape(d, s), "fd_conv2d_fwd: empty output");
    FD_REQUIRE((long)d->N * d->Cin * d->H * d->W < (1L << 29) && (long)d->N * d->Cout * s.Ho * s.Wo < (1L << 29),
               "fd_conv2d_fwd: tensor too large for 32-bit byte offsets (2 GiB per tensor)");
    FD_REQUIRE(!stat_part || r.stat_slots > 0, "fd_conv2d_fwd_stats: no statistics epilogue for this shape");
    const Fam fam = (r.fam == Fam::STEM7 && bias) ? Fam::GENERIC : r.fam;     // the stem kernels have no bias
    conv_log("fwd", fam == r.fam ? r.name : "generic", d);
    if (r.njobs) {
        FD_REQUIRE(wt, "fd_conv2d_fwd: weight-layout buffer required (fd_conv2d_fwd_wt_floats)");
        if (!wt_ready)
            if (int rc = relayout_launch(r, d, w, wt, st)) return rc;
    }
    switch (fam) {
    case Fam::C1: return c1_fwd_launch(d, x, w, bias, y, st);
    case Fam::N16: return n16_launch(d, d->Cout, d->Cin, x, w, bias, y, 0, d->pad_mode, d->act, st);
    case Fam::STEM7: return stem7_fwd_launch(d, x, w, bias, y, st);
    case Fam::LIMB_1X1: return limb_gemm_launch(wt, x, y, bias, nullptr, ws, d->Cout, d->Cin, d->N, d->H * d->W, d->act, st);
    case Fam::WINO: return wino_conv_launch(d, x, wt, bias, y, ws, st, nullptr, stat_part);
    case Fam::LIMB_S2: case Fam::DIRECT: {
        FastGemmArgs f;
        fill_fwd_args(d, s, f);
        f.A = wt; f.X = x; f.Y = y; f.bias = bias;
        f.slabs = ws;
        return fam == Fam::LIMB_S2 ? limb_conv_launch(f, st) : fast_gemm_launch(f, st);
    }
    default: break;
    }
    GemmProblem g = {};
    g.A = w; g.X = x; g.Y = y; g.bias = bias;
    g.M = d->Cout; g.K = d->Cin * d->KH * d->KW;
    g.Nb = d->N; g.C = d->Cin; g.Hi = d->H; g.Wi = d->W;
    g.NY = s.Ho; g.NX = s.Wo;
    g.sy = d->stride; g.oy = -d->pad; g.da = 1; g.sx = d->stride; g.ox = -d->pad; g.db = 1;
    g.pad_mode = d->pad_mode;
    g.out_ns = (long)d->Cout * s.Ho * s.Wo; g.out_cs = (long)s.Ho * s.Wo;
    g.out_w = s.Wo; g.osy = 1; g.ooy = 0; g.osx = 1; g.oox = 0;
    g.act = d->act; g.in_norm = d->in_norm;
    if (int rc = dispatch_gemm(d->KH, d->KW, g, st)) return rc;
    FD_LAUNCH_CHECK("fd_conv2d_fwd");
    return 0;
}

int bwd_data_impl(const fd_conv_desc* d, const Route& r, const float* gy, const float* w, float* gx, float* wt_base, int wt_ready,
                  float* ws, void* stream, const float* gx_add = nullptr) {
    // gx_add joins in the epilogue of the MFMA kernels (and of their split-K reduction); the remaining paths (generic gather
    // GEMM, reflect padding with its fold pass, parity classes without taps) add it with one element-wise launch afterwards
    const long gx_n = (long)d->N * d->Cin * d->H * d->W;
    auto add_after = [&]() -> int { return gx_add ? fd_axpby(gx, gx_add, gx, gx_n, 1.0f, 1.0f, stream) : 0; };
    hipStream_t st = (hipStream_t)stream;
    conv_log("dgrad", r.name, d);
    if (r.fam == Fam::C1) {                              // dispconv: a stencil with the reflect adjoint folded in (conv_c1.hip)
        FD_REQUIRE(gy && w && gx, "fd_conv2d_bwd_data: NULL tensor");
        if (int rc = c1_dgrad_launch(d, gy, w, gx, st)) return rc;
        return add_after();
    }
    FD_REQUIRE(gy && w && gx && wt_base, "fd_conv2d_bwd_data: NULL tensor");
    ConvShape s;
    FD_REQUIRE(conv_out_shape(d, s), "fd_conv2d_bwd_data: empty output");
    FD_REQUIRE((long)d->N * d->Cin * (d->H + 2) * (d->W + 2) < (1L << 29) && (long)d->N * d->Cout * s.Ho * s.Wo < (1L << 29),
               "fd_conv2d_bwd_data: tensor too large for 32-bit byte offsets (2 GiB per tensor)");
    const int KH = d->KH, KW = d->KW;
    const long pad_n = d->pad_mode == 1 ? align4((long)d->N * d->Cin * (d->H + 2) * (d->W + 2)) : 0;
    FD_REQUIRE(ws || (pad_n == 0), "fd_conv2d_bwd_data: workspace required for reflect padding");
    float* gpad = ws;
    float* slabs = ws ? ws + pad_n : nullptr;
    if (!wt_ready && d->stride == 1)                     // (stride 2: each parity class's re-layout just before its launch, below)
        if (int rc = relayout_launch(r, d, w, wt_base, st)) return rc;

    switch (r.fam) {
    case Fam::LIMB_1X1:                                  // gx[n][ci][p] = sum_co W[co][ci] gy[n][co][p]
        return limb_gemm_launch(wt_base, gy, gx, nullptr, gx_add, ws, d->Cin, d->Cout, d->N, d->H * d->W, 0, st);
    case Fam::WINO:
        return wino_conv_launch(&r.g, gy, wt_base, nullptr, gx, ws, st, gx_add);
    case Fam::WINO_PADDED: {
        const long planes_in = (long)d->N * d->Cout, bx = ((long)(d->H + 2) * (d->W + 2) + 255) / 256;
        float* gyp = slabs + wino_ws_floats(&r.g);
        hipLaunchKernelGGL(k_zero_border_copy, dim3((unsigned)(bx > 64 ? 64 : bx), (unsigned)(planes_in > 32768 ? 32768 : planes_in)), dim3(256), 0, st,
                           gy, gyp, planes_in, d->H, d->W);
        FD_LAUNCH_CHECK("fd_conv2d_bwd_data(zero border)");
        if (int rc = wino_conv_launch(&r.g, gyp, wt_base, nullptr, gpad, slabs, st, nullptr)) return rc;
        reflect_fold_launch(gpad, gx, d, st);
        FD_LAUNCH_CHECK("fd_conv2d_bwd_data(fold)");
        return add_after();
    }
    default: break;
    }
    const bool fast = r.fam != Fam::GENERIC;

    // common geometry of "a conv over gy": channels = Cout, spatial = Ho x Wo
    GemmProblem g = {};
    g.X = gy; g.bias = nullptr; g.act = 0; g.in_norm = 0; g.pad_mode = 0;
    g.M = d->Cin; g.Nb = d->N; g.C = d->Cout; g.Hi = s.Ho; g.Wi = s.Wo;
    auto run = [&](const float* A, int TA, int TB, const float* add) -> int {
        if (fast) {
            FastGemmArgs f = {};
            f.A = A; f.X = gy; f.Y = g.Y; f.bias = nullptr;
            f.M = d->Cin; f.C = d->Cout; f.T = TA * TB; f.TB = TB; f.K = f.T * f.C;
            f.Nb = d->N; f.Hi = s.Ho; f.Wi = s.Wo; f.NY = g.NY; f.NX = g.NX;
            f.sy = g.sy; f.oy = g.oy; f.da = g.da; f.sx = g.sx; f.ox = g.ox; f.db = g.db;
            f.pad_mode = 0;
            f.out_ns = g.out_ns; f.out_cs = g.out_cs; f.out_w = g.out_w;
            f.osy = g.osy; f.ooy = g.ooy; f.osx = g.osx; f.oox = g.oox;
            f.out_total = (long)d->N * g.out_ns; f.slab_stride = f.out_total;
            f.slabs = slabs;       // split-K is only chosen for unit-stride outputs (fast_splitk_slab_floats)
            f.add = add;
            return fast_gemm_launch(f, st);
        }
        g.A = A; g.K = d->Cout * TA * TB;
        if (int rc = dispatch_gemm(TA, TB, g, st)) return rc;
        FD_LAUNCH_CHECK("fd_conv2d_bwd_data(gemm)");
        return 0;
    };

    if (d->stride == 1) {
        g.sy = 1; g.da = 1; g.sx = 1; g.db = 1;
        g.osy = 1; g.ooy = 0; g.osx = 1; g.oox = 0;
        if (r.fam == Fam::RING_WINO || r.fam == Fam::RING_N16 || r.fam == Fam::RING_DIRECT) {
            // Reflect padding, 3x3: (1) the interior of the padded grid = the zero-padded data gradient, straight into gx (with the
            // second gradient of the tensor, if any, in the epilogue); (2) the ring's four strips as ONE grouped launch of thin
            // problems into a small buffer; (3) k_reflect_ring_fold.  The padded-grid gradient + k_reflect_fold of rounds 1-2 wrote
            // and re-read the whole (H+2) x (W+2) tensor on the decoder's serial chain (0.65 ms per training step).
            g.NY = d->H; g.NX = d->W; g.oy = -1; g.ox = -1;
            g.Y = gx; g.out_w = d->W; g.out_cs = (long)d->H * d->W; g.out_ns = g.out_cs * d->Cin;
            // a second gradient of the tensor (not used by the decoder) is added after the fold, so that the sum keeps the order
            // (interior + ring) + other of the fold path, bit for bit
            if (r.fam == Fam::RING_WINO) {               // the decoder's wide blocks: the interior on the Winograd kernels
                if (int rc = wino_conv_launch(&r.g, gy, wt_base + r.job[1].off, nullptr, gx, slabs, st, nullptr)) return rc;
            } else if (r.fam == Fam::RING_N16) {         // the zero-padded data gradient of a 16 / 32-channel block: conv_n16.hip on dY
                if (int rc = n16_launch(d, d->Cin, d->Cout, gy, w, nullptr, gx, 1, 0, 0, st)) return rc;
            } else if (int rc = run(wt_base, KH, KW, nullptr)) return rc;
            const int Hp = d->H, Wp2 = d->W + 2;
            const long ring_plane = 2L * Wp2 + 2L * Hp;
            float* ring = gpad;                                   // [N][Cin][top W+2 | bottom W+2 | left H | right H]
            FastGemmArgs f = {};
            FastGemmGroup q = {};
            f.A = wt_base; f.X = gy; f.Y = ring; f.bias = nullptr;
            f.M = d->Cin; f.C = d->Cout; f.T = 9; f.TB = 3; f.K = 9 * d->Cout;
            f.Nb = d->N; f.Hi = s.Ho; f.Wi = s.Wo;
            f.sy = 1; f.da = 1; f.sx = 1; f.db = 1; f.pad_mode = 0;       // the flip is in the weight layout (kh0 = 2, dkh = -1)
            f.osy = 1; f.osx = 1; f.ooy = 0; f.oox = 0;
            f.out_total = (long)d->N * d->Cin * ring_plane; f.slab_stride = f.out_total; f.slabs = nullptr; f.add = nullptr;
            q.n = 4; q.own_out = 1;
            const int ny[4] = {1, 1, Hp, Hp}, nx[4] = {Wp2, Wp2, 1, 1};
            const int oy4[4] = {-2, -2 + d->H + 1, -1, -1}, ox4[4] = {-2, -2, -2, -2 + d->W + 1};
            const long yoff[4] = {0, Wp2, 2L * Wp2, 2L * Wp2 + Hp};
            for (int j = 0; j < 4; ++j) {
                q.A[j] = wt_base; q.NY[j] = ny[j]; q.NX[j] = nx[j]; q.oy[j] = oy4[j]; q.ox[j] = ox4[j]; q.ooy[j] = 0; q.oox[j] = 0;
                q.T[j] = 9; q.TB[j] = 3; q.K[j] = 9 * d->Cout;
                q.y_off[j] = yoff[j]; q.out_w[j] = nx[j]; q.out_cs[j] = ring_plane; q.out_ns[j] = ring_plane * d->Cin;
            }
            f.NY = q.NY[0]; f.NX = q.NX[0]; f.oy = q.oy[0]; f.ox = q.ox[0];
            f.out_w = q.out_w[0]; f.out_cs = q.out_cs[0]; f.out_ns = q.out_ns[0];
            if (int rc = fast_gemm_group_launch(f, q, st)) return rc;
            const long planes = (long)d->N * d->Cin;
            const int rows2 = (d->H - 2 != 1) ? 2 : 1, cols2 = (d->W - 2 != 1) ? 2 : 1;
            const long targets = planes * ((long)rows2 * d->W + (long)(d->H - rows2) * cols2);
            hipLaunchKernelGGL(k_reflect_ring_fold, dim3((unsigned)ew_blocks(targets)), dim3(256), 0, st, ring, gx, planes, d->H, d->W);
            FD_LAUNCH_CHECK("fd_conv2d_bwd_data(ring fold)");
            return add_after();
        }
        if (d->pad_mode == 1) {   // gradient on the reflect-padded grid, then fold (adjoint of ReflectionPad2d(1))
            g.NY = d->H + 2; g.NX = d->W + 2; g.oy = -(KH - 1); g.ox = -(KW - 1);
            g.Y = gpad; g.out_w = d->W + 2;
            g.out_cs = (long)(d->H + 2) * (d->W + 2); g.out_ns = g.out_cs * d->Cin;
            if (int rc = run(wt_base, KH, KW, nullptr)) return rc;
            reflect_fold_launch(gpad, gx, d, st);
            FD_LAUNCH_CHECK("fd_conv2d_bwd_data(fold)");
            return add_after();
        }
        g.NY = d->H; g.NX = d->W; g.oy = -(KH - 1 - d->pad); g.ox = -(KW - 1 - d->pad);
        g.Y = gx; g.out_w = d->W; g.out_cs = (long)d->H * d->W; g.out_ns = g.out_cs * d->Cin;
        const float* add = fast ? gx_add : nullptr;
        if (int rc = run(wt_base, KH, KW, add)) return rc;
        return add ? 0 : add_after();
    }
    // stride 2: the route's output-parity classes, each a dense conv over its own tap subset
    g.out_w = d->W; g.out_cs = (long)d->H * d->W; g.out_ns = g.out_cs * d->Cin; g.Y = gx;
    FD_REQUIRE(!r.need_zero || hipMemsetAsync(gx, 0, sizeof(float) * (size_t)gx_n, st) == hipSuccess, "fd_conv2d_bwd_data: memset failed");
    const float* add = fast && !r.need_zero ? gx_add : nullptr;     // every element of gx is written by exactly one parity class
    if (fast) {
        // the (up to) four classes in ONE launch: alone, a class has a quarter of the pixels and no split-K (its output is strided) -
        // 92 workgroups for layer4.0 at batch 24; four launches in a row measured 253 us there (27 TFLOP/s)
        FastGemmArgs f = {};
        FastGemmGroup q = {};
        f.X = gy; f.Y = gx; f.bias = nullptr;
        f.M = d->Cin; f.C = d->Cout;
        f.Nb = d->N; f.Hi = s.Ho; f.Wi = s.Wo;
        f.sy = 1; f.da = -1; f.sx = 1; f.db = -1;
        f.pad_mode = 0;
        f.out_ns = g.out_ns; f.out_cs = g.out_cs; f.out_w = g.out_w;
        f.osy = 2; f.osx = 2;
        f.out_total = (long)d->N * g.out_ns; f.slab_stride = f.out_total; f.slabs = nullptr;
        f.add = add;
        // the classes' weights: [Cin][(tap, Cout)] fp32 for k_conv_fast_grp, or its pre-split image for k_conv_limb_grp (in the same slots:
        // 1.5 x (<= 4 of 9 taps) of a slot; a 1x1 kernel has one class and four slots)
        // (classes with the most taps first: their workgroups are the launch's longest - 4, 2, 2, 1 taps for a 3x3 kernel with pad 1)
        for (int i = r.njobs - 1; i >= 0; --i) {
            const Job& c = r.job[i];
            if (!wt_ready)
                if (int rc = relayout_launch(r, d, w, wt_base, st, i, 1)) return rc;
            const int j = q.n++;
            q.A[j] = wt_base + c.off; q.NY[j] = (d->H - c.ph + 1) / 2; q.NX[j] = (d->W - c.pw + 1) / 2;
            q.oy[j] = (c.ph + d->pad - c.kh0) / 2; q.ox[j] = (c.pw + d->pad - c.kw0) / 2;
            q.ooy[j] = c.ph; q.oox[j] = c.pw;
            q.T[j] = c.TA * c.TB; q.TB[j] = c.TB; q.K[j] = c.TA * c.TB * d->Cout;
        }
        if (q.n > 0) {
            f.A = q.A[0]; f.NY = q.NY[0]; f.NX = q.NX[0]; f.T = q.T[0]; f.TB = q.TB[0]; f.K = q.K[0];
            if (r.fam == Fam::LIMB_S2) { if (int rc = limb_conv_group_launch(f, q, st)) return rc; }
            else if (int rc = fast_gemm_group_launch(f, q, st)) return rc;
        }
        return add ? 0 : add_after();
    }
    for (int i = 0; i < r.njobs; ++i) {
        const Job& c = r.job[i];
        if (!wt_ready)
            if (int rc = relayout_launch(r, d, w, wt_base, st, i, 1)) return rc;
        g.NY = (d->H - c.ph + 1) / 2; g.NX = (d->W - c.pw + 1) / 2;
        g.sy = 1; g.oy = (c.ph + d->pad - c.kh0) / 2; g.da = -1;
        g.sx = 1; g.ox = (c.pw + d->pad - c.kw0) / 2; g.db = -1;
        g.osy = 2; g.ooy = c.ph; g.osx = 2; g.oox = c.pw;
        if (int rc = run(wt_base + c.off, c.TA, c.TB, nullptr)) return rc;
    }
    return add_after();
}
}  // namespace

extern "C" long fd_conv2d_fwd_wt_floats(const fd_conv_desc* d) { return d ? route_fwd(d).wt : 0; }
extern "C" long fd_conv2d_fwd_ws_floats(const fd_conv_desc* d) { return d ? route_fwd(d).ws : 0; }

extern "C" int fd_conv2d_fwd(const fd_conv_desc* d, const float* x, const float* w, const float* bias, float* y, float* wt,
                             int wt_ready, float* ws, void* stream) {
    if (int rc = check_desc(d, "fd_conv2d_fwd")) return rc;
    return conv2d_fwd_impl(d, route_fwd(d), x, w, bias, y, wt, wt_ready, ws, nullptr, (hipStream_t)stream);
}
extern "C" int fd_conv2d_fwd_bn_ok(const fd_conv_desc* d, int groups) {
    if (!d || check_desc(d, "fd_conv2d_fwd_bn_ok")) return 0;
    return route_fwd(d).bn && bn_small_slabs_ok(d->N, d->Cout, d->H, d->W, groups) ? 1 : 0;
}
extern "C" int fd_conv2d_fwd_bn(const fd_conv_desc* d, const float* x, const float* w, float* y, float* wt, int wt_ready, float* ws,
                                const float* bn_weight, const float* bn_bias, const float* residual, float* out, float* running_mean,
                                float* running_var, float* save_mean, float* save_invstd, int groups, float eps, float momentum, int relu,
                                void* stream) {
    FD_REQUIRE(fd_conv2d_fwd_bn_ok(d, groups), "fd_conv2d_fwd_bn: not a slab-route 3x3 convolution followed by a small-plane BatchNorm (fd_conv2d_fwd_bn_ok == 0)");
    FD_REQUIRE(x && w && y && wt && ws && out && save_mean && save_invstd, "fd_conv2d_fwd_bn: NULL argument");
    FD_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "fd_conv2d_fwd_bn: running stats must come in pairs");
    hipStream_t st = (hipStream_t)stream;
    conv_log("fwd", "wino + bn", d);
    if (!wt_ready)
        if (int rc = relayout_launch(route_fwd(d), d, w, wt, st)) return rc;
    BnAfterConv bn = {bn_weight, bn_bias, residual, out, running_mean, running_var, save_mean, save_invstd, groups, eps, momentum, relu};
    return wino_conv_launch(d, x, wt, nullptr, y, ws, st, nullptr, nullptr, &bn);
}
extern "C" long fd_conv2d_fwd_stat_slots(const fd_conv_desc* d) {
    if (!d || check_desc(d, "fd_conv2d_fwd_stat_slots")) return 0;
    return route_fwd(d).stat_slots;
}
extern "C" int fd_conv2d_fwd_stats(const fd_conv_desc* d, const float* x, const float* w, const float* bias, float* y, float* wt,
                                   int wt_ready, float* ws, float* stat_part, void* stream) {
    FD_REQUIRE(stat_part, "fd_conv2d_fwd_stats: stat_part is NULL");
    if (int rc = check_desc(d, "fd_conv2d_fwd_stats")) return rc;
    const Route r = route_fwd(d);
    FD_REQUIRE(r.stat_slots > 0, "fd_conv2d_fwd_stats: this convolution has no statistics epilogue (fd_conv2d_fwd_stat_slots == 0)");
    return conv2d_fwd_impl(d, r, x, w, bias, y, wt, wt_ready, ws, stat_part, (hipStream_t)stream);
}

extern "C" long fd_conv2d_bwd_data_wt_floats(const fd_conv_desc* d) { return d ? route_dgrad(d).wt : 0; }
extern "C" long fd_conv2d_bwd_data_ws_floats(const fd_conv_desc* d) { return d ? route_dgrad(d).ws : 0; }

extern "C" int fd_conv2d_bwd_data(const fd_conv_desc* d, const float* gy, const float* w, float* gx, float* wt_base,
                                  int wt_ready, float* ws, void* stream) {
    if (int rc = check_desc(d, "fd_conv2d_bwd_data")) return rc;
    return bwd_data_impl(d, route_dgrad(d), gy, w, gx, wt_base, wt_ready, ws, stream);
}
extern "C" int fd_conv2d_bwd_data_add(const fd_conv_desc* d, const float* gy, const float* w, const float* gx_add, float* gx,
                                      float* wt_base, int wt_ready, float* ws, void* stream) {
    FD_REQUIRE(gx_add != gx, "fd_conv2d_bwd_data_add: gx_add must not alias gx");
    if (int rc = check_desc(d, "fd_conv2d_bwd_data")) return rc;
    return bwd_data_impl(d, route_dgrad(d), gy, w, gx, wt_base, wt_ready, ws, stream, gx_add);
}
extern "C" int fd_conv2d_bwd_data_inact(const fd_conv_desc* d, const float* gy, const float* w, const float* x_in, int in_act, float* gx,
                                        float* wt_base, int wt_ready, float* ws, void* stream) {
    if (int rc = check_desc(d, "fd_conv2d_bwd_data_inact")) return rc;
    FD_REQUIRE(x_in && in_act >= 1 && in_act <= 4, "fd_conv2d_bwd_data_inact: needs the layer's input and an activation id 1..4");
    const Route r = route_dgrad(d);
    if (r.fam == Fam::C1) {                              // dispconv: the factor act'(x_in) rides in the stencil's store
        FD_REQUIRE(gy && w && gx, "fd_conv2d_bwd_data_inact: NULL tensor");
        conv_log("dgrad", "c1 stencil * act'(input)", d);
        return c1_dgrad_launch(d, gy, w, gx, (hipStream_t)stream, x_in, in_act);
    }
    if (int rc = bwd_data_impl(d, r, gy, w, gx, wt_base, wt_ready, ws, stream, nullptr)) return rc;
    return fd_act_bwd(x_in, gx, gx, (long)d->N * d->Cin * d->H * d->W, in_act, stream);       // every other kernel family: one element-wise pass
}

extern "C" int fd_conv2d_relayout_jobs(const fd_conv_desc* d, int kind, const float* w, float* wt, fd_relayout_job* jobs) {
    if (check_desc(d, "fd_conv2d_relayout_jobs") || !w || !wt || !jobs) return 0;
    const Route r = kind == 0 ? route_fwd(d) : route_dgrad(d);
    for (int i = 0; i < r.njobs; ++i) {
        const Job& c = r.job[i];
        fd_relayout_job& j = jobs[i];
        j = fd_relayout_job{};
        j.w = w; j.dst = wt + c.off; j.Co = d->Cout; j.Ci = d->Cin; j.KH = d->KH; j.KW = d->KW;
        j.TA = c.TA; j.TB = c.TB; j.kh0 = c.kh0; j.dkh = c.dkh; j.kw0 = c.kw0; j.dkw = c.dkw; j.mode = c.mode;
        j.n = (long)d->Cout * d->Cin * c.TA * c.TB;
    }
    return r.njobs;
}

extern "C" long fd_relayout_plan(fd_relayout_job* jobs, int n) {
    long blocks = 0;
    for (int i = 0; i < n; ++i) { jobs[i].first_block = blocks; blocks += relayout_units(jobs[i]); }
    return blocks;
}

extern "C" int fd_relayout_batch(const fd_relayout_job* jobs_dev, int n, long total_blocks, void* stream) {
    FD_REQUIRE(jobs_dev && n > 0 && total_blocks > 0 && total_blocks < (1L << 31), "fd_relayout_batch: bad args");
    hipLaunchKernelGGL(k_relayout_batch, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs_dev, n);
    FD_LAUNCH_CHECK("fd_relayout_batch");
    return 0;
}

extern "C" long fd_conv2d_bwd_weight_ws_floats(const fd_conv_desc* d) { return d ? route_wgrad(d).ws : 0; }

extern "C" int fd_conv2d_bwd_weight(const fd_conv_desc* d, const float* x, const float* gy, float* gw, float* gbias,
                                    float* ws, int accumulate, void* stream) {
    if (int rc = check_desc(d, "fd_conv2d_bwd_weight")) return rc;
    FD_REQUIRE(x && gy && gw && ws, "fd_conv2d_bwd_weight: NULL tensor / workspace");
    ConvShape s;
    FD_REQUIRE(conv_out_shape(d, s), "fd_conv2d_bwd_weight: empty output");
    FD_REQUIRE((long)d->N * d->Cin * d->H * d->W < (1L << 29) && (long)d->N * d->Cout * s.Ho * s.Wo < (1L << 29),
               "fd_conv2d_bwd_weight: tensor too large for 32-bit byte offsets (2 GiB per tensor)");
    hipStream_t st = (hipStream_t)stream;
    const long Np = (long)d->N * s.Ho * s.Wo;
    const Route r = route_wgrad(d);
    const bool aligned = (((uintptr_t)x | (uintptr_t)gy) & 15) == 0;
    const bool limb = r.fam == Fam::LIMB_1X1 || r.fam == Fam::LIMB_S2;
    const Fam fam = limb && !aligned ? r.fallback : r.fam;
    conv_log("wgrad", limb && !aligned ? r.fallback_name : r.name, d);
    int rc = 0;
    switch (fam) {
    case Fam::LIMB_1X1: rc = limb_wgrad_launch(x, gy, gw, ws, d->Cout, d->Cin, d->N, d->H * d->W, accumulate, st); break;
    case Fam::LIMB_S2: rc = limb_wgrad_s2_launch(x, gy, gw, ws, d->Cout, d->Cin, d->N, d->H, d->W, s.Ho, s.Wo, d->KH * d->KW, accumulate, st); break;
    case Fam::NARROW: rc = narrow_wgrad_launch(d, x, gy, gw, ws, accumulate, st); break;
    case Fam::STEM_WGRAD: rc = stem_wgrad_launch(d, x, gy, gw, ws, accumulate, st); break;
    case Fam::WINO: rc = wino_wgrad_launch(d, x, gy, gw, ws, accumulate, st); break;
    case Fam::DIRECT: {
        FastWgradArgs f = {};
        f.dY = gy; f.X = x; f.slabs = ws;
        f.M = d->Cout; f.C = d->Cin; f.T = d->KH * d->KW; f.TB = d->KW;
        f.Nb = d->N; f.Hi = d->H; f.Wi = d->W; f.NY = s.Ho; f.NX = s.Wo;
        f.sy = d->stride; f.oy = -d->pad; f.da = 1; f.sx = d->stride; f.ox = -d->pad; f.db = 1;
        f.pad_mode = d->pad_mode;
        f.dy_cs = (long)s.Ho * s.Wo; f.dy_ns = f.dy_cs * d->Cout;
        rc = fast_wgrad_launch(f, gw, fast_wgrad_splits(f.M, f.C, f.T, Np), accumulate, st);
        break;
    }
    default: {
        const int sp = wgrad_splits(d, s);
        const bool staged = sp > 1 || accumulate;
        WgradProblem g = {};
        g.dY = gy; g.X = x; g.out = staged ? ws : gw;
        g.M = d->Cout; g.J = d->Cin * d->KH * d->KW;
        g.Nb = d->N; g.C = d->Cin; g.Hi = d->H; g.Wi = d->W;
        g.NY = s.Ho; g.NX = s.Wo;
        g.sy = d->stride; g.oy = -d->pad; g.da = 1; g.sx = d->stride; g.ox = -d->pad; g.db = 1;
        g.pad_mode = d->pad_mode; g.in_norm = d->in_norm;
        g.dy_cs = (long)s.Ho * s.Wo; g.dy_ns = g.dy_cs * d->Cout;
        long pps = (Np + sp - 1) / sp;
        pps = (pps + 31) / 32 * 32;
        g.pix_per_split = pps;
        if ((rc = dispatch_wgrad(d->KH, d->KW, g, sp, st))) return rc;
        FD_LAUNCH_CHECK("fd_conv2d_bwd_weight");
        if (staged) {
            const long n = (long)g.M * g.J;
            hipLaunchKernelGGL(k_reduce_slabs, dim3(ew_blocks(n)), dim3(256), 0, st, ws, gw, n, sp, accumulate);
            FD_LAUNCH_CHECK("fd_conv2d_bwd_weight(reduce)");
        }
    }
    }
    if (rc) return rc;
    if (gbias) {
        const long plane = (long)s.Ho * s.Wo;
        const bool vec = (plane & 3) == 0 && ((uintptr_t)gy & 15) == 0;
        hipLaunchKernelGGL((vec ? k_channel_sum_part<true> : k_channel_sum_part<false>), dim3(d->Cout, CS_SPLITS), dim3(256), 0, st, gy, ws, d->N,
                           d->Cout, plane);
        FD_LAUNCH_CHECK("fd_conv2d_bwd_weight(bias)");
        hipLaunchKernelGGL(k_channel_sum_fin, dim3(fd_cdiv(d->Cout, 64)), dim3(64), 0, st, ws, gbias, d->Cout, accumulate);
        FD_LAUNCH_CHECK("fd_conv2d_bwd_weight(bias fin)");
    }
    return 0;
}
