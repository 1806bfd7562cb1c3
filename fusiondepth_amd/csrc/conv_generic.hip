// FP32 implicit-GEMM convolution on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact f32, k-ordered
// fmaf chain) — forward, data-gradient and weight-gradient for every conv of the hot path:
//   ResNet trunk   networks/resnet_encoder.py:92-103  (7x7 s2, 3x3 s1/s2, 1x1 s1/s2; zero pad)
//   DepthDecoder   networks/depth_decoder.py:63-96     (3x3 reflect pad + bias + ELU / sigmoid)
//   PoseDecoder    networks/pose_decoder.py:29-51      (1x1 / 3x3 + bias + ReLU)
//
// One "gather GEMM" kernel does forward AND data-gradient:  D[m][p] = sum_k A[m][k] * G[k][p]
//   A   dense row-major [M][K] matrix in HBM (weights, or a re-laid-out copy made by the prep kernels)
//   G   never materialised: k = (c, a, b) indexes channel c and tap (a,b); p = (n, y, x) indexes a pixel of
//       the GEMM-N domain; G[k][p] = X[n][c][y*sy+oy+a*da][x*sx+ox+b*db]  (zero or reflect outside)
//   D   written through an affine pixel map (so stride-2 dgrad parity classes scatter into dX directly).
// NCHW keeps pixels contiguous, so both the G loads and the D stores are coalesced along the 64 lanes.
// Tiles: workgroup = WAVES_M x WAVES_N waves, each wave owns WM x WN accumulators of 32x32, K-chunk 16,
// register-staged double-buffered LDS (one barrier per chunk).
#include "fd_common.h"
#include "conv_generic.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BK = 16;

struct GemmArgs : GemmProblem {};       // the kernels' parameter types: conv_generic.h's structs under the names the symbols carry

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == 1) return v > 0.f ? v : 0.f;
    if (act == 2) return v > 0.f ? v : expm1f(v);
    if (act == 3) return 1.0f / (1.0f + expf(-v));
    if (act == 4) return tanhf(v);
    return v;
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

template <int TA, int TB, int WAVES_M, int WAVES_N, int WM, int WN, bool NORM>
__global__ void __launch_bounds__(64 * WAVES_M * WAVES_N) k_gather_gemm(GemmArgs g) {
    constexpr int NT = 64 * WAVES_M * WAVES_N;
    constexpr int BM = WAVES_M * 32 * WM, BN = WAVES_N * 32 * WN;
    constexpr int LDA = BM + 2, LDB = BN;
    constexpr int RP = NT / BN;            // k rows covered per pass of the G loader
    constexpr int NB_LOAD = BK / RP;       // G elements per thread per chunk
    constexpr int MP = NT / BK;            // m rows covered per pass of the A loader
    constexpr int NA_LOAD = BM / MP;
    static_assert(NT % BN == 0 && BK % RP == 0 && BM % MP == 0, "tile/loader mismatch");
    __shared__ float sA[2][BK * LDA];
    __shared__ float sB[2][BK * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;

    // block -> tile (optionally XCD-aware: consecutive pixel tiles stay on one XCD / one L2)
    int bx = blockIdx.x;
    if (g.xcd_swizzle) { const int per = gridDim.x >> 3; bx = (bx & 7) * per + (bx >> 3); }
    const int m0 = blockIdx.y * BM;
    const long p0 = (long)bx * BN;
    const long plane = (long)g.NY * g.NX, Np = (long)g.Nb * plane;
    const long chw = (long)g.Hi * g.Wi;

    // ---- G loader: this thread always fetches pixel column jn, k rows kr + RP*i
    const int jn = tid % BN;
    const int kr = __builtin_amdgcn_readfirstlane(tid / BN);
    const long pg = p0 + jn;
    const bool pvalid = pg < Np;
    int ry0 = 0, cx0 = 0;
    unsigned nbase = 0u;
    {
        const long pp = pvalid ? pg : 0;
        const int n = (int)(pp / plane);
        const int rem = (int)(pp - (long)n * plane);
        const int y = rem / g.NX, x = rem - y * g.NX;
        ry0 = y * g.sy + g.oy; cx0 = x * g.sx + g.ox;
        nbase = (unsigned)n * (unsigned)g.C * (unsigned)chw;
    }
    // ---- A loader: k column ka, m rows ma + MP*i
    const int ka = tid % BK, ma = tid / BK;
    const __amdgpu_buffer_rsrc_t rsA = fd_make_rsrc(g.A), rsX = fd_make_rsrc(g.X);
    const bool refl = g.pad_mode == 1;

    // Raw buffer loads (32-bit byte offsets, out-of-range = 0.0f): padding taps, k >= K, rows >= M and pixels past the end
    // need no selects; only the NORM variant keeps a validity mask because its padding must stay 0 AFTER the affine map.
    float ra[NA_LOAD], rb[NB_LOAD];
    unsigned okmask = 0u;
    int k0 = 0;                                        // first k of the chunk being fetched
    auto load_a = [&](int i) __attribute__((always_inline)) {
        const int m = m0 + ma + MP * i, k = k0 + ka;
        ra[i] = fd_ldg32(rsA, (m < g.M) & (k < g.K) ? 4u * ((unsigned)m * (unsigned)g.K + (unsigned)k) : FD_OOB);
    };
    auto load_b = [&](int i) __attribute__((always_inline)) {
        const int k = k0 + kr + RP * i;                // wave-uniform
        const int c = k / (TA * TB), t = k - c * (TA * TB);
        const int ta = t / TB, tb = t - ta * TB;
        int r = ry0 + ta * g.da, cc = cx0 + tb * g.db;
        const bool inside = ((unsigned)r < (unsigned)g.Hi) & ((unsigned)cc < (unsigned)g.Wi);
        const int rr = reflect_idx(r, g.Hi), cr = reflect_idx(cc, g.Wi);
        r = refl ? rr : r; cc = refl ? cr : cc;
        const bool ok = pvalid & (k < g.K) & (refl | inside);
        rb[i] = fd_ldg32(rsX, ok ? 4u * (nbase + (unsigned)c * (unsigned)chw + (unsigned)(r * g.Wi + cc)) : FD_OOB);
        if (NORM) okmask = (okmask & ~(1u << i)) | (ok ? (1u << i) : 0u);
    };
    auto store_a = [&](int buf, int i) __attribute__((always_inline)) { sA[buf][ka * LDA + ma + MP * i] = ra[i]; };
    auto store_b = [&](int buf, int i) __attribute__((always_inline)) {
        float v = rb[i];
        if (NORM) v = ((okmask >> i) & 1u) ? (v - 0.45f) / 0.225f : 0.f;          // resnet_encoder.py:94, padding stays 0
        sB[buf][(kr + RP * i) * LDB + jn] = v;
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunk = (g.K + BK - 1) / BK;
    constexpr int NK = BK / 2, LS = NK / 2;           // first LS k-steps issue the next chunk's loads, the last LS store them
#pragma unroll
    for (int i = 0; i < NA_LOAD; ++i) load_a(i);
#pragma unroll
    for (int i = 0; i < NB_LOAD; ++i) load_b(i);
#pragma unroll
    for (int i = 0; i < NA_LOAD; ++i) store_a(0, i);
#pragma unroll
    for (int i = 0; i < NB_LOAD; ++i) store_b(0, i);
    __syncthreads();
    const int arow = lane >> 5, acol = lane & 31;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int cur = ch & 1;
        k0 = (ch + 1) * BK;                            // past the end: k >= K, every load out of range
        const float* pa = &sA[cur][arow * LDA + wave_m * 32 * WM + acol];
        const float* pb = &sB[cur][arow * LDB + wave_n * 32 * WN + acol];
        float av[2][WM], bv[2][WN];
#pragma unroll
        for (int i = 0; i < WM; ++i) av[0][i] = pa[i * 32];
#pragma unroll
        for (int j = 0; j < WN; ++j) bv[0][j] = pb[j * 32];
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
            const int cb = kk & 1, nb = cb ^ 1;
            if (kk + 1 < NK) {
#pragma unroll
                for (int i = 0; i < WM; ++i) av[nb][i] = pa[(kk + 1) * 2 * LDA + i * 32];
#pragma unroll
                for (int j = 0; j < WN; ++j) bv[nb][j] = pb[(kk + 1) * 2 * LDB + j * 32];
            }
            if (kk < LS) {
#pragma unroll
                for (int i = 0; i < NA_LOAD; ++i) if ((i * LS) / NA_LOAD == kk) load_a(i);
#pragma unroll
                for (int i = 0; i < NB_LOAD; ++i) if ((i * LS) / NB_LOAD == kk) load_b(i);
            } else if (kk >= NK - LS) {
#pragma unroll
                for (int i = 0; i < NA_LOAD; ++i) if ((i * LS) / NA_LOAD == kk - (NK - LS)) store_a(cur ^ 1, i);
#pragma unroll
                for (int i = 0; i < NB_LOAD; ++i) if ((i * LS) / NB_LOAD == kk - (NK - LS)) store_b(cur ^ 1, i);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][i], bv[cb][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }

    // ---- epilogue: bias + activation, affine pixel map.  C/D layout of 32x32 MFMA:
    //      col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const long p = p0 + wave_n * 32 * WN + j * 32 + acol;
        if (p >= Np) continue;
        const int n = (int)(p / plane);
        const int rem = (int)(p - (long)n * plane);
        const int y = rem / g.NX, x = rem - y * g.NX;
        float* yo = g.Y + (long)n * g.out_ns + (long)(y * g.osy + g.ooy) * g.out_w + (x * g.osx + g.oox);
#pragma unroll
        for (int i = 0; i < WM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wave_m * 32 * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * arow;
                if (m < g.M) {
                    float v = acc[i][j][r];
                    if (g.bias) v += g.bias[m];
                    yo[(long)m * g.out_cs] = apply_act(v, g.act);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient:  dW[m][j] = sum_p dY[m][p] * G[j][p]   (j = (c,a,b) as above, p over the OUTPUT pixels
// of the forward conv), split over the pixel axis; partial slabs are reduced in a fixed order.
struct WgradArgs : WgradProblem {};

// Loader design (same recipe as conv_fast.hip): raw buffer loads with 32-bit byte offsets, out-of-range = 0.0f; every
// per-row quantity (dY row offset, the (channel, tap) decode of a G row) is fixed per thread and precomputed; the pixel
// decode advances incrementally; loads of chunk ch+1 / their LDS stores are interleaved with the MFMAs of chunk ch.
template <int TA, int TB, int WAVES_M, int WAVES_N, int WM, int WN, bool REFL, bool NORM>
__global__ void __launch_bounds__(64 * WAVES_M * WAVES_N) k_wgrad(WgradArgs g) {
    constexpr int NT = 64 * WAVES_M * WAVES_N;
    constexpr int BM = WAVES_M * 32 * WM, BN = WAVES_N * 32 * WN;
    constexpr int BP = 32;                       // pixels (GEMM-K) per chunk
    constexpr int LDA = BM + 1, LDB = BN + 1;
    constexpr int RPW = NT / BP;                 // rows (m or j) covered per pass
    constexpr int NA_LOAD = BM / RPW, NB_LOAD = BN / RPW;
    static_assert(BM % RPW == 0 && BN % RPW == 0, "tile/loader mismatch");
    __shared__ float sA[2][BP * LDA];
    __shared__ float sB[2][BP * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;
    const int m0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
    const int plane = g.NY * g.NX;
    const long Np = (long)g.Nb * plane;
    const unsigned chw = (unsigned)(g.Hi * g.Wi);
    const long pbeg = (long)blockIdx.z * g.pix_per_split;
    long pend = pbeg + g.pix_per_split;
    if (pend > Np) pend = Np;

    const int pl = tid % BP, rw = tid / BP;      // pixel within chunk, first row handled
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(g.dY), rsX = fd_make_rsrc(g.X);
    const int nrow = g.M - m0 < BM ? g.M - m0 : BM;
    // dY rows past M are clamped to the last valid row: their products land in accumulator rows that are never stored
    unsigned rowa[NA_LOAD];
#pragma unroll
    for (int i = 0; i < NA_LOAD; ++i) {
        const int r = rw + RPW * i < nrow ? rw + RPW * i : nrow - 1;
        rowa[i] = 4u * (unsigned)(m0 + r) * (unsigned)g.dy_cs;
    }
    // G rows j = (channel, tap): byte offset of the (channel, tap) relative to the pixel's gather origin, and the tap
    // displacement for the bounds / reflect logic.  Rows >= J are clamped to row J-1 (their output columns are never stored).
    unsigned joff[NB_LOAD];
    int jro[NB_LOAD], jco[NB_LOAD];
#pragma unroll
    for (int i = 0; i < NB_LOAD; ++i) {
        const int j = j0 + rw + RPW * i < g.J ? j0 + rw + RPW * i : g.J - 1;
        const int c = j / (TA * TB), t = j - c * (TA * TB);
        const int ta = t / TB, tb = t - ta * TB;
        jro[i] = ta * g.da; jco[i] = tb * g.db;
        if (REFL) joff[i] = 4u * (unsigned)c * chw;
        else joff[i] = 4u * ((unsigned)c * chw + (unsigned)(jro[i] * g.Wi + jco[i]));
    }

    float ra[NA_LOAD], rb[NB_LOAD];
    unsigned offa = FD_OOB, xbase = FD_OOB, okmask = 0u;
    int ry0 = 0, cx0 = 0;
    int pn, prem;
    { const long p = pbeg + pl; pn = (int)(p / plane); prem = (int)(p - (long)pn * plane); }
    long pcur = pbeg + pl;
    const float inv_nx = 1.0f / (float)g.NX;
    auto prep_chunk = [&]() __attribute__((always_inline)) {      // pixels >= pend: everything out of range (zeros)
        const bool pv = pcur < pend;
        int y = (int)(((float)prem + 0.5f) * inv_nx);             // estimate within +-1 for planes < 2^23; fixed up below
        int x = prem - y * g.NX;
        if (x < 0) { --y; x += g.NX; }
        if (x >= g.NX) { ++y; x -= g.NX; }
        offa = pv ? 4u * ((unsigned)pn * (unsigned)g.dy_ns + (unsigned)prem) : FD_OOB;
        ry0 = y * g.sy + g.oy; cx0 = x * g.sx + g.ox;
        // zero padding: origin of the gather window (may lie outside the image: the sum with joff is used only in bounds)
        if (REFL) xbase = pv ? 4u * (unsigned)pn * (unsigned)g.C * chw : FD_OOB;
        else xbase = 4u * ((unsigned)pn * (unsigned)g.C * chw + (unsigned)(ry0 * g.Wi + cx0));
        if (!REFL && !pv) ry0 = -(1 << 20);                       // fails every bounds test below
        pcur += BP; prem += BP;
        while (prem >= plane) { prem -= plane; ++pn; }
        okmask = 0u;
    };
    auto load_a = [&](int i) __attribute__((always_inline)) { ra[i] = fd_ldg32(rsY, offa + rowa[i]); };
    auto load_b = [&](int i) __attribute__((always_inline)) {
        const int r = ry0 + jro[i], cc = cx0 + jco[i];
        unsigned off;
        bool ok;
        if (REFL) {
            const int rr = reflect_idx(r, g.Hi), cr = reflect_idx(cc, g.Wi);
            off = xbase + joff[i] + 4u * (unsigned)(rr * g.Wi + cr);          // xbase carries FD_OOB for pixels past the end
            ok = true;
        } else {
            ok = ((unsigned)r < (unsigned)g.Hi) & ((unsigned)cc < (unsigned)g.Wi);
            off = ok ? xbase + joff[i] : FD_OOB;
        }
        if (NORM) okmask |= ok ? (1u << i) : 0u;
        rb[i] = fd_ldg32(rsX, off);
    };
    auto store_a = [&](int buf, int i) __attribute__((always_inline)) { sA[buf][pl * LDA + rw + RPW * i] = ra[i]; };
    auto store_b = [&](int buf, int i) __attribute__((always_inline)) {
        float v = rb[i];
        if (NORM) v = ((okmask >> i) & 1u) ? (v - 0.45f) / 0.225f : 0.f;      // resnet_encoder.py:94, padding stays 0
        sB[buf][pl * LDB + rw + RPW * i] = v;
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunk = pend > pbeg ? (int)((pend - pbeg + BP - 1) / BP) : 0;
    constexpr int NK = BP / 2, HS = NK / 2;
    const int arow = lane >> 5, acol = lane & 31;
    if (nchunk > 0) {
        prep_chunk();
#pragma unroll
        for (int i = 0; i < NA_LOAD; ++i) load_a(i);
#pragma unroll
        for (int i = 0; i < NB_LOAD; ++i) load_b(i);
#pragma unroll
        for (int i = 0; i < NA_LOAD; ++i) store_a(0, i);
#pragma unroll
        for (int i = 0; i < NB_LOAD; ++i) store_b(0, i);
        __syncthreads();
        for (int ch = 0; ch < nchunk; ++ch) {
            const int cur = ch & 1;
            prep_chunk();
            const float* pa = &sA[cur][arow * LDA + wave_m * 32 * WM + acol];
            const float* pb = &sB[cur][arow * LDB + wave_n * 32 * WN + acol];
            float av[2][WM], bv[2][WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) av[0][i] = pa[i * 32];
#pragma unroll
            for (int j = 0; j < WN; ++j) bv[0][j] = pb[j * 32];
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                const int cb = kk & 1, nb = cb ^ 1;
                if (kk + 1 < NK) {
#pragma unroll
                    for (int i = 0; i < WM; ++i) av[nb][i] = pa[(kk + 1) * 2 * LDA + i * 32];
#pragma unroll
                    for (int j = 0; j < WN; ++j) bv[nb][j] = pb[(kk + 1) * 2 * LDB + j * 32];
                }
                if (kk < HS) {
#pragma unroll
                    for (int i = 0; i < NA_LOAD; ++i) if ((i * HS) / NA_LOAD == kk) load_a(i);
#pragma unroll
                    for (int i = 0; i < NB_LOAD; ++i) if ((i * HS) / NB_LOAD == kk) load_b(i);
                } else {
#pragma unroll
                    for (int i = 0; i < NA_LOAD; ++i) if ((i * HS) / NA_LOAD == kk - HS) store_a(cur ^ 1, i);
#pragma unroll
                    for (int i = 0; i < NB_LOAD; ++i) if ((i * HS) / NB_LOAD == kk - HS) store_b(cur ^ 1, i);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][i], bv[cb][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        }
    }
    float* out = g.out + (long)blockIdx.z * g.M * g.J;
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int jj = j0 + wave_n * 32 * WN + j * 32 + acol;
        if (jj >= g.J) continue;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wave_m * 32 * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * arow;
                if (m < g.M) out[(long)m * g.J + jj] = acc[i][j][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------
template <int TA, int TB>
int launch_gemm(const GemmProblem& g, hipStream_t st) {
    const long Np = (long)g.Nb * g.NY * g.NX;
    GemmArgs a{g};
    auto go = [&](auto kern, int BM, int BN, int nt) {
        const int gx = fd_cdiv(Np, BN), gy = fd_cdiv(g.M, BM);
        a.xcd_swizzle = (gx % 8 == 0 && gx >= 16) ? 1 : 0;
        hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(nt), 0, st, a);
    };
    // pick the largest tile that still yields >= ~2 workgroups per CU
    auto blocks = [&](int BM, int BN) { return (long)fd_cdiv(Np, BN) * fd_cdiv(g.M, BM); };
    constexpr bool CAN_NORM = (TA == 7 && TB == 7);
    if (g.in_norm && !CAN_NORM) { fd_set_error("conv: in_norm is only built for the 7x7 stem"); return -1; }
    if (CAN_NORM && g.in_norm) {
        if (blocks(64, 128) >= 512) go(k_gather_gemm<TA, TB, 2, 2, 1, 2, CAN_NORM>, 64, 128, 256);
        else go(k_gather_gemm<TA, TB, 2, 2, 1, 1, CAN_NORM>, 64, 64, 256);
        return 0;
    }
    if (g.M <= 32) {
        go(k_gather_gemm<TA, TB, 1, 4, 1, 1, false>, 32, 128, 256);
    } else if (g.M >= 128 && blocks(128, 128) >= 512) {
        go(k_gather_gemm<TA, TB, 2, 2, 2, 2, false>, 128, 128, 256);
    } else if (blocks(64, 128) >= 512) {
        go(k_gather_gemm<TA, TB, 2, 2, 1, 2, false>, 64, 128, 256);
    } else {
        go(k_gather_gemm<TA, TB, 2, 2, 1, 1, false>, 64, 64, 256);
    }
    return 0;
}

}  // namespace

int dispatch_gemm(int TA, int TB, const GemmProblem& g, hipStream_t st) {
    if (TA == 1 && TB == 1) return launch_gemm<1, 1>(g, st);
    if (TA == 3 && TB == 3) return launch_gemm<3, 3>(g, st);
    if (TA == 7 && TB == 7) return launch_gemm<7, 7>(g, st);
    if (TA == 5 && TB == 5) return launch_gemm<5, 5>(g, st);
    if (TA == 1 && TB == 2) return launch_gemm<1, 2>(g, st);
    if (TA == 2 && TB == 1) return launch_gemm<2, 1>(g, st);
    if (TA == 2 && TB == 2) return launch_gemm<2, 2>(g, st);
    if (TA == 3 && TB == 4) return launch_gemm<3, 4>(g, st);
    if (TA == 4 && TB == 3) return launch_gemm<4, 3>(g, st);
    if (TA == 4 && TB == 4) return launch_gemm<4, 4>(g, st);
    if (TA == 2 && TB == 3) return launch_gemm<2, 3>(g, st);
    if (TA == 3 && TB == 2) return launch_gemm<3, 2>(g, st);
    fd_set_error("conv: unsupported tap shape %dx%d", TA, TB);
    return -1;
}

namespace {
template <int TA, int TB>
int launch_wgrad(const WgradProblem& g, int splits, hipStream_t st) {
    constexpr bool CAN_REFL = (TA == 3 && TB == 3), CAN_NORM = (TA == 7 && TB == 7);
    if (g.pad_mode == 1 && !CAN_REFL) { fd_set_error("conv wgrad: reflect padding is only built for 3x3"); return -1; }
    if (g.in_norm && !CAN_NORM) { fd_set_error("conv wgrad: in_norm is only built for the 7x7 stem"); return -1; }
    auto go = [&](auto kern, int BM, int BN) {
        dim3 grid(fd_cdiv(g.J, BN), fd_cdiv(g.M, BM), splits);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, WgradArgs{g});
    };
    const bool refl = CAN_REFL && g.pad_mode == 1, norm = CAN_NORM && g.in_norm;
    if (g.J <= 64) {
        if (refl) go(k_wgrad<TA, TB, 2, 2, 1, 1, CAN_REFL, false>, 64, 64);
        else if (norm) go(k_wgrad<TA, TB, 2, 2, 1, 1, false, CAN_NORM>, 64, 64);
        else go(k_wgrad<TA, TB, 2, 2, 1, 1, false, false>, 64, 64);
    } else if (g.M <= 32) {
        if (refl) go(k_wgrad<TA, TB, 1, 4, 1, 1, CAN_REFL, false>, 32, 128);
        else if (norm) go(k_wgrad<TA, TB, 1, 4, 1, 1, false, CAN_NORM>, 32, 128);
        else go(k_wgrad<TA, TB, 1, 4, 1, 1, false, false>, 32, 128);
    } else {
        if (refl) go(k_wgrad<TA, TB, 2, 2, 1, 2, CAN_REFL, false>, 64, 128);
        else if (norm) go(k_wgrad<TA, TB, 2, 2, 1, 2, false, CAN_NORM>, 64, 128);
        else go(k_wgrad<TA, TB, 2, 2, 1, 2, false, false>, 64, 128);
    }
    return 0;
}

}  // namespace

int dispatch_wgrad(int TA, int TB, const WgradProblem& g, int splits, hipStream_t st) {
    if (TA == 1 && TB == 1) return launch_wgrad<1, 1>(g, splits, st);
    if (TA == 3 && TB == 3) return launch_wgrad<3, 3>(g, splits, st);
    if (TA == 7 && TB == 7) return launch_wgrad<7, 7>(g, splits, st);
    if (TA == 5 && TB == 5) return launch_wgrad<5, 5>(g, splits, st);
    fd_set_error("conv wgrad: unsupported kernel %dx%d", TA, TB);
    return -1;
}
