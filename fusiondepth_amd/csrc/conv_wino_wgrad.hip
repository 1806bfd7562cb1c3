// The weight gradient of the 3x3 stride-1 convolutions through the transposed Winograd algorithm, F(2, 3) or F(2x2, 3x3):
// k_wgrad_wino, its split-precision form k_wgrad_wino_limb, the predicates that size their workspace, and their launch.
#include "conv_wino.h"
#include "conv_fast.h"
#include "conv_limb.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------ weight gradient
// dW[m][c][ky][kx] = sum over pixels dY[m][y][x] * X[c][y+ky-1][x+kx-1].  Per pixel pair (dy0, dy1) and the same four inputs
// d0..d3 as the forward, the transposed F(2,3) algorithm needs 4 products instead of 6:
//   P = (dy0, dy0+dy1, dy0-dy1, dy1),  Q = (d0-d2, d1+d2, d2-d1, d1-d3)  (Q is the forward's input transform),
//   M_t = sum_pairs P_t Q_t   (4 GEMMs, M = Cout, N = Cin, K = pixel pairs),
//   dW[kx=0] = M0 + (M1+M2)/2,  dW[1] = (M1-M2)/2,  dW[2] = (M1+M2)/2 - M3.
// One workgroup = (64 output channels) x (64 input channels) x one kernel row ky x a slice of the pairs; wave t owns component t.
// Slices write [split][m][ky*3+kx][c] slabs, reduced in fixed order by k_wgrad_finish (deterministic).
constexpr int WGP = 16;                                          // pairs per chunk (GEMM-K 16 -> 8 MFMA k-steps)

// Both operands stay RAW in LDS and the transforms P = (y0, y0+y1, y0-y1, y1), Q = (d0-d2, d1+d2, d2-d1, d1-d3) are applied when the
// MFMA operands are read.  dY: one row of the chunk's 32 pixels per output channel (stride 34 floats: a lane (= channel) reads
// 8-byte pairs at 34 i mod 64 - 32 different bank pairs).  X: per input channel and PAIR the four pixels (d0, d1, d2, d3) the pair's
// products need, i.e. every pair carries its own left / right neighbour pixel (stride 68 floats: 16-byte reads at 4 i mod 64 banks).
// The loader thread of a pair knows whether it touches an image border and writes the padding value (0, or the mirror pixel) into
// d0 / d3 itself, so the readers need no border flags, no neighbour-cell reads and no halo cells: the round-3a layout (one raw
// 34-float row per channel, flags as scalar lane masks) spent 10 scalar + 2 vector instructions and 2 extra LDS reads per k-step on
// them.  26 KB per chunk and buffer, 52 KB per workgroup: three workgroups per CU.
constexpr int LDG = 2 * WGP + 2;                                 // dY row stride
constexpr int LDX = 4 * WGP + 4;                                 // X row stride: 16 pairs x (d0, d1, d2, d3) + 4
constexpr int WG_BUF_FLOATS = WBM * LDG + WBN * LDX;             // dY rows + X rows
constexpr int WG_LDS_FLOATS = 2 * WG_BUF_FLOATS;

// TWOD: the transposed F(2x2, 3x3) algorithm - the vertical direction is transformed as well.  The GEMM-K unit is a 2x2 tile of dY
// (image rows 2 ty, 2 ty + 1) instead of a pixel pair, and the "kernel row" of a workgroup becomes a row COMPONENT ri = 0 .. 3:
//   dY row combination  (y_r0,  y_r0 + y_r1,  y_r0 - y_r1,  y_r1)[ri]          (rows 2 ty, 2 ty + 1)
//   X  row combination  (x_r0 - x_r2,  x_r1 + x_r2,  x_r2 - x_r1,  x_r1 - x_r3)[ri]   (rows 2 ty - 1 .. 2 ty + 2, padded like the columns)
// formed by the LOADER (two row loads per operand, one fused multiply-add per value) before the pair goes to LDS; everything behind
// that - LDS layout, operand reads, the horizontal transforms, the MFMA loop, the horizontal output transform - is the 1-D kernel's.
// 4 components x half the K of 3 kernel rows: 16 products per 2x2 tile instead of 24 (direct: 36).  Slab rows are [ri][kx]; the
// vertical output transform dW[ky] = (T0 + (T1+T2)/2, (T1-T2)/2, (T1+T2)/2 - T3) is applied by k_wgrad_finish9<12> while it sums the slices.
// HALFM (round 5): at most 32 output channels (the depth decoder's upconv(1, *)) - rows 32 .. 63 of the tile do not exist, so the two waves that
// would own them (wm = 1) take the SECOND HALF OF EVERY CHUNK'S K-STEPS of the first 32 rows instead, and the two partial sums meet in LDS
// once, in front of the epilogue (fixed order: deterministic).  Without it half of the launch's matrix instructions multiply clamped rows.
template <bool REFL, bool TWOD, bool HALFM = false>      // REFL: reflection (decoder) or zero (ResNet trunk) padding - a template flag keeps the border selects out of the trunk's loop
__global__ void __launch_bounds__(WNT) k_wgrad_wino(WinoWgradArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1;
    const int HT = TWOD ? g.H >> 1 : g.H;                        // rows of GEMM-K units per image
    constexpr int R = TWOD ? 4 : 3;                              // workgroup groups along the vertical direction
    const int plane2 = HT * W2, Np = g.Nb * plane2;              // pixel pairs / tiles: < 2^29 (size guard of the entry point)
    const unsigned hw = (unsigned)(g.H * g.W);
    // grid (default): x = (kernel row, input-channel tile), y = output-channel tile, z = pixel slice.  The alternative
    // (slice_major: x = slice with the slice count a multiple of 8, so that all workgroups of a slice share an XCD / L2) measured
    // slightly slower in the training step and is kept as a tuning switch (FD_WINO_WGRAD_MAP=1).
    const int ctiles = (g.C + WBN - 1) / WBN;
    int bt, bs, by;
    if (g.slice_major == 2) {
        // 1-D grid, XCD-aware: consecutive workgroup ids go round-robin to the 8 XCDs, so id L runs on XCD L % 8.  All (kernel row,
        // c tile, m tile) workgroups of one pixel slice get ids 8 apart - same XCD, dispatched back to back - and find the slice's
        // dY / X rows in that XCD's L2 (the 3 kernel rows alone re-read both operands: 3x the HBM traffic when they sit on 3 XCDs).
        const int mtiles = (g.M + WBM - 1) / WBM, nt = R * ctiles * mtiles;
        const int L = blockIdx.x, xcd = L & 7, k = L >> 3;
        int t;
        if (g.xcds_per_slice <= 1) { t = k % nt; bs = (k / nt) * 8 + xcd; }
        // fewer than 8 slices (2 or 4: ResNet layer3 at the step's batch sizes): a slice owns 8 / slices XCDs, each of which takes a
        // contiguous range of the slice's tiles (m-tile major): it reads the slice's X rows once and only its own m tiles' dY rows
        else { const int per = nt / g.xcds_per_slice; bs = xcd / g.xcds_per_slice; t = (xcd % g.xcds_per_slice) * per + k; }
        by = t / (R * ctiles);
        bt = t - by * R * ctiles;
    } else {
        bt = g.slice_major ? blockIdx.z : blockIdx.x; bs = g.slice_major ? blockIdx.x : blockIdx.z; by = blockIdx.y;
    }
    const int ky = bt / ctiles, c0 = (bt - ky * ctiles) * WBN;
    const int m0 = by * WBM;
    const int pp_lo = (int)((long)bs * g.pairs_per_split < Np ? (long)bs * g.pairs_per_split : Np);
    const int pp_hi = (long)pp_lo + g.pairs_per_split < Np ? pp_lo + (int)g.pairs_per_split : Np;
    const int nchunk = pp_hi > pp_lo ? (pp_hi - pp_lo + WGP - 1) / WGP : 0;

    // ---- loader: pair p of the chunk, rows rw + 16 i (dY rows = output channels, X rows = input channels)
    const int p = tid & 15, rw = tid >> 4;
    unsigned a_row[4], b_row[4];                                 // byte offsets of the 4 channel rows (clamped: never stored)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int m = m0 + rw + 16 * i; m = m < g.M ? m : g.M - 1;
        int c = c0 + rw + 16 * i; c = c < g.C ? c : g.C - 1;
        a_row[i] = 4u * (unsigned)m * hw; b_row[i] = 4u * (unsigned)c * hw;
    }
    constexpr bool refl = REFL;
    const int H2m2 = 2 * g.H - 2;
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(g.dY);
    // X with its true size: the 16-byte load of a pair may reach one pixel past the tensor's last one - that lane reads 0.0
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.X), 0, (int)(4u * (unsigned)g.Nb * (unsigned)g.C * hw), 0x00020000);
    f32x2 ra[4], rb[TWOD ? 4 : 1];
    float4 rx[4], rz[TWOD ? 4 : 1];
    unsigned a_off = FD_OOB, x_off = FD_OOB, a_off2 = FD_OOB, x_off2 = FD_OOB;
    // TWOD, row component ri = ky (workgroup-uniform): which rows are combined, and the sign of the second one
    const int yr_a = ky == 3 ? 1 : 0;
    const bool y_two = ky == 1 || ky == 2;
    const float y_sgn = ky == 2 ? -1.f : 1.f;
    const int xr_a = ky == 0 ? 0 : (ky == 2 ? 2 : 1), xr_b = ky == 3 ? 3 : (ky == 2 ? 1 : 2);
    const float x_sgn = ky == 1 ? 1.f : -1.f;
    int pf = 0, rf = 0;          // bit 0 / 1: the pair of the PREPARED chunk (pf) / of the chunk whose data sit in ra, rx (rf) starts / ends an image row
    int pc = pp_lo;                                              // first pair of the chunk being prepared
    // (image, row, pair in row) of this thread's pair of the chunk being prepared: divided out once, then advanced by one chunk per
    // call with two carries - the two integer divisions per chunk of the first version were 15 % of the kernel (profiles/round3_experiments.md)
    int cn, cy, cj;
    {
        const int pq = pp_lo + p;
        cn = pq / plane2;
        const int rem = pq - cn * plane2;
        cy = rem / W2; cj = rem - cy * W2;
    }
    auto prep_chunk = [&](bool live) __attribute__((always_inline)) {
        const int pg = pc + p;
        const bool ok = live & (pg < pp_hi);
        const int n = cn, y = cy, j = cj;
        const bool e_left = j == 0, e_right = 2 * j + 2 >= g.W;
        auto x_row = [&](int r) __attribute__((always_inline)) {              // byte offset of the pair's four pixels in image row r (padded)
            const bool inb = (unsigned)r < (unsigned)g.H;
            int rr_ = r < 0 ? -r : r;
            rr_ = rr_ >= g.H ? H2m2 - rr_ : rr_;
            const int ruse = refl ? rr_ : r;
            const bool okb = ok & (refl | inb);
            const unsigned base = 4u * ((unsigned)n * (unsigned)g.C * hw + (unsigned)(ruse * g.W + 2 * j));
            // four pixels from column 2j - 1 on; a pair at the left border has no such column: it loads from 2j and shifts (store_row)
            return okb ? (e_left ? base : base - 4u) : FD_OOB;
        };
        if constexpr (TWOD) {
            const unsigned ya = 4u * ((unsigned)n * (unsigned)g.M * hw + (unsigned)((2 * y + yr_a) * g.W + 2 * j));
            a_off = ok ? ya : FD_OOB;
            a_off2 = (ok & y_two) ? ya + 4u * (unsigned)g.W : FD_OOB;        // rows 2 ty and 2 ty + 1 (yr_a = 0 whenever both are used)
            x_off = x_row(2 * y - 1 + xr_a);
            x_off2 = x_row(2 * y - 1 + xr_b);
        } else {
            a_off = ok ? 4u * ((unsigned)n * (unsigned)g.M * hw + (unsigned)(y * g.W + 2 * j)) : FD_OOB;
            x_off = x_row(y + ky - 1);
        }
        pf = (e_left ? 1 : 0) | (e_right ? 2 : 0);
        pc += WGP;
        // advance (cn, cy, cj) by one chunk (values past the slice are never used: `ok` is false there)
        cj += g.adv_j;
        const bool c1 = cj >= W2;
        cj -= c1 ? W2 : 0;
        cy += g.adv_y + (c1 ? 1 : 0);
        const bool c2 = cy >= HT;
        cy -= c2 ? HT : 0;
        cn += g.adv_n + (c2 ? 1 : 0);
    };
    auto load_row = [&](int i) __attribute__((always_inline)) {
        if (!HALFM || i < 2) ra[i] = fd_ldg64(rsY, a_off + a_row[i]);     // FD_OOB + (< 2^31) stays out of range: reads 0  (HALFM: dY rows 0 .. 31 only)
        rx[i] = fd_ldg128(rsX, x_off + b_row[i]);
        if constexpr (TWOD) {
            if (!HALFM || i < 2) rb[i] = fd_ldg64(rsY, a_off2 + a_row[i]);
            rz[i] = fd_ldg128(rsX, x_off2 + b_row[i]);
        }
    };
    auto store_row = [&](int buf, int i) __attribute__((always_inline)) {
        float* qa = smem + buf * WG_BUF_FLOATS + (rw + 16 * i) * LDG + 2 * p;
        if constexpr (TWOD) {                                             // the row combinations (exact products: a +- b)
            if (!HALFM || i < 2) { ra[i].x = fmaf(y_sgn, rb[i].x, ra[i].x); ra[i].y = fmaf(y_sgn, rb[i].y, ra[i].y); }
            rx[i].x = fmaf(x_sgn, rz[i].x, rx[i].x); rx[i].y = fmaf(x_sgn, rz[i].y, rx[i].y);
            rx[i].z = fmaf(x_sgn, rz[i].z, rx[i].z); rx[i].w = fmaf(x_sgn, rz[i].w, rx[i].w);
        }
        if (!HALFM || i < 2) *reinterpret_cast<f32x2*>(qa) = ra[i];
        // (d0, d1, d2, d3) of the pair; column -1 is column 1 (reflect) or 0, column W is column W - 2 (reflect) or 0
        const bool L = rf & 1, R = rf & 2;
        float4 d;
        d.y = L ? rx[i].x : rx[i].y;
        d.z = L ? rx[i].y : rx[i].z;
        d.w = L ? rx[i].z : rx[i].w;
        d.x = L ? (refl ? d.z : 0.f) : rx[i].x;
        d.w = R ? (refl ? d.y : 0.f) : d.w;
        *reinterpret_cast<float4*>(smem + buf * WG_BUF_FLOATS + WBM * LDG + (rw + 16 * i) * LDX + 4 * p) = d;
    };

    // Wave w owns the 32 (output channels) x 32 (input channels) block (w >> 1, w & 1) of the tile with all four components (one
    // accumulator each): the output transform dW = (M0 + (M1+M2)/2, (M1-M2)/2, (M1+M2)/2 - M3) is register arithmetic.
    const int wm = wave >> 1, wn = wave & 1;
    const int arow = lane >> 5, acol = lane & 31;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    constexpr int NK = WGP / 2, LS = NK / 2;
    constexpr int NKW = HALFM ? NK / 2 : NK;                     // k-steps per wave and chunk
    static_assert(!HALFM || NKW == LS, "HALFM: the four row loads / stores of a chunk sit in its four k-steps");
    const int kb = HALFM ? wm * NKW : 0;
    if (nchunk > 0) {
        prep_chunk(true);
        rf = pf;
#pragma unroll
        for (int i = 0; i < 4; ++i) load_row(i);
#pragma unroll
        for (int i = 0; i < 4; ++i) store_row(0, i);
        prep_chunk(1 < nchunk);                                   // chunk 1: loaded now, written to LDS during chunk 0
        rf = pf;
#pragma unroll
        for (int i = 0; i < 4; ++i) load_row(i);
        prep_chunk(2 < nchunk);                                   // offsets of chunk 2, re-loaded during chunk 0
        __syncthreads();
        for (int ch = 0; ch < nchunk; ++ch) {
            const int cur = ch & 1;
            // operands of pair k = 2 kk + arow: A = P(dY row 32 wm + acol), B = Q(X row 32 wn + acol)
            // (HALFM: every wave reads dY rows 0 .. 31; wave pair wm takes the k-steps kb .. kb + NKW - 1 of the chunk)
            const float* pa = smem + cur * WG_BUF_FLOATS + ((HALFM ? 0 : 32 * wm) + acol) * LDG + 2 * arow + 4 * kb;
            const float* pb = smem + cur * WG_BUF_FLOATS + WBM * LDG + (32 * wn + acol) * LDX + 4 * arow + 8 * kb;
            float av[2][4], bv[2][4];
            f32x2 yy;
            float4 dd;
            auto read_ops = [&](int kk2) __attribute__((always_inline)) {           // pair 2 kk2 + arow
                yy = *reinterpret_cast<const f32x2*>(pa + 4 * kk2);
                dd = *reinterpret_cast<const float4*>(pb + 8 * kk2);
            };
            auto xform = [&](int nb) __attribute__((always_inline)) {
                av[nb][0] = yy.x; av[nb][1] = yy.x + yy.y; av[nb][2] = yy.x - yy.y; av[nb][3] = yy.y;
                bv[nb][0] = dd.x - dd.z; bv[nb][1] = dd.y + dd.z; bv[nb][2] = dd.z - dd.y; bv[nb][3] = dd.y - dd.w;
            };
            read_ops(0); xform(0);
#pragma unroll
            for (int kk = 0; kk < NKW; ++kk) {
                const int cb = kk & 1, nb = cb ^ 1;
                __builtin_amdgcn_sched_barrier(0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0], bv[cb][0], acc[0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NKW) read_ops(kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1], bv[cb][1], acc[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < LS) store_row(cur ^ 1, kk);              // registers loaded one chunk ago -> the other buffer
                __builtin_amdgcn_sched_barrier(0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][2], bv[cb][2], acc[2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NKW) xform(nb);
                __builtin_amdgcn_sched_barrier(0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][3], bv[cb][3], acc[3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < LS) load_row(kk);                        // ... and re-loaded with the chunk after next
                if (kk == (HALFM ? NKW - 1 : LS)) rf = pf;                                  // the flags travel with the registers (all four rows re-loaded by now)
                if (kk == NKW - 1) prep_chunk(ch + 3 < nchunk);
            }
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
        }
    }

    if constexpr (HALFM) {                                       // the two K halves of the 32 rows meet: wm = 0 keeps acc(wm = 0) + acc(wm = 1)
        float* red = smem + ((wn * 64) << 6) + lane;             // [wn][component * 16 + register][lane]; the chunk loop ended with a barrier
        if (wm == 1) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(t * 16 + r) << 6] = acc[t][r];
        }
        __syncthreads();
        if (wm == 1) return;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] += red[(t * 16 + r) << 6];
    }
    // ---- epilogue: slab[z][m][ky*3 + kx][c] from the four accumulators (C/D layout: column = lane & 31, row = (reg & 3) +
    //      8 * (reg >> 2) + 4 * (lane >> 5))
    const int c = c0 + 32 * wn + acol;
    // this slice's slab through a buffer resource: 32-bit offsets (a slab is M * 9 * C floats < 2^29), rows / columns past the tensor
    // are dropped by an out-of-range offset instead of a branch per row
    const __amdgpu_buffer_rsrc_t rsS = fd_make_rsrc(g.slabs + (size_t)bs * ((size_t)g.M * (3 * R) * g.C));
    const int mb = m0 + (HALFM ? 0 : 32 * wm) + 4 * arow;
    const unsigned col = (c < g.C) ? 4u * (unsigned)(ky * 3 * g.C + c) : FD_OOB;
    const unsigned row_step = 4u * (3u * R) * (unsigned)g.C, kx_step = 4u * (unsigned)g.C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        const unsigned off = (m < g.M) ? col + (unsigned)m * row_step : FD_OOB;        // FD_OOB + (< 2^31) stays out of range
        const float M0 = acc[0][r], M1 = acc[1][r], M2 = acc[2][r], M3 = acc[3][r];
        const float h = 0.5f * (M1 + M2);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, M0 + h), rsS, (int)off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, 0.5f * (M1 - M2)), rsS, (int)(off + kx_step), 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h - M3), rsS, (int)(off + 2u * kx_step), 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient, split precision
// k_wgrad_wino<false, true> (zero padding, transposed F(2x2, 3x3), >= 64 output channels) on the bf16 matrix pipes at fp32 accuracy
// (conv_limb.h: every fp32 operand = three bf16 limbs, six limb products, fp32 accumulation).  Same grid, slices, loader addressing, row
// combinations and epilogue; what changes is WHERE the horizontal transforms run and what LDS holds:
//   * the loader thread of a QUAD of pairs applies the vertical combination (as before), the padding (as before) AND the horizontal transforms
//     P = (y0, y0+y1, y0-y1, y1), Q = (d0-d2, d1+d2, d2-d1, d1-d3) of its four pairs, splits them into limbs and writes 8-byte pieces:
//     LDS holds, per operand, [component 4][limb 3][K half 2][row 64] 16-byte MFMA fragments of 8 pairs - the chunk's 16 pairs are ONE
//     v_mfma_f32_32x32x16_bf16 k-step;
//   * the matrix loop is 24 fragment reads + 24 MFMAs per chunk and wave (768 matrix-pipe cycles instead of the 2 048 of 32
//     v_mfma_f32_32x32x2_f32) with no vector arithmetic at all; every value is transformed and split ONCE per workgroup (the f32 kernel
//     transforms at operand-read time: once per wave that reads it);
//   * one LDS buffer (51 KB: three workgroups per CU), two barriers per chunk; the next chunk's global loads are issued in front of the
//     matrix phase and are in flight during it.
constexpr int WL_HPL = 64 * 16 + 64;              // one K half of a (component, limb) plane: 64 rows x 16 B, padded (bank spread of the two halves)
constexpr int WL_PLANE = 2 * WL_HPL;
constexpr int WL_OP = 12 * WL_PLANE;              // one operand: 4 components x 3 limbs
constexpr int WL_LDS_BYTES = 2 * WL_OP;


template <bool REFL>          // reflection (decoder) or zero (ResNet trunk) padding
__global__ void __launch_bounds__(WNT) k_wgrad_wino_limb(WinoWgradArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned char* smemb = reinterpret_cast<unsigned char*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1;
    const int HT = g.H >> 1;
    constexpr int R = 4;
    const int plane2 = HT * W2, Np = g.Nb * plane2;
    const unsigned hw = (unsigned)(g.H * g.W);
    const int ctiles = (g.C + WBN - 1) / WBN;
    int bt, bs, by;
    if (g.slice_major == 2) {                                    // XCD-aware 1-D grid (k_wgrad_wino)
        const int mtiles = (g.M + WBM - 1) / WBM, nt = R * ctiles * mtiles;
        const int L = blockIdx.x, xcd = L & 7, k = L >> 3;
        int t;
        if (g.xcds_per_slice <= 1) { t = k % nt; bs = (k / nt) * 8 + xcd; }
        else { const int per = nt / g.xcds_per_slice; bs = xcd / g.xcds_per_slice; t = (xcd % g.xcds_per_slice) * per + k; }
        by = t / (R * ctiles);
        bt = t - by * R * ctiles;
    } else {
        bt = g.slice_major ? blockIdx.z : blockIdx.x; bs = g.slice_major ? blockIdx.x : blockIdx.z; by = blockIdx.y;
    }
    const int ky = bt / ctiles, c0 = (bt - ky * ctiles) * WBN;
    const int m0 = by * WBM;
    const int pp_lo = (int)((long)bs * g.pairs_per_split < Np ? (long)bs * g.pairs_per_split : Np);
    const int pp_hi = (long)pp_lo + g.pairs_per_split < Np ? pp_lo + (int)g.pairs_per_split : Np;
    const int nchunk = pp_hi > pp_lo ? (pp_hi - pp_lo + WGP - 1) / WGP : 0;

    // ---- loader: thread = (row tid / 4 of both operands, QUAD tid % 4 = four consecutive pairs of the chunk, one tile row: W / 2 % 4 == 0).
    // Four adjacent lanes read 128 contiguous bytes of a dY row; two pairs of one component make one split2 (a dword = two consecutive K
    // positions), a quad an 8-byte store into the fragment - the first version (a thread = one pair of four rows, 2-byte stores: 96 LDS
    // store instructions per thread and chunk) ran at 0.76x the f32 kernel (profiles/round6_wgrad_wino_limb.log).
    const int q = tid & 3, row = tid >> 2;
    unsigned a_row, b_row;
    {
        int m = m0 + row; m = m < g.M ? m : g.M - 1;
        int c = c0 + row; c = c < g.C ? c : g.C - 1;
        a_row = 4u * (unsigned)m * hw; b_row = 4u * (unsigned)c * hw;
    }
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(g.dY);
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.X), 0, (int)(4u * (unsigned)g.Nb * (unsigned)g.C * hw), 0x00020000);
    // (a register ring of two chunks - loads two iterations ahead - measured the same alone and in the step at 196 registers: removed)
    float4 ya[1][2], yb[1][2];                 // dY: 8 columns of the two tile rows
    float4 xa[1][2], xb[1][2];                 // X: columns 2j-1 .. 2j+6 (left edge: 2j .. 2j+7) of the two combined rows ...
    f32x2 xa2[1], xb2[1];                      // ... and 2j+7, 2j+8 (left edge: 2j+8, 2j+9)
    unsigned a_off = FD_OOB, x_off = FD_OOB, a_off2 = FD_OOB, x_off2 = FD_OOB;
    const int yr_a = ky == 3 ? 1 : 0;
    const bool y_two = ky == 1 || ky == 2;
    const float y_sgn = ky == 2 ? -1.f : 1.f;
    const int xr_a = ky == 0 ? 0 : (ky == 2 ? 2 : 1), xr_b = ky == 3 ? 3 : (ky == 2 ? 1 : 2);
    const float x_sgn = ky == 1 ? 1.f : -1.f;
    int pf = 0, rf = 0;                        // bit 0 / 1: the quad starts / ends an image row
    int pc = pp_lo;
    int cn, cy, cj;
    {
        const int pq = pp_lo + 4 * q;
        cn = pq / plane2;
        const int rem = pq - cn * plane2;
        cy = rem / W2; cj = rem - cy * W2;
    }
    auto prep_chunk = [&](bool live) __attribute__((always_inline)) {
        const int pg = pc + 4 * q;
        const bool ok = live & (pg < pp_hi);
        const int n = cn, y = cy, j = cj;
        const bool e_left = j == 0, e_right = 2 * j + 8 >= g.W;
        auto x_row = [&](int r) __attribute__((always_inline)) {
            const bool inb = (unsigned)r < (unsigned)g.H;
            int rr_ = r < 0 ? -r : r;
            rr_ = rr_ >= g.H ? 2 * g.H - 2 - rr_ : rr_;
            const int ruse = REFL ? rr_ : r;
            const bool okb = ok & (REFL | inb);
            const unsigned base = 4u * ((unsigned)n * (unsigned)g.C * hw + (unsigned)(ruse * g.W + 2 * j));
            return okb ? (e_left ? base : base - 4u) : FD_OOB;
        };
        const unsigned yo = 4u * ((unsigned)n * (unsigned)g.M * hw + (unsigned)((2 * y + yr_a) * g.W + 2 * j));
        a_off = ok ? yo : FD_OOB;
        a_off2 = (ok & y_two) ? yo + 4u * (unsigned)g.W : FD_OOB;
        x_off = x_row(2 * y - 1 + xr_a);
        x_off2 = x_row(2 * y - 1 + xr_b);
        pf = (e_left ? 1 : 0) | (e_right ? 2 : 0);
        pc += WGP;
        cj += g.adv_j;
        const bool c1 = cj >= W2;
        cj -= c1 ? W2 : 0;
        cy += g.adv_y + (c1 ? 1 : 0);
        const bool c2 = cy >= HT;
        cy -= c2 ? HT : 0;
        cn += g.adv_n + (c2 ? 1 : 0);
    };
    auto load_all = [&](auto slot_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(slot_tag)::value;
        ya[S][0] = fd_ldg128(rsY, a_off + a_row); ya[S][1] = fd_ldg128(rsY, a_off + a_row + 16u);
        yb[S][0] = fd_ldg128(rsY, a_off2 + a_row); yb[S][1] = fd_ldg128(rsY, a_off2 + a_row + 16u);
        xa[S][0] = fd_ldg128(rsX, x_off + b_row); xa[S][1] = fd_ldg128(rsX, x_off + b_row + 16u); xa2[S] = fd_ldg64(rsX, x_off + b_row + 32u);
        xb[S][0] = fd_ldg128(rsX, x_off2 + b_row); xb[S][1] = fd_ldg128(rsX, x_off2 + b_row + 16u); xb2[S] = fd_ldg64(rsX, x_off2 + b_row + 32u);
    };
    // this quad's 8-byte slot inside the fragments of its row: K half q / 2, positions 4 (q % 2) .. + 3
    unsigned char* const slot = smemb + (q >> 1) * WL_HPL + row * 16 + 8 * (q & 1);
    auto store_all = [&](auto slot_tag) __attribute__((always_inline)) {
        constexpr int S = decltype(slot_tag)::value;
        // vertical combinations (exact products: a +- b)
        float Y[8], X[10];
        Y[0] = fmaf(y_sgn, yb[S][0].x, ya[S][0].x); Y[1] = fmaf(y_sgn, yb[S][0].y, ya[S][0].y); Y[2] = fmaf(y_sgn, yb[S][0].z, ya[S][0].z); Y[3] = fmaf(y_sgn, yb[S][0].w, ya[S][0].w);
        Y[4] = fmaf(y_sgn, yb[S][1].x, ya[S][1].x); Y[5] = fmaf(y_sgn, yb[S][1].y, ya[S][1].y); Y[6] = fmaf(y_sgn, yb[S][1].z, ya[S][1].z); Y[7] = fmaf(y_sgn, yb[S][1].w, ya[S][1].w);
        float r[10];
        r[0] = fmaf(x_sgn, xb[S][0].x, xa[S][0].x); r[1] = fmaf(x_sgn, xb[S][0].y, xa[S][0].y); r[2] = fmaf(x_sgn, xb[S][0].z, xa[S][0].z); r[3] = fmaf(x_sgn, xb[S][0].w, xa[S][0].w);
        r[4] = fmaf(x_sgn, xb[S][1].x, xa[S][1].x); r[5] = fmaf(x_sgn, xb[S][1].y, xa[S][1].y); r[6] = fmaf(x_sgn, xb[S][1].z, xa[S][1].z); r[7] = fmaf(x_sgn, xb[S][1].w, xa[S][1].w);
        r[8] = fmaf(x_sgn, xb2[S].x, xa2[S].x); r[9] = fmaf(x_sgn, xb2[S].y, xa2[S].y);
        // columns 2j-1 .. 2j+8; a quad at the left edge was loaded from column 2j on (shift); its column -1 and the right edge's column W
        // are the padding: 0, or the mirror columns 1 and W - 2
        const bool L = rf & 1, Rr = rf & 2;
#pragma unroll
        for (int k = 1; k < 10; ++k) X[k] = L ? r[k - 1] : r[k];
        X[0] = L ? (REFL ? X[2] : 0.f) : r[0];
        X[9] = Rr ? (REFL ? X[7] : 0.f) : X[9];
        // horizontal transforms of the four pairs, limbs, fragments (component t: planes 3 t .. 3 t + 2 = limbs h, m, l)
        unsigned char* qa = slot;
        unsigned char* qb = slot + WL_OP;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float pv[4], qv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float y0 = Y[2 * k], y1 = Y[2 * k + 1];
                const float d0 = X[2 * k], d1 = X[2 * k + 1], d2 = X[2 * k + 2], d3 = X[2 * k + 3];
                pv[k] = t == 0 ? y0 : (t == 1 ? y0 + y1 : (t == 2 ? y0 - y1 : y1));
                qv[k] = t == 0 ? d0 - d2 : (t == 1 ? d1 + d2 : (t == 2 ? d2 - d1 : d1 - d3));
            }
            unsigned h0, m0_, l0, h1, m1, l1;
            fdlimb::split2(pv[0], pv[1], h0, m0_, l0); fdlimb::split2(pv[2], pv[3], h1, m1, l1);
            *reinterpret_cast<u32x2*>(qa + (3 * t) * WL_PLANE) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(qa + (3 * t + 1) * WL_PLANE) = u32x2{m0_, m1};
            *reinterpret_cast<u32x2*>(qa + (3 * t + 2) * WL_PLANE) = u32x2{l0, l1};
            fdlimb::split2(qv[0], qv[1], h0, m0_, l0); fdlimb::split2(qv[2], qv[3], h1, m1, l1);
            *reinterpret_cast<u32x2*>(qb + (3 * t) * WL_PLANE) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(qb + (3 * t + 1) * WL_PLANE) = u32x2{m0_, m1};
            *reinterpret_cast<u32x2*>(qb + (3 * t + 2) * WL_PLANE) = u32x2{l0, l1};
        }
    };

    const int wm = wave >> 1, wn = wave & 1;
    const int arow = lane >> 5, acol = lane & 31;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    if (nchunk > 0) {
        constexpr std::integral_constant<int, 0> S0{};
        prep_chunk(true);
        rf = pf;
        load_all(S0);
        prep_chunk(1 < nchunk);
        const unsigned char* fa = smemb + arow * WL_HPL + (32 * wm + acol) * 16;
        const unsigned char* fb = smemb + WL_OP + arow * WL_HPL + (32 * wn + acol) * 16;
        for (int ch = 0; ch < nchunk; ++ch) {
            store_all(S0);
            __syncthreads();
            load_all(S0);                                             // chunk ch + 1: in flight during the matrix phase
            rf = pf;
            prep_chunk(ch + 2 < nchunk);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                uint4 af[3], bf[3];
#pragma unroll
                for (int Lm = 0; Lm < 3; ++Lm) {
                    af[Lm] = *reinterpret_cast<const uint4*>(fa + (t * 3 + Lm) * WL_PLANE);
                    bf[Lm] = *reinterpret_cast<const uint4*>(fb + (t * 3 + Lm) * WL_PLANE);
                }
                FD_WLIMB_MFMA6(acc[t], af, bf);
            }
            __syncthreads();
        }
    }
    // ---- epilogue (k_wgrad_wino's): slab[z][m][ri * 3 + kx][c] from the four accumulators
    const int c = c0 + 32 * wn + acol;
    const __amdgpu_buffer_rsrc_t rsS = fd_make_rsrc(g.slabs + (size_t)bs * ((size_t)g.M * (3 * R) * g.C));
    const int mb = m0 + 32 * wm + 4 * arow;
    const unsigned col = (c < g.C) ? 4u * (unsigned)(ky * 3 * g.C + c) : FD_OOB;
    const unsigned row_step = 4u * (3u * R) * (unsigned)g.C, kx_step = 4u * (unsigned)g.C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        const unsigned off = (m < g.M) ? col + (unsigned)m * row_step : FD_OOB;
        const float M0 = acc[0][r], M1 = acc[1][r], M2 = acc[2][r], M3 = acc[3][r];
        const float hh = 0.5f * (M1 + M2);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, M0 + hh), rsS, (int)off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, 0.5f * (M1 - M2)), rsS, (int)(off + kx_step), 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, hh - M3), rsS, (int)(off + 2u * kx_step), 0, 0);
    }
}
}  // namespace

// ---- weight gradient
bool wino_wgrad_ok(const fd_conv_desc* d) {
    return d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->Cin % 16 == 0 && d->Cin >= 64 && d->Cout >= fd_tun().wino_wgrad_min_cout &&
           d->W % 2 == 0 && !d->in_norm;
}
// The 2-D algorithm needs whole 2x2 tiles of dY (fd_tuning.wino_wgrad_2d = 0: the 1-D kernel everywhere, for A/B timing)
bool wino_wgrad_2d(const fd_conv_desc* d) {
    // wino_wgrad_2d = 1: where Cin is a multiple of 32 (rounds 4-5); 2: every Cin the Winograd path takes (multiples of 16: the
    // Refiner decoder's 272 / 144 / 112-channel layers)
    const int mode = fd_tun().wino_wgrad_2d;
    return mode != 0 && d->H % 2 == 0 && (d->Cin % 32 == 0 || mode >= 2);
}
int wino_wgrad_splits(const fd_conv_desc* d) {
    const bool twod = wino_wgrad_2d(d);
    const long tiles = (twod ? 4L : 3L) * fd_cdiv(d->Cin, WBN) * fd_cdiv(d->Cout, WBM);
    const long Np = (long)d->N * (twod ? d->H / 2 : d->H) * (d->W / 2);
    const long target = fd_tun().wino_wgrad_target;          // in-step optimum 384 (768: -1 %)
    long sp = target / tiles;
    const long maxs = (Np + 4 * WGP - 1) / (4 * WGP);          // at least 4 chunks per split
    if (sp > maxs) sp = maxs;
    if (sp > 512) sp = 512;
    if (sp >= 8) sp &= ~7L;                                     // XCD alignment, see k_wgrad_wino
    if (sp < 1) sp = 1;
    return (int)sp;
}
long wino_wgrad_ws_floats(const fd_conv_desc* d) { return (long)wino_wgrad_splits(d) * d->Cout * (wino_wgrad_2d(d) ? 12 : 9) * d->Cin; }
int wino_wgrad_launch(const fd_conv_desc* d, const float* x, const float* gy, float* gw, float* ws, int accumulate, hipStream_t st) {
    WinoWgradArgs g = {};
    g.dY = gy; g.X = x; g.slabs = ws;
    g.M = d->Cout; g.C = d->Cin; g.Nb = d->N; g.H = d->H; g.W = d->W; g.pad_mode = d->pad_mode;
    const int sp = wino_wgrad_splits(d);
    const bool twod = wino_wgrad_2d(d);
    const int HT = twod ? d->H / 2 : d->H;
    g.slab_rows = twod ? 12 : 9;
    const long Np = (long)d->N * HT * (d->W / 2);
    long pps = (Np + sp - 1) / sp;
    pps = (pps + WGP - 1) / WGP * WGP;
    g.pairs_per_split = pps;
    {
        const int W2 = d->W / 2, plane2 = HT * W2;
        g.adv_n = WGP / plane2;
        const int rem = WGP - g.adv_n * plane2;
        g.adv_y = rem / W2; g.adv_j = rem - g.adv_y * W2;
    }
    const int slice_major = 2;        // XCD-aware 1-D grid: layer1 HBM traffic 157 -> 76 MB per launch, step -0.5 %; (1: slice-major 3-D grid measured slower than 0)
    g.slice_major = slice_major;
    const int nt = (twod ? 4 : 3) * fd_cdiv(d->Cin, WBN);
    const int mt = fd_cdiv(d->Cout, WBM);
    g.xcds_per_slice = 1;
    if (slice_major == 2 && sp % 8 != 0) {                                // the XCD map needs whole groups of 8 slices ...
        const int q = (sp == 2 || sp == 4) ? 8 / sp : 0;                  // ... or 2 / 4 slices that own 4 / 2 XCDs each
        if (q > 0 && (nt * mt) % q == 0 && fd_tun().wino_wgrad_xcd_few != 0) g.xcds_per_slice = q;
        else g.slice_major = 0;
    }
    const dim3 grid = g.slice_major == 2 ? dim3((unsigned)(nt * mt * sp)) : (g.slice_major ? dim3(sp, mt, nt) : dim3(nt, mt, sp));
    const size_t lds = sizeof(float) * WG_LDS_FLOATS;
    const bool halfm = d->Cout <= 32 && fd_tun().wino_wgrad_halfm != 0;   // at most 32 output channels: two waves per K half (k_wgrad_wino<.., HALFM>)
    const bool refl = d->pad_mode == 1;
    if (fd_tun().wino_wgrad_limb != 0 && twod && (d->pad_mode == 0 || fd_tun().wino_wgrad_limb >= 2) && d->Cout >= 64 && d->W % 8 == 0) {
        // split-precision matrix loop: the ResNet trunk's layers (wino_wgrad_limb = 1), the reflect-padded decoder blocks as well (2)
        if (refl) fd_launch_lds<k_wgrad_wino_limb<true>>(grid, dim3(WNT), (size_t)WL_LDS_BYTES, st, g);
        else fd_launch_lds<k_wgrad_wino_limb<false>>(grid, dim3(WNT), (size_t)WL_LDS_BYTES, st, g);
    } else if (twod && halfm) {
        if (refl) fd_launch_lds<k_wgrad_wino<true, true, true>>(grid, dim3(WNT), lds, st, g);
        else fd_launch_lds<k_wgrad_wino<false, true, true>>(grid, dim3(WNT), lds, st, g);
    } else if (halfm) {
        if (refl) fd_launch_lds<k_wgrad_wino<true, false, true>>(grid, dim3(WNT), lds, st, g);
        else fd_launch_lds<k_wgrad_wino<false, false, true>>(grid, dim3(WNT), lds, st, g);
    } else if (twod) {
        if (refl) fd_launch_lds<k_wgrad_wino<true, true>>(grid, dim3(WNT), lds, st, g);
        else fd_launch_lds<k_wgrad_wino<false, true>>(grid, dim3(WNT), lds, st, g);
    } else {
        if (refl) fd_launch_lds<k_wgrad_wino<true, false>>(grid, dim3(WNT), lds, st, g);
        else fd_launch_lds<k_wgrad_wino<false, false>>(grid, dim3(WNT), lds, st, g);
    }
    FD_LAUNCH_CHECK("k_wgrad_wino");
    return fast_wgrad_finish_launch(ws, gw, d->Cout, d->Cin, twod ? 12 : 9, sp, accumulate, st);
}
