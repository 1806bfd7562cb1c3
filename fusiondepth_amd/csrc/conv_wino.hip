// 3x3 stride-1 convolutions with the Winograd F(2x2, 3x3) transform computed by ONE workgroup per output tile: k_conv_wino2p and
// k_conv_wino2p_dma, the training step's dominant kernels (the roofline probe of bench.py reads this file).  The other Winograd
// families: conv_wino.h.
#include "conv_wino.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------ F(2x2, 3x3) in ONE workgroup
// k_conv_wino2p (round 4): the 16 components of F(2x2, 3x3) for the layers where slabs cost more than the matrix work they save
// (ResNet layer1 / layer2, the decoder's wide blocks: few channels, many pixels - the 1-D kernel's territory until now).  A
// workgroup keeps its 64 (channels) x 64 (2x2 tiles) output tile for the WHOLE computation and runs the four row components one
// after the other through the same four horizontal accumulators: GEMM-K = (ri, input channel), a flat sequence of 4 C / 16 chunks
// fed by one uninterrupted register-staged pipeline (the 2-D loader of k_conv_wino2d with ri advancing per chunk).  At the end of
// a row component the horizontal output transform h = (M0 + M1 + M2, M1 - M2 - M3) is folded into two more accumulator pairs - the
// vertical output transform y[2 ty] = S0 + S1 + S2, y[2 ty + 1] = S1 - S2 - S3 is linear - and the epilogue writes FINAL outputs
// (bias, activation, residual, BatchNorm partial sums): no slabs, no finishing launch, 16 instead of 24 products per 2x2 tile,
// K loops a third longer than the 1-D kernel's (4 C / 16 against 3 C / 16 chunks per tile of twice the pixels), and the four row
// combinations of a tile's input rows are formed by ONE workgroup out of L1 / L2 instead of four.  128 accumulator registers per
// lane: two waves per SIMD.
// Final outputs of a k_conv_wino2p tile from the two folded accumulator pairs (shared by the register-staged and the direct-to-LDS
// variant of the kernel)
template <bool STATS>
__device__ __forceinline__ void w2p_epilogue(const WinoArgs& g, const f32x16 (&ya)[2], const f32x16 (&yb)[2], int p0, int m0, int Np, int plane2,
                                             int W2, unsigned hw, int lane, int wm, int wn) {
    const int arow = lane >> 5, acol = lane & 31;
    // ---- epilogue: final outputs of the tile's two rows (C/D layout: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5))
    const int po = p0 + 32 * wn + acol;
    unsigned out_base = FD_OOB;
    if (po < Np) {
        const int n = po / plane2;
        const int rem = po - n * plane2;
        const int yy = rem / W2, jj = rem - yy * W2;
        out_base = 4u * ((unsigned)n * (unsigned)g.M * hw + (unsigned)(2 * yy * g.W + 2 * jj));
    }
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(g.Y);
    const __amdgpu_buffer_rsrc_t rsAdd = fd_make_rsrc(g.add ? g.add : g.Y);
    const bool has_add = g.add != nullptr;
    const int mbase = m0 + 32 * wm + 4 * arow;
    const unsigned row_b = 4u * (unsigned)g.W;
    float bias_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = 0.f;
    if (g.bias) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mbase + (r & 3) + 8 * (r >> 2);
            bias_r[r] = g.bias[m < g.M ? m : g.M - 1];
        }
    }
    float s1[16], s2[16];                       // STATS: (sum, M2) of each row's four pixels
    auto rows = [&](auto act_tag) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mbase + (r & 3) + 8 * (r >> 2);
            const unsigned off = (m < g.M) ? out_base + 4u * (unsigned)m * hw : FD_OOB;
            f32x2 oa, ob;
            oa.x = ya[0][r] + bias_r[r]; oa.y = ya[1][r] + bias_r[r];
            ob.x = yb[0][r] + bias_r[r]; ob.y = yb[1][r] + bias_r[r];
            if (ACT != 0) { oa.x = wino_act(oa.x, g.act); oa.y = wino_act(oa.y, g.act); ob.x = wino_act(ob.x, g.act); ob.y = wino_act(ob.y, g.act); }
            if (has_add) {
                const f32x2 a2 = fd_ldg64(rsAdd, off), b2 = fd_ldg64(rsAdd, off + row_b);
                oa.x += a2.x; oa.y += a2.y; ob.x += b2.x; ob.y += b2.y;
            }
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, oa), rsY, (int)off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, ob), rsY, (int)(off + row_b), 0, 0);
            if (STATS) {
                const float da = oa.x - oa.y, db = ob.x - ob.y;
                const float ta = oa.x + oa.y, tb = ob.x + ob.y, dab = ta - tb;
                s1[r] = ta + tb;
                s2[r] = fmaf(dab * dab, 0.25f, 0.5f * da * da + 0.5f * db * db);      // two pairs of two: (sa - sb)^2 / (2 * 2)
            }
        }
    };
    if (g.act == 0) rows(std::integral_constant<int, 0>{});
    else rows(std::integral_constant<int, -1>{});
    if (STATS) {
        // the butterfly of k_conv_wino with four pixels per lane and row to start from: slots of 32 tiles = 128 pixels
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const int width = 8 >> step;
            const int xm = 16 >> step;
            const bool hi = (lane & xm) != 0;
            const float inv2n = 0.125f / (float)(1 << step);                // each side holds n = 4 << step pixels
#pragma unroll
            for (int j = 0; j < width; ++j) {
                const float k1 = hi ? s1[j + width] : s1[j], g1 = hi ? s1[j] : s1[j + width];
                const float k2 = hi ? s2[j + width] : s2[j], g2 = hi ? s2[j] : s2[j + width];
                const float o1 = __shfl_xor(g1, xm, 64), o2 = __shfl_xor(g2, xm, 64);
                const float df = k1 - o1;
                s1[j] = k1 + o1;
                s2[j] = fmaf(df * df, inv2n, k2 + o2);
            }
        }
        {
            const float o1 = __shfl_xor(s1[0], 1, 64), o2 = __shfl_xor(s2[0], 1, 64);
            const float df = s1[0] - o1;
            s2[0] = fmaf(df * df, 1.0f / 128.0f, s2[0] + o2);               // n = 64 per side
            s1[0] += o1;
        }
        const int rr = ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
        const int m = mbase + (rr & 3) + 8 * (rr >> 2);
        const int n = p0 / plane2, tile = (p0 - n * plane2) / WBN;         // the whole tile lies in image n (launcher's guarantee)
        if (!(lane & 1) && m < g.M && 2 * tile + wn < g.stat_slots) {      // (image-aligned tiling: the last tile's second half may be empty)
            f32x2 v; v.x = s1[0]; v.y = s2[0];
            *reinterpret_cast<f32x2*>(g.stat_part + (((size_t)n * g.M + m) * g.stat_slots + 2 * tile + wn) * 2) = v;
        }
    }
}

template <bool STATS>
__global__ void __launch_bounds__(WNT) __attribute__((amdgpu_waves_per_eu(2, 2))) k_conv_wino2p(WinoArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1, HT = g.H >> 1;
    const int plane2 = HT * W2;                                          // 2x2 tiles per image; Nb * plane2 < 2^29 (size guard)
    const int Np = g.Nb * plane2;
    const unsigned hw = (unsigned)(g.H * g.W);
    int bx = blockIdx.x;
    const int by = blockIdx.y;
    if (g.xcd_swizzle) { const int per = gridDim.x >> 3; bx = (bx & 7) * per + (bx >> 3); }     // vertical neighbours share input rows: same XCD
    const int m0 = by * WBM, p0 = bx * WBN;
    const int cpt = g.C / WBKC, nchunk = 4 * cpt;
    auto ri_of = [&](int f) __attribute__((always_inline)) { return (f >= cpt ? 1 : 0) + (f >= 2 * cpt ? 1 : 0) + (f >= 3 * cpt ? 1 : 0); };

    // ---- activation loader: this thread always fetches tile jn of the workgroup's 64, channel rows kr + 4 i
    const int jn = lane, kr = wave;
    const int pg = p0 + jn;
    const bool pvalid = pg < Np;
    int y0, j0;
    unsigned nbase;
    {
        const int pp = pvalid ? pg : 0;
        const int n = pp / plane2;
        const int rem = pp - n * plane2;
        y0 = rem / W2; j0 = rem - y0 * W2;
        nbase = (unsigned)n * (unsigned)g.C * hw;
    }
    const bool refl = g.pad_mode == 1;
    const bool left_edge = j0 == 0, right_edge = 2 * j0 + 2 >= g.W;
    const bool halo_l = jn == 0 && !left_edge, halo_r = jn == WBN - 1 && !right_edge;
    const int a4 = tid & 3, ar = tid >> 2;
    int mrow = m0 + ar;
    mrow = mrow < g.M ? mrow : g.M - 1;
    const unsigned u_comp = 4u * (unsigned)g.M * 4u * (unsigned)g.C;     // bytes between components of U2[t][m][ri][c]
    const __amdgpu_buffer_rsrc_t rsU = fd_make_rsrc(g.U), rsX = fd_make_rsrc(g.X);
    float4 ru[4];
    f32x2 rmid[4], rmid2[4];
    float rh[4], rh2[4];
    unsigned u_off = FD_OOB, mid_off = FD_OOB, h_off = FD_OOB, mid_off2 = FD_OOB, h_off2 = FD_OOB;
    const unsigned c_step = 4u * 4u * hw;
    int pc_f = 0;                                                        // flat chunk index being prepared
    int pc_ri = 0, pc_c0 = 0;
    unsigned prep_base = 0u, prep_base2 = 0u;
    bool prep_ok = false, prep_ok2 = false;
    const int H2m2 = 2 * g.H - 2;
    auto prep_a = [&]() __attribute__((always_inline)) {
        const bool live = pc_f < nchunk;
        const int ri = pc_ri;
        const int xr_a = ri == 0 ? 0 : (ri == 2 ? 2 : 1), xr_b = ri == 3 ? 3 : (ri == 2 ? 1 : 2);
        u_off = live ? 4u * (((unsigned)mrow * 4u + (unsigned)ri) * (unsigned)g.C + (unsigned)pc_c0 + 4u * a4) : FD_OOB;
        auto row = [&](int r, bool& ok, unsigned& base) __attribute__((always_inline)) {
            const bool inb = (unsigned)r < (unsigned)g.H;
            int rr_ = r < 0 ? -r : r;
            rr_ = rr_ >= g.H ? H2m2 - rr_ : rr_;
            const int ruse = refl ? rr_ : r;
            ok = pvalid & live & (refl | inb);
            base = 4u * (nbase + (unsigned)(pc_c0 + kr) * hw + (unsigned)(ruse * g.W + 2 * j0));
        };
        row(2 * y0 - 1 + xr_a, prep_ok, prep_base);
        row(2 * y0 - 1 + xr_b, prep_ok2, prep_base2);
    };
    auto prep_b = [&]() __attribute__((always_inline)) {
        mid_off = prep_ok ? prep_base : FD_OOB;
        h_off = (prep_ok & halo_l) ? prep_base - 4u : ((prep_ok & halo_r) ? prep_base + 8u : FD_OOB);
        mid_off2 = prep_ok2 ? prep_base2 : FD_OOB;
        h_off2 = (prep_ok2 & halo_l) ? prep_base2 - 4u : ((prep_ok2 & halo_r) ? prep_base2 + 8u : FD_OOB);
        ++pc_f;
        pc_c0 += WBKC;
        const bool wrap = pc_c0 >= g.C;
        pc_c0 = wrap ? 0 : pc_c0;
        pc_ri += wrap ? 1 : 0;
    };
    auto load_u = [&](int t) __attribute__((always_inline)) { ru[t] = fd_ldg128(rsU, u_off + (unsigned)t * u_comp); };
    auto load_mid = [&](int i) __attribute__((always_inline)) {
        rmid[i] = fd_ldg64(rsX, mid_off + (unsigned)i * c_step);
        rmid2[i] = fd_ldg64(rsX, mid_off2 + (unsigned)i * c_step);
    };
    auto load_h = [&](int i) __attribute__((always_inline)) {
        rh[i] = fd_ldg32(rsX, h_off + (unsigned)i * c_step);
        rh2[i] = fd_ldg32(rsX, h_off2 + (unsigned)i * c_step);
    };
    auto store_u = [&](int buf, int t) __attribute__((always_inline)) {
        float* q = smem + buf * W_BUF_FLOATS + t * WBKC * LDU + (4 * a4) * LDU + ar;
        q[0] = ru[t].x; q[LDU] = ru[t].y; q[2 * LDU] = ru[t].z; q[3 * LDU] = ru[t].w;
    };
    const int v_row = 4 * WBKC * LDU + kr * LDR;
    const int h_col = jn == 0 ? 3 : 2 * WBN + 4;
    // `sgn`: sign of the second row in the row combination of the chunk whose data sit in the staging registers (+1 for ri = 1)
    auto store_v = [&](int buf, int i, float sgn) __attribute__((always_inline)) {
        float* q = smem + buf * W_BUF_FLOATS + v_row + 4 * i * LDR;
        rmid[i].x = fmaf(sgn, rmid2[i].x, rmid[i].x); rmid[i].y = fmaf(sgn, rmid2[i].y, rmid[i].y);
        rh[i] = fmaf(sgn, rh2[i], rh[i]);
        *reinterpret_cast<f32x2*>(q + 4 + 2 * jn) = rmid[i];
        if (jn == 0 || jn == WBN - 1) q[h_col] = rh[i];
    };

    const int wm = wave >> 1, wn = wave & 1;
    int o12, o0, o3;
    float ml, mr;
    {
        const int jp = 32 * wn + (lane & 31);
        const int pp = p0 + jp < Np ? p0 + jp : 0;
        const int rem = pp % plane2;
        const int jj = rem % W2;
        const bool le = jj == 0, re = 2 * jj + 2 >= g.W;
        o12 = 4 + 2 * jp;
        o0 = (le && refl) ? o12 : o12 - 2;       // 8-byte cell whose .y is d0 (reflection: column -1 is column 1 = d12.y)
        o3 = (re && refl) ? o12 : o12 + 2;       // 8-byte cell whose .x is d3 (reflection: column W is column W - 2 = d12.x)
        ml = (le && !refl) ? 0.f : 1.f;
        mr = (re && !refl) ? 0.f : 1.f;
    }
    f32x16 acc[4], ya[2], yb[2];                 // working components; output rows 2 ty (ya) / 2 ty + 1 (yb), columns 2 j / 2 j + 1
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][r] = 0.f;
        ya[0][r] = ya[1][r] = yb[0][r] = yb[1][r] = 0.f;
    }

    constexpr int NK = WBKC / 2, LS = NK / 2;
    const int arow = lane >> 5, acol = lane & 31;
    {
        prep_a(); prep_b();
#pragma unroll
        for (int t = 0; t < 4; ++t) load_u(t);
#pragma unroll
        for (int i = 0; i < 4; ++i) { load_mid(i); load_h(i); }
#pragma unroll
        for (int t = 0; t < 4; ++t) store_u(0, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) store_v(0, i, -1.f);             // chunk 0 is ri = 0: x_r0 - x_r2
        prep_a(); prep_b();                                          // chunk 1: loaded now, written to LDS during chunk 0
#pragma unroll
        for (int t = 0; t < 4; ++t) load_u(t);
#pragma unroll
        for (int i = 0; i < 4; ++i) { load_mid(i); load_h(i); }
        prep_a(); prep_b();                                          // offsets of chunk 2, re-loaded during chunk 0
        __syncthreads();
        int next_fold = cpt - 1;                                     // last chunk of the current row component
        int ri_cur = 0;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int cur = ch & 1;
            const float sgn_regs = ri_of(ch + 1) == 1 ? 1.f : -1.f;  // the registers hold chunk ch + 1
            const float* pa = smem + cur * W_BUF_FLOATS + arow * LDU + 32 * wm + acol;
            const float* pr = smem + cur * W_BUF_FLOATS + 4 * WBKC * LDU + arow * LDR;
            float av[2][4], bv[2][4];
            auto read_a = [&](int nb, int k2, int t) __attribute__((always_inline)) { av[nb][t] = pa[t * WBKC * LDU + k2 * LDU]; };
            f32x2 d12, dl, dr;                                           // three 8-byte reads (conflict-free at stride 8 over a half-wave;
            auto read_b = [&](int k2) __attribute__((always_inline)) {   // the 4-byte reads of d0 / d3 at stride 8 were 2-way bank conflicts)
                d12 = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o12);
                dl = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o0); dr = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o3);
            };
            auto xform_b = [&](int nb) __attribute__((always_inline)) {
                asm volatile("" : "+v"(dl), "+v"(dr));                   // both halves live: keeps the reads 8 bytes wide
                bv[nb][0] = fmaf(dl.y, ml, -d12.y); bv[nb][1] = d12.x + d12.y; bv[nb][2] = d12.y - d12.x; bv[nb][3] = fmaf(-dr.x, mr, d12.x);
            };
#pragma unroll
            for (int t = 0; t < 4; ++t) read_a(0, 0, t);
            read_b(0); xform_b(0);
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                const int cb = kk & 1, nb = cb ^ 1;
                __builtin_amdgcn_sched_barrier(0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0], bv[cb][0], acc[0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NK) { read_b(2 * (kk + 1)); read_a(nb, 2 * (kk + 1), 0); read_a(nb, 2 * (kk + 1), 1); }
                if (kk < LS) store_u(cur ^ 1, kk);
                __builtin_amdgcn_sched_barrier(0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1], bv[cb][1], acc[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NK) { read_a(nb, 2 * (kk + 1), 2); read_a(nb, 2 * (kk + 1), 3); }
                if (kk < LS) load_u(kk);
                __builtin_amdgcn_sched_barrier(0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][2], bv[cb][2], acc[2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < LS) store_v(cur ^ 1, kk, sgn_regs);
                if (kk + 1 < NK) xform_b(nb);
                __builtin_amdgcn_sched_barrier(0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][3], bv[cb][3], acc[3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < LS) { load_mid(kk); load_h(kk); }
                if (kk == NK - 2) prep_a();                          // chunk ch + 3; every load of chunk ch + 2 has been issued by now
                if (kk == NK - 1) prep_b();
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ch == next_fold) {
                // end of row component ri_cur: fold the horizontally transformed products into the two output rows and start afresh
                const float sa = ri_cur <= 2 ? 1.f : 0.f;             // y[2 ty]     = S0 + S1 + S2
                const float sb = ri_cur == 0 ? 0.f : (ri_cur == 1 ? 1.f : -1.f);   // y[2 ty + 1] = S1 - S2 - S3
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float h0 = (acc[0][r] + acc[1][r]) + acc[2][r];
                    const float h1 = (acc[1][r] - acc[2][r]) - acc[3][r];
                    ya[0][r] = fmaf(sa, h0, ya[0][r]); ya[1][r] = fmaf(sa, h1, ya[1][r]);
                    yb[0][r] = fmaf(sb, h0, yb[0][r]); yb[1][r] = fmaf(sb, h1, yb[1][r]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t][r] = 0.f;
                }
                next_fold += cpt;
                ++ri_cur;
            }
            __syncthreads();
        }
    }
    w2p_epilogue<STATS>(g, ya, yb, p0, m0, Np, plane2, W2, hw, lane, wm, wn);
}

// The same computation with the activations on the LDS-DMA path (needs W % 4 == 0, a 16-byte aligned tensor): BOTH input rows of the
// chunk's row combination go from global memory straight into LDS as raw rows (`buffer_load_dwordx4 ... lds`, three 1-KB pieces per
// wave and row set), and the vertical AND the horizontal input transform are applied when the B operands are read:
//   d = rowA + sgn * rowB  (4 fused multiply-adds),  V = (d0 - d2, d1 + d2, d2 - d1, d1 - d3).
// No staging registers, no s_waitcnt + ds_write for the activations in the MFMA stream (the VGPR -> LDS stores were the largest
// removable term of the register-staged loop: profiles/round4_w2p_ablation.md); 70 KB of LDS: two workgroups per CU, which is what
// the 128 accumulator registers allow anyway.  Flat pixel order of the DMA pieces: (image, tile row, x) - 64 consecutive 2x2 tiles are
// 128 consecutive columns of one tile row (or wrap into the next), exactly the 1-D kernel's scheme with H / 2 rows.
constexpr int W2D_BUF_FLOATS = 4 * WBKC * LDU + 2 * V_RAW_FLOATS;
constexpr int W2D_LDS_FLOATS = 2 * W2D_BUF_FLOATS;
// HALFM (round 5): at most 32 output channels (upconv(1, *) of the depth decoder) - the tile's rows 32 .. 63 do not exist, so the wave pair that
// would own them (wm = 1) takes the second half of every chunk's k-steps of rows 0 .. 31, and the two partial results (the folded accumulator
// pairs) meet in LDS once, in front of the epilogue, in a fixed order.
template <bool STATS, bool HALFM = false>
__global__ void __launch_bounds__(WNT) __attribute__((amdgpu_waves_per_eu(2, 2))) k_conv_wino2p_dma(WinoArgs g) {
    static_assert(!(STATS && HALFM), "no statistics epilogue for the 32-channel variant");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1, HT = g.H >> 1;
    const int plane2 = HT * W2;
    const int Np = g.Nb * plane2;
    const unsigned hw = (unsigned)(g.H * g.W);
    int bx = blockIdx.x;
    const int by = blockIdx.y;
    if (g.xcd_swizzle) { const int per = gridDim.x >> 3; bx = (bx & 7) * per + (bx >> 3); }
    // g.img_tiles > 0: image-aligned tiling - workgroup bx is tile bx % img_tiles of image bx / img_tiles, so that no tile straddles
    // two images (the BatchNorm partial sums are per image) although the image's tile count is not a multiple of 64; tiles past the
    // image's last one (`lim`) are computed on whatever the loads return and never stored
    const int m0 = by * WBM;
    const int p0 = g.img_tiles > 0 ? (bx / g.img_tiles) * plane2 + (bx % g.img_tiles) * WBN : bx * WBN;
    const int lim = g.img_tiles > 0 ? (bx / g.img_tiles + 1) * plane2 : Np;
    const int cpt = g.C / WBKC, nchunk = 4 * cpt;
    const bool refl = g.pad_mode == 1;
    const int a4 = tid & 3, ar = tid >> 2;
    int mrow = m0 + ar;
    mrow = mrow < g.M ? mrow : g.M - 1;
    const unsigned u_comp = 4u * (unsigned)g.M * 4u * (unsigned)g.C;
    const __amdgpu_buffer_rsrc_t rsU = fd_make_rsrc(g.U);
    const __amdgpu_buffer_rsrc_t rsXd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.X), 0, (int)(4u * (unsigned)g.Nb * (unsigned)g.C * hw), 0x00020000);
    // per lane and DMA piece, fixed for the whole tile: tile row and byte offset (channel 0, image row 0) of its four pixels
    unsigned d_base[3] = {FD_OOB, FD_OOB, FD_OOB};
    int d_ty[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int L = 64 * (wave + 4 * q) + lane;
        const int row = L / 34, seg = L - row * 34;
        const int F = 2 * p0 - 4 + 4 * seg;                              // flat pixel index over (image, tile row, x)
        const bool ok = row < WBKC && F >= 0 && F < g.Nb * HT * g.W;
        const int Fc = ok ? F : 0;
        const int nrow = Fc / g.W, x = Fc - nrow * g.W;
        const int n = nrow / HT;
        d_ty[q] = nrow - n * HT;
        d_base[q] = ok ? 4u * ((unsigned)n * (unsigned)g.C * hw + (unsigned)row * hw + (unsigned)x) : FD_OOB;
    }
    unsigned d_off[2][3] = {{FD_OOB, FD_OOB, FD_OOB}, {FD_OOB, FD_OOB, FD_OOB}};
    unsigned d_soff = 0u, u_off = FD_OOB;
    float4 ru[4];
    int pc_f = 0, pc_ri = 0, pc_c0 = 0;
    const int H2m2 = 2 * g.H - 2;
    auto prep = [&]() __attribute__((always_inline)) {                  // offsets of flat chunk pc_f, then advance
        const bool live = pc_f < nchunk;
        const int ri = pc_ri;
        const int xr[2] = {ri == 0 ? 0 : (ri == 2 ? 2 : 1), ri == 3 ? 3 : (ri == 2 ? 1 : 2)};
        u_off = live ? 4u * (((unsigned)mrow * 4u + (unsigned)ri) * (unsigned)g.C + (unsigned)pc_c0 + 4u * a4) : FD_OOB;
        d_soff = 4u * (unsigned)pc_c0 * hw;                              // wave-uniform: first channel of the chunk
        if (pc_c0 == 0) {                                                // the pieces' row offsets change with the row component only
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int r = 2 * d_ty[q] - 1 + xr[s_];
                    const bool inb = (unsigned)r < (unsigned)g.H;
                    int rr_ = r < 0 ? -r : r;
                    rr_ = rr_ >= g.H ? H2m2 - rr_ : rr_;
                    const int ruse = refl ? rr_ : r;
                    d_off[s_][q] = (live & (refl | inb)) ? d_base[q] + (unsigned)(ruse * g.W * 4) : FD_OOB;   // FD_OOB base + anything stays out of range
                }
        }
        ++pc_f;
        pc_c0 += WBKC;
        const bool wrap = pc_c0 >= g.C;
        pc_c0 = wrap ? 0 : pc_c0;
        pc_ri += wrap ? 1 : 0;
    };
    const bool u_rows = !HALFM || wave < 2;                          // HALFM: weight rows 0 .. 31 = the loader threads of waves 0 and 1
    auto load_u = [&](int t) __attribute__((always_inline)) { if (u_rows) ru[t] = fd_ldg128(rsU, u_off + (unsigned)t * u_comp); };
    auto store_u = [&](int buf, int t) __attribute__((always_inline)) {
        if (!u_rows) return;
        float* q = smem + buf * W2D_BUF_FLOATS + t * WBKC * LDU + (4 * a4) * LDU + ar;
        q[0] = ru[t].x; q[LDU] = ru[t].y; q[2 * LDU] = ru[t].z; q[3 * LDU] = ru[t].w;
    };
    auto dma_v = [&](int buf, int s_, int q) __attribute__((always_inline)) {
        float* dst = smem + buf * W2D_BUF_FLOATS + 4 * WBKC * LDU + s_ * V_RAW_FLOATS + (wave + 4 * q) * 256;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsXd, (__attribute__((address_space(3))) void*)dst, 16, (int)d_off[s_][q], (int)d_soff, 0, 0);
    };

    const int wm = wave >> 1, wn = wave & 1;
    int o12, o0, o3;
    float ml, mr;
    {
        const int jp = 32 * wn + (lane & 31);
        const int pp = p0 + jp < lim ? p0 + jp : 0;
        const int rem = pp % plane2;
        const int jj = rem % W2;
        const bool le = jj == 0, re = 2 * jj + 2 >= g.W;
        o12 = 4 + 2 * jp;
        o0 = (le && refl) ? o12 : o12 - 2;       // 8-byte cell whose .y is d0 (reflection: column -1 is column 1 = d12.y)
        o3 = (re && refl) ? o12 : o12 + 2;       // 8-byte cell whose .x is d3 (reflection: column W is column W - 2 = d12.x)
        ml = (le && !refl) ? 0.f : 1.f;
        mr = (re && !refl) ? 0.f : 1.f;
    }
    f32x16 acc[4], ya[2], yb[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][r] = 0.f;
        ya[0][r] = ya[1][r] = yb[0][r] = yb[1][r] = 0.f;
    }

    constexpr int NK = WBKC / 2, LS = NK / 2;
    constexpr int NKW = HALFM ? NK / 2 : NK;                         // k-steps per wave and chunk (HALFM: wave pair wm takes k-steps NKW wm ...)
    const int kb2 = HALFM ? 2 * NKW * wm : 0;                        // first LDS operand row (= input channel of the chunk) of this wave's k-steps
    const int arow = lane >> 5, acol = lane & 31;
    {
        prep();                                                      // chunk 0
#pragma unroll
        for (int t = 0; t < 4; ++t) load_u(t);
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            dma_v(0, s_, 0); dma_v(0, s_, 1);
            if (wave == 0) dma_v(0, s_, 2);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) store_u(0, t);
        prep();                                                      // offsets of chunk 1: fetched DURING chunk 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int next_fold = cpt - 1, ri_cur = 0;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int cur = ch & 1;
            float sgn = ri_cur == 1 ? 1.f : -1.f;                    // this chunk's row combination: rowA + sgn * rowB
            asm volatile("" : "+v"(sgn));                            // in a VGPR: an SGPR operand halves the VALU rate on gfx950
            const float* pa = smem + cur * W2D_BUF_FLOATS + (arow + kb2) * LDU + (HALFM ? 0 : 32 * wm) + acol;
            const float* pr = smem + cur * W2D_BUF_FLOATS + 4 * WBKC * LDU + (arow + kb2) * LDR;
            typedef const __attribute__((address_space(3))) float* lds_cf;       // (stays an LDS pointer through the asm: a generic one
            typedef const __attribute__((address_space(3))) f32x2* lds_cf2;      //  turns the reads into flat loads)
            lds_cf pe = (lds_cf)(pr + V_RAW_FLOATS);                     // row set B through its own address register: with one base hipcc
            asm volatile("" : "+v"(pe));                                 // pairs the reads into ds_read2st64_b64 (8 LDS cycles instead of 2 x 2)
            float av[2][4], bv[2][4];
            auto read_a = [&](int nb, int k2, int t) __attribute__((always_inline)) { av[nb][t] = pa[t * WBKC * LDU + k2 * LDU]; };
            f32x2 d12, e12, dl, dr, el, er;                              // 8-byte reads only (d0 / d3 as 4-byte reads at stride 8: 2-way bank conflicts)
            auto read_b = [&](int k2) __attribute__((always_inline)) {
                d12 = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o12);
                e12 = *(lds_cf2)(pe + k2 * LDR + o12);
                dl = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o0); dr = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o3);
                el = *(lds_cf2)(pe + k2 * LDR + o0); er = *(lds_cf2)(pe + k2 * LDR + o3);
            };
            auto xform_b = [&](int nb) __attribute__((always_inline)) {
                asm volatile("" : "+v"(dl), "+v"(dr), "+v"(el), "+v"(er));   // both halves live: keeps the reads 8 bytes wide
                const float c0 = fmaf(sgn, el.y, dl.y), c1 = fmaf(sgn, e12.x, d12.x), c2 = fmaf(sgn, e12.y, d12.y), c3 = fmaf(sgn, er.x, dr.x);
                bv[nb][0] = fmaf(c0, ml, -c2); bv[nb][1] = c1 + c2; bv[nb][2] = c2 - c1; bv[nb][3] = fmaf(-c3, mr, c1);
            };
#pragma unroll
            for (int t = 0; t < 4; ++t) read_a(0, 0, t);
            read_b(0); xform_b(0);
#pragma unroll
            for (int kk = 0; kk < NKW; ++kk) {
                const int cb = kk & 1, nb = cb ^ 1;
                __builtin_amdgcn_sched_barrier(0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0], bv[cb][0], acc[0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NKW) { read_b(2 * (kk + 1)); read_a(nb, 2 * (kk + 1), 0); read_a(nb, 2 * (kk + 1), 1); }
                if (!HALFM && kk >= LS) store_u(cur ^ 1, kk - LS);
                if (HALFM && kk >= 2) { store_u(cur ^ 1, 2 * (kk - 2)); store_u(cur ^ 1, 2 * (kk - 2) + 1); }     // loaded in k-steps 0, 1
                __builtin_amdgcn_sched_barrier(0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1], bv[cb][1], acc[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NKW) { read_a(nb, 2 * (kk + 1), 2); read_a(nb, 2 * (kk + 1), 3); }
                if (!HALFM && kk < LS) load_u(kk);
                if (HALFM && kk < 2) { load_u(2 * kk); load_u(2 * kk + 1); }
                __builtin_amdgcn_sched_barrier(0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][2], bv[cb][2], acc[2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NKW) xform_b(nb);
                __builtin_amdgcn_sched_barrier(0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][3], bv[cb][3], acc[3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (!HALFM) {
                    if (kk < 4) dma_v(cur ^ 1, kk >> 1, kk & 1);         // row set A: pieces 0, 1; row set B: pieces 0, 1
                    if (kk == 4 && wave == 0) { dma_v(cur ^ 1, 0, 2); dma_v(cur ^ 1, 1, 2); }
                    if (kk == NK - 2) prep();                            // chunk ch + 2; every fetch of chunk ch + 1 has been issued by now
                } else {                                                 // the same six fetches in three k-steps, the offsets of chunk ch + 2 in the fourth
                    if (kk < 2) { dma_v(cur ^ 1, kk, 0); dma_v(cur ^ 1, kk, 1); }
                    if (kk == 2 && wave == 0) { dma_v(cur ^ 1, 0, 2); dma_v(cur ^ 1, 1, 2); }
                    if (kk == 3) prep();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ch == next_fold) {
                const float sa = ri_cur <= 2 ? 1.f : 0.f;
                const float sb = ri_cur == 0 ? 0.f : (ri_cur == 1 ? 1.f : -1.f);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float h0 = (acc[0][r] + acc[1][r]) + acc[2][r];
                    const float h1 = (acc[1][r] - acc[2][r]) - acc[3][r];
                    ya[0][r] = fmaf(sa, h0, ya[0][r]); ya[1][r] = fmaf(sa, h1, ya[1][r]);
                    yb[0][r] = fmaf(sb, h0, yb[0][r]); yb[1][r] = fmaf(sb, h1, yb[1][r]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t][r] = 0.f;
                }
                next_fold += cpt;
                ++ri_cur;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this chunk's DMAs (into the other buffer) have landed
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
        }
    }
    if constexpr (HALFM) {                                           // wm = 0 keeps (its own) + (wm = 1's) partial outputs
        float* red = smem + ((wn * 64) << 6) + lane;                 // [wn][64 registers][lane]; the chunk loop ended with a barrier
        if (wm == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                red[r << 6] = ya[0][r]; red[(16 + r) << 6] = ya[1][r]; red[(32 + r) << 6] = yb[0][r]; red[(48 + r) << 6] = yb[1][r];
            }
        }
        __syncthreads();
        if (wm == 1) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ya[0][r] += red[r << 6]; ya[1][r] += red[(16 + r) << 6]; yb[0][r] += red[(32 + r) << 6]; yb[1][r] += red[(48 + r) << 6];
        }
    }
    w2p_epilogue<STATS>(g, ya, yb, p0, m0, lim, plane2, W2, hw, lane, HALFM ? 0 : wm, wn);
}

}  // namespace

// dma: k_conv_wino2p_dma (W % 4 == 0, 16-byte aligned x); stats: BatchNorm partial sums in the epilogue; halfm: at most 32 output
// channels (with dma, without stats)
int wino2p_launch(const WinoProblem& p, dim3 grid, bool dma, bool stats, bool halfm, hipStream_t st) {
    const WinoArgs g{p};
    const size_t lds = sizeof(float) * (dma ? W2D_LDS_FLOATS : W_LDS_FLOATS);
    if (dma && halfm) fd_launch_lds<k_conv_wino2p_dma<false, true>>(grid, dim3(WNT), lds, st, g);
    else if (dma && stats) fd_launch_lds<k_conv_wino2p_dma<true>>(grid, dim3(WNT), lds, st, g);
    else if (dma) fd_launch_lds<k_conv_wino2p_dma<false>>(grid, dim3(WNT), lds, st, g);
    else if (stats) fd_launch_lds<k_conv_wino2p<true>>(grid, dim3(WNT), lds, st, g);
    else fd_launch_lds<k_conv_wino2p<false>>(grid, dim3(WNT), lds, st, g);
    FD_LAUNCH_CHECK("k_conv_wino2p");
    return 0;
}
