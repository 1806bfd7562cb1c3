// 3x3 stride-1 convolutions with the Winograd F(2,3) transform along x (1-D), on the FP32 MFMA.
//
// For an output pair (x, x+1) = (2j, 2j+1) of row y and each of the three kernel rows ky, the four inputs d0..d3 at columns
// 2j-1 .. 2j+2 of row y+ky-1 become  V = (d0-d2, d1+d2, d2-d1, d1-d3); the kernel row (g0,g1,g2) becomes
// U = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2) once per optimiser step; then with  M_t = sum_{c,ky} U_t V_t  (4 independent GEMMs, M = Cout,
// N = pixel PAIRS, K = 3*Cin)  the two outputs are  M0+M1+M2  and  M1-M2-M3.  6 multiplies per output instead of 9: the matrix
// pipe - the resource that bounds the training step - does 1.5x less work for the same convolution; the transform
// arithmetic (4 adds per 4 loaded values, 4 adds per 2 outputs) rides in the loader / epilogue.  Coefficients are +-1 and 1/2, so
// the fp32 rounding error stays within a few ulps of the direct sum (tests: 1e-5 of the output scale).
//
// Kernel shape: 256 threads = 4 waves, wave t owns component t and a 64 (channels) x 64 (pairs) accumulator block = 2x2 MFMA
// 32x32x2 tiles (4 MFMAs per 4 LDS operand reads); a chunk is 16 input channels of one kernel row; LDS double-buffered
// (66 KB -> 2 workgroups per CU); the four component blocks meet in LDS for the output transform; split-K over the (ky, channel)
// chunks writes partial OUTPUTS to the usual slabs (the transform is linear), finished by k_splitk_finish.
#include "conv_wino.h"
#include <type_traits>

namespace {

// VDMA: the raw activation rows go from global memory straight into LDS (buffer_load_dwordx4 ... lds; needs W % 4 == 0 so that a
// lane's four pixels share an image row): no staging registers, no s_waitcnt + ds_write in the MFMA stream for them - the VGPR ->
// LDS stores of the activations cost 0.9 of the 6.7 us per chunk-round of the register-staged loop (scripts/wino_ksweep.py).
// STATS: the epilogue also reduces the tile to the BatchNorm partial sums (g.stat_part != nullptr).  A template flag, not a run-time
// test: with `if (g.stat_part)` around writes into the accumulator array the compiler kept BOTH versions of every remaining
// accumulator alive and emitted two v_accvgpr_read + a v_cndmask per accumulator and ROW - 700 of the 1 430 vector instructions of
// the epilogue, 15 % of the kernel's time on the layer1 shape (profiles/round3_experiments.md).
// TWOD: F(2x2, 3x3) for the deep layers, where split-K slabs are written anyway.  The GEMM-N unit becomes a 2x2 output tile (tile
// row ty = output rows 2 ty, 2 ty + 1), and blockIdx.z carries a row COMPONENT ri = z & 3 (z >> 2: split of the input channels)
// instead of a share of the (kernel row, channel) chunks: the workgroup convolves the row combination
//   (x_r0 - x_r2,  x_r1 + x_r2,  x_r2 - x_r1,  x_r1 - x_r3)[ri]      (input rows 2 ty - 1 .. 2 ty + 2, padded like the columns)
// - formed by the loader from two row loads, register-staged - with U2[.][.][ri][.] over the input channels only (a third of the
// 1-D kernel's K for four instead of one or two z), and writes the horizontally transformed products S_ri [N][M][H/2][W] to slab z.
// k_wino2d_finish applies the vertical output transform  y[2 ty] = S0 + S1 + S2,  y[2 ty + 1] = S1 - S2 - S3  (+ bias, activation,
// residual) while it sums the slabs: 16 products per 2x2 tile instead of 24, for the slab traffic of a 2-way split.
template <bool VDMA, bool STATS, bool TWOD>
__device__ __forceinline__ void conv_wino_body(const WinoArgs& g) {
    static_assert(!TWOD || (!VDMA && !STATS), "the 2-D variant is register-staged and always writes slabs");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1;
    const int HT = TWOD ? g.H >> 1 : g.H;                                // rows of GEMM-N units (pairs / 2x2 tiles) per image
    const int plane2 = HT * W2;                                          // units per image; Nb * plane2 < 2^29 (size guard)
    const int Np = g.Nb * plane2;
    const unsigned hw = (unsigned)(g.H * g.W);
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, nz = gridDim.z;
    if (TWOD && g.xcd_swizzle == 2) {
        // Workgroup id L runs on XCD L % 8.  The deep layers are weight-heavy (layer4: 16.8 MB of U2 against 6 MB of activations at
        // batch 24): with the pixel tile as the fastest grid index every XCD pulled every U2 slice through its own L2 - 154 MB of
        // fetches per launch (profiles/round3_pmc_conv_wino2d_layer4.md).  Here the pixel tiles of one (channel tile, row
        // component, split) slice get ids 8 apart: one XCD, back to back, the slice's 512 KB of U2 read from HBM once.
        const int L = blockIdx.x, xcd = L & 7, k = L >> 3;
        bx = k % g.gx;
        const int sl = (k / g.gx) * 8 + xcd;
        by = sl % g.gy; bz = sl / g.gy; nz = g.gz;
    } else if (g.xcd_swizzle) { const int per = gridDim.x >> 3; bx = (bx & 7) * per + (bx >> 3); }
    const int m0 = by * WBM;
    const int p0 = bx * WBN;
    const int cpt = g.C / WBKC, nchunk_all = TWOD ? cpt : 3 * cpt;
    const int zs = bz;
    const int ri = TWOD ? zs & 3 : 0;                                    // row component of this workgroup
    const int nsplit = TWOD ? nz >> 2 : nz;
    const int ks = TWOD ? zs >> 2 : zs;
    constexpr unsigned UR = TWOD ? 4u : 3u;                              // weight rows per output channel
    const int xr_a = ri == 0 ? 0 : (ri == 2 ? 2 : 1), xr_b = ri == 3 ? 3 : (ri == 2 ? 1 : 2);
    const float x_sgn = ri == 1 ? 1.f : -1.f;
    const int per_split = (nchunk_all + nsplit - 1) / nsplit;
    const int ch_lo = ks * per_split;
    const int ch_hi = ch_lo + per_split < nchunk_all ? ch_lo + per_split : nchunk_all;

    // ---- activation loader: this thread always fetches pair jn of the tile, channel rows kr + 4 i
    const int jn = lane;
    const int kr = wave;
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
    // the tile's two halo pixels per channel row are fetched by lane 0 (left of its pair) and lane 63 (right of its pair); a pair
    // at an image border has no such pixel (its reader substitutes the padding value), every other lane stays out of range
    const bool halo_l = jn == 0 && !left_edge, halo_r = jn == WBN - 1 && !right_edge;
    // ---- weight loader: float4 a4 (of the chunk's 16 channels) of row ar, for each component
    const int a4 = tid & 3, ar = tid >> 2;
    int mrow = m0 + ar;
    mrow = mrow < g.M ? mrow : g.M - 1;                                  // rows >= M are never stored
    const unsigned u_comp = 4u * (unsigned)g.M * UR * (unsigned)g.C;     // bytes between components
    const __amdgpu_buffer_rsrc_t rsU = fd_make_rsrc(g.U), rsX = fd_make_rsrc(g.X);

    // ---- VDMA: the raw buffer is ONE linear stream of 16 rows x 34 sixteen-byte pieces (pixels -4 .. 131 of the tile's flat pixel
    //      range, row stride 136 floats); piece L = 64 * (wave + 4 q) + lane of DMA q belongs to row L / 34, piece L % 34.
    //      Per lane and DMA, fixed for the whole tile: image row / byte offset of its four pixels inside channel 0.
    const __amdgpu_buffer_rsrc_t rsXd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.X), 0, (int)(4u * (unsigned)g.Nb * (unsigned)g.C * hw), 0x00020000);
    unsigned d_base[3] = {FD_OOB, FD_OOB, FD_OOB};
    int d_y[3] = {0, 0, 0};
    unsigned d_off[3] = {FD_OOB, FD_OOB, FD_OOB};
    if (VDMA) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int L = 64 * (wave + 4 * q) + lane;
            const int row = L / 34, seg = L - row * 34;
            const int F = 2 * p0 - 4 + 4 * seg;                              // flat pixel index over (image, y, x)
            const bool ok = row < WBKC && F >= 0 && F < g.Nb * (int)hw;
            const int Fc = ok ? F : 0;
            const int n = Fc / (int)hw, rem = Fc - n * (int)hw;
            d_y[q] = rem / g.W;
            d_base[q] = ok ? 4u * ((unsigned)n * (unsigned)g.C * hw + (unsigned)row * hw + (unsigned)rem) : FD_OOB;
        }
    }
    float4 ru[4];
    f32x2 rmid[4], rmid2[TWOD ? 4 : 1];
    float rh[4], rh2[TWOD ? 4 : 1];
    unsigned u_off = FD_OOB, mid_off = FD_OOB, h_off = FD_OOB, mid_off2 = FD_OOB, h_off2 = FD_OOB;
    unsigned d_soff = 0u;
    const unsigned c_step = 4u * 4u * hw;                                // 4 channel rows further
    int pc_ky, pc_c0;
    { pc_ky = ch_lo / cpt; pc_c0 = (ch_lo - pc_ky * cpt) * WBKC; }
    // Offsets of the next chunk to fetch, in two branch-free halves (each small enough to hide behind one MFMA, see the k-loop)
    unsigned prep_base = 0u, prep_base2 = 0u;
    bool prep_ok = false, prep_ok2 = false;
    const int H2m2 = 2 * g.H - 2;
    auto prep_a = [&](bool live) __attribute__((always_inline)) {
        u_off = live ? 4u * (((unsigned)mrow * UR + (unsigned)(TWOD ? ri : pc_ky)) * (unsigned)g.C + (unsigned)pc_c0 + 4u * a4) : FD_OOB;
        const int r = TWOD ? 2 * y0 - 1 + xr_a : y0 + pc_ky - 1;
        const bool inb = (unsigned)r < (unsigned)g.H;
        int rr_ = r < 0 ? -r : r;
        rr_ = rr_ >= g.H ? H2m2 - rr_ : rr_;
        const int ruse = refl ? rr_ : r;
        prep_ok = pvalid & live & (refl | inb);
        prep_base = 4u * (nbase + (unsigned)(pc_c0 + kr) * hw + (unsigned)(ruse * g.W + 2 * j0));
        if constexpr (TWOD) {
            const int r2 = 2 * y0 - 1 + xr_b;
            const bool inb2 = (unsigned)r2 < (unsigned)g.H;
            int rr2 = r2 < 0 ? -r2 : r2;
            rr2 = rr2 >= g.H ? H2m2 - rr2 : rr2;
            const int ruse2 = refl ? rr2 : r2;
            prep_ok2 = pvalid & live & (refl | inb2);
            prep_base2 = 4u * (nbase + (unsigned)(pc_c0 + kr) * hw + (unsigned)(ruse2 * g.W + 2 * j0));
        }
        if (VDMA) {
            d_soff = 4u * (unsigned)pc_c0 * hw;                          // wave-uniform: first channel of the chunk
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int yq = d_y[q] + pc_ky - 1;
                const bool in_q = (unsigned)yq < (unsigned)g.H;
                int yr = yq < 0 ? -yq : yq;
                yr = yr >= g.H ? H2m2 - yr : yr;
                const int dyq = (refl ? yr : yq) - d_y[q];
                d_off[q] = (live & (refl | in_q)) ? d_base[q] + (unsigned)(dyq * g.W * 4) : FD_OOB;   // FD_OOB base + anything stays out of range
            }
        }
    };
    auto prep_b = [&]() __attribute__((always_inline)) {
        mid_off = prep_ok ? prep_base : FD_OOB;
        h_off = (prep_ok & halo_l) ? prep_base - 4u : ((prep_ok & halo_r) ? prep_base + 8u : FD_OOB);
        if constexpr (TWOD) {
            mid_off2 = prep_ok2 ? prep_base2 : FD_OOB;
            h_off2 = (prep_ok2 & halo_l) ? prep_base2 - 4u : ((prep_ok2 & halo_r) ? prep_base2 + 8u : FD_OOB);
        }
        pc_c0 += WBKC;
        const bool wrap = pc_c0 >= g.C;
        pc_c0 = wrap ? 0 : pc_c0;
        pc_ky += wrap ? 1 : 0;
    };
    auto load_u = [&](int t) __attribute__((always_inline)) { ru[t] = fd_ldg128(rsU, u_off + (unsigned)t * u_comp); };   // FD_OOB + (< 2^31) stays out of range
    // an FD_OOB base + (offset < 2^31) is still >= 2^31: reads 0 - vertical zero padding and pairs past the end need no select
    auto load_mid = [&](int i) __attribute__((always_inline)) {
        rmid[i] = fd_ldg64(rsX, mid_off + (unsigned)i * c_step);
        if constexpr (TWOD) rmid2[i] = fd_ldg64(rsX, mid_off2 + (unsigned)i * c_step);
    };
    auto load_h = [&](int i) __attribute__((always_inline)) {
        rh[i] = fd_ldg32(rsX, h_off + (unsigned)i * c_step);
        if constexpr (TWOD) rh2[i] = fd_ldg32(rsX, h_off2 + (unsigned)i * c_step);
    };
    auto store_u = [&](int buf, int t) __attribute__((always_inline)) {
        float* q = smem + buf * W_BUF_FLOATS + t * WBKC * LDU + (4 * a4) * LDU + ar;
        q[0] = ru[t].x; q[LDU] = ru[t].y; q[2 * LDU] = ru[t].z; q[3 * LDU] = ru[t].w;
    };
    const int v_row = 4 * WBKC * LDU + kr * LDR;                         // this thread's first channel row of the raw buffer
    const int h_col = jn == 0 ? 3 : 2 * WBN + 4;                         // where a halo lane puts its pixel
    auto store_v = [&](int buf, int i) __attribute__((always_inline)) {
        float* q = smem + buf * W_BUF_FLOATS + v_row + 4 * i * LDR;
        if constexpr (TWOD) {                                            // the row combination (exact products: a +- b)
            rmid[i].x = fmaf(x_sgn, rmid2[i].x, rmid[i].x); rmid[i].y = fmaf(x_sgn, rmid2[i].y, rmid[i].y);
            rh[i] = fmaf(x_sgn, rh2[i], rh[i]);
        }
        *reinterpret_cast<f32x2*>(q + 4 + 2 * jn) = rmid[i];
        if (jn == 0 || jn == WBN - 1) q[h_col] = rh[i];
    };
    // DMA q of this wave -> the raw rows of buffer `buf` (LDS destination = wave-uniform base + 16 bytes x lane)
    auto dma_v = [&](int buf, int q) __attribute__((always_inline)) {
        float* dst = smem + buf * W_BUF_FLOATS + 4 * WBKC * LDU + (wave + 4 * q) * 256;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsXd, (__attribute__((address_space(3))) void*)dst, 16, (int)d_off[q], (int)d_soff, 0, 0);
    };

    // Wave w owns the 32 (channels) x 32 (pairs) block (w >> 1, w & 1) of the tile with ALL FOUR Winograd components: one
    // accumulator per component.  The four component products of an output therefore sit in the same lane and register, and the
    // output transform (M0 + M1 + M2, M1 - M2 - M3) is plain register arithmetic in the epilogue.  (Round 1 / 2 gave each wave ONE
    // component of the whole 64 x 64 tile - half the LDS operand reads per MFMA - and met the other components in LDS: a
    // 64 KB round trip + barrier that took ~6 us per workgroup, a fifth of a 12-chunk tile; scripts/wino_ksweep.py.)
    const int wm = wave >> 1, wn = wave & 1;
    // Columns of the raw row this lane's B operands come from: d1, d2 = the pair itself, d0 / d3 = its left / right neighbour
    // pixel - the halo cells for the tile's first / last pair - or, where the pair touches an image border, the padding value:
    // for reflection padding the mirror pixel (column -1 is column 1, column W is column W - 2), for zero padding the factor 0.
    int o12, o0, o3;
    float ml, mr;                                                        // 0.0 where zero padding replaces d0 / d3
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
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // Main loop.  One v_mfma_f32_32x32x2_f32 occupies the SIMD's matrix pipe for 64 cycles, during which the issuing wave is free
    // to issue a handful of other instructions.  Everything that is not an MFMA is therefore cut into pieces of <= 4-5
    // instructions and placed BETWEEN the four MFMAs of a k-step (sched_barrier pins the order): the operand reads of the next
    // k-step, the staging of the following chunks and their address arithmetic.  With the same instructions in one block ahead
    // of the four MFMAs (round 2) the matrix pipe idled while that block issued: scripts/ubench/mfma_ablate2.hip measures
    // 112 -> 128 TFLOP/s for this instruction mix at two workgroups per CU on random operands (124 -> 142 on constants).
    //
    // Staging pipeline, one register set, three chunks deep: in slot i (= k-step i of the first half) of chunk ch the registers
    // of slot i - loaded one whole chunk earlier - are written to the LDS buffer of chunk ch + 1 and immediately re-loaded with
    // chunk ch + 2.  Every global load thus has a full chunk (8 k-steps, >= 2 000 cycles) to return before its s_waitcnt; with
    // load and store of the same chunk four k-steps apart (round 2) the wait stalled the wave - and the MFMAs behind it - whenever
    // the fabric was slower than that (14 % of the loop time: profiles/round3_experiments.md section 1).
    constexpr int NK = WBKC / 2;       // 8 MFMA k-steps per chunk
    constexpr int LS = NK / 2;         // staging slots: k-steps 0-3
    const int arow = lane >> 5, acol = lane & 31;
    if (ch_lo < ch_hi) {
        prep_a(true); prep_b();
#pragma unroll
        for (int t = 0; t < 4; ++t) load_u(t);
        if (VDMA) {
            dma_v(0, 0); dma_v(0, 1);
            if (wave == 0) dma_v(0, 2);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { load_mid(i); load_h(i); }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) store_u(0, t);
        if (!VDMA) {
#pragma unroll
            for (int i = 0; i < 4; ++i) store_v(0, i);
        }
        prep_a(ch_lo + 1 < ch_hi); prep_b();                     // chunk ch_lo + 1
        if (!VDMA) {                                             // ... loaded now, written to LDS during chunk ch_lo
#pragma unroll
            for (int t = 0; t < 4; ++t) load_u(t);
#pragma unroll
            for (int i = 0; i < 4; ++i) { load_mid(i); load_h(i); }
            prep_a(ch_lo + 2 < ch_hi); prep_b();                 // offsets of chunk ch_lo + 2, re-loaded during chunk ch_lo
        } else {
            // VDMA: chunk ch + 1 is fetched DURING chunk ch (weights: k-steps 0-3 into registers, stored in k-steps 4-7; activations:
            // three DMAs) with the offsets prepared one chunk earlier; the DMAs must have landed before anyone reads them
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        for (int ch = ch_lo; ch < ch_hi; ++ch) {
            const int cur = (ch - ch_lo) & 1;
            // operands of component t: A = U_t[k][32 wm + acol], B = input transform of the raw row k at this lane's pair;
            // k = 2 kk + arow
            const float* pa = smem + cur * W_BUF_FLOATS + arow * LDU + 32 * wm + acol;
            const float* pr = smem + cur * W_BUF_FLOATS + 4 * WBKC * LDU + arow * LDR;
            float av[2][4], bv[2][4];
            auto read_a = [&](int nb, int k2, int t) __attribute__((always_inline)) { av[nb][t] = pa[t * WBKC * LDU + k2 * LDU]; };
            f32x2 d12, dl, dr;                                           // three 8-byte reads (conflict-free at stride 8 over a half-wave;
            auto read_b = [&](int k2) __attribute__((always_inline)) {   // the 4-byte reads of d0 / d3 at stride 8 were 2-way bank conflicts)
                d12 = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o12);
                dl = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o0); dr = *reinterpret_cast<const f32x2*>(pr + k2 * LDR + o3);
            };
            auto xform_b = [&](int nb) __attribute__((always_inline)) {   // (d0 - d2, d1 + d2, d2 - d1, d1 - d3)
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
                if (!VDMA && kk < LS) store_u(cur ^ 1, kk);
                if (VDMA && kk >= LS) store_u(cur ^ 1, kk - LS);
                __builtin_amdgcn_sched_barrier(0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1], bv[cb][1], acc[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 1 < NK) { read_a(nb, 2 * (kk + 1), 2); read_a(nb, 2 * (kk + 1), 3); }
                if (kk < LS) load_u(kk);
                __builtin_amdgcn_sched_barrier(0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][2], bv[cb][2], acc[2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (!VDMA && kk < LS) store_v(cur ^ 1, kk);
                if (kk + 1 < NK) xform_b(nb);
                __builtin_amdgcn_sched_barrier(0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][3], bv[cb][3], acc[3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (VDMA) {
                    if (kk < 2) dma_v(cur ^ 1, kk);
                    if (kk == 2 && wave == 0) dma_v(cur ^ 1, 2);
                    if (kk == NK - 2) prep_a(ch + 2 < ch_hi);    // every fetch of chunk ch + 1 has been issued by now
                } else {
                    if (kk < LS) { load_mid(kk); load_h(kk); }
                    if (kk == NK - 2) prep_a(ch + 3 < ch_hi);    // every load of chunk ch + 2 has been issued by now
                }
                if (kk == NK - 1) prep_b();
            }
            __builtin_amdgcn_sched_barrier(0);
            if (VDMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this chunk's DMAs (into the other buffer) have landed
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
        }
    }

    // ---- epilogue: output transform in registers.  C/D layout of the 32x32 MFMA: column (pair) = lane & 31,
    //      row (channel) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int po = p0 + 32 * wn + acol;                                   // this lane's output pair
    const bool final_pass = !TWOD && nsplit == 1;
    const unsigned hwo = TWOD ? (unsigned)(HT * g.W) : hw;                // plane of the tensor written: S_ri has H / 2 rows
    unsigned out_base = FD_OOB;
    if (po < Np) {
        const int n = po / plane2;
        const int rem = po - n * plane2;
        const int yy = rem / W2, jj = rem - yy * W2;
        out_base = 4u * ((unsigned)n * (unsigned)g.M * hwo + (unsigned)(yy * g.W + 2 * jj));
    }
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(final_pass ? g.Y : g.slabs + (size_t)zs * g.slab_stride);
    const __amdgpu_buffer_rsrc_t rsAdd = fd_make_rsrc(g.add ? g.add : g.Y);
    const bool has_add = final_pass && g.add;
    const int mbase = m0 + 32 * wm + 4 * arow;
    // the 16 bias values of this lane's rows: one batch of loads in front of the row loop (a load + wait per row serialised 16
    // memory latencies in the epilogue of every biased - i.e. every decoder - convolution)
    float bias_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias_r[r] = 0.f;
    if (final_pass && g.bias) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mbase + (r & 3) + 8 * (r >> 2);
            bias_r[r] = g.bias[m < g.M ? m : g.M - 1];
        }
    }
    float s1[16], s2[16];                       // STATS: (sum, M2) of each row's two pixels
    auto rows = [&](auto act_tag) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_tag)::value;            // 0: none (compile-time), -1: g.act at run time
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mbase + (r & 3) + 8 * (r >> 2);
            const unsigned off = (m < g.M) ? out_base + 4u * (unsigned)m * hwo : FD_OOB;      // out of range: the store is dropped
            f32x2 o;
            o.x = (acc[0][r] + acc[1][r]) + acc[2][r];
            o.y = (acc[1][r] - acc[2][r]) - acc[3][r];
            if (final_pass) {
                o.x += bias_r[r]; o.y += bias_r[r];
                if (ACT != 0) { o.x = wino_act(o.x, g.act); o.y = wino_act(o.y, g.act); }
                if (has_add) {
                    const f32x2 a2 = fd_ldg64(rsAdd, off);
                    o.x += a2.x; o.y += a2.y;
                }
            }
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsY, (int)off, 0, 0);
            if (STATS) { const float dd = o.x - o.y; s1[r] = o.x + o.y; s2[r] = 0.5f * dd * dd; }
        }
    };
    if (g.act == 0 || !final_pass) rows(std::integral_constant<int, 0>{});
    else rows(std::integral_constant<int, -1>{});
    // ---- BatchNorm statistics of the tile (fd_conv2d_fwd_stats): (sum, M2 = sum of squared deviations from the partial's OWN
    //      mean) over the 32 pairs of each half-wave for its 16 channel rows, by a transposing butterfly - after the steps 16, 8, 4,
    //      2 a lane holds ONE row's partial, the step 1 completes it: 16 cross-lane moves per statistic instead of 80, fixed order
    //      (deterministic).  Two halves of n elements each merge as M2 = M2a + M2b + (sa - sb)^2 / 2n (pairwise update of Chan
    //      et al.): no E[x^2] - E[x]^2 anywhere, so a channel whose mean is many standard deviations from zero loses nothing.
    if (STATS && final_pass) {
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const int width = 8 >> step;                                   // rows kept by a lane after this step
            const int xm = 16 >> step;                                     // lane distance of the exchange
            const bool hi = (lane & xm) != 0;
            const float inv2n = 0.25f / (float)(1 << step);                // each side holds n = 2 << step pixels
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
            s2[0] = fmaf(df * df, 1.0f / 64.0f, s2[0] + o2);                // n = 32 per side
            s1[0] += o1;
        }
        // row held by this lane: bits (lane >> 4, lane >> 3, lane >> 2, lane >> 1) -> reg index, then the C/D layout above
        const int rr = ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
        const int m = mbase + (rr & 3) + 8 * (rr >> 2);
        if (!(lane & 1) && m < g.M) {
            const int n = p0 / plane2, tile = (p0 - n * plane2) / WBN;     // the whole tile lies in image n (launcher's guarantee)
            f32x2 v; v.x = s1[0]; v.y = s2[0];
            *reinterpret_cast<f32x2*>(g.stat_part + (((size_t)n * g.M + m) * g.stat_slots + 2 * tile + wn) * 2) = v;
        }
    }
}

template <bool VDMA, bool STATS>
__global__ void __launch_bounds__(WNT) __attribute__((amdgpu_waves_per_eu(3, 3))) k_conv_wino(WinoArgs g) { conv_wino_body<VDMA, STATS, false>(g); }
__global__ void __launch_bounds__(WNT) __attribute__((amdgpu_waves_per_eu(3, 3))) k_conv_wino2d(WinoArgs g) { conv_wino_body<false, false, true>(g); }

}  // namespace

int wino_x_launch(const WinoProblem& p, dim3 grid, bool twod, bool vdma, bool stats, hipStream_t st) {
    const WinoArgs g{p};
    const size_t lds = sizeof(float) * W_LDS_FLOATS;
    if (twod) fd_launch_lds<k_conv_wino2d>(grid, dim3(WNT), lds, st, g);
    else if (vdma && stats) fd_launch_lds<k_conv_wino<true, true>>(grid, dim3(WNT), lds, st, g);
    else if (vdma) fd_launch_lds<k_conv_wino<true, false>>(grid, dim3(WNT), lds, st, g);
    else if (stats) fd_launch_lds<k_conv_wino<false, true>>(grid, dim3(WNT), lds, st, g);
    else fd_launch_lds<k_conv_wino<false, false>>(grid, dim3(WNT), lds, st, g);
    FD_LAUNCH_CHECK(twod ? "k_conv_wino2d" : "k_conv_wino");
    return 0;
}
