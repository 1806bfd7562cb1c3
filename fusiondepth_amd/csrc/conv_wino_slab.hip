// 3x3 stride-1 convolutions with the Winograd F(2x2, 3x3) transform whose four row components are separate workgroups that write
// slabs (the deep layers, where split-K slabs are written anyway): the 128-channel kernel, the slabs' finish - which k_conv_wino2d
// (conv_wino_x.hip: the 64-channel kernel of this route, on the 1-D kernel's body) shares - and, last and in one block, everything
// of the default-off split-precision variant (fd_tuning.wino_fwd_limb).
#include "conv_wino.h"
#include "conv_limb.h"

namespace {

// y[n][m][2 ty + (0, 1)][x] = act(bias[m] + (S0 + S1 + S2,  S1 - S2 - S3)) + add, S_ri = sum over the channel splits of slab 4 ks + ri
// (fixed order => deterministic); one thread per pair of columns of a tile row.
__global__ void __launch_bounds__(256) k_wino2d_finish(const float* __restrict__ slabs, float* __restrict__ Y, const float* __restrict__ bias,
                                                       const float* __restrict__ add, unsigned total2, long slab_stride, int ksplit,
                                                       int HT, int W, int M, int act) {
    const unsigned W2 = (unsigned)W >> 1, hw2 = (unsigned)HT * W2;       // total2 = N * M * HT * W / 2 < 2^30
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total2; i += gridDim.x * 256u) {
        f32x2 s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[r].x = 0.f; s[r].y = 0.f; }
        for (int k = 0; k < ksplit; ++k) {
            f32x2 a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const f32x2*>(slabs + (size_t)(4 * k + r) * slab_stride + 2 * (size_t)i);
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[r].x += a[r].x; s[r].y += a[r].y; }
        }
        const unsigned plane = i / hw2, rem = i - plane * hw2;
        const unsigned ty = rem / W2, j = rem - ty * W2;
        const float b = bias ? bias[plane % (unsigned)M] : 0.f;
        f32x2 o0, o1;
        o0.x = (s[0].x + s[1].x) + s[2].x + b; o0.y = (s[0].y + s[1].y) + s[2].y + b;
        o1.x = (s[1].x - s[2].x) - s[3].x + b; o1.y = (s[1].y - s[2].y) - s[3].y + b;
        if (act != 0) { o0.x = wino_act(o0.x, act); o0.y = wino_act(o0.y, act); o1.x = wino_act(o1.x, act); o1.y = wino_act(o1.y, act); }
        const size_t o = ((size_t)plane * (2u * HT) + 2u * ty) * (unsigned)W + 2u * j;
        if (add) {
            const f32x2 a0 = *reinterpret_cast<const f32x2*>(add + o), a1 = *reinterpret_cast<const f32x2*>(add + o + W);
            o0.x += a0.x; o0.y += a0.y; o1.x += a1.x; o1.y += a1.y;
        }
        *reinterpret_cast<f32x2*>(Y + o) = o0;
        *reinterpret_cast<f32x2*>(Y + o + W) = o1;
    }
}

// ------------------------------------------------------------------------------------------------ F(2x2, 3x3) slabs, 128 x 64 tile
// k_conv_wino2d_m128 (round 4): k_conv_wino2d for layers with Cout % 128 == 0 (ResNet layer2 .. layer4) with TWICE the output
// channels per workgroup and wave: a wave owns 64 (channels) x 32 (2x2 tiles) = two 32 x 32 blocks per Winograd component that
// share every B operand.  The B side is the expensive one (per k-step 6 LDS reads, the row combination and the horizontal input
// transform: 8 vector instructions) and is now paid once per EIGHT matrix instructions instead of four; the activations of a pixel
// tile are fetched from L2 / HBM by half as many workgroups.  Activations go global -> LDS raw (both input rows of the row
// combination, k_conv_wino2p_dma's scheme with the row component fixed per workgroup, so the DMA offsets are computed once), weights
// register-staged.  128 accumulator registers -> two waves per SIMD; chunks of 8 input channels keep two workgroups per CU in LDS
// (2 x 26.1 KB each) at the same 32 matrix instructions per wave and barrier as the other Winograd kernels.  Same slabs, same
// k_wino2d_finish.
constexpr int M2_LDU = M2_BM + 1;
constexpr int M2_VRAW = 5 * 256;                                 // one raw row set: 8 rows x 34 sixteen-byte pieces in 5 wave-wide DMAs
constexpr int M2_BUF_FLOATS = 4 * M2_KC * M2_LDU + 2 * M2_VRAW;
constexpr int M2_LDS_FLOATS = 2 * M2_BUF_FLOATS;
__global__ void __launch_bounds__(WNT) __attribute__((amdgpu_waves_per_eu(2, 2))) k_conv_wino2d_m128(WinoArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1, HT = g.H >> 1;
    const int plane2 = HT * W2;
    const int Np = g.Nb * plane2;
    const unsigned hw = (unsigned)(g.H * g.W);
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, nz = gridDim.z;
    if (g.xcd_swizzle == 2) {                                    // all pixel tiles of a (channel tile, row component, split) slice on one XCD
        const int L = blockIdx.x, xcd = L & 7, k = L >> 3;
        bx = k % g.gx;
        const int sl = (k / g.gx) * 8 + xcd;
        by = sl % g.gy; bz = sl / g.gy; nz = g.gz;
    } else if (g.xcd_swizzle) { const int per = gridDim.x >> 3; bx = (bx & 7) * per + (bx >> 3); }
    const int m0 = by * M2_BM;
    const int p0 = bx * WBN;
    const int ri = bz & 3, ks = bz >> 2, nsplit = nz >> 2;
    const int cpt = g.C / M2_KC;
    const int per_split = (cpt + nsplit - 1) / nsplit;
    const int ch_lo = ks * per_split;
    const int ch_hi = ch_lo + per_split < cpt ? ch_lo + per_split : cpt;
    const int nchunk = ch_hi > ch_lo ? ch_hi - ch_lo : 0;
    const bool refl = g.pad_mode == 1;
    // ---- weight loader: float4 a4 (of the chunk's 8 channels) of row ar, for each horizontal component
    const int a4 = tid & 1, ar = tid >> 1;
    int mrow = m0 + ar;
    mrow = mrow < g.M ? mrow : g.M - 1;
    const unsigned u_comp = 4u * (unsigned)g.M * 4u * (unsigned)g.C;
    const unsigned u_base = 4u * (((unsigned)mrow * 4u + (unsigned)ri) * (unsigned)g.C + (unsigned)(ch_lo * M2_KC) + 4u * a4);
    const __amdgpu_buffer_rsrc_t rsU = fd_make_rsrc(g.U);
    const __amdgpu_buffer_rsrc_t rsXd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.X), 0, (int)(4u * (unsigned)g.Nb * (unsigned)g.C * hw), 0x00020000);
    // ---- activation DMAs: piece L = 64 (wave + 4 q) + lane of the linear raw stream (8 rows x 34 pieces: pixels -4 .. 131 of the tile's
    //      flat pixel range over (image, tile row, x)); the two input rows of row component ri are fixed for the whole workgroup
    const int xr[2] = {ri == 0 ? 0 : (ri == 2 ? 2 : 1), ri == 3 ? 3 : (ri == 2 ? 1 : 2)};
    const int H2m2 = 2 * g.H - 2;
    unsigned d_row[2][2];                                        // [row set][q]: byte offset of the piece at channel 0 of the chunk, or FD_OOB
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int L = 64 * (wave + 4 * q) + lane;
        const int row = L / 34, seg = L - row * 34;
        const int F = 2 * p0 - 4 + 4 * seg;
        const bool ok = row < M2_KC && F >= 0 && F < g.Nb * HT * g.W;
        const int Fc = ok ? F : 0;
        const int nrow = Fc / g.W, x = Fc - nrow * g.W;
        const int n = nrow / HT, ty = nrow - n * HT;
        const unsigned base = 4u * ((unsigned)n * (unsigned)g.C * hw + (unsigned)row * hw + (unsigned)x);
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            const int r = 2 * ty - 1 + xr[s_];
            const bool inb = (unsigned)r < (unsigned)g.H;
            int rr_ = r < 0 ? -r : r;
            rr_ = rr_ >= g.H ? H2m2 - rr_ : rr_;
            const int ruse = refl ? rr_ : r;
            d_row[s_][q] = (ok & (refl | inb)) ? base + (unsigned)(ruse * g.W * 4) : FD_OOB;
        }
    }
    unsigned d_off[2][2] = {{FD_OOB, FD_OOB}, {FD_OOB, FD_OOB}};
    unsigned d_soff = 0u, u_off = FD_OOB;
    int pc = 0;                                                  // chunk (relative to ch_lo) the offsets point at
    auto prep = [&]() __attribute__((always_inline)) {           // offsets of chunk pc, then advance
        const bool live = pc < nchunk;
        u_off = live ? u_base + 4u * (unsigned)(pc * M2_KC) : FD_OOB;
        d_soff = 4u * (unsigned)((ch_lo + pc) * M2_KC) * hw;     // wave-uniform: first channel of the chunk
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
            for (int q = 0; q < 2; ++q) d_off[s_][q] = live ? d_row[s_][q] : FD_OOB;
        ++pc;
    };
    float4 ru[4];
    auto load_u = [&](int t) __attribute__((always_inline)) { ru[t] = fd_ldg128(rsU, u_off + (unsigned)t * u_comp); };
    auto store_u = [&](int buf, int t) __attribute__((always_inline)) {
        float* q = smem + buf * M2_BUF_FLOATS + t * M2_KC * M2_LDU + (4 * a4) * M2_LDU + ar;
        q[0] = ru[t].x; q[M2_LDU] = ru[t].y; q[2 * M2_LDU] = ru[t].z; q[3 * M2_LDU] = ru[t].w;
    };
    auto dma_v = [&](int buf, int s_, int q) __attribute__((always_inline)) {
        float* dst = smem + buf * M2_BUF_FLOATS + 4 * M2_KC * M2_LDU + s_ * M2_VRAW + (wave + 4 * q) * 256;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsXd, (__attribute__((address_space(3))) void*)dst, 16, (int)d_off[s_][q], (int)d_soff, 0, 0);
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
    f32x16 acc[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][t][r] = 0.f;

    constexpr int NK = M2_KC / 2;                                // 4 k-steps of 8 matrix instructions per chunk
    const int arow = lane >> 5, acol = lane & 31;
    float sgn = ri == 1 ? 1.f : -1.f;                            // the row combination: rowA + sgn * rowB
    asm volatile("" : "+v"(sgn));                                // in a VGPR: an SGPR operand halves the VALU rate on gfx950
    if (nchunk > 0) {
        prep();                                                  // chunk 0
#pragma unroll
        for (int t = 0; t < 4; ++t) load_u(t);
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            dma_v(0, s_, 0);
            if (wave == 0) dma_v(0, s_, 1);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) store_u(0, t);
        prep();                                                  // offsets of chunk 1: fetched DURING chunk 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int ch = 0; ch < nchunk; ++ch) {
            const int cur = ch & 1;
            const float* pa = smem + cur * M2_BUF_FLOATS + arow * M2_LDU + 64 * wm + acol;
            const float* pr = smem + cur * M2_BUF_FLOATS + 4 * M2_KC * M2_LDU + arow * LDR;
            typedef const __attribute__((address_space(3))) float* lds_cf;       // (stays an LDS pointer through the asm: a generic one
            typedef const __attribute__((address_space(3))) f32x2* lds_cf2;      //  turns the reads into flat loads)
            lds_cf pe = (lds_cf)(pr + M2_VRAW);                      // row set B through its own address register: with one base hipcc
            asm volatile("" : "+v"(pe));                             // pairs the reads into ds_read2st64_b64 (8 LDS cycles instead of 2 x 2)
            float av[2][2][4], bv[2][4];
            auto read_a = [&](int nb, int k2, int b, int t) __attribute__((always_inline)) { av[nb][b][t] = pa[t * M2_KC * M2_LDU + k2 * M2_LDU + 32 * b]; };
            f32x2 d12, e12, dl, dr, el, er;
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
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t) read_a(0, 0, b, t);
            read_b(0); xform_b(0);
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                const int cb = kk & 1, nb = cb ^ 1;
                const bool more = kk + 1 < NK;
                __builtin_amdgcn_sched_barrier(0);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0][0], bv[cb][0], acc[0][0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (more) read_b(2 * (kk + 1));
                __builtin_amdgcn_sched_barrier(0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0][1], bv[cb][1], acc[0][1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (more) { read_a(nb, 2 * (kk + 1), 0, 0); read_a(nb, 2 * (kk + 1), 0, 1); read_a(nb, 2 * (kk + 1), 0, 2); }
                __builtin_amdgcn_sched_barrier(0);
                acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0][2], bv[cb][2], acc[0][2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (more) { read_a(nb, 2 * (kk + 1), 0, 3); read_a(nb, 2 * (kk + 1), 1, 0); read_a(nb, 2 * (kk + 1), 1, 1); }
                __builtin_amdgcn_sched_barrier(0);
                acc[0][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][0][3], bv[cb][3], acc[0][3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (more) { read_a(nb, 2 * (kk + 1), 1, 2); read_a(nb, 2 * (kk + 1), 1, 3); }
                if (kk < 2) load_u(2 * kk);
                if (kk >= 2) store_u(cur ^ 1, 2 * (kk - 2));
                __builtin_amdgcn_sched_barrier(0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1][0], bv[cb][0], acc[1][0], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < 2) load_u(2 * kk + 1);
                if (kk >= 2) store_u(cur ^ 1, 2 * (kk - 2) + 1);
                __builtin_amdgcn_sched_barrier(0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1][1], bv[cb][1], acc[1][1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (more) xform_b(nb);
                __builtin_amdgcn_sched_barrier(0);
                acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1][2], bv[cb][2], acc[1][2], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < 2) dma_v(cur ^ 1, kk, 0);                       // row set A, then row set B
                if (kk == 2 && wave == 0) { dma_v(cur ^ 1, 0, 1); dma_v(cur ^ 1, 1, 1); }
                if (kk == NK - 1) prep();                                // chunk ch + 2; every fetch of chunk ch + 1 has been issued by now
                __builtin_amdgcn_sched_barrier(0);
                acc[1][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb][1][3], bv[cb][3], acc[1][3], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this chunk's DMAs (into the other buffer) have landed
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
        }
    }

    // ---- epilogue: the horizontally transformed products S_ri [N][M][H/2][W] of this (row component, channel split) to slab bz
    const int po = p0 + 32 * wn + acol;
    const unsigned hwo = (unsigned)(HT * g.W);
    unsigned out_base = FD_OOB;
    if (po < Np) {
        const int n = po / plane2;
        const int rem = po - n * plane2;
        const int yy = rem / W2, jj = rem - yy * W2;
        out_base = 4u * ((unsigned)n * (unsigned)g.M * hwo + (unsigned)(yy * g.W + 2 * jj));
    }
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(g.slabs + (size_t)bz * g.slab_stride);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int mbase = m0 + 64 * wm + 32 * b + 4 * arow;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mbase + (r & 3) + 8 * (r >> 2);
            const unsigned off = (m < g.M) ? out_base + 4u * (unsigned)m * hwo : FD_OOB;      // out of range: the store is dropped
            f32x2 o;
            o.x = (acc[b][0][r] + acc[b][1][r]) + acc[b][2][r];
            o.y = (acc[b][1][r] - acc[b][2][r]) - acc[b][3][r];
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsY, (int)off, 0, 0);
        }
    }
}

}  // namespace

int wino2d_finish_launch(const WinoProblem& p, int ksplit, hipStream_t st) {
    const unsigned total2 = (unsigned)((long)p.Nb * p.M * p.H * p.W / 4);         // one thread per (tile row, column pair)
    const unsigned blocks = (total2 + 255u) / 256u;
    hipLaunchKernelGGL(k_wino2d_finish, dim3(blocks > 4096u ? 4096u : blocks), dim3(256), 0, st, p.slabs, p.Y, p.bias, p.add, total2,
                       p.slab_stride, ksplit, p.H / 2, p.W, p.M, p.act);
    FD_LAUNCH_CHECK("k_wino2d_finish");
    return 0;
}

// ================================================================================================ fd_tuning.wino_fwd_limb (default off)
namespace {

// The same 16 components as the split-precision image k_conv_wino2d_limb reads (conv_limb.h arithmetic): for row component ri, K-chunk
// (16 input channels), horizontal component t, limb L, K half h and output channel m one 16-byte piece of 8 bf16,
//   piece index = ((((ri * C/16 + chunk) * 4 + t) * 3 + L) * 2 + h) * M + m
// - a chunk's 24 planes of M consecutive pieces are what the kernel copies into LDS, a lane's MFMA fragment is one piece.
__host__ __device__ inline long wino_limb_piece(int ri, int chunk, int t, int L, int h, long m, long M, int cpt) {
    return ((((long)(ri * cpt + chunk) * 4 + t) * 3 + L) * 2 + h) * M + m;
}
__global__ void k_wino_weight2d_limb(const float* __restrict__ w, uint4* __restrict__ A3, int M, int C, int flip) {
    const int c8n = C >> 3, cpt = C >> 4;
    const long n = (long)M * 4 * c8n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i % M);
        const int ri = (int)((i / M) % 4);
        const int c8 = (int)(i / (4L * M));
        float u[4][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c8 * 8 + e;
            float g[3][3];
            const float* p = flip ? w + ((long)c * M + m) * 9 : w + ((long)m * C + c) * 9;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) g[a][b] = flip ? p[(2 - a) * 3 + (2 - b)] : p[a * 3 + b];
            float v[3];
#pragma unroll
            for (int b = 0; b < 3; ++b)
                v[b] = ri == 0 ? g[0][b] : (ri == 3 ? g[2][b] : (ri == 1 ? 0.5f * (g[0][b] + g[1][b] + g[2][b]) : 0.5f * (g[0][b] - g[1][b] + g[2][b])));
            u[0][e] = v[0]; u[1][e] = 0.5f * (v[0] + v[1] + v[2]); u[2][e] = 0.5f * (v[0] - v[1] + v[2]); u[3][e] = v[2];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint4 h, md, l;
            fdlimb::split8(u[t], h, md, l);
            A3[wino_limb_piece(ri, c8 >> 1, t, 0, c8 & 1, m, M, cpt)] = h;
            A3[wino_limb_piece(ri, c8 >> 1, t, 1, c8 & 1, m, M, cpt)] = md;
            A3[wino_limb_piece(ri, c8 >> 1, t, 2, c8 & 1, m, M, cpt)] = l;
        }
    }
}
// ------------------------------------------------------------------------------------------------ F(2x2, 3x3) slabs, split precision
// k_conv_wino2d_limb: the slab kernel of the deep layers (k_conv_wino2d / _m128: matrix pipes 0.7 busy - matrix-bound, unlike the
// one-workgroup kernel, whose split-precision form gained nothing: profiles/round6_wino2p_limb.log) with a bf16x3 matrix loop at fp32
// accuracy (conv_limb.h).  Same grid (pixel tile, 64-channel tile, row component x channel split; XCD-aware), same raw activation DMAs
// (row component fixed per workgroup), same slabs and finish kernels.  Different:
//   * the weights arrive PRE-SPLIT (re-layout modes 11 / 12: wino_limb_piece) - a chunk's (16 input channels) 24 planes of 64 fragments
//     are plain 16-byte copies global -> registers -> LDS;
//   * the activations are combined, transformed and split ONCE per workgroup by a transform stage between two barriers - thread = (2x2
//     tile, four channels of the chunk): 24 eight-byte raw reads, 16 fused multiply-adds + 16 transform operations, 8 split2, 12 eight-byte
//     fragment stores;
//   * the matrix phase of a chunk is 24 fragment reads + 24 v_mfma_f32_32x32x16_bf16 per wave (768 matrix-pipe cycles; the f32 kernels
//     spend 2 048 on the same 16 channels x 32 x 32 x 4 components).
// One raw buffer (consumed before the first barrier, refilled by DMA during the matrix phase), one fragment buffer per operand: 68 KB.
constexpr int W2L_HPL = 64 * 16 + 64;                 // one K half of a (component, limb) plane: 64 rows / tiles x 16 B, padded
constexpr int W2L_PLANE = 2 * W2L_HPL;
constexpr int W2L_OP = 12 * W2L_PLANE;                // one operand: 4 components x 3 limbs
constexpr int W2L_RAW_BYTES = 2 * V_RAW_FLOATS * 4;   // two raw row sets of 16 channels
constexpr int W2L_LDS_BYTES = 2 * W2L_OP + W2L_RAW_BYTES;

__global__ void __launch_bounds__(WNT) k_conv_wino2d_limb(WinoArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned char* const smA = reinterpret_cast<unsigned char*>(smem);
    unsigned char* const smB = smA + W2L_OP;
    float* const raw = reinterpret_cast<float*>(smA + 2 * W2L_OP);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W2 = g.W >> 1, HT = g.H >> 1;
    const int plane2 = HT * W2;
    const int Np = g.Nb * plane2;
    const unsigned hw = (unsigned)(g.H * g.W);
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, nz = gridDim.z;
    if (g.xcd_swizzle == 2) {                                    // all pixel tiles of a (channel tile, row component, split) slice on one XCD
        const int L = blockIdx.x, xcd = L & 7, k = L >> 3;
        bx = k % g.gx;
        const int sl = (k / g.gx) * 8 + xcd;
        by = sl % g.gy; bz = sl / g.gy; nz = g.gz;
    } else if (g.xcd_swizzle) { const int per = gridDim.x >> 3; bx = (bx & 7) * per + (bx >> 3); }
    const int m0 = by * WBM;
    const int p0 = bx * WBN;
    const int ri = bz & 3, ks = bz >> 2, nsplit = nz >> 2;
    const int cpt = g.C / WBKC;
    const int per_split = (cpt + nsplit - 1) / nsplit;
    const int ch_lo = ks * per_split;
    const int ch_hi = ch_lo + per_split < cpt ? ch_lo + per_split : cpt;
    const int nchunk = ch_hi > ch_lo ? ch_hi - ch_lo : 0;
    const bool refl = g.pad_mode == 1;
    const __amdgpu_buffer_rsrc_t rsU = fd_make_rsrc(g.U);
    const __amdgpu_buffer_rsrc_t rsXd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.X), 0, (int)(4u * (unsigned)g.Nb * (unsigned)g.C * hw), 0x00020000);
    // ---- raw activation DMAs: piece L = 64 (wave + 4 q) + lane of the linear raw stream (16 rows x 34 pieces: pixels -4 .. 131 of the tile's
    //      flat pixel range over (image, tile row, x)); the two input rows of row component ri are fixed for the whole workgroup
    const int xr[2] = {ri == 0 ? 0 : (ri == 2 ? 2 : 1), ri == 3 ? 3 : (ri == 2 ? 1 : 2)};
    const int H2m2 = 2 * g.H - 2;
    unsigned d_row[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int L = 64 * (wave + 4 * q) + lane;
        const int row = L / 34, seg = L - row * 34;
        const int F = 2 * p0 - 4 + 4 * seg;
        const bool ok = row < WBKC && F >= 0 && F < g.Nb * HT * g.W;
        const int Fc = ok ? F : 0;
        const int nrow = Fc / g.W, x = Fc - nrow * g.W;
        const int n = nrow / HT, ty = nrow - n * HT;
        const unsigned base = 4u * ((unsigned)n * (unsigned)g.C * hw + (unsigned)row * hw + (unsigned)x);
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
            const int r = 2 * ty - 1 + xr[s_];
            const bool inb = (unsigned)r < (unsigned)g.H;
            int rr_ = r < 0 ? -r : r;
            rr_ = rr_ >= g.H ? H2m2 - rr_ : rr_;
            const int ruse = refl ? rr_ : r;
            d_row[s_][q] = (ok & (refl | inb)) ? base + (unsigned)(ruse * g.W * 4) : FD_OOB;
        }
    }
    // ---- weight fragments of a chunk: 24 planes x 64 rows = 1 536 pieces, six per thread (piece tid + 256 i: plane (tid + 256 i) / 64)
    unsigned u_lane[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int q = tid + 256 * i;
        const int pl = q >> 6, row = q & 63;
        int m = m0 + row; m = m < g.M ? m : g.M - 1;
        u_lane[i] = 16u * ((unsigned)pl * (unsigned)g.M + (unsigned)m);
    }
    const unsigned u_chunk = 16u * 24u * (unsigned)g.M;               // bytes per chunk of the image
    int pc = 0;                                                       // chunk (relative to ch_lo) the next fetch takes
    uint4 ru[6];
    auto fetch = [&]() __attribute__((always_inline)) {               // weights of chunk pc -> registers, raw rows of chunk pc -> LDS; then advance
        const bool live = pc < nchunk;
        const unsigned u_soff = (unsigned)(ri * cpt + ch_lo + (live ? pc : 0)) * u_chunk;
        const unsigned d_soff = 4u * (unsigned)((ch_lo + pc) * WBKC) * hw;
#pragma unroll
        for (int i = 0; i < 6; ++i)
            ru[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsU, (int)(live ? u_lane[i] : FD_OOB), (int)u_soff, 0));
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (q == 2 && wave != 0) continue;
                float* dst = raw + s_ * V_RAW_FLOATS + (wave + 4 * q) * 256;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsXd, (__attribute__((address_space(3))) void*)dst, 16, (int)(live ? d_row[s_][q] : FD_OOB), (int)d_soff, 0, 0);
            }
        ++pc;
    };
    auto store_u = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int q = tid + 256 * i;
            const int pl = q >> 6, row = q & 63;                      // plane = (t * 3 + L) * 2 + h
            *reinterpret_cast<uint4*>(smA + (pl >> 1) * W2L_PLANE + (pl & 1) * W2L_HPL + row * 16) = ru[i];
        }
    };
    // ---- transform stage: this thread's 2x2 tile (lane) and channels 4 wave .. 4 wave + 3 of the chunk
    int t12, t0, t3;
    float tml, tmr;
    {
        const int pp = p0 + lane < Np ? p0 + lane : 0;
        const int rem = pp % plane2;
        const int jj = rem % W2;
        const bool le = jj == 0, re = 2 * jj + 2 >= g.W;
        t12 = 4 + 2 * lane;
        t0 = (le && refl) ? t12 : t12 - 2;
        t3 = (re && refl) ? t12 : t12 + 2;
        tml = (le && !refl) ? 0.f : 1.f;
        tmr = (re && !refl) ? 0.f : 1.f;
    }
    float sgn = ri == 1 ? 1.f : -1.f;                                 // the row combination: rowA + sgn * rowB
    asm volatile("" : "+v"(sgn));
    unsigned char* const bslot = smB + (wave >> 1) * W2L_HPL + lane * 16 + 8 * (wave & 1);
    auto transform = [&]() __attribute__((always_inline)) {
        float v[4][4];                                               // [component][channel]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* pr = raw + (4 * wave + i) * LDR;
            const float* pe = pr + V_RAW_FLOATS;
            const f32x2 d12 = *reinterpret_cast<const f32x2*>(pr + t12), e12 = *reinterpret_cast<const f32x2*>(pe + t12);
            const f32x2 dl = *reinterpret_cast<const f32x2*>(pr + t0), dr = *reinterpret_cast<const f32x2*>(pr + t3);
            const f32x2 el = *reinterpret_cast<const f32x2*>(pe + t0), er = *reinterpret_cast<const f32x2*>(pe + t3);
            const float c0 = fmaf(sgn, el.y, dl.y), c1 = fmaf(sgn, e12.x, d12.x), c2 = fmaf(sgn, e12.y, d12.y), c3 = fmaf(sgn, er.x, dr.x);
            v[0][i] = fmaf(c0, tml, -c2); v[1][i] = c1 + c2; v[2][i] = c2 - c1; v[3][i] = fmaf(-c3, tmr, c1);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            unsigned h0, m0_, l0, h1, m1, l1;
            fdlimb::split2(v[t][0], v[t][1], h0, m0_, l0); fdlimb::split2(v[t][2], v[t][3], h1, m1, l1);
            *reinterpret_cast<u32x2*>(bslot + (3 * t) * W2L_PLANE) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(bslot + (3 * t + 1) * W2L_PLANE) = u32x2{m0_, m1};
            *reinterpret_cast<u32x2*>(bslot + (3 * t + 2) * W2L_PLANE) = u32x2{l0, l1};
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
        fetch();                                                     // chunk 0
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const unsigned char* fa = smA + arow * W2L_HPL + (32 * wm + acol) * 16;
        const unsigned char* fb = smB + arow * W2L_HPL + (32 * wn + acol) * 16;
        for (int ch = 0; ch < nchunk; ++ch) {
            store_u();                                               // weight fragments of chunk ch (in registers since the last matrix phase)
            transform();                                             // raw rows of chunk ch -> activation fragments
            __syncthreads();                                         // fragments complete, raw buffer free
            fetch();                                                 // chunk ch + 1 (past the end: nothing is fetched)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                uint4 af[3], bf[3];
#pragma unroll
                for (int Lm = 0; Lm < 3; ++Lm) {
                    af[Lm] = *reinterpret_cast<const uint4*>(fa + (t * 3 + Lm) * W2L_PLANE);
                    bf[Lm] = *reinterpret_cast<const uint4*>(fb + (t * 3 + Lm) * W2L_PLANE);
                }
                FD_WLIMB_MFMA6(acc[t], af, bf);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the next chunk's DMAs and weight loads have landed
            __syncthreads();
        }
    }
    // ---- epilogue (k_conv_wino2d_m128's, one 32-row block per wave): S_ri [N][M][H/2][W] of this (row component, channel split) to slab bz
    const int po = p0 + 32 * wn + acol;
    const unsigned hwo = (unsigned)(HT * g.W);
    unsigned out_base = FD_OOB;
    if (po < Np) {
        const int n = po / plane2;
        const int rem = po - n * plane2;
        const int yy = rem / W2, jj = rem - yy * W2;
        out_base = 4u * ((unsigned)n * (unsigned)g.M * hwo + (unsigned)(yy * g.W + 2 * jj));
    }
    const __amdgpu_buffer_rsrc_t rsY = fd_make_rsrc(g.slabs + (size_t)bz * g.slab_stride);
    const int mbase = m0 + 32 * wm + 4 * arow;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mbase + (r & 3) + 8 * (r >> 2);
        const unsigned off = (m < g.M) ? out_base + 4u * (unsigned)m * hwo : FD_OOB;
        f32x2 o;
        o.x = (acc[0][r] + acc[1][r]) + acc[2][r];
        o.y = (acc[1][r] - acc[2][r]) - acc[3][r];
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsY, (int)off, 0, 0);
    }
}

}  // namespace

int wino_limb_weight_launch(const float* w, float* U, int M, int C, int flip, hipStream_t st) {
    const long nl = (long)M * 4 * (C >> 3);
    hipLaunchKernelGGL(k_wino_weight2d_limb, dim3(fd_cdiv(nl, 256) > 4096 ? 4096 : fd_cdiv(nl, 256)), dim3(256), 0, st, w, reinterpret_cast<uint4*>(U), M, C, flip);
    FD_LAUNCH_CHECK("wino weight transform (limbs)");
    return 0;
}
// ================================================================================================ end of fd_tuning.wino_fwd_limb

int wino_slab_launch(const WinoProblem& p, dim3 grid, bool limb, hipStream_t st) {
    const WinoArgs g{p};
    if (limb) fd_launch_lds<k_conv_wino2d_limb>(grid, dim3(WNT), (size_t)W2L_LDS_BYTES, st, g);
    else fd_launch_lds<k_conv_wino2d_m128>(grid, dim3(WNT), sizeof(float) * M2_LDS_FLOATS, st, g);
    FD_LAUNCH_CHECK("k_conv_wino2d");
    return 0;
}
