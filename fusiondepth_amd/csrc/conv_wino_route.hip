// The host side of the Winograd convolutions (3x3, stride 1): which shapes they take and with which kernel family
// (wino_fwd_ok / wino_fwd_mode), what that costs in weight-layout and workspace floats, the weight transforms, and wino_conv_launch,
// which fills the problem, picks the family once and calls that family's launch function (conv_wino.h).
#include "conv_wino.h"
#include "conv_fast.h"
#include <stdlib.h>

namespace {

// U[t][m][ky][c] from W[m][c][ky][kx] (forward) or, for the data gradient (flip = 1: a conv over dY with the spatially flipped,
// channel-transposed kernel), from W[c][m][2-ky][2-kx].
__global__ void k_wino_weight(const float* __restrict__ w, float* __restrict__ U, int M, int C, int flip) {
    const long n = (long)M * 3 * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int ky = (int)((i / C) % 3);
        const int m = (int)(i / (3L * C));
        float g0, g1, g2;
        if (!flip) {
            const float* p = w + (((long)m * C + c) * 3 + ky) * 3;
            g0 = p[0]; g1 = p[1]; g2 = p[2];
        } else {
            const float* p = w + (((long)c * M + m) * 3 + (2 - ky)) * 3;
            g0 = p[2]; g1 = p[1]; g2 = p[0];
        }
        U[i] = g0;
        U[n + i] = 0.5f * (g0 + g1 + g2);
        U[2 * n + i] = 0.5f * (g0 - g1 + g2);
        U[3 * n + i] = g2;
    }
}

// TWOD (k_conv_wino<.., true>): U2[t][m][ri][c], the vertical transform (g_0, (g_0+g_1+g_2)/2, (g_0-g_1+g_2)/2, g_2)[ri] of the three
// kernel rows applied first, then the horizontal one: the 16 components of F(2x2, 3x3), four per row component.
__global__ void k_wino_weight2d(const float* __restrict__ w, float* __restrict__ U, int M, int C, int flip) {
    const long n = (long)M * 4 * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int ri = (int)((i / C) % 4);
        const int m = (int)(i / (4L * C));
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
        U[i] = v[0];
        U[n + i] = 0.5f * (v[0] + v[1] + v[2]);
        U[2 * n + i] = 0.5f * (v[0] - v[1] + v[2]);
        U[3 * n + i] = v[2];
    }
}
inline int wino_splits(const fd_conv_desc* d, int M, int C) {
    const long tiles = (long)fd_cdiv((long)d->N * d->H * (d->W / 2), WBN) * fd_cdiv(M, WBM);
    const int nchunk = 3 * (C / WBKC);
    int sp = 1;
    const long target = fd_tun().wino_target;              // alone on the GPU 768 is best; inside the step 256-384 (less slab traffic)
    if (tiles < target) {
        sp = (int)(target / tiles);
        const int cap = nchunk / 3 > 0 ? (nchunk / 3 < 16 ? nchunk / 3 : 16) : 1;
        if (sp > cap) sp = cap;
        if (sp < 1) sp = 1;
    }
    return sp;
}

}  // namespace

bool wino_fwd_ok(const fd_conv_desc* d) {
    return d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->Cin % 16 == 0 && d->W % 2 == 0 && !d->in_norm &&
           (long)d->Cout * 3 * d->Cin * 4 * 4 < 2147483648L;
}
// F(2x2, 3x3) (k_conv_wino2d) for the layers whose matrix work dwarfs their output: Cin * Cout >= 256 * 256 (FD_WINO_FWD_2D_MIN) and
// whole 2x2 tiles.  A function of the descriptor and of fd_tuning, so that the weight-layout size, the workspace size, the
// re-layout job and the launch agree.
// -> 0: F(2, 3) along x (k_conv_wino), 1: F(2x2, 3x3) with the row components as slabs (k_conv_wino2d + k_wino2d_finish),
//    2: F(2x2, 3x3) with all 16 components in one workgroup (k_conv_wino2p): the layers with enough 2x2 tiles to fill the chip
//    without splitting anything - ResNet layer1 / layer2 at the step's batch sizes, the decoder's wide full-resolution blocks
int wino_fwd_mode(const fd_conv_desc* d) {
    if (!wino_fwd_ok(d) || d->H % 2 != 0 || (long)d->Cout * 4 * d->Cin * 4 * 4 >= 2147483648L) return 0;
    const fd_tuning& t = fd_tun();
    const long wgs = (long)fd_cdiv((long)d->N * (d->H / 2) * (d->W / 2), WBN) * fd_cdiv(d->Cout, WBM);
    // (reflect padding = a ConvBlock of the depth decoder: these run ALONE on the main stream - decoder -> loss -> decoder is the step's
    // serial section - where the stand-alone time decides, and there the slab kernel wins from 128 x 64 channels on:
    // upconv(3,1) 77 against 113 us, upconv(2,1) 85 against 98 us, scripts/decoder_conv_time.py; the trunk's zero-padded layers run
    // beside three other streams, where fewer matrix cycles per launch decide: k_conv_wino2p, -0.7 ms per step)
    const long cc_min = d->pad_mode == 1 ? (t.wino_fwd_2d_min < 8192 ? t.wino_fwd_2d_min : 8192) : t.wino_fwd_2d_min;
    const bool deep = t.wino_fwd_2d_min > 0 && (long)d->Cin * d->Cout >= cc_min;
    if (t.wino_fwd_2dp_min_wgs > 0 && wgs >= (long)t.wino_fwd_2dp_min_wgs && (!deep || t.wino_fwd_2dp_deep)) return 2;
    return deep ? 1 : 0;
}
bool wino_fwd_2d(const fd_conv_desc* d) { return wino_fwd_mode(d) != 0; }      // the weights are U2[t][m][ri][c] for both 2-D kernels
// the F(2x2, 3x3) slab kernel with a split-precision matrix loop (k_conv_wino2d_limb): its weights are the limb image of U2
bool wino_fwd_limb(const fd_conv_desc* d) {
    return fd_tun().wino_fwd_limb != 0 && wino_fwd_mode(d) == 1 && d->Cout >= 64 && d->W % 4 == 0 && d->Cin % 16 == 0 && d->Cin >= 64;
}
// channel splits of the 2-D kernel on top of its four row components
// channel splits of the 2-D slab kernels on top of their four row components, for workgroup tiles of `bm` output channels
inline int wino2d_ksplits_bm(const fd_conv_desc* d, int bm) {
    const long tiles = 4L * fd_cdiv((long)d->N * (d->H / 2) * (d->W / 2), WBN) * fd_cdiv(d->Cout, bm);
    const long target = fd_tun().wino_target;
    long ks = tiles < target ? target / tiles : 1;
    const long cap = d->Cin / WBKC / 4 > 0 ? d->Cin / WBKC / 4 : 1;          // at least 4 chunks per split
    if (ks > cap) ks = cap;
    if (ks > 4) ks = 4;
    return ks < 1 ? 1 : (int)ks;
}
// k_conv_wino2d_m128 (128 output channels per workgroup, two workgroups per CU) instead of k_conv_wino2d (64, three per CU): its
// loop carries 40 % fewer vector instructions per matrix instruction, but it halves the workgroup count.  Stand-alone it wins exactly
// where its launch fills the chip's workgroup slots better (scripts/conv2d_m128_time.py: layer3 / layer4 at batch 12 and layer4 at
// batch 24 -4 ... -10 %; layer3 at batch 24, 720 -> 360 workgroups, +14 %) - fd_tuning.wino_fwd_2d_m128 = 2 chooses by that rule.
// INSIDE the training step the other streams fill a launch's empty slots, and the kernel with the leaner loop is the better one
// everywhere it can run (19.07 / 19.07 / 19.17 / 19.14 ms against 19.15 - 19.34 for the rule or the 64-channel kernel): the default (1).
// The launcher additionally needs a 16-byte aligned x.
inline bool wino2d_m128(const fd_conv_desc* d) {
    if (fd_tun().wino_fwd_2d_m128 == 0 || d->Cout % M2_BM != 0 || d->W % 4 != 0 || d->Cin % M2_KC != 0) return false;
    if (fd_tun().wino_fwd_2d_m128 != 2) return true;
    const long px = fd_cdiv((long)d->N * (d->H / 2) * (d->W / 2), WBN);
    const long n64 = 4L * px * fd_cdiv(d->Cout, WBM) * wino2d_ksplits_bm(d, WBM), n128 = 4L * px * (d->Cout / M2_BM) * wino2d_ksplits_bm(d, M2_BM);
    const long s64 = 3 * 256, s128 = 2 * 256;                               // workgroup slots of the chip
    // fill = n / (rounds * slots), compared as cross products
    return n128 * (fd_cdiv(n64, s64) * s64) > n64 * (fd_cdiv(n128, s128) * s128);
}
inline int wino2d_ksplits(const fd_conv_desc* d) { return wino2d_ksplits_bm(d, (!wino_fwd_limb(d) && wino2d_m128(d)) ? M2_BM : WBM); }
long wino_wt_floats(const fd_conv_desc* d) {
    if (wino_fwd_limb(d)) return 24L * d->Cout * d->Cin;                  // 16 components x 3 bf16 limbs
    return 4L * d->Cout * (wino_fwd_2d(d) ? 4 : 3) * d->Cin;
}
long wino_ws_floats(const fd_conv_desc* d) {
    const int mode = wino_fwd_mode(d);
    if (mode == 2) return 0;
    if (mode == 1) return 4L * wino2d_ksplits(d) * d->N * d->Cout * (d->H / 2) * d->W;
    const int sp = wino_splits(d, d->Cout, d->Cin);
    return sp > 1 ? (long)sp * d->N * d->Cout * d->H * d->W : 0;
}
// U for the convolution `d` computes (for a data gradient: Cin / Cout already swapped, flip = 1; w is always [Cout][Cin][3][3] of the layer)
int wino_weight_launch(const fd_conv_desc* d, const float* w, float* U, int flip, hipStream_t st) {
    const int M = d->Cout, C = d->Cin;
    const bool twod = wino_fwd_2d(d);
    if (wino_fwd_limb(d)) return wino_limb_weight_launch(w, U, M, C, flip, st);
    const long n = (long)M * (twod ? 4 : 3) * C;
    const dim3 grid(fd_cdiv(n, 256) > 4096 ? 4096 : fd_cdiv(n, 256));
    if (twod) hipLaunchKernelGGL(k_wino_weight2d, grid, dim3(256), 0, st, w, U, M, C, flip);
    else hipLaunchKernelGGL(k_wino_weight, grid, dim3(256), 0, st, w, U, M, C, flip);
    FD_LAUNCH_CHECK("wino weight transform");
    return 0;
}
// y = act(conv3x3(x; U) + bias); d describes the convolution being computed (for a data gradient: Cin / Cout already swapped).
// slots of BatchNorm partial sums per (image, channel) the kernel can emit for `d`, 0 if not (split-K, tiles across images)
int wino_stat_slots(const fd_conv_desc* d) {
    if (!wino_fwd_ok(d) || d->act != 0) return 0;
    const int mode = wino_fwd_mode(d);
    if (mode == 1) return 0;
    if (mode == 2) {                                                       // slots of 32 tiles x 4 pixels
        const long tiles = (long)(d->H / 2) * (d->W / 2);
        if (tiles % WBN == 0) return (int)(2 * tiles / WBN);
        // half a tile left over per image (ResNet layer2 at 640x192: 480 tiles): the direct-to-LDS kernel tiles image by image
        return (tiles % 32 == 0 && d->W % 4 == 0 && fd_tun().wino_fwd_2dp_dma != 0) ? (int)(tiles / 32) : 0;
    }
    const long plane2 = (long)d->H * (d->W / 2);
    if (plane2 % WBN != 0 || wino_splits(d, d->Cout, d->Cin) != 1) return 0;
    return (int)(2 * plane2 / WBN);
}

bool wino_fwd_slab_route(const fd_conv_desc* d) { return wino_fwd_ok(d) && wino_fwd_mode(d) == 1; }

int wino_conv_launch(const fd_conv_desc* d, const float* x, const float* U, const float* bias, float* y, float* ws, hipStream_t st,
                     const float* add, float* stat_part, const BnAfterConv* bn) {
    const int mode = wino_fwd_mode(d);                                     // the one decision; the family launch functions take it as flags
    if (bn && (mode != 1 || bias || add || d->act != 0)) { fd_set_error("wino conv: the fused BatchNorm needs the slab route without bias / activation"); return -1; }
    WinoProblem g = {};
    g.U = U; g.X = x; g.Y = y; g.bias = bias; g.slabs = ws; g.add = add;
    g.stat_part = stat_part; g.stat_slots = stat_part ? wino_stat_slots(d) : 0;
    if (stat_part && g.stat_slots == 0) { fd_set_error("wino conv: no statistics epilogue for this shape"); return -1; }
    g.M = d->Cout; g.C = d->Cin; g.Nb = d->N; g.H = d->H; g.W = d->W;
    g.pad_mode = d->pad_mode; g.act = d->act;
    const long out_total = (long)d->N * d->Cout * d->H * d->W;
    g.slab_stride = out_total;
    const bool twod = mode == 1;
    const int sp = twod ? 4 * wino2d_ksplits(d) : (mode == 2 ? 1 : wino_splits(d, d->Cout, d->Cin));
    if (sp > 1 && !ws) { fd_set_error("wino conv: split-K workspace missing"); return -1; }
    const bool stats = stat_part != nullptr;
    if (mode == 2) {
        const long img_tiles = (long)(d->H / 2) * (d->W / 2);
        const bool aligned = stats && img_tiles % WBN != 0;                 // statistics on a plane of 64 k + 32 tiles: tile image by image
        const int gx2 = aligned ? d->N * fd_cdiv(img_tiles, WBN) : fd_cdiv((long)d->N * img_tiles, WBN), gy2 = fd_cdiv(d->Cout, WBM);
        g.img_tiles = aligned ? fd_cdiv(img_tiles, WBN) : 0;
        g.xcd_swizzle = (gx2 % 8 == 0 && gx2 >= 16) ? 1 : 0;
        // direct-to-LDS activations need 16-byte pieces that stay inside one image row and a 16-byte aligned tensor
        const bool vdma = fd_tun().wino_fwd_2dp_dma != 0 && d->W % 4 == 0 && ((uintptr_t)x & 15) == 0;
        if (aligned && !vdma) { fd_set_error("wino conv: the statistics epilogue of this shape needs a 16-byte aligned input"); return -1; }
        const bool halfm = vdma && !stats && d->Cout <= 32 && fd_tun().wino_fwd_halfm != 0;   // the decoder's 32-channel blocks: both wave pairs on rows 0 .. 31
        return wino2p_launch(g, dim3(gx2, gy2), vdma, stats, halfm, st);
    }
    if (twod) {
        if (stats) { fd_set_error("wino conv: no statistics epilogue for this shape"); return -1; }
        const int gx2 = fd_cdiv((long)d->N * (d->H / 2) * (d->W / 2), WBN);
        g.slab_stride = out_total / 2;                                     // S_ri: [N][M][H/2][W]
        const bool limb2d = wino_fwd_limb(d);                              // the weights are the limb image: only k_conv_wino2d_limb reads it
        if (limb2d && ((uintptr_t)x & 15) != 0) { fd_set_error("wino conv: the split-precision slab kernel needs a 16-byte aligned input"); return -1; }
        const bool m128 = !limb2d && wino2d_m128(d) && ((uintptr_t)x & 15) == 0;      // (unaligned x: k_conv_wino2d with the same split count)
        const int gy2 = fd_cdiv(d->Cout, m128 ? M2_BM : WBM);
        const int xmap = 1;        // XCD-aware 1-D grid (plain 3-D grid: layer4 162 instead of 79 MB of HBM traffic per launch, -0.35 % in the step)
        g.xcd_swizzle = (gx2 % 8 == 0 && gx2 >= 16) ? 1 : 0;
        dim3 grid(gx2, gy2, sp);
        if (xmap && (gy2 * sp) % 8 == 0) { g.xcd_swizzle = 2; g.gx = gx2; g.gy = gy2; g.gz = sp; grid = dim3((unsigned)(gx2 * gy2 * sp)); }
        if (int rc = (limb2d || m128) ? wino_slab_launch(g, grid, limb2d, st) : wino_x_launch(g, grid, true, false, false, st)) return rc;
        if (bn)             // the slab reduction + vertical output transform inside the small-plane BatchNorm kernel that follows (round 5)
            return bn_small_slabs_launch(ws, g.slab_stride, sp / 4, y, *bn, d->N, d->Cout, d->H, d->W, st);
        return wino2d_finish_launch(g, sp / 4, st);
    }
    const int gx = fd_cdiv((long)d->N * d->H * (d->W / 2), WBN), gy = fd_cdiv(d->Cout, WBM);
    g.xcd_swizzle = (gx % 8 == 0 && gx >= 16) ? 1 : 0;
    // direct-to-LDS activations need 16-byte pieces that stay inside one image row and a 16-byte aligned tensor (otherwise the
    // register-staged loader: same results bit for bit, +0.12 ... +0.20 ms per step when forced)
    const bool vdma = d->W % 4 == 0 && ((uintptr_t)x & 15) == 0;
    if (int rc = wino_x_launch(g, dim3(gx, gy, sp), false, vdma, stats, st)) return rc;
    if (sp > 1) return fast_splitk_finish_launch(ws, y, bias, out_total, out_total, sp, (long)d->H * d->W, d->Cout, d->act, st, add);
    return 0;
}

// ---- probe entry points (scripts/wino_probe.py, tests): the Winograd path on its own
extern "C" long fd_conv3x3_wino_wt_floats(const fd_conv_desc* d) { return (d && wino_fwd_ok(d)) ? wino_wt_floats(d) : 0; }
extern "C" long fd_conv3x3_wino_ws_floats(const fd_conv_desc* d) { return (d && wino_fwd_ok(d)) ? wino_ws_floats(d) : 0; }
extern "C" int fd_conv3x3_wino_fwd(const fd_conv_desc* d, const float* x, const float* w, const float* bias, float* y, float* wt,
                                   int wt_ready, float* ws, void* stream) {
    FD_REQUIRE(d && x && w && y && wt, "fd_conv3x3_wino_fwd: NULL argument");
    FD_REQUIRE(wino_fwd_ok(d), "fd_conv3x3_wino_fwd: needs a 3x3 stride-1 pad-1 convolution with Cin %% 16 == 0 and an even width");
    hipStream_t st = (hipStream_t)stream;
    if (!wt_ready)
        if (int rc = wino_weight_launch(d, w, wt, 0, st)) return rc;
    return wino_conv_launch(d, x, wt, bias, y, ws, st);
}
