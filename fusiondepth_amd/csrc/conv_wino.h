// Internal interface of the Winograd convolution units (3x3, stride 1): what the rest of the library calls, what the units call in
// each other, and the device-side vocabulary their kernels share.
//   conv_wino_route.hip   shape predicates, weight transforms, wino_conv_launch (decides the family once), the probe entry points
//   conv_wino_x.hip       F(2, 3) along x: k_conv_wino, and k_conv_wino2d on the same body
//   conv_wino_slab.hip    F(2x2, 3x3) with the row components as slabs: k_conv_wino2d_m128, k_conv_wino2d_limb, k_wino2d_finish
//   conv_wino.hip         F(2x2, 3x3) in one workgroup: k_conv_wino2p, k_conv_wino2p_dma
//   conv_wino_wgrad.hip   the weight gradient: k_wgrad_wino, k_wgrad_wino_limb
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/fdhip.h"
#include "fd_common.h"

// ---- conv_wino_route.hip
bool wino_fwd_ok(const fd_conv_desc* d);
int wino_fwd_mode(const fd_conv_desc* d);       // 0: k_conv_wino, 1: the slab kernels, 2: k_conv_wino2p
long wino_wt_floats(const fd_conv_desc* d);
bool wino_fwd_2d(const fd_conv_desc* d);
bool wino_fwd_limb(const fd_conv_desc* d);      // k_conv_wino2d_limb: the weight layout is the limb image of U2 (re-layout modes 11 / 12)
long wino_ws_floats(const fd_conv_desc* d);
int wino_weight_launch(const fd_conv_desc* d, const float* w, float* U, int flip, hipStream_t st);
// the BatchNorm that follows a slab-route convolution, fused with the slab reduction (norm.hip: k_bn_train_small_slabs)
struct BnAfterConv {
    const float* weight; const float* bias; const float* residual; float* out;
    float* running_mean; float* running_var; float* save_mean; float* save_invstd;
    int groups; float eps, momentum; int relu;
};
bool bn_small_slabs_ok(int N, int C, int H, int W, int groups);
int bn_small_slabs_launch(const float* slabs, long slab_stride, int ksplit, float* y, const BnAfterConv& bn, int N, int C, int H, int W,
                          hipStream_t st);
bool wino_fwd_slab_route(const fd_conv_desc* d);
int wino_conv_launch(const fd_conv_desc* d, const float* x, const float* U, const float* bias, float* y, float* ws, hipStream_t st,
                     const float* add = nullptr, float* stat_part = nullptr, const BnAfterConv* bn = nullptr);
int wino_stat_slots(const fd_conv_desc* d);

// What wino_conv_launch fills for a forward kernel.  (The kernels' parameter type is WinoArgs below - the same fields, inside the
// anonymous namespace: a type of that namespace cannot appear in a function that two translation units share.)
struct WinoProblem {
    const float* U; const float* X; float* Y; const float* bias; float* slabs;
    const float* add;    // optional, laid out like Y: Y = act(conv + bias) + add
    long slab_stride;
    int M, C, Nb, H, W;
    int pad_mode, act;
    int xcd_swizzle;     // 1: consecutive pixel tiles (vertical neighbours share input rows) go to the same XCD / L2
                         // 2 (k_conv_wino2d): 1-D grid, all pixel tiles of a (channel tile, row component, split) on one XCD
    int gx, gy, gz;      // the logical grid of xcd_swizzle == 2
    // optional: per-channel statistics of the output for the BatchNorm that follows (fd_conv2d_fwd_stats): [Nb][M][stat_slots][2] =
    // (sum, sum of squares) over the 64 pixels of each (pixel tile, 32-pair half); needs tiles that do not straddle images
    float* stat_part;
    int stat_slots;
    int img_tiles;       // k_conv_wino2p_dma: > 0 = tiles per image of the image-aligned tiling (statistics on planes of 32 k tiles)
};
// ---- the launch function of each forward family: the kernel for these flags on `grid`, nothing decided again
int wino_x_launch(const WinoProblem& p, dim3 grid, bool twod, bool vdma, bool stats, hipStream_t st);      // conv_wino_x.hip
int wino2p_launch(const WinoProblem& p, dim3 grid, bool dma, bool stats, bool halfm, hipStream_t st);      // conv_wino.hip
// conv_wino_slab.hip: k_conv_wino2d_m128 or (limb) k_conv_wino2d_limb; the finish of every slab kernel, k_conv_wino2d included;
// the weight image k_conv_wino2d_limb reads
int wino_slab_launch(const WinoProblem& p, dim3 grid, bool limb, hipStream_t st);
int wino2d_finish_launch(const WinoProblem& p, int ksplit, hipStream_t st);
int wino_limb_weight_launch(const float* w, float* U, int M, int C, int flip, hipStream_t st);

// ---- conv_wino_wgrad.hip
bool wino_wgrad_ok(const fd_conv_desc* d);
long wino_wgrad_ws_floats(const fd_conv_desc* d);
int wino_wgrad_launch(const fd_conv_desc* d, const float* x, const float* gy, float* gw, float* ws, int accumulate, hipStream_t st);

// ---- device side.  Internal linkage: every unit compiles its own copy of what it uses.
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((__vector_size__(2 * sizeof(unsigned int))));

__device__ __forceinline__ f32x2 fd_ldg64(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)byte_off, 0, 0));
}
// ELU / sigmoid / tanh (decoder layers): one out-of-line copy, so that the fully unrolled epilogue (32 values per lane) does not
// carry 32 inlined copies of three libm routines
__device__ __attribute__((noinline)) float wino_act_slow(float v, int act) {
    if (act == 2) return v > 0.f ? v : expm1f(v);
    if (act == 3) return 1.0f / (1.0f + expf(-v));
    return tanhf(v);
}
__device__ __forceinline__ float wino_act(float v, int act) {
    if (act >= 2) return wino_act_slow(v, act);
    return act == 1 ? fmaxf(v, 0.f) : v;
}

constexpr int WBM = 64, WBN = 64, WBKC = 16, WNT = 256;
constexpr int LDU = WBM + 1, LDV = WBN, LDM = WBN + 1;
// k_conv_wino keeps the activations RAW in LDS - one row of the tile's 128 pixels per channel: [0] a cell that stays 0.0,
// [3] the pixel left of the tile, [4 .. 131] the tile, [132] the pixel right of it - and applies the input transform when the
// B operands are read: 8.7 KB per chunk instead of the 16.4 KB of four transformed components (the VGPR -> LDS store path is what
// bounds the main loop, scripts/wino_ksweep.py), and 50.7 KB per workgroup = three workgroups per CU.
constexpr int LDR = 2 * WBN + 8;
constexpr int V_RAW_FLOATS = 9 * 64 * 4;                      // 16 rows x 136 = 2176 floats, rounded up to 9 wave-wide 16-byte DMAs
constexpr int W_BUF_FLOATS = 4 * WBKC * LDU + V_RAW_FLOATS;   // one operand buffer: U (four components) + raw activations
// double-buffered operands: 66 KB -> 2 workgroups per CU.  (A single-buffered variant - 33 KB, 4 per CU, two barriers per chunk - and a
// one-chunk-deep register pipeline both measured the same; an 8-channel-chunk variant - 33 KB, 3 per CU - was 2-5 % faster alone
// and 2 % slower inside the training step, where its extra resident waves take CUs from the other streams' kernels.)
constexpr int W_LDS_FLOATS = 2 * W_BUF_FLOATS;       // k_conv_wino: the double-buffered operands (its output transform stays in registers)
constexpr int M2_KC = 8, M2_BM = 128;                // k_conv_wino2d_m128: channels per chunk, output channels per workgroup

struct WinoArgs : WinoProblem {};      // the forward kernels' parameter: WinoProblem under the name their symbols carry

struct WinoWgradArgs {
    const float* dY; const float* X; float* slabs;
    int M, C, Nb, H, W;
    int pad_mode;
    long pairs_per_split;
    int slice_major;     // 1: grid x = pixel slice (XCD-aligned), z = (ky, c tile); 0: x = (ky, c tile), z = slice
    int slab_rows;       // rows per output channel in a slab: 9 = [ky][kx], 12 = [ri][kx] (k_wgrad_wino<.., true>)
    int xcds_per_slice;  // slice_major == 2 with fewer than 8 slices: XCDs per slice (8 / slices), else 1
    int adv_n, adv_y, adv_j;   // one chunk of WGP pairs = adv_n images + adv_y rows + adv_j pairs (host: divisions once per launch)
};

// the six limb products of one split-precision MFMA k-step (conv_limb.h), smallest terms first: the forward and the
// weight-gradient limb kernels
typedef __bf16 wl_bf16x8 __attribute__((ext_vector_type(8)));
#define FD_WLIMB_MFMA6(ACC, AF, BF)                                                                                                   \
    do {                                                                                                                              \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wl_bf16x8, AF[2]), __builtin_bit_cast(wl_bf16x8, BF[0]), ACC, 0, 0, 0); \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wl_bf16x8, AF[0]), __builtin_bit_cast(wl_bf16x8, BF[2]), ACC, 0, 0, 0); \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wl_bf16x8, AF[1]), __builtin_bit_cast(wl_bf16x8, BF[1]), ACC, 0, 0, 0); \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wl_bf16x8, AF[1]), __builtin_bit_cast(wl_bf16x8, BF[0]), ACC, 0, 0, 0); \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wl_bf16x8, AF[0]), __builtin_bit_cast(wl_bf16x8, BF[1]), ACC, 0, 0, 0); \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wl_bf16x8, AF[0]), __builtin_bit_cast(wl_bf16x8, BF[0]), ACC, 0, 0, 0); \
    } while (0)

}  // namespace
