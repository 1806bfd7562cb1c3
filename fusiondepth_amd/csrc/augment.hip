// FD_HIPCC_FLAGS: -ffp-contract=off
// The image half of a KITTI training item on the GPU (reference datasets/mono_dataset.py:85-104): Pillow's 8-bit antialiased
// Lanczos resample, the four ColorJitter operations on a uint8 image, and ToTensor.  Inputs and intermediates are uint8 HWC
// (what a decoder produces); the network inputs leave as float32 NCHW planes.
//
// Everything here is pinned BIT FOR BIT to PIL (tests/augment_ref.py restates the rules in numpy and is itself checked against
// PIL): the resample is integer arithmetic on host-built coefficient tables; brightness / contrast / saturation are PIL's
// float32 blend; the hue shift follows PIL's RGB <-> HSV conversion with its mix of float32 and double steps.  This file is
// compiled with -ffp-contract=off and spells the rounding-sensitive steps with the *_rn intrinsics: a fused multiply-add in the
// blend or in the HSV code changes bytes.
//
// Memory: global accesses are 16 bytes per lane wherever the addresses allow it (source rows of the horizontal pass are staged
// in LDS through aligned 16-byte chunks, whatever the row pitch); byte accesses remain only on the unaligned fall-back paths
// (an output row pitch that is not a multiple of 16, the last partial group of an image).
#include "../../include/fdhip.h"
#include "fd_common.h"

namespace {

constexpr int PREC = 22;                 // Pillow Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int TX = 64, TY = 8;           // horizontal pass: output columns x rows per block
constexpr int VROWS = 4;                 // vertical pass: output rows per block (one wave each)
constexpr int JBPI = 64;                 // contrast statistics: blocks (= partial sums) per image

__host__ __device__ inline long round16(long v) { return (v + 15) & ~15L; }
// Accumulators are unsigned: like Pillow's int sums they may pass 2^31 on the way (renormalised edge windows have coefficients of
// twice the usual size) and come back; unsigned wrap-around is defined, signed overflow is not.
// The empty asm keeps the shift and the clamp apart: hipcc (ROCm 7) otherwise fuses two neighbouring bytes into gfx950's
// v_ashr_pk_u8_i32 and ORs the other bytes of the word into its result as if bits 31:16 of that result were zero - on the
// MI355X they are not, and bytes 2 and 3 of every packed word came out ORed with stale register contents.
__device__ __forceinline__ unsigned clip8(unsigned acc) {
    int v = (int)acc >> PREC;
    asm volatile("" : "+v"(v));
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ------------------------------------------------------------------------------------------------ Lanczos, horizontal pass
// src [N][Hin][Win][3] -> tmp [N][Hin][pitch] (pitch = Wout * 3 rounded up to 16).  tab: per output column (first tap, tap count,
// kx coefficients).  A block owns TX output columns of TY rows: it stages the tile's tap table and the source span of each row
// in LDS, forms the integer dot products from LDS, and stores the output tile through LDS in 16-byte chunks.  Every LDS index
// is clamped to the staged span, so a malformed table gives wrong pixels, never an out-of-range access.
__global__ void __launch_bounds__(256) k_lanczos_h(const uint8_t* __restrict__ src, long src_bytes, uint8_t* __restrict__ tmp, int Hin,
                                                   int Win, int Wout, int pitch, const int* __restrict__ tab, int kx,
                                                   const int* __restrict__ mirror, int span_px, int lrow) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int stride = 2 + kx;
    int* s_tab = (int*)smem;                                             // [TX][2 + kx]
    unsigned char* s_src = smem + round16((long)TX * stride * 4);        // [TY][lrow]
    unsigned char* s_out = s_src + (long)TY * lrow;                      // [TY][TX * 3]
    const int tid = threadIdx.x, n = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int nx = min(TX, Wout - x0), ny = min(TY, Hin - y0);
    for (int i = tid; i < nx * stride; i += 256) s_tab[i] = tab[(long)x0 * stride + i];
    __syncthreads();
    const int lo = fd_clampi(s_tab[0], 0, Win - 1);
    int hi = fd_clampi(s_tab[(nx - 1) * stride] + s_tab[(nx - 1) * stride + 1], lo + 1, Win);
    if (hi - lo > span_px) hi = lo + span_px;
    const bool mir = mirror != nullptr && mirror[n] != 0;
    const int mlo = mir ? Win - hi : lo;                                 // the span's first pixel in memory
    const int len = (hi - lo) * 3;
    const int nch_max = lrow >> 4;
    for (int i = tid; i < ny * nch_max; i += 256) {
        const int r = i / nch_max, c = i - r * nch_max;
        const long g0 = ((long)((long)n * Hin + y0 + r) * Win + mlo) * 3;
        const int head = (int)(g0 & 15);
        if (c * 16 >= head + len) continue;
        const long a = (g0 - head) + 16L * c;
        uint4 v;
        if (a + 16 <= src_bytes) {
            v = *reinterpret_cast<const uint4*>(src + a);
        } else {                                                         // the buffer's last, partial chunk
            unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (a + b < src_bytes) w[b >> 2] |= (unsigned)src[a + b] << (8 * (b & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(s_src + (long)r * lrow + 16 * c) = v;
    }
    __syncthreads();
    const int per_row = nx * 3;
    for (int i = tid; i < ny * per_row; i += 256) {
        const int r = i / per_row, rem = i - r * per_row, xx = rem / 3, c = rem - xx * 3;
        const int* t = s_tab + xx * stride;
        const int xmin = t[0], cnt = fd_clampi(t[1], 0, kx);
        const int head = (int)((((long)((long)n * Hin + y0 + r) * Win + mlo) * 3) & 15);
        const unsigned char* row = s_src + (long)r * lrow + head + c;
        unsigned acc = 1u << (PREC - 1);
        for (int k = 0; k < cnt; ++k) {
            const int px = xmin + k;
            const int rel = fd_clampi(mir ? hi - 1 - px : px - lo, 0, hi - lo - 1);
            acc += (unsigned)row[rel * 3] * (unsigned)t[2 + k];
        }
        s_out[r * (TX * 3) + rem] = (unsigned char)clip8(acc);
    }
    __syncthreads();
    constexpr int OCH = TX * 3 / 16;
    for (int i = tid; i < ny * OCH; i += 256) {
        const int r = i / OCH, c = i - r * OCH;
        const int off = x0 * 3 + 16 * c;
        if (off < pitch)
            *reinterpret_cast<uint4*>(tmp + ((long)n * Hin + y0 + r) * pitch + off) =
                *reinterpret_cast<const uint4*>(s_out + r * (TX * 3) + 16 * c);
    }
}

// ------------------------------------------------------------------------------------------------ Lanczos, vertical pass
// tmp [N][Hin][pitch] -> dst [N][Hout][rowbytes].  A wave owns one output row, a lane 16 consecutive bytes of it: one 16-byte
// load per tap row, 16 integer accumulators, one 16-byte store (ALIGNED: rowbytes and dst are multiples of 16).
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_lanczos_v(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst, int Hin, int Hout,
                                                   int rowbytes, int pitch, const int* __restrict__ tab, int ky) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* s_tab = (int*)smem;                                             // [VROWS][2 + ky]
    const int stride = 2 + ky;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = blockIdx.z;
    const int y0 = blockIdx.y * VROWS, ny = min(VROWS, Hout - y0);
    for (int i = tid; i < ny * stride; i += 256) s_tab[i] = tab[(long)y0 * stride + i];
    __syncthreads();
    const int y = y0 + wv, j = blockIdx.x * 64 + lane;
    if (wv >= ny || 16 * j >= rowbytes) return;
    const int* t = s_tab + wv * stride;
    const int ymin = t[0], cnt = fd_clampi(t[1], 0, ky);
    unsigned acc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = 1u << (PREC - 1);
    const uint8_t* col = tmp + (long)n * Hin * pitch + 16 * j;
    for (int k = 0; k < cnt; ++k) {
        const int r = fd_clampi(ymin + k, 0, Hin - 1);
        const uint4 v = *reinterpret_cast<const uint4*>(col + (long)r * pitch);
        const unsigned cf = (unsigned)t[2 + k];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] += ((w[b >> 2] >> (8 * (b & 3))) & 255u) * cf;
    }
    unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) o[b >> 2] |= clip8(acc[b]) << (8 * (b & 3));
    uint8_t* out = dst + ((long)n * Hout + y) * rowbytes + 16 * j;
    if (ALIGNED) {
        *reinterpret_cast<uint4*>(out) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int nb = min(16, rowbytes - 16 * j);
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (b < nb) out[b] = (uint8_t)((o[b >> 2] >> (8 * (b & 3))) & 255u);
    }
}

// ------------------------------------------------------------------------------------------------ groups of 16 pixels
// A lane handles 16 consecutive pixels of an image = 48 bytes = three 16-byte words, and writes 16 floats per colour plane.
__device__ __forceinline__ void load16(const uint8_t* p, int npx, bool vec, unsigned (&w)[12]) {
    if (vec && npx == 16) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        const uint4 a = q[0], b = q[1], c = q[2];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = 0u;
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < npx * 3) w[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
    }
}

__device__ __forceinline__ void store16(uint8_t* p, int npx, bool vec, const unsigned (&w)[12]) {
    if (vec && npx == 16) {
        uint4* q = reinterpret_cast<uint4*>(p);
        q[0] = make_uint4(w[0], w[1], w[2], w[3]);
        q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        q[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < npx * 3) p[i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
    }
}

__device__ __forceinline__ int byte_of(const unsigned (&w)[12], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// ToTensor: v / 255 correctly rounded; plane c of the image starts at planes + c * hw
__device__ __forceinline__ void store_planes16(float* planes, long hw, long first, int npx, bool vec, const unsigned (&w)[12]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) f[i] = __fdiv_rn((float)byte_of(w, 3 * i + c), 255.0f);
        float* o = planes + c * hw + first;
        if (vec && npx == 16) {
            float4* q = reinterpret_cast<float4*>(o);
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < npx) o[i] = f[i];
        }
    }
}

__global__ void __launch_bounds__(256) k_u8_to_planes(const uint8_t* __restrict__ src, float* __restrict__ dst, long hw, long dst_stride,
                                                      int vec_in, int vec_out) {
    const int n = blockIdx.y;
    const long ngrp = (hw + 15) / 16;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ngrp; g += (long)gridDim.x * 256) {
        const int npx = (int)min(16L, hw - 16 * g);
        unsigned w[12];
        load16(src + ((long)n * hw + 16 * g) * 3, npx, vec_in != 0, w);
        store_planes16(dst + (long)n * dst_stride, hw, 16 * g, npx, vec_out != 0, w);
    }
}

// ------------------------------------------------------------------------------------------------ ColorJitter
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// PIL Image.blend(degenerate, image, f): float32, truncated; clipped first when f lies outside [0, 1]
__device__ __forceinline__ int blend1(int deg, int v, float f, bool inside) {
    float t = __fadd_rn((float)deg, __fmul_rn(f, (float)(v - deg)));
    if (!inside) t = t <= 0.f ? 0.f : (t >= 255.f ? 255.f : t);
    return (int)t;
}

__device__ __forceinline__ int round_half_away(double x) { return (int)(x >= 0.0 ? floor(x + 0.5) : ceil(x - 0.5)); }

// PIL Convert.c rgb2hsv_row, H += shift (uint8 wrap-around), hsv2rgb.  Where the C code evaluates in double (a float operand
// meeting a double literal) this does too; the float32 steps use the *_rn intrinsics.
__device__ __forceinline__ void hue_px(int& r, int& g, int& b, int shift) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
        float h;
        if (r == maxc) h = __fsub_rn(bc, gc);
        else if (g == maxc) h = (float)__dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc);
        else h = (float)__dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc);
        const double hd = __dadd_rn(__ddiv_rn((double)h, 6.0), 1.0);        // in (0, 2): fmod(hd, 1.0) = hd - floor(hd), exact
        h = (float)(hd - floor(hd));
        uh = fd_clampi((int)__dmul_rn((double)h, 255.0), 0, 255);
        us = fd_clampi((int)__dmul_rn((double)s, 255.0), 0, 255);
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double h6 = __ddiv_rn(__dmul_rn((double)uh, 6.0), 255.0);
    const double fi = floor(h6);
    const float f = (float)(h6 - fi);
    const float fs = (float)__ddiv_rn((double)(float)us, 255.0);
    const double vf = (double)uv;
    const int p = fd_clampi(round_half_away(__dmul_rn(vf, __dsub_rn(1.0, (double)fs))), 0, 255);
    const int q = fd_clampi(round_half_away(__dmul_rn(vf, __dsub_rn(1.0, (double)__fmul_rn(fs, f)))), 0, 255);
    const int t = fd_clampi(round_half_away(__dmul_rn(vf, __dsub_rn(1.0, __dmul_rn((double)fs, __dsub_rn(1.0, (double)f))))), 0, 255);
    switch ((int)fi % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// What a block needs of its image's table entry, read once through the table pointer (the entry is the same for the whole block, so
// these live in scalar registers; a per-thread copy of the struct indexed by order[k] would be spilled to LDS).
struct JitterOps {
    float fb, fc, fs;      // brightness, contrast, saturation factors
    int shift;             // uint8 hue offset
    int ord;               // operation k in bits 2k+1 : 2k
    int n_ops;
    int cpos;              // position of the contrast operation, -1: none
    bool ok;               // n_ops in range, ids in range, no operation twice
};

__device__ __forceinline__ JitterOps load_ops(const fd_jitter_desc* __restrict__ d) {
    JitterOps o;
    o.fb = d->factor[0]; o.fc = d->factor[1]; o.fs = d->factor[2];
    o.shift = d->hue_shift & 255;
    o.n_ops = d->n_ops;
    o.ok = o.n_ops >= 0 && o.n_ops <= 4;
    o.ord = 0; o.cpos = -1;
    int seen = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (o.ok && k < o.n_ops) {
            const int op = d->order[k];
            if (op < 0 || op > 3 || ((seen >> op) & 1)) o.ok = false;
            seen |= 1 << (op & 3);
            o.ord |= (op & 3) << (2 * k);
            if (op == 1) o.cpos = k;
        }
    }
    return o;
}

// operations [first, last) of the image's order on one pixel; `mean` = the contrast operation's grey level
__device__ __forceinline__ void apply_ops(int& r, int& g, int& b, const JitterOps& o, int first, int last, int mean) {
    for (int k = first; k < last; ++k) {
        const int op = (o.ord >> (2 * k)) & 3;
        if (op == 3) {
            hue_px(r, g, b, o.shift);
            continue;
        }
        const float f = op == 0 ? o.fb : (op == 1 ? o.fc : o.fs);
        const bool inside = f >= 0.f && f <= 1.f;
        const int deg = op == 0 ? 0 : (op == 1 ? mean : luma(r, g, b));
        r = blend1(deg, r, f, inside); g = blend1(deg, g, f, inside); b = blend1(deg, b, f, inside);
    }
}

// an image whose extent leaves a buffer is skipped as a whole (the table lives on the device: the host cannot check it)
__device__ __forceinline__ bool extent_ok(const fd_jitter_desc* __restrict__ d, long src_bytes) {
    return d->H > 0 && d->W > 0 && d->src_off >= 0 && d->src_off + 3L * d->H * d->W <= src_bytes;
}

__device__ __forceinline__ bool outputs_ok(const fd_jitter_desc* __restrict__ d, long dst_bytes, long planes_floats, bool has_u8, bool has_planes) {
    const long hw = (long)d->H * d->W;
    if (d->u8_off >= 0 && (!has_u8 || d->u8_off + 3 * hw > dst_bytes)) return false;
    if (d->planes_off >= 0 && (!has_planes || d->planes_off + 3 * hw > planes_floats)) return false;
    if (d->plain_off >= 0 && (!has_planes || d->plain_off + 3 * hw > planes_floats)) return false;
    return true;
}

// exact integer sum of L over the image as it stands when the contrast operation is reached: wave shuffle, then LDS, then one
// partial per block; k_jitter_mean adds an image's JBPI partials in a fixed order.  Integers: any order gives the same sum.
__global__ void __launch_bounds__(256) k_jitter_stats(const uint8_t* __restrict__ src, long src_bytes, const fd_jitter_desc* __restrict__ desc,
                                                      unsigned long long* __restrict__ part, int src_vec) {
    __shared__ unsigned long long red[4];
    const int img = blockIdx.y, tid = threadIdx.x;
    const fd_jitter_desc* __restrict__ d = desc + img;
    const JitterOps o = load_ops(d);
    unsigned long long sum = 0ull;
    if (extent_ok(d, src_bytes) && o.ok && o.cpos >= 0) {
        const long src_off = d->src_off, hw = (long)d->H * d->W, ngrp = (hw + 15) / 16;
        const bool vec = src_vec && (src_off & 15) == 0;
        for (long g = (long)blockIdx.x * 256 + tid; g < ngrp; g += (long)JBPI * 256) {
            const int npx = (int)min(16L, hw - 16 * g);
            unsigned w[12];
            load16(src + src_off + 48 * g, npx, vec, w);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < npx) {
                    int r = byte_of(w, 3 * i), gg = byte_of(w, 3 * i + 1), b = byte_of(w, 3 * i + 2);
                    apply_ops(r, gg, b, o, 0, o.cpos, 0);
                    sum += (unsigned long long)luma(r, gg, b);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, FD_WAVE);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) part[(long)img * JBPI + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one wave per image: mean[img] = int(sum / pixels + 0.5) in double (PIL ImageStat mean), -1 for an image without contrast
__global__ void __launch_bounds__(256) k_jitter_mean(const unsigned long long* __restrict__ part, const fd_jitter_desc* __restrict__ desc,
                                                     int n_images, int* __restrict__ mean) {
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (img >= n_images) return;
    unsigned long long sum = part[(long)img * JBPI + lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, FD_WAVE);
    if (lane == 0) {
        const fd_jitter_desc* __restrict__ d = desc + img;
        const JitterOps o = load_ops(d);
        const bool has = d->H > 0 && d->W > 0 && o.ok && o.cpos >= 0;
        mean[img] = has ? (int)(__ddiv_rn((double)sum, (double)((long)d->H * d->W)) + 0.5) : -1;
    }
}

__global__ void __launch_bounds__(256) k_jitter_apply(const uint8_t* __restrict__ src, long src_bytes, uint8_t* __restrict__ dst_u8,
                                                      long dst_bytes, float* __restrict__ dst_planes, long planes_floats,
                                                      const fd_jitter_desc* __restrict__ desc, const int* __restrict__ mean, int base_vec) {
    const int img = blockIdx.y;
    const fd_jitter_desc* __restrict__ d = desc + img;
    const JitterOps o = load_ops(d);
    if (!o.ok || !extent_ok(d, src_bytes) || !outputs_ok(d, dst_bytes, planes_floats, dst_u8 != nullptr, dst_planes != nullptr)) return;
    const long src_off = d->src_off, u8_off = d->u8_off, planes_off = d->planes_off, plain_off = d->plain_off;
    const long hw = (long)d->H * d->W, ngrp = (hw + 15) / 16;
    const int m = mean[img];
    const bool vec_in = (base_vec & 1) && (src_off & 15) == 0;
    const bool vec_u8 = (base_vec & 2) && (u8_off & 15) == 0;
    const bool vec_pl = (base_vec & 4) && (planes_off & 3) == 0 && (hw & 3) == 0;
    const bool vec_pp = (base_vec & 4) && (plain_off & 3) == 0 && (hw & 3) == 0;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ngrp; g += (long)gridDim.x * 256) {
        const int npx = (int)min(16L, hw - 16 * g);
        unsigned w[12];
        load16(src + src_off + 48 * g, npx, vec_in, w);
        if (plain_off >= 0) store_planes16(dst_planes + plain_off, hw, 16 * g, npx, vec_pp, w);
        if (o.n_ops > 0) {
            unsigned q[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) q[i] = 0u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                int r = byte_of(w, 3 * i), gg = byte_of(w, 3 * i + 1), b = byte_of(w, 3 * i + 2);
                apply_ops(r, gg, b, o, 0, o.n_ops, m);
                q[(3 * i) >> 2] |= (unsigned)r << (8 * ((3 * i) & 3));
                q[(3 * i + 1) >> 2] |= (unsigned)gg << (8 * ((3 * i + 1) & 3));
                q[(3 * i + 2) >> 2] |= (unsigned)b << (8 * ((3 * i + 2) & 3));
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) w[i] = q[i];
        }
        if (u8_off >= 0) store16(dst_u8 + u8_off + 48 * g, npx, vec_u8, w);
        if (planes_off >= 0) store_planes16(dst_planes + planes_off, hw, 16 * g, npx, vec_pl, w);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------ entry points
extern "C" long fd_resize_lanczos_u8_ws_bytes(int N, int Hin, int Win, int Hout, int Wout) {
    if (N <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return 0;
    return (long)N * Hin * round16((long)Wout * 3);
}

extern "C" int fd_resize_lanczos_u8(const uint8_t* src, uint8_t* dst, int N, int Hin, int Win, int Hout, int Wout, const int* xtab,
                                    int kx, const int* ytab, int ky, const int* mirror, void* ws, void* stream) {
    FD_REQUIRE(src && dst && xtab && ytab && ws, "fd_resize_lanczos_u8: bad args (null pointer)");
    FD_REQUIRE(N > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && kx > 0 && ky > 0, "fd_resize_lanczos_u8: bad args (N %d, %dx%d -> %dx%d, taps %d / %d)",
               N, Hin, Win, Hout, Wout, kx, ky);
    FD_REQUIRE(N <= 65535 && (long)N * Hin * (long)Win * 3 < (1L << 40), "fd_resize_lanczos_u8: batch too large");
    FD_REQUIRE(aligned16(src) && aligned16(ws), "fd_resize_lanczos_u8: src and ws must be 16-byte aligned");
    const int kx_need = 2 * (int)((3L * (Win > Wout ? Win : Wout) + Wout - 1) / Wout) + 1;
    const int ky_need = 2 * (int)((3L * (Hin > Hout ? Hin : Hout) + Hout - 1) / Hout) + 1;
    FD_REQUIRE(kx == kx_need && ky == ky_need, "fd_resize_lanczos_u8: tap counts %d / %d, the Lanczos support of %dx%d -> %dx%d needs %d / %d",
               kx, ky, Hin, Win, Hout, Wout, kx_need, ky_need);
    hipStream_t st = (hipStream_t)stream;
    const int pitch = (int)round16((long)Wout * 3);
    // source pixels one tile of TX output columns can touch
    int span_px = (int)(((long)TX * Win + Wout - 1) / Wout) + kx + 2;
    if (span_px > Win) span_px = Win;
    const int lrow = (int)round16((long)span_px * 3 + 15);
    const long lds_h = round16((long)TX * (2 + kx) * 4) + (long)TY * lrow + (long)TY * TX * 3;
    const long lds_v = (long)VROWS * (2 + ky) * 4;
    FD_REQUIRE(lds_h <= 64 * 1024 && lds_v <= 64 * 1024, "fd_resize_lanczos_u8: %dx%d -> %dx%d shrinks too far for the LDS tiles (%ld / %ld bytes)", Hin,
               Win, Hout, Wout, lds_h, lds_v);
    const long src_bytes = (long)N * Hin * Win * 3;
    dim3 gh(fd_cdiv(Wout, TX), fd_cdiv(Hin, TY), N);
    FD_REQUIRE(gh.y <= 65535, "fd_resize_lanczos_u8: image too tall");
    hipLaunchKernelGGL(k_lanczos_h, gh, dim3(256), (size_t)lds_h, st, src, src_bytes, (uint8_t*)ws, Hin, Win, Wout, pitch, xtab, kx, mirror,
                       span_px, lrow);
    FD_LAUNCH_CHECK("fd_resize_lanczos_u8(horizontal)");
    const int rowbytes = Wout * 3;
    dim3 gv(fd_cdiv(fd_cdiv(rowbytes, 16), 64), fd_cdiv(Hout, VROWS), N);
    FD_REQUIRE(gv.y <= 65535, "fd_resize_lanczos_u8: image too tall");
    if (rowbytes % 16 == 0 && aligned16(dst))
        hipLaunchKernelGGL(k_lanczos_v<true>, gv, dim3(256), (size_t)lds_v, st, (const uint8_t*)ws, dst, Hin, Hout, rowbytes, pitch, ytab, ky);
    else
        hipLaunchKernelGGL(k_lanczos_v<false>, gv, dim3(256), (size_t)lds_v, st, (const uint8_t*)ws, dst, Hin, Hout, rowbytes, pitch, ytab, ky);
    FD_LAUNCH_CHECK("fd_resize_lanczos_u8(vertical)");
    return 0;
}

extern "C" int fd_u8_to_planes(const uint8_t* src, float* dst, int N, int H, int W, long dst_image_stride, void* stream) {
    FD_REQUIRE(src && dst && N > 0 && H > 0 && W > 0 && N <= 65535, "fd_u8_to_planes: bad args");
    const long hw = (long)H * W;
    FD_REQUIRE(dst_image_stride >= 3 * hw, "fd_u8_to_planes: image stride %ld < 3 * %d * %d", dst_image_stride, H, W);
    const int vec_in = aligned16(src) && (hw * 3) % 16 == 0;
    const int vec_out = aligned16(dst) && hw % 4 == 0 && dst_image_stride % 4 == 0;
    long blocks = ((hw + 15) / 16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_u8_to_planes, dim3((unsigned)blocks, N), dim3(256), 0, (hipStream_t)stream, src, dst, hw, dst_image_stride, vec_in,
                       vec_out);
    FD_LAUNCH_CHECK("fd_u8_to_planes");
    return 0;
}

extern "C" long fd_color_jitter_u8_ws_bytes(int n_images) {
    if (n_images <= 0) return 0;
    return (long)n_images * JBPI * 8 + round16((long)n_images * 4);
}

extern "C" long fd_color_jitter_u8_means_offset(int n_images) {
    if (n_images <= 0) return 0;
    return (long)n_images * JBPI * 8;
}

extern "C" int fd_color_jitter_u8(const uint8_t* src, long src_bytes, uint8_t* dst_u8, long dst_bytes, float* dst_planes,
                                  long planes_floats, const fd_jitter_desc* desc, int n_images, long max_pixels, void* ws, void* stream) {
    FD_REQUIRE(src && desc && ws && (dst_u8 || dst_planes), "fd_color_jitter_u8: bad args (null pointer)");
    FD_REQUIRE(n_images > 0 && n_images <= 65535 && max_pixels > 0 && src_bytes > 0, "fd_color_jitter_u8: bad args (%d images, %ld pixels, %ld bytes)",
               n_images, max_pixels, src_bytes);
    FD_REQUIRE((!dst_u8 || dst_bytes > 0) && (!dst_planes || planes_floats > 0), "fd_color_jitter_u8: an output buffer needs its size");
    FD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)desc & 7) == 0, "fd_color_jitter_u8: ws and desc must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* part = (unsigned long long*)ws;
    int* mean = (int*)((char*)ws + fd_color_jitter_u8_means_offset(n_images));
    const int base_vec = (aligned16(src) ? 1 : 0) | (dst_u8 && aligned16(dst_u8) ? 2 : 0) | (dst_planes && aligned16(dst_planes) ? 4 : 0);
    hipLaunchKernelGGL(k_jitter_stats, dim3(JBPI, n_images), dim3(256), 0, st, src, src_bytes, desc, part, base_vec & 1);
    FD_LAUNCH_CHECK("fd_color_jitter_u8(stats)");
    hipLaunchKernelGGL(k_jitter_mean, dim3(fd_cdiv(n_images, 4)), dim3(256), 0, st, (const unsigned long long*)part, desc, n_images, mean);
    FD_LAUNCH_CHECK("fd_color_jitter_u8(mean)");
    long blocks = ((max_pixels + 15) / 16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_jitter_apply, dim3((unsigned)blocks, n_images), dim3(256), 0, st, src, src_bytes, dst_u8, dst_bytes, dst_planes,
                       planes_floats, desc, (const int*)mean, base_vec);
    FD_LAUNCH_CHECK("fd_color_jitter_u8(apply)");
    return 0;
}
