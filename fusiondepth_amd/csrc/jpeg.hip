// FD_HIPCC_FLAGS: -fwrapv
// Baseline JPEG frames (include/fdhip.h, "baseline JPEG frames"): the C ABI of the host entropy decoder (csrc/jpeg_entropy.h) and the
// device half - dequantisation + libjpeg's ISLOW inverse DCT into uint8 component planes (launch A), fancy chroma upsampling + YCbCr
// -> RGB + the packed [H][W][3] store (launch B).  Integer arithmetic throughout; int32 wraps (-fwrapv), as the header states.
//   k_jpeg_idct    blockIdx.y = the frame; a workgroup takes 32 blocks per step, 8 lanes per block: lane l loads coefficient row l
//                  (one 16-byte load, one 16-byte table load), the column pass and the row pass go through an LDS tile padded to 9
//                  ints per row (a column read then touches 8 different banks), and lane l stores sample row l as one 8-byte store.
//   k_jpeg_rgb     blockIdx.y = the frame; a thread owns one 16-byte chunk of the frame's RGB bytes - the six pixels that touch it -
//                  and writes one uint4; the bytes before the first and after the last 16-byte boundary go out one by one.
#include "fd_common.h"
#include "fdhip.h"
#include "jpeg_entropy.h"

extern "C" int fd_jpeg_probe(const unsigned char* file, long n, fd_jpeg_info* info) {
    char err[fdjpeg::ERR_LEN] = "";
    const int st = fdjpeg::probe(file, n, info, err);
    if (st != 0 || err[0]) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_jpeg_entropy_decode(const unsigned char* file, long n, int16_t* coef, long coef_cap, uint16_t* qt, fd_jpeg_info* info) {
    char err[fdjpeg::ERR_LEN] = "";
    const int st = fdjpeg::entropy_decode(file, n, coef, coef_cap, qt, info, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

namespace {

struct JFrame {
    bool out_ok;          // the frame lies inside `out`: something is written
    bool ok;              // ... and its sources lie inside staging: else zeros
    int kind, comps, hs, vs, W, H;
    int pw[3];            // plane widths in bytes
    unsigned nb[3];       // blocks per component (3 * W * H < 2^31 bounds them)
    long coef_off, qt_off, plane_off[3], out_off;
};

__device__ __forceinline__ bool jpeg_region(long off, long bytes, long total, long align) {
    return off >= 0 && (off & (align - 1)) == 0 && bytes <= total && off <= total - bytes;
}

__device__ __forceinline__ void jpeg_frame(const fd_jpeg_desc& d, long staging_bytes, long out_bytes, JFrame& f) {
    f.kind = d.kind; f.comps = d.components; f.hs = d.h_samp; f.vs = d.v_samp; f.W = d.width; f.H = d.height;
    f.coef_off = d.coef_off; f.qt_off = d.qt_off; f.out_off = d.out_off;
    f.out_ok = f.ok = false;
    if (f.W < 1 || f.W > 65535 || f.H < 1 || f.H > 65535) return;
    const long rgb = 3L * f.W * f.H;
    if (rgb > 0x7fffffffL) return;                                // byte and block indices inside a frame are 32-bit below
    f.out_ok = jpeg_region(f.out_off, rgb, out_bytes, 1);
    if (!f.out_ok) return;
    if (f.kind == 1) {
        f.ok = jpeg_region(f.coef_off, rgb, staging_bytes, 1);
        return;
    }
    if (f.kind != 0) return;
    // each factor on its own, before any shift uses it: 1x1, 2x1 or 2x2, and 1x1 alone for one component
    if (f.comps != 1 && f.comps != 3) return;
    if (f.hs < 1 || f.hs > 2 || f.vs < 1 || f.vs > f.hs) return;
    if (f.comps == 1 && f.hs != 1) return;
    const int sx = 2 + f.hs, sy = 2 + f.vs;                       // log2 of the MCU's size in pixels
    const int mcux = (f.W + (1 << sx) - 1) >> sx, mcuy = (f.H + (1 << sy) - 1) >> sy;
    long blocks = 0, at = d.plane_off;
    for (int c = 0; c < 3; ++c) {
        const int bw = c < f.comps ? mcux * (c ? 1 : f.hs) : 0, bh = c < f.comps ? mcuy * (c ? 1 : f.vs) : 0;
        f.pw[c] = 8 * bw;
        f.nb[c] = (unsigned)bw * (unsigned)bh;
        f.plane_off[c] = at;
        at += 64L * f.nb[c];
        blocks += f.nb[c];
    }
    f.ok = jpeg_region(f.coef_off, 128 * blocks, staging_bytes, 16) && jpeg_region(f.qt_off, 384, staging_bytes, 16) &&
           jpeg_region(d.plane_off, 64 * blocks, staging_bytes, 16);
}

// jidctint.c's 1-D pass on x[0..7] -> the eight sums before descaling
__device__ __forceinline__ void jpeg_idct8(int (&x)[8]) {
    int z1 = (x[2] + x[6]) * 4433;
    const int t2 = z1 - x[6] * 15137, t3 = z1 + x[2] * 6270;
    const int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int o0 = x[7], o1 = x[5], o2 = x[3], o3 = x[1];
    z1 = o0 + o3;
    int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const int z5 = (z3 + z4) * 9633;
    o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    x[0] = t10 + o3; x[7] = t10 - o3;
    x[1] = t11 + o2; x[6] = t11 - o2;
    x[2] = t12 + o1; x[5] = t12 - o1;
    x[3] = t13 + o0; x[4] = t13 - o0;
}

__device__ __forceinline__ unsigned jpeg_limit(int y) {
    const int i = y & 1023;
    return (unsigned)(i < 128 ? 128 + i : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

__global__ __launch_bounds__(256) void k_jpeg_idct(unsigned char* __restrict__ staging, long staging_bytes,
                                                   const fd_jpeg_desc* __restrict__ desc, long out_bytes) {
    __shared__ int tile[32][8][9];
    JFrame f;
    jpeg_frame(desc[blockIdx.y], staging_bytes, out_bytes, f);
    if (!f.ok || f.kind != 0) return;                             // uniform over the workgroup
    const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
    const unsigned nb = f.nb[0] + f.nb[1] + f.nb[2];
    for (unsigned base = blockIdx.x * 32u; base < nb; base += gridDim.x * 32u) {
        const unsigned b = base + g;
        const bool act = b < nb;
        int c = 0;
        unsigned bl = b;
        if (bl >= f.nb[0] && f.comps == 3) {
            bl -= f.nb[0];
            c = 1;
            if (bl >= f.nb[1]) {
                bl -= f.nb[1];
                c = 2;
            }
        }
        int x[8];
        if (act) {
            const uint4 cw = *reinterpret_cast<const uint4*>(staging + f.coef_off + 128L * b + 16 * l);
            const uint4 qw = *reinterpret_cast<const uint4*>(staging + f.qt_off + 128 * c + 16 * l);
            const unsigned cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                tile[g][l][2 * j] = (int)(short)(cs[j] & 0xFFFFu) * (int)(qs[j] & 0xFFFFu);
                tile[g][l][2 * j + 1] = (int)(short)(cs[j] >> 16) * (int)(qs[j] >> 16);
            }
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = tile[g][j][l];
            jpeg_idct8(x);
#pragma unroll
            for (int j = 0; j < 8; ++j) tile[g][j][l] = (x[j] + (1 << 10)) >> 11;
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = tile[g][l][j];
            jpeg_idct8(x);
            unsigned s[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = jpeg_limit((x[j] + (1 << 17)) >> 18);
            // selects, not f.pw[c]: an array indexed by a run-time value would live in scratch memory
            const unsigned pwc = (unsigned)(c == 0 ? f.pw[0] : f.pw[1]), bwc = pwc >> 3;
            const long plane = c == 0 ? f.plane_off[0] : (c == 1 ? f.plane_off[1] : f.plane_off[2]);
            const unsigned by = bl / bwc, bx = bl - by * bwc;
            uint2 v;
            v.x = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
            v.y = s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24);
            *reinterpret_cast<uint2*>(staging + plane + (long)((by * 8 + l) * pwc + bx * 8)) = v;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int jpeg_chroma(const unsigned char* __restrict__ C, int pw, int x, int y, int hs, int vs, int dw, int dh) {
    if (hs == 1) return C[y * pw + x];
    const int c = x >> 1;
    if (dw <= 2) return C[(vs == 2 ? y >> 1 : y) * pw + c];
    if (vs == 1) {
        const unsigned char* r = C + y * pw;
        const int a = r[c];
        if (x & 1) return c == dw - 1 ? a : (3 * a + r[c + 1] + 2) >> 2;
        return c == 0 ? a : (3 * a + r[c - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const int far = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    const unsigned char* r0 = C + r * pw;
    const unsigned char* r1 = C + far * pw;
    const int s = 3 * r0[c] + r1[c];
    if (x & 1) return c == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[c + 1] + r1[c + 1] + 7) >> 4;
    return c == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[c - 1] + r1[c - 1] + 8) >> 4;
}

__device__ __forceinline__ unsigned jpeg_clamp8(int v) { return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// pixel `pix` = (x, y) of the frame as R | G << 8 | B << 16
__device__ __forceinline__ unsigned jpeg_pixel(const JFrame& f, const unsigned char* __restrict__ st, unsigned pix, int x, int y) {
    if (!f.ok) return 0u;
    if (f.kind == 1) {
        const unsigned char* p = st + f.coef_off + 3L * pix;
        return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
    const int Y = st[f.plane_off[0] + y * f.pw[0] + x];
    if (f.comps == 1) return (unsigned)Y * 0x010101u;
    const int dw = f.hs == 2 ? (f.W + 1) >> 1 : f.W, dh = f.vs == 2 ? (f.H + 1) >> 1 : f.H;
    const int cb = jpeg_chroma(st + f.plane_off[1], f.pw[1], x, y, f.hs, f.vs, dw, dh) - 128;
    const int cr = jpeg_chroma(st + f.plane_off[2], f.pw[2], x, y, f.hs, f.vs, dw, dh) - 128;
    const unsigned R = jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
    const unsigned G = jpeg_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    const unsigned B = jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    return R | (G << 8) | (B << 16);
}

__global__ __launch_bounds__(256) void k_jpeg_rgb(const unsigned char* __restrict__ staging, long staging_bytes,
                                                  const fd_jpeg_desc* __restrict__ desc, unsigned char* __restrict__ out, long out_bytes) {
    JFrame f;
    jpeg_frame(desc[blockIdx.y], staging_bytes, out_bytes, f);
    if (!f.out_ok) return;
    const unsigned Wu = (unsigned)f.W, npix = Wu * (unsigned)f.H, total = 3u * npix;       // 3 * W * H < 2^31
    unsigned char* o = out + f.out_off;
    unsigned head = (16u - (unsigned)((uintptr_t)o & 15u)) & 15u;
    head = head < total ? head : total;
    const unsigned chunks = (total - head) / 16u;
    const unsigned tail = head + 16u * chunks;                   // first byte after the last whole chunk
    const unsigned t = threadIdx.x;
    if (blockIdx.x == 0 && t < 32) {                             // the head and the tail: fewer than 16 bytes each
        const unsigned b = t < 16 ? t : tail + (t - 16);
        const bool in = t < 16 ? b < head : b < total;
        if (in) {
            const unsigned p = b / 3u, y = p / Wu;
            o[b] = (unsigned char)(jpeg_pixel(f, staging, p, (int)(p - y * Wu), (int)y) >> (8 * (int)(b - 3u * p)));
        }
    }
    for (unsigned ck = blockIdx.x * 256u + t; ck < chunks; ck += gridDim.x * 256u) {
        const unsigned b0 = head + 16u * ck;
        const unsigned p0 = b0 / 3u;
        const int r = (int)(b0 - 3u * p0);
        unsigned y = p0 / Wu, x = p0 - y * Wu;
        unsigned px[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            px[j] = p0 + j < npix ? jpeg_pixel(f, staging, p0 + j, (int)x, (int)y) : 0u;
            if (++x == Wu) {
                x = 0;
                ++y;
            }
        }
        unsigned w[5];
        w[0] = px[0] | (px[1] << 24);
        w[1] = (px[1] >> 8) | (px[2] << 16);
        w[2] = (px[2] >> 16) | (px[3] << 8);
        w[3] = px[4] | (px[5] << 24);
        w[4] = px[5] >> 8;
        uint4 v;
        v.x = (unsigned)(((((unsigned long long)w[1]) << 32) | w[0]) >> (8 * r));
        v.y = (unsigned)(((((unsigned long long)w[2]) << 32) | w[1]) >> (8 * r));
        v.z = (unsigned)(((((unsigned long long)w[3]) << 32) | w[2]) >> (8 * r));
        v.w = (unsigned)(((((unsigned long long)w[4]) << 32) | w[3]) >> (8 * r));
        *reinterpret_cast<uint4*>(o + b0) = v;
    }
}

}  // namespace

extern "C" int fd_jpeg_reconstruct(void* staging, long staging_bytes, const fd_jpeg_desc* desc, int N, unsigned char* out, long out_bytes,
                                   void* stream) {
    FD_REQUIRE(staging && desc && out && N >= 1 && N <= 65535 && staging_bytes > 0 && out_bytes > 0, "fd_jpeg_reconstruct: bad args");
    FD_REQUIRE(((uintptr_t)staging & 15) == 0 && ((uintptr_t)desc & 7) == 0, "fd_jpeg_reconstruct: staging must be 16-byte aligned, desc 8-byte");
    hipStream_t st = (hipStream_t)stream;
    // the descriptors live on the device: size both grids from the mean frame, the workgroups of a frame stride over its work
    const long mean = out_bytes / N;
    int gx = fd_cdiv(fd_cdiv(mean, 64), 32);                      // blocks of a 4:4:4 frame of the mean size, 32 per workgroup step
    gx = gx < 1 ? 1 : (gx > 16384 ? 16384 : gx);
    hipLaunchKernelGGL(k_jpeg_idct, dim3(gx, N), dim3(256), 0, st, (unsigned char*)staging, staging_bytes, desc, out_bytes);
    FD_LAUNCH_CHECK("k_jpeg_idct");
    gx = fd_cdiv(fd_cdiv(mean, 16), 256);
    gx = gx < 1 ? 1 : (gx > 16384 ? 16384 : gx);
    hipLaunchKernelGGL(k_jpeg_rgb, dim3(gx, N), dim3(256), 0, st, (const unsigned char*)staging, staging_bytes, desc, out, out_bytes);
    FD_LAUNCH_CHECK("k_jpeg_rgb");
    return 0;
}
