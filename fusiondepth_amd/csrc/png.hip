// PNG frames (include/fdhip.h, "PNG frames"): the C ABI of the host inflate (csrc/png_inflate.h) and the device half - the five scanline
// filters undone in place (launch A), the packed RGB / host-order uint16 store (launch B).  Bytes and integer arithmetic throughout.
//   k_png_unfilter blockIdx.x = the frame, FD_PNG_BAND_ROWS lanes = as many rows, walked as a skewed wavefront: at step t lane r
//                  reconstructs pixel t - r of its row, hands it to lane r + 1 through a double-buffered LDS word (one barrier per
//                  step) and keeps what it got a step ago as the above-left pixel.  A lane streams its own row: aligned 16-byte loads
//                  three pieces ahead of the one in use, a 64-bit window for the bytes, aligned 4-byte stores (single bytes up to the
//                  row's first aligned word and behind its last) back over the filtered bytes.  Bands of a taller frame follow each
//                  other in the same workgroup; lane 0 of a later band replays the row above it as an unfiltered row.
//   k_png_store    blockIdx.y = the frame; a thread owns one 16-byte chunk of the frame's output bytes and writes one uint4; the
//                  bytes before the first and after the last 16-byte boundary go out one by one.
#include "fd_common.h"
#include "fdhip.h"
#include "png_inflate.h"

extern "C" int fd_png_probe(const unsigned char* file, long n, fd_png_info* info) {
    char err[fdpng::ERR_LEN] = "";
    const int st = fdpng::probe(file, n, info, err);
    if (st != 0 || err[0]) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_png_inflate(const unsigned char* file, long n, unsigned char* dst, long dst_cap, fd_png_info* info) {
    char err[fdpng::ERR_LEN] = "";
    const int st = fdpng::inflate(file, n, dst, dst_cap, info, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_png_band_rows(void) { return FD_PNG_BAND_ROWS; }

namespace {

constexpr int BAND = FD_PNG_BAND_ROWS;

struct PFrame {
    int kind, W, H, bpp, mode;
    long raw_off, out_off;
    unsigned total;       // output bytes
    unsigned raw_bytes;   // source bytes
};

// The descriptor rule of include/fdhip.h: nullptr when `d` may be used, else what is wrong with it.  The host applies it to the
// caller's table before any launch, the kernels to the copy they read.
__host__ __device__ inline const char* png_check(const fd_png_desc& d, long table_end, long staging_bytes, long out_bytes, PFrame& f) {
    f.kind = d.kind; f.W = d.width; f.H = d.height; f.bpp = d.bpp; f.mode = d.mode; f.raw_off = d.raw_off; f.out_off = d.out_off;
    f.total = f.raw_bytes = 0;
    if (f.kind != 0 && f.kind != 1) return "kind is neither 0 nor 1";
    if (f.mode != 0 && f.mode != 1) return "mode is neither 0 (rgb) nor 1 (gray16)";
    if (f.kind == 0 && !((f.bpp == 3 && f.mode == 0) || (f.bpp == 1 && f.mode == 0) || (f.bpp == 2 && f.mode == 1)))
        return "bpp and mode are none of (3, rgb), (1, rgb), (2, gray16)";
    if (f.W < 1 || f.W > 65535 || f.H < 1 || f.H > 65535) return "width or height outside 1 .. 65535";
    const long total = (f.mode ? 2L : 3L) * f.W * f.H;
    const long raw = f.kind == 0 ? (long)f.H * (1 + (long)f.W * f.bpp) : total;
    if (total > 0x7fffffffL || raw > 0x7fffffffL) return "more than 2^31 - 1 bytes in one frame";
    f.total = (unsigned)total;
    f.raw_bytes = (unsigned)raw;
    if (f.raw_off < table_end) return "raw_off lies before the end of the descriptor table";
    const long span = f.kind == 0 ? (raw + (f.raw_off & 15) + 15) / 16 * 16 - (f.raw_off & 15) : raw;   // up to the next 16-byte boundary
    if (span > staging_bytes || f.raw_off > staging_bytes - span) return "the frame's source leaves staging";
    if (f.out_off < 0 || total > out_bytes || f.out_off > out_bytes - total) return "the frame leaves out";
    if (f.mode == 1 && (f.out_off & 1)) return "out_off of a gray16 frame is odd";
    return nullptr;
}

__device__ __forceinline__ long png_table_end(int N) { return ((long)N * (long)sizeof(fd_png_desc) + 15) / 16 * 16; }

// one byte of the five predictors, chosen by `ft`
__device__ __forceinline__ unsigned png_predict(unsigned ft, unsigned a, unsigned b, unsigned c) {
    const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    const unsigned paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    return ft == 1 ? a : (ft == 2 ? b : (ft == 3 ? (a + b) >> 1 : (ft == 4 ? paeth : 0u)));
}

template <int BPP>
__device__ __forceinline__ void png_walk(unsigned char* __restrict__ staging, const PFrame& f, unsigned* sh) {
    const int lane = (int)threadIdx.x;
    const unsigned pitch = 1u + (unsigned)f.W * BPP;
    const long lim = (f.raw_off + (long)f.raw_bytes + 15) / 16 * 16;           // no 16-byte load reaches past it; png_check holds it inside staging
    constexpr unsigned MASK = BPP == 3 ? 0xFFFFFFu : (BPP == 2 ? 0xFFFFu : 0xFFu);
    for (int first = 0; first < f.H;) {
        const int shift = first > 0 ? 1 : 0;                     // a later band: lane 0 replays the row above it
        const int rows_here = min(BAND - shift, f.H - first);
        const int lanes = rows_here + shift;
        const int row = first + lane - shift;
        const bool valid = lane < lanes;
        const bool pass = shift && lane == 0;
        long at = 0;                                             // the next byte to read, from staging
        uint4 c0 = make_uint4(0, 0, 0, 0), c1 = c0, c2 = c0, c3 = c0;
        long pn = 0;
        int taken = 0, have = 0, oh = 0;
        unsigned long long win = 0, ow = 0;
        unsigned ft = 0, prev = 0, cprev = 0;
        long q = 0;                                              // the next byte to write
        auto load = [&](long off) { return off + 16 <= lim ? *reinterpret_cast<const uint4*>(staging + off) : make_uint4(0, 0, 0, 0); };
        auto next_word = [&]() {
            const unsigned d = c0.x;
            c0.x = c0.y; c0.y = c0.z; c0.z = c0.w;
            if (++taken == 4) {
                c0 = c1; c1 = c2; c2 = c3;
                c3 = load(pn);
                pn += 16;
                taken = 0;
            }
            return d;
        };
        if (valid) {
            at = f.raw_off + (long)row * pitch;
            ft = pass ? 0u : (unsigned)staging[at];
            ft = ft > 4u ? 0u : ft;
            ++at;
            q = at;
            const long chunk = at & ~15L;
            c0 = load(chunk); c1 = load(chunk + 16); c2 = load(chunk + 32); c3 = load(chunk + 48);
            pn = chunk + 64;
            const int skip = (int)(at & 15);
            for (int i = 0; i < (skip >> 2); ++i) next_word();
            win = next_word() >> (8 * (skip & 3));
            have = 4 - (skip & 3);
        }
        const int steps = f.W + lanes - 1;
        for (int t = 0; t < steps; ++t) {
            const int x = t - lane;
            const unsigned ub = lane > 0 ? sh[((t + 1) & 1) * BAND + lane - 1] : 0u;
            if (valid && x >= 0 && x < f.W) {
                if (have < BPP) {
                    win |= (unsigned long long)next_word() << (8 * have);
                    have += 4;
                }
                const unsigned px = (unsigned)win & MASK;
                win >>= 8 * BPP;
                have -= BPP;
                const unsigned b = row == 0 ? 0u : ub;
                unsigned cur = 0;
#pragma unroll
                for (int k = 0; k < BPP; ++k) {
                    const unsigned p = png_predict(ft, (prev >> (8 * k)) & 255u, (b >> (8 * k)) & 255u, (cprev >> (8 * k)) & 255u);
                    cur |= ((((px >> (8 * k)) & 255u) + p) & 255u) << (8 * k);
                }
                cprev = b;
                prev = cur;
                sh[(t & 1) * BAND + lane] = cur;
                if (!pass) {
                    ow |= (unsigned long long)cur << (8 * oh);
                    oh += BPP;
                    while ((q & 3) && oh) {                      // up to the row's first aligned word
                        staging[q++] = (unsigned char)ow;
                        ow >>= 8;
                        --oh;
                    }
                    if (!(q & 3) && oh >= 4) {
                        *reinterpret_cast<unsigned*>(staging + q) = (unsigned)ow;
                        ow >>= 32;
                        oh -= 4;
                        q += 4;
                    }
                }
            }
            // LDS alone crosses this barrier: __syncthreads() would also wait for the row stores, and with them for the loads ahead
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        if (valid && !pass) {
            for (; oh; --oh, ow >>= 8) staging[q++] = (unsigned char)ow;
            staging[f.raw_off + (long)row * pitch] = 0;          // the row now is an unfiltered one: a second call changes nothing
        }
        __syncthreads();                                         // the band's last row is read by the next band's lane 0
        first += rows_here;
    }
}

__global__ __launch_bounds__(BAND) void k_png_unfilter(unsigned char* __restrict__ staging, long staging_bytes, int N, long out_bytes) {
    __shared__ unsigned sh[2 * BAND];
    PFrame f;
    const fd_png_desc* desc = reinterpret_cast<const fd_png_desc*>(staging);
    if (png_check(desc[blockIdx.x], png_table_end(N), staging_bytes, out_bytes, f) || f.kind != 0) return;   // uniform over the workgroup
    if (f.bpp == 3) png_walk<3>(staging, f, sh);
    else if (f.bpp == 2) png_walk<2>(staging, f, sh);
    else png_walk<1>(staging, f, sh);
}

// byte j of the frame's output, from the reconstructed scanlines (or the raw bytes)
__device__ __forceinline__ unsigned png_out_byte(const PFrame& f, const unsigned char* __restrict__ src, unsigned j) {
    if (f.kind == 1) return src[j];
    const unsigned W = (unsigned)f.W;
    if (f.mode == 1) {                                           // big-endian sample -> host order
        const unsigned p = j >> 1, y = p / W, x = p - y * W;
        return src[y * (1u + 2u * W) + 1u + 2u * x + (1u - (j & 1u))];
    }
    if (f.bpp == 3) {
        const unsigned y = j / (3u * W);
        return src[j + y + 1u];
    }
    const unsigned p = j / 3u, y = p / W;
    return src[p + y + 1u];
}

__global__ __launch_bounds__(256) void k_png_store(const unsigned char* __restrict__ staging, long staging_bytes, int N,
                                                   unsigned char* __restrict__ out, long out_bytes) {
    PFrame f;
    const fd_png_desc* desc = reinterpret_cast<const fd_png_desc*>(staging);
    if (png_check(desc[blockIdx.y], png_table_end(N), staging_bytes, out_bytes, f)) return;
    const unsigned char* src = staging + f.raw_off;
    unsigned char* o = out + f.out_off;
    const unsigned total = f.total;
    unsigned head = (16u - (unsigned)((uintptr_t)o & 15u)) & 15u;
    head = head < total ? head : total;
    const unsigned chunks = (total - head) / 16u;
    const unsigned tail = head + 16u * chunks;                   // first byte after the last whole chunk
    const unsigned t = threadIdx.x;
    if (blockIdx.x == 0 && t < 32) {                             // the head and the tail: fewer than 16 bytes each
        const unsigned b = t < 16 ? t : tail + (t - 16);
        const bool in = t < 16 ? b < head : b < total;
        if (in) o[b] = (unsigned char)png_out_byte(f, src, b);
    }
    for (unsigned ck = blockIdx.x * 256u + t; ck < chunks; ck += gridDim.x * 256u) {
        const unsigned b0 = head + 16u * ck;
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) w[i] |= png_out_byte(f, src, b0 + 4 * i + k) << (8 * k);
        }
        *reinterpret_cast<uint4*>(o + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

extern "C" int fd_png_unfilter(void* staging, long staging_bytes, const fd_png_desc* desc, int N, unsigned char* out, long out_bytes,
                               void* stream) {
    FD_REQUIRE(staging && desc && out && N >= 1 && N <= 65535 && staging_bytes > 0 && out_bytes > 0, "fd_png_unfilter: bad args");
    FD_REQUIRE(((uintptr_t)staging & 15) == 0 && ((uintptr_t)out & 15) == 0, "fd_png_unfilter: staging and out must be 16-byte aligned");
    const long table_end = ((long)N * (long)sizeof(fd_png_desc) + 15) / 16 * 16;
    FD_REQUIRE(table_end <= staging_bytes, "fd_png_unfilter: staging is shorter than its descriptor table");
    for (int i = 0; i < N; ++i) {
        PFrame f;
        const char* why = png_check(desc[i], table_end, staging_bytes, out_bytes, f);
        FD_REQUIRE(!why, "fd_png_unfilter: descriptor %d: %s", i, why);
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_png_unfilter, dim3(N), dim3(BAND), 0, st, (unsigned char*)staging, staging_bytes, N, out_bytes);
    FD_LAUNCH_CHECK("k_png_unfilter");
    int gx = fd_cdiv(fd_cdiv(out_bytes / N, 16), 256);           // the descriptors differ in size: the workgroups of a frame stride over it
    gx = gx < 1 ? 1 : (gx > 16384 ? 16384 : gx);
    hipLaunchKernelGGL(k_png_store, dim3(gx, N), dim3(256), 0, st, (const unsigned char*)staging, staging_bytes, N, out, out_bytes);
    FD_LAUNCH_CHECK("k_png_store");
    return 0;
}
