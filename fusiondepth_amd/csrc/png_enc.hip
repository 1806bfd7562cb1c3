// PNG outputs (include/fdhip.h, "PNG outputs"): the C ABI of the host plan (csrc/png_deflate.h) and the three launches of the encoder.
// Bytes and integer arithmetic throughout; every shared word is combined with an integer atomic, so two calls give the same bytes.
//   k_png_enc_filter   blockIdx.x = a group of FD_PNG_ENC_GROUP_ROWS scanlines of one frame, a wave per scanline, a lane per byte.
//                      Walk 1 sums the five filters' costs; walk 2 writes the winner's bytes, counts the tokens into LDS and sums
//                      the Adler pair.
//   k_png_enc_rowbits  the same grid over the filtered scanlines: the bits each row's tokens take under its block's code.
//   k_png_enc_emit     the same grid: headers, tokens, end-of-block and the file's fixed bytes ORed into the cleared output.
// A run of equal bytes is closed by the lane that holds the NEXT run's first byte: it knows the run's value (the byte before its
// own) and, from the wave's ballot of run starts, where the run began.
#include "fd_common.h"
#include "fdhip.h"
#include "png_deflate.h"

extern "C" int fd_png_enc_block_rows(void) { return FD_PNG_ENC_BLOCK_ROWS; }

extern "C" int fd_png_enc_layout(fd_png_enc_desc* desc, int N, fd_png_enc_sizes* sizes) {
    char err[fdpngenc::ERR_LEN] = "";
    const int st = fdpngenc::layout(desc, N, sizes, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_png_enc_plan(fd_png_enc_desc* desc, int N, const unsigned* stats, fd_png_enc_block* blocks, long* total_bytes) {
    char err[fdpngenc::ERR_LEN] = "";
    const int st = fdpngenc::plan(desc, N, stats, blocks, total_bytes, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

extern "C" int fd_png_enc_finish(unsigned char* files, long nbytes, const fd_png_enc_desc* desc) {
    char err[fdpngenc::ERR_LEN] = "";
    const int st = fdpngenc::finish(files, nbytes, desc, err);
    if (st != 0) fd_set_error("%s", err);
    return st;
}

namespace {

constexpr int GROUP = FD_PNG_ENC_GROUP_ROWS;
constexpr int ROWS = FD_PNG_ENC_BLOCK_ROWS;
constexpr int HIST = FD_PNG_ENC_HIST;
constexpr unsigned ADLER = 65521u;

__constant__ unsigned short LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};

__device__ __forceinline__ int len_extra(int k) { return k < 8 || k == 28 ? 0 : (k - 4) >> 2; }

// match length m (3 .. 258) -> k, its symbol being 257 + k
__device__ __forceinline__ void fill_len_index(unsigned char* lidx) {
    for (int m = threadIdx.x; m < 259; m += blockDim.x) {
        int k = 0;
        for (int q = 1; q < 29; ++q) k = m >= (int)LEN_BASE[q] ? q : k;
        lidx[m] = (unsigned char)k;
    }
}

struct Row {
    const fd_png_enc_desc* d;
    int row;                 // inside the frame; -1: this wave has none
};

// The scanline of wave (threadIdx.x / 64) of group blockIdx.x: the frame is the last one whose first_group is not above the group.
__device__ __forceinline__ Row find_row(const fd_png_enc_desc* desc, int N) {
    const int g = (int)blockIdx.x;
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].first_group <= g) lo = mid;
        else hi = mid - 1;
    }
    Row r;
    r.d = desc + lo;
    r.row = (g - desc[lo].first_group) * GROUP + (int)(threadIdx.x >> 6);
    if (r.row < 0 || r.row >= desc[lo].height) r.row = -1;
    return r;
}

// Calls on_run(has, value, length) once per 64-byte step and once at the row's end, in EVERY lane of the wave (so on_run may use
// wave-wide operations); `has` lanes hold one closed run each, in the row's order by lane.  get(j) = byte j of the scanline, j < P.
template <class Get, class OnRun>
__device__ __forceinline__ void for_runs(unsigned P, Get get, OnRun on_run) {
    const unsigned lane = threadIdx.x & 63u;
    unsigned open = 0, carry = 0, cur = 0;
    for (unsigned base = 0; base < P; base += 64u) {
        const unsigned j = base + lane;
        const bool in = j < P;
        cur = in ? get(j) : 0u;
        unsigned prev = __shfl_up(cur, 1, 64);
        prev = lane == 0 ? carry : prev;
        const bool start = in && (j == 0 || cur != prev);
        const unsigned long long mask = __ballot(start);
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        const unsigned from = below ? base + 63u - (unsigned)__clzll((long long)below) : open;
        on_run(start && j > 0, prev, j - from);
        if (mask) open = base + 63u - (unsigned)__clzll((long long)mask);
        carry = __shfl(cur, 63, 64);
    }
    const unsigned last = __shfl(cur, (int)((P - 1u) & 63u), 64);
    on_run(lane == 0, last, P - open);
}

struct Pixels {
    const unsigned char* cur;    // the row's bytes in memory
    const unsigned char* up;     // the row above, or nullptr
    unsigned bpp, swap;          // swap = 1: 16-bit samples, byte i of the scanline is byte i ^ 1 in memory
};

// byte i (0 .. R-1) of the row under each filter
__device__ __forceinline__ void filtered5(const Pixels& p, unsigned i, unsigned f[5]) {
    const unsigned k = i ^ p.swap;
    const unsigned x = p.cur[k];
    const unsigned a = i >= p.bpp ? p.cur[k - p.bpp] : 0u;
    const unsigned b = p.up ? p.up[k] : 0u;
    const unsigned c = (p.up && i >= p.bpp) ? p.up[k - p.bpp] : 0u;
    const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    const unsigned paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = x;
    f[1] = (x - a) & 255u;
    f[2] = (x - b) & 255u;
    f[3] = (x - ((a + b) >> 1)) & 255u;
    f[4] = (x - paeth) & 255u;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64 * GROUP) void k_png_enc_filter(unsigned char* __restrict__ work, int N, long stat_off, long blocks) {
    __shared__ unsigned hist[HIST];
    __shared__ unsigned char lidx[259];
    const fd_png_enc_desc* desc = reinterpret_cast<const fd_png_enc_desc*>(work);
    for (int s = threadIdx.x; s < HIST; s += blockDim.x) hist[s] = 0;
    fill_len_index(lidx);
    __syncthreads();
    const Row r = find_row(desc, N);
    const fd_png_enc_desc& d = *r.d;                             // the same frame in all four waves
    const unsigned lane = threadIdx.x & 63u;
    if (r.row >= 0) {
        const unsigned R = (unsigned)d.width * (unsigned)d.bpp, P = R + 1u;
        Pixels px;
        px.bpp = (unsigned)d.bpp;
        px.swap = d.bpp == 2 ? 1u : 0u;
        px.cur = reinterpret_cast<const unsigned char*>(d.src) + (long)r.row * R;
        px.up = r.row > 0 ? px.cur - R : nullptr;
        unsigned cost[5] = {0, 0, 0, 0, 0};
        for (unsigned i = lane; i < R; i += 64u) {
            unsigned f[5];
            filtered5(px, i, f);
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += f[t] < 128u ? f[t] : 256u - f[t];
        }
        unsigned ft = 0, best = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const unsigned c = wave_sum_u32(cost[t]);
            if (t == 0 || c < best) {
                best = c;
                ft = (unsigned)t;
            }
        }
        unsigned char* dst = work + d.ws_off + (long)r.row * P;
        unsigned sum = 0;
        unsigned long long wsum = 0;
        for_runs(P,
                 [&](unsigned j) {
                     unsigned v = ft;
                     if (j > 0) {
                         unsigned f[5];
                         filtered5(px, j - 1u, f);
                         v = f[ft];
                     }
                     dst[j] = (unsigned char)v;
                     sum += v;
                     wsum += (unsigned long long)(P - j) * v;
                     return v;
                 },
                 [&](bool has, unsigned v, unsigned L) {
                     if (!has) return;
                     const unsigned n258 = (L - 1u) / 258u, m = (L - 1u) % 258u;
                     atomicAdd(&hist[v & 255u], 1u + (m < 3u ? m : 0u));
                     if (n258) atomicAdd(&hist[285], n258);
                     if (m >= 3u) atomicAdd(&hist[257 + lidx[m]], 1u);
                     if (n258 || m >= 3u) atomicAdd(&hist[286], n258 + (m >= 3u ? 1u : 0u));
                 });
        sum = wave_sum_u32(sum);                                 // at most 65535 * 3 * 255 + 4
        wsum = wave_sum_u64(wsum);
        if (lane == 0) {
            unsigned* adler = reinterpret_cast<unsigned*>(work + stat_off) + blocks * HIST + 2L * (d.first_row + r.row);
            adler[0] = sum % ADLER;
            adler[1] = (unsigned)(wsum % ADLER);
        }
    }
    __syncthreads();
    const int block = d.first_block + ((int)blockIdx.x - d.first_group) * GROUP / ROWS;
    unsigned* gh = reinterpret_cast<unsigned*>(work + stat_off) + (long)block * HIST;
    for (int s = threadIdx.x; s < HIST - 1; s += blockDim.x)
        if (hist[s]) atomicAdd(&gh[s], hist[s]);
}

// what one closed run's tokens take under the block's code
__device__ __forceinline__ unsigned run_bits(const unsigned char* len, const unsigned char* lidx, unsigned dl, unsigned v, unsigned L) {
    const unsigned n258 = (L - 1u) / 258u, m = (L - 1u) % 258u;
    unsigned bits = len[v & 255u] * (1u + (m < 3u ? m : 0u)) + n258 * (len[285] + dl);
    if (m >= 3u) {
        const int k = lidx[m];
        bits += len[257 + k] + (unsigned)len_extra(k) + dl;
    }
    return bits;
}

__global__ __launch_bounds__(64 * GROUP) void k_png_enc_rowbits(unsigned char* __restrict__ work, int N, long rowbits_off, long table_off) {
    __shared__ unsigned char len[288];
    __shared__ unsigned char lidx[259];
    const fd_png_enc_desc* desc = reinterpret_cast<const fd_png_enc_desc*>(work);
    const Row r = find_row(desc, N);
    const fd_png_enc_desc& d = *r.d;
    const int block = d.first_block + ((int)blockIdx.x - d.first_group) * GROUP / ROWS;
    const fd_png_enc_block* blk = reinterpret_cast<const fd_png_enc_block*>(work + table_off) + block;
    for (int s = threadIdx.x; s < 288; s += blockDim.x) len[s] = blk->len[s];
    fill_len_index(lidx);
    __syncthreads();
    if (r.row < 0) return;
    const unsigned dl = blk->dist_len ? 1u : 0u;
    const unsigned P = (unsigned)d.width * (unsigned)d.bpp + 1u;
    const unsigned char* src = work + d.ws_off + (long)r.row * P;
    unsigned bits = 0;
    for_runs(P, [&](unsigned j) { return (unsigned)src[j]; },
             [&](bool has, unsigned v, unsigned L) { bits += has ? run_bits(len, lidx, dl, v, L) : 0u; });
    bits = wave_sum_u32(bits);                                   // at most 196606 * 15
    if ((threadIdx.x & 63u) == 0) reinterpret_cast<unsigned*>(work + rowbits_off)[d.first_row + r.row] = bits;
}

// The cleared output as 32-bit words, and the one file a wave may write to.
struct Sink {
    unsigned* words;
    unsigned long long lo, hi;   // the file's first bit and the bit behind its last
    // `bits` <= 32 bits of v at bit `at`: nothing outside [lo, hi) is touched
    __device__ __forceinline__ void put(unsigned long long at, unsigned v, unsigned bits) const {
        if (!bits || at < lo || at + bits > hi) return;
        const unsigned long long x = (unsigned long long)v << (at & 31ull);
        if ((unsigned)x) atomicOr(words + (at >> 5), (unsigned)x);
        if ((unsigned)(x >> 32)) atomicOr(words + (at >> 5) + 1, (unsigned)(x >> 32));
    }
};

// byte `i` (0 .. 54) of the file's fixed part -> its offset inside the file and its value; false: nothing at this index
__device__ __forceinline__ bool fixed_byte(const fd_png_enc_desc& d, int i, long& at, unsigned& v) {
    const long zlen = d.out_bytes - 57;
    const unsigned depth = d.bpp == 2 ? 16u : 8u, colour = d.bpp == 3 ? 2u : 0u;
    const unsigned char sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    at = i;
    if (i < 16) v = sig[i];
    else if (i < 20) v = ((unsigned)d.width >> (8 * (19 - i))) & 255u;
    else if (i < 24) v = ((unsigned)d.height >> (8 * (23 - i))) & 255u;
    else if (i == 24) v = depth;
    else if (i == 25) v = colour;
    else if (i < 33) return false;                               // compression, filter, interlace 0; IHDR's CRC is the host's
    else if (i < 37) v = (unsigned)(zlen >> (8 * (36 - i))) & 255u;
    else if (i < 41) v = (unsigned)"IDAT"[i - 37];
    else if (i == 41) v = 0x78u;
    else if (i == 42) v = 0x01u;
    else if (i < 47) {                                           // the Adler-32 behind the blocks
        at = 43 + (d.stream_bits + 7) / 8 + (i - 43);
        v = (d.adler >> (8 * (46 - i))) & 255u;
    } else if (i < 51) return false;                             // IEND's length 0
    else if (i < 55) {
        at = d.out_bytes - 8 + (i - 51);
        v = (unsigned)"IEND"[i - 51];
    } else return false;
    return true;
}

__global__ __launch_bounds__(64 * GROUP) void k_png_enc_emit(const unsigned char* __restrict__ work, int N, long rowbits_off, long table_off,
                                                             unsigned* __restrict__ out, long out_bytes) {
    __shared__ unsigned char len[288];
    __shared__ unsigned short code[288];
    __shared__ unsigned char lidx[259];
    const fd_png_enc_desc* desc = reinterpret_cast<const fd_png_enc_desc*>(work);
    const Row r = find_row(desc, N);
    const fd_png_enc_desc& d = *r.d;
    const int block = d.first_block + ((int)blockIdx.x - d.first_group) * GROUP / ROWS;
    const fd_png_enc_block* blk = reinterpret_cast<const fd_png_enc_block*>(work + table_off) + block;
    for (int s = threadIdx.x; s < 288; s += blockDim.x) {
        len[s] = blk->len[s];
        code[s] = blk->code[s];
    }
    fill_len_index(lidx);
    __syncthreads();
    if (r.row < 0) return;
    if (d.out_off < 0 || d.out_bytes < 63 || d.out_bytes > out_bytes || d.out_off > out_bytes - d.out_bytes) return;
    const unsigned lane = threadIdx.x & 63u;
    Sink sink;
    sink.words = out;
    sink.lo = 8ull * (unsigned long long)d.out_off;
    sink.hi = sink.lo + 8ull * (unsigned long long)d.out_bytes;
    if (r.row == 0) {
        long at;
        unsigned v;
        if (fixed_byte(d, (int)lane, at, v)) sink.put(sink.lo + 8ull * (unsigned long long)at, v, 8);
    }
    const unsigned dl = blk->dist_len ? 1u : 0u;
    const int in_block = r.row % ROWS;
    const unsigned* rowbits = reinterpret_cast<const unsigned*>(work + rowbits_off) + d.first_row + (r.row - in_block);
    const unsigned long long before = wave_sum_u64((int)lane < in_block ? rowbits[lane] : 0u);
    const unsigned long long start = sink.lo + 8ull * 43ull + blk->bit_off;
    if (in_block == 0) {                                         // the block's header
        const unsigned words = (blk->header_bits + 31u) / 32u;
        for (unsigned w = lane; w < words && w < FD_PNG_ENC_HEADER_WORDS; w += 64u) {
            const unsigned left = blk->header_bits - 32u * w;
            sink.put(start + 32ull * w, blk->header[w], left < 32u ? left : 32u);
        }
    }
    unsigned long long pos = start + blk->header_bits + before;
    const unsigned P = (unsigned)d.width * (unsigned)d.bpp + 1u;
    const unsigned char* src = work + d.ws_off + (long)r.row * P;
    for_runs(P, [&](unsigned j) { return (unsigned)src[j]; },
             [&](bool has, unsigned v, unsigned L) {
                 const unsigned mine = has ? run_bits(len, lidx, dl, v, L) : 0u;
                 unsigned incl = mine;
#pragma unroll
                 for (int off = 1; off < 64; off <<= 1) {
                     const unsigned o = __shfl_up(incl, off, 64);
                     incl += (int)lane >= off ? o : 0u;
                 }
                 if (has) {
                     unsigned long long at = pos + (incl - mine);
                     const unsigned n258 = (L - 1u) / 258u, m = (L - 1u) % 258u;
                     v &= 255u;
                     sink.put(at, code[v], len[v]);
                     at += len[v];
                     for (unsigned k = 0; k < n258; ++k, at += len[285] + dl) sink.put(at, code[285], len[285] + dl);
                     for (unsigned k = 0; m < 3u && k < m; ++k, at += len[v]) sink.put(at, code[v], len[v]);
                     if (m >= 3u) {
                         const int k = lidx[m];
                         const unsigned l = len[257 + k], eb = (unsigned)len_extra(k);
                         sink.put(at, code[257 + k] | ((m - LEN_BASE[k]) << l), l + eb + dl);
                     }
                 }
                 pos += __shfl(incl, 63, 64);
             });
    if (lane == 0 && (in_block == ROWS - 1 || r.row == d.height - 1)) sink.put(pos, code[256], len[256]);
}

}  // namespace

extern "C" int fd_png_enc_filter(void* work, long work_bytes, const fd_png_enc_desc* desc, int N, void* stream) {
    FD_REQUIRE(work && desc && ((uintptr_t)work & 15) == 0, "fd_png_enc_filter: bad args (work must be 16-byte aligned)");
    fd_png_enc_sizes sz;
    char err[fdpngenc::ERR_LEN] = "";
    FD_REQUIRE(fdpngenc::check_layout(desc, N, work_bytes, &sz, err) == 0, "fd_png_enc_filter: %s", err);
    for (int i = 0; i < N; ++i)
        FD_REQUIRE(desc[i].bpp != 2 || ((uintptr_t)desc[i].src & 1) == 0, "fd_png_enc_filter: descriptor %d: src of a 16-bit frame is odd", i);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(work, desc, (size_t)N * sizeof(fd_png_enc_desc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync((unsigned char*)work + sz.stat_off, 0, (size_t)sz.stat_bytes, st);
    FD_REQUIRE(e == hipSuccess, "fd_png_enc_filter: copy or clear failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_png_enc_filter, dim3((unsigned)sz.groups), dim3(64 * GROUP), 0, st, (unsigned char*)work, N, sz.stat_off, sz.blocks);
    FD_LAUNCH_CHECK("k_png_enc_filter");
    return 0;
}

extern "C" int fd_png_enc_emit(void* work, long work_bytes, const fd_png_enc_desc* desc, int N, const fd_png_enc_block* blocks,
                               unsigned char* out, long out_bytes, void* stream) {
    FD_REQUIRE(work && desc && blocks && out && ((uintptr_t)work & 15) == 0 && ((uintptr_t)out & 3) == 0 && out_bytes >= 8 && out_bytes % 4 == 0,
               "fd_png_enc_emit: bad args (work 16-byte aligned; out 4-byte aligned, out_bytes a multiple of 4)");
    fd_png_enc_sizes sz;
    char err[fdpngenc::ERR_LEN] = "";
    FD_REQUIRE(fdpngenc::check_layout(desc, N, work_bytes, &sz, err) == 0, "fd_png_enc_emit: %s", err);
    for (int i = 0; i < N; ++i) {
        const fd_png_enc_desc& d = desc[i];
        FD_REQUIRE(d.stream_bits >= 0 && d.out_bytes == fdpngenc::FILE_FIXED + 2 + (d.stream_bits + 7) / 8 + 4,
                   "fd_png_enc_emit: descriptor %d: out_bytes is not what fd_png_enc_plan wrote", i);
        FD_REQUIRE(d.out_off >= 0 && d.out_bytes <= out_bytes - 4 && d.out_off <= out_bytes - 4 - d.out_bytes,
                   "fd_png_enc_emit: descriptor %d: the file leaves out", i);
        const int nb = (d.height + ROWS - 1) / ROWS;
        for (int k = 0; k < nb; ++k) {
            const fd_png_enc_block& b = blocks[d.first_block + k];
            FD_REQUIRE(b.header_bits <= 32u * FD_PNG_ENC_HEADER_WORDS && b.header_bits <= b.bits && b.bits <= (unsigned long long)d.stream_bits &&
                           b.bit_off <= (unsigned long long)d.stream_bits - b.bits,
                       "fd_png_enc_emit: block %d of descriptor %d leaves the frame's stream", k, i);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(work, desc, (size_t)N * sizeof(fd_png_enc_desc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync((unsigned char*)work + sz.table_off, blocks, (size_t)sz.blocks * sizeof(fd_png_enc_block), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(out, 0, (size_t)out_bytes, st);
    FD_REQUIRE(e == hipSuccess, "fd_png_enc_emit: copy or clear failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_png_enc_rowbits, dim3((unsigned)sz.groups), dim3(64 * GROUP), 0, st, (unsigned char*)work, N, sz.rowbits_off, sz.table_off);
    FD_LAUNCH_CHECK("k_png_enc_rowbits");
    hipLaunchKernelGGL(k_png_enc_emit, dim3((unsigned)sz.groups), dim3(64 * GROUP), 0, st, (const unsigned char*)work, N, sz.rowbits_off,
                       sz.table_off, (unsigned*)out, out_bytes);
    FD_LAUNCH_CHECK("k_png_enc_emit");
    return 0;
}
