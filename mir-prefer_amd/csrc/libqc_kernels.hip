// Device side of the library profile (mirp_libqc_reads): the 3' adapter of a raw library, found from its reads, and three tables.
//
// The upload, the line split, the records and the adapter scan are the trim's (mirp_device_trim_parse, mirp_device_trim_cut; trim_kernels.hip).
//   k-mers   libqc_kmer_kernel    one lane per sampled read: the rolling 12-mer code over its first 64 bases; at every base the equal codes of a
//                                 wave are merged into one atomic on the 4^12 32-bit counters (cl_wave_count32)
//   adapter  libqc_seed_kernel    the eligible 12-mer with the largest counter, ties to the smallest code: atomicMax of (count << 24 | ~code)
//            libqc_walk_kernel    one lane: the left and the right walk, four counters per step
//   tables   libqc_cycles_kernel  raw lengths and per-cycle base classes / quality sums, in LDS per workgroup: the classes of a cycle by ballots,
//                                 the quality sum by a wave reduction, so that a cycle costs a wave six LDS atomics
//            libqc_insert_kernel  the trim kernel's final lengths by the read's first base, in LDS per workgroup
// Every counter is an integer sum, so no output depends on scheduling.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include "mirp_ctx.h"
#include "wave_atomic.h"

namespace mirp {

#define LQ_K 12                    // k-mer length
#define LQ_W 64                    // bases of a read that are counted
#define LQ_CODES (1 << 24)         // 4^12
#define LQ_LIMIT 1024              // longest read (TR_LIMIT)
#define LQ_LEFT_CAP 1024           // length at which the left walk stops
#define LQ_RIGHT_CAP (1024 + 64)   // and the right walk
#define LQ_MIN_COUNT 16
#define LQ_NT 256                  // threads per workgroup of the table kernels
// q_hist, 64-bit: raw_len[1025], cycles[1024][6], insert[1025][6], dimers
#define LQ_H_LEN 0
#define LQ_H_CYC (LQ_LIMIT + 1)
#define LQ_H_INS (LQ_H_CYC + LQ_LIMIT * 6)
#define LQ_H_DIM (LQ_H_INS + (LQ_LIMIT + 1) * 6)
#define LQ_H_N (LQ_H_DIM + 1)
// q_found, bytes: the seed key, the found record, the walk's bases (the seed at LQ_LEFT_CAP - LQ_K, so that both walks have room)
#define LQ_F_KEY 0
#define LQ_F_REC 8
#define LQ_F_S 128
#define LQ_F_BYTES (LQ_F_S + LQ_LEFT_CAP - LQ_K + LQ_RIGHT_CAP + 8)

// class of an upper-cased base: A 0, C 1, G 2, T 3, anything else 4
__device__ __forceinline__ int lq_class(unsigned u) {
    const unsigned x = (u >> 1) & 3u;          // A 0, C 1, T 2, G 3
    return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? (int)(x ^ (x >> 1)) : 4;
}

__device__ __forceinline__ int lq_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// read r < Rs: every 12-mer of ACGT within its first LQ_W bases adds 1 to table[code]; a read with len < 0 (a refused record) adds nothing
__global__ void __launch_bounds__(LQ_NT) libqc_kmer_kernel(const unsigned char* __restrict__ base, const long long* __restrict__ src, const int* __restrict__ len,
                                                           long long Rs, unsigned* __restrict__ table) {
    const long long r = (long long)blockIdx.x * LQ_NT + threadIdx.x;
    const int nn = r < Rs ? min(len[r], LQ_W) : 0;
    const unsigned char* s = base + (nn > 0 ? src[r] : 0);
    const int wmax = lq_wave_max(nn);
    unsigned code = 0;
    int run = 0;
    for (int j = 0; j < wmax; j++) {
        int slot = -1;
        if (j < nn) {
            const int cl = lq_class(s[j] & 0xdfu);
            code = ((code << 2) | (unsigned)(cl & 3)) & (LQ_CODES - 1);
            run = cl < 4 ? run + 1 : 0;
            if (run >= LQ_K) slot = (int)code;
        }
        cl_wave_count32(table, slot);
    }
}

// a 12-mer is eligible when no base occurs in it more than 6 times
__device__ __forceinline__ bool lq_eligible(unsigned code) {
    const unsigned M = 0x555555u, lo = code & M, hi = (code >> 1) & M;
    return __popc(hi & lo) <= 6 && __popc(hi & ~lo) <= 6 && __popc(~hi & lo) <= 6 && __popc(~hi & ~lo & M) <= 6;
}

// *key = max over the eligible codes of (count << 24 | (4^12 - 1 - code)): the largest count, ties to the smallest code; *key is 0 before
__global__ void __launch_bounds__(256) libqc_seed_kernel(const unsigned* __restrict__ table, unsigned long long* __restrict__ key) {
    unsigned long long best = 0;
    for (unsigned c = blockIdx.x * blockDim.x + threadIdx.x; c < LQ_CODES; c += gridDim.x * blockDim.x)
        if (lq_eligible(c)) {
            const unsigned long long k = ((unsigned long long)table[c] << 24) | (unsigned long long)(LQ_CODES - 1 - c);
            best = k > best ? k : best;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(best, o);
        best = y > best ? y : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(key, best);
}

// the step of both walks: the four counters of the 12-mers `stem | b << shift`; -> the base to add, or -1 support, -2 purity
__device__ __forceinline__ int lq_step(const unsigned* __restrict__ table, unsigned stem, int shift, unsigned long long minc) {
    unsigned long long m = 0, t = 0;
    int bb = 0;
    for (int b = 0; b < 4; b++) {
        const unsigned long long cb = table[stem | ((unsigned)b << shift)];
        t += cb;
        if (cb > m) { m = cb; bb = b; }
    }
    if (m < minc) return -1;
    if (5 * m < 4 * t) return -2;
    return bb;
}

// one lane.  s = bytes for the walk's bases (LQ_F_S); f is written whole
__global__ void libqc_walk_kernel(const unsigned* __restrict__ table, long long R, const unsigned long long* __restrict__ key, MirpLibqcFound* __restrict__ f,
                                  unsigned char* __restrict__ s) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long k = *key;
    const unsigned long long count = k >> 24;
    const unsigned seed = (unsigned)(LQ_CODES - 1) - (unsigned)(k & (LQ_CODES - 1));
    for (int i = 0; i < 64; i++) f->adapter[i] = 0;
    f->adapter_len = 0;
    f->status = MIRP_LIBQC_NONE;
    f->seed_code = (int)seed;
    f->left_steps = 0;
    f->left_stop = 0;
    f->reserved = 0;
    f->seed_count = (long long)count;
    f->min_count = 0;
    if (count < LQ_MIN_COUNT || R == 0) return;
    const unsigned long long minc = count / 64 > LQ_MIN_COUNT ? count / 64 : LQ_MIN_COUNT;
    int lo = LQ_LEFT_CAP - LQ_K, hi = LQ_LEFT_CAP;
    for (int i = 0; i < LQ_K; i++) s[lo + i] = (unsigned char)((seed >> (2 * (LQ_K - 1 - i))) & 3u);
    unsigned cur = seed;
    int stop = 2;
    while (hi - lo < LQ_LEFT_CAP) {
        const int b = lq_step(table, cur >> 2, 22, minc);
        if (b < 0) { stop = b == -1 ? 1 : 0; break; }
        cur = (cur >> 2) | ((unsigned)b << 22);
        s[--lo] = (unsigned char)b;
    }
    const int steps = LQ_LEFT_CAP - LQ_K - lo;
    cur = seed;
    while (hi - lo < LQ_RIGHT_CAP) {
        const int b = lq_step(table, (cur << 2) & (LQ_CODES - 1), 0, minc);
        if (b < 0) break;
        cur = ((cur << 2) & (LQ_CODES - 1)) | (unsigned)b;
        s[hi++] = (unsigned char)b;
    }
    const int m = min(hi - lo, 64);
    for (int i = 0; i < m; i++) f->adapter[i] = "ACGT"[s[lo + i]];
    f->adapter_len = m;
    f->status = stop == 0 ? MIRP_LIBQC_OK : MIRP_LIBQC_UNSURE;
    f->left_steps = steps;
    f->left_stop = stop;
    f->min_count = (long long)minc;
}

// raw_len and cycles of all reads (every len >= 0: the refusals are behind).  A workgroup takes LQ_NT reads at a time, grid-strided, and keeps its
// counts in LDS: at most 2^31 / gridDim.x reads each, so 32 bits hold them when the grid has at least 64 workgroups per 2^31 reads.
__global__ void __launch_bounds__(LQ_NT) libqc_cycles_kernel(const unsigned char* __restrict__ base, const unsigned char* __restrict__ text,
                                                             const long long* __restrict__ src, const int* __restrict__ len, const long long* __restrict__ qual,
                                                             long long R, unsigned long long* __restrict__ hist) {
    __shared__ unsigned s_h[LQ_H_INS];                  // raw_len, then cycles
    for (int k = threadIdx.x; k < LQ_H_INS; k += LQ_NT) s_h[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const bool fq = qual != nullptr;
    for (long long r0 = (long long)blockIdx.x * LQ_NT; r0 < R; r0 += (long long)gridDim.x * LQ_NT) {
        const long long r = r0 + threadIdx.x;
        const int n = r < R ? len[r] : -1;
        const unsigned char* s = base + (n > 0 ? src[r] : 0);
        const unsigned char* q = text + (n > 0 && fq ? qual[r] : 0);
        cl_wave_count32(s_h + LQ_H_LEN, n);
        const int wmax = lq_wave_max(n);
        for (int i = 0; i < wmax; i++) {
            const int cl = i < n ? lq_class(s[i] & 0xdfu) : 5;
            int qs = i < n && fq ? (int)q[i] - 33 : 0;
            unsigned cnt = 0;
#pragma unroll
            for (int b = 0; b < 5; b++) {
                const unsigned long long bal = __ballot(cl == b);
                if (lane == b) cnt = (unsigned)__popcll(bal);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) qs += __shfl_xor(qs, o);
            if (lane == 5) cnt = (unsigned)qs;
            if (lane < 6 && cnt) atomicAdd(&s_h[LQ_H_CYC + i * 6 + lane], cnt);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < LQ_H_INS; k += LQ_NT)
        if (s_h[k]) atomicAdd(&hist[k], (unsigned long long)s_h[k]);
}

// insert[p][first base, total] of all reads from the trim kernel's final lengths, and the dimers: reads with bases that are cut at 0
__global__ void __launch_bounds__(LQ_NT) libqc_insert_kernel(const unsigned char* __restrict__ base, const long long* __restrict__ src, const int* __restrict__ len,
                                                             const int* __restrict__ flen, long long R, unsigned long long* __restrict__ hist) {
    __shared__ unsigned s_h[(LQ_LIMIT + 1) * 6 + 1];
    for (int k = threadIdx.x; k < (LQ_LIMIT + 1) * 6 + 1; k += LQ_NT) s_h[k] = 0;
    __syncthreads();
    for (long long r0 = (long long)blockIdx.x * LQ_NT; r0 < R; r0 += (long long)gridDim.x * LQ_NT) {
        const long long r = r0 + threadIdx.x;
        const int n = r < R ? len[r] : -1;
        const int p = n >= 0 ? flen[r] : -1;
        if (p >= 0 && p <= LQ_LIMIT) {
            const int cl = p == 0 ? 4 : lq_class(base[src[r]] & 0xdfu);
            atomicAdd(&s_h[p * 6 + cl], 1u);
            atomicAdd(&s_h[p * 6 + 5], 1u);
        }
        const unsigned long long dim = __ballot(p == 0 && n > 0);
        if ((threadIdx.x & 63) == 0 && dim) atomicAdd(&s_h[(LQ_LIMIT + 1) * 6], (unsigned)__popcll(dim));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (LQ_LIMIT + 1) * 6 + 1; k += LQ_NT)
        if (s_h[k]) atomicAdd(&hist[LQ_H_INS + k], (unsigned long long)s_h[k]);
}

}  // namespace mirp

static inline int lq_grid(long long R) {
    const long long g = (R + LQ_NT - 1) / LQ_NT;
    return (int)(g < 1 ? 1 : g > 1024 ? 1024 : g);
}

// The profile of one file held in host memory (mirp_libqc.cpp checks the arguments).  found, stats, the tables and seconds as mirp_libqc_reads;
// none of them is written on a refusal.
int mirp_device_libqc_reads(mirp_ctx* c, const char* text, long long n, const char* name, const MirpLibqcOpts& o, MirpLibqcFound* found, long long stats[4],
                            long long* raw_len, long long* cycles, long long* insert, double seconds[6]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    if (c->q_table.ensure(4 * (size_t)LQ_CODES) || c->q_found.ensure(LQ_F_BYTES) || c->q_hist.ensure(8 * (size_t)LQ_H_N))
        return fail(c, -6, "device allocation failed (libqc: tables)");
    unsigned* d_table = (unsigned*)c->q_table.p;
    unsigned char* d_found = (unsigned char*)c->q_found.p;
    unsigned long long* d_hist = (unsigned long long*)c->q_hist.p;
    HIPCHK(c, hipMemsetAsync(d_table, 0, 4 * (size_t)LQ_CODES, st));
    HIPCHK(c, hipMemsetAsync(d_found, 0, LQ_F_BYTES, st));
    HIPCHK(c, hipMemsetAsync(d_hist, 0, 8 * (size_t)LQ_H_N, st));
    double sec[6] = {0, 0, 0, 0, 0, 0};
    MirpTrimParsed p{};
    if (n > 0)
        if (int rc = mirp_device_trim_parse(c, text, n, name, 0, &p, sec)) return rc;
    const long long R = p.R, Rs = std::min<long long>(R, o.sample);
    const long long* d_src = (const long long*)c->t_src.p;
    const int* d_len = (const int*)c->t_len.p;

    // ---- k-mers + adapter
    double t = mirp::now();
    if (Rs > 0)
        hipLaunchKernelGGL(libqc_kmer_kernel, dim3((unsigned)((Rs + LQ_NT - 1) / LQ_NT)), dim3(LQ_NT), 0, st, p.d_base, d_src, d_len, Rs, d_table);
    hipLaunchKernelGGL(libqc_seed_kernel, dim3(1024), dim3(256), 0, st, (const unsigned*)d_table, (unsigned long long*)(d_found + LQ_F_KEY));
    hipLaunchKernelGGL(libqc_walk_kernel, dim3(1), dim3(64), 0, st, (const unsigned*)d_table, R, (const unsigned long long*)(d_found + LQ_F_KEY),
                       (MirpLibqcFound*)(d_found + LQ_F_REC), d_found + LQ_F_S);
    MirpLibqcFound f;
    HIPCHK(c, hipMemcpyAsync(&f, d_found + LQ_F_REC, sizeof f, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    sec[3] += mirp::now() - t;

    // ---- trim: the adapter step alone, which also sees the quality bytes
    t = mirp::now();
    MirpTrimOpts to{};
    to.adapter_len = o.adapter_len > 0 ? o.adapter_len : f.adapter_len;
    std::memcpy(to.adapter, o.adapter_len > 0 ? o.adapter : f.adapter, (size_t)to.adapter_len);
    to.error_permille = o.error_permille;
    to.min_overlap = std::min(o.min_overlap > 0 ? o.min_overlap : 3, to.adapter_len);
    unsigned long long res[9] = {~0ull, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n > 0)
        if (int rc = mirp_device_trim_cut(c, p, name, to, res)) return rc;
    sec[4] += mirp::now() - t;

    // ---- tables
    t = mirp::now();
    if (R > 0) {
        hipLaunchKernelGGL(libqc_cycles_kernel, dim3(lq_grid(R)), dim3(LQ_NT), 0, st, p.d_base, p.d_text, d_src, d_len,
                           p.fq ? (const long long*)c->t_qual.p : (const long long*)nullptr, R, d_hist);
        if (to.adapter_len > 0)
            hipLaunchKernelGGL(libqc_insert_kernel, dim3(lq_grid(R)), dim3(LQ_NT), 0, st, p.d_base, d_src, d_len, (const int*)c->t_flen.p, R, d_hist);
    }
    std::vector<unsigned long long> h(LQ_H_N);
    HIPCHK(c, hipMemcpyAsync(h.data(), d_hist, 8 * (size_t)LQ_H_N, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    sec[5] += mirp::now() - t;

    if (found) *found = f;
    if (stats) {
        stats[0] = R;
        stats[1] = Rs;
        stats[2] = to.adapter_len > 0 ? (long long)res[2] : 0;
        stats[3] = (long long)h[LQ_H_DIM];
    }
    if (raw_len) for (int i = 0; i <= LQ_LIMIT; i++) raw_len[i] = (long long)h[LQ_H_LEN + i];
    if (cycles) for (int i = 0; i < LQ_LIMIT * 6; i++) cycles[i] = (long long)h[LQ_H_CYC + i];
    if (insert) for (int i = 0; i < (LQ_LIMIT + 1) * 6; i++) insert[i] = (long long)h[LQ_H_INS + i];
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    c->t_paths[0] = (long long)res[7];
    c->t_paths[1] = (long long)res[8];
    return 0;
}

int mirp_device_libqc_table(mirp_ctx* c, unsigned* out) {
    HIPCHK(c, hipMemcpy(out, c->q_table.p, 4 * (size_t)LQ_CODES, hipMemcpyDeviceToHost));
    return 0;
}
