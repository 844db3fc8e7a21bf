// Device side of the read collapse of the reference's scripts/process-reads-fasta.py:60-80 (mirp_collapse_reads): every line of an uncollapsed
// FASTA file that does not start with '>' is a read (the line after str.strip()); identical reads are counted, and every distinct read is written as
// ">" + prefix + "_r" + A + "_x" + B + "\n" + read + "\n" with A = 0, 1, ... in order of first occurrence (Python 3 dict order), B = its count.
//
// The file is uploaded once and stays resident; offsets are 64-bit throughout.
//   split   reads_count_kernel    ends of lines under the universal-newline rule (\n, \r\n, a lone \r) per 4 KiB tile, 16 B per lane; bytes >= 0x80
//           launch_excl_scan      tile bases
//           reads_starts_kernel   line start offsets (block scan of the per-lane counts)
//           reads_flag_kernel     read (raw first byte != '>') or header; launch_excl_scan gives the read index
//   hash    reads_hash_kernel     strip over the ASCII whitespace set, 64-bit hash of length + bytes (dwords out of 16-byte loads)
//           mirp_device_sort_hashes  stable LSD radix sort of (hash, read index) by hash (sort_kernels.hip): within a hash run the reads stay in
//                                 file order, so a run's head is its first occurrence
//   verify  reads_runhead_kernel / reads_runfirst_kernel   runs of equal hash and their first element
//           reads_verify_kernel   every read against the head of its run, byte for byte in dwords; a mismatch marks the run as a hash collision
//           reads_tally_kernel    verified runs: count at the head's read index.  Collided runs go to the host, which groups them by their bytes
//                                 (exactness never depends on the hash), and reads_fix_kernel scatters its counts the same way
//           launch_excl_scan      of the head flags in file order = A
//   emit    reads_size_kernel, launch_excl_scan, reads_emit_kernel   record sizes, their offsets, the text; one download
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>
#include "mirp_ctx.h"

namespace mirp {

#define RD_NT 256
#define RD_TILE (RD_NT * 16)     // bytes per workgroup of the split kernels
#define RD_PAD 64                // zero bytes behind the text: the 16-byte loads of a line's last bytes read up to 32 bytes past its end

__device__ __forceinline__ bool rd_ws(unsigned ch) { return ch == 32u || (ch >= 9u && ch <= 13u) || (ch >= 0x1cu && ch <= 0x1fu); }   // str.strip(), ASCII

// 16-bit mask of the line ends among the 16 bytes at `base` (bit j: byte base + j ends a line that is followed by another line) and the
// smallest offset of a byte >= 0x80 among them (-1: none)
__device__ __forceinline__ unsigned rd_ends(const unsigned char* __restrict__ text, long long n, long long base, long long* bad) {
    const uint4 v = *(const uint4*)(text + base);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    const unsigned next = text[base + 16];
    unsigned mask = 0;
    *bad = -1;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const unsigned ch = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        const unsigned nx = j < 15 ? (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u : next;
        const long long q = base + j;
        if (q + 1 < n && (ch == 10u || (ch == 13u && nx != 10u))) mask |= 1u << j;
        if (q < n && ch >= 0x80u && *bad < 0) *bad = q;
    }
    return mask;
}

__global__ void __launch_bounds__(RD_NT) reads_count_kernel(const unsigned char* __restrict__ text, long long n, int* __restrict__ tile_cnt,
                                                            unsigned long long* __restrict__ first_bad) {
    __shared__ int part[RD_NT / 64];
    const long long base = (long long)blockIdx.x * RD_TILE + threadIdx.x * 16;
    int cnt = 0;
    if (base < n) {
        long long bad;
        cnt = __popc(rd_ends(text, n, base, &bad));
        if (bad >= 0) atomicMin(first_bad, (unsigned long long)bad);
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// starts[1 + k] = offset behind the k-th line end (starts[0] = 0 and starts[n_lines] = n are set by the host)
__global__ void __launch_bounds__(RD_NT) reads_starts_kernel(const unsigned char* __restrict__ text, long long n, const long long* __restrict__ tile_base,
                                                             long long* __restrict__ starts) {
    __shared__ int wsum[RD_NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * RD_TILE + threadIdx.x * 16;
    unsigned mask = 0;
    if (base < n) { long long bad; mask = rd_ends(text, n, base, &bad); }
    const int cnt = __popc(mask);
    int inc = cnt;
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long k = tile_base[blockIdx.x] + inc - cnt;
    for (int w = 0; w < wave; w++) k += wsum[w];
    while (mask) {
        const int j = __ffs(mask) - 1;
        mask &= mask - 1;
        starts[1 + k++] = base + j + 1;
    }
}

__global__ void reads_flag_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ starts, long long n_lines, int* __restrict__ is_read) {
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n_lines; k += (long long)gridDim.x * blockDim.x)
        is_read[k] = text[starts[k]] != '>';
}

// The 16 bytes text[b + j, b + j + 16) as four dwords (b arbitrary, j a multiple of 16): two aligned 16-byte loads and a funnel shift
__device__ __forceinline__ void rd_content16(const uint4* __restrict__ t16, long long b, long long j, unsigned d[4]) {
    const long long p = b + j;
    const uint4 v0 = t16[p >> 4], v1 = t16[(p >> 4) + 1];
    const int o = (int)(p & 15), s2 = o & 8, s1 = o & 4, sb = o & 3;
    // shift the eight dwords down by (o >> 2) with selects (no indexed register array)
    const unsigned t0 = s2 ? v0.z : v0.x, t1 = s2 ? v0.w : v0.y, t2 = s2 ? v1.x : v0.z, t3 = s2 ? v1.y : v0.w, t4 = s2 ? v1.z : v1.x, t5 = s2 ? v1.w : v1.y;
    const unsigned u0 = s1 ? t1 : t0, u1 = s1 ? t2 : t1, u2 = s1 ? t3 : t2, u3 = s1 ? t4 : t3, u4 = s1 ? t5 : t4;
    d[0] = __builtin_amdgcn_alignbyte(u1, u0, sb);
    d[1] = __builtin_amdgcn_alignbyte(u2, u1, sb);
    d[2] = __builtin_amdgcn_alignbyte(u3, u2, sb);
    d[3] = __builtin_amdgcn_alignbyte(u4, u3, sb);
}
// keep the bytes of dword i of a 16-byte step that lie before the end (valid = bytes of the step inside the read)
__device__ __forceinline__ unsigned rd_keep(unsigned d, long long valid, int i) {
    const long long nb = valid - 4 * i;
    return nb >= 4 ? d : nb <= 0 ? 0u : d & ((1u << (8 * (int)nb)) - 1u);
}

__device__ __forceinline__ unsigned long long rd_hash(const uint4* __restrict__ t16, long long b, long long len) {
    unsigned long long h = 0x243f6a8885a308d3ull;
    for (long long j = 0; j < len; j += 16) {
        unsigned d[4];
        rd_content16(t16, b, j, d);
        const long long valid = len - j;
        const unsigned long long w0 = rd_keep(d[0], valid, 0) | ((unsigned long long)rd_keep(d[1], valid, 1) << 32);
        const unsigned long long w1 = rd_keep(d[2], valid, 2) | ((unsigned long long)rd_keep(d[3], valid, 3) << 32);
        h = (h ^ w0) * 0xff51afd7ed558ccdull; h ^= h >> 32;
        h = (h ^ w1) * 0xc4ceb9fe1a85ec53ull; h ^= h >> 29;
    }
    h ^= (unsigned long long)len * 0x9e3779b97f4a7c15ull;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}

// per read r (file order): stripped span [b, e) and the (hash, r) record; max_len[0] = longest read
__global__ void reads_hash_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ starts, long long n_lines, const int* __restrict__ is_read,
                                  const long long* __restrict__ rscan, unsigned long long hmask, longlong2* __restrict__ span, MirpHashRec* __restrict__ rec,
                                  unsigned long long* __restrict__ max_len) {
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n_lines; k += (long long)gridDim.x * blockDim.x) {
        if (!is_read[k]) continue;
        long long b = starts[k], e = starts[k + 1];
        while (b < e && rd_ws(text[b])) b++;
        while (e > b && rd_ws(text[e - 1])) e--;
        const long long r = rscan[k];
        span[r] = make_longlong2(b, e);
        rec[r] = MirpHashRec{rd_hash((const uint4*)text, b, e - b) & hmask, (unsigned)r, 0u};
        if (e - b > 0) atomicMax(max_len, (unsigned long long)(e - b));
    }
}

__global__ void reads_runhead_kernel(const MirpHashRec* __restrict__ rec, long long n, int* __restrict__ head) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        head[i] = i == 0 || rec[i].hash != rec[i - 1].hash;
}
// first[run] = sorted position of the run's first read; first[n_runs] = n
__global__ void reads_runfirst_kernel(const int* __restrict__ head, const long long* __restrict__ hscan, long long n, long long* __restrict__ first) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (head[i]) first[hscan[i]] = i;
        if (i == n - 1) first[hscan[i] + head[i]] = n;
    }
}

__device__ __forceinline__ bool rd_same(const uint4* __restrict__ t16, longlong2 x, longlong2 y) {
    const long long len = x.y - x.x;
    if (y.y - y.x != len) return false;
    for (long long j = 0; j < len; j += 16) {
        unsigned a[4], b[4];
        rd_content16(t16, x.x, j, a);
        rd_content16(t16, y.x, j, b);
        const long long valid = len - j;
        unsigned diff = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) diff |= rd_keep(a[i] ^ b[i], valid, i);
        if (diff) return false;
    }
    return true;
}

__global__ void reads_verify_kernel(const unsigned char* __restrict__ text, const MirpHashRec* __restrict__ rec, const longlong2* __restrict__ span,
                                    const int* __restrict__ head, const long long* __restrict__ hscan, const long long* __restrict__ first, long long n,
                                    int* __restrict__ bad) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long run = hscan[i] + head[i] - 1, h = first[run];
        if (i != h && !rd_same((const uint4*)text, span[rec[i].idx], span[rec[h].idx])) bad[run] = 1;
    }
}

// verified runs: count and head flag at the first occurrence's read index; in_bad[i] = read i (sorted) lies in a collided run
__global__ void reads_tally_kernel(const MirpHashRec* __restrict__ rec, const int* __restrict__ head, const long long* __restrict__ hscan,
                                   const long long* __restrict__ first, const int* __restrict__ bad, long long n, int* __restrict__ cnt,
                                   int* __restrict__ is_first, int* __restrict__ in_bad) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long run = hscan[i] + head[i] - 1;
        const int b = bad[run];
        in_bad[i] = b;
        if (head[i] && !b) {
            const unsigned idx = rec[i].idx;
            cnt[idx] = (int)(first[run + 1] - i);
            is_first[idx] = 1;
        }
    }
}

struct RdCollide { unsigned long long hash; long long idx, b, e; };
__global__ void reads_collide_kernel(const MirpHashRec* __restrict__ rec, const longlong2* __restrict__ span, const int* __restrict__ in_bad,
                                     const long long* __restrict__ bscan, long long n, RdCollide* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        if (in_bad[i]) {
            const unsigned idx = rec[i].idx;
            out[bscan[i]] = RdCollide{rec[i].hash, (long long)idx, span[idx].x, span[idx].y};
        }
}
// the host's groups of the collided runs: (first occurrence, count) pairs
__global__ void reads_fix_kernel(const longlong2* __restrict__ groups, long long n, int* __restrict__ cnt, int* __restrict__ is_first) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        cnt[groups[i].x] = (int)groups[i].y;
        is_first[groups[i].x] = 1;
    }
}

__device__ __forceinline__ int rd_digits(long long v) { int d = 1; while (v >= 10) { v /= 10; d++; } return d; }

__global__ void reads_size_kernel(const int* __restrict__ is_first, const long long* __restrict__ rank, const int* __restrict__ cnt,
                                  const longlong2* __restrict__ span, long long n, int prefix_len, int* __restrict__ size) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x)
        size[r] = is_first[r] ? 1 + prefix_len + 2 + rd_digits(rank[r]) + 2 + rd_digits(cnt[r]) + 1 + (int)(span[r].y - span[r].x) + 1 : 0;
}

__device__ __forceinline__ char* rd_put_num(char* p, long long v) {
    const int d = rd_digits(v);
    for (int k = d - 1; k >= 0; k--) { p[k] = (char)('0' + v % 10); v /= 10; }
    return p + d;
}
__global__ void reads_emit_kernel(const unsigned char* __restrict__ text, const int* __restrict__ is_first, const long long* __restrict__ rank,
                                  const int* __restrict__ cnt, const longlong2* __restrict__ span, const long long* __restrict__ off, long long n,
                                  const char* __restrict__ prefix, int prefix_len, char* __restrict__ out) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        if (!is_first[r]) continue;
        char* p = out + off[r];
        *p++ = '>';
        for (int k = 0; k < prefix_len; k++) *p++ = prefix[k];
        *p++ = '_'; *p++ = 'r';
        p = rd_put_num(p, rank[r]);
        *p++ = '_'; *p++ = 'x';
        p = rd_put_num(p, cnt[r]);
        *p++ = '\n';
        for (long long q = span[r].x; q < span[r].y; q++) *p++ = (char)text[q];
        *p = '\n';
    }
}

}  // namespace mirp

static inline int rd_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

// The collapse of one file held in host memory.  seconds[0] gains the upload, [1] .. [4] are split, hash + sort, verify + rank, emit + download.
// -9 with *bad_offset set: a byte >= 0x80 (the caller names the file).
int mirp_device_collapse_reads(mirp_ctx* c, const char* text, long long n, const char* prefix, int hash_bits, char** out, long long* out_len,
                               long long* n_reads, long long* n_unique, long long* bad_offset, double seconds[6]) {
    using namespace mirp;
    *out = nullptr; *out_len = 0; *n_reads = 0; *n_unique = 0; *bad_offset = -1;
    c->last_collapse_collisions = 0;
    hipStream_t st = c->stream;
    const int plen = (int)std::strlen(prefix);
    double t = mirp::now();
    if (c->r_text.ensure((size_t)n + RD_PAD) || c->r_small.ensure(64 + (size_t)plen)) return fail(c, -6, "device allocation failed (collapse: text)");
    unsigned char* d_text = (unsigned char*)c->r_text.p;
    unsigned long long* d_small = (unsigned long long*)c->r_small.p;     // [0] first byte >= 0x80, [1] longest read, then the prefix
    char* d_prefix = (char*)c->r_small.p + 64;
    if (n > 0) HIPCHK(c, hipMemcpy(d_text, text, (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(d_text + n, 0, RD_PAD, st));
    const unsigned long long init[2] = {~0ull, 0ull};
    HIPCHK(c, hipMemcpyAsync(d_small, init, sizeof init, hipMemcpyHostToDevice, st));
    if (plen) HIPCHK(c, hipMemcpyAsync(d_prefix, prefix, (size_t)plen, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] += mirp::now() - t;

    // ---- split
    t = mirp::now();
    long long n_lines = 0, R = 0;
    if (n > 0) {
        if (int rc = mirp_device_split_lines(c, d_text, n, 0x7fffffffll, c->r_bcnt, c->r_bscan, c->r_starts, d_small, &n_lines, bad_offset)) return rc;
        if (c->r_flag.ensure(4 * (size_t)n_lines) || c->r_fscan.ensure(8 * (size_t)(n_lines + 1))) return fail(c, -6, "device allocation failed (collapse: lines)");
        const long long* d_starts = (const long long*)c->r_starts.p;
        hipLaunchKernelGGL(reads_flag_kernel, dim3(rd_grid(n_lines)), dim3(256), 0, st, (const unsigned char*)d_text, (const long long*)d_starts, n_lines, (int*)c->r_flag.p);
        launch_excl_scan(st, (const int*)c->r_flag.p, (long long*)c->r_fscan.p, n_lines);
        HIPCHK(c, hipMemcpyAsync(&R, (long long*)c->r_fscan.p + n_lines, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
    }
    seconds[1] += mirp::now() - t;
    *n_reads = R;
    if (R == 0) return 0;

    // ---- hash + sort
    t = mirp::now();
    if (c->r_span.ensure(16 * (size_t)R) || c->r_rec.ensure(sizeof(MirpHashRec) * (size_t)R) || c->r_rectmp.ensure(sizeof(MirpHashRec) * (size_t)R))
        return fail(c, -6, "device allocation failed (collapse: reads)");
    longlong2* d_span = (longlong2*)c->r_span.p;
    MirpHashRec* d_rec = (MirpHashRec*)c->r_rec.p;
    const unsigned long long hmask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1ull;
    hipLaunchKernelGGL(reads_hash_kernel, dim3(rd_grid(n_lines)), dim3(256), 0, st, (const unsigned char*)d_text, (const long long*)c->r_starts.p, n_lines,
                       (const int*)c->r_flag.p, (const long long*)c->r_fscan.p, hmask, d_span, d_rec, d_small + 1);
    unsigned long long max_len = 0;
    HIPCHK(c, hipMemcpyAsync(&max_len, d_small + 1, 8, hipMemcpyDeviceToHost, st));
    if (int rc = mirp_device_sort_hashes(c, d_rec, (MirpHashRec*)c->r_rectmp.p, R, (hash_bits + 7) / 8 * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    if (max_len > (1ull << 30)) return fail(c, -5, "a read longer than 2^30 bytes");
    seconds[2] += mirp::now() - t;

    // ---- verify + rank
    t = mirp::now();
    if (c->r_rscan.ensure(8 * (size_t)(R + 1)) || c->r_first.ensure(8 * (size_t)(R + 1)) || c->r_bad.ensure(4 * (size_t)R) || c->r_cnt.ensure(4 * (size_t)R) ||
        c->r_isfirst.ensure(4 * (size_t)R) || c->r_inbad.ensure(4 * (size_t)R) || c->r_rank.ensure(8 * (size_t)(R + 1)))
        return fail(c, -6, "device allocation failed (collapse: runs)");
    int* d_head = (int*)c->r_flag.p;              // the line flags are done with: run heads in sorted order (R <= n_lines)
    long long* d_hscan = (long long*)c->r_rscan.p;
    long long* d_first = (long long*)c->r_first.p;
    int* d_bad = (int*)c->r_bad.p;
    int* d_cnt = (int*)c->r_cnt.p;
    int* d_isfirst = (int*)c->r_isfirst.p;
    int* d_inbad = (int*)c->r_inbad.p;
    HIPCHK(c, hipMemsetAsync(d_bad, 0, 4 * (size_t)R, st));
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 4 * (size_t)R, st));
    HIPCHK(c, hipMemsetAsync(d_isfirst, 0, 4 * (size_t)R, st));
    const int g = rd_grid(R);
    hipLaunchKernelGGL(reads_runhead_kernel, dim3(g), dim3(256), 0, st, (const MirpHashRec*)d_rec, R, d_head);
    launch_excl_scan(st, d_head, d_hscan, R);
    hipLaunchKernelGGL(reads_runfirst_kernel, dim3(g), dim3(256), 0, st, (const int*)d_head, (const long long*)d_hscan, R, d_first);
    hipLaunchKernelGGL(reads_verify_kernel, dim3(g), dim3(256), 0, st, (const unsigned char*)d_text, (const MirpHashRec*)d_rec, (const longlong2*)d_span,
                       (const int*)d_head, (const long long*)d_hscan, (const long long*)d_first, R, d_bad);
    hipLaunchKernelGGL(reads_tally_kernel, dim3(g), dim3(256), 0, st, (const MirpHashRec*)d_rec, (const int*)d_head, (const long long*)d_hscan,
                       (const long long*)d_first, (const int*)d_bad, R, d_cnt, d_isfirst, d_inbad);
    long long* d_bscan = (long long*)c->r_fscan.p;     // the read-index scan is done with (R + 1 <= n_lines + 1)
    launch_excl_scan(st, (const int*)d_inbad, d_bscan, R);
    long long n_bad = 0;
    HIPCHK(c, hipMemcpyAsync(&n_bad, d_bscan + R, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (n_bad > 0) {
        // hash collisions: the reads of the collided runs, grouped here by their bytes; a run is in file order (stable sort), so the first read of
        // a group is its first occurrence
        TmpDevice T;
        RdCollide* d_coll = (RdCollide*)T.get(sizeof(RdCollide) * (size_t)n_bad);
        if (!d_coll) return fail(c, -6, "device allocation failed (collapse: collisions)");
        hipLaunchKernelGGL(reads_collide_kernel, dim3(g), dim3(256), 0, st, (const MirpHashRec*)d_rec, (const longlong2*)d_span, (const int*)d_inbad,
                           (const long long*)d_bscan, R, d_coll);
        std::vector<RdCollide> coll((size_t)n_bad);
        HIPCHK(c, hipMemcpyAsync(coll.data(), d_coll, sizeof(RdCollide) * (size_t)n_bad, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        std::vector<longlong2> groups;
        std::unordered_map<std::string_view, size_t> seen;
        for (size_t a = 0; a < coll.size();) {
            size_t z = a;
            while (z < coll.size() && coll[z].hash == coll[a].hash) z++;
            seen.clear();
            for (size_t i = a; i < z; i++) {
                const std::string_view key(text + coll[i].b, (size_t)(coll[i].e - coll[i].b));
                auto it = seen.find(key);
                if (it == seen.end()) { seen.emplace(key, groups.size()); groups.push_back(make_longlong2(coll[i].idx, 1)); }
                else groups[it->second].y++;
            }
            a = z;
        }
        longlong2* d_groups = (longlong2*)T.get(sizeof(longlong2) * groups.size());
        if (!d_groups) return fail(c, -6, "device allocation failed (collapse: collisions)");
        HIPCHK(c, hipMemcpyAsync(d_groups, groups.data(), sizeof(longlong2) * groups.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(reads_fix_kernel, dim3(rd_grid((long long)groups.size())), dim3(256), 0, st, (const longlong2*)d_groups, (long long)groups.size(), d_cnt, d_isfirst);
        HIPCHK(c, hipStreamSynchronize(st));
        c->last_collapse_collisions = n_bad;
    }
    long long* d_rank = (long long*)c->r_rank.p;
    launch_excl_scan(st, (const int*)d_isfirst, d_rank, R);
    long long U = 0;
    HIPCHK(c, hipMemcpyAsync(&U, d_rank + R, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    seconds[3] += mirp::now() - t;

    // ---- emit + download
    t = mirp::now();
    int* d_size = d_head;                     // run heads are done with
    long long* d_off = d_bscan;
    hipLaunchKernelGGL(reads_size_kernel, dim3(g), dim3(256), 0, st, (const int*)d_isfirst, (const long long*)d_rank, (const int*)d_cnt, (const longlong2*)d_span, R,
                       plen, d_size);
    launch_excl_scan(st, (const int*)d_size, d_off, R);
    long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_off + R, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (c->r_out.ensure((size_t)total + 16)) return fail(c, -6, "device allocation failed (collapse: output)");
    hipLaunchKernelGGL(reads_emit_kernel, dim3(g), dim3(256), 0, st, (const unsigned char*)d_text, (const int*)d_isfirst, (const long long*)d_rank, (const int*)d_cnt,
                       (const longlong2*)d_span, (const long long*)d_off, R, (const char*)d_prefix, plen, (char*)c->r_out.p);
    char* h_out = (char*)std::malloc((size_t)total + 1);
    if (!h_out) return fail(c, -7, "host allocation failed (collapse: output)");
    if (total > 0) {
        const hipError_t e = hipMemcpyAsync(h_out, c->r_out.p, (size_t)total, hipMemcpyDeviceToHost, st);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(st) : e;
        if (e2 != hipSuccess) { std::free(h_out); return fail(c, -2, std::string("collapse download: ") + hipGetErrorString(e2)); }
    }
    const hipError_t e3 = hipGetLastError();
    if (e3 != hipSuccess) { std::free(h_out); return fail(c, -2, std::string("collapse: ") + hipGetErrorString(e3)); }
    seconds[4] += mirp::now() - t;
    *out = h_out;
    *out_len = total;
    *n_unique = U;
    return 0;
}

// The split phase of the collapse and the trim (trim_kernels.hip) on an uploaded text: d_text holds n bytes plus RD_PAD zero bytes.
// starts[0 .. n_lines] as reads_starts_kernel leaves them (starts[n_lines] = n).  -9 with *bad_offset set: a byte >= 0x80; -5: more than
// max_lines lines.  n > 0.
int mirp_device_split_lines(mirp_ctx* c, const unsigned char* d_text, long long n, long long max_lines, DevBuf& tile_cnt, DevBuf& tile_scan, DevBuf& starts,
                            unsigned long long* d_first_bad, long long* n_lines, long long* bad_offset) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long tiles = (n + RD_TILE - 1) / RD_TILE;
    if (tile_cnt.ensure(4 * (size_t)tiles) || tile_scan.ensure(8 * (size_t)(tiles + 1))) return fail(c, -6, "device allocation failed (split: tiles)");
    const unsigned long long none = ~0ull;
    HIPCHK(c, hipMemcpyAsync(d_first_bad, &none, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(reads_count_kernel, dim3((unsigned)tiles), dim3(RD_NT), 0, st, d_text, n, (int*)tile_cnt.p, d_first_bad);
    launch_excl_scan(st, (const int*)tile_cnt.p, (long long*)tile_scan.p, tiles);
    unsigned long long first_bad = 0;
    long long ends = 0;
    HIPCHK(c, hipMemcpyAsync(&first_bad, d_first_bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&ends, (long long*)tile_scan.p + tiles, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (first_bad != ~0ull) { *bad_offset = (long long)first_bad; return fail(c, -9, "byte outside ASCII"); }
    *n_lines = ends + 1;
    if (*n_lines > max_lines) return fail(c, -5, "more than 2^31 - 1 lines in one file");
    if (starts.ensure(8 * (size_t)(*n_lines + 1))) return fail(c, -6, "device allocation failed (split: lines)");
    long long* d_starts = (long long*)starts.p;
    const long long edge[2] = {0, n};
    HIPCHK(c, hipMemcpyAsync(d_starts, &edge[0], 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_starts + *n_lines, &edge[1], 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(reads_starts_kernel, dim3((unsigned)tiles), dim3(RD_NT), 0, st, d_text, n, (const long long*)tile_scan.p, d_starts);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return 0;
}
