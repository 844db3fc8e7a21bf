// Device side of the 3' adapter and quality trimming of raw reads (mirp_trim_reads): FASTQ or FASTA in, one FASTA record per kept
// read out, in input order.
//
// The text is uploaded once; offsets are 64-bit throughout.
//   split    mirp_device_split_lines (reads_kernels.hip)  the collapse's line split: ends under the universal-newline rule, bytes >= 0x80, starts
//   records  FASTQ  trim_fastq_records_kernel   lines 4r .. 4r + 3 of read r: the '@' / '+' roles, stripped sequence and quality, the name; the first
//                                               bad (record, reason) is an atomicMin of (r << 3 | reason)
//            FASTA  trim_fasta_lines_kernel     header flag and stripped span of every line; launch_excl_scan of the flags (record index) and of the
//                                               stripped lengths (gather offsets: the lines of a record are consecutive, so its read is one range)
//                   trim_fasta_first_kernel, trim_fasta_records_kernel, trim_fasta_gather_kernel   read ranges, names, the contiguous read bytes
//   trim     trim_reads_kernel   one workgroup per TR_NT reads: their slab of text staged in LDS with 16-byte loads, then per read the quality check,
//                                the 3' quality trim and the adapter scan, bit-parallel on 2-bit codes (one xor / or / popcount per shift)
//   emit     trim_size_kernel, launch_excl_scan, trim_emit_kernel   record sizes, their offsets, the text; downloaded in pieces of at most 1 GiB
// On the host the first three steps are mirp_device_trim_parse and the fourth mirp_device_trim_cut, which the library profile (libqc_kernels.hip;
// DESIGN.md §35) calls as well; mirp_device_trim_reads calls both and emits.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include "mirp_ctx.h"

namespace mirp {

#define TR_PAD 64                // zero bytes behind the text and the gathered reads: the slab loads read up to 15 bytes past the last read
#define TR_LIMIT 1024            // longest read
#define TR_NAME_LIMIT (1 << 20)  // longest name
#define TR_NT 128                // reads per workgroup of the trim kernel
#define TR_SLAB 32768            // LDS bytes of a workgroup's slab; a larger slab (long reads) is read from global memory instead

// reasons of a refused record, in the order they are tested (the smallest of a record is reported)
enum { TR_E_AT = 0, TR_E_PLUS = 1, TR_E_LONG = 2, TR_E_QLEN = 3, TR_E_NAME = 4, TR_E_QBYTE = 5 };

struct TrimArgs {
    unsigned long long a0, a1;   // adapter bases 0..31 and 32..63, 2 bits each (tr_code)
    int m, e_pm, ovl, q, min_len, max_len, discard;
};

__device__ __forceinline__ bool tr_ws(unsigned ch) { return ch == 32u || (ch >= 9u && ch <= 13u) || (ch >= 0x1cu && ch <= 0x1fu); }   // str.strip(), ASCII

__device__ __forceinline__ void tr_err(unsigned long long* err, long long r, int why) { atomicMin(err, ((unsigned long long)r << 3) | (unsigned)why); }

// name = the header's bytes after its first, up to the first whitespace or the line's end e; its length, TR_NAME_LIMIT + 1 when longer
__device__ __forceinline__ int tr_name(const unsigned char* __restrict__ text, long long h, long long e) {
    long long q = h + 1;
    while (q < e && q - h - 1 <= TR_NAME_LIMIT && !tr_ws(text[q])) q++;
    return (int)(q - h - 1);
}

__device__ __forceinline__ void tr_strip(const unsigned char* __restrict__ text, long long* b, long long* e) {
    while (*b < *e && tr_ws(text[*b])) (*b)++;
    while (*e > *b && tr_ws(text[*e - 1])) (*e)--;
}

// FASTQ: read r = lines 4r .. 4r + 3 (the host has cut the trailing blank lines and checked that R whole records are there)
__global__ void trim_fastq_records_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ starts, long long R, long long* __restrict__ src,
                                          int* __restrict__ len, long long* __restrict__ qual, long long* __restrict__ nameb, int* __restrict__ namel,
                                          unsigned long long* __restrict__ err) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < R; r += (long long)gridDim.x * blockDim.x) {
        const long long* s = starts + 4 * r;
        const long long h = s[0], pl = s[2];
        long long b = s[1], e = pl, qb = s[3], qe = s[4];
        tr_strip(text, &b, &e);
        tr_strip(text, &qb, &qe);
        const int nl = tr_name(text, h, s[1]);
        int why = -1;
        if (text[h] != '@') why = TR_E_AT;
        else if (text[pl] != '+') why = TR_E_PLUS;
        else if (e - b > TR_LIMIT) why = TR_E_LONG;
        else if (qe - qb != e - b) why = TR_E_QLEN;
        else if (nl > TR_NAME_LIMIT) why = TR_E_NAME;
        if (why >= 0) tr_err(err, r, why);
        src[r] = b;
        len[r] = why >= 0 ? -1 : (int)(e - b);
        qual[r] = qb;
        nameb[r] = h + 1;
        namel[r] = nl;
    }
}

// FASTA: per line the header flag, the stripped start and the stripped length (capped at TR_LIMIT + 1: such a read is refused anyway)
__global__ void trim_fasta_lines_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ starts, long long n_lines, int* __restrict__ hdr,
                                        int* __restrict__ llen, long long* __restrict__ lb) {
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n_lines; k += (long long)gridDim.x * blockDim.x) {
        long long b = starts[k], e = starts[k + 1];
        const bool h = text[b] == '>';
        if (!h) tr_strip(text, &b, &e);
        hdr[k] = h;
        llen[k] = h ? 0 : (int)(e - b > TR_LIMIT ? TR_LIMIT + 1 : e - b);
        lb[k] = b;
    }
}
// first[record] = its header line (first[R] = n_lines is set by the host)
__global__ void trim_fasta_first_kernel(const int* __restrict__ hdr, const long long* __restrict__ hscan, long long n_lines, long long* __restrict__ first) {
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n_lines; k += (long long)gridDim.x * blockDim.x)
        if (hdr[k]) first[hscan[k]] = k;
}
// read r = the gathered bytes [goff[first[r]], goff[first[r + 1]])
__global__ void trim_fasta_records_kernel(const unsigned char* __restrict__ text, const long long* __restrict__ starts, const long long* __restrict__ first,
                                          const long long* __restrict__ goff, long long R, long long* __restrict__ src, int* __restrict__ len,
                                          long long* __restrict__ nameb, int* __restrict__ namel, unsigned long long* __restrict__ err) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < R; r += (long long)gridDim.x * blockDim.x) {
        const long long k0 = first[r], k1 = first[r + 1], L = goff[k1] - goff[k0];
        const int nl = tr_name(text, starts[k0], starts[k0 + 1]);
        const int why = L > TR_LIMIT ? TR_E_LONG : nl > TR_NAME_LIMIT ? TR_E_NAME : -1;
        if (why >= 0) tr_err(err, r, why);
        src[r] = goff[k0];
        len[r] = why >= 0 ? -1 : (int)L;
        nameb[r] = starts[k0] + 1;
        namel[r] = nl;
    }
}
__global__ void trim_fasta_gather_kernel(const unsigned char* __restrict__ text, const int* __restrict__ hdr, const int* __restrict__ llen,
                                         const long long* __restrict__ lb, const long long* __restrict__ goff, long long n_lines, unsigned char* __restrict__ g) {
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n_lines; k += (long long)gridDim.x * blockDim.x) {
        if (hdr[k]) continue;
        const unsigned char* s = text + lb[k];
        unsigned char* d = g + goff[k];
        for (int j = 0, e = llen[k]; j < e; j++) d[j] = s[j];
    }
}

// 2-bit code of an upper-cased base: A 0, C 1, T 2, G 3 (bits 1..2 of the ASCII code); the adapter is packed the same way on the host
__device__ __forceinline__ bool tr_acgt(unsigned u) { return u == 'A' || u == 'C' || u == 'G' || u == 'T'; }

// bases [start, start + 32) of a read of length L: codes (2 bits per base) and the non-ACGT mask (bit 2k for base start + k); bases past L are 0
__device__ __forceinline__ void tr_pack(const unsigned char* s, int L, int start, unsigned long long* code, unsigned long long* nm) {
    unsigned long long c = 0, x = 0;
    const int e = min(L - start, 32);
    for (int k = 0; k < e; k++) {
        const unsigned u = s[start + k] & 0xdfu;
        c |= (unsigned long long)((u >> 1) & 3u) << (2 * k);
        if (!tr_acgt(u)) x |= 1ull << (2 * k);
    }
    *code = c;
    *nm = x;
}

__device__ __forceinline__ unsigned long long tr_win(unsigned long long w0, unsigned long long w1, int sh) { return sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0; }

// flags of one read: 1 quality-trimmed, 2 adapter, 4 untrimmed discarded, 8 too short, 16 too long, 32 written, 64 bad quality byte
// s = the read's bytes, q = its quality bytes (fq); *f = the final length
__device__ __forceinline__ unsigned tr_one(const unsigned char* s, const unsigned char* q, bool fq, int n, const TrimArgs& a, int* f) {
    unsigned fl = 0;
    int L = n;
    if (fq) {
        for (int i = 0; i < n; i++) {
            const unsigned ch = q[i];
            if (ch < 33u || ch > 126u) return 64u;
        }
        if (a.q > 0) {
            int sum = 0, best = 0, cut = n;
            for (int i = n - 1; i >= 0; i--) {
                sum += a.q - ((int)q[i] - 33);
                if (sum < 0) break;
                if (sum > best) { best = sum; cut = i; }
            }
            if (cut < n) fl |= 1u;
            L = cut;
        }
    }
    bool found = false;
    if (a.m > 0) {
        const unsigned long long EVEN = 0x5555555555555555ull;
        unsigned long long c0, n0, c1, n1, c2, n2;
        tr_pack(s, L, 0, &c0, &n0);
        tr_pack(s, L, 32, &c1, &n1);
        tr_pack(s, L, 64, &c2, &n2);
        for (int p = 0;; p++) {
            const int l = min(a.m, L - p);
            if (l < a.ovl) break;
            const int j = p & 31;
            if (j == 0 && p > 0) {
                c0 = c1; n0 = n1; c1 = c2; n1 = n2;
                tr_pack(s, L, p + 64, &c2, &n2);
            }
            const int sh = 2 * j;
            const unsigned long long x0 = tr_win(c0, c1, sh) ^ a.a0, x1 = tr_win(c1, c2, sh) ^ a.a1;
            const unsigned long long v0 = l >= 32 ? EVEN : EVEN & ((1ull << (2 * l)) - 1ull);
            const unsigned long long v1 = l <= 32 ? 0ull : l == 64 ? EVEN : EVEN & ((1ull << (2 * (l - 32))) - 1ull);
            const unsigned long long m0 = ((x0 | (x0 >> 1)) | tr_win(n0, n1, sh)) & v0;
            const unsigned long long m1 = ((x1 | (x1 >> 1)) | tr_win(n1, n2, sh)) & v1;
            if (__popcll(m0) + __popcll(m1) <= (a.e_pm * l) / 1000) {
                found = true;
                L = p;
                break;
            }
        }
        if (found) fl |= 2u;
    }
    *f = -1;
    if (a.discard && !found) return fl | 4u;
    if (L < a.min_len) return fl | 8u;
    if (a.max_len > 0 && L > a.max_len) return fl | 16u;
    *f = L;
    return fl | 32u;
}

// one workgroup per TR_NT consecutive reads; base = the text (FASTQ, qual = quality starts) or the gathered reads (FASTA, qual = nullptr)
// counts[0 .. 6) = the reads per flag bit 0..5; counts[6], counts[7] = the workgroups that staged their slab in LDS / read from global memory
__global__ void __launch_bounds__(TR_NT) trim_reads_kernel(const unsigned char* __restrict__ base, const long long* __restrict__ src, const int* __restrict__ len,
                                                           const long long* __restrict__ qual, long long R, TrimArgs a, int* __restrict__ flen,
                                                           unsigned long long* __restrict__ counts, unsigned long long* __restrict__ err) {
    __shared__ uint4 slab[TR_SLAB / 16];
    __shared__ unsigned long long s_lo, s_hi;
    __shared__ unsigned s_cnt[6];
    const long long r = (long long)blockIdx.x * TR_NT + threadIdx.x;
    const bool fq = qual != nullptr;
    const int n = r < R ? len[r] : -1;
    const long long sb = n >= 0 ? src[r] : 0, qb = n >= 0 && fq ? qual[r] : 0;
    if (threadIdx.x == 0) { s_lo = ~0ull; s_hi = 0; }
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (n >= 0) {
        atomicMin(&s_lo, (unsigned long long)sb);
        atomicMax(&s_hi, (unsigned long long)((fq ? qb : sb) + n));
    }
    __syncthreads();
    const long long lo = (long long)(s_lo & ~15ull), span = (long long)s_hi - lo;
    unsigned fl = 0;
    int f = -1;
    if (threadIdx.x == 0 && s_lo != ~0ull) atomicAdd(&counts[span <= TR_SLAB ? 6 : 7], 1ull);
    if (s_lo != ~0ull && span <= TR_SLAB) {
        for (long long o = threadIdx.x * 16; o < span; o += TR_NT * 16) slab[o >> 4] = *(const uint4*)(base + lo + o);
        __syncthreads();
        const unsigned char* ls = (const unsigned char*)slab;
        if (n >= 0) fl = tr_one(ls + (sb - lo), ls + (qb - lo), fq, n, a, &f);
    } else if (n >= 0) {
        fl = tr_one(base + sb, base + qb, fq, n, a, &f);
    }
    if (r < R) flen[r] = f;
    if (fl & 64u) tr_err(err, r, TR_E_QBYTE);
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int b = 0; b < 6; b++) {
        const unsigned long long bal = __ballot((fl >> b) & 1u);
        if (lane == 0 && bal) atomicAdd(&s_cnt[b], (unsigned)__popcll(bal));
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

__global__ void trim_size_kernel(const int* __restrict__ flen, const int* __restrict__ namel, long long R, int* __restrict__ size) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < R; r += (long long)gridDim.x * blockDim.x)
        size[r] = flen[r] >= 0 ? namel[r] + flen[r] + 3 : 0;
}
__global__ void trim_emit_kernel(const unsigned char* __restrict__ text, const unsigned char* __restrict__ base, const long long* __restrict__ nameb,
                                 const int* __restrict__ namel, const long long* __restrict__ src, const int* __restrict__ flen, const long long* __restrict__ off,
                                 long long R, char* __restrict__ out) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < R; r += (long long)gridDim.x * blockDim.x) {
        const int f = flen[r];
        if (f < 0) continue;
        char* p = out + off[r];
        *p++ = '>';
        const unsigned char* nm = text + nameb[r];
        for (int k = 0, e = namel[r]; k < e; k++) *p++ = (char)nm[k];
        *p++ = '\n';
        const unsigned char* s = base + src[r];
        for (int k = 0; k < f; k++) *p++ = (char)s[k];
        *p = '\n';
    }
}

}  // namespace mirp

static inline int tr_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}
static inline bool tr_host_ws(unsigned char ch) { return ch == 32 || (ch >= 9 && ch <= 13) || (ch >= 0x1c && ch <= 0x1f); }

static const char* const kTrimReason[] = {"line 1 does not start with '@'", "line 3 does not start with '+'", "the read is longer than 1,024 nt (not supported)",
                                          "the sequence and quality lengths differ", "the name is longer than 1,048,576 bytes (not supported)",
                                          "a quality byte is outside 33..126", "the file ends inside the record (a FASTQ record is 4 lines)"};

static int tr_refuse_record(mirp_ctx* c, const char* name, long long r, int why) {
    return fail(c, -10, std::string(name) + ": record " + std::to_string(r + 1) + ": " + kTrimReason[why]);
}

// Upload, line split and records of one file held in host memory (n > 0), shared by the trim and by the library profile (libqc_kernels.hip): on
// return the per-read arrays t_src, t_len, t_qual, t_nameb, t_namel of the context are filled, and p says how to read them.  A refusal that
// needs no look at a read's bytes is returned here; the first bad FASTQ record waits in d_small[1] for mirp_device_trim_cut.  seconds[0 .. 3) gain
// upload, split and records.
int mirp_device_trim_parse(mirp_ctx* c, const char* text, long long n, const char* name, int quality_cutoff, MirpTrimParsed* p, double seconds[3]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    double t = mirp::now();
    if (c->t_text.ensure((size_t)n + TR_PAD) || c->t_small.ensure(80)) return fail(c, -6, "device allocation failed (trim: text)");
    unsigned char* d_text = (unsigned char*)c->t_text.p;
    unsigned long long* d_small = (unsigned long long*)c->t_small.p;   // [0] first byte >= 0x80, [1] first bad record key, [2 .. 8) counts, [8 .. 10) workgroups per path
    HIPCHK(c, hipMemcpy(d_text, text, (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(d_text + n, 0, TR_PAD, st));
    unsigned long long init[10] = {~0ull, ~0ull, 0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(d_small, init, sizeof init, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] += mirp::now() - t;

    // ---- split
    t = mirp::now();
    long long n_lines = 0, bad = -1;
    if (int rc = mirp_device_split_lines(c, d_text, n, 0x7fffffffffffffffll, c->t_bcnt, c->t_bscan, c->t_starts, d_small, &n_lines, &bad)) {
        if (rc == -9) {
            char msg[160];
            std::snprintf(msg, sizeof msg, ": byte 0x%02x at offset %lld is not ASCII (bytes >= 0x80 are not supported)", (unsigned)(unsigned char)text[bad], bad);
            c->err = std::string(name) + msg;
        }
        return rc;
    }
    const long long* d_starts = (const long long*)c->t_starts.p;
    seconds[1] += mirp::now() - t;

    // ---- records
    t = mirp::now();
    const bool fq = text[0] == '@';
    if (!fq && text[0] != '>') return fail(c, -10, std::string(name) + ": the first byte is neither '@' (FASTQ) nor '>' (FASTA)");
    if (!fq && quality_cutoff > 0) return fail(c, -10, std::string(name) + ": quality trimming needs FASTQ input, this file is FASTA");
    const long long max_reads = 0x7fffffffll;
    long long R = 0, rem = 0;
    const unsigned char* d_base = d_text;
    if (fq) {
        // the trailing blank lines are cut: the lines behind the one holding the last non-whitespace byte
        long long q = n - 1;
        while (q > 0 && tr_host_ws((unsigned char)text[q])) q--;
        long long after = 0;
        for (long long j = q + 1; j + 1 < n; j++)
            if (text[j] == '\n' || (text[j] == '\r' && text[j + 1] != '\n')) after++;
        const long long L = n_lines - after;
        R = L / 4;
        rem = L % 4;
        if (R > max_reads) return fail(c, -10, std::string(name) + ": more than 2^31 - 1 reads in one file");
    } else {
        if (c->t_hdr.ensure(4 * (size_t)n_lines) || c->t_llen.ensure(4 * (size_t)n_lines) || c->t_lb.ensure(8 * (size_t)n_lines) ||
            c->t_hscan.ensure(8 * (size_t)(n_lines + 1)) || c->t_goff.ensure(8 * (size_t)(n_lines + 1)))
            return fail(c, -6, "device allocation failed (trim: lines)");
        hipLaunchKernelGGL(trim_fasta_lines_kernel, dim3(tr_grid(n_lines)), dim3(256), 0, st, (const unsigned char*)d_text, d_starts, n_lines, (int*)c->t_hdr.p,
                           (int*)c->t_llen.p, (long long*)c->t_lb.p);
        launch_excl_scan(st, (const int*)c->t_hdr.p, (long long*)c->t_hscan.p, n_lines);
        launch_excl_scan(st, (const int*)c->t_llen.p, (long long*)c->t_goff.p, n_lines);
        HIPCHK(c, hipMemcpyAsync(&R, (long long*)c->t_hscan.p + n_lines, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (R > max_reads) return fail(c, -10, std::string(name) + ": more than 2^31 - 1 reads in one file");
    }
    if (c->t_src.ensure(8 * (size_t)R + 8) || c->t_len.ensure(4 * (size_t)R + 4) || c->t_qual.ensure(8 * (size_t)R + 8) || c->t_nameb.ensure(8 * (size_t)R + 8) ||
        c->t_namel.ensure(4 * (size_t)R + 4) || c->t_flen.ensure(4 * (size_t)R + 4) || c->t_off.ensure(8 * (size_t)(R + 1)))
        return fail(c, -6, "device allocation failed (trim: reads)");
    long long* d_src = (long long*)c->t_src.p;
    int* d_len = (int*)c->t_len.p;
    long long* d_nameb = (long long*)c->t_nameb.p;
    int* d_namel = (int*)c->t_namel.p;
    unsigned long long* d_err = d_small + 1;
    if (fq) {
        if (R > 0)
            hipLaunchKernelGGL(trim_fastq_records_kernel, dim3(tr_grid(R)), dim3(256), 0, st, (const unsigned char*)d_text, d_starts, R, d_src, d_len,
                               (long long*)c->t_qual.p, d_nameb, d_namel, d_err);
    } else {
        if (c->t_first.ensure(8 * (size_t)(R + 1))) return fail(c, -6, "device allocation failed (trim: records)");
        long long* d_first = (long long*)c->t_first.p;
        HIPCHK(c, hipMemcpyAsync(d_first + R, &n_lines, 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(trim_fasta_first_kernel, dim3(tr_grid(n_lines)), dim3(256), 0, st, (const int*)c->t_hdr.p, (const long long*)c->t_hscan.p, n_lines, d_first);
        hipLaunchKernelGGL(trim_fasta_records_kernel, dim3(tr_grid(R)), dim3(256), 0, st, (const unsigned char*)d_text, d_starts, (const long long*)d_first,
                           (const long long*)c->t_goff.p, R, d_src, d_len, d_nameb, d_namel, d_err);
        unsigned long long key = 0;
        long long G = 0;
        HIPCHK(c, hipMemcpyAsync(&key, d_err, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&G, (long long*)c->t_goff.p + n_lines, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (key != ~0ull) return tr_refuse_record(c, name, (long long)(key >> 3), (int)(key & 7));
        if (c->t_gbuf.ensure((size_t)G + TR_PAD)) return fail(c, -6, "device allocation failed (trim: reads)");
        hipLaunchKernelGGL(trim_fasta_gather_kernel, dim3(tr_grid(n_lines)), dim3(256), 0, st, (const unsigned char*)d_text, (const int*)c->t_hdr.p,
                           (const int*)c->t_llen.p, (const long long*)c->t_lb.p, (const long long*)c->t_goff.p, n_lines, (unsigned char*)c->t_gbuf.p);
        d_base = (const unsigned char*)c->t_gbuf.p;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    seconds[2] += mirp::now() - t;
    p->fq = fq;
    p->R = R;
    p->rem = rem;
    p->n_lines = n_lines;
    p->d_text = d_text;
    p->d_base = d_base;
    return 0;
}

// trim_reads_kernel over the reads of mirp_device_trim_parse under o: t_flen of the context gains the final lengths, res = {first bad record key,
// reads per flag bit 0..5, workgroups per path}.  The refusals that wait for the reads' bytes are returned here: the first bad record, then a file
// that ends inside a record.
int mirp_device_trim_cut(mirp_ctx* c, const MirpTrimParsed& p, const char* name, const MirpTrimOpts& o, unsigned long long res[9]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const bool fq = p.fq;
    const long long R = p.R, rem = p.rem;
    const unsigned char* d_base = p.d_base;
    unsigned long long* d_small = (unsigned long long*)c->t_small.p;
    unsigned long long* d_err = d_small + 1;
    const long long* d_src = (const long long*)c->t_src.p;
    const int* d_len = (const int*)c->t_len.p;
    TrimArgs a{};
    a.m = o.adapter_len; a.e_pm = o.error_permille; a.ovl = o.min_overlap; a.q = o.quality_cutoff;
    a.min_len = o.min_length; a.max_len = o.max_length; a.discard = o.discard_untrimmed;
    for (int k = 0; k < o.adapter_len; k++) {
        const unsigned long long code = ((unsigned)(o.adapter[k] & 0xdf) >> 1) & 3u;
        if (k < 32) a.a0 |= code << (2 * k);
        else a.a1 |= code << (2 * (k - 32));
    }
    int* d_flen = (int*)c->t_flen.p;
    if (R > 0)
        hipLaunchKernelGGL(trim_reads_kernel, dim3((unsigned)((R + TR_NT - 1) / TR_NT)), dim3(TR_NT), 0, st, d_base, (const long long*)d_src, (const int*)d_len,
                           fq ? (const long long*)c->t_qual.p : (const long long*)nullptr, R, a, d_flen, d_small + 2, d_err);
    HIPCHK(c, hipMemcpyAsync(res, d_small + 1, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (res[0] != ~0ull) return tr_refuse_record(c, name, (long long)(res[0] >> 3), (int)(res[0] & 7));
    if (rem) return tr_refuse_record(c, name, R, 6);
    return 0;
}

// The trim of one file held in host memory (mirp_trim.cpp checks the arguments and writes the file through sink; sink is called only once every
// refusal has been ruled out).  stats and seconds as mirp_trim_reads; seconds[5] gains the time spent in sink.
int mirp_device_trim_reads(mirp_ctx* c, const char* text, long long n, const char* name, const MirpTrimOpts& o,
                           const std::function<int(const char*, size_t)>& sink, long long stats[7], double seconds[6]) {
    using namespace mirp;
    for (int i = 0; i < 7; i++) stats[i] = 0;
    c->t_paths[0] = c->t_paths[1] = 0;
    if (n == 0) return 0;
    hipStream_t st = c->stream;
    MirpTrimParsed p;
    if (int rc = mirp_device_trim_parse(c, text, n, name, o.quality_cutoff, &p, seconds)) return rc;
    const long long R = p.R;
    const unsigned char *d_text = p.d_text, *d_base = p.d_base;
    const long long* d_src = (const long long*)c->t_src.p;
    int* d_len = (int*)c->t_len.p;
    const long long* d_nameb = (const long long*)c->t_nameb.p;
    const int* d_namel = (const int*)c->t_namel.p;
    int* d_flen = (int*)c->t_flen.p;

    // ---- trim
    double t = mirp::now();
    unsigned long long res[9];
    if (int rc = mirp_device_trim_cut(c, p, name, o, res)) return rc;
    seconds[3] += mirp::now() - t;

    // ---- emit + download
    t = mirp::now();
    long long total = 0;
    long long* d_off = (long long*)c->t_off.p;
    if (R > 0) {
        int* d_size = d_len;              // the read lengths are done with
        hipLaunchKernelGGL(trim_size_kernel, dim3(tr_grid(R)), dim3(256), 0, st, (const int*)d_flen, (const int*)d_namel, R, d_size);
        launch_excl_scan(st, (const int*)d_size, d_off, R);
        HIPCHK(c, hipMemcpyAsync(&total, d_off + R, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    if (c->t_out.ensure((size_t)total + 16)) return fail(c, -6, "device allocation failed (trim: output)");
    if (total > 0)
        hipLaunchKernelGGL(trim_emit_kernel, dim3(tr_grid(R)), dim3(256), 0, st, (const unsigned char*)d_text, d_base, (const long long*)d_nameb,
                           (const int*)d_namel, (const long long*)d_src, (const int*)d_flen, (const long long*)d_off, R, (char*)c->t_out.p);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    double in_sink = 0;
    if (int rc = mirp_download_text(c, (const char*)c->t_out.p, total, sink, &in_sink)) return rc;
    seconds[4] += mirp::now() - t - in_sink;
    seconds[5] += in_sink;
    stats[0] = R;
    for (int i = 0; i < 6; i++) stats[1 + i] = (long long)res[1 + i];
    c->t_paths[0] = (long long)res[7];
    c->t_paths[1] = (long long)res[8];
    return 0;
}
