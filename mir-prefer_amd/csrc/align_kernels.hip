// Device side of the read alignment (mirp_align_index / mirp_align_reads, mirp_align.cpp): what the reference's scripts/bowtie-align-reads.py
// gets from `bowtie-build` and `bowtie -v V --best --strata -k K [-m M] -S`, with the semantics of DESIGN.md §12.
//
// Reference (resident for the context's lifetime, built once per invocation):
//   pk[]   2-bit bases, 16 per u32, base i at bits 2 (i % 16); amb[] 1 bit per position (non-ACGT, and every position past the end);
//   cst[]  1 bit per contig start.  Positions are global over the concatenation of the contigs in reference order (u32, < 2^32).
//   Index  a truncated suffix array: every unambiguous position p with the key of its first 16 bases (bases up to the first ambiguous base or
//          the next contig start; the rest padded with A), sorted stably by key: SA[] = positions, ascending within a key.
//          al_keys_kernel writes key << 32 | p, mirp_device_sort_u64 sorts by the high 32 bits (4 passes of 8), al_strip_kernel keeps p.
//          bkt[b] = first SA slot whose key starts with the 12 bases b (4^12 + 1 entries: a histogram in al_strip_kernel + launch_excl_scan).
//
// Reads (one batch at a time, see mirp_device_align_batch):
//   seeds     al_seedcount_kernel, launch_excl_scan, al_seedfill_kernel.  v = 0: the whole read on each strand.  v > 0: the two halves of the
//             oriented read (first ceil(L/2) bases, the rest); with e = v / 2 = 1 also every single-substitution variant of a half.  A seed is the
//             SA range of its first min(len, 16) bases (bucket table, then a binary search inside the bucket that recomputes keys).
//   verify    launch_excl_scan over the seed ranges = a flat candidate space; al_verify_kernel takes one candidate per thread: the window must lie
//             in one contig and hold no ambiguous base, the seed's bases must equal the genome exactly, the read must have <= v mismatches, and
//             the hit counts only from its canonical finder (half A if it has <= e mismatches there, otherwise half B), so no hit is found twice.
//             Pass 1 counts hits per read and mismatch level; al_status_kernel takes the best stratum and the -m decision; pass 2 writes the
//             best-stratum hits of the kept reads as (read << 33 | gpos << 1 | strand) at scanned per-read offsets.
//   order     mirp_device_sort_u64 by the whole record: per read, (contig, offset, + before -); the first K per read are kept.
//   emit      al_size_kernel, launch_excl_scan, al_emit_kernel: the SAM records on the device (one shared routine counts and writes).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "text_out.h"
#include "align_device.h"

namespace mirp {

// ---------------------------------------------------------------- index
__global__ void al_count_kernel(const unsigned* __restrict__ amb, long long n_words, int* __restrict__ cnt) {
    for (long long w = blockIdx.x * (long long)blockDim.x + threadIdx.x; w < n_words; w += (long long)gridDim.x * blockDim.x) cnt[w] = __popc(~amb[w]);
}
__global__ void al_keys_kernel(AlRef R, long long n_words, const long long* __restrict__ wscan, unsigned long long* __restrict__ rec) {
    for (long long w = blockIdx.x * (long long)blockDim.x + threadIdx.x; w < n_words; w += (long long)gridDim.x * blockDim.x) {
        unsigned m = ~R.amb[w];
        long long o = wscan[w];
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            const unsigned long long p = ((unsigned long long)w << 5) + j;
            rec[o++] = ((unsigned long long)al_key16(R, p) << 32) | p;
        }
    }
}
__global__ void al_strip_kernel(const unsigned long long* __restrict__ rec, long long n, unsigned* __restrict__ sa, int* __restrict__ hist) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long r = rec[i];
        sa[i] = (unsigned)r;
        atomicAdd(&hist[r >> (64 - 2 * AL_BKT_BASES)], 1);
    }
}

// ---------------------------------------------------------------- reads
__global__ void al_seedcount_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ roff, long long n, AlParams P, int* __restrict__ cnt) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const unsigned char* rd = codes + roff[r];
        const int L = (int)(roff[r + 1] - roff[r]);
        int c = 0;
        if (L > P.v)
            for (int s = 0; s < 2; s++)
                for (int h = 0; h < (P.v ? 2 : 1); h++) {
                    int hoff, hlen, bp;
                    al_half(L, P.v, h, &hoff, &hlen);
                    c += al_nseeds(rd, L, s, hoff, hlen, P.e, &bp);
                }
        cnt[r] = c;
    }
}

__global__ void al_seedfill_kernel(AlRef R, const unsigned char* __restrict__ codes, const long long* __restrict__ roff, long long n, AlParams P,
                                   const long long* __restrict__ sscan, AlSeed* __restrict__ seeds, int* __restrict__ ccnt, int* __restrict__ overflow) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const unsigned char* rd = codes + roff[r];
        const int L = (int)(roff[r + 1] - roff[r]);
        if (L <= P.v) continue;
        long long o = sscan[r];
        for (int s = 0; s < 2; s++)
            for (int h = 0; h < (P.v ? 2 : 1); h++) {
                int hoff, hlen, bp;
                al_half(L, P.v, h, &hoff, &hlen);
                const int ns = al_nseeds(rd, L, s, hoff, hlen, P.e, &bp);
                const int m = hlen < 16 ? hlen : 16;
                for (int k = 0; k < ns; k++) {
                    // variant k: -1 = exact; otherwise position and base (the one non-ACGT position takes all 4 bases)
                    int vpos = -1, vbase = 0;
                    if (bp >= 0) { vpos = bp; vbase = k; }
                    else if (k > 0) {
                        vpos = (k - 1) / 3;
                        const unsigned rb = al_oriented(rd, L, s, hoff + vpos);
                        vbase = (int)((rb + 1 + (k - 1) % 3) & 3u);
                    }
                    unsigned key = 0;
                    for (int i = 0; i < m; i++) key = (key << 2) | (i == vpos ? (unsigned)vbase : al_oriented(rd, L, s, hoff + i));
                    long long lo, hi;
                    al_range(R, key, m, &lo, &hi);
                    AlSeed sd;
                    sd.lo = lo; sd.read = (unsigned)r; sd.strand = (unsigned char)s; sd.half = (unsigned char)h; sd.vbase = (unsigned char)vbase; sd.pad = 0;
                    sd.vpos = vpos;
                    seeds[o] = sd;
                    const long long c = hi - lo;
                    if (c > 0x7fffffffll) { atomicOr(overflow, 1); ccnt[o] = 0x7fffffff; }
                    else ccnt[o] = (int)c;
                    o++;
                }
            }
    }
}

// pass 0: hit counts per read and level; pass 1: the best-stratum hits of the kept reads at scanned offsets.  One candidate per thread; its seed
// comes from a binary search over the seed scan.
template <int PASS>
__global__ void al_verify_kernel(AlRef R, const unsigned char* __restrict__ codes, const long long* __restrict__ roff, const AlSeed* __restrict__ seeds,
                                 long long n_seeds, const long long* __restrict__ cscan, AlParams P, unsigned* __restrict__ lvl, const int* __restrict__ best,
                                 const long long* __restrict__ off, unsigned* __restrict__ cursor, unsigned long long* __restrict__ out) {
    const long long total = cscan[n_seeds];
    for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < total; c += (long long)gridDim.x * blockDim.x) {
        long long a = 0, z = n_seeds;                 // last seed with cscan <= c
        while (z - a > 1) { const long long md = (a + z) >> 1; if (cscan[md] <= c) a = md; else z = md; }
        const AlSeed sd = seeds[a];
        const unsigned long long pos = R.sa[sd.lo + (c - cscan[a])];
        const long long rb = roff[sd.read];
        const int L = (int)(roff[sd.read + 1] - rb);
        const int mm = al_check(R, codes + rb, L, sd, pos, P);
        if (mm < 0) continue;
        if (PASS == 0) {
            atomicAdd(&lvl[4 * (long long)sd.read + mm], 1u);
        } else if (best[sd.read] == mm) {
            int hoff, hlen;
            al_half(L, P.v, sd.half, &hoff, &hlen);
            const unsigned slot = atomicAdd(&cursor[sd.read], 1u);
            if ((long long)slot < off[sd.read + 1] - off[sd.read])          // pass 1 found the same hits: always true
                out[off[sd.read] + slot] = ((unsigned long long)sd.read << 33) | ((pos - hoff) << 1) | sd.strand;
        }
    }
}

// sum of v over the 64 lanes, added to *dst by lane 0 (every lane of the wave calls it)
__device__ __forceinline__ void al_wave_add(unsigned long long* dst, unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// per read: best stratum (best[r] = mismatches, -1 none / suppressed), slots of its output records; stats {aligned, unaligned, suppressed}
__global__ void al_status_kernel(const unsigned* __restrict__ lvl, const long long* __restrict__ roff, long long n, AlParams P, int* __restrict__ best,
                                 int* __restrict__ supp, int* __restrict__ slots, unsigned long long* __restrict__ stats) {
    unsigned long long cnt[3] = {0, 0, 0};
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        int b = -1;
        unsigned nb = 0;
        for (int l = 0; l <= P.v && b < 0; l++)
            if (lvl[4 * r + l]) { b = l; nb = lvl[4 * r + l]; }
        int s = 0;
        if (b >= 0 && P.m > 0 && nb > (unsigned)P.m) { b = -1; s = 1; }
        best[r] = b;
        supp[r] = s;
        slots[r] = b >= 0 ? (nb > 0x7fffffffu ? 0x7fffffff : (int)nb) : (P.filter ? 0 : 1);
        cnt[b >= 0 ? 0 : s ? 2 : 1]++;
    }
    for (int i = 0; i < 3; i++) al_wave_add(&stats[i], cnt[i]);
}
__global__ void al_unaln_kernel(const int* __restrict__ best, const long long* __restrict__ off, long long n, unsigned long long* __restrict__ out) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x)
        if (best[r] < 0 && off[r + 1] > off[r]) out[off[r]] = (unsigned long long)r << 33;
}

// ---------------------------------------------------------------- SAM text
struct AlText {
    const unsigned char* codes; const long long* roff;
    const char* qn; const long long* qoff;
    const char* names; const long long* noff;
    const unsigned long long* cstart; int n_contigs;
};

// one SAM record: item = read << 33 | gpos << 1 | strand; best < 0: unaligned (XM:i:0, or XM:i:<M+1> when suppressed)
template <bool WRITE>
__device__ long long al_record(const AlRef& R, const AlText& T, const AlParams& P, unsigned long long item, int best, int supp, char* out) {
    TextOut<WRITE> o{out};
    const long long r = (long long)(item >> 33);
    const long long rb = T.roff[r];
    const int L = (int)(T.roff[r + 1] - rb);
    const unsigned char* rd = T.codes + rb;
    o.str(T.qn + T.qoff[r], T.qoff[r + 1] - T.qoff[r]);
    const char* ACGTN = "ACGTN";
    if (best < 0) {
        o.lit("\t4\t*\t0\t0\t*\t*\t0\t0\t");
        if (L == 0) o.ch('*'); else for (int i = 0; i < L; i++) o.ch(ACGTN[rd[i]]);
        o.ch('\t');
        if (L == 0) o.ch('*'); else for (int i = 0; i < L; i++) o.ch('I');
        o.lit("\tXM:i:");
        o.num(supp ? (unsigned long long)P.m + 1 : 0ull);
        o.ch('\n');
        return o.n;
    }
    const int strand = (int)(item & 1);
    const unsigned long long g = (item >> 1) & 0xffffffffull;
    const int a = site_contig(T.cstart, T.n_contigs, g);
    o.ch('\t');
    o.num(strand ? 16 : 0);
    o.ch('\t');
    o.str(T.names + T.noff[a], T.noff[a + 1] - T.noff[a]);
    o.ch('\t');
    o.num(g - T.cstart[a] + 1);
    o.lit("\t255\t");
    o.num((unsigned long long)L);
    o.lit("M\t*\t0\t0\t");
    for (int i = 0; i < L; i++) o.ch(ACGTN[al_oriented(rd, L, strand, i)]);
    o.ch('\t');
    for (int i = 0; i < L; i++) o.ch('I');
    o.lit("\tXA:i:");
    o.num((unsigned long long)best);
    o.lit("\tMD:Z:");
    int run = 0;
    for (int i = 0; i < L; i++) {
        const unsigned gb = al_base(R.pk, g + i);
        if (al_oriented(rd, L, strand, i) == gb) { run++; continue; }
        o.num((unsigned long long)run);
        o.ch(ACGTN[gb]);
        run = 0;
    }
    o.num((unsigned long long)run);
    o.lit("\tNM:i:");
    o.num((unsigned long long)best);
    o.ch('\n');
    return o.n;
}

// size[i] of sorted item i (0: cut by -k); records[0] += kept items
__global__ void al_size_kernel(AlRef R, AlText T, AlParams P, const unsigned long long* __restrict__ items, long long n, const long long* __restrict__ off,
                               const int* __restrict__ best, const int* __restrict__ supp, int* __restrict__ size, unsigned long long* __restrict__ records) {
    unsigned long long kept = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long it = items[i];
        const long long r = (long long)(it >> 33);
        const bool keep = i - off[r] < (long long)P.k;
        size[i] = keep ? (int)al_record<false>(R, T, P, it, best[r], supp[r], nullptr) : 0;
        kept += keep;
    }
    al_wave_add(records, kept);
}
__global__ void al_emit_kernel(AlRef R, AlText T, AlParams P, const unsigned long long* __restrict__ items, long long n, const long long* __restrict__ toff,
                               const int* __restrict__ best, const int* __restrict__ supp, char* __restrict__ text) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (toff[i + 1] == toff[i]) continue;
        const unsigned long long it = items[i];
        const long long r = (long long)(it >> 33);
        (void)al_record<true>(R, T, P, it, best[r], supp[r], text + toff[i]);
    }
}

}  // namespace mirp

static inline int al_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

static mirp::AlRef al_ref(const mirp_ctx* c) {
    return mirp::AlRef{(const unsigned*)c->a_pk.p, (const unsigned*)c->a_amb.p, (const unsigned*)c->a_cst.p, (const unsigned*)c->a_sa.p,
                       (const long long*)c->a_bkt.p, (unsigned long long)c->a_total};
}

// Uploads the packed reference and builds the index.  pk: (total + 15) / 16 + 2 words, amb / cst: (total + 31) / 32 + 2 words (amb set past the end).
// seconds: [0] upload, [1] keys, [2] sort, [3] strip + buckets.
int mirp_device_align_index(mirp_ctx* c, const unsigned* pk, const unsigned* amb, const unsigned* cst, long long total,
                            const std::vector<unsigned long long>& cstart, const std::string& names, const std::vector<long long>& noff, double seconds[4]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    c->a_ready = false;
    const long long n_pk = (total + 15) / 16 + 2, n_bm = (total + 31) / 32 + 2, n_words = (total + 31) / 32;
    double t = mirp::now();
    if (c->a_pk.ensure(4 * (size_t)n_pk) || c->a_amb.ensure(4 * (size_t)n_bm) || c->a_cst.ensure(4 * (size_t)n_bm) ||
        c->a_cstart.ensure(8 * cstart.size()) || c->a_names.ensure(names.size() + 1) || c->a_noff.ensure(8 * noff.size()))
        return fail(c, -6, "device allocation failed (align: reference)");
    HIPCHK(c, hipMemcpyAsync(c->a_pk.p, pk, 4 * (size_t)n_pk, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_amb.p, amb, 4 * (size_t)n_bm, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_cst.p, cst, 4 * (size_t)n_bm, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_cstart.p, cstart.data(), 8 * cstart.size(), hipMemcpyHostToDevice, st));
    if (!names.empty()) HIPCHK(c, hipMemcpyAsync(c->a_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_noff.p, noff.data(), 8 * noff.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] = mirp::now() - t;

    // ---- keys of the unambiguous positions, in position order
    t = mirp::now();
    TmpDevice T;
    int* wcnt = (int*)T.get(4 * (size_t)std::max<long long>(n_words, 1));
    long long* wscan = (long long*)T.get(8 * (size_t)(n_words + 1));
    if (!wcnt || !wscan) return fail(c, -6, "device allocation failed (align: index scan)");
    long long N = 0;
    if (n_words > 0) {
        hipLaunchKernelGGL(al_count_kernel, dim3(al_grid(n_words)), dim3(256), 0, st, (const unsigned*)c->a_amb.p, n_words, wcnt);
        launch_excl_scan(st, wcnt, wscan, n_words);
        HIPCHK(c, hipMemcpyAsync(&N, wscan + n_words, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    unsigned long long* rec = (unsigned long long*)T.get(8 * (size_t)std::max<long long>(N, 1));
    unsigned long long* rtmp = (unsigned long long*)T.get(8 * (size_t)std::max<long long>(N, 1));
    if (!rec || !rtmp) return fail(c, -6, "device allocation failed (align: index records)");
    const AlRef R0{(const unsigned*)c->a_pk.p, (const unsigned*)c->a_amb.p, (const unsigned*)c->a_cst.p, nullptr, nullptr, (unsigned long long)total};
    if (N > 0) hipLaunchKernelGGL(al_keys_kernel, dim3(al_grid(n_words)), dim3(256), 0, st, R0, n_words, (const long long*)wscan, rec);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    seconds[1] = mirp::now() - t;

    // ---- stable sort by key
    t = mirp::now();
    if (int rc = mirp_device_sort_u64(c, rec, rtmp, N, 32, 32)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[2] = mirp::now() - t;

    // ---- positions + bucket table
    t = mirp::now();
    if (c->a_sa.ensure(4 * (size_t)std::max<long long>(N, 1) + 16) || c->a_bkt.ensure(8 * ((size_t)AL_NBKT + 1)))
        return fail(c, -6, "device allocation failed (align: index)");
    int* hist = (int*)rtmp;     // the sort's second buffer is done with (4^12 ints = 64 MiB; N >= 2^23 records or a separate buffer)
    if ((size_t)N * 8 < 4 * (size_t)AL_NBKT) {
        hist = (int*)T.get(4 * (size_t)AL_NBKT);
        if (!hist) return fail(c, -6, "device allocation failed (align: buckets)");
    }
    HIPCHK(c, hipMemsetAsync(hist, 0, 4 * (size_t)AL_NBKT, st));
    if (N > 0) hipLaunchKernelGGL(al_strip_kernel, dim3(al_grid(N)), dim3(256), 0, st, (const unsigned long long*)rec, N, (unsigned*)c->a_sa.p, hist);
    launch_excl_scan(st, hist, (long long*)c->a_bkt.p, (long long)AL_NBKT);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    seconds[3] = mirp::now() - t;
    c->a_total = total;
    c->a_nsa = N;
    c->a_n_contigs = (int)cstart.size() - 1;
    c->a_ready = true;
    return 0;
}

// One batch of reads: codes (0..3 ACGT, 4 other) at roff[0..n], QNAMEs at qoff[0..n], all on the host.  The batch's SAM text goes to `sink` in
// pieces of at most 1 GiB.  stats += {aligned, unaligned, suppressed, records}; seconds += [0] upload, [1] seeds, [2] verify, [3] sort, [4] emit
int mirp_device_align_batch(mirp_ctx* c, const unsigned char* codes, const long long* roff, const char* qn, const long long* qoff, long long n, int v, int k,
                            int m, int filter, const std::function<int(const char*, size_t)>& sink, long long stats[4], double seconds[5]) {
    using namespace mirp;
    if (!c->a_ready) return fail(c, -1, "mirp_align_reads: no index (mirp_align_index first)");
    if (n <= 0) return 0;
    hipStream_t st = c->stream;
    const AlParams P{v, v / 2, k, m, filter};
    const AlRef R = al_ref(c);
    double t = mirp::now();
    const long long nb = roff[n], nq = qoff[n];
    if (c->a_codes.ensure((size_t)nb + 16) || c->a_roff.ensure(8 * (size_t)(n + 1)) || c->a_qn.ensure((size_t)nq + 16) || c->a_qoff.ensure(8 * (size_t)(n + 1)) ||
        c->a_small.ensure(64))
        return fail(c, -6, "device allocation failed (align: reads)");
    if (nb) HIPCHK(c, hipMemcpyAsync(c->a_codes.p, codes, (size_t)nb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_roff.p, roff, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    if (nq) HIPCHK(c, hipMemcpyAsync(c->a_qn.p, qn, (size_t)nq, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_qoff.p, qoff, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    unsigned long long* d_small = (unsigned long long*)c->a_small.p;    // [0..2] aligned / unaligned / suppressed, [3] records, [4] overflow flag
    HIPCHK(c, hipMemsetAsync(d_small, 0, 64, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] += mirp::now() - t;
    const unsigned char* d_codes = (const unsigned char*)c->a_codes.p;
    const long long* d_roff = (const long long*)c->a_roff.p;
    const int g = al_grid(n);

    // ---- seeds
    t = mirp::now();
    if (c->a_rcnt.ensure(4 * (size_t)n) || c->a_rscan.ensure(8 * (size_t)(n + 1))) return fail(c, -6, "device allocation failed (align: seeds)");
    int* d_rcnt = (int*)c->a_rcnt.p;
    long long* d_rscan = (long long*)c->a_rscan.p;
    hipLaunchKernelGGL(al_seedcount_kernel, dim3(g), dim3(256), 0, st, d_codes, d_roff, n, P, d_rcnt);
    launch_excl_scan(st, d_rcnt, d_rscan, n);
    long long S = 0;
    HIPCHK(c, hipMemcpyAsync(&S, d_rscan + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (c->a_seeds.ensure(sizeof(AlSeed) * (size_t)std::max<long long>(S, 1)) || c->a_ccnt.ensure(4 * (size_t)std::max<long long>(S, 1)) ||
        c->a_cscan.ensure(8 * (size_t)(S + 1)))
        return fail(c, -6, "device allocation failed (align: seeds)");
    AlSeed* d_seeds = (AlSeed*)c->a_seeds.p;
    long long* d_cscan = (long long*)c->a_cscan.p;
    hipLaunchKernelGGL(al_seedfill_kernel, dim3(g), dim3(256), 0, st, R, d_codes, d_roff, n, P, (const long long*)d_rscan, d_seeds, (int*)c->a_ccnt.p,
                       (int*)(d_small + 4));
    if (S > 0) launch_excl_scan(st, (const int*)c->a_ccnt.p, d_cscan, S);
    else HIPCHK(c, hipMemsetAsync(d_cscan, 0, 8, st));
    unsigned long long ovf = 0;
    long long TC = 0;
    HIPCHK(c, hipMemcpyAsync(&ovf, d_small + 4, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&TC, d_cscan + S, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (ovf) return fail(c, -5, "a seed matches 2^31 or more index positions");
    seconds[1] += mirp::now() - t;

    // ---- verify: counts, strata, best-stratum hits
    t = mirp::now();
    if (c->a_lvl.ensure(16 * (size_t)n) || c->a_best.ensure(4 * (size_t)n) || c->a_supp.ensure(4 * (size_t)n) || c->a_slots.ensure(4 * (size_t)n) ||
        c->a_off.ensure(8 * (size_t)(n + 1)) || c->a_cursor.ensure(4 * (size_t)n))
        return fail(c, -6, "device allocation failed (align: strata)");
    unsigned* d_lvl = (unsigned*)c->a_lvl.p;
    int* d_best = (int*)c->a_best.p;
    int* d_supp = (int*)c->a_supp.p;
    long long* d_off = (long long*)c->a_off.p;
    HIPCHK(c, hipMemsetAsync(d_lvl, 0, 16 * (size_t)n, st));
    HIPCHK(c, hipMemsetAsync(c->a_cursor.p, 0, 4 * (size_t)n, st));
    const int gc = al_grid(TC);
    if (TC > 0)
        hipLaunchKernelGGL(al_verify_kernel<0>, dim3(gc), dim3(256), 0, st, R, d_codes, d_roff, (const AlSeed*)d_seeds, S, (const long long*)d_cscan, P, d_lvl,
                           (const int*)nullptr, (const long long*)nullptr, (unsigned*)nullptr, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(al_status_kernel, dim3(g), dim3(256), 0, st, (const unsigned*)d_lvl, d_roff, n, P, d_best, d_supp, (int*)c->a_slots.p, d_small);
    launch_excl_scan(st, (const int*)c->a_slots.p, d_off, n);
    long long NI = 0;
    HIPCHK(c, hipMemcpyAsync(&NI, d_off + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (c->a_items.ensure(8 * (size_t)std::max<long long>(NI, 1)) || c->a_itmp.ensure(8 * (size_t)std::max<long long>(NI, 1)))
        return fail(c, -6, "device allocation failed (align: hits)");
    unsigned long long* d_items = (unsigned long long*)c->a_items.p;
    if (TC > 0)
        hipLaunchKernelGGL(al_verify_kernel<1>, dim3(gc), dim3(256), 0, st, R, d_codes, d_roff, (const AlSeed*)d_seeds, S, (const long long*)d_cscan, P,
                           (unsigned*)nullptr, (const int*)d_best, (const long long*)d_off, (unsigned*)c->a_cursor.p, d_items);
    hipLaunchKernelGGL(al_unaln_kernel, dim3(g), dim3(256), 0, st, (const int*)d_best, (const long long*)d_off, n, d_items);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    seconds[2] += mirp::now() - t;

    // ---- order: by (read, gpos, strand)
    t = mirp::now();
    int rbits = 0;
    while ((1ll << rbits) < n) rbits++;
    if (int rc = mirp_device_sort_u64(c, d_items, (unsigned long long*)c->a_itmp.p, NI, 0, (33 + rbits + 7) / 8 * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[3] += mirp::now() - t;

    // ---- emit + download
    t = mirp::now();
    if (c->a_size.ensure(4 * (size_t)std::max<long long>(NI, 1)) || c->a_toff.ensure(8 * (size_t)(NI + 1)))
        return fail(c, -6, "device allocation failed (align: text offsets)");
    const AlText TX{d_codes, d_roff, (const char*)c->a_qn.p, (const long long*)c->a_qoff.p, (const char*)c->a_names.p, (const long long*)c->a_noff.p,
                    (const unsigned long long*)c->a_cstart.p, c->a_n_contigs};
    long long* d_toff = (long long*)c->a_toff.p;
    long long bytes = 0;
    if (NI > 0) {
        hipLaunchKernelGGL(al_size_kernel, dim3(al_grid(NI)), dim3(256), 0, st, R, TX, P, (const unsigned long long*)d_items, NI, (const long long*)d_off,
                           (const int*)d_best, (const int*)d_supp, (int*)c->a_size.p, d_small + 3);
        launch_excl_scan(st, (const int*)c->a_size.p, d_toff, NI);
        HIPCHK(c, hipMemcpyAsync(&bytes, d_toff + NI, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    if (c->a_text.ensure((size_t)bytes + 16)) return fail(c, -6, "device allocation failed (align: text)");
    if (NI > 0)
        hipLaunchKernelGGL(al_emit_kernel, dim3(al_grid(NI)), dim3(256), 0, st, R, TX, P, (const unsigned long long*)d_items, NI, (const long long*)d_toff,
                           (const int*)d_best, (const int*)d_supp, (char*)c->a_text.p);
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt, d_small, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (int rc = mirp_download_text(c, (const char*)c->a_text.p, bytes, sink)) return rc;
    seconds[4] += mirp::now() - t;
    for (int i = 0; i < 4; i++) stats[i] += (long long)cnt[i];
    return 0;
}
