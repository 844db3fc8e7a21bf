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
// Reads (one batch at a time, see mirp_device_align_upload / _hits / _emit):
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
//   place     (align --place) between order and emit: al_unique_kernel collects the file's unique reads over all batches; after the last batch
//             one sort by position and two int32 scans give the 64-bit prefix of their depths; al_weight_kernel (one item per thread, two binary
//             searches) and al_pick_kernel (one read per thread: hash, running sum) choose one item per read, which the emit step then writes.
//   tails     (align --tail) inside the hits step, between al_status_kernel and the scan of the per-read slots: align_tail_kernels.hip searches the
//             reads left without a hit for a templated 5' part and 1 .. T non-templated 3' bases; their items are sorted, cut and emitted with the
//             rest, and al_record prints the tailed forms (soft clip, XT:Z:) from the per-read tail length.
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
    // placement (AlParams::place != 0), per read: hits in the best stratum, class 'N' / 'U' / 'R', weight of the chosen hit, sum of the weights
    const int* pn; const unsigned char* pcls; const unsigned long long* pw; const unsigned long long* pwt;
    // tails (align --tail), per read: length of the non-templated 3' tail of its records, 0 = an end-to-end hit; null without --tail
    const unsigned char* tt;
};

#define AL_NO_ITEM (~0ull)      // placement: a read without a record (unaligned under -f)

// one SAM record: item = read << 33 | gpos << 1 | strand; best < 0: unaligned (XM:i:0, or XM:i:<M+1> when suppressed).  With P.place the record of
// an aligned read carries NH:i:<n> XY:Z:<class> XW:Z:<w>/<Wt> after NM:i:.  A tailed read (T.tt[read] = t > 0, DESIGN.md §12 "Tails"): the item's
// offset is that of its templated 5' part of m = L - t bases; <m>M<t>S on +, <t>S<m>M on -, MD:Z:<m>, XT:Z:<the last t letters as sequenced>; with
// P.tail_trim SEQ and QUAL hold the templated part only and the CIGAR is <m>M
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
    const int t = T.tt ? (int)T.tt[r] : 0;
    if (t > 0) {
        const int m = L - t;
        const int first = P.tail_trim ? (strand ? t : 0) : 0, last = P.tail_trim ? first + m : L;      // the part of the oriented read in SEQ
        if (strand && !P.tail_trim) { o.num((unsigned long long)t); o.ch('S'); }
        o.num((unsigned long long)m);
        o.ch('M');
        if (!strand && !P.tail_trim) { o.num((unsigned long long)t); o.ch('S'); }
        o.lit("\t*\t0\t0\t");
        for (int i = first; i < last; i++) o.ch(ACGTN[al_oriented(rd, L, strand, i)]);
        o.ch('\t');
        for (int i = first; i < last; i++) o.ch('I');
        o.lit("\tXA:i:0\tMD:Z:");
        o.num((unsigned long long)m);
        o.lit("\tNM:i:0\tXT:Z:");
        for (int i = m; i < L; i++) o.ch(ACGTN[rd[i]]);
        o.ch('\n');
        return o.n;
    }
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
    if (P.place) {
        o.lit("\tNH:i:");
        o.num((unsigned long long)T.pn[r]);
        o.lit("\tXY:Z:");
        o.ch((char)T.pcls[r]);
        o.lit("\tXW:Z:");
        o.num(T.pw[r]);
        o.ch('/');
        o.num(T.pwt[r]);
    }
    o.ch('\n');
    return o.n;
}

// size[i] of sorted item i (0: cut by -k); records[0] += kept items.  With P.place the items are the picks, one per read (AL_NO_ITEM: no record)
__global__ void al_size_kernel(AlRef R, AlText T, AlParams P, const unsigned long long* __restrict__ items, long long n, const long long* __restrict__ off,
                               const int* __restrict__ best, const int* __restrict__ supp, int* __restrict__ size, unsigned long long* __restrict__ records) {
    unsigned long long kept = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long it = items[i];
        const long long r = P.place ? i : (long long)(it >> 33);
        const bool keep = P.place ? it != AL_NO_ITEM : i - off[r] < (long long)P.k;
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

// ---------------------------------------------------------------- placement (align --place, DESIGN.md §12 "Placement")
// a unique read: one hit in its best stratum.  WRITE = false: flag[r]; WRITE = true: gpos << 32 | depth at uscan[r] of this batch's part of the list
template <bool WRITE>
__global__ void al_unique_kernel(const unsigned long long* __restrict__ items, const long long* __restrict__ off, const int* __restrict__ best, long long n,
                                 const unsigned* __restrict__ depth, int* __restrict__ flag, const long long* __restrict__ uscan,
                                 unsigned long long* __restrict__ ulist) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const bool u = best[r] >= 0 && off[r + 1] - off[r] == 1;
        if (!WRITE) flag[r] = u;
        else if (u) ulist[uscan[r]] = (((items[off[r]] >> 1) & 0xffffffffull) << 32) | depth[r];
    }
}
// the sorted unique list -> positions, and the depths as their low 30 bits and the rest (two int32 scans make the exact 64-bit prefix)
__global__ void al_usplit_kernel(const unsigned long long* __restrict__ ulist, long long n, unsigned* __restrict__ upos, int* __restrict__ lo, int* __restrict__ hi) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long u = ulist[i];
        upos[i] = (unsigned)(u >> 32);
        lo[i] = (int)(u & 0x3fffffffull);
        hi[i] = (int)((u >> 30) & 3ull);
    }
}
// upre[i] = sum of the depths of the unique reads before i, i = 0 .. n
__global__ void al_uprefix_kernel(const long long* __restrict__ lo_scan, const long long* __restrict__ hi_scan, long long n, unsigned long long* __restrict__ upre) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i <= n; i += (long long)gridDim.x * blockDim.x)
        upre[i] = (unsigned long long)lo_scan[i] + ((unsigned long long)hi_scan[i] << 30);
}

// first index of upos[0 .. n) with upos[i] >= g (g may be 2^32: past every position)
__device__ __forceinline__ long long al_ulower(const unsigned* __restrict__ upos, long long n, unsigned long long g) {
    long long a = 0, z = n;
    while (a < z) { const long long md = (a + z) >> 1; if ((unsigned long long)upos[md] < g) a = md + 1; else z = md; }
    return a;
}

// weight of every best-stratum item of a multi-mapped read: the depths of the unique reads whose position lies in the hit's footprint widened by
// W on both sides and clipped to the hit's contig.  One item per thread; items of other reads get 0.
__global__ void al_weight_kernel(const unsigned long long* __restrict__ items, long long n_items, const long long* __restrict__ off,
                                 const int* __restrict__ best, const long long* __restrict__ roff, const unsigned long long* __restrict__ cstart, int n_contigs,
                                 int W, const unsigned* __restrict__ upos, const unsigned long long* __restrict__ upre, long long n_unique,
                                 unsigned long long* __restrict__ w) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n_items; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long it = items[i];
        const long long r = (long long)(it >> 33);
        unsigned long long wi = 0;
        if (best[r] >= 0 && off[r + 1] - off[r] > 1) {
            const unsigned long long g = (it >> 1) & 0xffffffffull;
            const unsigned long long L = (unsigned long long)(roff[r + 1] - roff[r]);
            const int a = site_contig(cstart, n_contigs, g);
            const unsigned long long c0 = cstart[a], c1 = cstart[a + 1];                  // the contig is [c0, c1)
            const unsigned long long lo = g - c0 > (unsigned long long)W ? g - W : c0;
            const unsigned long long hi = g + L + W < c1 ? g + L + W : c1;               // one past the last position counted
            wi = upre[al_ulower(upos, n_unique, hi)] - upre[al_ulower(upos, n_unique, lo)];
        }
        w[i] = wi;
    }
}

// FNV-1a-64 over the read's codes, xor seed, splitmix64 finaliser
__device__ __forceinline__ unsigned long long al_draw(const unsigned char* __restrict__ rd, int L, unsigned long long seed) {
    unsigned long long x = 0xcbf29ce484222325ull;
    for (int i = 0; i < L; i++) { x ^= rd[i]; x *= 0x100000001b3ull; }
    x ^= seed;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// per read: the one item that is reported (AL_NO_ITEM: none), n, class, w of the chosen hit and Wt; counts += {unique, by density, at random}
__global__ void al_pick_kernel(const unsigned long long* __restrict__ items, const long long* __restrict__ off, const int* __restrict__ best,
                               const unsigned char* __restrict__ codes, const long long* __restrict__ roff, long long n, int mode, unsigned long long seed,
                               const unsigned long long* __restrict__ w, unsigned long long* __restrict__ pick, int* __restrict__ pn,
                               unsigned char* __restrict__ pcls, unsigned long long* __restrict__ pw, unsigned long long* __restrict__ pwt,
                               unsigned long long* __restrict__ counts) {
    unsigned long long cnt[3] = {0, 0, 0};
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const long long o = off[r], nh = off[r + 1] - o;
        unsigned long long it = AL_NO_ITEM, wc = 0, wt = 0;
        unsigned char cls = 'N';
        if (best[r] < 0 || nh == 1) {
            if (nh > 0) it = items[o];
            if (best[r] >= 0) cnt[0]++;
        } else {
            const unsigned long long x = al_draw(codes + roff[r], (int)(roff[r + 1] - roff[r]), seed);
            long long idx = -1;
            if (mode == 1) {
                for (long long i = 0; i < nh; i++) wt += w[o + i];
                if (wt > 0) {
                    const unsigned long long t = x % wt;
                    unsigned long long run = 0;
                    for (long long i = 0; i < nh; i++) {
                        run += w[o + i];
                        if (run > t) { idx = i; break; }
                    }
                    wc = w[o + idx];
                    cls = 'U';
                }
            }
            if (idx < 0) { idx = (long long)(x % (unsigned long long)nh); cls = 'R'; if (mode == 1) wc = 0; }
            it = items[o + idx];
            cnt[cls == 'U' ? 1 : 2]++;
        }
        pick[r] = it;
        pn[r] = (int)nh;
        pcls[r] = cls;
        pw[r] = wc;
        pwt[r] = wt;
    }
    for (int i = 0; i < 3; i++) al_wave_add(&counts[i], cnt[i]);
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

// A batch of reads runs in three steps that share the context's a_* buffers: upload, hits (seeds .. sort) and emit (size, scan, emit, download).
// mirp_align_reads runs them back to back; the placement (mirp_align_reads_placed) runs upload + hits of every batch first, then the placing
// and the emit.  seconds += [0] upload, [1] seeds, [2] verify, [3] sort, [4] emit, [5] the tail pass (mirp_align_reads_tailed).

// Upload: codes (0..3 ACGT, 4 other) at roff[0..n], QNAMEs at qoff[0..n], depth[0..n) (placement only, or null), all on the host.
int mirp_device_align_upload(mirp_ctx* c, const unsigned char* codes, const long long* roff, const char* qn, const long long* qoff, const unsigned* depth,
                             long long n, double seconds[5]) {
    if (!c->a_ready) return fail(c, -1, "mirp_align_reads: no index (mirp_align_index first)");
    hipStream_t st = c->stream;
    double t = mirp::now();
    const long long nb = roff[n], nq = qoff[n];
    if (c->a_codes.ensure((size_t)nb + 16) || c->a_roff.ensure(8 * (size_t)(n + 1)) || c->a_qn.ensure((size_t)nq + 16) || c->a_qoff.ensure(8 * (size_t)(n + 1)) ||
        c->a_small.ensure(128) || (depth && c->a_depth.ensure(4 * (size_t)n)))
        return fail(c, -6, "device allocation failed (align: reads)");
    if (nb) HIPCHK(c, hipMemcpyAsync(c->a_codes.p, codes, (size_t)nb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_roff.p, roff, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    if (nq) HIPCHK(c, hipMemcpyAsync(c->a_qn.p, qn, (size_t)nq, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_qoff.p, qoff, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    if (depth) HIPCHK(c, hipMemcpyAsync(c->a_depth.p, depth, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    // a_small: [0..2] aligned / unaligned / suppressed, [3] records, [4] overflow flag, [5..7] placed unique / by density / at random,
    // [8..9] tailed / suppressed in the tail pass (both are counted in [1] as well: mirp_align.cpp moves them)
    HIPCHK(c, hipMemsetAsync(c->a_small.p, 0, 128, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] += mirp::now() - t;
    return 0;
}

// Hits of the uploaded batch: a_items = the *n_items sorted best-stratum items (and one item per unaligned read unless filter), a_off their
// per-read offsets, a_best / a_supp the per-read stratum and -m decision; a_small[0..2] += {aligned, unaligned, suppressed}.  With tail (max_tail
// > 0) the reads left without a hit go through the tail search (align_tail_kernels.hip) between the strata and the offsets: a tailed read gets
// best = 0, its stratum's hits as items and a_tt[read] = its tail length; seconds[5] += the tail pass.
int mirp_device_align_hits(mirp_ctx* c, long long n, int v, int m, int filter, const MirpAlignTailOpts* tail, long long* n_items, double seconds[6]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const AlParams P{v, v / 2, 1, m, filter, 0};
    const AlRef R = al_ref(c);
    unsigned long long* d_small = (unsigned long long*)c->a_small.p;
    const unsigned char* d_codes = (const unsigned char*)c->a_codes.p;
    const long long* d_roff = (const long long*)c->a_roff.p;
    const int g = al_grid(n);

    // ---- seeds
    double t = mirp::now();
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
    double tail_sec = 0;
    if (tail && tail->max_tail > 0) {
        HIPCHK(c, hipStreamSynchronize(st));             // the counts and strata above belong to the verify phase
        const double t0 = mirp::now();
        if (int rc = mirp_device_align_tail_strata(c, n, *tail, m)) return rc;
        tail_sec += mirp::now() - t0;
    }
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
    if (tail && tail->max_tail > 0) {
        const double t0 = mirp::now();
        if (int rc = mirp_device_align_tail_hits(c, *tail)) return rc;
        tail_sec += mirp::now() - t0;
        seconds[5] += tail_sec;
    }
    seconds[2] += mirp::now() - t - tail_sec;

    // ---- order: by (read, gpos, strand)
    t = mirp::now();
    int rbits = 0;
    while ((1ll << rbits) < n) rbits++;
    if (int rc = mirp_device_sort_u64(c, d_items, (unsigned long long*)c->a_itmp.p, NI, 0, (33 + rbits + 7) / 8 * 8)) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[3] += mirp::now() - t;
    *n_items = NI;
    return 0;
}

// Emit + download: the records of the batch's items go to `sink` in pieces of at most 1 GiB.  place = 0: the n_items items of
// mirp_device_align_hits, the first k of every read.  place != 0: the picks of mirp_device_place_pick, one per read, with the placement tags.
// cnt[0..8) = a_small after the batch ({aligned, unaligned, suppressed, records, -, placed unique, by density, at random}).  tail: the options the
// batch's hits were made with (null: none); the records of its tailed reads take the tailed form.
int mirp_device_align_emit(mirp_ctx* c, long long n, long long n_items, int v, int k, int m, int filter, int place, const MirpAlignTailOpts* tail,
                           const std::function<int(const char*, size_t)>& sink, unsigned long long cnt[8], double seconds[6]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const bool tailed = tail && tail->max_tail > 0;
    const AlParams P{v, v / 2, k, m, filter, place, tailed && tail->trim ? 1 : 0};
    const AlRef R = al_ref(c);
    unsigned long long* d_small = (unsigned long long*)c->a_small.p;
    const unsigned long long* d_items = (const unsigned long long*)(place ? c->a_pick.p : c->a_items.p);
    const long long NI = place ? n : n_items;
    double t = mirp::now();
    if (c->a_size.ensure(4 * (size_t)std::max<long long>(NI, 1)) || c->a_toff.ensure(8 * (size_t)(NI + 1)))
        return fail(c, -6, "device allocation failed (align: text offsets)");
    const AlText TX{(const unsigned char*)c->a_codes.p, (const long long*)c->a_roff.p, (const char*)c->a_qn.p, (const long long*)c->a_qoff.p,
                    (const char*)c->a_names.p, (const long long*)c->a_noff.p, (const unsigned long long*)c->a_cstart.p, c->a_n_contigs,
                    (const int*)c->a_pn.p, (const unsigned char*)c->a_pcls.p, (const unsigned long long*)c->a_pw.p, (const unsigned long long*)c->a_pwt.p,
                    tailed ? (const unsigned char*)c->a_tt.p : nullptr};
    const long long* d_off = (const long long*)c->a_off.p;
    const int* d_best = (const int*)c->a_best.p;
    const int* d_supp = (const int*)c->a_supp.p;
    long long* d_toff = (long long*)c->a_toff.p;
    long long bytes = 0;
    if (NI > 0) {
        hipLaunchKernelGGL(al_size_kernel, dim3(al_grid(NI)), dim3(256), 0, st, R, TX, P, d_items, NI, d_off, d_best, d_supp, (int*)c->a_size.p, d_small + 3);
        launch_excl_scan(st, (const int*)c->a_size.p, d_toff, NI);
        HIPCHK(c, hipMemcpyAsync(&bytes, d_toff + NI, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    if (c->a_text.ensure((size_t)bytes + 16)) return fail(c, -6, "device allocation failed (align: text)");
    if (NI > 0)
        hipLaunchKernelGGL(al_emit_kernel, dim3(al_grid(NI)), dim3(256), 0, st, R, TX, P, d_items, NI, (const long long*)d_toff, d_best, d_supp,
                           (char*)c->a_text.p);
    HIPCHK(c, hipMemcpyAsync(cnt, d_small, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (int rc = mirp_download_text(c, (const char*)c->a_text.p, bytes, sink)) return rc;
    seconds[4] += mirp::now() - t;
    return 0;
}

// ---------------------------------------------------------------- placement, host side
// Appends the unique reads of the batch whose hits are resident to the context's unique list (a_ulist, *n_unique entries before and after).
int mirp_device_place_unique(mirp_ctx* c, long long n, long long* n_unique) {
    using namespace mirp;
    hipStream_t st = c->stream;
    if (n <= 0) return 0;
    int* d_flag = (int*)c->a_rcnt.p;                    // the seed counts and their scan are done with
    long long* d_uscan = (long long*)c->a_rscan.p;
    const int g = al_grid(n);
    hipLaunchKernelGGL(al_unique_kernel<false>, dim3(g), dim3(256), 0, st, (const unsigned long long*)c->a_items.p, (const long long*)c->a_off.p,
                       (const int*)c->a_best.p, n, (const unsigned*)c->a_depth.p, d_flag, (const long long*)nullptr, (unsigned long long*)nullptr);
    launch_excl_scan(st, d_flag, d_uscan, n);
    long long add = 0;
    HIPCHK(c, hipMemcpyAsync(&add, d_uscan + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const size_t need = 8 * (size_t)(*n_unique + add);
    if (need > c->a_ulist.cap) {                        // grow and keep what the earlier batches wrote
        DevBuf bigger;
        if (bigger.ensure(std::max(need, 2 * c->a_ulist.cap))) return fail(c, -6, "device allocation failed (align: unique reads)");
        if (*n_unique) HIPCHK(c, hipMemcpyAsync(bigger.p, c->a_ulist.p, 8 * (size_t)*n_unique, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        std::swap(bigger.p, c->a_ulist.p);
        std::swap(bigger.cap, c->a_ulist.cap);
    }
    if (add > 0)
        hipLaunchKernelGGL(al_unique_kernel<true>, dim3(g), dim3(256), 0, st, (const unsigned long long*)c->a_items.p, (const long long*)c->a_off.p,
                           (const int*)c->a_best.p, n, (const unsigned*)c->a_depth.p, (int*)nullptr, (const long long*)d_uscan,
                           (unsigned long long*)c->a_ulist.p + *n_unique);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    *n_unique += add;
    return 0;
}

// After the last batch: sorts the unique list by position and builds a_upos[n_unique] and the exact 64-bit prefix a_upre[n_unique + 1] of the depths.
int mirp_device_place_prepare(mirp_ctx* c, long long n_unique, unsigned long long* depth_sum) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long NU = n_unique;
    const size_t one = (size_t)std::max<long long>(NU, 1);
    if (c->a_ulist.ensure(8) || c->a_utmp.ensure(8 * one) || c->a_upos.ensure(4 * one) || c->a_ulo.ensure(4 * one) || c->a_uhi.ensure(4 * one) ||
        c->a_uls.ensure(8 * (one + 1)) || c->a_uhs.ensure(8 * (one + 1)) || c->a_upre.ensure(8 * (one + 1)))
        return fail(c, -6, "device allocation failed (align: unique reads)");
    *depth_sum = 0;
    if (NU == 0) {
        HIPCHK(c, hipMemsetAsync(c->a_upre.p, 0, 8, st));
        HIPCHK(c, hipStreamSynchronize(st));
        return 0;
    }
    if (int rc = mirp_device_sort_u64(c, (unsigned long long*)c->a_ulist.p, (unsigned long long*)c->a_utmp.p, NU, 32, 32)) return rc;
    hipLaunchKernelGGL(al_usplit_kernel, dim3(al_grid(NU)), dim3(256), 0, st, (const unsigned long long*)c->a_ulist.p, NU, (unsigned*)c->a_upos.p,
                       (int*)c->a_ulo.p, (int*)c->a_uhi.p);
    launch_excl_scan(st, (const int*)c->a_ulo.p, (long long*)c->a_uls.p, NU);
    launch_excl_scan(st, (const int*)c->a_uhi.p, (long long*)c->a_uhs.p, NU);
    hipLaunchKernelGGL(al_uprefix_kernel, dim3(al_grid(NU + 1)), dim3(256), 0, st, (const long long*)c->a_uls.p, (const long long*)c->a_uhs.p, NU,
                       (unsigned long long*)c->a_upre.p);
    HIPCHK(c, hipMemcpyAsync(depth_sum, (unsigned long long*)c->a_upre.p + NU, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Places the reads of the batch whose hits are resident: a_pick (one item per read) and the tag fields; a_small[5..7] += the class counts.
int mirp_device_place_pick(mirp_ctx* c, long long n, long long n_items, int mode, int window, unsigned long long seed, long long n_unique) {
    using namespace mirp;
    hipStream_t st = c->stream;
    if (n <= 0) return 0;
    if (c->a_w.ensure(8 * (size_t)std::max<long long>(n_items, 1)) || c->a_pick.ensure(8 * (size_t)n) || c->a_pn.ensure(4 * (size_t)n) ||
        c->a_pcls.ensure((size_t)n) || c->a_pw.ensure(8 * (size_t)n) || c->a_pwt.ensure(8 * (size_t)n))
        return fail(c, -6, "device allocation failed (align: placement)");
    if (mode == 1 && n_items > 0)
        hipLaunchKernelGGL(al_weight_kernel, dim3(al_grid(n_items)), dim3(256), 0, st, (const unsigned long long*)c->a_items.p, n_items,
                           (const long long*)c->a_off.p, (const int*)c->a_best.p, (const long long*)c->a_roff.p, (const unsigned long long*)c->a_cstart.p,
                           c->a_n_contigs, window, (const unsigned*)c->a_upos.p, (const unsigned long long*)c->a_upre.p, n_unique,
                           (unsigned long long*)c->a_w.p);
    hipLaunchKernelGGL(al_pick_kernel, dim3(al_grid(n)), dim3(256), 0, st, (const unsigned long long*)c->a_items.p, (const long long*)c->a_off.p,
                       (const int*)c->a_best.p, (const unsigned char*)c->a_codes.p, (const long long*)c->a_roff.p, n, mode, seed,
                       (const unsigned long long*)c->a_w.p, (unsigned long long*)c->a_pick.p, (int*)c->a_pn.p, (unsigned char*)c->a_pcls.p,
                       (unsigned long long*)c->a_pw.p, (unsigned long long*)c->a_pwt.p, (unsigned long long*)c->a_small.p + 5);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

