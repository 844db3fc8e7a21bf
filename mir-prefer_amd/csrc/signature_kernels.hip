// siRNA duplexes and the 5' overlap signature on given loci, on the context's resident alignments (mirp_signature_scan).  The host
// (signature.py) reads the interval file, derives the peak, z-score and fraction and writes the files; everything per record, per locus, per
// 5' end and per placement runs here.
//
// A kept record (min_len <= len <= max_len) belongs to a locus by its 5' end f (pos on '+', pos + len - 1 on '-').  The join of the two strands
// needs the records ordered by f, which the resident (tid, pos) order is not for '-', so the call builds three tables once, not per locus:
//   keys     sg_key_kernel keys every record twice: strand | tid | f for the 5' ends and, as lc_key_kernel does, (first record of its (tid, pos)
//            run) << 17 | strand << 16 | len for the placements.  A record that is not kept, or whose 5' end lies outside its contig (no locus
//            can hold it), gets a key above every real one; it sorts behind the tables, which saves a compaction.
//   tables   mirp_device_sort_hashes, sg_run_kernel (run heads, depths split at bit 30), three scans (cl_prefix) and sg_ends_kernel /
//            sg_place_kernel compact the runs: U and V in one table {tid << 32 | f, 64-bit depth sum}, V behind U (the strand is the top key bit),
//            and the placement table {tid << 32 | pos, strand << 16 | len, sum} in (tid, pos, strand, len) order.
//   partner  sg_pair_kernel, one lane per '+' placement (p, L): one binary search for (tid, p - overhang, '-', L); the partner's row and whether
//            m = min of the two sums reaches min_reads are kept per row, and one scan counts the listed rows before every row.
//   ranges   lc_range_kernel (loci_device.h) twice: the U entries with f in [start, end], and the placements with pos in
//            [start - max_len + 1, end], which hold every placement whose 5' end is in the locus; ceil(range / C) jobs each, one scan per table.
//   overlap  sg_overlap_kernel, one wave per (locus, chunk of C U entries) on a capped resident grid, wave w serving jobs w, w + waves, ...:
//            a lane takes one U entry x, finds the first V entry >= x by one binary search and walks at most K entries forward while
//            y <= min(x + K - 1, end).  min(U, V) is added to the job's H in LDS (one 64-bit counter per overlap and wave); the job leaves with
//            one global atomic per overlap that is not zero.
//   duplex   sg_duplex_kernel, one wave per (locus, chunk of C placements), two passes: <0> sums reads and plus reads, counts the duplexes and
//            the listed ones, sums m and takes its atomicMax; <1> the atomicMin of the row among the duplexes that reach the maximum = the
//            tie rule (smallest p, then the shorter L).
//   out      sg_out_kernel writes one MirpSignatureRow per locus and the listed count as the input of the scan that places the loci in the list.
//   emit     sg_emit_kernel, the jobs of the duplex kernel again: a job's place inside its locus is the number of listed duplexes of the locus
//            before the job's first row.  Only the right locus edge can exclude a listed row (p - overhang + L - 1 <= end), and only among the
//            rows with p > end - (max_len - 1 - overhang); before them the count is a difference of the scan, the few rows behind are counted by
//            the wave.  Inside a job the ballots of 64 rows give the ranks, so the list's order (locus, p, L) follows from the layout.
// Every sum, maximum and minimum is an integer atomic, so no result depends on scheduling; no lane loops over a locus alone.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "mirp_ctx.h"
#include "loci_device.h"
#include "wave_atomic.h"

namespace mirp {

static_assert(MIRP_SIGNATURE_CHUNK == LC_C, "lc_range_kernel cuts the ranges into the jobs of this scan");
static_assert(MIRP_SIGNATURE_MAX_OVERLAP == 64, "one lane per overlap carries a job's H out of LDS");

#define SG_K MIRP_SIGNATURE_MAX_OVERLAP

struct SgOpts {
    int n_contigs, min_len, max_len, K, overhang, tid_bits;
    long long min_reads;
};

__device__ __forceinline__ void sg_sync() {       // the wave's LDS traffic before this point is done before any after it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ends: strand << (31 + tid_bits) | tid << 31 | f, idx = depth; placements: lc_key_kernel's key; cnt[0] = the kept records
__global__ void __launch_bounds__(CL_NT) sg_key_kernel(const MirpAln* __restrict__ a, long long n, const long long* __restrict__ clen, SgOpts O,
                                                       MirpHashRec* __restrict__ ends, MirpHashRec* __restrict__ places, unsigned long long* __restrict__ cnt) {
    unsigned long long kept = 0;
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < n; i += (long long)gridDim.x * CL_NT) {
        const MirpAln r = a[i];
        const bool len_ok = (int)r.len >= O.min_len && (int)r.len <= O.max_len;
        const long long f = r.strand ? (long long)r.pos + (long long)r.len - 1 : (long long)r.pos;
        const bool on = len_ok && r.tid >= 0 && r.tid < O.n_contigs && f >= 1 && f <= clen[r.tid];
        kept += len_ok ? 1 : 0;
        MirpHashRec e, p;
        e.hash = 2ull << (31 + O.tid_bits);
        p.hash = (unsigned long long)n << 17;
        e.idx = p.idx = 0;
        e.pad = p.pad = 0;
        if (on) {
            const long long k = lc_key(a, i);
            long long lo = 0, hi = i;                  // first record of this (tid, pos)
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (lc_key(a, mid) < k) lo = mid + 1;
                else hi = mid;
            }
            e.hash = ((unsigned long long)(r.strand ? 1 : 0) << (31 + O.tid_bits)) | ((unsigned long long)r.tid << 31) | (unsigned long long)f;
            p.hash = ((unsigned long long)lo << 17) | ((unsigned long long)(r.strand ? 1 : 0) << 16) | (unsigned long long)r.len;
            e.idx = p.idx = r.depth;
        }
        ends[i] = e;
        places[i] = p;
    }
    cl_wave_atomic<0>(cnt, kept ? 0 : -1, kept);
}

// depth of every sorted key split at bit 30 (for the two exact scans) and the heads of the runs below the key `none`
__global__ void __launch_bounds__(CL_NT) sg_run_kernel(const MirpHashRec* __restrict__ p, long long n, unsigned long long none, int* __restrict__ lo,
                                                       int* __restrict__ hi, int* __restrict__ head) {
    for (long long j = (long long)blockIdx.x * CL_NT + threadIdx.x; j < n; j += (long long)gridDim.x * CL_NT) {
        const unsigned d = p[j].idx;
        lo[j] = (int)(d & 0x3fffffffu);
        hi[j] = (int)(d >> 30);
        head[j] = p[j].hash < none && (j == 0 || p[j - 1].hash != p[j].hash);
    }
}

// U and V: row hs[j] of every run head j = {tid << 32 | f, the run's depth sum}; cnt[1] = the rows of U
__global__ void __launch_bounds__(CL_NT) sg_ends_kernel(const MirpHashRec* __restrict__ p, long long n, const int* __restrict__ head,
                                                        const long long* __restrict__ hs, const long long* __restrict__ slo,
                                                        const long long* __restrict__ shi, int tid_bits, long long* __restrict__ ekey,
                                                        unsigned long long* __restrict__ esum, unsigned long long* __restrict__ cnt) {
    unsigned long long plus = 0;
    for (long long j = (long long)blockIdx.x * CL_NT + threadIdx.x; j < n; j += (long long)gridDim.x * CL_NT) {
        if (!head[j]) continue;
        const unsigned long long h = p[j].hash;
        const long long e = cl_upper_rec(p, j + 1, n, h);
        const long long t = hs[j];
        const long long tid = (long long)((h >> 31) & ((1ull << tid_bits) - 1));
        ekey[t] = (tid << 32) + (long long)(h & 0x7fffffffull);
        esum[t] = (unsigned long long)(cl_prefix(slo, shi, e) - cl_prefix(slo, shi, j));
        plus += (h >> (31 + tid_bits)) ? 0 : 1;
    }
    cl_wave_atomic<0>(cnt, plus ? 1 : -1, plus);
}

// placement table: row hs[j] of every run head j = {tid << 32 | pos, strand << 16 | len, the run's depth sum}
__global__ void __launch_bounds__(CL_NT) sg_place_kernel(const MirpAln* __restrict__ a, const MirpHashRec* __restrict__ p, long long n,
                                                         const int* __restrict__ head, const long long* __restrict__ hs,
                                                         const long long* __restrict__ slo, const long long* __restrict__ shi,
                                                         long long* __restrict__ pkey, unsigned* __restrict__ pmeta, unsigned long long* __restrict__ psum) {
    for (long long j = (long long)blockIdx.x * CL_NT + threadIdx.x; j < n; j += (long long)gridDim.x * CL_NT) {
        if (!head[j]) continue;
        const unsigned long long h = p[j].hash;
        const long long e = cl_upper_rec(p, j + 1, n, h);
        const long long t = hs[j];
        pkey[t] = lc_key(a, (long long)(h >> 17));
        pmeta[t] = (unsigned)(h & 0x1ffffu);
        psum[t] = (unsigned long long)(cl_prefix(slo, shi, e) - cl_prefix(slo, shi, j));
    }
}

// partner[t] = the row of (tid, p - overhang, '-', L) for the '+' row t = (tid, p, L), -1 without one; listed[t] = m >= min_reads
__global__ void __launch_bounds__(CL_NT) sg_pair_kernel(const long long* __restrict__ pkey, const unsigned* __restrict__ pmeta,
                                                        const unsigned long long* __restrict__ psum, long long np, int overhang, long long min_reads,
                                                        int* __restrict__ partner, int* __restrict__ listed) {
    for (long long t = (long long)blockIdx.x * CL_NT + threadIdx.x; t < np; t += (long long)gridDim.x * CL_NT) {
        const unsigned m = pmeta[t];
        int at = -1, ls = 0;
        if ((m >> 16) == 0) {
            const long long k = pkey[t] - overhang;
            const unsigned want = m | 0x10000u;
            long long lo = 0, hi = np;                 // first row >= (k, want)
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                const long long km = pkey[mid];
                if (km < k || (km == k && pmeta[mid] < want)) lo = mid + 1;
                else hi = mid;
            }
            if (lo < np && pkey[lo] == k && pmeta[lo] == want) {
                at = (int)lo;
                ls = (long long)std::min(psum[t], psum[lo]) >= min_reads ? 1 : 0;
            }
        }
        partner[t] = at;
        listed[t] = ls;
    }
}

struct SgSums {
    unsigned long long *reads, *plus, *duplexes, *dreads, *nlisted, *cmax, *cmaj;   // [nl] each
    unsigned long long* H;                                                           // [nl * K]
};

__global__ void __launch_bounds__(CL_NT) sg_overlap_kernel(const long long* __restrict__ ukey, const unsigned long long* __restrict__ usum,
                                                           const long long* __restrict__ vkey, const unsigned long long* __restrict__ vsum, long long nv,
                                                           const MirpLocusSpan* __restrict__ loci, long long nl, const long long* __restrict__ first,
                                                           const long long* __restrict__ last, const long long* __restrict__ joff, long long n_jobs,
                                                           int K, unsigned long long* __restrict__ H) {
    __shared__ unsigned long long acc[LC_WAVES][SG_K];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long waves = (long long)gridDim.x * LC_WAVES;
    acc[w][lane] = 0;
    sg_sync();
    for (long long j = (long long)blockIdx.x * LC_WAVES + w; j < n_jobs; j += waves) {
        const long long q = lc_job_locus(joff, nl, j);
        const long long end = lc_locus(loci[q]).hi;
        const long long b = first[q] + (j - joff[q]) * LC_C;
        const long long e = std::min(b + LC_C, last[q]);
        for (long long i = b + lane; i < e; i += 64) {
            const long long x = ukey[i];
            const unsigned long long du = usum[i];
            const long long top = std::min(x + K - 1, end);
            long long lo = 0, hi = nv;                 // first V entry >= x
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (vkey[mid] < x) lo = mid + 1;
                else hi = mid;
            }
            for (; lo < nv; lo++) {                    // at most K entries: the keys of V are distinct
                const long long y = vkey[lo];
                if (y > top) break;
                const unsigned long long m = std::min(du, vsum[lo]);
                if (m) atomicAdd(&acc[w][(int)(y - x)], m);
            }
        }
        sg_sync();
        const unsigned long long h = acc[w][lane];
        acc[w][lane] = 0;
        if (lane < K && h) atomicAdd(&H[q * K + lane], h);
        sg_sync();
    }
}

// is the '+' row (key k, length len) with a partner a duplex of the locus?  Its own 5' end is inside; the partner's is p - overhang + L - 1 >= p.
__device__ __forceinline__ bool sg_inside(const LcLocus& L, long long k, int len, int overhang) { return k - overhang + len - 1 <= L.hi; }

template <int PASS>
__global__ void __launch_bounds__(CL_NT) sg_duplex_kernel(const long long* __restrict__ pkey, const unsigned* __restrict__ pmeta,
                                                          const unsigned long long* __restrict__ psum, const int* __restrict__ partner,
                                                          const int* __restrict__ listed, const MirpLocusSpan* __restrict__ loci, long long nl,
                                                          const long long* __restrict__ first, const long long* __restrict__ last,
                                                          const long long* __restrict__ joff, long long n_jobs, int overhang, SgSums S) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * LC_WAVES;
    for (long long j = (long long)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); j < n_jobs; j += waves) {
        const long long q = lc_job_locus(joff, nl, j);
        const LcLocus L = lc_locus(loci[q]);
        const long long b = first[q] + (j - joff[q]) * LC_C;
        const long long e = std::min(b + LC_C, last[q]);
        unsigned long long reads = 0, plus = 0, dup = 0, dreads = 0, nls = 0, best = 0, at = ~0ull;
        const unsigned long long cmax = PASS ? S.cmax[q] : 0;
        for (long long i = b + lane; i < e; i += 64) {
            const long long k = pkey[i];
            const unsigned m = pmeta[i];
            const int len = (int)(m & 0xffffu);
            const long long f = (m >> 16) ? k + len - 1 : k;
            if (f < L.lo || f > L.hi) continue;
            const unsigned long long d = psum[i];
            if (PASS == 0) {
                reads += d;
                plus += (m >> 16) ? 0ull : d;
            }
            const int pt = partner[i];
            if (pt < 0 || !sg_inside(L, k, len, overhang)) continue;
            const unsigned long long mm = std::min(d, psum[pt]);
            if (PASS == 0) {
                dup++;
                dreads += mm;
                nls += (unsigned long long)listed[i];
                best = std::max(best, mm);
            } else if (mm == cmax) {
                at = std::min(at, (unsigned long long)i);
            }
        }
        if (PASS == 0) {
            cl_wave_atomic<0>(S.reads, reads ? q : -1, reads);
            cl_wave_atomic<0>(S.plus, plus ? q : -1, plus);
            cl_wave_atomic<0>(S.duplexes, dup ? q : -1, dup);
            cl_wave_atomic<0>(S.dreads, dreads ? q : -1, dreads);
            cl_wave_atomic<0>(S.nlisted, nls ? q : -1, nls);
            cl_wave_atomic<1>(S.cmax, dup ? q : -1, best);
        } else {
            cl_wave_atomic<2>(S.cmaj, at != ~0ull ? q : -1, at);
        }
    }
}

__global__ void __launch_bounds__(CL_NT) sg_out_kernel(long long nl, SgSums S, const long long* __restrict__ pkey, const unsigned* __restrict__ pmeta,
                                                       const unsigned long long* __restrict__ psum, const int* __restrict__ partner,
                                                       MirpSignatureRow* __restrict__ out, int* __restrict__ nsites) {
    for (long long q = (long long)blockIdx.x * CL_NT + threadIdx.x; q < nl; q += (long long)gridDim.x * CL_NT) {
        MirpSignatureRow o;
        o.reads = (long long)S.reads[q];
        o.plus_reads = (long long)S.plus[q];
        o.duplexes = (long long)S.duplexes[q];
        o.duplex_reads = (long long)S.dreads[q];
        o.major_pos = o.major_plus = o.major_minus = 0;
        o.major_len = o.reserved = 0;
        if (S.duplexes[q]) {
            const unsigned long long m = S.cmaj[q];
            o.major_pos = (long long)(int)(pkey[m] & 0xffffffffll);
            o.major_plus = (long long)psum[m];
            o.major_minus = (long long)psum[partner[m]];
            o.major_len = (int)(pmeta[m] & 0xffffu);
        }
        out[q] = o;
        nsites[q] = (int)S.nlisted[q];                 // at most the rows of the placement table, which are fewer than 2^31
    }
}

__global__ void __launch_bounds__(CL_NT) sg_emit_kernel(const long long* __restrict__ pkey, const unsigned* __restrict__ pmeta,
                                                        const unsigned long long* __restrict__ psum, const int* __restrict__ partner,
                                                        const int* __restrict__ listed, const long long* __restrict__ lscan,
                                                        const MirpLocusSpan* __restrict__ loci, long long nl, const long long* __restrict__ first,
                                                        const long long* __restrict__ last, const long long* __restrict__ joff, long long n_jobs,
                                                        int overhang, int max_len, const long long* __restrict__ sbase, MirpDuplexSite* __restrict__ sites) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    const long long waves = (long long)gridDim.x * LC_WAVES;
    for (long long j = (long long)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); j < n_jobs; j += waves) {
        const long long q = lc_job_locus(joff, nl, j);
        if (sbase[q + 1] == sbase[q]) continue;                      // the same for every lane of the wave
        const LcLocus L = lc_locus(loci[q]);
        const long long z = last[q];
        const long long b = first[q] + (j - joff[q]) * LC_C;
        const long long e = std::min(b + LC_C, z);
        long long lo = first[q], hi = z;                             // in: the first row with p >= start
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (pkey[mid] < L.lo) lo = mid + 1;
            else hi = mid;
        }
        const long long in = lo;
        const long long sure = L.hi - (max_len - 1 - overhang);     // a row with p <= sure has its partner's 5' end inside
        hi = z;                                                      // edge: the first row with p > sure
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (pkey[mid] <= sure) lo = mid + 1;
            else hi = mid;
        }
        const long long edge = lo;
        auto site = [&](long long i, long long stop) {
            if (i >= stop || !listed[i]) return false;
            const long long k = pkey[i];
            return k >= L.lo && k <= L.hi && sg_inside(L, k, (int)(pmeta[i] & 0xffffu), overhang);
        };
        long long at = sbase[q] + lscan[std::min(std::max(b, in), edge)] - lscan[in];
        for (long long base = edge; base < b; base += 64) at += __popcll(__ballot(site(base + lane, b)));
        for (long long base = b; base < e; base += 64) {             // the same trip count in every lane
            const long long i = base + lane;
            const bool ok = site(i, e);
            const unsigned long long mask = __ballot(ok);
            if (ok) {
                MirpDuplexSite s;
                s.locus = q;
                s.pos = (long long)(int)(pkey[i] & 0xffffffffll);
                s.plus_reads = (long long)psum[i];
                s.minus_reads = (long long)psum[partner[i]];
                s.len = (int)(pmeta[i] & 0xffffu);
                s.reserved = 0;
                sites[at + __popcll(mask & below)] = s;
            }
            at += __popcll(mask);
        }
    }
}

}  // namespace mirp

extern "C" int mirp_signature_scan(mirp_ctx* c, const MirpLocusSpan* loci, int64_t n_loci, const MirpSignatureOpts* o, MirpSignatureRow** rows,
                                   int64_t** overlaps, MirpDuplexSite** sites, int64_t* n_sites, int64_t stats[6]) {
    using namespace mirp;
    if (!c) return -1;
    if (!o || !rows || !overlaps || !sites || !n_sites || (n_loci > 0 && !loci) || (o->n_contigs > 0 && !o->contig_len))
        return fail(c, -1, "mirp_signature_scan: bad argument");
    if (n_loci < 0 || n_loci > MIRP_LOCI_MAX || o->n_contigs < 0 || o->min_len < 1 || o->min_len > o->max_len || o->max_len > 65535 || o->max_overlap < 1 ||
        o->max_overlap > MIRP_SIGNATURE_MAX_OVERLAP || o->overhang < 0 || o->overhang > 8 || o->overhang >= o->min_len || o->min_reads < 1)
        return fail(c, -1, "mirp_signature_scan: bad options");
    for (int t = 0; t < o->n_contigs; t++)
        if (o->contig_len[t] < 0 || o->contig_len[t] > 0x7fffffffll) return fail(c, -1, "mirp_signature_scan: a contig length outside 0..2^31 - 1");
    for (long long q = 0; q < n_loci; q++) {
        const MirpLocusSpan& l = loci[q];
        if (l.tid < 0 || l.tid >= o->n_contigs || l.start < 1 || l.start > l.end || l.end > o->contig_len[l.tid])
            return fail(c, -1, "mirp_signature_scan: locus " + std::to_string(q + 1) + " is not an interval of a contig");
    }
    *rows = nullptr;
    *overlaps = nullptr;
    *sites = nullptr;
    *n_sites = 0;
    c->reset_jobs_per_slot(7);
    const long long n = c->n_alns, nl = n_loci;
    const int K = o->max_overlap;
    if (n > (1ll << 31) - 2) return fail(c, -5, "mirp_signature_scan: more than 2^31 records");
    MirpSignatureRow* h_rows = (MirpSignatureRow*)std::calloc((size_t)std::max(nl, 1ll), sizeof(MirpSignatureRow));
    int64_t* h_H = (int64_t*)std::calloc((size_t)std::max(nl * K, 1ll), 8);
    MirpDuplexSite* h_sites = nullptr;
    auto give_up = [&](int rc) {
        std::free(h_rows);
        std::free(h_H);
        std::free(h_sites);
        return rc;
    };
    if (!h_rows || !h_H) return give_up(fail(c, -6, "host allocation failed (signature scan)"));
    long long ujobs = 0, pjobs = 0, nuv = 0, np = 0, ns = 0;
    unsigned long long h_cnt[2] = {0, 0};                    // kept records, rows of U
    if (n > 0 && nl > 0) {
        // the device work in a function of its own, so that HIPCHK's early returns free the host results
        auto run = [&]() -> int {
            HIPCHK(c, hipSetDevice(c->device));
            const hipStream_t st = c->stream;
            const MirpAln* alns = (const MirpAln*)c->alns.p;
            SgOpts O;
            O.n_contigs = o->n_contigs;
            O.min_len = o->min_len;
            O.max_len = o->max_len;
            O.K = K;
            O.overhang = o->overhang;
            O.tid_bits = lc_bits((long long)o->n_contigs - 1);
            O.min_reads = o->min_reads;
            // per-locus accumulators: reads, plus, duplexes, dreads, nlisted, cmax, cmaj, H[K]; then the two counters
            const size_t nacc = (size_t)nl * (7 + (size_t)K) + 2;
            // one device allocation for the tables and the per-locus state, carved at 256-byte boundaries; the list gets its own once it is counted
            size_t need = 0;
            auto room = [&](size_t bytes) {
                const size_t at = need;
                need += (bytes + 255) & ~(size_t)255;
                return at;
            };
            const size_t a_clen = room(8 * (size_t)o->n_contigs), a_loci = room(sizeof(MirpLocusSpan) * (size_t)nl), a_acc = room(8 * nacc),
                         a_fringe = room(8), a_ufirst = room(8 * (size_t)nl), a_ulast = room(8 * (size_t)nl), a_pfirst = room(8 * (size_t)nl),
                         a_plast = room(8 * (size_t)nl), a_njob = room(4 * (size_t)nl), a_ujoff = room(8 * (size_t)(nl + 1)),
                         a_pjoff = room(8 * (size_t)(nl + 1)), a_sbase = room(8 * (size_t)(nl + 1)), a_out = room(sizeof(MirpSignatureRow) * (size_t)nl),
                         a_ends = room(16 * (size_t)n), a_places = room(16 * (size_t)n), a_tmp = room(16 * (size_t)n), a_lo = room(4 * (size_t)n),
                         a_hi = room(4 * (size_t)n), a_head = room(4 * (size_t)n), a_slo = room(8 * (size_t)(n + 1)), a_shi = room(8 * (size_t)(n + 1)),
                         a_hs = room(8 * (size_t)(n + 1)), a_ekey = room(8 * (size_t)n), a_esum = room(8 * (size_t)n);
            TmpDevice T;
            char* base = (char*)T.get(need);
            if (!base) return fail(c, -6, "device allocation failed (signature scan)");
            long long* d_clen = (long long*)(base + a_clen);
            MirpLocusSpan* d_loci = (MirpLocusSpan*)(base + a_loci);
            unsigned long long* acc = (unsigned long long*)(base + a_acc);
            unsigned* d_fringe = (unsigned*)(base + a_fringe);
            long long* ufirst = (long long*)(base + a_ufirst);
            long long* ulast = (long long*)(base + a_ulast);
            long long* pfirst = (long long*)(base + a_pfirst);
            long long* plast = (long long*)(base + a_plast);
            int* njob = (int*)(base + a_njob);
            long long* ujoff = (long long*)(base + a_ujoff);
            long long* pjoff = (long long*)(base + a_pjoff);
            long long* sbase = (long long*)(base + a_sbase);
            MirpSignatureRow* d_out = (MirpSignatureRow*)(base + a_out);
            MirpHashRec* ends = (MirpHashRec*)(base + a_ends);
            MirpHashRec* places = (MirpHashRec*)(base + a_places);
            MirpHashRec* tmp = (MirpHashRec*)(base + a_tmp);
            int* lo = (int*)(base + a_lo);
            int* hi = (int*)(base + a_hi);
            int* head = (int*)(base + a_head);
            long long* slo = (long long*)(base + a_slo);
            long long* shi = (long long*)(base + a_shi);
            long long* hs = (long long*)(base + a_hs);
            long long* ekey = (long long*)(base + a_ekey);
            unsigned long long* esum = (unsigned long long*)(base + a_esum);
            const unsigned h_fringe[2] = {1u, (unsigned)o->max_len};          // lc_range_kernel's M: none for the 5' ends, max_len for the placements
            HIPCHK(c, hipMemcpyAsync(d_clen, o->contig_len, 8 * (size_t)o->n_contigs, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_loci, loci, sizeof(MirpLocusSpan) * (size_t)nl, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_fringe, h_fringe, 8, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemsetAsync(acc, 0, 8 * nacc, st));
            SgSums Su;
            Su.reads = acc;
            Su.plus = acc + (size_t)nl;
            Su.duplexes = acc + 2 * (size_t)nl;
            Su.dreads = acc + 3 * (size_t)nl;
            Su.nlisted = acc + 4 * (size_t)nl;
            Su.cmax = acc + 5 * (size_t)nl;
            Su.cmaj = acc + 6 * (size_t)nl;
            Su.H = acc + 7 * (size_t)nl;
            unsigned long long* d_cnt = Su.H + (size_t)nl * K;
            HIPCHK(c, hipMemsetAsync(Su.cmaj, 0xff, 8 * (size_t)nl, st));
            // both key lists, then U and V
            hipLaunchKernelGGL(sg_key_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, n, d_clen, O, ends, places, d_cnt);
            HIPCHK(c, hipGetLastError());
            if (int rc = mirp_device_sort_hashes(c, ends, tmp, n, 33 + O.tid_bits)) return rc;
            hipLaunchKernelGGL(sg_run_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, ends, n, 2ull << (31 + O.tid_bits), lo, hi, head);
            launch_excl_scan(st, lo, slo, n);
            launch_excl_scan(st, hi, shi, n);
            launch_excl_scan(st, head, hs, n);
            hipLaunchKernelGGL(sg_ends_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, ends, n, head, hs, slo, shi, O.tid_bits, ekey, esum, d_cnt);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&nuv, hs + n, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, st));
            // the placement table; it takes the sort's second buffer and the list of the 5' ends, which are read for the last time above
            if (int rc = mirp_device_sort_hashes(c, places, tmp, n, 17 + lc_bits(n))) return rc;
            hipLaunchKernelGGL(sg_run_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, places, n, (unsigned long long)n << 17, lo, hi, head);
            launch_excl_scan(st, lo, slo, n);
            launch_excl_scan(st, hi, shi, n);
            launch_excl_scan(st, head, hs, n);
            long long* pkey = (long long*)tmp;
            unsigned long long* psum = (unsigned long long*)tmp + (size_t)n;
            unsigned* pmeta = (unsigned*)ends;
            int* partner = (int*)ends + (size_t)n;
            int* listed = (int*)ends + 2 * (size_t)n;
            hipLaunchKernelGGL(sg_place_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, places, n, head, hs, slo, shi, pkey, pmeta, psum);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&np, hs + n, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            const long long nu = (long long)h_cnt[1], nv = nuv - nu;
            // partners, the listed rows before every row (the scan takes slo, which the table no longer needs), and the ranges of both tables
            long long* lscan = slo;
            if (np > 0) {
                hipLaunchKernelGGL(sg_pair_kernel, dim3(cl_grid(np)), dim3(CL_NT), 0, st, pkey, pmeta, psum, np, O.overhang, O.min_reads, partner, listed);
                launch_excl_scan(st, listed, lscan, np);
            }
            hipLaunchKernelGGL(lc_range_kernel<const long long*>, dim3(cl_grid(nl)), dim3(CL_NT), 0, st, (const long long*)ekey, nu, d_loci, nl, d_fringe,
                               ufirst, ulast, njob);
            launch_excl_scan(st, njob, ujoff, nl);
            hipLaunchKernelGGL(lc_range_kernel<const long long*>, dim3(cl_grid(nl)), dim3(CL_NT), 0, st, (const long long*)pkey, np, d_loci, nl, d_fringe + 1,
                               pfirst, plast, njob);
            launch_excl_scan(st, njob, pjoff, nl);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&ujobs, ujoff + nl, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(&pjobs, pjoff + nl, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (ujobs > 0) {
                const unsigned grid = lc_job_grid(c, ujobs);
                hipLaunchKernelGGL(sg_overlap_kernel, dim3(grid), dim3(CL_NT), 0, st, ekey, esum, ekey + nu, esum + nu, nv, d_loci, nl, ufirst, ulast, ujoff,
                                   ujobs, K, Su.H);
                HIPCHK(c, hipGetLastError());
                c->note_jobs_per_slot(7, ujobs, (long long)grid * LC_WAVES);
            }
            const unsigned pgrid = lc_job_grid(c, pjobs);
            if (pjobs > 0) {
                hipLaunchKernelGGL(sg_duplex_kernel<0>, dim3(pgrid), dim3(CL_NT), 0, st, pkey, pmeta, psum, partner, listed, d_loci, nl, pfirst, plast, pjoff,
                                   pjobs, O.overhang, Su);
                hipLaunchKernelGGL(sg_duplex_kernel<1>, dim3(pgrid), dim3(CL_NT), 0, st, pkey, pmeta, psum, partner, listed, d_loci, nl, pfirst, plast, pjoff,
                                   pjobs, O.overhang, Su);
            }
            hipLaunchKernelGGL(sg_out_kernel, dim3(cl_grid(nl)), dim3(CL_NT), 0, st, nl, Su, pkey, pmeta, psum, partner, d_out, njob);
            launch_excl_scan(st, njob, sbase, nl);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&ns, sbase + nl, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_rows, d_out, sizeof(MirpSignatureRow) * (size_t)nl, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_H, Su.H, 8 * (size_t)nl * K, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (ns > 0) {
                h_sites = (MirpDuplexSite*)std::malloc(sizeof(MirpDuplexSite) * (size_t)ns);
                if (!h_sites) return fail(c, -6, "host allocation failed (signature scan)");
                MirpDuplexSite* d_sites = (MirpDuplexSite*)T.get(sizeof(MirpDuplexSite) * (size_t)ns);
                if (!d_sites) return fail(c, -6, "device allocation failed (signature scan)");
                hipLaunchKernelGGL(sg_emit_kernel, dim3(pgrid), dim3(CL_NT), 0, st, pkey, pmeta, psum, partner, listed, lscan, d_loci, nl, pfirst, plast,
                                   pjoff, pjobs, O.overhang, O.max_len, sbase, d_sites);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipMemcpyAsync(h_sites, d_sites, sizeof(MirpDuplexSite) * (size_t)ns, hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
            }
            return 0;
        };
        if (int rc = run()) return give_up(rc);
    }
    *rows = h_rows;
    *overlaps = h_H;
    *sites = h_sites;
    *n_sites = ns;
    if (stats) {
        stats[0] = n;
        stats[1] = (long long)h_cnt[0];
        stats[2] = (long long)h_cnt[1];
        stats[3] = nuv - (long long)h_cnt[1];
        stats[4] = ujobs;
        stats[5] = ns;
    }
    return 0;
}
