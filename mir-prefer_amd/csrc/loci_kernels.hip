// Reads on given loci per sample on the context's resident alignments (mirp_locus_scan).  The host (loci.py) reads the interval
// file, makes the strand and Dicer calls and writes the files; everything per record, per locus and per placement runs here.
//
// The loci may overlap, nest and repeat, so a record counts in every locus of its contig that its clipped span (cl_span) touches: an interval
// join, not the monotone one-to-one assignment of cl_assign_kernel.  Records and placements are sorted by (tid, pos), so the partners of a
// locus [start, end] lie in one range of either table: pos in [start - M + 1, end], M = the longest resident record.
//   longest  lc_maxlen_kernel: M, a wave-reduced atomicMax.
//   ranges   lc_range_kernel, one lane per locus: two binary searches over the keys tid << 32 | pos give the range, ceil(range / C) its jobs
//            (C = MIRP_LOCI_CHUNK table rows); one scan numbers the jobs of all loci.  Run once over the records and once over the placements.
//   count    lc_count_kernel, one wave per (locus, chunk of C records) on a capped resident grid, wave w serving jobs w, w + waves, ...: no job
//            table, a job finds its locus by one binary search over the scanned offsets (64-bit job index).  Lanes load the 16-byte records
//            coalesced and apply the overlap and strand predicate; reads, plus reads and the size classes are kept per lane and leave with
//            one cl_wave_atomic each per job, the sample counts with one per distinct sample of every 64 records.
//   placements  built once per call: lc_key_kernel keys every record (first record of its (tid, pos) run) << 17 | strand << 16 | len, as
//            cl_place_kernel does; mirp_device_sort_hashes groups them; run heads + two split-at-bit-30 scans give exact run sums;
//            lc_table_kernel compacts the runs into the placement table, which is in (tid, pos, strand, len) order.  A record with an empty
//            span is keyed too: its placement overlaps no locus (a locus lies inside its contig), so it is never counted.
//   major    lc_major_kernel, one wave per (locus, chunk of C placements), two passes: <0> counts the passing placements and takes the
//            atomicMax of their sums, <1> the atomicMin of the index among those that reach the maximum = the tie rule of §16.
//   out      lc_out_kernel writes one MirpCluster per locus.
// Every sum, maximum and minimum is an integer atomic, so no result depends on scheduling; no lane loops over a locus's records alone.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "mirp_ctx.h"
#include "loci_device.h"
#include "wave_atomic.h"

namespace mirp {

// does the span [s, e] (keys; s, e inside the contig) on `strand` count in the locus?
__device__ __forceinline__ bool lc_counts(const LcLocus& L, long long s, long long e, int strand, int stranded) {
    return s <= L.hi && e >= L.lo && (!stranded || L.strand == 2 || L.strand == strand);
}

__global__ void __launch_bounds__(CL_NT) lc_maxlen_kernel(const MirpAln* __restrict__ a, long long n, unsigned* __restrict__ maxlen) {
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < n; i += (long long)gridDim.x * CL_NT) m = max(m, (unsigned)a[i].len);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(maxlen, m);
}

struct LcSums {
    unsigned long long *reads, *plus, *sizes, *samples;   // [nl], [nl], [nl * 7], [nl * n_samples]
    unsigned long long *placements, *cmax, *cmaj;         // [nl] each
    unsigned long long* pairs;
    int* bad_sample;
};

__global__ void __launch_bounds__(CL_NT) lc_count_kernel(const MirpAln* __restrict__ a, const long long* __restrict__ clen, int n_contigs,
                                                         const MirpLocusSpan* __restrict__ loci, long long nl, const long long* __restrict__ first,
                                                         const long long* __restrict__ last, const long long* __restrict__ joff, long long n_jobs,
                                                         int n_samples, int stranded, LcSums S) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * LC_WAVES;
    for (long long j = (long long)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); j < n_jobs; j += waves) {
        const long long q = lc_job_locus(joff, nl, j);
        const LcLocus L = lc_locus(loci[q]);
        const long long b = first[q] + (j - joff[q]) * LC_C;
        const long long e = std::min(b + LC_C, last[q]);
        unsigned long long reads = 0, plus = 0, pairs = 0, sz[CL_NCLS] = {0, 0, 0, 0, 0, 0, 0};
        for (long long base = b; base < e; base += 64) {             // the same trip count in every lane
            const long long i = base + lane;
            long long slot = -1;
            unsigned long long d = 0;
            if (i < e) {
                const MirpAln r = a[i];
                const ClSpan sp = cl_span(r, clen, n_contigs);
                if (sp.ok && lc_counts(L, (long long)sp.s, (long long)sp.e - 1, r.strand, stranded)) {
                    if (r.sample >= n_samples) atomicOr(S.bad_sample, 1);
                    else {
                        d = r.depth;
                        slot = q * n_samples + r.sample;
                        const int cls = r.len < 20 ? 0 : r.len > 24 ? 6 : r.len - 19;
                        reads += d;
                        plus += r.strand ? 0ull : d;
                        pairs++;
#pragma unroll
                        for (int k = 0; k < CL_NCLS; k++) sz[k] += cls == k ? d : 0ull;
                    }
                }
            }
            cl_wave_atomic<0>(S.samples, slot, d);
        }
        cl_wave_atomic<0>(S.reads, reads ? q : -1, reads);
        cl_wave_atomic<0>(S.plus, plus ? q : -1, plus);
        cl_wave_atomic<0>(S.pairs, pairs ? 0 : -1, pairs);
#pragma unroll
        for (int k = 0; k < CL_NCLS; k++) cl_wave_atomic<0>(S.sizes, sz[k] ? q * CL_NCLS + k : -1, sz[k]);
    }
}

__global__ void __launch_bounds__(CL_NT) lc_key_kernel(const MirpAln* __restrict__ a, long long n, MirpHashRec* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < n; i += (long long)gridDim.x * CL_NT) {
        const long long k = lc_key(a, i);
        long long lo = 0, hi = i;                      // first record of this (tid, pos)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (lc_key(a, mid) < k) lo = mid + 1;
            else hi = mid;
        }
        const MirpAln r = a[i];
        MirpHashRec p;
        p.hash = ((unsigned long long)lo << 17) | ((unsigned long long)r.strand << 16) | (unsigned long long)r.len;
        p.idx = r.depth;
        p.pad = 0;
        out[i] = p;
    }
}

// depth of every sorted key split at bit 30 (for the two exact scans) and the run heads
__global__ void __launch_bounds__(CL_NT) lc_run_kernel(const MirpHashRec* __restrict__ p, long long n, int* __restrict__ lo, int* __restrict__ hi,
                                                       int* __restrict__ head) {
    for (long long j = (long long)blockIdx.x * CL_NT + threadIdx.x; j < n; j += (long long)gridDim.x * CL_NT) {
        const unsigned d = p[j].idx;
        lo[j] = (int)(d & 0x3fffffffu);
        hi[j] = (int)(d >> 30);
        head[j] = j == 0 || p[j - 1].hash != p[j].hash;
    }
}

// placement table: row hs[j] of every run head j = {tid << 32 | pos, strand << 16 | len, the run's depth sum}
__global__ void __launch_bounds__(CL_NT) lc_table_kernel(const MirpAln* __restrict__ a, const MirpHashRec* __restrict__ p, long long n,
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

template <int PASS>
__global__ void __launch_bounds__(CL_NT) lc_major_kernel(const long long* __restrict__ pkey, const unsigned* __restrict__ pmeta,
                                                         const unsigned long long* __restrict__ psum, const long long* __restrict__ clen,
                                                         const MirpLocusSpan* __restrict__ loci, long long nl, const long long* __restrict__ first,
                                                         const long long* __restrict__ last, const long long* __restrict__ joff, long long n_jobs,
                                                         int stranded, LcSums S) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * LC_WAVES;
    for (long long j = (long long)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); j < n_jobs; j += waves) {
        const long long q = lc_job_locus(joff, nl, j);
        const MirpLocusSpan lq = loci[q];
        const LcLocus L = lc_locus(lq);
        const long long t0 = (long long)lq.tid << 32, top = t0 + clen[lq.tid];   // the contig's position 0 and last base as keys
        const long long b = first[q] + (j - joff[q]) * LC_C;
        const long long e = std::min(b + LC_C, last[q]);
        unsigned long long cnt = 0, best = 0, at = ~0ull;
        const unsigned long long cmax = PASS ? S.cmax[q] : 0;
        for (long long i = b + lane; i < e; i += 64) {
            const long long k = pkey[i];
            const unsigned m = pmeta[i];
            const long long s = std::max(k, t0 + 1);                            // cl_span's clipping
            const long long t = std::min(k + (long long)(m & 0xffffu) - 1, top);
            if (s > t || !lc_counts(L, s, t, (int)(m >> 16), stranded)) continue;
            if (PASS == 0) {
                cnt++;
                best = std::max(best, psum[i]);
            } else if (psum[i] == cmax) {
                at = std::min(at, (unsigned long long)i);
            }
        }
        if (PASS == 0) {
            cl_wave_atomic<0>(S.placements, cnt ? q : -1, cnt);
            cl_wave_atomic<1>(S.cmax, cnt ? q : -1, best);
        } else {
            cl_wave_atomic<2>(S.cmaj, at != ~0ull ? q : -1, at);
        }
    }
}

__global__ void __launch_bounds__(CL_NT) lc_out_kernel(const MirpLocusSpan* __restrict__ loci, long long nl, LcSums S, const long long* __restrict__ pkey,
                                                       const unsigned* __restrict__ pmeta, MirpCluster* __restrict__ out) {
    for (long long q = (long long)blockIdx.x * CL_NT + threadIdx.x; q < nl; q += (long long)gridDim.x * CL_NT) {
        MirpCluster o;
        o.tid = loci[q].tid;
        o.start = loci[q].start;
        o.end = loci[q].end;
        o.reads = (long long)S.reads[q];
        o.plus_reads = (long long)S.plus[q];
        o.placements = (long long)S.placements[q];
        o.major_reads = (long long)S.cmax[q];
        o.reserved = 0;
        if (S.placements[q]) {
            const unsigned long long m = S.cmaj[q];
            o.major_pos = (long long)(int)(pkey[m] & 0xffffffffll);
            o.major_strand = (int)(pmeta[m] >> 16);
            o.major_len = (int)(pmeta[m] & 0xffffu);
        } else {
            o.major_pos = 0;
            o.major_strand = 0;
            o.major_len = 0;
        }
#pragma unroll
        for (int k = 0; k < CL_NCLS; k++) o.sizes[k] = (long long)S.sizes[q * CL_NCLS + k];
        out[q] = o;
    }
}

}  // namespace mirp

extern "C" int mirp_locus_scan(mirp_ctx* c, const MirpLocusSpan* loci, int64_t n_loci, const MirpLocusOpts* o, MirpCluster** out, int64_t** sample_counts,
                               int64_t stats[5]) {
    using namespace mirp;
    if (!c) return -1;
    if (!o || !out || !sample_counts || (n_loci > 0 && !loci) || (o->n_contigs > 0 && !o->contig_len)) return fail(c, -1, "mirp_locus_scan: bad argument");
    if (n_loci < 0 || n_loci > MIRP_LOCI_MAX || o->n_contigs < 0 || o->n_samples < 1 || o->n_samples > MIRP_MAX_SAMPLES)
        return fail(c, -1, "mirp_locus_scan: bad options");
    for (int t = 0; t < o->n_contigs; t++)
        if (o->contig_len[t] < 0 || o->contig_len[t] > 0x7fffffffll) return fail(c, -1, "mirp_locus_scan: a contig length outside 0..2^31 - 1");
    for (long long q = 0; q < n_loci; q++) {
        const MirpLocusSpan& l = loci[q];
        if (l.tid < 0 || l.tid >= o->n_contigs || l.strand < 0 || l.strand > 2 || l.start < 1 || l.start > l.end || l.end > o->contig_len[l.tid])
            return fail(c, -1, "mirp_locus_scan: locus " + std::to_string(q + 1) + " is not an interval of a contig with strand 0..2");
    }
    *out = nullptr;
    *sample_counts = nullptr;
    c->reset_jobs_per_slot(5);
    const long long n = c->n_alns, nl = n_loci;
    const int S = o->n_samples;
    if (n > (1ll << 31) - 2) return fail(c, -5, "mirp_locus_scan: more than 2^31 records");
    MirpCluster* h_out = (MirpCluster*)std::calloc((size_t)std::max(nl, 1ll), sizeof(MirpCluster));
    int64_t* h_samples = (int64_t*)std::calloc((size_t)std::max(nl * S, 1ll), 8);
    auto give_up = [&](int rc) {
        std::free(h_out);
        std::free(h_samples);
        return rc;
    };
    if (!h_out || !h_samples) return give_up(fail(c, -6, "host allocation failed (locus scan)"));
    for (long long q = 0; q < nl; q++) {                     // what a locus without reads keeps
        h_out[q].tid = loci[q].tid;
        h_out[q].start = loci[q].start;
        h_out[q].end = loci[q].end;
    }
    long long jobs = 0, pjobs = 0, np = 0;
    unsigned long long h_pairs = 0;
    unsigned h_maxlen = 0;
    if (n > 0 && nl > 0) {
        // the device work in a function of its own, so that HIPCHK's early returns free the host results
        auto run = [&]() -> int {
            HIPCHK(c, hipSetDevice(c->device));
            const hipStream_t st = c->stream;
            const MirpAln* alns = (const MirpAln*)c->alns.p;
            // per-locus accumulators: reads, plus, placements, cmax, cmaj, sizes[7], samples[S], then pairs, the bad flag, M
            const size_t nacc = (size_t)nl * (12 + (size_t)S) + 3;
            // one device allocation for the call, carved at 256-byte boundaries
            size_t need = 0;
            auto room = [&](size_t bytes) {
                const size_t at = need;
                need += (bytes + 255) & ~(size_t)255;
                return at;
            };
            const size_t a_clen = room(8 * (size_t)o->n_contigs), a_loci = room(sizeof(MirpLocusSpan) * (size_t)nl), a_acc = room(8 * nacc),
                         a_first = room(8 * (size_t)nl), a_last = room(8 * (size_t)nl), a_njob = room(4 * (size_t)nl), a_joff = room(8 * (size_t)(nl + 1)),
                         a_out = room(sizeof(MirpCluster) * (size_t)nl), a_pl = room(16 * (size_t)n), a_tmp = room(16 * (size_t)n),
                         a_lo = room(4 * (size_t)n), a_hi = room(4 * (size_t)n), a_head = room(4 * (size_t)n), a_slo = room(8 * (size_t)(n + 1)),
                         a_shi = room(8 * (size_t)(n + 1)), a_hs = room(8 * (size_t)(n + 1));
            TmpDevice T;
            char* base = (char*)T.get(need);
            if (!base) return fail(c, -6, "device allocation failed (locus scan)");
            long long* d_clen = (long long*)(base + a_clen);
            MirpLocusSpan* d_loci = (MirpLocusSpan*)(base + a_loci);
            unsigned long long* acc = (unsigned long long*)(base + a_acc);
            long long* first = (long long*)(base + a_first);
            long long* last = (long long*)(base + a_last);
            int* njob = (int*)(base + a_njob);
            long long* joff = (long long*)(base + a_joff);
            MirpCluster* d_out = (MirpCluster*)(base + a_out);
            MirpHashRec* pl = (MirpHashRec*)(base + a_pl);
            MirpHashRec* tmp = (MirpHashRec*)(base + a_tmp);
            int* lo = (int*)(base + a_lo);
            int* hi = (int*)(base + a_hi);
            int* head = (int*)(base + a_head);
            long long* slo = (long long*)(base + a_slo);
            long long* shi = (long long*)(base + a_shi);
            long long* hs = (long long*)(base + a_hs);
            HIPCHK(c, hipMemcpyAsync(d_clen, o->contig_len, 8 * (size_t)o->n_contigs, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_loci, loci, sizeof(MirpLocusSpan) * (size_t)nl, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemsetAsync(acc, 0, 8 * nacc, st));
            LcSums Su;
            Su.reads = acc;
            Su.plus = acc + (size_t)nl;
            Su.placements = acc + 2 * (size_t)nl;
            Su.cmax = acc + 3 * (size_t)nl;
            Su.cmaj = acc + 4 * (size_t)nl;
            Su.sizes = acc + 5 * (size_t)nl;
            Su.samples = acc + 12 * (size_t)nl;
            Su.pairs = acc + (12 + (size_t)S) * (size_t)nl;
            Su.bad_sample = (int*)(Su.pairs + 1);
            unsigned* d_maxlen = (unsigned*)(Su.pairs + 2);
            HIPCHK(c, hipMemsetAsync(Su.cmaj, 0xff, 8 * (size_t)nl, st));
            // the longest record, the record range and the jobs of every locus
            hipLaunchKernelGGL(lc_maxlen_kernel, dim3(std::min(cl_grid(n), 4096u)), dim3(CL_NT), 0, st, alns, n, d_maxlen);
            hipLaunchKernelGGL(lc_range_kernel<const MirpAln*>, dim3(cl_grid(nl)), dim3(CL_NT), 0, st, alns, n, d_loci, nl, d_maxlen, first, last, njob);
            launch_excl_scan(st, njob, joff, nl);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&jobs, joff + nl, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(&h_maxlen, d_maxlen, 4, hipMemcpyDeviceToHost, st));
            // the placement table (independent of the loci): keys, sort, run sums, compaction
            hipLaunchKernelGGL(lc_key_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, n, pl);
            HIPCHK(c, hipGetLastError());
            if (int rc = mirp_device_sort_hashes(c, pl, tmp, n, 17 + lc_bits(n - 1))) return rc;
            hipLaunchKernelGGL(lc_run_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, pl, n, lo, hi, head);
            launch_excl_scan(st, lo, slo, n);
            launch_excl_scan(st, hi, shi, n);
            launch_excl_scan(st, head, hs, n);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&np, hs + n, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (jobs > 0) {
                const unsigned grid = lc_job_grid(c, jobs);
                hipLaunchKernelGGL(lc_count_kernel, dim3(grid), dim3(CL_NT), 0, st, alns, d_clen, o->n_contigs, d_loci, nl, first, last, joff, jobs, S,
                                   o->stranded ? 1 : 0, Su);
                HIPCHK(c, hipGetLastError());
                c->note_jobs_per_slot(5, jobs, (long long)grid * LC_WAVES);
            }
            // the sorted keys are read for the last time by lc_table_kernel: the table takes the sort's second buffer
            long long* pkey = (long long*)tmp;
            unsigned long long* psum = (unsigned long long*)tmp + (size_t)n;
            unsigned* pmeta = (unsigned*)lo;                  // np <= n entries; lo is free once its scan is done
            hipLaunchKernelGGL(lc_table_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, pl, n, head, hs, slo, shi, pkey, pmeta, psum);
            hipLaunchKernelGGL(lc_range_kernel<const long long*>, dim3(cl_grid(nl)), dim3(CL_NT), 0, st, (const long long*)pkey, np, d_loci, nl, d_maxlen,
                               first, last, njob);
            launch_excl_scan(st, njob, joff, nl);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&pjobs, joff + nl, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (pjobs > 0) {
                const unsigned grid = lc_job_grid(c, pjobs);
                hipLaunchKernelGGL(lc_major_kernel<0>, dim3(grid), dim3(CL_NT), 0, st, pkey, pmeta, psum, d_clen, d_loci, nl, first, last, joff, pjobs,
                                   o->stranded ? 1 : 0, Su);
                hipLaunchKernelGGL(lc_major_kernel<1>, dim3(grid), dim3(CL_NT), 0, st, pkey, pmeta, psum, d_clen, d_loci, nl, first, last, joff, pjobs,
                                   o->stranded ? 1 : 0, Su);
            }
            hipLaunchKernelGGL(lc_out_kernel, dim3(cl_grid(nl)), dim3(CL_NT), 0, st, d_loci, nl, Su, pkey, pmeta, d_out);
            HIPCHK(c, hipGetLastError());
            unsigned long long h_tail[2];
            HIPCHK(c, hipMemcpyAsync(h_tail, Su.pairs, 16, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_out, d_out, sizeof(MirpCluster) * (size_t)nl, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemcpyAsync(h_samples, Su.samples, 8 * (size_t)nl * S, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            h_pairs = h_tail[0];
            if ((int)(h_tail[1] & 0xffffffffu)) return fail(c, -1, "mirp_locus_scan: a record's sample index is not below n_samples");
            return 0;
        };
        if (int rc = run()) return give_up(rc);
    } else if (n > 0) {                                      // no locus: only the longest record is left to find
        const MirpAln* alns = (const MirpAln*)c->alns.p;
        auto run = [&]() -> int {
            HIPCHK(c, hipSetDevice(c->device));
            TmpDevice T;
            unsigned* d_maxlen = (unsigned*)T.get(4);
            if (!d_maxlen) return fail(c, -6, "device allocation failed (locus scan)");
            HIPCHK(c, hipMemsetAsync(d_maxlen, 0, 4, c->stream));
            hipLaunchKernelGGL(lc_maxlen_kernel, dim3(std::min(cl_grid(n), 4096u)), dim3(CL_NT), 0, c->stream, alns, n, d_maxlen);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&h_maxlen, d_maxlen, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return 0;
        };
        if (int rc = run()) return give_up(rc);
    }
    *out = h_out;
    *sample_counts = h_samples;
    if (stats) {
        stats[0] = n;
        stats[1] = nl;
        stats[2] = jobs;
        stats[3] = (long long)h_pairs;
        stats[4] = (long long)h_maxlen;
    }
    return 0;
}
