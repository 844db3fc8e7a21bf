// Small-RNA clusters and their per-sample counts on the context's resident alignments (mirp_cluster_scan).  The host
// (clusters.py) turns -m into the integer threshold T, makes the strand and Dicer calls and writes the files; everything per record, per event,
// per island and per placement runs here.
//
// Positions are 64-bit keys tid << 32 | p (p < 2^32: pos < 2^31 and len < 2^16).  A record's span is clipped to the contig, [max(pos, 1),
// min(pos + len, LN + 1)); a record whose clipped span is empty adds no coverage and counts nowhere.
//   events   cl_event_kernel: the start keys are already sorted (the records are sorted by (tid, pos)); the end keys with their depths are
//            sorted by mirp_device_sort_hashes (the 16-byte (u64 key, u32, u32) records of the read collapse).  cl_merge_kernel merges the two
//            streams by merge path (starts before ends on equal keys) into signed deltas, split into their low 30 bits and the rest, so that two
//            int32 scans (launch_excl_scan) give the exact 64-bit coverage prefix P.
//   islands  cl_island_kernel: the last event of each key k has the coverage on [k, next key) = P(after it) and the coverage before k = P(the
//            first event of k), found by a binary search; c >= T starting or ending there flags an island boundary.  Boundaries alternate
//            start / end, so one scan numbers both (cl_island_write_kernel).
//   clusters cl_cluster_head_kernel: an island starts a cluster unless it follows one of the same contig with a gap <= pad; a scan numbers them
//            (cl_cluster_write_kernel).
//   assign   cl_assign_kernel: one binary search per record finds the first cluster whose end is >= the record's start; the record counts there
//            if that cluster starts before the record ends.  Its depth goes to the cluster's reads, plus reads, size class and sample count.
//   placements cl_place_kernel keys the assigned records (first record of their (tid, pos) run) << 17 | strand << 16 | len, a placement of one
//            cluster each; mirp_device_sort_hashes groups them.  cl_run_kernel + two scans give exact depth prefixes, cl_run_sum_kernel sums
//            each run with one binary search for its end, counts it and takes the cluster maximum; cl_major_kernel takes the smallest run of
//            the maximum (= smallest pos, then + before -, then the shorter len); cl_out_kernel writes the clusters.
// Sums, maxima and minima per cluster are integer atomics, one per distinct address of a wave (cl_wave_atomic): a hotspot cluster costs one
// atomic per wave, no lane loops over its records, and the results do not depend on scheduling.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "mirp_ctx.h"
#include "clusters_device.h"
#include "wave_atomic.h"

namespace mirp {

__global__ void __launch_bounds__(CL_NT) cl_event_kernel(const MirpAln* __restrict__ a, long long n, const long long* __restrict__ clen, int n_contigs,
                                                         unsigned long long* __restrict__ skey, unsigned* __restrict__ sdep,
                                                         MirpHashRec* __restrict__ ends) {
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < n; i += (long long)gridDim.x * CL_NT) {
        const MirpAln r = a[i];
        const ClSpan sp = cl_span(r, clen, n_contigs);
        const unsigned d = sp.ok ? r.depth : 0u;
        skey[i] = sp.s;
        sdep[i] = d;
        MirpHashRec e;
        e.hash = sp.e;
        e.idx = d;
        e.pad = 0;
        ends[i] = e;
    }
}

__global__ void __launch_bounds__(CL_NT) cl_merge_kernel(const unsigned long long* __restrict__ skey, const unsigned* __restrict__ sdep,
                                                         const MirpHashRec* __restrict__ ends, long long n, unsigned long long* __restrict__ mkey,
                                                         int* __restrict__ lo, int* __restrict__ hi) {
    for (long long v = (long long)blockIdx.x * CL_NT + threadIdx.x; v < 2 * n; v += (long long)gridDim.x * CL_NT) {
        unsigned long long k;
        unsigned d;
        long long r;
        int sign;
        if (v < n) {
            k = skey[v];
            d = sdep[v];
            r = v + cl_lower_rec(ends, 0, n, k);
            sign = 1;
        } else {
            const MirpHashRec e = ends[v - n];
            k = e.hash;
            d = e.idx;
            r = (v - n) + cl_upper(skey, 0, n, k);
            sign = -1;
        }
        mkey[r] = k;
        lo[r] = sign * (int)(d & 0x3fffffffu);
        hi[r] = sign * (int)(d >> 30);
    }
}

__global__ void __launch_bounds__(CL_NT) cl_island_kernel(const unsigned long long* __restrict__ mkey, const long long* __restrict__ slo,
                                                          const long long* __restrict__ shi, long long m, unsigned long long T, int* __restrict__ flag) {
    for (long long r = (long long)blockIdx.x * CL_NT + threadIdx.x; r < m; r += (long long)gridDim.x * CL_NT) {
        const unsigned long long k = mkey[r];
        int f = 0;
        if (r + 1 == m || mkey[r + 1] != k) {
            const unsigned long long cur = (unsigned long long)cl_prefix(slo, shi, r + 1);
            const unsigned long long prev = (unsigned long long)cl_prefix(slo, shi, cl_lower(mkey, 0, r, k));
            f = (cur >= T) != (prev >= T);
        }
        flag[r] = f;
    }
}

__global__ void __launch_bounds__(CL_NT) cl_island_write_kernel(const unsigned long long* __restrict__ mkey, const int* __restrict__ flag,
                                                                const long long* __restrict__ bs, long long m, long long ni,
                                                                unsigned long long* __restrict__ istart, unsigned long long* __restrict__ iend) {
    for (long long r = (long long)blockIdx.x * CL_NT + threadIdx.x; r < m; r += (long long)gridDim.x * CL_NT) {
        if (!flag[r]) continue;
        const long long b = bs[r];
        if ((b >> 1) >= ni) continue;                 // (the boundaries pair up: every contig ends at coverage 0)
        if (b & 1) iend[b >> 1] = mkey[r] - 1;        // the coverage drops below T at this key: the island ended one position before
        else istart[b >> 1] = mkey[r];
    }
}

__global__ void __launch_bounds__(CL_NT) cl_cluster_head_kernel(const unsigned long long* __restrict__ istart, const unsigned long long* __restrict__ iend,
                                                                long long ni, long long pad, int* __restrict__ head) {
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < ni; i += (long long)gridDim.x * CL_NT) {
        int h = 1;
        if (i > 0) {
            const unsigned long long a = istart[i], b = iend[i - 1];
            h = (a >> 32) != (b >> 32) || (long long)(a - b) - 1 > pad;
        }
        head[i] = h;
    }
}

__global__ void __launch_bounds__(CL_NT) cl_cluster_write_kernel(const unsigned long long* __restrict__ istart, const unsigned long long* __restrict__ iend,
                                                                 const int* __restrict__ head, const long long* __restrict__ cs, long long ni,
                                                                 unsigned long long* __restrict__ cstart, unsigned long long* __restrict__ cend) {
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < ni; i += (long long)gridDim.x * CL_NT) {
        const long long c = cs[i] + head[i] - 1;
        if (head[i]) cstart[c] = istart[i];
        if (i + 1 == ni || head[i + 1]) cend[c] = iend[i];
    }
}

struct ClSums {
    unsigned long long *reads, *plus, *sizes, *samples;   // [nc], [nc], [nc * 7], [nc * n_samples]
    unsigned long long *total, *assigned;
    int* bad_sample;
};

__global__ void __launch_bounds__(CL_NT) cl_assign_kernel(const MirpAln* __restrict__ a, long long n, const long long* __restrict__ clen, int n_contigs,
                                                          const unsigned long long* __restrict__ cstart, const unsigned long long* __restrict__ cend,
                                                          long long nc, int n_samples, ClSums S, int* __restrict__ cid, int* __restrict__ asg) {
    for (long long base = (long long)blockIdx.x * CL_NT; base < n; base += (long long)gridDim.x * CL_NT) {
        const long long i = base + threadIdx.x;
        long long c = -1;
        unsigned long long d = 0;
        MirpAln r = {};
        if (i < n) {
            r = a[i];
            d = r.depth;
            const ClSpan sp = cl_span(r, clen, n_contigs);
            if (sp.ok) {
                const long long k = cl_lower(cend, 0, nc, sp.s);
                if (k < nc && cstart[k] <= sp.e - 1) c = k;
            }
            if (c >= 0 && r.sample >= n_samples) {
                atomicOr(S.bad_sample, 1);
                c = -1;
            }
            cid[i] = (int)c;
            asg[i] = c >= 0;
        }
        cl_wave_atomic<0>(S.total, i < n ? 0 : -1, d);
        const unsigned long long took = __ballot(c >= 0);
        if ((threadIdx.x & 63) == 0 && took) atomicAdd(S.assigned, (unsigned long long)__popcll(took));
        const int cls = r.len < 20 ? 0 : r.len > 24 ? 6 : r.len - 19;
        cl_wave_atomic<0>(S.reads, c, d);
        cl_wave_atomic<0>(S.plus, c >= 0 && !r.strand ? c : -1, d);
        cl_wave_atomic<0>(S.sizes, c >= 0 ? c * CL_NCLS + cls : -1, d);
        cl_wave_atomic<0>(S.samples, c >= 0 ? c * n_samples + r.sample : -1, d);
    }
}

__global__ void __launch_bounds__(CL_NT) cl_place_kernel(const MirpAln* __restrict__ a, long long n, const int* __restrict__ cid,
                                                         const long long* __restrict__ as, MirpHashRec* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * CL_NT + threadIdx.x; i < n; i += (long long)gridDim.x * CL_NT) {
        const int c = cid[i];
        if (c < 0) continue;
        const MirpAln r = a[i];
        long long lo = 0, hi = i;                      // first record of this (tid, pos)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            const MirpAln q = a[mid];
            if (q.tid < r.tid || (q.tid == r.tid && q.pos < r.pos)) lo = mid + 1;
            else hi = mid;
        }
        MirpHashRec p;
        p.hash = ((unsigned long long)lo << 17) | ((unsigned long long)r.strand << 16) | (unsigned long long)r.len;
        p.idx = r.depth;
        p.pad = (unsigned)c;
        out[as[i]] = p;
    }
}

__global__ void __launch_bounds__(CL_NT) cl_run_kernel(const MirpHashRec* __restrict__ p, long long n, int* __restrict__ lo, int* __restrict__ hi) {
    for (long long j = (long long)blockIdx.x * CL_NT + threadIdx.x; j < n; j += (long long)gridDim.x * CL_NT) {
        const unsigned d = p[j].idx;
        lo[j] = (int)(d & 0x3fffffffu);
        hi[j] = (int)(d >> 30);
    }
}

__global__ void __launch_bounds__(CL_NT) cl_run_sum_kernel(const MirpHashRec* __restrict__ p, long long n, const long long* __restrict__ slo,
                                                           const long long* __restrict__ shi, unsigned long long* __restrict__ rsum,
                                                           unsigned long long* __restrict__ placements, unsigned long long* __restrict__ cmax) {
    for (long long base = (long long)blockIdx.x * CL_NT; base < n; base += (long long)gridDim.x * CL_NT) {
        const long long j = base + threadIdx.x;
        long long c = -1;
        unsigned long long s = 0;
        if (j < n) {
            const MirpHashRec q = p[j];
            if (j == 0 || p[j - 1].hash != q.hash) {
                const long long e = cl_upper_rec(p, j + 1, n, q.hash);
                s = (unsigned long long)(cl_prefix(slo, shi, e) - cl_prefix(slo, shi, j));
                c = q.pad;
                rsum[j] = s;
            }
        }
        cl_wave_atomic<0>(placements, c, 1ull);
        cl_wave_atomic<1>(cmax, c, s);
    }
}

__global__ void __launch_bounds__(CL_NT) cl_major_kernel(const MirpHashRec* __restrict__ p, long long n, const unsigned long long* __restrict__ rsum,
                                                         const unsigned long long* __restrict__ cmax, unsigned long long* __restrict__ cmaj) {
    for (long long base = (long long)blockIdx.x * CL_NT; base < n; base += (long long)gridDim.x * CL_NT) {
        const long long j = base + threadIdx.x;
        long long c = -1;
        if (j < n) {
            const MirpHashRec q = p[j];
            if ((j == 0 || p[j - 1].hash != q.hash) && rsum[j] == cmax[q.pad]) c = q.pad;
        }
        cl_wave_atomic<2>(cmaj, c, (unsigned long long)j);
    }
}

__global__ void __launch_bounds__(CL_NT) cl_out_kernel(const MirpAln* __restrict__ a, const unsigned long long* __restrict__ cstart,
                                                       const unsigned long long* __restrict__ cend, long long nc, ClSums S,
                                                       const unsigned long long* __restrict__ placements, const unsigned long long* __restrict__ cmax,
                                                       const unsigned long long* __restrict__ cmaj, const MirpHashRec* __restrict__ p,
                                                       MirpCluster* __restrict__ out) {
    for (long long c = (long long)blockIdx.x * CL_NT + threadIdx.x; c < nc; c += (long long)gridDim.x * CL_NT) {
        MirpCluster o;
        o.tid = (int)(cstart[c] >> 32);
        o.start = (long long)(cstart[c] & 0xffffffffull);
        o.end = (long long)(cend[c] & 0xffffffffull);
        o.reads = (long long)S.reads[c];
        o.plus_reads = (long long)S.plus[c];
        o.placements = (long long)placements[c];
        o.major_reads = (long long)cmax[c];
        o.reserved = 0;
        if (placements[c]) {
            const unsigned long long k = p[cmaj[c]].hash;
            o.major_pos = a[k >> 17].pos;
            o.major_strand = (int)((k >> 16) & 1);
            o.major_len = (int)(k & 0xffff);
        } else {
            o.major_pos = 0;
            o.major_strand = 0;
            o.major_len = 0;
        }
#pragma unroll
        for (int q = 0; q < CL_NCLS; q++) o.sizes[q] = (long long)S.sizes[c * CL_NCLS + q];
        out[c] = o;
    }
}

}  // namespace mirp

namespace {

int cl_count(mirp_ctx* c, const long long* d, long long* h) {
    HIPCHK(c, hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cl_bits(long long v) {      // bits of the largest value v
    int b = 0;
    while (b < 63 && (1ll << b) <= v) b++;
    return b;
}

}  // namespace

extern "C" int mirp_cluster_scan(mirp_ctx* c, const MirpClusterOpts* o, MirpCluster** clusters, int64_t* n_clusters, int64_t** sample_counts,
                                 int64_t stats[5]) {
    using namespace mirp;
    if (!c) return -1;
    if (!o || !clusters || !n_clusters || !sample_counts || (o->n_contigs > 0 && !o->contig_len)) return fail(c, -1, "mirp_cluster_scan: bad argument");
    if (o->threshold < 1 || o->pad < 0 || o->pad > 1000000 || o->n_contigs < 0 || o->n_samples < 1 || o->n_samples > MIRP_MAX_SAMPLES)
        return fail(c, -1, "mirp_cluster_scan: bad options");
    for (int t = 0; t < o->n_contigs; t++)
        if (o->contig_len[t] < 0) return fail(c, -1, "mirp_cluster_scan: negative contig length");
    *clusters = nullptr;
    *n_clusters = 0;
    *sample_counts = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    const long long n = c->n_alns;
    const int S = o->n_samples;
    const MirpAln* alns = (const MirpAln*)c->alns.p;
    long long ni = 0, nc = 0, nA = 0;
    unsigned long long h_sum[2] = {0, 0};        // total depth, assigned records
    TmpDevice T;
    auto grab = [&](size_t bytes) { return T.get(bytes); };
    MirpCluster* d_out = nullptr;
    unsigned long long* d_samples = nullptr;
    if (n > 0) {
        if (n > (1ll << 31) - 2) return fail(c, -5, "mirp_cluster_scan: more than 2^31 records");
        const int nct = std::max(o->n_contigs, 1);
        const int ntid = std::max({nct, c->n_contigs, c->ingest_n_contigs});      // the records' tids are below this
        long long* d_clen = (long long*)grab(8 * (size_t)nct);
        unsigned long long* skey = (unsigned long long*)grab(8 * (size_t)n);
        unsigned* sdep = (unsigned*)grab(4 * (size_t)n);
        MirpHashRec* ends = (MirpHashRec*)grab(16 * (size_t)n);
        MirpHashRec* tmp = (MirpHashRec*)grab(16 * (size_t)n);
        const long long m = 2 * n;
        unsigned long long* mkey = (unsigned long long*)grab(8 * (size_t)m);
        int* lo = (int*)grab(4 * (size_t)m);
        int* hi = (int*)grab(4 * (size_t)m);
        long long* slo = (long long*)grab(8 * (size_t)(m + 1));
        long long* shi = (long long*)grab(8 * (size_t)(m + 1));
        if (!d_clen || !skey || !sdep || !ends || !tmp || !mkey || !lo || !hi || !slo || !shi) return fail(c, -6, "device allocation failed (cluster scan)");
        if (o->n_contigs > 0) HIPCHK(c, hipMemcpyAsync(d_clen, o->contig_len, 8 * (size_t)o->n_contigs, hipMemcpyHostToDevice, st));
        // coverage events, merged; the exact coverage prefix
        hipLaunchKernelGGL(cl_event_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, n, d_clen, o->n_contigs, skey, sdep, ends);
        HIPCHK(c, hipGetLastError());
        if (int rc = mirp_device_sort_hashes(c, ends, tmp, n, 32 + cl_bits(ntid - 1))) return rc;
        hipLaunchKernelGGL(cl_merge_kernel, dim3(cl_grid(m)), dim3(CL_NT), 0, st, skey, sdep, ends, n, mkey, lo, hi);
        launch_excl_scan(st, lo, slo, m);
        launch_excl_scan(st, hi, shi, m);
        // islands, then clusters: the boundary flags go to hi and their scan to slo (both free once the coverage is read)
        int* flag = hi;
        long long* bs = slo;
        hipLaunchKernelGGL(cl_island_kernel, dim3(cl_grid(m)), dim3(CL_NT), 0, st, mkey, slo, shi, m, (unsigned long long)o->threshold, flag);
        HIPCHK(c, hipGetLastError());
        launch_excl_scan(st, flag, bs, m);
        long long nb = 0;
        if (int rc = cl_count(c, bs + m, &nb)) return rc;
        ni = nb / 2;
        if (ni > 0) {
            unsigned long long* istart = (unsigned long long*)grab(8 * (size_t)ni);
            unsigned long long* iend = (unsigned long long*)grab(8 * (size_t)ni);
            int* head = (int*)grab(4 * (size_t)ni);
            long long* cs = (long long*)grab(8 * (size_t)(ni + 1));
            if (!istart || !iend || !head || !cs) return fail(c, -6, "device allocation failed (cluster scan)");
            hipLaunchKernelGGL(cl_island_write_kernel, dim3(cl_grid(m)), dim3(CL_NT), 0, st, mkey, flag, bs, m, ni, istart, iend);
            hipLaunchKernelGGL(cl_cluster_head_kernel, dim3(cl_grid(ni)), dim3(CL_NT), 0, st, istart, iend, ni, (long long)o->pad, head);
            launch_excl_scan(st, head, cs, ni);
            HIPCHK(c, hipGetLastError());
            if (int rc = cl_count(c, cs + ni, &nc)) return rc;
            unsigned long long* cstart = (unsigned long long*)grab(8 * (size_t)nc);
            unsigned long long* cend = (unsigned long long*)grab(8 * (size_t)nc);
            // per-cluster accumulators, one allocation: reads, plus, placements, cmax, cmaj, sizes[7], samples[S], then total, assigned, bad flag
            const size_t nacc = (size_t)nc * (12 + (size_t)S) + 3;
            unsigned long long* acc = (unsigned long long*)grab(8 * nacc);
            int* cid = (int*)grab(4 * (size_t)n);
            int* asg = (int*)grab(4 * (size_t)n);
            long long* as = (long long*)grab(8 * (size_t)(n + 1));
            d_out = (MirpCluster*)grab(sizeof(MirpCluster) * (size_t)nc);
            if (!cstart || !cend || !acc || !cid || !asg || !as || !d_out) return fail(c, -6, "device allocation failed (cluster scan)");
            hipLaunchKernelGGL(cl_cluster_write_kernel, dim3(cl_grid(ni)), dim3(CL_NT), 0, st, istart, iend, head, cs, ni, cstart, cend);
            HIPCHK(c, hipMemsetAsync(acc, 0, 8 * nacc, st));
            unsigned long long* placements = acc + 2 * (size_t)nc;
            unsigned long long* cmax = acc + 3 * (size_t)nc;
            unsigned long long* cmaj = acc + 4 * (size_t)nc;
            HIPCHK(c, hipMemsetAsync(cmaj, 0xff, 8 * (size_t)nc, st));
            ClSums Su;
            Su.reads = acc;
            Su.plus = acc + (size_t)nc;
            Su.sizes = acc + 5 * (size_t)nc;
            Su.samples = acc + 12 * (size_t)nc;
            Su.total = acc + (12 + (size_t)S) * (size_t)nc;
            Su.assigned = Su.total + 1;
            Su.bad_sample = (int*)(Su.total + 2);
            d_samples = Su.samples;
            hipLaunchKernelGGL(cl_assign_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, n, d_clen, o->n_contigs, cstart, cend, nc, S, Su, cid, asg);
            launch_excl_scan(st, asg, as, n);
            HIPCHK(c, hipGetLastError());
            unsigned long long h_tail[3];
            HIPCHK(c, hipMemcpyAsync(h_tail, Su.total, 24, hipMemcpyDeviceToHost, st));
            if (int rc = cl_count(c, as + n, &nA)) return rc;
            h_sum[0] = h_tail[0];
            h_sum[1] = h_tail[1];
            if ((int)(h_tail[2] & 0xffffffffu)) return fail(c, -1, "mirp_cluster_scan: a record's sample index is not below n_samples");
            // placements: the records of one cluster, grouped by (pos, strand, len)
            MirpHashRec* pl = ends;                    // the end events are no longer needed
            MirpHashRec* ptmp = tmp;
            hipLaunchKernelGGL(cl_place_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, n, cid, as, pl);
            HIPCHK(c, hipGetLastError());
            if (int rc = mirp_device_sort_hashes(c, pl, ptmp, nA, 17 + cl_bits(n - 1))) return rc;
            int* plo = lo;
            int* phi = asg;                            // nA <= n entries
            long long* splo = shi;
            long long* sphi = as;
            unsigned long long* rsum = skey;
            hipLaunchKernelGGL(cl_run_kernel, dim3(cl_grid(nA)), dim3(CL_NT), 0, st, pl, nA, plo, phi);
            launch_excl_scan(st, plo, splo, nA);
            launch_excl_scan(st, phi, sphi, nA);
            hipLaunchKernelGGL(cl_run_sum_kernel, dim3(cl_grid(nA)), dim3(CL_NT), 0, st, pl, nA, splo, sphi, rsum, placements, cmax);
            hipLaunchKernelGGL(cl_major_kernel, dim3(cl_grid(nA)), dim3(CL_NT), 0, st, pl, nA, rsum, cmax, cmaj);
            hipLaunchKernelGGL(cl_out_kernel, dim3(cl_grid(nc)), dim3(CL_NT), 0, st, alns, cstart, cend, nc, Su, placements, cmax, cmaj, pl, d_out);
            HIPCHK(c, hipGetLastError());
        }
        if (ni == 0) {                                 // no island: only the total is left to count
            unsigned long long* acc = (unsigned long long*)grab(8 * 3);
            int* cid = (int*)grab(4 * (size_t)n);
            if (!acc || !cid) return fail(c, -6, "device allocation failed (cluster scan)");
            HIPCHK(c, hipMemsetAsync(acc, 0, 24, st));
            ClSums Su = {nullptr, nullptr, nullptr, nullptr, acc, acc + 1, (int*)(acc + 2)};
            hipLaunchKernelGGL(cl_assign_kernel, dim3(cl_grid(n)), dim3(CL_NT), 0, st, alns, n, d_clen, o->n_contigs, (const unsigned long long*)nullptr,
                               (const unsigned long long*)nullptr, 0ll, S, Su, cid, lo);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(h_sum, acc, 16, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
    }
    MirpCluster* h_out = (MirpCluster*)std::malloc(sizeof(MirpCluster) * (size_t)std::max(nc, 1ll));
    int64_t* h_samples = (int64_t*)std::malloc(8 * (size_t)std::max(nc * S, 1ll));
    if (!h_out || !h_samples) {
        std::free(h_out);
        std::free(h_samples);
        return fail(c, -6, "host allocation failed (cluster scan)");
    }
    if (nc > 0) {
        hipError_t e = hipMemcpyAsync(h_out, d_out, sizeof(MirpCluster) * (size_t)nc, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_samples, d_samples, 8 * (size_t)nc * S, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            std::free(h_out);
            std::free(h_samples);
            return fail(c, -2, std::string("mirp_cluster_scan: ") + hipGetErrorString(e));
        }
    }
    *clusters = h_out;
    *n_clusters = nc;
    *sample_counts = h_samples;
    if (stats) {
        stats[0] = n;
        stats[1] = (long long)h_sum[0];
        stats[2] = ni;
        stats[3] = nc;
        stats[4] = (long long)h_sum[1];
    }
    return 0;
}
