// isomiR counts: aligned records with their 3' tail codes joined against annotated miRNA loci, grouped into isomiRs and summed per sample
// (mirp_isomir_scan).  The host (isomirs.py) reads the annotation, names the columns and writes the files; everything per record,
// per isomiR and per locus runs here, in exact integer arithmetic.
//
// The loci are sorted on the host by tid << 33 | strand << 32 | l5 (l5 = the 5' end: start on +, end on -; below 2^32) and keep their file-order
// number.  A record's r5 = pos (+) or pos + len - 1 (-) is below 2^31 + 2^16, so r5 +- 15 neither wraps 64 bits nor leaves the key's 32.
//   assign   iso_assign_kernel, one record per lane: one binary search for the first locus of the record's (tid, strand) with l5 >= r5 - max5, then
//            a walk over the loci with l5 <= r5 + max5 that keeps the admitting one with the smallest (|d5|, |d3|, number).  The key is
//            locus << 37 | d5 + 15 << 32 | d3 + 15 << 27 | tail << 8 | sample with the depth as payload; a scan compacts the assigned records
//            (iso_compact_kernel) and the radix sort of the read collapse (mirp_device_sort_hashes) orders them.
//   runs     iso_head_kernel flags the first record of every (isomiR, sample) run and of every isomiR run and splits the depths into their low 30
//            bits and the rest; four scans number the runs and give exact 64-bit depth prefixes.
//   sums     iso_isomir_kernel: the head of an isomiR run finds its end by one binary search, writes the isomiR and adds its sum to the locus'
//            totals and classes; iso_sample_kernel does the same per (isomiR, sample) run for the two count matrices; iso_major_kernel takes the
//            first isomiR that reaches the locus' maximum.
// Sums, maxima and minima per locus are integer atomics, one per distinct address of a wave (cl_wave_atomic): a hotspot locus costs one atomic
// per wave, no lane loops over records, and no result depends on scheduling.  The grids are capped, so a resident wave takes further records in
// strides of the grid.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mirp_ctx.h"
#include "wave_atomic.h"

namespace mirp {

#define ISO_NT 256
#define ISO_MAX_BLOCKS 1024          // 4 workgroups of 4 waves per CU
#define ISO_NSUM 11                  // int64 fields of MirpIsoLocusSum
#define ISO_F_MAJOR_READS 9
#define ISO_F_MAJOR 10

static inline unsigned iso_grid(long long n) { return (unsigned)std::max(1ll, std::min((n + ISO_NT - 1) / ISO_NT, (long long)ISO_MAX_BLOCKS)); }

struct IsoLoci {
    const unsigned long long* key;   // tid << 33 | strand << 32 | l5, ascending
    const long long* l3;
    const int* num;                  // file-order number
    long long n;
};

// exact 64-bit prefix from the two int32 scans of the low 30 bits and the rest
__device__ __forceinline__ long long iso_prefix(const long long* __restrict__ slo, const long long* __restrict__ shi, long long i) {
    return (shi[i] << 30) + slo[i];
}

// first index in (lo, hi) whose key >> shift differs from t (hi if none); the keys are sorted
__device__ __forceinline__ long long iso_run_end(const MirpHashRec* __restrict__ a, long long lo, long long hi, unsigned long long t, int shift) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((a[mid].hash >> shift) <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(ISO_NT) iso_assign_kernel(const MirpAln* __restrict__ a, const unsigned* __restrict__ tails, long long n, IsoLoci L,
                                                            int max5, int max3, int n_samples, unsigned long long* __restrict__ keys,
                                                            int* __restrict__ flag, int* __restrict__ bad_sample) {
    for (long long i = (long long)blockIdx.x * ISO_NT + threadIdx.x; i < n; i += (long long)gridDim.x * ISO_NT) {
        const MirpAln r = a[i];
        unsigned long long best = ~0ull;     // |d5| << 29 | |d3| << 24 | number
        long long bd5 = 0, bd3 = 0;
        if (r.tid >= 0 && r.strand < 2 && r.pos >= 0 && r.len > 0) {
            const long long p = r.pos, q = p + (long long)r.len - 1;
            const long long r5 = r.strand ? q : p, r3 = r.strand ? p : q;
            const long long sg = r.strand ? -1 : 1;
            const unsigned long long g = ((unsigned long long)(unsigned)r.tid << 33) | ((unsigned long long)r.strand << 32);
            const unsigned long long first = g | (unsigned long long)std::max(r5 - max5, 0ll), last = g | (unsigned long long)(r5 + max5);
            long long lo = 0, hi = L.n;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (L.key[mid] < first) lo = mid + 1;
                else hi = mid;
            }
            for (long long k = lo; k < L.n; k++) {
                const unsigned long long lk = L.key[k];
                if (lk > last) break;
                const long long d5 = sg * (r5 - (long long)(lk & 0xffffffffull));
                const long long d3 = sg * (r3 - L.l3[k]);
                const long long a5 = d5 < 0 ? -d5 : d5, a3 = d3 < 0 ? -d3 : d3;
                if (a5 > max5 || a3 > max3) continue;
                const unsigned long long c = ((unsigned long long)a5 << 29) | ((unsigned long long)a3 << 24) | (unsigned long long)(unsigned)L.num[k];
                if (c < best) { best = c; bd5 = d5; bd3 = d3; }
            }
        }
        bool took = best != ~0ull;
        if (took && r.sample >= n_samples) {
            atomicOr(bad_sample, 1);
            took = false;
        }
        unsigned long long key = ~0ull;
        if (took)
            key = ((best & 0xffffffull) << 37) | ((unsigned long long)(bd5 + 15) << 32) | ((unsigned long long)(bd3 + 15) << 27) |
                  ((unsigned long long)(tails[i] & 0x7ffffu) << 8) | (unsigned long long)r.sample;
        keys[i] = key;
        flag[i] = took;
    }
}

__global__ void __launch_bounds__(ISO_NT) iso_compact_kernel(const MirpAln* __restrict__ a, const unsigned long long* __restrict__ keys,
                                                             const int* __restrict__ flag, const long long* __restrict__ at, long long n,
                                                             MirpHashRec* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * ISO_NT + threadIdx.x; i < n; i += (long long)gridDim.x * ISO_NT) {
        if (!flag[i]) continue;
        MirpHashRec p;
        p.hash = keys[i];
        p.idx = a[i].depth;
        p.pad = 0;
        out[at[i]] = p;
    }
}

__global__ void __launch_bounds__(ISO_NT) iso_head_kernel(const MirpHashRec* __restrict__ p, long long n, int* __restrict__ hs, int* __restrict__ hi,
                                                          int* __restrict__ dlo, int* __restrict__ dhi) {
    for (long long j = (long long)blockIdx.x * ISO_NT + threadIdx.x; j < n; j += (long long)gridDim.x * ISO_NT) {
        const MirpHashRec q = p[j];
        const unsigned long long prev = j ? p[j - 1].hash : ~q.hash;
        hs[j] = prev != q.hash;
        hi[j] = (prev >> 8) != (q.hash >> 8);
        dlo[j] = (int)(q.idx & 0x3fffffffu);
        dhi[j] = (int)(q.idx >> 30);
    }
}

// tail code -> 1: every letter A, 2: every letter T, 0: anything else (none included).  A tail of t letters has the codes off(t) .. off(t + 1) - 1
// with off(t) = (5^t - 5) / 4 + 1; all A is the first of them, all T lies 3 (5^t - 1) / 4 above it.
__device__ __forceinline__ int iso_tail_class(unsigned code) {
    unsigned pw = 5;
#pragma unroll
    for (int t = 1; t <= 8; t++) {
        const unsigned off = (pw - 5) / 4 + 1;
        if (code == off) return 1;
        if (code == off + 3 * ((pw - 1) / 4)) return 2;
        pw *= 5;
    }
    return 0;
}

__global__ void __launch_bounds__(ISO_NT) iso_init_kernel(unsigned long long* __restrict__ sums, long long n_loci) {
    for (long long k = (long long)blockIdx.x * ISO_NT + threadIdx.x; k < n_loci * ISO_NSUM; k += (long long)gridDim.x * ISO_NT)
        sums[k] = (k % ISO_NSUM) == ISO_F_MAJOR ? ~0ull : 0ull;
}

__global__ void __launch_bounds__(ISO_NT) iso_isomir_kernel(const MirpHashRec* __restrict__ p, long long n, const int* __restrict__ hi,
                                                            const long long* __restrict__ si, const long long* __restrict__ slo,
                                                            const long long* __restrict__ shi, MirpIsomir* __restrict__ out,
                                                            unsigned long long* __restrict__ sums) {
    for (long long base = (long long)blockIdx.x * ISO_NT; base < n; base += (long long)gridDim.x * ISO_NT) {
        const long long j = base + threadIdx.x;
        long long c = -1;
        unsigned long long s = 0;
        int d5 = 0, d3 = 0, cls = 0;
        unsigned tail = 0;
        if (j < n && hi[j]) {
            const unsigned long long k = p[j].hash;
            const long long e = iso_run_end(p, j + 1, n, k >> 8, 8);
            s = (unsigned long long)(iso_prefix(slo, shi, e) - iso_prefix(slo, shi, j));
            c = (long long)(k >> 37);
            d5 = (int)((k >> 32) & 31) - 15;
            d3 = (int)((k >> 27) & 31) - 15;
            tail = (unsigned)((k >> 8) & 0x7ffffu);
            cls = iso_tail_class(tail);
            MirpIsomir o;
            o.locus = (int)c;
            o.d5 = d5;
            o.d3 = d3;
            o.tail = tail;
            o.reads = (long long)s;
            out[si[j]] = o;
        }
        const long long b = c * ISO_NSUM;
        cl_wave_atomic<0>(sums, c >= 0 ? b + 0 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && !d5 && !d3 && !tail ? b + 1 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && d5 ? b + 2 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && d3 < 0 ? b + 3 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && d3 > 0 ? b + 4 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && tail ? b + 5 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && cls == 2 ? b + 6 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 && cls == 1 ? b + 7 : -1, s);
        cl_wave_atomic<0>(sums, c >= 0 ? b + 8 : -1, 1ull);
        cl_wave_atomic<1>(sums, c >= 0 ? b + ISO_F_MAJOR_READS : -1, s);
    }
}

__global__ void __launch_bounds__(ISO_NT) iso_major_kernel(const MirpIsomir* __restrict__ iso, long long ni, unsigned long long* __restrict__ sums) {
    for (long long base = (long long)blockIdx.x * ISO_NT; base < ni; base += (long long)gridDim.x * ISO_NT) {
        const long long q = base + threadIdx.x;
        long long slot = -1;
        if (q < ni) {
            const MirpIsomir o = iso[q];
            if ((unsigned long long)o.reads == sums[(long long)o.locus * ISO_NSUM + ISO_F_MAJOR_READS]) slot = (long long)o.locus * ISO_NSUM + ISO_F_MAJOR;
        }
        cl_wave_atomic<2>(sums, slot, (unsigned long long)q);
    }
}

__global__ void __launch_bounds__(ISO_NT) iso_sample_kernel(const MirpHashRec* __restrict__ p, long long n, const int* __restrict__ hs,
                                                            const long long* __restrict__ si, const long long* __restrict__ slo,
                                                            const long long* __restrict__ shi, int n_samples,
                                                            unsigned long long* __restrict__ iso_counts, unsigned long long* __restrict__ locus_counts) {
    for (long long base = (long long)blockIdx.x * ISO_NT; base < n; base += (long long)gridDim.x * ISO_NT) {
        const long long j = base + threadIdx.x;
        long long slot = -1;
        unsigned long long s = 0;
        if (j < n && hs[j]) {
            const unsigned long long k = p[j].hash;
            const long long e = iso_run_end(p, j + 1, n, k, 0);
            s = (unsigned long long)(iso_prefix(slo, shi, e) - iso_prefix(slo, shi, j));
            const long long sample = (long long)(k & 0xff);
            // si[j] counts the isomiR heads before j; j's own run started at or before j, so its isomiR is si[j + 1] - 1
            iso_counts[(si[j + 1] - 1) * n_samples + sample] = s;
            slot = (long long)(k >> 37) * n_samples + sample;
        }
        cl_wave_atomic<0>(locus_counts, slot, s);
    }
}

}  // namespace mirp

namespace {

int iso_bits(long long v) {      // bits of the largest value v
    int b = 0;
    while (b < 63 && (1ll << b) <= v) b++;
    return b;
}

}  // namespace

extern "C" int mirp_isomir_scan(mirp_ctx* c, const MirpAln* alns, const uint32_t* tails, int64_t n, const MirpIsoLocus* loci, int64_t n_loci,
                                const MirpIsomirOpts* o, MirpIsomir** isomirs, int64_t* n_isomirs, MirpIsoLocusSum** sums, int64_t** locus_counts,
                                int64_t** isomir_counts, int64_t stats[4]) {
    using namespace mirp;
    if (!c) return -1;
    if (!o || !loci || !isomirs || !n_isomirs || !sums || !locus_counts || !isomir_counts || n < 0 || (n > 0 && (!alns || !tails)))
        return fail(c, -1, "mirp_isomir_scan: bad argument");
    if (o->max5 < 0 || o->max5 > 15 || o->max3 < 0 || o->max3 > 15 || o->n_samples < 1 || o->n_samples > MIRP_MAX_SAMPLES)
        return fail(c, -1, "mirp_isomir_scan: bad options");
    if (n_loci < 1 || n_loci > (1ll << 24)) return fail(c, -1, "mirp_isomir_scan: the number of loci must be between 1 and 2^24");
    if (n > (1ll << 31) - 2) return fail(c, -5, "mirp_isomir_scan: more than 2^31 records");
    static_assert(sizeof(MirpIsoLocusSum) == 8 * ISO_NSUM, "MirpIsoLocusSum is ISO_NSUM int64 fields");
    for (int64_t k = 0; k < n_loci; k++)
        if (loci[k].tid < 0 || loci[k].strand < 0 || loci[k].strand > 1 || loci[k].start < 1 || loci[k].end < loci[k].start || loci[k].end > 0x7fffffffll)
            return fail(c, -1, "mirp_isomir_scan: locus " + std::to_string(k) + " is not a 1-based interval on a strand of a contig");
    *isomirs = nullptr;
    *n_isomirs = 0;
    *sums = nullptr;
    *locus_counts = nullptr;
    *isomir_counts = nullptr;
    const int S = o->n_samples;
    // the loci by (tid, strand, 5' end); ties keep file order (the walk compares numbers anyway)
    std::vector<int> order((size_t)n_loci);
    std::vector<unsigned long long> h_key((size_t)n_loci);
    std::vector<long long> h_l3((size_t)n_loci);
    for (int64_t k = 0; k < n_loci; k++) order[(size_t)k] = (int)k;
    auto key_of = [&](int k) {
        const MirpIsoLocus& l = loci[k];
        return ((unsigned long long)(unsigned)l.tid << 33) | ((unsigned long long)l.strand << 32) | (unsigned long long)(l.strand ? l.end : l.start);
    };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key_of(x) < key_of(y); });
    for (int64_t k = 0; k < n_loci; k++) {
        const MirpIsoLocus& l = loci[order[(size_t)k]];
        h_key[(size_t)k] = key_of(order[(size_t)k]);
        h_l3[(size_t)k] = l.strand ? l.start : l.end;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    TmpDevice T;
    auto grab = [&](size_t bytes) { return T.get(bytes); };
    MirpIsoLocusSum* h_sums = (MirpIsoLocusSum*)std::malloc(sizeof(MirpIsoLocusSum) * (size_t)n_loci);
    int64_t* h_lc = (int64_t*)std::malloc(8 * (size_t)n_loci * (size_t)S);
    MirpIsomir* h_iso = nullptr;
    int64_t* h_ic = nullptr;
    auto bail = [&](int code, const std::string& m) {
        std::free(h_sums); std::free(h_lc); std::free(h_iso); std::free(h_ic);
        return fail(c, code, m);
    };
    if (!h_sums || !h_lc) return bail(-6, "host allocation failed (isomir scan)");
    long long nA = 0, nI = 0;
#define ISO_HIP(call)                                                                                            \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) return bail(-2, std::string("mirp_isomir_scan: ") + hipGetErrorString(e_));        \
    } while (0)
    unsigned long long* d_sums = (unsigned long long*)grab(8 * (size_t)n_loci * ISO_NSUM);
    unsigned long long* d_lc = (unsigned long long*)grab(8 * (size_t)n_loci * (size_t)S);
    if (!d_sums || !d_lc) return bail(-6, "device allocation failed (isomir scan)");
    hipLaunchKernelGGL(iso_init_kernel, dim3(iso_grid(n_loci * ISO_NSUM)), dim3(ISO_NT), 0, st, d_sums, (long long)n_loci);
    ISO_HIP(hipMemsetAsync(d_lc, 0, 8 * (size_t)n_loci * (size_t)S, st));
    MirpIsomir* d_iso = nullptr;
    unsigned long long* d_ic = nullptr;
    if (n > 0) {
        unsigned long long* d_key = (unsigned long long*)grab(8 * (size_t)n_loci);
        long long* d_l3 = (long long*)grab(8 * (size_t)n_loci);
        int* d_num = (int*)grab(4 * (size_t)n_loci);
        MirpAln* d_alns = (MirpAln*)grab(sizeof(MirpAln) * (size_t)n);
        unsigned* d_tails = (unsigned*)grab(4 * (size_t)n);
        unsigned long long* d_rkey = (unsigned long long*)grab(8 * (size_t)n);
        int* d_flag = (int*)grab(4 * (size_t)n + 4);
        long long* d_at = (long long*)grab(8 * (size_t)(n + 1));
        if (!d_key || !d_l3 || !d_num || !d_alns || !d_tails || !d_rkey || !d_flag || !d_at) return bail(-6, "device allocation failed (isomir scan)");
        int* d_bad = d_flag + n;
        ISO_HIP(hipMemcpyAsync(d_key, h_key.data(), 8 * (size_t)n_loci, hipMemcpyHostToDevice, st));
        ISO_HIP(hipMemcpyAsync(d_l3, h_l3.data(), 8 * (size_t)n_loci, hipMemcpyHostToDevice, st));
        ISO_HIP(hipMemcpyAsync(d_num, order.data(), 4 * (size_t)n_loci, hipMemcpyHostToDevice, st));
        ISO_HIP(hipMemcpyAsync(d_alns, alns, sizeof(MirpAln) * (size_t)n, hipMemcpyHostToDevice, st));
        ISO_HIP(hipMemcpyAsync(d_tails, tails, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        ISO_HIP(hipMemsetAsync(d_bad, 0, 4, st));
        const IsoLoci L = {d_key, d_l3, d_num, (long long)n_loci};
        hipLaunchKernelGGL(iso_assign_kernel, dim3(iso_grid(n)), dim3(ISO_NT), 0, st, (const MirpAln*)d_alns, (const unsigned*)d_tails, (long long)n, L,
                           o->max5, o->max3, S, d_rkey, d_flag, d_bad);
        launch_excl_scan(st, d_flag, d_at, n);
        ISO_HIP(hipGetLastError());
        int h_bad = 0;
        ISO_HIP(hipMemcpyAsync(&nA, d_at + n, 8, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        if (h_bad) return bail(-1, "mirp_isomir_scan: a record's sample index is not below n_samples");
        if (nA > 0) {
            MirpHashRec* rec = (MirpHashRec*)grab(16 * (size_t)nA);
            MirpHashRec* tmp = (MirpHashRec*)grab(16 * (size_t)nA);
            int* hs = (int*)grab(4 * (size_t)nA);
            int* hi = (int*)grab(4 * (size_t)nA);
            int* dlo = (int*)grab(4 * (size_t)nA);
            int* dhi = (int*)grab(4 * (size_t)nA);
            long long* si = (long long*)grab(8 * (size_t)(nA + 1));
            long long* slo = (long long*)grab(8 * (size_t)(nA + 1));
            long long* shi = (long long*)grab(8 * (size_t)(nA + 1));
            if (!rec || !tmp || !hs || !hi || !dlo || !dhi || !si || !slo || !shi) return bail(-6, "device allocation failed (isomir scan)");
            hipLaunchKernelGGL(iso_compact_kernel, dim3(iso_grid(n)), dim3(ISO_NT), 0, st, (const MirpAln*)d_alns, (const unsigned long long*)d_rkey,
                               (const int*)d_flag, (const long long*)d_at, (long long)n, rec);
            ISO_HIP(hipGetLastError());
            if (int rc = mirp_device_sort_hashes(c, rec, tmp, nA, 37 + iso_bits(n_loci - 1))) { bail(rc, c->err); return rc; }
            hipLaunchKernelGGL(iso_head_kernel, dim3(iso_grid(nA)), dim3(ISO_NT), 0, st, (const MirpHashRec*)rec, nA, hs, hi, dlo, dhi);
            launch_excl_scan(st, hi, si, nA);
            launch_excl_scan(st, dlo, slo, nA);
            launch_excl_scan(st, dhi, shi, nA);
            ISO_HIP(hipGetLastError());
            ISO_HIP(hipMemcpyAsync(&nI, si + nA, 8, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipStreamSynchronize(st));
            d_iso = (MirpIsomir*)grab(sizeof(MirpIsomir) * (size_t)nI);
            d_ic = (unsigned long long*)grab(8 * (size_t)nI * (size_t)S);
            if (!d_iso || !d_ic) return bail(-6, "device allocation failed (isomir scan)");
            ISO_HIP(hipMemsetAsync(d_ic, 0, 8 * (size_t)nI * (size_t)S, st));
            hipLaunchKernelGGL(iso_isomir_kernel, dim3(iso_grid(nA)), dim3(ISO_NT), 0, st, (const MirpHashRec*)rec, nA, (const int*)hi, (const long long*)si,
                               (const long long*)slo, (const long long*)shi, d_iso, d_sums);
            hipLaunchKernelGGL(iso_major_kernel, dim3(iso_grid(nI)), dim3(ISO_NT), 0, st, (const MirpIsomir*)d_iso, nI, d_sums);
            hipLaunchKernelGGL(iso_sample_kernel, dim3(iso_grid(nA)), dim3(ISO_NT), 0, st, (const MirpHashRec*)rec, nA, (const int*)hs, (const long long*)si,
                               (const long long*)slo, (const long long*)shi, S, d_ic, d_lc);
            ISO_HIP(hipGetLastError());
            h_iso = (MirpIsomir*)std::malloc(sizeof(MirpIsomir) * (size_t)nI);
            h_ic = (int64_t*)std::malloc(8 * (size_t)nI * (size_t)S);
            if (!h_iso || !h_ic) return bail(-6, "host allocation failed (isomir scan)");
            ISO_HIP(hipMemcpyAsync(h_iso, d_iso, sizeof(MirpIsomir) * (size_t)nI, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipMemcpyAsync(h_ic, d_ic, 8 * (size_t)nI * (size_t)S, hipMemcpyDeviceToHost, st));
        }
    }
    ISO_HIP(hipGetLastError());
    ISO_HIP(hipMemcpyAsync(h_sums, d_sums, sizeof(MirpIsoLocusSum) * (size_t)n_loci, hipMemcpyDeviceToHost, st));
    ISO_HIP(hipMemcpyAsync(h_lc, d_lc, 8 * (size_t)n_loci * (size_t)S, hipMemcpyDeviceToHost, st));
    ISO_HIP(hipStreamSynchronize(st));
#undef ISO_HIP
    if (!h_iso) h_iso = (MirpIsomir*)std::malloc(sizeof(MirpIsomir));
    if (!h_ic) h_ic = (int64_t*)std::malloc(8);
    if (!h_iso || !h_ic) return bail(-6, "host allocation failed (isomir scan)");
    long long depth = 0;
    for (int64_t k = 0; k < n_loci; k++) depth += h_sums[k].reads;
    *isomirs = h_iso;
    *n_isomirs = nI;
    *sums = h_sums;
    *locus_counts = h_lc;
    *isomir_counts = h_ic;
    if (stats) {
        stats[0] = n;
        stats[1] = nA;
        stats[2] = depth;
        stats[3] = nI;
    }
    return 0;
}
