// What the scans over given loci share (loci_kernels.hip, signature_kernels.hip): a locus with its bounds as keys, the range of a sorted key
// table that holds a locus's partners, the (locus, chunk) jobs of a range and the resident grid that serves them.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mirp_ctx.h"
#include "clusters_device.h"

namespace mirp {

#define LC_C MIRP_LOCI_CHUNK
#define LC_WAVES (CL_NT / 64)

struct LcLocus {                 // MirpLocusSpan with the bounds as keys
    long long lo, hi;            // tid << 32 | start, tid << 32 | end
    int strand;                  // 0 '+', 1 '-', 2 none
};

__device__ __forceinline__ LcLocus lc_locus(const MirpLocusSpan& l) {
    LcLocus o;
    o.lo = ((long long)l.tid << 32) + l.start;
    o.hi = ((long long)l.tid << 32) + l.end;
    o.strand = l.strand;
    return o;
}

// tid << 32 | pos of row i of the records / of the placement table: monotone in either table (pos >= -2^31)
__device__ __forceinline__ long long lc_key(const MirpAln* __restrict__ a, long long i) { return ((long long)a[i].tid << 32) + (long long)a[i].pos; }
__device__ __forceinline__ long long lc_key(const long long* __restrict__ k, long long i) { return k[i]; }

// rows [first, first + C * jobs) of the table hold the partners of locus q: key in [lo - M + 1, hi]
template <typename Table>
__global__ void __launch_bounds__(CL_NT) lc_range_kernel(Table tab, long long n, const MirpLocusSpan* __restrict__ loci, long long nl,
                                                         const unsigned* __restrict__ maxlen, long long* __restrict__ first, long long* __restrict__ last,
                                                         int* __restrict__ jobs) {
    const long long M = *maxlen;
    for (long long q = (long long)blockIdx.x * CL_NT + threadIdx.x; q < nl; q += (long long)gridDim.x * CL_NT) {
        const LcLocus L = lc_locus(loci[q]);
        long long lo = 0, hi = n;                                   // first row with key >= L.lo - M + 1
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (lc_key(tab, mid) < L.lo - M + 1) lo = mid + 1;
            else hi = mid;
        }
        const long long f = lo;
        hi = n;                                                     // first row with key > L.hi
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (lc_key(tab, mid) <= L.hi) lo = mid + 1;
            else hi = mid;
        }
        first[q] = f;
        last[q] = lo;
        jobs[q] = (int)((lo - f + LC_C - 1) / LC_C);
    }
}

// the locus of job j: the last q with joff[q] <= j (a locus without jobs shares its offset with the next one and is skipped)
__device__ __forceinline__ long long lc_job_locus(const long long* __restrict__ joff, long long nl, long long j) {
    long long lo = 0, hi = nl;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (joff[mid + 1] <= j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

static inline int lc_bits(long long v) {      // bits of the largest value v
    int b = 0;
    while (b < 63 && (1ll << b) <= v) b++;
    return b;
}

// blocks of a wave-per-job launch: every job a wave of its own up to the resident cap of 4 blocks (16 waves) per CU
static inline unsigned lc_job_grid(const mirp_ctx* c, long long jobs) {
    return (unsigned)std::max(1ll, std::min((jobs + LC_WAVES - 1) / LC_WAVES, 4ll * std::max(c->n_cu, 1)));
}

}  // namespace mirp
