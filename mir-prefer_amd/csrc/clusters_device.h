// Device helpers of the scans over the resident alignments (clusters_kernels.hip, loci_kernels.hip): the clipped span of a record as 64-bit keys,
// binary searches over sorted keys and the exact 64-bit prefix from two int32 scans.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mirp_ctx.h"

namespace mirp {

#define CL_NT 256
#define CL_NCLS 7            // size classes: < 20, 20, 21, 22, 23, 24, > 24

static inline unsigned cl_grid(long long n) { return (unsigned)std::max(1ll, std::min((n + CL_NT - 1) / CL_NT, 1ll << 20)); }

struct ClSpan {
    unsigned long long s, e;     // [s, e) as keys; s is monotone in record order also when the span is empty (then e == s)
    bool ok;
};

__device__ __forceinline__ ClSpan cl_span(const MirpAln& r, const long long* __restrict__ clen, int n_contigs) {
    const long long ln = (r.tid >= 0 && r.tid < n_contigs) ? clen[r.tid] : 0;
    const long long s = r.pos > 1 ? (long long)r.pos : 1;
    const long long e = std::min((long long)r.pos + (long long)r.len, ln + 1);
    const unsigned long long t = (unsigned long long)(unsigned)r.tid << 32;
    ClSpan o;
    o.ok = s < e;
    o.s = t + (unsigned long long)s;
    o.e = o.ok ? t + (unsigned long long)e : o.s;
    return o;
}

// first index in [lo, hi) whose key is >= t (hi if none)
__device__ __forceinline__ long long cl_lower(const unsigned long long* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ long long cl_lower_rec(const MirpHashRec* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid].hash < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// first index in [lo, hi) whose key is > t
__device__ __forceinline__ long long cl_upper(const unsigned long long* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ long long cl_upper_rec(const MirpHashRec* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid].hash <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// exact 64-bit prefix from the two int32 scans of the low 30 bits and the rest
__device__ __forceinline__ long long cl_prefix(const long long* __restrict__ slo, const long long* __restrict__ shi, long long i) {
    return (shi[i] << 30) + slo[i];
}

}  // namespace mirp
