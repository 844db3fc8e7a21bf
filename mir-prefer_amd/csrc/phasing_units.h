// The unit arrays of the phasing test, shared by the window scan of mirp_phase_scan (phasing_kernels.hip) and the trigger scan of
// mirp_trigger_scan (trigger_kernels.hip, §29): the units of one length on the context's resident alignments, + stream then - stream, each sorted
// by the key tid << 32 | c, with exact 64-bit abundance prefixes; the binary searches over them and the bounded counting of one strand of a window.
#pragma once
#include <hip/hip_runtime.h>
#include "mirp_ctx.h"

namespace mirp {

struct PhUnits {
    const unsigned long long* key;   // + units [0, np), - units [np, n)
    const long long* slo;            // prefix sums of the abundance, low 30 bits / the rest (n + 1 entries)
    const long long* shi;
    long long np, n;
};

// Builds the units of length L with abundance >= min_depth from c->alns (ph_flag_kernel .. ph_compact_kernel and the scans of phasing_kernels.hip)
// into allocations of T; *records = the records of length L.  With no unit left U->n is 0 and its arrays are null.
int ph_build_units(mirp_ctx* c, int L, int min_depth, TmpDevice& T, PhUnits* U, long long* records);

// first index in [lo, hi) whose key is >= t (hi if none)
__device__ __forceinline__ long long ph_lower(const unsigned long long* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// first index in [lo, hi) whose key is > t
__device__ __forceinline__ long long ph_upper(const unsigned long long* __restrict__ a, long long lo, long long hi, unsigned long long t) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long long ph_prefix(const PhUnits& U, long long v) { return (U.shi[v] << 30) + U.slo[v]; }

// One strand of the window of register x: its units are [b, hi) (b = the lower bound of the window's first key, hi of its end), and phased
// coordinate j0 + i, i = 0 .. cycles - 1, has the key t0 + i L; t0 is the window's first key or, for a window that starts below coordinate 0,
// at most L - 1 above it.  Each phased key is found by a binary search over at most L units that starts where the previous one stopped (the keys
// are distinct integers and cur's key is >= t - L), so the strand costs O(m log L) also when every coordinate is taken.  exact0: b is t0's lower
// bound, which needs no search.
template <int EMIT>
__device__ __forceinline__ void ph_count_phased(const PhUnits& U, long long b, long long hi, unsigned long long t0, int L, int cycles, bool exact0, int& k,
                                                long long& phased) {
    long long cur = b;
    for (int j = 0; j < cycles && cur < hi; j++) {
        const unsigned long long t = t0 + (unsigned long long)(j * L);
        const long long p = j || !exact0 ? ph_lower(U.key, cur, cur + L < hi ? cur + L : hi, t) : cur;
        if (p < hi && U.key[p] == t) {
            k++;
            if (EMIT) phased += ph_prefix(U, p + 1) - ph_prefix(U, p);
            cur = p + 1;
        } else {
            cur = p;
        }
    }
}

// one strand of the window [x, x + mL) of anchor key x: units from b (the anchor's lower bound in this strand) to e (the strand's end)
template <int EMIT>
__device__ __forceinline__ void ph_strand(const PhUnits& U, long long b, long long e, unsigned long long x, int L, int m, int& n, int& k,
                                          long long& phased, long long& reads) {
    const long long cap = b + (long long)m * L;
    const long long hi = ph_lower(U.key, b, cap < e ? cap : e, x + (unsigned long long)(m * L));
    n += (int)(hi - b);
    if (EMIT) reads += ph_prefix(U, hi) - ph_prefix(U, b);
    ph_count_phased<EMIT>(U, b, hi, x, L, m, true, k, phased);
}

}  // namespace mirp
