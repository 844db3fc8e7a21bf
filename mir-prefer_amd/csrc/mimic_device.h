// Device functions of the target-mimic scan (mimic_kernels.hip): the seed key, the 38-base span of a lane as bit planes, and the
// choice of the loop position from two window evaluations.  Windows, masks and pair classes are those of targets_device.h / targets_bulge_device.h.
#pragma once
#include "targets_bulge_device.h"

namespace mirp {

#define MM_SHIFT 38                  // key: miRNA (file order) << 38 | imperfect << 35 | start << 3 | strand << 2 | (P - 9)
#define MM_NBIN 8                    // imperfect 0 .. 6 (one bin spare)
#define MM_STAT_SLOTS 1024           // addresses the waves' lookup counts are spread over (a power of two)

// the reverse complement of a 7-mer held as 14 bits (first base in the low bits)
__device__ __forceinline__ unsigned mm_revcomp7(unsigned k) {
    unsigned x = __brev(~k & 0x3fffu);                              // base order reversed, and the two bits of every base swapped
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    return x >> 18;
}

// 64 positions from b = q - back as bit planes (pl / ph as in tg_even) and as bitmaps of the ambiguous bases (am) and the contig starts (cs); where
// q < back the positions before 0 count as ambiguous.  The caller uses bits 0 .. 37.
struct MmSpan { unsigned long long pl, ph, am, cs; };

__device__ __forceinline__ MmSpan mm_span(const TgRef& R, unsigned long long q, unsigned back) {
    const unsigned d = q >= back ? 0u : back - (unsigned)q;
    const unsigned long long b = q + d - back;
    const unsigned long long w = b >> 5;
    const unsigned sh = 2 * (unsigned)(b & 31), sa = (unsigned)(b & 31);
    unsigned long long lo = R.pk[w], hi = R.pk[w + 1];
    unsigned long long am = R.amb[w] | ((unsigned long long)R.amb[w + 1] << 32), cs = R.cst[w] | ((unsigned long long)R.cst[w + 1] << 32);
    if (sa) {
        lo = (lo >> sh) | (hi << (64 - sh));
        hi = (hi >> sh) | (R.pk[w + 2] << (64 - sh));
        am = (am >> sa) | ((unsigned long long)R.amb[w + 2] << (64 - sa));
        cs = (cs >> sa) | ((unsigned long long)R.cst[w + 2] << (64 - sa));
    }
    MmSpan S;
    S.pl = tg_even(lo) | ((unsigned long long)tg_even(hi) << 32);
    S.ph = tg_even(lo >> 1) | ((unsigned long long)tg_even(hi >> 1) << 32);
    S.am = (am << d) | ((1ull << d) - 1ull);
    S.cs = cs << d;
    S.pl <<= d;
    S.ph <<= d;
    return S;
}

// the n bases from bit sh of the span are unambiguous bases of one contig (sh + n <= 38)
__device__ __forceinline__ bool mm_span_clear(const MmSpan& S, unsigned sh, unsigned n) {
    const unsigned long long m = ((1ull << n) - 1ull) << sh;
    return ((S.am & m) | (S.cs & m & ~(1ull << sh))) == 0;
}

// The loop position of one (interval, miRNA, strand) whose positions 2..8 are Watson-Crick pairs: among P = 9, 10, 11 (P < L) whose closing pairs P
// and P + 1 are not mismatches, the lowest imperfect = non-Watson-Crick pairs, the smallest P on a tie.  (nwA, mmA): the evaluation of the window
// that pairs positions 1..P, (nwB, mmB): of the one that pairs P + 1..L.  -> imperfect << 8 | P, or ~0u when no P closes the loop.
__device__ __forceinline__ unsigned mm_best(unsigned lmask, int L, int s, unsigned nwA, unsigned mmA, unsigned nwB, unsigned mmB) {
    unsigned best = ~0u, bp = 0;
    #pragma unroll
    for (int P = 9; P <= 11; P++) {
        if (P >= L) break;
        const unsigned MA = s ? (1u << P) - 1u : lmask & ~((1u << (L - P)) - 1u);
        const unsigned MB = lmask & ~MA;
        const unsigned close = s ? 3u << (P - 1) : 3u << (L - P - 1);        // window positions of P and P + 1
        const unsigned nw = (nwA & MA) | (nwB & MB), mm = (mmA & MA) | (mmB & MB);
        if (mm & close) continue;
        const unsigned h = __popc(nw);
        if (h < best) { best = h; bp = (unsigned)P; }
    }
    return best == ~0u ? ~0u : best << 8 | bp;
}

}  // namespace mirp
