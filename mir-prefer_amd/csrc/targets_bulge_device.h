// The scan of the target-site search with --bulge ("Bulged sites"): next to every ungapped site U(o) it reports the sites with
// exactly one unpaired nucleotide whose interval starts at o.  A bulged site is the 5' part (miRNA positions up to P) of one ungapped alignment A
// joined to the 3' part of another, B, one base apart:
//     tP (target bulge, interval [o, o + L + 1)):  plus A = U(o + 1), B = U(o);  minus A = U(o), B = U(o + 1);  positions 1..P | P + 1..L
//     mP (miRNA bulge, interval [o, o + L - 1)):   plus A = U(o - 1), B = U(o);  minus A = U(o), B = U(o - 1);  positions 1..P - 1 | P + 1..L
// A lane holds the bit planes of the three windows at o - 1, o and o + 1 and evaluates the same TgStrand masks against each, so bit j is the same
// miRNA position in all three (j = L - i on the plus strand, i - 1 on the minus strand) and a placement is a bit select between two evaluations.
//
// Filter: a paired position costs at least what it costs in the cheaper of A and B, and that minimum is the cost of (nonwcA & nonwcB, mmA & mmB).
// A t site pairs every position and pays a gap of at least 2: bound + 2.  An m site leaves position P out, whose weighted cost is at most its gap
// (4 in 2..13, else 2): the bound itself.  Only lanes whose bound is within smax run the loop over P.
#pragma once
#include "targets_device.h"

namespace mirp {

#define TG_BULGE_SHIFT 45            // key: mloc << 45 | half << 40 | start << 8 | strand << 7 | kind << 5 | P; kind 0 = m, 1 = ungapped, 2 = t

__device__ __forceinline__ void tg_masks(const TgStrand& S, unsigned lmask, unsigned wl, unsigned wh, int s, unsigned* nonwc, unsigned* mm) {
    const unsigned n = ((wl ^ S.pl) | (wh ^ S.ph) | S.unk) & lmask;
    const unsigned x1 = s ? ~(wl | wh) : wl & wh, x2 = s ? wl & ~wh : ~wl & wh;        // plus: T, G; minus: A, C
    *nonwc = n;
    *mm = n & ~((x1 & S.g1) | (x2 & S.g2));
}

__device__ __forceinline__ unsigned tg_cost(unsigned nonwc, unsigned mm, unsigned seed) {
    return __popc(nonwc) + __popc(mm) + __popc(nonwc & seed) + __popc(mm & seed);
}

// The slow path of one (offset, miRNA, strand, kind): the placement P with the lowest score (the smallest P on a tie), then -c and the domination
// rule.  t1 (and t(L - 1) where its gap costs 2) is never reported, its ungapped alignment that pairs the end position instead always dominates
// it, but it stays in the loop: where it is the best placement the interval is judged by it and dropped, not handed to the next best P.
// (nwA, mmA) / (nwB, mmB): the evaluations of A and B; validA / validB: whether A / B is a site of its own (window inside the contig,
// unambiguous).  -> half-score << 8 | P, or ~0u when the site is not reported.
template <bool T>
__device__ __forceinline__ unsigned tg_bulge_best(const TgStrand& S, unsigned lmask, int L, int s, unsigned nwA, unsigned mmA, unsigned nwB, unsigned mmB,
                                                  bool validA, bool validB) {
    unsigned best = ~0u, bp = 0, bmm = 0;
    for (int P = T ? 1 : 2; P < L; P++) {
        unsigned MA, MB;                     // window positions paired as in A / as in B
        if (T) {
            MA = s ? (1u << P) - 1u : lmask & ~((1u << (L - P)) - 1u);
            MB = lmask & ~MA;
        } else {
            MA = s ? (1u << (P - 1)) - 1u : lmask & ~((2u << (L - P)) - 1u);
            MB = s ? lmask & ~((1u << P) - 1u) : (1u << (L - P)) - 1u;
        }
        const unsigned nw = (nwA & MA) | (nwB & MB), mm = (mmA & MA) | (mmB & MB);
        const unsigned gap = T ? (P >= 2 && P <= 12 ? 4u : 2u) : (P <= 13 ? 4u : 2u);
        const unsigned h = tg_cost(nw, mm, S.seed) + gap;
        if (h < best) { best = h; bp = (unsigned)P; bmm = mm; }
    }
    if (S.cleave && ((bmm & S.cleave) || bp == 10 || (!T && bp == 11))) return ~0u;
    if (validA && (mmA & S.cleave) == 0 && tg_cost(nwA, mmA, S.seed) <= best) return ~0u;
    if (validB && (mmB & S.cleave) == 0 && tg_cost(nwB, mmB, S.seed) <= best) return ~0u;
    return best << 8 | bp;
}

template <int MODE>
__device__ __forceinline__ void tg_bulge_hit(int m, unsigned h, unsigned long long o, int s, unsigned kind, unsigned P, unsigned long long* __restrict__ keys,
                                             unsigned long long cap, unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hist) {
    if (MODE == 0) {
        const unsigned long long i = atomicAdd(counter, 1ull);
        if (i < cap)
            keys[i] = ((unsigned long long)m << TG_BULGE_SHIFT) | ((unsigned long long)h << 40) | (o << 8) | ((unsigned long long)s << 7) | (kind << 5) | P;
    } else {
        atomicAdd(&hist[(long long)m * TG_NHALF + h], 1ull);
    }
}

// tg_scan_kernel's arguments and modes; the keys have the layout above, and a site of any kind counts under its own half-score.
template <int MODE, bool BOTH>
__global__ __launch_bounds__(256) void tg_bulge_scan_kernel(TgRef R, const TgMirna* __restrict__ mi, int m0, int m1, unsigned long long p0, unsigned long long p1,
                                                            unsigned long long* __restrict__ keys, unsigned long long cap,
                                                            unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hist) {
    const unsigned long long o = p0 + (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    unsigned wl[3] = {0, 0, 0}, wh[3] = {0, 0, 0}, stop = 0;   // windows at o - 1, o, o + 1; a lane past p1 has stop 0: nothing fits
    bool prev = false;                                         // o - 1 is an unambiguous base of o's contig
    if (o < p1) {
        const unsigned long long b = o ? o - 1 : 0;            // the 34 bases from o - 1 (o = 0: from 0, moved up one base below)
        const unsigned long long q = b >> 5;
        const unsigned sh = 2 * (unsigned)(b & 31);
        unsigned long long lo = R.pk[q], hi = R.pk[q + 1];
        if (sh) {
            lo = (lo >> sh) | (hi << (64 - sh));
            hi = (hi >> sh) | (R.pk[q + 2] << (64 - sh));
        }
        if (!o) { hi = (hi << 2) | (lo >> 62); lo <<= 2; }
        const unsigned e = (unsigned)hi;
        const unsigned long long pl = tg_even(lo) | ((unsigned long long)((e & 1u) | ((e >> 1) & 2u)) << 32);
        const unsigned long long ph = tg_even(lo >> 1) | ((unsigned long long)(((e >> 1) & 1u) | ((e >> 2) & 2u)) << 32);
        #pragma unroll
        for (int k = 0; k < 3; k++) { wl[k] = (unsigned)(pl >> k); wh[k] = (unsigned)(ph >> k); }
        const unsigned long long qa = o >> 5;
        const unsigned sa = (unsigned)(o & 31);
        unsigned long long am = R.amb[qa] | ((unsigned long long)R.amb[qa + 1] << 32), cs = R.cst[qa] | ((unsigned long long)R.cst[qa + 1] << 32);
        if (sa) {
            am = (am >> sa) | ((unsigned long long)R.amb[qa + 2] << (64 - sa));
            cs = (cs >> sa) | ((unsigned long long)R.cst[qa + 2] << (64 - sa));
        }
        const unsigned long long bad = am | (cs & ~1ull);
        stop = bad ? (unsigned)(__ffsll((long long)bad) - 1) : 64u;
        prev = o && !((R.amb[(o - 1) >> 5] >> ((o - 1) & 31)) & 1u) && !(cs & 1ull);
    }
    for (int m = m0; m < m1; m++) {
        const TgMirna& M = mi[m];
        const unsigned L = (unsigned)M.L;
        if (L - 1 > stop) continue;                            // not even the m site fits
        const unsigned smin = (unsigned)M.smin, smax = (unsigned)M.smax, span = smax - smin;
        const bool fit = L <= stop, fit1 = L + 1 <= stop;      // U(o); the t site, and with it U(o + 1)
        #pragma unroll
        for (int s = 0; s < (BOTH ? 2 : 1); s++) {
            const TgStrand& S = M.s[s];
            unsigned nw[3], mm[3];
            #pragma unroll
            for (int k = 0; k < 3; k++) tg_masks(S, M.lmask, wl[k], wh[k], s, &nw[k], &mm[k]);
            const unsigned h = tg_cost(nw[1], mm[1], S.seed);
            if (fit && h - smin <= span && (mm[1] & S.cleave) == 0) tg_bulge_hit<MODE>(m, h, o, s, 1u, 0u, keys, cap, counter, hist);
            if (fit1 && tg_cost(nw[1] & nw[2], mm[1] & mm[2], S.seed) + 2u <= smax) {
                const int a = s ? 1 : 2, b = s ? 2 : 1;
                const unsigned r = tg_bulge_best<true>(S, M.lmask, (int)L, s, nw[a], mm[a], nw[b], mm[b], true, true);
                if ((r >> 8) - smin <= span) tg_bulge_hit<MODE>(m, r >> 8, o, s, 2u, r & 31u, keys, cap, counter, hist);
            }
            if (tg_cost(nw[0] & nw[1], mm[0] & mm[1], S.seed) <= smax) {
                const int a = s ? 1 : 0, b = s ? 0 : 1;            // U(o - 1) is a site when its first base is (prev): its other L - 1 fit here
                const unsigned r = tg_bulge_best<false>(S, M.lmask, (int)L, s, nw[a], mm[a], nw[b], mm[b], s ? fit : prev, s ? prev : fit);
                if ((r >> 8) - smin <= span) tg_bulge_hit<MODE>(m, r >> 8, o, s, 0u, r & 31u, keys, cap, counter, hist);
            }
        }
    }
}

}  // namespace mirp
