// Device code shared by the target-site search (targets_kernels.hip) and the degradome scan (degradome_kernels.hip, §18): the packed
// targets, the 32-base window planes, the evaluation of one (window, miRNA, strand) and the scan over every offset of the targets.
//
// Targets: pk as 64-bit words of 32 2-bit bases (base i at bits 2 (i % 32)), amb / cst bitmaps as in align_kernels.hip (amb also set on every
// position past the end).  Positions are global over the targets in file order.
//
// miRNAs: one TgMirna per miRNA, built on the host.  Every mask is a 32-bit mask over the window positions j, and the Watson-Crick target bases
// are held as two bit planes (low and high bit of the 2-bit code), so one (position, miRNA, strand) evaluation is
//     nonwc = ((wl ^ pl) | (wh ^ ph) | unk) & lmask            bases that are not Watson-Crick pairs (an unknown miRNA letter never is)
//     gu    = (isX & g1) | (isY & g2)                          G:U pairs: X = T, Y = G on the plus strand, X = A, Y = C on the minus strand
//     mm    = nonwc & ~gu
//     half  = popc(nonwc) + popc(mm) + popc(nonwc & seed) + popc(mm & seed)      the score in half-units: mismatch 2, G:U 1, doubled in the seed
// and the site is a hit when smin <= half <= smax and mm & cleave == 0.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "mirp_ctx.h"

namespace mirp {

#define TG_GROUP (1 << 16)           // miRNAs per group (the key holds 16 bits of miRNA index)
#define TG_NHALF 17                  // half-scores 0 .. 16
#define TG_LAUNCH_POS (1ll << 30)    // offsets per scan launch (the grid's work-items stay below 2^32)

struct TgRef {
    const unsigned long long* pk;
    const unsigned* amb;
    const unsigned* cst;
    unsigned long long total;
};

// Host: sizes tg_pk / tg_amb / tg_cst / tg_cstart for a packed FASTA of `total` bases (pk: (total + 31) / 32 + 2 u64 words; amb / cst: as many u32
// words) and enqueues its upload on the context's stream; the caller synchronises before its host arrays go.
inline int tg_upload_packed(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                            const std::vector<unsigned long long>& cstart, TgRef* R) {
    const size_t n_w = (size_t)((total + 31) / 32 + 2);
    if (c->tg_pk.ensure(8 * n_w) || c->tg_amb.ensure(4 * n_w) || c->tg_cst.ensure(4 * n_w) || c->tg_cstart.ensure(8 * cstart.size()))
        return fail(c, -6, "device allocation failed (packed targets)");
    HIPCHK(c, hipMemcpyAsync(c->tg_pk.p, pk, 8 * n_w, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tg_amb.p, amb, 4 * n_w, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tg_cst.p, cst, 4 * n_w, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->tg_cstart.p, cstart.data(), 8 * cstart.size(), hipMemcpyHostToDevice, c->stream));
    *R = TgRef{(const unsigned long long*)c->tg_pk.p, (const unsigned*)c->tg_amb.p, (const unsigned*)c->tg_cst.p, (unsigned long long)total};
    return 0;
}

__device__ __forceinline__ unsigned tg_base(const unsigned long long* __restrict__ pk, unsigned long long q) { return (unsigned)(pk[q >> 5] >> (2 * (q & 31))) & 3u; }

// the even bits of x, packed into 32 bits
__device__ __forceinline__ unsigned tg_even(unsigned long long x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return (unsigned)x;
}

__device__ __forceinline__ unsigned tg_bits32(const unsigned* __restrict__ bm, unsigned long long p) {
    const unsigned long long w = bm[p >> 5] | ((unsigned long long)bm[(p >> 5) + 1] << 32);
    return (unsigned)(w >> (p & 31));
}

// one strand of one miRNA: a hit when (half - smin) <= span (unsigned) and no mismatch under the cleavage mask
__device__ __forceinline__ bool tg_eval(const TgStrand& S, unsigned lmask, unsigned wl, unsigned wh, unsigned x1, unsigned x2, unsigned smin, unsigned span,
                                        unsigned* half) {
    const unsigned nonwc = ((wl ^ S.pl) | (wh ^ S.ph) | S.unk) & lmask;
    const unsigned gu = (x1 & S.g1) | (x2 & S.g2);
    const unsigned mm = nonwc & ~gu;
    const unsigned h = __popc(nonwc) + __popc(mm) + __popc(nonwc & S.seed) + __popc(mm & S.seed);
    *half = h;
    return h - smin <= span && (mm & S.cleave) == 0;
}

// Window position j of a lane at offset o is the forward base t[o + j]; miRNA position i pairs with j = L - i on the plus strand and j = i - 1 on
// the minus strand; the site also needs L <= stop, stop = the distance to the first ambiguous base or to the next contig start (per lane, once).
// MODE 0: keys mloc << 38 | half << 33 | o << 1 | strand (keys[0 .. cap), counter[0] = hits, also past cap); MODE 1: hist[mloc * 17 + half] += hits.
// miRNAs [m0, m1) of the group's array, offsets [p0, p1).
template <int MODE, bool BOTH>
__global__ __launch_bounds__(256) void tg_scan_kernel(TgRef R, const TgMirna* __restrict__ mi, int m0, int m1, unsigned long long p0, unsigned long long p1,
                                                      unsigned long long* __restrict__ keys, unsigned long long cap, unsigned long long* __restrict__ counter,
                                                      unsigned long long* __restrict__ hist) {
    const unsigned long long o = p0 + (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    unsigned wl = 0, wh = 0, stop = 0;                         // a lane past p1 has stop 0: no miRNA (L >= 12) fits
    if (o < p1) {
        const unsigned long long q = o >> 5;
        const unsigned sh = 2 * (unsigned)(o & 31);
        unsigned long long w = R.pk[q];
        if (sh) w = (w >> sh) | (R.pk[q + 1] << (64 - sh));
        wl = tg_even(w);
        wh = tg_even(w >> 1);
        const unsigned sm = tg_bits32(R.amb, o) | (tg_bits32(R.cst, o) & ~1u);
        stop = sm ? (unsigned)(__ffs(sm) - 1) : 32u;
    }
    const unsigned tA = ~(wl | wh), tC = wl & ~wh, tG = ~wl & wh, tT = wl & wh;
    for (int m = m0; m < m1; m++) {
        const TgMirna& M = mi[m];
        if ((unsigned)M.L > stop) continue;
        const unsigned span = (unsigned)(M.smax - M.smin);
        unsigned h;
        #pragma unroll
        for (int s = 0; s < (BOTH ? 2 : 1); s++) {
            if (tg_eval(M.s[s], M.lmask, wl, wh, s ? tA : tT, s ? tC : tG, (unsigned)M.smin, span, &h)) {
                if (MODE == 0) {
                    const unsigned long long i = atomicAdd(counter, 1ull);
                    if (i < cap) keys[i] = ((unsigned long long)m << 38) | ((unsigned long long)h << 33) | (o << 1) | (unsigned long long)s;
                } else {
                    atomicAdd(&hist[(long long)m * TG_NHALF + h], 1ull);
                }
            }
        }
    }
}

}  // namespace mirp
