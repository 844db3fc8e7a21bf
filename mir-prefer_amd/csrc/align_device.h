// Device code of the resident alignment index shared by align_kernels.hip and homolog_kernels.hip: the packed reference and its
// bitmaps, the 16-base keys, the seed lookup in the truncated suffix array, the seeds of a read and the verification of one candidate.
#pragma once
#include <hip/hip_runtime.h>

namespace mirp {

#define AL_BKT_BASES 12
#define AL_NBKT (1u << (2 * AL_BKT_BASES))

struct AlRef {
    const unsigned* pk;
    const unsigned* amb;
    const unsigned* cst;
    const unsigned* sa;
    const long long* bkt;
    unsigned long long total;
};

__device__ __forceinline__ unsigned al_base(const unsigned* __restrict__ pk, unsigned long long q) { return (pk[q >> 4] >> (2 * (q & 15))) & 3u; }

// 16-bit window of a bitmap starting at bit p
__device__ __forceinline__ unsigned al_bits16(const unsigned* __restrict__ bm, unsigned long long p) {
    const unsigned long long w = bm[p >> 5] | ((unsigned long long)bm[(p >> 5) + 1] << 32);
    return (unsigned)(w >> (p & 31)) & 0xffffu;
}

// key of position p: its first 16 bases, first base in the top two bits; bases from the first ambiguous position or the next contig start on are 0
__device__ __forceinline__ unsigned al_key16(const AlRef& R, unsigned long long p) {
    const unsigned long long x = R.pk[p >> 4] | ((unsigned long long)R.pk[(p >> 4) + 1] << 32);
    unsigned r = __brev((unsigned)(x >> (2 * (p & 15))));
    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
    const unsigned stop = al_bits16(R.amb, p) | (al_bits16(R.cst, p) & ~1u) | 0x10000u;
    const int run = __ffs(stop) - 1;
    return run >= 16 ? r : run == 0 ? 0u : r & ~(0xffffffffu >> (2 * run));
}

// any bit set in [a, b)
__device__ __forceinline__ bool al_any(const unsigned* __restrict__ bm, unsigned long long a, unsigned long long b) {
    while (a < b) {
        const int lo = (int)(a & 31);
        const int n = b - a < (unsigned long long)(32 - lo) ? (int)(b - a) : 32 - lo;
        const unsigned m = (n == 32 ? 0xffffffffu : ((1u << n) - 1u)) << lo;
        if (bm[a >> 5] & m) return true;
        a += n;
    }
    return false;
}

// SA range of the positions whose key starts with the m <= 16 bases P (first base in the top bits of the low 2m bits)
__device__ void al_range(const AlRef& R, unsigned P, int m, long long* lo_out, long long* hi_out) {
    if (m <= AL_BKT_BASES) {
        const int sh = 2 * (AL_BKT_BASES - m);
        *lo_out = R.bkt[(unsigned long long)P << sh];
        *hi_out = R.bkt[((unsigned long long)P + 1) << sh];
        return;
    }
    const unsigned b = P >> (2 * (m - AL_BKT_BASES));
    const unsigned long long k0 = (unsigned long long)P << (2 * (16 - m)), k1 = ((unsigned long long)P + 1) << (2 * (16 - m));
    long long lo = R.bkt[b], hi = R.bkt[b + 1];
    long long a = lo, z = hi;                    // first key >= k0
    while (a < z) { const long long md = (a + z) >> 1; if ((unsigned long long)al_key16(R, R.sa[md]) < k0) a = md + 1; else z = md; }
    lo = a;
    z = hi;                                      // first key >= k1
    while (a < z) { const long long md = (a + z) >> 1; if ((unsigned long long)al_key16(R, R.sa[md]) < k1) a = md + 1; else z = md; }
    *lo_out = lo;
    *hi_out = a;
}

// a read's base i on a strand: codes 0..3 = ACGT, 4 = anything else (mismatches every base)
__device__ __forceinline__ unsigned al_oriented(const unsigned char* __restrict__ rd, int L, int strand, int i) {
    if (!strand) return rd[i];
    const unsigned c = rd[L - 1 - i];
    return c < 4 ? 3u - c : 4u;
}

struct AlSeed { long long lo; unsigned read; unsigned char strand, half, vbase, pad; int vpos; };   // vpos -1: the exact half

struct AlParams { int v, e, k, m, filter, place, tail_trim; };   // place: 0 off, 1 by density, 2 uniform (align --place; -k is then not consulted)
                                                                 // tail_trim: the record of a tailed read holds its templated part only (align --tail-trim)

__device__ __forceinline__ void al_half(int L, int v, int half, int* hoff, int* hlen) {
    if (v == 0) { *hoff = 0; *hlen = L; return; }
    const int a = (L + 1) / 2;
    *hoff = half ? a : 0;
    *hlen = half ? L - a : a;
}

// seeds of one (strand, half): 1 exact (no non-ACGT base); with e = 1 also 3 per position (none non-ACGT) or the 4 at the one non-ACGT position
__device__ __forceinline__ int al_nseeds(const unsigned char* __restrict__ rd, int L, int strand, int hoff, int hlen, int e, int* bad_pos) {
    int nbad = 0, bp = -1;
    for (int i = 0; i < hlen; i++)
        if (al_oriented(rd, L, strand, hoff + i) > 3u) { nbad++; bp = i; }
    *bad_pos = bp;
    if (e == 0) return nbad == 0 ? 1 : 0;
    return nbad == 0 ? 1 + 3 * hlen : nbad == 1 ? 4 : 0;
}

// mismatches of the hit found by candidate pos of seed sd, or -1 if it is not a hit that this seed reports
__device__ int al_check(const AlRef& R, const unsigned char* __restrict__ rd, int L, const AlSeed& sd, unsigned long long pos, const AlParams& P) {
    int hoff, hlen;
    al_half(L, P.v, sd.half, &hoff, &hlen);
    if (pos < (unsigned long long)hoff) return -1;
    const unsigned long long o = pos - hoff;
    if (o + L > R.total) return -1;
    if (al_any(R.amb, o, o + L) || al_any(R.cst, o + 1, o + L)) return -1;
    for (int i = 0; i < hlen; i++) {
        const unsigned b = i == sd.vpos ? (unsigned)sd.vbase : al_oriented(rd, L, sd.strand, hoff + i);
        if (b != al_base(R.pk, o + hoff + i)) return -1;
    }
    const int a = (L + 1) / 2;
    int mm = 0, mm_a = 0;
    for (int i = 0; i < L; i++) {
        const int d = al_oriented(rd, L, sd.strand, i) != al_base(R.pk, o + i);
        mm += d;
        if (i < a) mm_a += d;
        if (mm > P.v) return -1;
    }
    if (P.v && sd.half == 1 && mm_a <= P.e) return -1;    // half A finds it
    return mm;
}

}  // namespace mirp
