// Device functions on the sorted site keys of the (miRNA, bin) searches (targets_kernels.hip, mimic_kernels.hip) and of the kernels that read the
// same keys (duplex_kernels.hip, unpaired_kernels.hip; degradome_kernels.hip takes the contig lookup): the -k cut, the decoder of the target
// search's two key layouts, the contig of a packed position and the class of a pair.  The layouts are documented at TG_BULGE_SHIFT
// (targets_bulge_device.h), tg_scan_kernel (targets_device.h) and MM_SHIFT (mimic_device.h); `shift` is the number of key bits below the miRNA index.
#pragma once
#include "targets_bulge_device.h"

namespace mirp {

// first index of the miRNA run that holds keys[i] (the keys are sorted)
__device__ __forceinline__ long long site_run_first(const unsigned long long* __restrict__ keys, long long i, int shift) {
    const unsigned long long lo = keys[i] >> shift << shift;
    long long a = 0, z = i;
    while (a < z) { const long long md = (a + z) >> 1; if (keys[md] < lo) a = md + 1; else z = md; }
    return a;
}

// -k keeps sorted key i: its rank inside its miRNA's run plus what earlier passes emitted for that miRNA (emitted[key >> shift]) is below k; k = 0 keeps all
__device__ __forceinline__ bool site_kept(const unsigned long long* __restrict__ keys, long long i, long long k, const unsigned long long* __restrict__ emitted,
                                          int shift) {
    return k == 0 || emitted[keys[i] >> shift] + (unsigned long long)(i - site_run_first(keys, i, shift)) < (unsigned long long)k;
}

// a key of the target search: the ungapped scan's (kind 1, P 0) or the --bulge scan's
template <bool BULGE>
struct SiteKey {
    static constexpr int shift = BULGE ? TG_BULGE_SHIFT : 38;
    int mloc;                               // the miRNA's index in its group
    unsigned half;                          // the score in half-units
    unsigned long long g;                   // packed position of the interval's first base
    int strand, kind, P;                    // kind 0 = m, 1 = ungapped, 2 = t; P: the bulge's position
    __device__ __forceinline__ explicit SiteKey(unsigned long long key)
        : mloc((int)(key >> shift)),
          half((unsigned)(key >> (BULGE ? 40 : 33)) & 31u),
          g((key >> (BULGE ? 8 : 1)) & 0xffffffffull),
          strand((int)(key >> (BULGE ? 7 : 0)) & 1),
          kind(BULGE ? (int)(key >> 5) & 3 : 1),
          P(BULGE ? (int)(key & 31) : 0) {}
    // bases of the interval of a miRNA of L nt
    __device__ __forceinline__ int len(int L) const { return L + kind - 1; }
};

// the contig of packed position g: the last index with cstart[index] <= g (cstart[0] = 0)
__device__ __forceinline__ int site_contig(const unsigned long long* __restrict__ cstart, int n_contigs, unsigned long long g) {
    int a = 0, z = n_contigs;
    while (z - a > 1) { const int md = (a + z) >> 1; if (cstart[md] <= g) a = md; else z = md; }
    return a;
}

// pair class of miRNA code mc (0..3 A C G U, 4 unknown) with target-strand base y (0..3 A C G U): 0 Watson-Crick, 1 G:U, 2 mismatch
__device__ __forceinline__ int site_class(unsigned mc, unsigned y) {
    if (mc > 3) return 2;
    if (mc + y == 3) return 0;
    return (mc == 2 && y == 3) || (mc == 3 && y == 2) ? 1 : 2;
}

}  // namespace mirp
