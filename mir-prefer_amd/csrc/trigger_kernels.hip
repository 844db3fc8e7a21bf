// Device side of the miRNA triggers of PHAS loci (mirp_trigger_scan, mirp_triggers.cpp): the target sites of §14 inside the locus
// intervals, and the phasing test of §15 in the windows that each site's cut anchors.
//
//   sites    tr_scan_kernel: one lane per offset of the concatenated locus intervals (the locus by a binary search in the prefix of the interval
//            lengths).  The lane builds the 32-base window planes as tg_scan_kernel does (targets_device.h); its stop distance is the distance to
//            the first ambiguous base, to the next contig start or to the interval's end, whichever is nearest.  The miRNAs of a group of <= 2^16
//            come in wave-uniform loads and are evaluated with tg_eval on both strands, the cleavage mask set.  <0> counts the hits (one atomic per
//            wave), the keys are allocated exactly, <1> fills them: a ballot per (miRNA, strand), one atomic per wave with a hit, every hit lane
//            stores at its rank.  Key = locus | miRNA | half-score | offset in the interval | strand, the field widths sized to the call, so the
//            radix sort of the whole key (sort_kernels.hip) gives the output order: locus, miRNA, score, start, + before -.
//   counts   tr_locus_sites_kernel: the sites of every locus, two binary searches in the sorted keys.
//   units    ph_build_units (phasing_units.h): the arrays mirp_phase_scan works on.
//   windows  tr_window_kernel, one lane per (site, side, offset), in output order.  The register x of the window comes from the cut (§29); it is
//            no unit, so each strand takes one full binary search for the window's first key, clamped to the contig's key range (x can be <= 0, and
//            tid << 32 | c must not wrap), then the bounded counting of phasing_units.h: O(m log L) also in a saturated region; phased coordinates
//            below 0 are skipped.  <0> writes the pass flags k >= max(kmin[n], K); launch_excl_scan; <1> recomputes the passing windows with their
//            abundance sums (30-bit-split prefixes) and writes the MirpTrigger rows at their ranks.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "phasing_units.h"
#include "targets_device.h"
#include "trigger_device.h"

namespace mirp {

#define TR_NT 256

static inline unsigned tr_grid(long long n) { return (unsigned)std::max(1ll, std::min((n + TR_NT - 1) / TR_NT, 1ll << 20)); }

// the key's fields from bit 0: strand (1), offset in the interval (tb), half-score (5), miRNA (mb), locus (the rest)
struct TrKey {
    int tb, mb;
    __host__ __device__ int half_shift() const { return 1 + tb; }
    __host__ __device__ int mirna_shift() const { return 6 + tb; }
    __host__ __device__ int locus_shift() const { return 6 + tb + mb; }
};

struct TrLoci {
    const long long* ipre;              // prefix of the interval lengths (n + 1)
    const unsigned long long* g0;       // packed position of every interval's first base
    const int* tid;                     // tid of the resident alignments
    const long long* o0;                // 0-based contig offset of the interval's first base
    long long n;
};

// lanes [p0, p1) of the concatenated intervals, miRNAs [m0, m1) of the group's array, which starts at miRNA `mbase` of the file
template <int FILL>
__global__ __launch_bounds__(TR_NT) void tr_scan_kernel(TgRef R, const TgMirna* __restrict__ mi, int m0, int m1, int mbase, unsigned smax, TrLoci Q,
                                                        long long p0, long long p1, TrKey K, unsigned long long* __restrict__ keys,
                                                        unsigned long long cap, unsigned long long* __restrict__ counter) {
    const long long i = p0 + (long long)blockIdx.x * TR_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned wl = 0, wh = 0, stop = 0;                         // a lane past p1 has stop 0: no miRNA (L >= 12) fits
    unsigned long long kbase = 0;
    if (i < p1) {
        long long lo = 0, hi = Q.n;                            // the locus: the last q with ipre[q] <= i
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (Q.ipre[mid] <= i) lo = mid;
            else hi = mid;
        }
        const long long t = i - Q.ipre[lo], left = Q.ipre[lo + 1] - i;
        const unsigned long long o = Q.g0[lo] + (unsigned long long)t;
        const unsigned long long q = o >> 5;
        const unsigned sh = 2 * (unsigned)(o & 31);
        unsigned long long w = R.pk[q];
        if (sh) w = (w >> sh) | (R.pk[q + 1] << (64 - sh));
        wl = tg_even(w);
        wh = tg_even(w >> 1);
        const unsigned sm = tg_bits32(R.amb, o) | (tg_bits32(R.cst, o) & ~1u);
        stop = sm ? (unsigned)(__ffs(sm) - 1) : 32u;
        if ((long long)stop > left) stop = (unsigned)left;
        kbase = ((unsigned long long)lo << K.locus_shift()) | ((unsigned long long)t << 1);
    }
    const unsigned tA = ~(wl | wh), tC = wl & ~wh, tG = ~wl & wh, tT = wl & wh;
    unsigned long long found = 0;                              // wave-uniform
    for (int m = m0; m < m1; m++) {
        const TgMirna& M = mi[m];
        const bool fits = (unsigned)M.L <= stop;
        #pragma unroll
        for (int s = 0; s < 2; s++) {
            unsigned h;
            const bool hit = tg_eval(M.s[s], M.lmask, wl, wh, s ? tA : tT, s ? tC : tG, 0u, smax, &h) && fits;
            const unsigned long long b = __ballot(hit);
            if (!b) continue;
            if (!FILL) {
                found += (unsigned long long)__popcll(b);
            } else {
                const int leader = __ffsll((long long)b) - 1;
                unsigned long long at = 0;
                if (lane == leader) at = atomicAdd(counter, (unsigned long long)__popcll(b));
                at = __shfl(at, leader) + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
                if (hit && at < cap)
                    keys[at] = kbase | ((unsigned long long)(mbase + m) << K.mirna_shift()) | ((unsigned long long)h << K.half_shift()) | (unsigned long long)s;
            }
        }
    }
    if (!FILL && lane == 0 && found) atomicAdd(counter, found);
}

// sites[q] = the keys of locus q in the sorted keys
__global__ void __launch_bounds__(TR_NT) tr_locus_sites_kernel(const unsigned long long* __restrict__ keys, long long n, long long n_loci, int shift,
                                                               long long* __restrict__ sites) {
    for (long long q = (long long)blockIdx.x * TR_NT + threadIdx.x; q < n_loci; q += (long long)gridDim.x * TR_NT) {
        const long long a = ph_lower(keys, 0, n, (unsigned long long)q << shift);
        const long long b = q + 1 == n_loci ? n : ph_lower(keys, a, n, (unsigned long long)(q + 1) << shift);
        sites[q] = b - a;
    }
}

// one strand [s0, e) of the units in the window of register x (signed) on contig tid
template <int EMIT>
__device__ __forceinline__ void tr_strand(const PhUnits& U, long long s0, long long e, int tid, long long x, int L, int m, int& n, int& k,
                                          long long& phased, long long& reads) {
    const long long xe = x + (long long)m * L;
    const long long c0 = x > 0 ? x : 0, c1 = xe < (1ll << 32) ? xe : (1ll << 32);      // the contig's keys are tid << 32 | 0 .. 2^32 - 1
    if (c0 >= c1) return;
    const unsigned long long tb = (unsigned long long)(unsigned)tid << 32;
    const long long b = ph_lower(U.key, s0, e, tb + (unsigned long long)c0);
    const long long cap = b + (long long)m * L;
    const long long hi = ph_lower(U.key, b, cap < e ? cap : e, tb + (unsigned long long)c1);
    n += (int)(hi - b);
    if (EMIT) reads += ph_prefix(U, hi) - ph_prefix(U, b);
    const int j0 = x < 0 ? (int)((-x + L - 1) / L) : 0;         // the first phased coordinate that is not below 0
    ph_count_phased<EMIT>(U, b, hi, tb + (unsigned long long)(x + (long long)j0 * L), L, m - j0, x >= 0, k, phased);
}

template <int EMIT>
__global__ void __launch_bounds__(TR_NT) tr_window_kernel(const unsigned long long* __restrict__ keys, long long n_sites, TrKey K, TrLoci Q,
                                                          const unsigned char* __restrict__ mlen, PhUnits U, int L, int m, int drift, int min_phased,
                                                          const int* __restrict__ kmin, int* __restrict__ pass, const long long* __restrict__ pscan,
                                                          MirpTrigger* __restrict__ out) {
    const int nd = 2 * drift + 1, per = 2 * nd;
    const long long n = n_sites * per;
    for (long long w = (long long)blockIdx.x * TR_NT + threadIdx.x; w < n; w += (long long)gridDim.x * TR_NT) {
        if (EMIT && !pass[w]) continue;
        const unsigned long long key = keys[w / per];
        const int r = (int)(w % per), side = r / nd, delta = r % nd - drift;
        const int strand = (int)(key & 1ull);
        const long long t = (long long)((key >> 1) & ((1ull << K.tb) - 1ull));
        const int half = (int)((key >> K.half_shift()) & 31ull);
        const long long mir = (long long)((key >> K.mirna_shift()) & ((1ull << K.mb) - 1ull));
        const long long q = (long long)(key >> K.locus_shift());
        const int ML = mlen[mir];
        const long long o = Q.o0[q] + t;
        // the register of the cut and of the window (§29): plus cut = o + ML - 9, r = cut; minus cut = o + 10, r = cut - L + 3
        long long x;
        if (!strand) x = o + ML - 9 + (side ? -(long long)m * L : 0) + delta;
        else x = o + 13 - L + (side ? L : -(long long)(m - 1) * L) + delta;
        const int tid = Q.tid[q];
        int nn = 0, kk = 0;
        long long phased = 0, reads = 0;
        tr_strand<EMIT>(U, 0, U.np, tid, x, L, m, nn, kk, phased, reads);
        tr_strand<EMIT>(U, U.np, U.n, tid, x, L, m, nn, kk, phased, reads);
        if (!EMIT) {
            pass[w] = kk >= max(kmin[nn], min_phased);
        } else {
            MirpTrigger g;
            g.locus = (int)q;
            g.mirna = (int)mir;
            g.half = half;
            g.strand = strand;
            g.side = side;
            g.offset = delta;
            g.n = nn;
            g.k = kk;
            g.pos = o;
            g.phased_reads = phased;
            g.window_reads = reads;
            out[pscan[w]] = g;
        }
    }
}

}  // namespace mirp

namespace {

int tr_bits(unsigned long long v) {          // bits that hold 0 .. v
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

}  // namespace

int mirp_device_trigger_scan(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                             const std::vector<unsigned long long>& cstart, const std::vector<TgMirna>& mi, const std::vector<unsigned char>& mlen,
                             const MirpTriggerLocus* loci, long long n_loci, const MirpTriggerOpts& o, const int32_t* kmin, MirpTrigger** triggers,
                             int64_t* n_triggers, int64_t* site_counts, long long stats[6], double seconds[4]) {
    using namespace mirp;
    const hipStream_t st = c->stream;
    const long long n_mi = (long long)mi.size();
    const int L = o.length, m = o.cycles, S = 2 * m * L, per = 2 * (2 * o.drift + 1);
    double t0 = mirp::now();
    // the intervals
    std::vector<long long> ipre((size_t)n_loci + 1, 0), o0((size_t)std::max(n_loci, 1ll));
    std::vector<unsigned long long> g0((size_t)std::max(n_loci, 1ll));
    std::vector<int> tids((size_t)std::max(n_loci, 1ll));
    long long longest = 0;
    for (long long q = 0; q < n_loci; q++) {
        const long long len = loci[q].end - loci[q].start + 1;
        ipre[(size_t)q + 1] = ipre[(size_t)q] + len;
        longest = std::max(longest, len);
        o0[(size_t)q] = loci[q].start - 1;
        g0[(size_t)q] = cstart[(size_t)loci[q].contig] + (unsigned long long)(loci[q].start - 1);
        tids[(size_t)q] = loci[q].tid;
    }
    const long long lanes = ipre[(size_t)n_loci];
    TrKey K;
    K.tb = tr_bits((unsigned long long)std::max(longest - 1, 0ll));
    K.mb = tr_bits((unsigned long long)std::max(n_mi - 1, 0ll));
    const int key_bits = K.locus_shift() + tr_bits((unsigned long long)std::max(n_loci - 1, 0ll));
    if (key_bits > 64) return fail(c, -5, "triggers: the loci, their longest interval and the miRNAs do not fit one 64-bit key");
    for (long long q = 0; q < n_loci; q++) site_counts[q] = 0;
    *triggers = nullptr;
    *n_triggers = 0;
    long long n_sites = 0, n_trig = 0, records = 0;
    TmpDevice T;
    PhUnits U = {nullptr, nullptr, nullptr, 0, 0};
    MirpTrigger* d_out = nullptr;
    if (lanes > 0 && n_mi > 0) {
        TgRef R;
        if (c->tg_mi.ensure(sizeof(TgMirna) * TG_GROUP) || c->tg_small.ensure(64)) return fail(c, -6, "device allocation failed (triggers)");
        if (int rc = tg_upload_packed(c, pk, amb, cst, total, cstart, &R)) return rc;
        long long* d_ipre = (long long*)T.get(8 * (size_t)(n_loci + 1));
        long long* d_o0 = (long long*)T.get(8 * (size_t)n_loci);
        unsigned long long* d_g0 = (unsigned long long*)T.get(8 * (size_t)n_loci);
        int* d_tid = (int*)T.get(4 * (size_t)n_loci);
        unsigned char* d_mlen = (unsigned char*)T.get((size_t)n_mi);
        long long* d_sites = (long long*)T.get(8 * (size_t)n_loci);
        if (!d_ipre || !d_o0 || !d_g0 || !d_tid || !d_mlen || !d_sites) return fail(c, -6, "device allocation failed (triggers)");
        HIPCHK(c, hipMemcpyAsync(d_ipre, ipre.data(), 8 * (size_t)(n_loci + 1), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_o0, o0.data(), 8 * (size_t)n_loci, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_g0, g0.data(), 8 * (size_t)n_loci, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_tid, tids.data(), 4 * (size_t)n_loci, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mlen, mlen.data(), (size_t)n_mi, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        seconds[0] = mirp::now() - t0;
        t0 = mirp::now();
        const TrLoci Q = {d_ipre, d_g0, d_tid, d_o0, n_loci};
        unsigned long long* d_counter = (unsigned long long*)c->tg_small.p;
        unsigned long long* d_keys = nullptr;
        // the count pass, the exact allocation, the fill pass
        for (int fill = 0; fill < 2; fill++) {
            HIPCHK(c, hipMemsetAsync(d_counter, 0, 8, st));
            for (long long m0 = 0; m0 < n_mi; m0 += TG_GROUP) {
                const int gn = (int)std::min<long long>(TG_GROUP, n_mi - m0);
                HIPCHK(c, hipMemcpyAsync(c->tg_mi.p, mi.data() + m0, sizeof(TgMirna) * (size_t)gn, hipMemcpyHostToDevice, st));
                for (long long p0 = 0; p0 < lanes; p0 += TG_LAUNCH_POS) {
                    const long long p1 = std::min(lanes, p0 + TG_LAUNCH_POS);
                    const dim3 grid((unsigned)((p1 - p0 + TR_NT - 1) / TR_NT));
                    if (fill)
                        hipLaunchKernelGGL(tr_scan_kernel<1>, grid, dim3(TR_NT), 0, st, R, (const TgMirna*)c->tg_mi.p, 0, gn, (int)m0,
                                           (unsigned)o.max_half_score, Q, p0, p1, K, d_keys, (unsigned long long)n_sites, d_counter);
                    else
                        hipLaunchKernelGGL(tr_scan_kernel<0>, grid, dim3(TR_NT), 0, st, R, (const TgMirna*)c->tg_mi.p, 0, gn, (int)m0,
                                           (unsigned)o.max_half_score, Q, p0, p1, K, d_keys, 0ull, d_counter);
                }
                HIPCHK(c, hipStreamSynchronize(st));           // the next group overwrites tg_mi
            }
            HIPCHK(c, hipGetLastError());
            unsigned long long got = 0;
            HIPCHK(c, hipMemcpy(&got, d_counter, 8, hipMemcpyDeviceToHost));
            if (fill) {
                if ((long long)got != n_sites) return fail(c, -5, "triggers: the fill pass found other sites than the count pass");
                break;
            }
            n_sites = (long long)got;
            if (n_sites == 0) break;
            if (n_sites > (1ll << 31) / per) return fail(c, -6, "triggers: " + std::to_string(n_sites) + " sites are too many for one call; lower -s or scan fewer loci");
            d_keys = (unsigned long long*)T.get(8 * (size_t)n_sites);
            if (!d_keys) return fail(c, -6, "triggers: " + std::to_string(n_sites) + " sites do not fit the device's memory; lower -s or scan fewer loci");
        }
        if (n_sites > 0) {
            unsigned long long* d_ktmp = (unsigned long long*)T.get(8 * (size_t)n_sites);
            if (!d_ktmp) return fail(c, -6, "triggers: " + std::to_string(n_sites) + " sites do not fit the device's memory; lower -s or scan fewer loci");
            if (int rc = mirp_device_sort_u64(c, d_keys, d_ktmp, n_sites, 0, key_bits)) return rc;
            hipLaunchKernelGGL(tr_locus_sites_kernel, dim3(tr_grid(n_loci)), dim3(TR_NT), 0, st, (const unsigned long long*)d_keys, n_sites, n_loci,
                               K.locus_shift(), d_sites);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(site_counts, d_sites, 8 * (size_t)n_loci, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        seconds[1] = mirp::now() - t0;
        t0 = mirp::now();
        if (n_sites > 0)
            if (int rc = ph_build_units(c, L, o.min_depth, T, &U, &records)) return rc;
        HIPCHK(c, hipStreamSynchronize(st));
        seconds[2] = mirp::now() - t0;
        t0 = mirp::now();
        if (n_sites > 0 && U.n > 0) {
            const long long nw = n_sites * per;
            int* pass = (int*)T.get(4 * (size_t)nw);
            long long* pscan = (long long*)T.get(8 * (size_t)(nw + 1));
            int* d_kmin = (int*)T.get(4 * (size_t)(S + 1));
            if (!pass || !pscan || !d_kmin)
                return fail(c, -6, "triggers: the windows of " + std::to_string(n_sites) + " sites do not fit the device's memory; lower -s or scan fewer loci");
            HIPCHK(c, hipMemcpyAsync(d_kmin, kmin, 4 * (size_t)(S + 1), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(tr_window_kernel<0>, dim3(tr_grid(nw)), dim3(TR_NT), 0, st, (const unsigned long long*)d_keys, n_sites, K, Q,
                               (const unsigned char*)d_mlen, U, L, m, (int)o.drift, (int)o.min_phased, (const int*)d_kmin, pass,
                               (const long long*)nullptr, (MirpTrigger*)nullptr);
            launch_excl_scan(st, pass, pscan, nw);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(&n_trig, pscan + nw, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (n_trig > 0) {
                d_out = (MirpTrigger*)T.get(sizeof(MirpTrigger) * (size_t)n_trig);
                if (!d_out) return fail(c, -6, "device allocation failed (triggers)");
                hipLaunchKernelGGL(tr_window_kernel<1>, dim3(tr_grid(nw)), dim3(TR_NT), 0, st, (const unsigned long long*)d_keys, n_sites, K, Q,
                                   (const unsigned char*)d_mlen, U, L, m, (int)o.drift, (int)o.min_phased, (const int*)d_kmin, pass,
                                   (const long long*)pscan, d_out);
                HIPCHK(c, hipGetLastError());
            }
        }
    }
    MirpTrigger* h_out = (MirpTrigger*)std::malloc(sizeof(MirpTrigger) * (size_t)std::max(n_trig, 1ll));
    if (!h_out) return fail(c, -6, "host allocation failed (triggers)");
    if (n_trig > 0) {
        const hipError_t e1 = hipMemcpyAsync(h_out, d_out, sizeof(MirpTrigger) * (size_t)n_trig, hipMemcpyDeviceToHost, st);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(st) : e1;
        if (e2 != hipSuccess) {
            std::free(h_out);
            return fail(c, -2, std::string("mirp_trigger_scan: ") + hipGetErrorString(e2));
        }
    }
    seconds[3] = mirp::now() - t0;
    *triggers = h_out;
    *n_triggers = n_trig;
    stats[0] = n_mi;
    stats[1] = lanes;
    stats[2] = n_sites;
    stats[3] = n_sites * per;
    stats[4] = records;
    stats[5] = U.n;
    return 0;
}
