// Device side of the degradome (PARE) cleavage scan on the context's resident alignments (mirp_degradome_scan, mirp_degradome.cpp).
//
//   units      The records are sorted by (tid, pos), so the sense records (plus strand, 1 <= pos <= LN) in order are sorted by unit (tid, pos):
//              dg_flag_kernel + scan + dg_gather_kernel compact their keys tid << 32 | pos and depths, dg_head_kernel + scan number the units,
//              dg_unit_kernel writes each unit's key and sums its depths (64-bit, one atomic per unit and wave: cl_wave_atomic).
//   categories Per transcript (SAM tid) amax, npos, tot (dg_tstat_kernel) and nmax (dg_nmax_kernel) by the same wave-reduced integer atomics: no
//              lane loops over a transcript and the sums do not depend on scheduling.  dg_cat_kernel: one lane per unit, its category, the
//              histogram C_0..C_4 (one atomic per category and wave) and the keep flag (category <= --max-category).
//   windows    dg_window_kernel: one lane per kept unit builds, once, the two bit planes of the 32 bases that end at the base paired with miRNA
//              position 1 (transcript position p + 9), and avail = how many of them, counted back from that base, lie in the transcript before
//              the first ambiguous base: 16 bytes per kept unit {wl, wh, avail | category << 8, packed position of p}.
//   site counts tg_scan_kernel<1, false> (targets_device.h) over the whole packed transcriptome: N_m(h).
//   anchored   dg_scan_kernel: one lane per kept unit, the miRNAs in wave-uniform (scalar) loads, masks anchored at window position 32 - i
//              (make_mirna(..., anchored)), so one evaluation is tg_eval and nothing else; a miRNA of length L needs L <= avail.
//              MODE 1 counts hits per (miRNA, category, half-score); the host turns the counts into p-values and keeps the bins with p <= alpha.
//              MODE 0 appends the key mloc << 40 | category << 37 | half << 32 | packed position for hits in the kept bins of the pass;
//              the passes are those of plan_passes (pass_plan.h) over the kept bins, with packed positions inside a bin.
//   order      mirp_device_sort_u64 by the whole key = the output order; dg_hit_kernel looks each key's unit up again (two binary searches) and
//              adds its reads and its transcript's amax; the 24-byte hit records go to the host, which writes the lines.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"
#include "site_keys.h"
#include "wave_atomic.h"

namespace mirp {

#define DG_NT 256

struct DgWin { unsigned wl, wh, meta, gpos; };     // meta = avail | category << 8

static inline unsigned dg_grid(long long n) { return (unsigned)std::max(1ll, std::min((n + DG_NT - 1) / DG_NT, 1ll << 20)); }

// flag[i] = record i is a sense record; counts[0] += sense records, counts[1] += minus-strand records
__global__ void __launch_bounds__(DG_NT) dg_flag_kernel(const MirpAln* __restrict__ a, long long n, const long long* __restrict__ sqlen, int n_sq,
                                                        int* __restrict__ flag, unsigned long long* __restrict__ counts) {
    for (long long base = (long long)blockIdx.x * DG_NT; base < n; base += (long long)gridDim.x * DG_NT) {
        const long long i = base + threadIdx.x;
        bool sense = false, minus = false;
        if (i < n) {
            const MirpAln r = a[i];
            minus = r.strand != 0;
            sense = !minus && r.tid >= 0 && r.tid < n_sq && r.pos >= 1 && (long long)r.pos <= sqlen[r.tid];
            flag[i] = sense;
        }
        const unsigned long long bs = __ballot(sense), bm = __ballot(minus);
        if ((threadIdx.x & 63) == 0) {
            if (bs) atomicAdd(&counts[0], (unsigned long long)__popcll(bs));
            if (bm) atomicAdd(&counts[1], (unsigned long long)__popcll(bm));
        }
    }
}

__global__ void __launch_bounds__(DG_NT) dg_gather_kernel(const MirpAln* __restrict__ a, long long n, const int* __restrict__ flag,
                                                          const long long* __restrict__ fs, unsigned long long* __restrict__ skey,
                                                          unsigned* __restrict__ sdep) {
    for (long long i = (long long)blockIdx.x * DG_NT + threadIdx.x; i < n; i += (long long)gridDim.x * DG_NT) {
        if (!flag[i]) continue;
        const MirpAln r = a[i];
        const long long j = fs[i];
        skey[j] = ((unsigned long long)(unsigned)r.tid << 32) | (unsigned long long)(unsigned)r.pos;
        sdep[j] = r.depth;
    }
}

__global__ void __launch_bounds__(DG_NT) dg_head_kernel(const unsigned long long* __restrict__ skey, long long ns, int* __restrict__ head) {
    for (long long j = (long long)blockIdx.x * DG_NT + threadIdx.x; j < ns; j += (long long)gridDim.x * DG_NT)
        head[j] = j == 0 || skey[j] != skey[j - 1];
}

// ukey[u] = the unit's key, uab[u] += the depths of its records (uab zeroed before)
__global__ void __launch_bounds__(DG_NT) dg_unit_kernel(const unsigned long long* __restrict__ skey, const unsigned* __restrict__ sdep,
                                                        const int* __restrict__ head, const long long* __restrict__ hs, long long ns,
                                                        unsigned long long* __restrict__ ukey, unsigned long long* __restrict__ uab) {
    for (long long base = (long long)blockIdx.x * DG_NT; base < ns; base += (long long)gridDim.x * DG_NT) {
        const long long j = base + threadIdx.x;
        long long u = -1;
        unsigned long long d = 0;
        if (j < ns) {
            const int h = head[j];
            u = hs[j] + h - 1;
            d = sdep[j];
            if (h) ukey[u] = skey[j];
        }
        cl_wave_atomic<0>(uab, u, d);
    }
}

// per transcript: amax = the largest abundance, npos = units, tot = the sum of the abundances (all zeroed before)
__global__ void __launch_bounds__(DG_NT) dg_tstat_kernel(const unsigned long long* __restrict__ ukey, const unsigned long long* __restrict__ uab, long long nu,
                                                         unsigned long long* __restrict__ amax, unsigned long long* __restrict__ npos,
                                                         unsigned long long* __restrict__ tot) {
    for (long long base = (long long)blockIdx.x * DG_NT; base < nu; base += (long long)gridDim.x * DG_NT) {
        const long long u = base + threadIdx.x;
        long long t = -1;
        unsigned long long a = 0;
        if (u < nu) {
            t = (long long)(ukey[u] >> 32);
            a = uab[u];
        }
        cl_wave_atomic<1>(amax, t, a);
        cl_wave_atomic<0>(npos, t, 1ull);
        cl_wave_atomic<0>(tot, t, a);
    }
}

// nmax = units whose abundance is the transcript's amax
__global__ void __launch_bounds__(DG_NT) dg_nmax_kernel(const unsigned long long* __restrict__ ukey, const unsigned long long* __restrict__ uab, long long nu,
                                                        const unsigned long long* __restrict__ amax, unsigned long long* __restrict__ nmax) {
    for (long long base = (long long)blockIdx.x * DG_NT; base < nu; base += (long long)gridDim.x * DG_NT) {
        const long long u = base + threadIdx.x;
        long long t = -1;
        if (u < nu) {
            const long long tt = (long long)(ukey[u] >> 32);
            if (uab[u] == amax[tt]) t = tt;
        }
        cl_wave_atomic<0>(nmax, t, 1ull);
    }
}

// the category of every unit, ccount[k] += units of category k, keep[u] = category <= max_cat
__global__ void __launch_bounds__(DG_NT) dg_cat_kernel(const unsigned long long* __restrict__ ukey, const unsigned long long* __restrict__ uab, long long nu,
                                                       const unsigned long long* __restrict__ amax, const unsigned long long* __restrict__ nmax,
                                                       const unsigned long long* __restrict__ npos, const unsigned long long* __restrict__ tot, int max_cat,
                                                       unsigned char* __restrict__ ucat, int* __restrict__ keep, unsigned long long* __restrict__ ccount) {
    for (long long base = (long long)blockIdx.x * DG_NT; base < nu; base += (long long)gridDim.x * DG_NT) {
        const long long u = base + threadIdx.x;
        int cat = -1;
        if (u < nu) {
            const long long t = (long long)(ukey[u] >> 32);
            const unsigned long long a = uab[u], mx = amax[t], np = npos[t];
            // a * npos > tot in 128 bits
            const bool above = __umul64hi(a, np) != 0 || a * np > tot[t];
            cat = a == 1 ? 4 : a == mx ? (nmax[t] == 1 ? 0 : 1) : above ? 2 : 3;
            ucat[u] = (unsigned char)cat;
            keep[u] = cat <= max_cat;
        }
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const unsigned long long b = __ballot(cat == k);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ccount[k], (unsigned long long)__popcll(b));
        }
    }
}

// the window of every kept unit; sqstart / sqlen: the transcript's first packed position and its length, by SAM tid
__global__ void __launch_bounds__(DG_NT) dg_window_kernel(TgRef R, const unsigned long long* __restrict__ ukey, const unsigned char* __restrict__ ucat,
                                                          const int* __restrict__ keep, const long long* __restrict__ ks, long long nu,
                                                          const unsigned long long* __restrict__ sqstart, const long long* __restrict__ sqlen,
                                                          DgWin* __restrict__ win) {
    for (long long u = (long long)blockIdx.x * DG_NT + threadIdx.x; u < nu; u += (long long)gridDim.x * DG_NT) {
        if (!keep[u]) continue;
        const unsigned long long k = ukey[u];
        const long long t = (long long)(k >> 32);
        const long long p = (long long)(k & 0xffffffffull);           // 1 <= p <= LN
        const unsigned long long g = sqstart[t] + (unsigned long long)(p - 1);
        unsigned wl = 0, wh = 0, avail = 0;
        if (p + 9 <= sqlen[t]) {                                      // else no miRNA position 1 in the transcript: no site at all
            const long long s = (long long)g + 9 - 31;                // packed position of window position 0; g + 9 < total
            unsigned long long w;
            unsigned am;
            if (s >= 0) {
                const unsigned long long q = (unsigned long long)s >> 5;
                const unsigned sh = 2 * (unsigned)(s & 31);
                w = R.pk[q];
                if (sh) w = (w >> sh) | (R.pk[q + 1] << (64 - sh));
                am = tg_bits32(R.amb, (unsigned long long)s);
            } else {                                                  // before packed position 0: the first transcript, p + 9 = 32 + s bases
                const unsigned d = (unsigned)(-s);                    // 1 .. 22
                w = R.pk[0] << (2 * d);
                am = R.amb[0] << d;
            }
            wl = tg_even(w);
            wh = tg_even(w >> 1);
            const unsigned clean = am ? (unsigned)__clz((int)am) : 32u;
            avail = (unsigned)std::min<long long>(std::min<long long>(32, p + 9), (long long)clean);
        }
        DgWin o;
        o.wl = wl;
        o.wh = wh;
        o.meta = avail | ((unsigned)ucat[u] << 8);
        o.gpos = (unsigned)g;
        win[ks[u]] = o;
    }
}

// miRNAs [m0, m1) of the group's anchored array against the nk windows.  MODE 1: hist[(m * 5 + category) * 17 + half] += hits.
// MODE 0: hits at packed positions [g0, g1) whose bin is set in bins[m * 5 + category] (bit half) append their key (keys[0 .. cap), counter[0] =
// hits, also past cap).
template <int MODE>
__global__ __launch_bounds__(DG_NT) void dg_scan_kernel(const DgWin* __restrict__ win, long long nk, unsigned long long g0, unsigned long long g1,
                                                        const TgMirna* __restrict__ mi, int m0, int m1,
                                                        const unsigned* __restrict__ bins, unsigned long long* __restrict__ keys, unsigned long long cap,
                                                        unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hist) {
    const long long k = (long long)blockIdx.x * DG_NT + threadIdx.x;
    unsigned wl = 0, wh = 0, avail = 0, cat = 0, gpos = 0;            // a lane past nk has avail 0: no miRNA (L >= 12) fits
    if (k < nk) {
        const uint4 w = reinterpret_cast<const uint4*>(win)[k];
        wl = w.x;
        wh = w.y;
        avail = w.z & 0xffu;
        cat = w.z >> 8;
        gpos = w.w;
        if (MODE == 0 && (gpos < g0 || gpos >= g1)) avail = 0;
    }
    const unsigned tG = ~wl & wh, tT = wl & wh;
    for (int m = m0; m < m1; m++) {
        const TgMirna& M = mi[m];
        if ((unsigned)M.L > avail) continue;
        unsigned h;
        if (tg_eval(M.s[0], M.lmask, wl, wh, tT, tG, (unsigned)M.smin, (unsigned)(M.smax - M.smin), &h)) {
            if (MODE == 1) {
                atomicAdd(&hist[((long long)m * 5 + cat) * TG_NHALF + h], 1ull);
            } else if ((bins[(long long)m * 5 + cat] >> h) & 1u) {
                const unsigned long long i = atomicAdd(counter, 1ull);
                if (i < cap) keys[i] = ((unsigned long long)m << 40) | ((unsigned long long)cat << 37) | ((unsigned long long)h << 32) | gpos;
            }
        }
    }
}

// sorted key -> {key, the unit's reads, its transcript's amax}; cstart[0 .. n_f]: the transcripts' first packed positions, f2s: FASTA index -> SAM tid
__global__ void __launch_bounds__(DG_NT) dg_hit_kernel(const unsigned long long* __restrict__ keys, long long n, const unsigned long long* __restrict__ cstart,
                                                       int n_f, const int* __restrict__ f2s, const unsigned long long* __restrict__ ukey,
                                                       const unsigned long long* __restrict__ uab, long long nu, const unsigned long long* __restrict__ amax,
                                                       MirpDgHit* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * DG_NT + threadIdx.x; i < n; i += (long long)gridDim.x * DG_NT) {
        const unsigned long long key = keys[i], g = key & 0xffffffffull;
        const int a = site_contig(cstart, n_f, g);   // the transcript
        const unsigned long long t = (unsigned long long)(unsigned)f2s[a];
        const unsigned long long uk = (t << 32) | (g - cstart[a] + 1);
        long long lo = 0, hi = nu - 1;               // the unit exists
        while (lo < hi) { const long long md = (lo + hi) >> 1; if (ukey[md] < uk) lo = md + 1; else hi = md; }
        MirpDgHit o;
        o.key = key;
        o.reads = uab[lo];
        o.tmax = amax[t];
        out[i] = o;
    }
}

}  // namespace mirp


#define DG_SYNC(c, st)                          \
    do {                                        \
        HIPCHK(c, hipGetLastError());           \
        HIPCHK(c, hipStreamSynchronize(st));    \
    } while (0)

// See mirp_ctx.h.
int mirp_device_degradome(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                          const std::vector<unsigned long long>& cstart, const std::vector<int>& f2s, const std::vector<unsigned long long>& sqstart,
                          const std::vector<long long>& sqlen, std::vector<TgMirna>& mi, std::vector<TgMirna>& mi_anchored, int max_half, int max_cat, double alpha,
                          const MirpDgSink& sink, long long stats[12], double seconds[6]) {
    using namespace mirp;
    const hipStream_t st = c->stream;
    const long long n = c->n_alns;
    const MirpAln* alns = (const MirpAln*)c->alns.p;
    const int n_sq = (int)sqlen.size(), n_f = (int)cstart.size() - 1;
    const long long n_mi = (long long)mi.size();
    const long long cap = c->tg_cap > 0 ? c->tg_cap : (1ll << 26);
    std::memset(stats, 0, 12 * sizeof(long long));
    std::memset(seconds, 0, 6 * sizeof(double));
    if (n > (1ll << 31) - 2) return fail(c, -5, "mirp_degradome_scan: more than 2^31 records");
    TmpDevice T;
    double t0 = mirp::now();
    // ---- upload: the packed transcripts (the buffers of the target-site search) and the tables by SAM tid / FASTA index
    if (c->tg_mi.ensure(sizeof(TgMirna) * TG_GROUP) || c->tg_hist.ensure(8 * (size_t)TG_GROUP * TG_NHALF) || c->tg_small.ensure(64))
        return fail(c, -6, "device allocation failed (degradome)");
    long long* d_sqlen = (long long*)T.get(8 * (size_t)std::max(n_sq, 1));
    unsigned long long* d_sqstart = (unsigned long long*)T.get(8 * (size_t)std::max(n_sq, 1));
    int* d_f2s = (int*)T.get(4 * (size_t)std::max(n_f, 1));
    unsigned long long* d_tstat = (unsigned long long*)T.get(8 * 4 * (size_t)std::max(n_sq, 1));     // amax, nmax, npos, tot
    unsigned long long* d_counts = (unsigned long long*)T.get(8 * 8);                                 // sense, minus, C_0 .. C_4
    if (!d_sqlen || !d_sqstart || !d_f2s || !d_tstat || !d_counts) return fail(c, -6, "device allocation failed (degradome)");
    TgRef R;
    if (int rc = tg_upload_packed(c, pk, amb, cst, total, cstart, &R)) return rc;
    if (n_sq > 0) {
        HIPCHK(c, hipMemcpyAsync(d_sqlen, sqlen.data(), 8 * (size_t)n_sq, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_sqstart, sqstart.data(), 8 * (size_t)n_sq, hipMemcpyHostToDevice, st));
    }
    if (n_f > 0) HIPCHK(c, hipMemcpyAsync(d_f2s, f2s.data(), 4 * (size_t)n_f, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_tstat, 0, 8 * 4 * (size_t)std::max(n_sq, 1), st));
    HIPCHK(c, hipMemsetAsync(d_counts, 0, 64, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] = mirp::now() - t0;
    unsigned long long* amax = d_tstat;
    unsigned long long* nmax = d_tstat + (size_t)std::max(n_sq, 1);
    unsigned long long* npos = d_tstat + 2 * (size_t)std::max(n_sq, 1);
    unsigned long long* tot = d_tstat + 3 * (size_t)std::max(n_sq, 1);

    // ---- units, categories, windows
    t0 = mirp::now();
    long long ns = 0, nu = 0, nk = 0;
    unsigned long long* ukey = nullptr;
    unsigned long long* uab = nullptr;
    DgWin* win = nullptr;
    if (n > 0) {
        int* flag = (int*)T.get(4 * (size_t)n);
        long long* fs = (long long*)T.get(8 * (size_t)(n + 1));
        if (!flag || !fs) return fail(c, -6, "device allocation failed (degradome: records)");
        hipLaunchKernelGGL(dg_flag_kernel, dim3(dg_grid(n)), dim3(DG_NT), 0, st, alns, n, (const long long*)d_sqlen, n_sq, flag, d_counts);
        launch_excl_scan(st, flag, fs, n);
        HIPCHK(c, hipMemcpyAsync(&ns, fs + n, 8, hipMemcpyDeviceToHost, st));
        DG_SYNC(c, st);
        if (ns > 0) {
            unsigned long long* skey = (unsigned long long*)T.get(8 * (size_t)ns);
            unsigned* sdep = (unsigned*)T.get(4 * (size_t)ns);
            int* head = (int*)T.get(4 * (size_t)ns);
            long long* hs = (long long*)T.get(8 * (size_t)(ns + 1));
            if (!skey || !sdep || !head || !hs) return fail(c, -6, "device allocation failed (degradome: records)");
            hipLaunchKernelGGL(dg_gather_kernel, dim3(dg_grid(n)), dim3(DG_NT), 0, st, alns, n, (const int*)flag, (const long long*)fs, skey, sdep);
            hipLaunchKernelGGL(dg_head_kernel, dim3(dg_grid(ns)), dim3(DG_NT), 0, st, (const unsigned long long*)skey, ns, head);
            launch_excl_scan(st, head, hs, ns);
            HIPCHK(c, hipMemcpyAsync(&nu, hs + ns, 8, hipMemcpyDeviceToHost, st));
            DG_SYNC(c, st);
            ukey = (unsigned long long*)T.get(8 * (size_t)nu);
            uab = (unsigned long long*)T.get(8 * (size_t)nu);
            unsigned char* ucat = (unsigned char*)T.get((size_t)nu);
            int* keep = (int*)T.get(4 * (size_t)nu);
            long long* ks = (long long*)T.get(8 * (size_t)(nu + 1));
            if (!ukey || !uab || !ucat || !keep || !ks) return fail(c, -6, "device allocation failed (degradome: units)");
            HIPCHK(c, hipMemsetAsync(uab, 0, 8 * (size_t)nu, st));
            hipLaunchKernelGGL(dg_unit_kernel, dim3(dg_grid(ns)), dim3(DG_NT), 0, st, (const unsigned long long*)skey, (const unsigned*)sdep, (const int*)head,
                               (const long long*)hs, ns, ukey, uab);
            hipLaunchKernelGGL(dg_tstat_kernel, dim3(dg_grid(nu)), dim3(DG_NT), 0, st, (const unsigned long long*)ukey, (const unsigned long long*)uab, nu, amax,
                               npos, tot);
            hipLaunchKernelGGL(dg_nmax_kernel, dim3(dg_grid(nu)), dim3(DG_NT), 0, st, (const unsigned long long*)ukey, (const unsigned long long*)uab, nu,
                               (const unsigned long long*)amax, nmax);
            hipLaunchKernelGGL(dg_cat_kernel, dim3(dg_grid(nu)), dim3(DG_NT), 0, st, (const unsigned long long*)ukey, (const unsigned long long*)uab, nu,
                               (const unsigned long long*)amax, (const unsigned long long*)nmax, (const unsigned long long*)npos, (const unsigned long long*)tot,
                               max_cat, ucat, keep, d_counts + 2);
            launch_excl_scan(st, keep, ks, nu);
            HIPCHK(c, hipMemcpyAsync(&nk, ks + nu, 8, hipMemcpyDeviceToHost, st));
            DG_SYNC(c, st);
            if (nk > 0) {
                win = (DgWin*)T.get(sizeof(DgWin) * (size_t)nk);
                if (!win) return fail(c, -6, "device allocation failed (degradome: windows)");
                hipLaunchKernelGGL(dg_window_kernel, dim3(dg_grid(nu)), dim3(DG_NT), 0, st, R, (const unsigned long long*)ukey, (const unsigned char*)ucat,
                                   (const int*)keep, (const long long*)ks, nu, (const unsigned long long*)d_sqstart, (const long long*)d_sqlen, win);
                DG_SYNC(c, st);
            }
        }
    }
    unsigned long long h_counts[8];
    HIPCHK(c, hipMemcpyAsync(h_counts, d_counts, 64, hipMemcpyDeviceToHost, st));
    DG_SYNC(c, st);
    seconds[1] = mirp::now() - t0;
    stats[0] = n;
    stats[1] = (long long)h_counts[0];
    stats[2] = (long long)h_counts[1];
    stats[3] = nu;
    for (int k = 0; k < 5; k++) stats[4 + k] = (long long)h_counts[2 + k];
    stats[9] = nk * n_mi;
    if (nk == 0 || n_mi == 0 || total == 0) return 0;
    unsigned long long ccum[5];
    for (int k = 0; k < 5; k++) ccum[k] = h_counts[2 + k] + (k ? ccum[k - 1] : 0);

    // ---- per group of miRNAs: site counts, anchored counts, p-values, key passes
    const int gmax = (int)std::min<long long>(TG_GROUP, n_mi);
    TgMirna* d_mi = (TgMirna*)c->tg_mi.p;
    TgMirna* d_mia = (TgMirna*)T.get(sizeof(TgMirna) * (size_t)gmax);
    unsigned long long* d_hist = (unsigned long long*)T.get(8 * (size_t)gmax * 5 * TG_NHALF);
    unsigned* d_bins = (unsigned*)T.get(4 * (size_t)gmax * 5);
    unsigned long long* d_small = (unsigned long long*)c->tg_small.p;
    if (!d_mia || !d_hist || !d_bins) return fail(c, -6, "device allocation failed (degradome: miRNAs)");
    std::vector<unsigned long long> sites((size_t)gmax * TG_NHALF), hist((size_t)gmax * 5 * TG_NHALF);
    std::vector<double> pval((size_t)gmax * 5 * TG_NHALF);
    std::vector<unsigned> bins((size_t)gmax * 5), pbins((size_t)gmax * 5);
    std::vector<size_t> kept;                       // the kept bins of a group in output order, as indices into hist
    std::vector<MirpDgHit> h_hits;
    for (long long m = 0; m < n_mi; m++) {
        mi[(size_t)m].smin = mi_anchored[(size_t)m].smin = 0;
        mi[(size_t)m].smax = mi_anchored[(size_t)m].smax = max_half;
    }
    for (long long mbase = 0; mbase < n_mi; mbase += TG_GROUP) {
        const int gn = (int)std::min<long long>(TG_GROUP, n_mi - mbase);
        // site counts N_m(h): the counting scan of the target-site search over every offset, plus strand
        t0 = mirp::now();
        HIPCHK(c, hipMemcpyAsync(d_mi, mi.data() + mbase, sizeof(TgMirna) * (size_t)gn, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_mia, mi_anchored.data() + mbase, sizeof(TgMirna) * (size_t)gn, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(c->tg_hist.p, 0, 8 * (size_t)gn * TG_NHALF, st));
        for (unsigned long long q = 0; q < (unsigned long long)total; q += (unsigned long long)TG_LAUNCH_POS) {
            const unsigned long long q1 = std::min((unsigned long long)total, q + (unsigned long long)TG_LAUNCH_POS);
            hipLaunchKernelGGL((tg_scan_kernel<1, false>), dim3((unsigned)((q1 - q + 255) / 256)), dim3(256), 0, st, R, (const TgMirna*)d_mi, 0, gn, q, q1,
                               (unsigned long long*)nullptr, 0ull, (unsigned long long*)nullptr, (unsigned long long*)c->tg_hist.p);
        }
        HIPCHK(c, hipMemcpyAsync(sites.data(), c->tg_hist.p, 8 * (size_t)gn * TG_NHALF, hipMemcpyDeviceToHost, st));
        DG_SYNC(c, st);
        for (int m = 0; m < gn; m++)
            for (int h = 1; h < TG_NHALF; h++) sites[(size_t)m * TG_NHALF + h] += sites[(size_t)m * TG_NHALF + h - 1];
        seconds[2] += mirp::now() - t0;
        // anchored counting pass
        t0 = mirp::now();
        HIPCHK(c, hipMemsetAsync(d_hist, 0, 8 * (size_t)gn * 5 * TG_NHALF, st));
        hipLaunchKernelGGL((dg_scan_kernel<1>), dim3((unsigned)((nk + DG_NT - 1) / DG_NT)), dim3(DG_NT), 0, st, (const DgWin*)win, nk, 0ull, 0ull, (const TgMirna*)d_mia, 0, gn,
                           (const unsigned*)nullptr, (unsigned long long*)nullptr, 0ull, (unsigned long long*)nullptr, d_hist);
        HIPCHK(c, hipMemcpyAsync(hist.data(), d_hist, 8 * (size_t)gn * 5 * TG_NHALF, hipMemcpyDeviceToHost, st));
        DG_SYNC(c, st);
        seconds[3] += mirp::now() - t0;
        // p per (miRNA, category, half-score); the bins at or below alpha stay
        t0 = mirp::now();
        long long surviving = 0;
        kept.clear();
        for (int m = 0; m < gn; m++)
            for (int k = 0; k < 5; k++) {
                unsigned b = 0;
                for (int h = 0; h <= max_half; h++) {
                    const size_t i = ((size_t)m * 5 + k) * TG_NHALF + h;
                    const double nsites = (double)sites[(size_t)m * TG_NHALF + h];
                    const double p = ccum[k] >= (unsigned long long)total ? 1.0 : -std::expm1(nsites * std::log1p(-((double)ccum[k] / (double)total)));
                    pval[i] = p;
                    if (hist[i] && p <= alpha) {
                        b |= 1u << h;
                        surviving += (long long)hist[i];
                        kept.push_back(i);
                    }
                }
                bins[(size_t)m * 5 + k] = b;
            }
        if (surviving == 0) { seconds[4] += mirp::now() - t0; continue; }
        const long long kcap = std::max(2ll, std::min(cap, surviving));
        TmpDevice K;
        unsigned long long* d_keys = (unsigned long long*)K.get(8 * (size_t)kcap);
        unsigned long long* d_ktmp = (unsigned long long*)K.get(8 * (size_t)kcap);
        MirpDgHit* d_hits = (MirpDgHit*)K.get(sizeof(MirpDgHit) * (size_t)kcap);
        if (!d_keys || !d_ktmp || !d_hits) return fail(c, -6, "device allocation failed (degradome: keys)");
        int mbits = 0;
        while ((1 << mbits) < gn) mbits++;
        // one pass: miRNAs [ma, mb] with the bins of pbins, packed positions [g0, g1); `want` keys expected (-1: any number, may exceed kcap)
        auto pass = [&](int ma, int mb, unsigned long long g0, unsigned long long g1, long long want, long long* got) -> int {
            HIPCHK(c, hipMemcpyAsync(d_bins + (size_t)ma * 5, pbins.data() + (size_t)ma * 5, 4 * 5 * (size_t)(mb - ma + 1), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemsetAsync(d_small, 0, 8, st));
            hipLaunchKernelGGL((dg_scan_kernel<0>), dim3((unsigned)((nk + DG_NT - 1) / DG_NT)), dim3(DG_NT), 0, st, (const DgWin*)win, nk, g0, g1, (const TgMirna*)d_mia,
                               ma, mb + 1, (const unsigned*)d_bins, d_keys, (unsigned long long)kcap, d_small, (unsigned long long*)nullptr);
            unsigned long long h = 0;
            HIPCHK(c, hipMemcpyAsync(&h, d_small, 8, hipMemcpyDeviceToHost, st));
            DG_SYNC(c, st);
            *got = (long long)h;
            if (want >= 0 && *got != want) return fail(c, -5, "degradome: a pass found a different number of hits than counted");
            if (*got > kcap) return 0;
            stats[11]++;
            if (*got == 0) return 0;
            if (int rc = mirp_device_sort_u64(c, d_keys, d_ktmp, *got, 0, (40 + mbits + 7) / 8 * 8)) return rc;
            hipLaunchKernelGGL(dg_hit_kernel, dim3(dg_grid(*got)), dim3(DG_NT), 0, st, (const unsigned long long*)d_keys, *got,
                               (const unsigned long long*)c->tg_cstart.p, n_f, (const int*)d_f2s, (const unsigned long long*)ukey, (const unsigned long long*)uab, nu,
                               (const unsigned long long*)amax, d_hits);
            h_hits.resize((size_t)*got);
            HIPCHK(c, hipMemcpyAsync(h_hits.data(), d_hits, sizeof(MirpDgHit) * (size_t)*got, hipMemcpyDeviceToHost, st));
            DG_SYNC(c, st);
            stats[10] += *got;
            return sink((int)mbase, h_hits.data(), (size_t)*got, sites.data(), pval.data());
        };
        // the bins are the kept (miRNA, category, half-score), the positions of a bin over kcap are the packed positions.  pbins
        // holds the bins of the pass under way, bit h of row miRNA * 5 + category as in `bins`, and is cleared after it
        const auto count = [&](long long i) { return (long long)hist[kept[(size_t)i]]; };
        const auto flush = [&](long long first, long long last, long long expected) -> int {
            const size_t ra = kept[(size_t)first] / TG_NHALF, rb = kept[(size_t)last] / TG_NHALF;
            std::copy(bins.begin() + ra, bins.begin() + rb + 1, pbins.begin() + ra);
            pbins[ra] &= ~0u << (kept[(size_t)first] % TG_NHALF);
            pbins[rb] &= (2u << (kept[(size_t)last] % TG_NHALF)) - 1u;
            long long got = 0;
            const int rc = pass((int)(ra / 5), (int)(rb / 5), 0ull, (unsigned long long)total, expected, &got);
            std::fill(pbins.begin() + ra, pbins.begin() + rb + 1, 0u);
            return rc;
        };
        const auto range = [&](long long bin, unsigned long long g0, unsigned long long g1, long long* got) -> int {
            const size_t row = kept[(size_t)bin] / TG_NHALF;
            pbins[row] = 1u << (kept[(size_t)bin] % TG_NHALF);
            const int rc = pass((int)(row / 5), (int)(row / 5), g0, g1, -1, got);
            pbins[row] = 0;
            return rc;
        };
        std::fill(pbins.begin(), pbins.end(), 0u);
        const int rc = plan_passes((long long)kept.size(), count, kcap, (unsigned long long)total, flush, range);
        if (rc) return rc == PLAN_POSITION_OVER_CAP ? fail(c, -5, "degradome: one position holds more hits of one miRNA, category and score than a pass") : rc;
        seconds[4] += mirp::now() - t0;
    }
    return 0;
}
