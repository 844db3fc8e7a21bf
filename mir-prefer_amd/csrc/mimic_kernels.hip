// Device side of the endogenous-target-mimic search (mirp_mimic_scan, mirp_mimics.cpp), with the semantics of DESIGN.md §27.
//
// A mimic site pairs miRNA positions 2..8 with Watson-Crick pairs only, so the scan is anchored on that seed instead of walking every miRNA at every
// offset.  The host sorts the miRNAs by the 14-bit code of positions 2..8 (position 2 in the low bits, A C G U = 0..3) and builds the start table
// start[0 .. 16384]: bucket k = sorted entries [start[k], start[k + 1]).  The packed targets, the bit planes and the TgStrand masks are those of the
// target-site search (targets_device.h, targets_bulge_device.h).
//
//   scan   mm_scan_kernel: one lane per forward position q.  The 7-mer at q .. q + 6 is a seed when none of its bases is ambiguous and no contig
//          starts inside it.  On the minus strand the key is the 7-mer itself and the interval starts at o = q - 1; on the plus strand the key is
//          its reverse complement and o = q + 8 - G - L, which differs per miRNA of the bucket.  A lane with a non-empty bucket loads the 38 bases of
//          its strand's span (from q - 30 on the plus strand, from q - 1 on the minus strand) as 64-bit bit planes once and evaluates every entry of
//          the bucket from two windows, U(o) and U(o + G): a placement P is a mask select between the two, as in tg_bulge_best<true>.  A hit is the key
//          miRNA << 38 | imperfect << 35 | o << 3 | strand << 2 | (P - 9) (MODE 0) or a count in hist[miRNA * 8 + imperfect] (MODE 1).
//   order  mirp_device_sort_u64 by the whole key: miRNA (file order), imperfect, target, start, + before -.
//   cut    mm_size_kernel (-k from the rank inside the miRNA's run plus what earlier passes emitted), launch_excl_scan; emit: mm_emit_kernel.
// Passes of at most `cap` keys are planned by plan_passes (pass_plan.h) with (miRNA, imperfect) as the bins and the interval
// starts o as the positions (the output order within a bin; the lanes that can hold a start of [o0, o1) are q in [o0, o1 + 30)); one o holds at most
// two sites of one bin (one per strand), the smallest capacity the ABI takes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "mimic_device.h"
#include "mirp_ctx.h"
#include "pass_plan.h"
#include "text_out.h"

namespace mirp {

// ---------------------------------------------------------------- scan
template <int MODE>
__device__ __forceinline__ void mm_bucket(const MmSpan& W, int s, unsigned G, unsigned e0, unsigned e1, const TgMirna* __restrict__ mi,
                                          const unsigned* __restrict__ mid, unsigned long long q, unsigned long long o0, unsigned long long o1, unsigned long long* __restrict__ keys,
                                          unsigned long long cap, unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hist) {
    for (unsigned e = e0; e < e1; e++) {
        const TgMirna& M = mi[e];
        if (M.smin > M.smax) continue;                          // not in this pass
        const unsigned L = (unsigned)M.L, n = L + G;
        const unsigned sh = s ? 0u : 38u - n;                  // the interval's first base inside the span
        if (!mm_span_clear(W, sh, n)) continue;
        const unsigned long long o = s ? q - 1 : q + 8 - n;      // >= 0: the positions before 0 are not clear
        if (o < o0 || o >= o1) continue;
        const unsigned a = s ? sh : sh + G, b = s ? sh + G : sh;          // A pairs positions 1..P, B positions P + 1..L
        unsigned nwA, mmA, nwB, mmB;
        tg_masks(M.s[s], M.lmask, (unsigned)(W.pl >> a), (unsigned)(W.ph >> a), s, &nwA, &mmA);
        tg_masks(M.s[s], M.lmask, (unsigned)(W.pl >> b), (unsigned)(W.ph >> b), s, &nwB, &mmB);
        const unsigned r = mm_best(M.lmask, (int)L, s, nwA, mmA, nwB, mmB);
        const unsigned imp = r >> 8;
        if ((int)imp < M.smin || (int)imp > M.smax) continue;                          // also r = ~0u: no placement closes the loop
        if (MODE == 0) {
            const unsigned long long i = atomicAdd(counter, 1ull);
            if (i < cap)
                keys[i] = ((unsigned long long)mid[e] << MM_SHIFT) | ((unsigned long long)imp << 35) | (o << 3) | ((unsigned long long)s << 2) | ((r & 31u) - 9u);
        } else {
            atomicAdd(&hist[(unsigned long long)mid[e] * MM_NBIN + imp], 1ull);
        }
    }
}

// lanes [p0, p1), of which the sites whose interval starts in [o0, o1) are taken; mi / mid: the miRNAs in seed order (smin .. smax = the imperfect range of the pass, smin > smax = not in the pass) and their
// indices in file order; counter[0] = hits (also past cap); counter[8 + 2 k], counter[9 + 2 k], k < MM_STAT_SLOTS: seeds looked up and bucket entries evaluated, summed by the host.
template <int MODE, bool BOTH>
__global__ __launch_bounds__(256) void mm_scan_kernel(TgRef R, const unsigned* __restrict__ start, const TgMirna* __restrict__ mi, const unsigned* __restrict__ mid,
                                                      unsigned G, unsigned long long p0, unsigned long long p1, unsigned long long o0, unsigned long long o1,
                                                      unsigned long long* __restrict__ keys,
                                                      unsigned long long cap, unsigned long long* __restrict__ counter, unsigned long long* __restrict__ hist) {
    const unsigned long long q = p0 + (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    unsigned looked = 0, evaluated = 0;
    if (q < p1 && ((tg_bits32(R.amb, q) & 0x7fu) | (tg_bits32(R.cst, q) & 0x7eu)) == 0) {
        const unsigned long long w = R.pk[q >> 5];
        const unsigned sh = 2 * (unsigned)(q & 31);
        const unsigned kmer = (unsigned)(sh ? (w >> sh) | (R.pk[(q >> 5) + 1] << (64 - sh)) : w) & 0x3fffu;
        #pragma unroll
        for (int s = 0; s < (BOTH ? 2 : 1); s++) {
            const unsigned key = s ? kmer : mm_revcomp7(kmer);
            const unsigned e0 = start[key], e1 = start[key + 1];
            looked++;
            if (e0 == e1) continue;
            evaluated += e1 - e0;
            const MmSpan W = mm_span(R, q, s ? 1u : 30u);
            mm_bucket<MODE>(W, s, G, e0, e1, mi, mid, q, o0, o1, keys, cap, counter, hist);
        }
    }
    unsigned long long nl = looked, ne = evaluated;
    for (int off = 32; off > 0; off >>= 1) { nl += __shfl_xor(nl, off, 64); ne += __shfl_xor(ne, off, 64); }
    if ((threadIdx.x & 63) == 0 && (nl | ne)) {                     // spread over MM_STAT_SLOTS addresses: one address for every wave of the grid serialises
        unsigned long long* slot = counter + 8 + 2 * (blockIdx.x & (MM_STAT_SLOTS - 1));
        atomicAdd(slot, nl);
        atomicAdd(slot + 1, ne);
    }
}

// ---------------------------------------------------------------- text
struct MmText {
    const unsigned long long* pk;
    const unsigned char* mcodes;            // 32 per miRNA (file order): 0..3 = A C G U, 4 = unknown
    const int* mlen;                        // file order
    const char* mnames; const long long* mnoff;
    const char* tnames; const long long* tnoff;
    const unsigned long long* cstart; int n_contigs;
    int G;
};

__device__ __forceinline__ int mm_class(unsigned mc, unsigned y) {
    if (mc > 3) return 2;
    if (mc + y == 3) return 0;
    return (mc == 2 && y == 3) || (mc == 3 && y == 2) ? 1 : 2;
}

// one line: miRNA target start end strand imperfect mismatches gu mirna_5to3 pairs target_3to5 loop.  Column c = 1 .. L + G of the three aligned
// strings holds miRNA position c (c <= P), nothing (the G loop bases) or position c - G, over the target-strand base of the column.
template <bool WRITE>
__device__ long long mm_line(const MmText& T, unsigned long long key, char* out) {
    TextOut<WRITE> o{out};
    const long long m = (long long)(key >> MM_SHIFT);
    const unsigned imp = (unsigned)(key >> 35) & 7u;
    const unsigned long long g = (key >> 3) & 0xffffffffull;
    const int strand = (int)(key >> 2) & 1, P = 9 + (int)(key & 3), G = T.G;
    const int L = T.mlen[m], W = L + G;
    const unsigned char* mc = T.mcodes + 32 * m;
    int a = 0, z = T.n_contigs;                 // target: last cstart <= g
    while (z - a > 1) { const int md = (a + z) >> 1; if (T.cstart[md] <= g) a = md; else z = md; }
    auto pos = [&](int c) { return c <= P ? c : c <= P + G ? 0 : c - G; };
    auto base = [&](int c) -> unsigned {
        const unsigned b = tg_base(T.pk, strand ? g + c - 1 : g + W - c);
        return strand ? 3u - b : b;
    };
    int nmm = 0, ngu = 0;
    for (int c = 1; c <= W; c++) {
        const int i = pos(c);
        if (!i) continue;
        const int k = mm_class(mc[i - 1], base(c));
        nmm += k == 2;
        ngu += k == 1;
    }
    o.str(T.mnames + T.mnoff[m], T.mnoff[m + 1] - T.mnoff[m]);
    o.ch('\t');
    o.str(T.tnames + T.tnoff[a], T.tnoff[a + 1] - T.tnoff[a]);
    o.ch('\t');
    o.num(g - T.cstart[a] + 1);
    o.ch('\t');
    o.num(g - T.cstart[a] + W);
    o.ch('\t');
    o.ch(strand ? '-' : '+');
    o.ch('\t');
    o.num(imp);
    o.ch('\t');
    o.num((unsigned long long)nmm);
    o.ch('\t');
    o.num((unsigned long long)ngu);
    o.ch('\t');
    const char* RNA = "ACGUN";
    for (int c = 1; c <= W; c++) { const int i = pos(c); o.ch(i ? RNA[mc[i - 1]] : '-'); }
    o.ch('\t');
    for (int c = 1; c <= W; c++) {
        const int i = pos(c);
        const int k = i ? mm_class(mc[i - 1], base(c)) : 3;
        o.ch(k == 0 ? '|' : k == 1 ? 'o' : k == 2 ? 'x' : '-');
    }
    o.ch('\t');
    for (int c = 1; c <= W; c++) o.ch(RNA[base(c)]);
    o.ch('\t');
    o.num((unsigned long long)P);
    o.ch('\n');
    return o.n;
}

// first index of the miRNA run that holds keys[i] (the keys are sorted)
__device__ __forceinline__ long long mm_run_first(const unsigned long long* __restrict__ keys, long long i) {
    const unsigned long long lo = keys[i] >> MM_SHIFT << MM_SHIFT;
    long long a = 0, z = i;
    while (a < z) { const long long md = (a + z) >> 1; if (keys[md] < lo) a = md + 1; else z = md; }
    return a;
}

// size[i] of sorted key i, 0 when -k cuts it (emitted[m] = lines of the miRNA written by earlier passes); kept[0] += lines kept
__global__ void mm_size_kernel(MmText T, const unsigned long long* __restrict__ keys, long long n, long long k, const unsigned long long* __restrict__ emitted,
                               int* __restrict__ size, unsigned long long* __restrict__ kept) {
    unsigned long long cnt = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const bool keep = k == 0 || emitted[key >> MM_SHIFT] + (unsigned long long)(i - mm_run_first(keys, i)) < (unsigned long long)k;
        size[i] = keep ? (int)mm_line<false>(T, key, nullptr) : 0;
        cnt += keep;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(kept, cnt);
}
// emitted[m] += the miRNA's keys in this pass (after mm_size_kernel)
__global__ void mm_emitted_kernel(const unsigned long long* __restrict__ keys, long long n, unsigned long long* __restrict__ emitted) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        if (i == n - 1 || (keys[i + 1] >> MM_SHIFT) != (keys[i] >> MM_SHIFT)) emitted[keys[i] >> MM_SHIFT] += (unsigned long long)(i + 1 - mm_run_first(keys, i));
}
__global__ void mm_emit_kernel(MmText T, const unsigned long long* __restrict__ keys, long long i0, long long i1, const long long* __restrict__ toff,
                               char* __restrict__ text) {
    const long long base = toff[i0];
    for (long long i = i0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < i1; i += (long long)gridDim.x * blockDim.x)
        if (toff[i + 1] != toff[i]) (void)mm_line<true>(T, keys[i], text + (toff[i] - base));
}

}  // namespace mirp

static inline int mm_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

namespace {

struct MmRun {
    mirp_ctx* c;
    mirp::TgRef R;
    mirp::MmText T;
    const MirpMimicOpts* o;
    std::vector<TgMirna>* mi;                  // the miRNAs in seed order (host); smin / smax rewritten per pass
    const std::vector<unsigned>* slot;         // file index -> place in seed order, ~0u = no usable seed
    const std::function<int(const char*, size_t)>* sink;
    long long cap, n_mi;
    long long stats[4];                        // sites written, passes, seeds looked up, bucket entries evaluated
    double sec[3];                             // scan, sort + cut, emit + download + write
    bool counted = false;                      // the first scan covers every lane and miRNA: its lookups are the stats

    void set_range(long long m, int lo, int hi) {
        const unsigned e = (*slot)[(size_t)m];
        if (e == ~0u) return;
        (*mi)[e].smin = lo;
        (*mi)[e].smax = hi;
    }

    // the sites whose interval starts in [o0, o1), with the ranges as set in *mi: keys in tg_keys; -> hits (maybe > cap).  The lane of a site at o
    // is q = o + 1 on the minus strand and q = o + L + G - 8 <= o + 30 on the plus strand.
    int scan(int mode, unsigned long long o0, unsigned long long o1, long long* hits) {
        using namespace mirp;
        const double t = mirp::now();
        hipStream_t st = c->stream;
        if (!mi->empty()) HIPCHK(c, hipMemcpyAsync(c->tg_mi.p, mi->data(), sizeof(TgMirna) * mi->size(), hipMemcpyHostToDevice, st));
        const unsigned long long p0 = o0, p1 = std::min<unsigned long long>(R.total, o1 + 30);
        unsigned long long* d_small = (unsigned long long*)c->tg_small.p;
        HIPCHK(c, hipMemsetAsync(d_small, 0, 8 * (8 + 2 * MM_STAT_SLOTS), st));
        for (unsigned long long q = p0; q < p1; q += (unsigned long long)TG_LAUNCH_POS) {
            const unsigned long long q1 = std::min(p1, q + (unsigned long long)TG_LAUNCH_POS);
            const dim3 grid((unsigned)((q1 - q + 255) / 256));
            const unsigned* d_start = (const unsigned*)c->mm_start.p;
            const TgMirna* d_mi = (const TgMirna*)c->tg_mi.p;
            const unsigned* d_mid = (const unsigned*)c->mm_mid.p;
            unsigned long long* d_keys = (unsigned long long*)c->tg_keys.p;
            unsigned long long* d_hist = (unsigned long long*)c->tg_hist.p;
            const unsigned G = (unsigned)o->loop_len;
            if (mode == 0 && o->both_strands) hipLaunchKernelGGL((mm_scan_kernel<0, true>), grid, dim3(256), 0, st, R, d_start, d_mi, d_mid, G, q, q1, o0, o1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (mode == 0) hipLaunchKernelGGL((mm_scan_kernel<0, false>), grid, dim3(256), 0, st, R, d_start, d_mi, d_mid, G, q, q1, o0, o1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (o->both_strands) hipLaunchKernelGGL((mm_scan_kernel<1, true>), grid, dim3(256), 0, st, R, d_start, d_mi, d_mid, G, q, q1, o0, o1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else hipLaunchKernelGGL((mm_scan_kernel<1, false>), grid, dim3(256), 0, st, R, d_start, d_mi, d_mid, G, q, q1, o0, o1, d_keys, (unsigned long long)cap, d_small, d_hist);
        }
        unsigned long long h[8 + 2 * MM_STAT_SLOTS];
        HIPCHK(c, hipMemcpyAsync(h, d_small, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        *hits = (long long)h[0];
        if (!counted) {
            for (int k = 0; k < MM_STAT_SLOTS; k++) { stats[2] += (long long)h[8 + 2 * k]; stats[3] += (long long)h[9 + 2 * k]; }
            counted = true;
        }
        sec[0] += mirp::now() - t;
        return 0;
    }

    // sort, cut and write the n <= cap keys of the last scan
    int finish(long long n) {
        using namespace mirp;
        hipStream_t st = c->stream;
        stats[1]++;
        if (n == 0) return 0;
        double t = mirp::now();
        unsigned long long* d_keys = (unsigned long long*)c->tg_keys.p;
        int mbits = 0;                                         // the key's bits above the miRNA index are 0
        while ((1ll << mbits) < n_mi) mbits++;
        if (int rc = mirp_device_sort_u64(c, d_keys, (unsigned long long*)c->tg_ktmp.p, n, 0, (MM_SHIFT + mbits + 7) / 8 * 8)) return rc;
        unsigned long long* d_small = (unsigned long long*)c->tg_small.p;
        long long* d_toff = (long long*)c->tg_toff.p;
        HIPCHK(c, hipMemsetAsync(d_small + 1, 0, 8, st));
        hipLaunchKernelGGL(mm_size_kernel, dim3(mm_grid(n)), dim3(256), 0, st, T, (const unsigned long long*)d_keys, n, (long long)o->max_sites,
                           (const unsigned long long*)c->tg_emitted.p, (int*)c->tg_size.p, d_small + 1);
        hipLaunchKernelGGL(mm_emitted_kernel, dim3(mm_grid(n)), dim3(256), 0, st, (const unsigned long long*)d_keys, n, (unsigned long long*)c->tg_emitted.p);
        launch_excl_scan(st, (const int*)c->tg_size.p, d_toff, n);
        long long bytes = 0;
        unsigned long long kept = 0;
        HIPCHK(c, hipMemcpyAsync(&bytes, d_toff + n, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&kept, d_small + 1, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        stats[0] += (long long)kept;
        sec[1] += mirp::now() - t;
        t = mirp::now();
        // pieces of at most 1 GiB of text (at least one line each)
        const long long piece = 1ll << 30;
        for (long long i0 = 0; i0 < n;) {
            long long base = 0;
            HIPCHK(c, hipMemcpy(&base, d_toff + i0, 8, hipMemcpyDeviceToHost));
            long long i1 = n, end = bytes;
            if (bytes - base > piece) {                        // the last i1 in [i0 + 1, n) with toff[i1] - base <= piece
                long long a = i0 + 1, z = n - 1;
                while (a < z) {
                    const long long md = (a + z + 1) >> 1;
                    long long v = 0;
                    HIPCHK(c, hipMemcpy(&v, d_toff + md, 8, hipMemcpyDeviceToHost));
                    if (v - base <= piece) a = md; else z = md - 1;
                }
                i1 = a;
                HIPCHK(c, hipMemcpy(&end, d_toff + i1, 8, hipMemcpyDeviceToHost));
            }
            const long long len = end - base;
            if (len > 0) {
                if (c->tg_text.ensure((size_t)len + 16)) return fail(c, -6, "device allocation failed (mimics: text)");
                hipLaunchKernelGGL(mm_emit_kernel, dim3(mm_grid(i1 - i0)), dim3(256), 0, st, T, (const unsigned long long*)d_keys, i0, i1, (const long long*)d_toff,
                                   (char*)c->tg_text.p);
                HIPCHK(c, hipStreamSynchronize(st));
                HIPCHK(c, hipGetLastError());
                if (c->h_text.size() < (size_t)len) c->h_text.resize((size_t)len);
                HIPCHK(c, hipMemcpy(c->h_text.data(), c->tg_text.p, (size_t)len, hipMemcpyDeviceToHost));
                if (int rc = (*sink)(c->h_text.data(), (size_t)len)) return rc;
            }
            i0 = i1;
        }
        sec[2] += mirp::now() - t;
        return 0;
    }

    int run() {
        using namespace mirp;
        hipStream_t st = c->stream;
        const int nmax = o->max_imperfect;
        const unsigned long long total = R.total;
        HIPCHK(c, hipMemsetAsync(c->tg_emitted.p, 0, 8 * (size_t)n_mi, st));
        for (long long m = 0; m < n_mi; m++) set_range(m, 0, nmax);
        long long hits = 0;
        if (int rc = scan(0, 0, total, &hits)) return rc;
        if (hits <= cap) return finish(hits);
        // overflow: hits per (miRNA, imperfect), then passes of at most cap keys in output order
        HIPCHK(c, hipMemsetAsync(c->tg_hist.p, 0, 8 * (size_t)n_mi * MM_NBIN, st));
        if (int rc = scan(1, 0, total, &hits)) return rc;
        std::vector<unsigned long long> hist((size_t)n_mi * MM_NBIN);
        HIPCHK(c, hipMemcpy(hist.data(), c->tg_hist.p, 8 * hist.size(), hipMemcpyDeviceToHost));
        std::vector<signed char> lim((size_t)n_mi, (signed char)nmax);    // -k: no line of a miRNA past the imperfect at which its first k lines are reached
        if (o->max_sites > 0)
            for (long long m = 0; m < n_mi; m++) {
                unsigned long long cum = 0;
                for (int h = 0; h <= nmax; h++) {
                    cum += hist[(size_t)m * MM_NBIN + h];
                    if (cum >= (unsigned long long)o->max_sites) { lim[(size_t)m] = (signed char)h; break; }
                }
            }
        for (long long m = 0; m < n_mi; m++) set_range(m, 1, 0);          // a pass opens the ranges of its miRNAs and closes them again
        const auto count = [&](long long i) { return (int)(i % MM_NBIN) <= lim[(size_t)(i / MM_NBIN)] ? (long long)hist[(size_t)i] : 0ll; };
        const auto flush = [&](long long first, long long last, long long expected) -> int {
            const long long ma = first / MM_NBIN, mb = last / MM_NBIN;
            const int ha = (int)(first % MM_NBIN), hb = (int)(last % MM_NBIN);
            for (long long m = ma; m <= mb; m++) set_range(m, m == ma ? ha : 0, m == mb ? hb : lim[(size_t)m]);
            long long got = 0;
            int rc = scan(0, 0, total, &got);
            for (long long m = ma; m <= mb; m++) set_range(m, 1, 0);
            if (rc) return rc;
            if (got != expected) return fail(c, -5, "mimics: a pass found a different number of sites than counted");
            return finish(got);
        };
        const auto range = [&](long long bin, unsigned long long p, unsigned long long p1, long long* got) -> int {
            const long long m = bin / MM_NBIN;
            const int h = (int)(bin % MM_NBIN);
            set_range(m, h, h);
            const int rc = scan(0, p, p1, got);
            set_range(m, 1, 0);
            if (rc) return rc;
            return *got > cap ? 0 : finish(*got);
        };
        const int rc = plan_passes(n_mi * MM_NBIN, count, cap, total, flush, range);
        return rc == PLAN_POSITION_OVER_CAP ? fail(c, -5, "mimics: one position holds more sites of one miRNA and imperfect count than a pass") : rc;
    }
};

}  // namespace

// Uploads the packed targets, the miRNAs in seed order and the start table and runs the search; the TSV lines (no header) go to `sink`.  pk, amb,
// cst: as for mirp_device_target_scan; mi / mid: the miRNAs with a usable seed in seed order and their file indices; slot: the inverse (~0u = no
// usable seed); start: 16,385 entries; mcodes (32 per miRNA), mlens, mnames, mnoff: every miRNA in file order.  stats = {sites written, passes,
// seeds looked up, bucket entries evaluated}; seconds = {upload, scan, sort + cut, emit + download + write}.
int mirp_device_mimic_scan(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                           const std::vector<unsigned long long>& cstart, const std::string& tnames, const std::vector<long long>& tnoff,
                           std::vector<TgMirna>& mi, const std::vector<unsigned>& mid, const std::vector<unsigned>& slot, const std::vector<unsigned>& start,
                           const std::vector<unsigned char>& mcodes, const std::vector<int>& mlens, const std::string& mnames, const std::vector<long long>& mnoff,
                           const MirpMimicOpts& o, const std::function<int(const char*, size_t)>& sink, long long stats[4], double seconds[4]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long n_mi = (long long)mlens.size();
    const long long cap = c->tg_cap > 0 ? c->tg_cap : (1ll << 26);
    double t = mirp::now();
    if (c->tg_names.ensure(tnames.size() + 1) || c->tg_noff.ensure(8 * tnoff.size()) || c->tg_mcodes.ensure(mcodes.size() + 32) ||
        c->tg_mnames.ensure(mnames.size() + 1) || c->tg_mnoff.ensure(8 * mnoff.size()) || c->tg_mi.ensure(sizeof(TgMirna) * (mi.size() + 1)) ||
        c->mm_mid.ensure(4 * (mid.size() + 1)) || c->mm_len.ensure(4 * (size_t)(n_mi + 1)) || c->mm_start.ensure(4 * start.size()) ||
        c->tg_emitted.ensure(8 * (size_t)(n_mi + 1)) || c->tg_hist.ensure(8 * (size_t)(n_mi + 1) * MM_NBIN) || c->tg_small.ensure(8 * (8 + 2 * MM_STAT_SLOTS)) ||
        c->tg_keys.ensure(8 * (size_t)cap) || c->tg_ktmp.ensure(8 * (size_t)cap) || c->tg_size.ensure(4 * (size_t)cap) || c->tg_toff.ensure(8 * (size_t)(cap + 1)))
        return fail(c, -6, "device allocation failed (mimics)");
    MmRun run;
    if (int rc = tg_upload_packed(c, pk, amb, cst, total, cstart, &run.R)) return rc;
    if (!tnames.empty()) HIPCHK(c, hipMemcpyAsync(c->tg_names.p, tnames.data(), tnames.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->tg_noff.p, tnoff.data(), 8 * tnoff.size(), hipMemcpyHostToDevice, st));
    if (!mcodes.empty()) HIPCHK(c, hipMemcpyAsync(c->tg_mcodes.p, mcodes.data(), mcodes.size(), hipMemcpyHostToDevice, st));
    if (!mnames.empty()) HIPCHK(c, hipMemcpyAsync(c->tg_mnames.p, mnames.data(), mnames.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->tg_mnoff.p, mnoff.data(), 8 * mnoff.size(), hipMemcpyHostToDevice, st));
    if (!mid.empty()) HIPCHK(c, hipMemcpyAsync(c->mm_mid.p, mid.data(), 4 * mid.size(), hipMemcpyHostToDevice, st));
    if (n_mi) HIPCHK(c, hipMemcpyAsync(c->mm_len.p, mlens.data(), 4 * (size_t)n_mi, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->mm_start.p, start.data(), 4 * start.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] = mirp::now() - t;

    run.c = c;
    run.T = MmText{(const unsigned long long*)c->tg_pk.p, (const unsigned char*)c->tg_mcodes.p, (const int*)c->mm_len.p, (const char*)c->tg_mnames.p,
                   (const long long*)c->tg_mnoff.p, (const char*)c->tg_names.p, (const long long*)c->tg_noff.p, (const unsigned long long*)c->tg_cstart.p,
                   (int)cstart.size() - 1, o.loop_len};
    run.o = &o;
    run.mi = &mi;
    run.slot = &slot;
    run.sink = &sink;
    run.cap = cap;
    run.n_mi = n_mi;
    std::memset(run.stats, 0, sizeof run.stats);
    std::memset(run.sec, 0, sizeof run.sec);
    if (total > 0 && n_mi > 0)
        if (int rc = run.run()) return rc;
    for (int i = 0; i < 4; i++) stats[i] = run.stats[i];
    for (int i = 0; i < 3; i++) seconds[1 + i] = run.sec[i];
    return 0;
}
