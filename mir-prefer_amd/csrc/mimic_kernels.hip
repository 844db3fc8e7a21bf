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
//   order, cut, emit   site_finish_pass (site_lines.h) with the line MmLine: the sort by the whole key gives miRNA (file order), imperfect, target,
//          start, + before -; -k cuts by the rank inside the miRNA's run plus what earlier passes emitted.
// Passes of at most `cap` keys are planned by site_plan_passes (site_lines.h) with (miRNA, imperfect) as the bins and the interval
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
#include "site_lines.h"
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

// One line: miRNA target start end strand imperfect mismatches gu mirna_5to3 pairs target_3to5 loop.  Column c = 1 .. L + G of the three aligned
// strings holds miRNA position c (c <= P), nothing (the G loop bases) or position c - G, over the target-strand base of the column.
struct MmLine {
    MmText T;
    static constexpr int shift = MM_SHIFT;
    template <bool WRITE>
    __device__ long long line(unsigned long long key, long long, char* out) const {
        TextOut<WRITE> o{out};
        const long long m = (long long)(key >> MM_SHIFT);
        const unsigned imp = (unsigned)(key >> 35) & 7u;
        const unsigned long long g = (key >> 3) & 0xffffffffull;
        const int strand = (int)(key >> 2) & 1, P = 9 + (int)(key & 3), G = T.G;
        const int W = T.mlen[m] + G;
        const int a = site_contig(T.cstart, T.n_contigs, g);
        text_site_head(o, T.mnames, T.mnoff, m, T.tnames, T.tnoff, a, g - T.cstart[a] + 1, g - T.cstart[a] + W, strand);
        o.ch('\t');
        o.num(imp);
        o.ch('\t');
        const auto pos = [&](int c) { return c <= P ? c : c <= P + G ? 0 : c - G; };
        const auto base = [&](int c) -> int {
            const unsigned b = tg_base(T.pk, strand ? g + c - 1 : g + W - c);
            return (int)(strand ? 3u - b : b);
        };
        text_site_pairing(o, T.mcodes + 32 * m, W, pos, base);
        o.ch('\t');
        o.num((unsigned long long)P);
        o.ch('\n');
        return o.n;
    }
};

}  // namespace mirp

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

    int run() {
        using namespace mirp;
        hipStream_t st = c->stream;
        const int nmax = o->max_imperfect;
        const unsigned long long total = R.total;
        HIPCHK(c, hipMemsetAsync(c->tg_emitted.p, 0, 8 * (size_t)n_mi, st));
        for (long long m = 0; m < n_mi; m++) set_range(m, 0, nmax);
        long long hits = 0;
        if (int rc = scan(0, 0, total, &hits)) return rc;
        int mbits = 0;                                         // the key's bits above the miRNA index are 0
        while ((1ll << mbits) < n_mi) mbits++;
        const auto write_pass = [&](long long n) {
            return site_finish_pass(c, MmLine{T}, n, MM_SHIFT + mbits, (long long)o->max_sites, *sink, "mimics", stats, sec);
        };
        if (hits <= cap) return write_pass(hits);
        // overflow: passes of at most cap keys in output order, with (miRNA, imperfect) as the bins and the interval starts as the positions; a
        // scan takes every miRNA whose range is open
        return site_plan_passes(
            c, n_mi, MM_NBIN, nmax, (long long)o->max_sites, cap, total, "mimics",
            "mimics: one position holds more sites of one miRNA and imperfect count than a pass", [&](long long m, int lo, int hi) { set_range(m, lo, hi); },
            [&](int mode, long long, long long, unsigned long long p0, unsigned long long p1, long long* got) { return scan(mode, p0, p1, got); }, write_pass);
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
