// Device side of the plant miRNA target-site search (mirp_target_scan, mirp_targets.cpp), with the semantics of DESIGN.md §14.
//
// Targets (uploaded once per call): pk as 64-bit words of 32 2-bit bases (base i at bits 2 (i % 32)), amb / cst bitmaps as in align_kernels.hip
// (amb also set on every position past the end), the contigs' first positions and names.  Positions are global over the targets in file order.
//
// miRNAs: one TgMirna per miRNA, built on the host (mirp_targets.cpp).  Window position j of a lane at offset o is the forward base t[o + j];
// miRNA position i pairs with j = L - i on the plus strand and j = i - 1 on the minus strand.  Every mask is a 32-bit mask over j, and the
// Watson-Crick target bases are held as two bit planes (low and high bit of the 2-bit code), so one (position, miRNA, strand) evaluation is
//     nonwc = ((wl ^ pl) | (wh ^ ph) | unk) & lmask            bases that are not Watson-Crick pairs (an unknown miRNA letter never is)
//     gu    = (isX & g1) | (isY & g2)                          G:U pairs: X = T, Y = G on the plus strand, X = A, Y = C on the minus strand
//     mm    = nonwc & ~gu
//     half  = popc(nonwc) + popc(mm) + popc(nonwc & seed) + popc(mm & seed)      the score in half-units: mismatch 2, G:U 1, doubled in the seed
// and the site is a hit when smin <= half <= smax, mm & cleave == 0 and L <= stop, stop = the distance to the first ambiguous base or to the next
// contig start (per lane, computed once).  The packed-target types, the evaluation and the scan kernel are in targets_device.h, which the degradome
// scan (degradome_kernels.hip) shares.
//
//   scan   tg_scan_kernel<0>: one lane per target offset, miRNAs of the pass in wave-uniform (scalar) loads; every hit appends the key
//          mloc << 38 | half << 33 | o << 1 | strand (mloc = the miRNA's index in its group of <= 2^16) to a buffer of `cap` keys and counts it.
//          tg_scan_kernel<1>: the same scan counting hits per (miRNA, half-score) only, run when a pass's hits overflow the buffer: the counts go
//          to site_plan_passes (site_lines.h) with (miRNA, half-score) as the bins and the target offsets as the positions.
//   order, cut, emit   site_finish_pass (site_lines.h) with the line TgLine<false>: the sort by the whole key gives, per miRNA, (score, target,
//          start, + before -) = the output order; -k cuts by the rank inside the miRNA's run plus what earlier passes emitted.
// With --bulge the scan is tg_bulge_scan_kernel (targets_bulge_device.h), which also finds the sites with one unpaired base; its keys are
// mloc << 45 | half << 40 | start << 8 | strand << 7 | kind << 5 | P, again in output order, and the line is TgLine<true>.
// With --energy the sorted keys of a pass are folded (duplex_kernels.hip) before the cut measures the lines, and every line gains
// the columns mfe, mfe_perfect, mfe_ratio and duplex; without it TgText's energy pointers are null and the lines are as before.
// With --accessibility the windows of the sorted keys are folded as well (unpaired_kernels.hip) and every line gains the column upe.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "site_lines.h"
#include "text_out.h"

namespace mirp {

// ---------------------------------------------------------------- text
struct TgText {
    const unsigned long long* pk;
    const unsigned char* mcodes;            // 32 per miRNA: 0..3 = A C G U, 4 = unknown
    const TgMirna* mi;                      // the group's miRNAs (L)
    const char* mnames; const long long* mnoff;
    const char* tnames; const long long* tnoff;
    const unsigned long long* cstart; int n_contigs;
    int mbase;                              // the group's first miRNA
    // --energy, else null: the ambiguity bitmap, the fold of every sorted key of the pass (duplex_kernels.hip: mfe and the masks of
    // the paired positions of the miRNA and of the target strand) and the perfect duplex of every miRNA of the group
    const unsigned* amb;
    const int* e_mfe; const unsigned long long* e_ma; const unsigned long long* e_mb;
    const int* e_perf;
    // --accessibility, else null: upe x 1000, rounded, of every sorted key of the pass (unpaired_kernels.hip)
    const int* upe;
};

// the four last columns of an --energy line: mfe, mfe_perfect, mfe_ratio (half up to three decimals; NA when the perfect duplex is unbound) and the
// structure text of the miRNA (L nt) and the target strand (nb nt: the interval and its flanks)
template <bool WRITE>
__device__ void tg_energy_cols(TextOut<WRITE>& o, const TgText& T, long long idx, int mloc, int L, int nb) {
    const int e = T.e_mfe[idx], pe = T.e_perf[mloc];
    const int v[2] = {-e, -pe};
    for (int x = 0; x < 2; x++) {
        o.ch('\t');
        if (v[x] > 0) o.ch('-');
        o.num((unsigned long long)(v[x] / 100));
        o.ch('.');
        o.ch((char)('0' + v[x] / 10 % 10));
        o.ch((char)('0' + v[x] % 10));
    }
    o.ch('\t');
    if (pe == 0) { o.ch('N'); o.ch('A'); }
    else {
        const long long q = (2000ll * -e + -pe) / (2ll * -pe);
        o.num((unsigned long long)(q / 1000));
        o.ch('.');
        o.ch((char)('0' + q / 100 % 10));
        o.ch((char)('0' + q / 10 % 10));
        o.ch((char)('0' + q % 10));
    }
    o.ch('\t');
    const unsigned long long ma = T.e_ma[idx], mb = T.e_mb[idx];
    for (int i = 0; i < L; i++) o.ch((ma >> i) & 1 ? '(' : '.');
    o.ch('&');
    for (int j = 0; j < nb; j++) o.ch((mb >> j) & 1 ? ')' : '.');
}

// the last column of an --accessibility line: upe in kcal/mol to three decimals
template <bool WRITE>
__device__ void tg_upe_col(TextOut<WRITE>& o, const TgText& T, long long idx) {
    const int v = T.upe[idx];
    o.ch('\t');
    o.num((unsigned long long)(v / 1000));
    o.ch('.');
    o.ch((char)('0' + v / 100 % 10));
    o.ch((char)('0' + v / 10 % 10));
    o.ch((char)('0' + v % 10));
}

// One line: miRNA target start end strand score mismatches gu mirna_5to3 pairs target_3to5, with --bulge the bulge column (. / tP / mP), then the
// columns of --energy and --accessibility (idx: the key's index in the pass).  Column c of the three aligned strings holds miRNA position i(c) and
// the target base q(c); the t site has one column more (the unpaired target base under a '-'), the m site a '-' under miRNA position P.
template <bool BULGE>
struct TgLine {
    TgText T;
    static constexpr int shift = SiteKey<BULGE>::shift;
    template <bool WRITE>
    __device__ long long line(unsigned long long key, long long idx, char* out) const {
        TextOut<WRITE> o{out};
        const SiteKey<BULGE> K(key);
        const unsigned long long g = K.g;
        const int strand = K.strand, kind = K.kind, P = K.P;
        const long long m = (long long)T.mbase + K.mloc;
        const int L = T.mi[K.mloc].L, len = K.len(L);
        const int a = site_contig(T.cstart, T.n_contigs, g);
        text_site_head(o, T.mnames, T.mnoff, m, T.tnames, T.tnoff, a, g - T.cstart[a] + 1, g - T.cstart[a] + len, strand);
        o.ch('\t');
        o.num(K.half >> 1);
        o.ch('.');
        o.ch(K.half & 1 ? '5' : '0');
        o.ch('\t');
        // column c = 1 .. W: the miRNA position (0 = none) and the target-strand base (-1 = none)
        const auto pos = [&](int c) { return kind != 2 || c <= P ? c : c == P + 1 ? 0 : c - 1; };
        const auto base = [&](int c) -> int {
            unsigned long long q;
            if (kind == 2) q = strand ? g + c - 1 : g + L + 1 - c;
            else if (kind == 1) q = strand ? g + c - 1 : g + L - c;
            else if (c == P) return -1;
            else if (c < P) q = strand ? g + c - 1 : g + L - 1 - c;
            else q = strand ? g + c - 2 : g + L - c;
            const unsigned b = tg_base(T.pk, q);
            return (int)(strand ? 3u - b : b);
        };
        text_site_pairing(o, T.mcodes + 32 * m, L + (kind == 2), pos, base);
        if (BULGE) {
            o.ch('\t');
            if (kind == 1) o.ch('.');
            else { o.ch(kind == 2 ? 't' : 'm'); o.num((unsigned long long)P); }
        }
        if (T.e_mfe) tg_energy_cols(o, T, idx, K.mloc, L, len + (g > T.cstart[a]) + (g + len < T.cstart[a + 1]));
        if (T.upe) tg_upe_col(o, T, idx);
        o.ch('\n');
        return o.n;
    }
};

}  // namespace mirp

namespace {

struct TgRun {
    mirp_ctx* c;
    mirp::TgRef R;
    mirp::TgText T;
    const MirpTargetOpts* o;
    std::vector<TgMirna>* mi;                  // all miRNAs (host); smin / smax rewritten per pass
    const std::function<int(const char*, size_t)>* sink;
    long long cap;
    int group_n = 0;                           // miRNAs in the current group
    long long stats[2];                        // sites written, passes
    double sec[3];                             // scan, sort + cut, emit + download + write

    // scan miRNAs [a, b) of the group at mbase (their smin / smax as set in *mi) over offsets [p0, p1): keys in tg_keys; -> hits (maybe > cap)
    int scan(int mode, int mbase, int a, int b, unsigned long long p0, unsigned long long p1, long long* hits) {
        using namespace mirp;
        const double t = mirp::now();
        hipStream_t st = c->stream;
        const int n = b - a;
        HIPCHK(c, hipMemcpyAsync((TgMirna*)c->tg_mi.p + a, mi->data() + mbase + a, sizeof(TgMirna) * (size_t)n, hipMemcpyHostToDevice, st));
        unsigned long long* d_small = (unsigned long long*)c->tg_small.p;
        HIPCHK(c, hipMemsetAsync(d_small, 0, 8, st));
        for (unsigned long long q = p0; q < p1; q += (unsigned long long)TG_LAUNCH_POS) {
            const unsigned long long q1 = std::min(p1, q + (unsigned long long)TG_LAUNCH_POS);
            const dim3 grid((unsigned)((q1 - q + 255) / 256));
            const TgMirna* d_mi = (const TgMirna*)c->tg_mi.p;
            unsigned long long* d_keys = (unsigned long long*)c->tg_keys.p;
            unsigned long long* d_hist = (unsigned long long*)c->tg_hist.p;
            if (o->bulge && mode == 0 && o->both_strands) hipLaunchKernelGGL((tg_bulge_scan_kernel<0, true>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (o->bulge && mode == 0) hipLaunchKernelGGL((tg_bulge_scan_kernel<0, false>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (o->bulge && o->both_strands) hipLaunchKernelGGL((tg_bulge_scan_kernel<1, true>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (o->bulge) hipLaunchKernelGGL((tg_bulge_scan_kernel<1, false>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (mode == 0 && o->both_strands) hipLaunchKernelGGL((tg_scan_kernel<0, true>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (mode == 0) hipLaunchKernelGGL((tg_scan_kernel<0, false>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else if (o->both_strands) hipLaunchKernelGGL((tg_scan_kernel<1, true>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
            else hipLaunchKernelGGL((tg_scan_kernel<1, false>), grid, dim3(256), 0, st, R, d_mi, a, b, q, q1, d_keys, (unsigned long long)cap, d_small, d_hist);
        }
        unsigned long long h = 0;
        HIPCHK(c, hipMemcpyAsync(&h, d_small, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        *hits = (long long)h;
        sec[0] += mirp::now() - t;
        return 0;
    }

    // sort, cut and write the n <= cap keys of the last scan.  With --energy / --accessibility the sorted keys that -k keeps are folded before the
    // lines are measured: the widths of `mfe` and `upe` are part of a line's length.
    template <bool BULGE>
    int write_pass(int mbase, long long n) {
        using namespace mirp;
        T.mbase = mbase;
        int mbits = 0;                                         // the key's bits above the miRNA index are 0
        while ((1 << mbits) < group_n) mbits++;
        const auto folds = [&](const unsigned long long* d_keys, long long n) -> int {
            const DxTargets D{T.pk, (const unsigned*)c->tg_amb.p, T.mcodes, T.mi, T.cstart, T.n_contigs, mbase};
            const unsigned long long* d_emitted = (const unsigned long long*)c->tg_emitted.p;
            if (o->energy)
                if (int rc = mirp_device_duplex_sites(c, D, BULGE, d_keys, n, (long long)o->max_sites, d_emitted, (int*)c->tg_emfe.p,
                                                      (unsigned long long*)c->tg_ema.p, (unsigned long long*)c->tg_emb.p))
                    return rc;
            if (o->accessibility) {
                int longest = 0;                               // the group's longest interval sizes the launch's tables
                for (int m = 0; m < group_n; m++) longest = std::max(longest, (int)(*mi)[(size_t)(mbase + m)].L + (BULGE ? 1 : 0));
                if (int rc = mirp_device_unpaired_sites(c, D, BULGE, d_keys, n, (long long)o->max_sites, d_emitted, longest, c->tg_up, c->tg_down,
                                                        (int*)c->tg_upe.p))
                    return rc;
            }
            return 0;
        };
        return site_finish_pass(c, TgLine<BULGE>{T}, n, TgLine<BULGE>::shift + mbits, (long long)o->max_sites, *sink, "targets", stats, sec, folds);
    }
    int write_pass(int mbase, long long n) { return o->bulge ? write_pass<true>(mbase, n) : write_pass<false>(mbase, n); }

    void set_range(int mbase, int m, int smin, int smax) {
        TgMirna& x = (*mi)[(size_t)(mbase + m)];
        x.smin = smin;
        x.smax = smax;
    }

    // one group of miRNAs [mbase, mbase + n)
    int group(int mbase, int n) {
        using namespace mirp;
        hipStream_t st = c->stream;
        const int smax = o->max_half_score;
        const unsigned long long total = R.total;
        group_n = n;
        HIPCHK(c, hipMemsetAsync(c->tg_emitted.p, 0, 8 * (size_t)n, st));
        for (int m = 0; m < n; m++) set_range(mbase, m, 0, smax);
        long long hits = 0;
        if (int rc = scan(0, mbase, 0, n, 0, total, &hits)) return rc;
        if (o->energy) {                                       // mfe_perfect, once per miRNA (the scan has uploaded the group's TgMirna)
            const double t = mirp::now();
            if (int rc = mirp_device_duplex_perfect(c, (const unsigned char*)c->tg_mcodes.p + 32 * (size_t)mbase, (const TgMirna*)c->tg_mi.p, n, (int*)c->tg_perf.p,
                                                    nullptr, nullptr))
                return rc;
            HIPCHK(c, hipStreamSynchronize(st));
            sec[1] += mirp::now() - t;
        }
        if (hits <= cap) return write_pass(mbase, hits);
        // overflow: passes of at most cap keys in output order, with (miRNA, half-score) as the bins and the target offsets as the positions
        return site_plan_passes(
            c, n, TG_NHALF, smax, (long long)o->max_sites, cap, total, "targets", "targets: one offset holds more sites of one miRNA and score than a pass",
            [&](long long m, int lo, int hi) { set_range(mbase, (int)m, lo, hi); },
            [&](int mode, long long ma, long long mb, unsigned long long p0, unsigned long long p1, long long* got) {
                return scan(mode, mbase, (int)ma, (int)mb + 1, p0, p1, got);
            },
            [&](long long got) { return write_pass(mbase, got); });
    }
};

}  // namespace

// Uploads the packed targets and runs the search for every miRNA; the TSV lines (no header) go to `sink`.  pk: (total + 31) / 32 + 2 u64 words;
// amb / cst: (total + 31) / 32 + 2 words; mcodes: 32 per miRNA.  stats = {sites written, passes}; seconds = {upload, scan, sort + cut,
// emit + download + write}.
int mirp_device_target_scan(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                            const std::vector<unsigned long long>& cstart, const std::string& tnames, const std::vector<long long>& tnoff,
                            std::vector<TgMirna>& mi, const std::vector<unsigned char>& mcodes, const std::string& mnames, const std::vector<long long>& mnoff,
                            const MirpTargetOpts& o, const std::function<int(const char*, size_t)>& sink, long long stats[2], double seconds[4]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long n_mi = (long long)mi.size();
    long long cap = c->tg_cap > 0 ? c->tg_cap : (1ll << 26);
    if (o.bulge && cap < 4) cap = 4;            // one offset can hold 4 sites of one (miRNA, score): t and m on both strands (an ungapped site of
                                                // that score dominates both); without bulge it holds 2, the smallest capacity the ABI takes
    double t = mirp::now();
    if (c->tg_names.ensure(tnames.size() + 1) || c->tg_noff.ensure(8 * tnoff.size()) || c->tg_mcodes.ensure(mcodes.size() + 32) ||
        c->tg_mnames.ensure(mnames.size() + 1) || c->tg_mnoff.ensure(8 * mnoff.size()) || c->tg_mi.ensure(sizeof(TgMirna) * TG_GROUP) ||
        c->tg_emitted.ensure(8 * (size_t)TG_GROUP) || c->tg_hist.ensure(8 * (size_t)TG_GROUP * TG_NHALF) || c->tg_small.ensure(64) ||
        c->tg_keys.ensure(8 * (size_t)cap) || c->tg_ktmp.ensure(8 * (size_t)cap) || c->tg_size.ensure(4 * (size_t)cap) || c->tg_toff.ensure(8 * (size_t)(cap + 1)))
        return fail(c, -6, "device allocation failed (targets)");
    if (o.energy && (c->tg_emfe.ensure(4 * (size_t)cap) || c->tg_ema.ensure(8 * (size_t)cap) || c->tg_emb.ensure(8 * (size_t)cap) ||
                     c->tg_perf.ensure(4 * (size_t)TG_GROUP)))
        return fail(c, -6, "device allocation failed (targets: energies)");
    if (o.accessibility && c->tg_upe.ensure(4 * (size_t)cap)) return fail(c, -6, "device allocation failed (targets: accessibility)");
    TgRun run;
    if (int rc = tg_upload_packed(c, pk, amb, cst, total, cstart, &run.R)) return rc;
    if (!tnames.empty()) HIPCHK(c, hipMemcpyAsync(c->tg_names.p, tnames.data(), tnames.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->tg_noff.p, tnoff.data(), 8 * tnoff.size(), hipMemcpyHostToDevice, st));
    if (!mcodes.empty()) HIPCHK(c, hipMemcpyAsync(c->tg_mcodes.p, mcodes.data(), mcodes.size(), hipMemcpyHostToDevice, st));
    if (!mnames.empty()) HIPCHK(c, hipMemcpyAsync(c->tg_mnames.p, mnames.data(), mnames.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->tg_mnoff.p, mnoff.data(), 8 * mnoff.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    seconds[0] = mirp::now() - t;

    run.c = c;
    run.T = TgText{(const unsigned long long*)c->tg_pk.p, (const unsigned char*)c->tg_mcodes.p, (const TgMirna*)c->tg_mi.p, (const char*)c->tg_mnames.p,
                   (const long long*)c->tg_mnoff.p, (const char*)c->tg_names.p, (const long long*)c->tg_noff.p, (const unsigned long long*)c->tg_cstart.p,
                   (int)cstart.size() - 1, 0};
    if (o.energy) {
        run.T.amb = (const unsigned*)c->tg_amb.p;
        run.T.e_mfe = (const int*)c->tg_emfe.p;
        run.T.e_ma = (const unsigned long long*)c->tg_ema.p;
        run.T.e_mb = (const unsigned long long*)c->tg_emb.p;
        run.T.e_perf = (const int*)c->tg_perf.p;
    }
    if (o.accessibility) run.T.upe = (const int*)c->tg_upe.p;
    run.o = &o;
    run.mi = &mi;
    run.sink = &sink;
    run.cap = cap;
    std::memset(run.stats, 0, sizeof run.stats);
    std::memset(run.sec, 0, sizeof run.sec);
    if (total > 0)
        for (long long m0 = 0; m0 < n_mi; m0 += TG_GROUP)
            if (int rc = run.group((int)m0, (int)std::min<long long>(TG_GROUP, n_mi - m0))) return rc;
    for (int i = 0; i < 2; i++) stats[i] = run.stats[i];
    for (int i = 0; i < 3; i++) seconds[1 + i] = run.sec[i];
    return 0;
}
