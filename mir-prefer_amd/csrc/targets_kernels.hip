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
//          to plan_passes (pass_plan.h) with (miRNA, half-score) as the bins and the target offsets as the positions.
//   order  mirp_device_sort_u64 by the whole key: per miRNA, (score, target, start, + before -) = the output order.
//   cut    tg_size_kernel: -k from the rank inside the miRNA's run plus what earlier passes emitted; the line's length; launch_excl_scan.
//   emit   tg_emit_kernel writes the lines; the text goes to the sink in pieces of at most 1 GiB.
// With --bulge the scan is tg_bulge_scan_kernel (targets_bulge_device.h), which also finds the sites with one unpaired base; its keys are
// mloc << 45 | half << 40 | start << 8 | strand << 7 | kind << 5 | P, again in output order, and order, cut and emit run as their <true> instances.
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
#include "pass_plan.h"
#include "targets_bulge_device.h"
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

// pair class of miRNA code mc (0..3 A C G U, 4 unknown) with target-strand base y (0..3 A C G U): 0 Watson-Crick, 1 G:U, 2 mismatch
__device__ __forceinline__ int tg_class(unsigned mc, unsigned y) {
    if (mc > 3) return 2;
    if (mc + y == 3) return 0;
    return (mc == 2 && y == 3) || (mc == 3 && y == 2) ? 1 : 2;
}

// one line: miRNA target start end strand score mismatches gu mirna_5to3 pairs target_3to5 (idx: the key's index in the pass, for --energy)
template <bool WRITE>
__device__ long long tg_line(const TgText& T, unsigned long long key, long long idx, char* out) {
    TextOut<WRITE> o{out};
    const int mloc = (int)(key >> 38);
    const unsigned half = (unsigned)(key >> 33) & 31u;
    const unsigned long long g = (key >> 1) & 0xffffffffull;
    const int strand = (int)(key & 1);
    const long long m = (long long)T.mbase + mloc;
    const int L = T.mi[mloc].L;
    const unsigned char* mc = T.mcodes + 32 * m;
    int a = 0, z = T.n_contigs;                 // target: last cstart <= g
    while (z - a > 1) { const int md = (a + z) >> 1; if (T.cstart[md] <= g) a = md; else z = md; }
    int nmm = 0, ngu = 0;
    for (int i = 1; i <= L; i++) {
        const unsigned b = tg_base(T.pk, strand ? g + i - 1 : g + L - i);
        const int k = tg_class(mc[i - 1], strand ? 3u - b : b);
        nmm += k == 2;
        ngu += k == 1;
    }
    o.str(T.mnames + T.mnoff[m], T.mnoff[m + 1] - T.mnoff[m]);
    o.ch('\t');
    o.str(T.tnames + T.tnoff[a], T.tnoff[a + 1] - T.tnoff[a]);
    o.ch('\t');
    o.num(g - T.cstart[a] + 1);
    o.ch('\t');
    o.num(g - T.cstart[a] + L);
    o.ch('\t');
    o.ch(strand ? '-' : '+');
    o.ch('\t');
    o.num(half >> 1);
    o.ch('.');
    o.ch(half & 1 ? '5' : '0');
    o.ch('\t');
    o.num((unsigned long long)nmm);
    o.ch('\t');
    o.num((unsigned long long)ngu);
    o.ch('\t');
    const char* RNA = "ACGUN";
    for (int i = 0; i < L; i++) o.ch(RNA[mc[i]]);
    o.ch('\t');
    for (int i = 1; i <= L; i++) {
        const unsigned b = tg_base(T.pk, strand ? g + i - 1 : g + L - i);
        const int k = tg_class(mc[i - 1], strand ? 3u - b : b);
        o.ch(k == 0 ? '|' : k == 1 ? 'o' : 'x');
    }
    o.ch('\t');
    for (int i = 1; i <= L; i++) {
        const unsigned b = tg_base(T.pk, strand ? g + i - 1 : g + L - i);
        o.ch(RNA[strand ? 3u - b : b]);
    }
    if (T.e_mfe) tg_energy_cols(o, T, idx, mloc, L, L + (g > T.cstart[a]) + (g + L < T.cstart[a + 1]));
    if (T.upe) tg_upe_col(o, T, idx);
    o.ch('\n');
    return o.n;
}

// one line of a --bulge run: the columns of tg_line and the bulge column (. / tP / mP).  Column c of the three aligned strings holds miRNA position
// i(c) and the target base q(c); the t site has one column more (the unpaired target base under a '-'), the m site a '-' under miRNA position P.
template <bool WRITE>
__device__ long long tg_bulge_line(const TgText& T, unsigned long long key, long long idx, char* out) {
    TextOut<WRITE> o{out};
    const int mloc = (int)(key >> TG_BULGE_SHIFT);
    const unsigned half = (unsigned)(key >> 40) & 31u;
    const unsigned long long g = (key >> 8) & 0xffffffffull;
    const int strand = (int)(key >> 7) & 1, kind = (int)(key >> 5) & 3, P = (int)(key & 31);
    const long long m = (long long)T.mbase + mloc;
    const int L = T.mi[mloc].L;
    const int W = L + (kind == 2);                  // columns
    const unsigned char* mc = T.mcodes + 32 * m;
    int a = 0, z = T.n_contigs;                 // target: last cstart <= g
    while (z - a > 1) { const int md = (a + z) >> 1; if (T.cstart[md] <= g) a = md; else z = md; }
    // column c = 1 .. W: the miRNA position (0 = none) and the target-strand base (-1 = none)
    auto pos = [&](int c) { return kind != 2 || c <= P ? c : c == P + 1 ? 0 : c - 1; };
    auto base = [&](int c) -> int {
        unsigned long long q;
        if (kind == 2) q = strand ? g + c - 1 : g + L + 1 - c;
        else if (kind == 1) q = strand ? g + c - 1 : g + L - c;
        else if (c == P) return -1;
        else if (c < P) q = strand ? g + c - 1 : g + L - 1 - c;
        else q = strand ? g + c - 2 : g + L - c;
        const unsigned b = tg_base(T.pk, q);
        return (int)(strand ? 3u - b : b);
    };
    int nmm = 0, ngu = 0;
    for (int c = 1; c <= W; c++) {
        const int i = pos(c), y = base(c);
        if (i == 0 || y < 0) continue;
        const int k = tg_class(mc[i - 1], (unsigned)y);
        nmm += k == 2;
        ngu += k == 1;
    }
    o.str(T.mnames + T.mnoff[m], T.mnoff[m + 1] - T.mnoff[m]);
    o.ch('\t');
    o.str(T.tnames + T.tnoff[a], T.tnoff[a + 1] - T.tnoff[a]);
    o.ch('\t');
    o.num(g - T.cstart[a] + 1);
    o.ch('\t');
    o.num(g - T.cstart[a] + L + kind - 1);
    o.ch('\t');
    o.ch(strand ? '-' : '+');
    o.ch('\t');
    o.num(half >> 1);
    o.ch('.');
    o.ch(half & 1 ? '5' : '0');
    o.ch('\t');
    o.num((unsigned long long)nmm);
    o.ch('\t');
    o.num((unsigned long long)ngu);
    o.ch('\t');
    const char* RNA = "ACGUN";
    for (int c = 1; c <= W; c++) { const int i = pos(c); o.ch(i ? RNA[mc[i - 1]] : '-'); }
    o.ch('\t');
    for (int c = 1; c <= W; c++) {
        const int i = pos(c), y = base(c);
        const int k = i == 0 || y < 0 ? 3 : tg_class(mc[i - 1], (unsigned)y);
        o.ch(k == 0 ? '|' : k == 1 ? 'o' : k == 2 ? 'x' : '-');
    }
    o.ch('\t');
    for (int c = 1; c <= W; c++) { const int y = base(c); o.ch(y < 0 ? '-' : RNA[y]); }
    o.ch('\t');
    if (kind == 1) o.ch('.');
    else { o.ch(kind == 2 ? 't' : 'm'); o.num((unsigned long long)P); }
    if (T.e_mfe) {
        const int len = L + kind - 1;
        tg_energy_cols(o, T, idx, mloc, L, len + (g > T.cstart[a]) + (g + len < T.cstart[a + 1]));
    }
    if (T.upe) tg_upe_col(o, T, idx);
    o.ch('\n');
    return o.n;
}

// the bits of a key below the miRNA index: 38 for the ungapped scan's keys, 45 for the --bulge scan's
template <bool BULGE> struct TgKey { static constexpr int shift = BULGE ? TG_BULGE_SHIFT : 38; };

// first index of the miRNA run that holds keys[i] (the keys are sorted)
template <bool BULGE>
__device__ __forceinline__ long long tg_run_first(const unsigned long long* __restrict__ keys, long long i) {
    const unsigned long long lo = keys[i] >> TgKey<BULGE>::shift << TgKey<BULGE>::shift;
    long long a = 0, z = i;
    while (a < z) { const long long md = (a + z) >> 1; if (keys[md] < lo) a = md + 1; else z = md; }
    return a;
}

// size[i] of sorted key i, 0 when -k cuts it (emitted[mloc] = lines of the miRNA written by earlier passes); kept[0] += lines kept
template <bool BULGE>
__global__ void tg_size_kernel(TgText T, const unsigned long long* __restrict__ keys, long long n, long long k, const unsigned long long* __restrict__ emitted,
                               int* __restrict__ size, unsigned long long* __restrict__ kept) {
    unsigned long long cnt = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const bool keep = k == 0 || emitted[key >> TgKey<BULGE>::shift] + (unsigned long long)(i - tg_run_first<BULGE>(keys, i)) < (unsigned long long)k;
        size[i] = !keep ? 0 : BULGE ? (int)tg_bulge_line<false>(T, key, i, nullptr) : (int)tg_line<false>(T, key, i, nullptr);
        cnt += keep;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(kept, cnt);
}
// emitted[mloc] += the miRNA's keys in this pass (after tg_size_kernel)
template <bool BULGE>
__global__ void tg_emitted_kernel(const unsigned long long* __restrict__ keys, long long n, unsigned long long* __restrict__ emitted) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        if (i == n - 1 || (keys[i + 1] >> TgKey<BULGE>::shift) != (keys[i] >> TgKey<BULGE>::shift))
            emitted[keys[i] >> TgKey<BULGE>::shift] += (unsigned long long)(i + 1 - tg_run_first<BULGE>(keys, i));
}
template <bool BULGE>
__global__ void tg_emit_kernel(TgText T, const unsigned long long* __restrict__ keys, long long i0, long long i1, const long long* __restrict__ toff,
                               char* __restrict__ text) {
    const long long base = toff[i0];
    for (long long i = i0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < i1; i += (long long)gridDim.x * blockDim.x)
        if (toff[i + 1] != toff[i]) {
            if (BULGE) (void)tg_bulge_line<true>(T, keys[i], i, text + (toff[i] - base));
            else (void)tg_line<true>(T, keys[i], i, text + (toff[i] - base));
        }
}

}  // namespace mirp

static inline int tg_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

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

    // sort, cut and write the n <= cap keys of the last scan
    int finish(int mbase, long long n) {
        using namespace mirp;
        hipStream_t st = c->stream;
        stats[1]++;
        if (n == 0) return 0;
        double t = mirp::now();
        unsigned long long* d_keys = (unsigned long long*)c->tg_keys.p;
        int mbits = 0;                                         // the key's bits above the miRNA index are 0
        while ((1 << mbits) < group_n) mbits++;
        const bool bulge = o->bulge != 0;
        if (int rc = mirp_device_sort_u64(c, d_keys, (unsigned long long*)c->tg_ktmp.p, n, 0, ((bulge ? TG_BULGE_SHIFT : 38) + mbits + 7) / 8 * 8)) return rc;
        T.mbase = mbase;
        unsigned long long* d_small = (unsigned long long*)c->tg_small.p;
        long long* d_toff = (long long*)c->tg_toff.p;
        HIPCHK(c, hipMemsetAsync(d_small + 1, 0, 8, st));
        if (o->energy) {                                       // the folds of the sorted keys that -k keeps: the width of `mfe` is part of a line's length
            const DxTargets D{T.pk, T.amb, T.mcodes, T.mi, T.cstart, T.n_contigs, mbase};
            if (int rc = mirp_device_duplex_sites(c, D, bulge, (const unsigned long long*)d_keys, n, (long long)o->max_sites,
                                                  (const unsigned long long*)c->tg_emitted.p, (int*)c->tg_emfe.p, (unsigned long long*)c->tg_ema.p,
                                                  (unsigned long long*)c->tg_emb.p))
                return rc;
        }
        if (o->accessibility) {                                // likewise the windows of the kept keys: the width of `upe` is part of a line's length
            const DxTargets D{T.pk, (const unsigned*)c->tg_amb.p, T.mcodes, T.mi, T.cstart, T.n_contigs, mbase};
            int longest = 0;                                   // the group's longest interval sizes the launch's tables
            for (int m = 0; m < group_n; m++) longest = std::max(longest, (int)(*mi)[(size_t)(mbase + m)].L + (bulge ? 1 : 0));
            if (int rc = mirp_device_unpaired_sites(c, D, bulge, (const unsigned long long*)d_keys, n, (long long)o->max_sites,
                                                    (const unsigned long long*)c->tg_emitted.p, longest, c->tg_up, c->tg_down, (int*)c->tg_upe.p))
                return rc;
        }
        hipLaunchKernelGGL(bulge ? tg_size_kernel<true> : tg_size_kernel<false>, dim3(tg_grid(n)), dim3(256), 0, st, T, (const unsigned long long*)d_keys, n,
                           (long long)o->max_sites, (const unsigned long long*)c->tg_emitted.p, (int*)c->tg_size.p, d_small + 1);
        hipLaunchKernelGGL(bulge ? tg_emitted_kernel<true> : tg_emitted_kernel<false>, dim3(tg_grid(n)), dim3(256), 0, st, (const unsigned long long*)d_keys, n,
                           (unsigned long long*)c->tg_emitted.p);
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
                if (c->tg_text.ensure((size_t)len + 16)) return fail(c, -6, "device allocation failed (targets: text)");
                hipLaunchKernelGGL(bulge ? tg_emit_kernel<true> : tg_emit_kernel<false>, dim3(tg_grid(i1 - i0)), dim3(256), 0, st, T, (const unsigned long long*)d_keys, i0, i1, (const long long*)d_toff,
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
        if (hits <= cap) return finish(mbase, hits);
        // overflow: hits per (miRNA, half-score), then passes of at most cap keys in output order
        HIPCHK(c, hipMemsetAsync(c->tg_hist.p, 0, 8 * (size_t)n * TG_NHALF, st));
        if (int rc = scan(1, mbase, 0, n, 0, total, &hits)) return rc;
        std::vector<unsigned long long> hist((size_t)n * TG_NHALF);
        HIPCHK(c, hipMemcpy(hist.data(), c->tg_hist.p, 8 * hist.size(), hipMemcpyDeviceToHost));
        std::vector<int> lim(n, smax);               // -k: no line of a miRNA past the half-score at which its first k lines are reached
        if (o->max_sites > 0)
            for (int m = 0; m < n; m++) {
                unsigned long long cum = 0;
                for (int h = 0; h <= smax; h++) {
                    cum += hist[(size_t)m * TG_NHALF + h];
                    if (cum >= (unsigned long long)o->max_sites) { lim[m] = h; break; }
                }
            }
        // the bins are (miRNA, half-score) up to lim[], the positions of a bin over cap are the target offsets
        const auto count = [&](long long i) { return (int)(i % TG_NHALF) <= lim[(size_t)(i / TG_NHALF)] ? (long long)hist[(size_t)i] : 0ll; };
        const auto flush = [&](long long first, long long last, long long expected) -> int {
            const int ma = (int)(first / TG_NHALF), ha = (int)(first % TG_NHALF), mb = (int)(last / TG_NHALF), hb = (int)(last % TG_NHALF);
            for (int m = ma; m <= mb; m++) set_range(mbase, m, m == ma ? ha : 0, m == mb ? hb : lim[m]);
            long long got = 0;
            if (int rc = scan(0, mbase, ma, mb + 1, 0, total, &got)) return rc;
            if (got != expected) return fail(c, -5, "targets: a pass found a different number of sites than counted");
            return finish(mbase, got);
        };
        const auto range = [&](long long bin, unsigned long long p, unsigned long long p1, long long* got) -> int {
            const int m = (int)(bin / TG_NHALF), h = (int)(bin % TG_NHALF);
            set_range(mbase, m, h, h);
            if (int rc = scan(0, mbase, m, m + 1, p, p1, got)) return rc;
            return *got > cap ? 0 : finish(mbase, *got);
        };
        const int rc = plan_passes((long long)n * TG_NHALF, count, cap, total, flush, range);
        return rc == PLAN_POSITION_OVER_CAP ? fail(c, -5, "targets: one offset holds more sites of one miRNA and score than a pass") : rc;
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
