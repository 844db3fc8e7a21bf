// Data-parallel predict-stage filter: dot-bracket hairpin classification, mature/star duplex
// rules, expression rules and the per-window locus decision.  One wavefront per precursor window.
// Replaces the per-window Python loop of filter_next_loci / check_loci
// (/root/reference/miR_PREFeR.py = MP: a8 :1541-1724, a9 :1727-1999, a10 :2002-2163, a11 :2206-2347)
// and its two `samtools view` subprocesses per window.
//
// Phase 1 (lane per RNALfold line): structure list of the window (MP:1541-1599).
// Phase 2 (lane per (in-range mature, structure) pair, passes of 64 pairs): get_maturestar_info + check_expression_new.
// Phase 3 (per mature, over the lanes that hold its pairs): the sequential "lowest normalised energy that passes" rule (MP:2246-2343).
// The structure rules of phases 1 and 2 work on words of the staged text (ss_words.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mirp_internal.h"
#include "predict_device.h"

namespace mirp {

// Capacities of one launch (PredictCaps, mirp_internal.h): p_cap pieces per structure line (filter_ss keeps pieces longer than 55 characters: at most
// len / 56 of them), s_cap structures per window (lines x pieces), m_cap candidate matures per window.  A window that needs more is flagged
// (status 2 / 3) with what it needs, and run_predict_launch re-runs just those windows with capacities sized for them: the reference has no
// such limits (MP:1541-1599, 2241), so neither does the result.
#define PW_MIN_STRUCTS 192

// Diagnostics build (make DIAG=1): phase clocks of the filter, read by every wave at the phase edges (s_memtime is wave-uniform), summed over windows by
// lane 0 into one of PCLK_ROWS rows (so that the sums of thousands of waves do not queue on eight addresses in front of the next window's loads) and
// printed after the launch when MIRP_PREDICT_CLOCKS is set (profiles/tools/pred_clocks.py).  The product build carries none of this.
#ifdef MIRP_DIAG
#define PCLK_N 7
#define PCLK_ROWS 4096
__device__ unsigned long long g_pclk[PCLK_ROWS][PCLK_N + 1];
#define PCLK_DECL long long pc_t = clock64(), pc_acc[PCLK_N] = {0, 0, 0, 0, 0, 0, 0};
#define PCLK(i) { const long long t_ = clock64(); pc_acc[i] += t_ - pc_t; pc_t = t_; }
#define PCLK_FLUSH if (lane == 0) { unsigned long long* row_ = g_pclk[blockIdx.x & (PCLK_ROWS - 1)]; for (int q_ = 0; q_ < PCLK_N; q_++) atomicAdd(&row_[q_], (unsigned long long)pc_acc[q_]); atomicAdd(&row_[PCLK_N], 1ull); }
static void predict_clocks_print() {
    static const char* const name[PCLK_N] = {"line selection + text staging", "phase 1 (classification)", "phase 1 ordered compaction", "mature ranking + wave_lower_bound x2",
                                             "d_maturestar over all pairs", "d_expression", "arg-min, write and the rest"};
    std::vector<unsigned long long> all((size_t)PCLK_ROWS * (PCLK_N + 1)), z(all.size(), 0ull);
    if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_pclk), 8 * all.size()) != hipSuccess || hipMemcpyToSymbol(HIP_SYMBOL(g_pclk), z.data(), 8 * z.size()) != hipSuccess) return;
    unsigned long long h[PCLK_N + 1] = {};
    for (size_t k = 0; k < all.size(); k++) h[k % (PCLK_N + 1)] += all[k];
    unsigned long long tot = 0;
    for (int q = 0; q < PCLK_N; q++) tot += h[q];
    std::fprintf(stderr, "[mirp predict clocks] windows=%llu total=%llu ticks (sum over windows, s_memtime)\n", h[PCLK_N], tot);
    for (int q = 0; q < PCLK_N; q++)
        std::fprintf(stderr, "[mirp predict clocks] %-40s %14llu  %5.1f %%  %9.0f / window\n", name[q], h[q], tot ? 100.0 * (double)h[q] / (double)tot : 0.0,
                     h[PCLK_N] ? (double)h[q] / (double)h[PCLK_N] : 0.0);
}
#else
#define PCLK_DECL
#define PCLK(i)
#define PCLK_FLUSH
#endif

__device__ __forceinline__ long long aln_lower_bound(const MirpAln* __restrict__ a, long long n, int tid, long long pos) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        long long mid = (lo + hi) >> 1;
        MirpAln r = a[mid];
        if (r.tid < tid || (r.tid == tid && r.pos < pos)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// lower bound inside [lo, hi) (the window's own records: tens to hundreds, found once per window by the whole wave)
__device__ __forceinline__ long long aln_lower_bound_in(const MirpAln* __restrict__ a, long long lo, long long hi, int tid, long long pos) {
    while (lo < hi) {
        long long mid = (lo + hi) >> 1;
        MirpAln r = a[mid];
        if (r.tid < tid || (r.tid == tid && r.pos < pos)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the same lower bound over the whole record array with all 64 lanes probing at once: 3 round trips for 10^5 records, 5 for 10^7 (a lane's own binary
// search takes 17 .. 25 dependent ones, and every (mature, structure) pair of the window used to pay two of them)
__device__ __forceinline__ long long wave_lower_bound(const MirpAln* __restrict__ a, long long n, int tid, long long pos) {
    const int lane = threadIdx.x & 63;
    long long lo = 0, hi = n;
    while (hi - lo > 64) {
        const long long step = (hi - lo + 63) / 64;
        const long long idx = lo + step * (lane + 1) - 1;
        bool less = false;
        if (idx < hi) { const MirpAln r = a[idx]; less = r.tid < tid || (r.tid == tid && r.pos < pos); }
        const long long cnt = (long long)__popcll(__ballot(less));          // the probes below the key are a prefix of the lanes
        const long long nlo = lo + step * cnt, nhi = lo + step * (cnt + 1) - 1;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    bool less = false;
    if (lo + lane < hi) { const MirpAln r = a[lo + lane]; less = r.tid < tid || (r.tid == tid && r.pos < pos); }
    return lo + (long long)__popcll(__ballot(less));
}

struct ExprRes {
    long long total_this, total_mature, total_iso, total_star; // total_star = after max with imperfect (when key present)
    long long raw_star, total_anti, imp[3];                    // reasons mode: star before the imperfect maximum, antisense depth, the three imperfect-star depths
    int distance, has_imp_key, imp_start, imp_end, imp_which /* -1 none */;
    double ratio_total, ratio_iso;
    bool too_many_start, expressed_all, exception;
};

// check_expression_new (MP:2037-2163) on reads kept by gen_mapinfo_each_sample (MP:2021)
// Sample sets as bit masks over the 8-bit sample index of a record (any number of ALIGNMENT_FILEs up to MIRP_MAX_SAMPLES, MP:3300-3308): eight words,
// indexed through compile-time selects so that they stay in registers.
struct SampleSet {
    unsigned int w[8];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0u;
    }
    __device__ __forceinline__ bool test_and_set(int s) {          // -> was the bit clear?
        const unsigned int bit = 1u << (s & 31);
        const int wi = s >> 5;
        bool fresh = false;
#pragma unroll
        for (int i = 0; i < 8; i++) if (i == wi) { fresh = !(w[i] & bit); w[i] |= bit; }
        return fresh;
    }
    __device__ __forceinline__ bool holds_first(int n) const {       // bits 0 .. n-1 all set
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int lo = 32 * i;
            if (n > lo) { const unsigned int want = (n - lo >= 32) ? 0xffffffffu : ((1u << (n - lo)) - 1u); ok = ok && ((w[i] & want) == want); }
        }
        return ok;
    }
};

// mature_each (reasons mode): where the per-sample mature depths go -- the tail of the thread's own reasons record, already zeroed; nullptr otherwise
template <bool REASONS>
__device__ void d_expression(const MirpAln* __restrict__ a, long long na, int n_samples, int tid, int ws, int we, int fold_s, int fold_e,
                             int m0, int m1, int star_s, int star_e, int strand, int allow_3nt, ExprRes& o, int* mature_each, int mature_each_cap,
                             long long wk0, long long wk1) {
    const int mature_len = m1 - m0, star_len = star_e - star_s, pre_len = fold_e - fold_s;
    // [wk0, wk1) = the records that start inside the window [ws, we); a record that starts at or behind we fails the test below anyway
    (void)na;
    long long k0 = aln_lower_bound_in(a, wk0, wk1, tid, fold_s > ws ? fold_s : ws), k1 = aln_lower_bound_in(a, wk0, wk1, tid, fold_e);
    long long tot_pre = 0, tot_mat = 0, tot_iso = 0, tot_star = 0, imp[3] = {0, 0, 0};
    SampleSet mature_set;          // samples with reads_mature > 0
    SampleSet seen;                // samples with a read on this strand starting at cur_pos (the records are sorted by position)
    mature_set.clear(); seen.clear();
    int starts = 0, cur_pos = -1;
    long long tot_anti = 0;
    for (long long k = k0; k < k1; k++) {
        MirpAln r = a[k];
        if (r.pos < ws || r.pos + (int)r.len > we) continue;
        if ((int)r.strand != strand) { if (REASONS) tot_anti += (int)r.depth; continue; }   // antisense reads do not enter any rule used by check_loci
        int d = (int)r.depth, rl = r.len, sp = r.pos, sm = r.sample;
        if (sp != cur_pos) { cur_pos = sp; seen.clear(); }
        if (seen.test_and_set(sm)) starts++;          // once per (start position, sample with reads there), MP:2066-2068
        tot_pre += d;
        if (sp == m0 && rl == mature_len) {
            tot_mat += d;
            if (d > 0) (void)mature_set.test_and_set(sm);
            if (REASONS) { if (mature_each && sm < mature_each_cap) mature_each[sm] += d; }
        }
        if (sp == star_s && rl == star_len) tot_star += d;
        int dx = sp - m0, dl = rl - mature_len;
        if (dx >= -3 && dx <= 3 && dl >= -3 && dl <= 3) tot_iso += d;
        if (allow_3nt) {
            if (sp == star_s && rl == star_len + 1) imp[0] += d;
            else if (sp - 1 == star_s && rl == star_len - 1) imp[1] += d;
            else if (sp - 1 == star_s && rl == star_len) imp[2] += d;
        }
    }
    o.total_this = tot_pre; o.total_mature = tot_mat; o.total_iso = tot_iso;
    o.raw_star = tot_star; o.total_anti = tot_anti; o.imp[0] = imp[0]; o.imp[1] = imp[1]; o.imp[2] = imp[2];
    o.distance = (star_s > m1) ? star_s - m1 : m0 - star_e;
    long long max_imp = 0;
    o.has_imp_key = 0; o.imp_start = 0; o.imp_end = 0; o.imp_which = -1;
    if (tot_star == 0 && allow_3nt) {
        o.has_imp_key = 1;
        long long mx = imp[0] > imp[1] ? imp[0] : imp[1]; mx = mx > imp[2] ? mx : imp[2];
        if (mx > 0) {
            int which = (imp[0] == mx) ? 0 : (imp[1] == mx) ? 1 : 2;
            if (which == 0) { o.imp_start = star_s; o.imp_end = star_e + 1; }
            else if (which == 1) { o.imp_start = star_s + 1; o.imp_end = star_e; }
            else { o.imp_start = star_s + 1; o.imp_end = star_e + 1; }
            o.imp_which = which;
            max_imp = mx;
        }
    }
    long long st = tot_star > max_imp ? tot_star : max_imp;
    o.total_star = st;
    o.exception = (tot_pre == 0);
    o.ratio_total = o.exception ? 0.0 : (double)(tot_mat + st) / (double)tot_pre;
    o.ratio_iso = o.exception ? 0.0 : (double)(tot_iso + st) / (double)tot_pre;
    // only the LAST sample's start counter is ever non-zero (stale loop variable, MP:2046/2068)
    o.too_many_start = ((double)starts / pre_len) > 0.5;
    o.expressed_all = mature_set.holds_first(n_samples);
}

// REASONS: the -d mode of the reference (check_loci's dict_why_not_miRNA_reasons, MP:2206-2347): every evaluated (mature, structure) pair is
// appended to a record pool (rstride ints per record, layout in mirp_pipeline.cpp) together with one record per window; nothing else changes.
// GTEXT: the staged structure text lives in a global scratch area of the workgroup instead of LDS -- windows whose lines do not fit there (PRECURSOR_LEN in
// the thousands: hundreds of lines of thousands of characters); everything else is the same code.
template <bool REASONS, bool GTEXT>
#ifndef MIRP_PRED_WPS
#define MIRP_PRED_WPS 4
#endif
__global__ void __launch_bounds__(64, MIRP_PRED_WPS) predict_kernel(
    const MirpWindow* __restrict__ windows, int n_windows, const MirpMature* __restrict__ matures,
    const MirpAln* __restrict__ alns, long long n_alns, const MirpFoldLine* __restrict__ lines, const char* __restrict__ ss,
    int ss_stride, int max_lines, const int* __restrict__ n_lines, MirpPredictParams pp,
    MirpMirna* __restrict__ out /* [n_windows * MIRP_MAX_MIRNA_PER_WINDOW] */, int* __restrict__ n_out, int* __restrict__ status,
    unsigned int* __restrict__ rcount, int* __restrict__ rpool, unsigned int rcap, int rstride,
    const int* __restrict__ wsel, int n_sel, const int* __restrict__ skip, const int* __restrict__ wslot, PredictCaps caps, int* __restrict__ need,
    unsigned long long* __restrict__ gtext) {
    // wsel == nullptr: every window w in [0, n_windows) with its fold output at slot w, except those with skip[w] >= 0 (folded again at full
    // line capacity: a second launch handles them); wsel != nullptr: the windows wsel[k], k in [0, n_sel), with their fold output at slot
    // wslot[k] (wslot == nullptr: slot k).  need (optional): need[3 w] = structures, need[3 w + 1] = pieces of one line, need[3 w + 2] = staged lines the window has.
    extern __shared__ __align__(16) unsigned char smem[];
    const int wpl = ssw_words(ss_stride);                                 // 64-bit words per staged line (32 characters each)
    const int max_structs = caps.s_cap, PW_MAX_PIECES = caps.p_cap, PW_MAX_MATURES = caps.m_cap, L_CAP = caps.l_cap;
    unsigned long long* textw = GTEXT ? gtext + (size_t)blockIdx.x * L_CAP * wpl : (unsigned long long*)smem;      // l_cap * wpl: only the lines phase 1 looks at (printed, >= minlen) are staged
    PStruct* sts = (PStruct*)(smem + (GTEXT ? (size_t)0 : (((size_t)L_CAP * wpl * 8 + 15) & ~(size_t)15))); // max_structs
    PStruct* slot = sts + max_structs;                                // 64 * p_cap
    int* morder = (int*)(slot + 64 * PW_MAX_PIECES);                     // m_cap: mature indices in stable depth-descending order (MP:2241)
    unsigned short* lslot = (unsigned short*)(morder + PW_MAX_MATURES);  // max_lines: staged slot of a line, 0xffff = not staged
    unsigned short* lline = lslot + max_lines;                           // l_cap: line of a staged slot
    const int lane = threadIdx.x;
    const int n_iter = wsel ? n_sel : n_windows;
    for (int it = blockIdx.x; it < n_iter; it += gridDim.x) {
        const int w = wsel ? wsel[it] : it;
        if (!wsel && skip && skip[it] >= 0) continue;      // block-uniform
        const int sl = wslot ? wslot[it] : it;             // slot of the window's fold output
        const MirpWindow W = windows[w];
        const int nl = n_lines[sl] < max_lines ? n_lines[sl] : max_lines;
        const MirpFoldLine* wl = lines + (size_t)sl * max_lines;
        int st_flag = 0, need_pieces = 0;
        PCLK_DECL
        // which lines are staged: the printed ones of at least minlen characters (MP:1568-1570), in line order; about half of a window's lines
        // (23 of 42 on the benchmark input), which is what lets 16 instead of 11 windows be resident per CU
        int n_used = 0;
        for (int lb = 0; lb < nl; lb += 64) {
            const int k = lb + lane;
            bool used = false;
            if (k < nl) { const MirpFoldLine ln = wl[k]; used = ln.printed && ln.len >= pp.minlen; }
            const unsigned long long bal = __ballot(used);
            const int u = n_used + (int)__popcll(bal & ((1ull << lane) - 1ull));
            if (k < nl) lslot[k] = (used && u < L_CAP) ? (unsigned short)u : (unsigned short)0xffff;
            if (used && u < L_CAP) lline[u] = (unsigned short)k;
            if (used && u >= L_CAP) st_flag = 2;          // more lines than this launch stages: the window is run again with room for all of them
            n_used += (int)__popcll(bal);
        }
        __syncthreads();
        // stage their text as '(' and ')' bit planes (lane = one word = 32 characters)
        {
            const char* src = ss + (size_t)sl * max_lines * ss_stride;
            const int nu = n_used < L_CAP ? n_used : L_CAP;
            for (int x = lane; x < nu * wpl; x += 64) {
                const int us = x / wpl, wi = x - us * wpl, ln = lline[us];
                textw[x] = d_stage_word(src + (size_t)ln * ss_stride, ss_stride, wi);
            }
        }
        __syncthreads();
        PCLK(0)
        // ---- phase 1: structures (lane per line, chunks of 64 lines)
        int nst = 0;
        for (int lb = 0; lb < nl; lb += 64) {
            int k = lb + lane, cnt = 0;
            if (k < nl) {
                MirpFoldLine ln = wl[k];
                const int us = lslot[k];
                SSW s; s.w = textw + (size_t)(us == 0xffff ? 0 : us) * wpl; s.o = 0;
                if (ln.printed && ln.len >= pp.minlen && us != 0xffff) {
                    if (ssw_is_stem_loop(s, ln.len)) {
                        PStruct p; p.line = (unsigned short)k; p.off = 0; p.len = (unsigned short)ln.len; p.type = 0;
                        slot[lane * PW_MAX_PIECES + cnt++] = p;
                    } else {
                        // filter_ss (MP:1685-1724): one piece per top-level stem, [previous gap start, next stem start)
                        int len = ln.len;
                        int prefirst = ssw_find(s, '(', 0, len);
                        if (prefirst >= 0) {
                            int prelast = ssw_partner(s, len, prefirst), curfirst = prefirst, curlast = prelast, pregap0 = 0;
                            while (curfirst != -1) {
                                curfirst = ssw_find(s, '(', prelast < 0 ? len : prelast, len);
                                int after1 = len;
                                if (curfirst != -1) { after1 = curfirst; curlast = ssw_partner(s, len, curfirst); }
                                int ps = pregap0, pl = after1 - pregap0;
                                if (pl > 55) {
                                    int type = -1;
                                    if (ssw_is_stem_loop(s + ps, pl)) type = 0;
                                    else if (ssw_good_bifurcation(s + ps, pl)) type = 1;
                                    if (type >= 0) {
                                        if (cnt < PW_MAX_PIECES) {
                                            PStruct p; p.line = (unsigned short)k; p.off = (unsigned short)ps; p.len = (unsigned short)pl; p.type = (unsigned short)type;
                                            slot[lane * PW_MAX_PIECES + cnt++] = p;
                                        } else st_flag = 2;
                                        need_pieces++;
                                    }
                                }
                                pregap0 = prelast + 1;
                                prelast = curlast;
                            }
                        }
                    }
                }
            }
            PCLK(1)
            // ordered compaction (line order, piece order): a wave prefix sum of the lanes' counts
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
            const int base = nst + incl - cnt;
            for (int c = 0; c < cnt; c++) { if (base + c < max_structs) sts[base + c] = slot[lane * PW_MAX_PIECES + c]; else st_flag = 2; }
            nst += __shfl(incl, 63);
            __syncthreads();
            PCLK(2)
        }
        if (need) {          // what this window needs, for the re-run of flagged windows: structures in all, pieces of its richest line
            int np = need_pieces;
            for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(np, o); np = t > np ? t : np; }
            if (lane == 0) { need[3 * (size_t)w] = nst; need[3 * (size_t)w + 1] = np; need[3 * (size_t)w + 2] = n_used; }
        }
        if (nst > max_structs) nst = max_structs;
        // ---- phases 2+3 per mature, depth-descending stable order (MP:2241)
        int nm = W.n_matures < PW_MAX_MATURES ? W.n_matures : PW_MAX_MATURES;
        if (W.n_matures > PW_MAX_MATURES) st_flag = 3;
        if (nm <= 64) {          // lane k holds mature k, read once: its rank among the nm by shuffles
            int dk = 0;
            if (lane < nm) dk = matures[W.mature_off + lane].depth;
            int r = 0;
            for (int j = 0; j < nm; j++) { const int dj = __shfl(dk, j); if (dj > dk || (dj == dk && j < lane)) r++; }
            if (lane < nm) morder[r] = lane;
        } else {
            for (int k = lane; k < nm; k += 64) {          // rank of mature k among the first nm: lane-parallel, then the order is a table
                const int dk = matures[W.mature_off + k].depth;
                int r = 0;
                for (int j = 0; j < nm; j++) { const int dj = matures[W.mature_off + j].depth; if (dj > dk || (dj == dk && j < k)) r++; }
                morder[r] = k;
            }
        }
        __syncthreads();
        // keep the matures inside the length range, in rank order, in place: morder[0 .. n_in)
        int n_in = 0;
        for (int rb = 0; rb < nm; rb += 64) {
            const int rank = rb + lane;
            int mi = -1;
            bool inr = false;
            if (rank < nm) { mi = morder[rank]; const MirpMature mk = matures[W.mature_off + mi]; const int l = mk.end - mk.start; inr = !(l < pp.min_mature_len || l > pp.max_mature_len); }
            const unsigned long long bal = __ballot(inr);
            __syncthreads();          // every read of this chunk before a write into it (a write goes to an index <= its lane's rank)
            if (inr) morder[n_in + (int)__popcll(bal & ((1ull << lane) - 1ull))] = mi;
            n_in += (int)__popcll(bal);
        }
        __syncthreads();
        const bool any_in_range = n_in > 0;
        int nout = 0;
        const long long wk0 = wave_lower_bound(alns, n_alns, W.tid, W.ws), wk1 = wave_lower_bound(alns, n_alns, W.tid, W.we);
        PCLK(3)
        if (nst > 0 && any_in_range) {
            // Phases 2+3: a lane per (in-range mature in rank order, structure) pair, in passes of 64 pairs -- one pass for nearly every window, where the
            // loop over matures ran a pass per mature with a tenth of the lanes.  Per mature the sequential rule of MP:2246-2343 ("for s in order: skip if
            // ne > lowest; if it passes: best = s, lowest = ne", lowest starting at 0.0) selects the passing structure with the smallest normalised
            // energy <= 0 and, among equals, the LAST one in order: an arg-min over the lanes that hold the mature's pairs, carried (c_*) to the next
            // pass when the mature's pairs go on there.  The winner's lane writes the row; a better one of a later pass writes over it.
            const int npairs = n_in * nst;
            double c_ne = 0.0;
            int c_s = -1, c_i = -1;
            for (int pb = 0; pb < npairs; pb += 64) {
                const int pr = pb + lane;
                int pi = -1, s = -1, pass = 0;
                double ne = 0.0;
                MirpMature m;
                m.start = m.end = m.strand = m.depth = 0;
                int b_has_star = 0, b_star_s = 0, b_star_e = 0, b_fold_s = 0, b_fold_e = 0, b_tm = 0, b_ts = 0, b_imp = 0;
                {
                    if (pr < npairs) {
                        pi = pr / nst; s = pr - pi * nst;
                        const int mi = morder[pi];          // the pi-th in-range mature in stable depth-descending order
                        m = matures[W.mature_off + mi];
                        const PStruct p = sts[s];
                        const MirpFoldLine ln = wl[p.line];
                        ne = ((double)ln.energy / 100.0) / (double)ln.len;
                        SSW str; str.w = textw + (size_t)lslot[p.line] * wpl; str.o = p.off;
                        MStar ms;
                        PCLK(6)
                        ssw_maturestar(str, p.len, m.start, m.end, ln.start + p.off, W.ws, W.we, m.strand, ms);
                        PCLK(4)
                        int has_star = 0, star_s = ms.star_s, star_e = ms.star_e, impf = 0;
                        long long tm = 0, ts = 0;
                        ExprRes rx;
                        rx.exception = true;
                        int* rrec = nullptr;          // reasons mode: this (mature, structure) pair's record, claimed before the expression test fills its tail
                        if (REASONS) {
                            const unsigned int ridx = atomicAdd(rcount, 1u);
                            if (ridx < rcap) { rrec = rpool + (size_t)ridx * rstride; for (int q = 12; q < rstride; q++) rrec[q] = 0; }
                        }
                        if (ms.code == 0) {
                            ExprRes& ex = rx;
                            d_expression<REASONS>(alns, n_alns, pp.n_samples, W.tid, W.ws, W.we, ms.fold_s, ms.fold_e, m.start, m.end, ms.star_s, ms.star_e,
                                         m.strand, pp.allow_3nt, ex, (REASONS && rrec && rstride > 21) ? rrec + 21 : nullptr, rstride - 21, wk0, wk1);
                            tm = ex.total_mature; ts = ex.total_star;
                            // 'max_imperfect_star' in exprinfo (MP:2161, 2631-2635): bit0 key present, bits1-2 which+1, bit3 max > 0
                            impf = (ex.has_imp_key ? 1 : 0) | ((ex.imp_which + 1) << 1) | ((ex.imp_which >= 0) ? 8 : 0);
                            if (!ex.exception && ex.distance > 4) {
                                if (ex.total_star > 0) {
                                    if (!(ex.ratio_total < 0.2)) {
                                        pass = 1; has_star = 1;
                                        if (ex.has_imp_key) { star_s = ex.imp_start; star_e = ex.imp_end; }
                                    }
                                } else if (pp.allow_no_star && !ex.too_many_start) {
                                    if (ex.ratio_iso >= 0.8 && (ex.expressed_all || ex.total_mature >= 1000)) pass = 1;
                                }
                            }
                        }
                        PCLK(5)
                        if (REASONS) {
                            int flags = 0;
                            ExprRes* exp_ = nullptr;
                            (void)exp_;
                            if (rrec) {
                                int* r = rrec;
                                r[0] = w; r[1] = morder[pi]; r[2] = s; r[3] = p.line; r[4] = p.off; r[5] = p.len; r[6] = ms.code; r[8] = ms.fold_s; r[9] = ms.fold_e;
                                r[10] = ms.star_s; r[11] = ms.star_e;
                                if (ms.code == 0) {
                                    // the depth fields saturate at 2^31 - 1 like MirpMirna's totals; the flags below follow the 64-bit sums
                                    const long long dv[8] = {rx.total_this, rx.total_anti, rx.total_mature, rx.total_iso, rx.raw_star, rx.imp[0], rx.imp[1], rx.imp[2]};
#pragma unroll
                                    for (int q = 0; q < 8; q++) r[12 + q] = (int)(dv[q] > 0x7fffffffLL ? 0x7fffffffLL : dv[q]);
                                    r[20] = rx.distance;
                                    if (rx.exception) flags |= 256;
                                    else if (rx.distance <= 4) flags |= 1;
                                    else if (rx.total_star > 0) { if (rx.ratio_total < 0.2) flags |= 2; else flags |= 128; }
                                    else if (!pp.allow_no_star) flags |= 4;
                                    else if (rx.too_many_start) flags |= 8;
                                    else if (rx.ratio_iso >= 0.8 && (rx.expressed_all || rx.total_mature >= 1000)) flags |= 128;
                                    else {
                                        if (rx.ratio_iso < 0.8) flags |= 16;
                                        if (rx.total_mature <= 100) flags |= 32;
                                        if (!rx.expressed_all) flags |= 64;
                                    }
                                }
                                r[7] = flags;
                            }
                        }
                        pass = (pass && ne <= 0.0) ? 1 : 0;
                        b_has_star = has_star; b_star_s = star_s; b_star_e = star_e; b_fold_s = ms.fold_s; b_fold_e = ms.fold_e;
                        b_tm = (int)(tm > 0x7fffffffLL ? 0x7fffffffLL : tm); b_ts = (int)(ts > 0x7fffffffLL ? 0x7fffffffLL : ts); b_imp = impf;
                    }
                }
                // the matures of this pass, in rank order
                const int last_pair = (pb + 63 < npairs - 1) ? pb + 63 : npairs - 1;
                for (int ii = pb / nst; ii <= last_pair / nst; ii++) {
                    if (c_i != ii) { c_i = ii; c_ne = 0.0; c_s = -1; }
                    const bool mine = pi == ii && pass;
                    if (__ballot(mine) != 0ull) {
                        // wave arg-min over (ne ascending, s descending) among the lanes that hold a passing pair of this mature
                        double r_ne = ne;
                        int r_s = mine ? s : -1;
                        for (int o = 32; o > 0; o >>= 1) {
                            const double t_ne = __shfl_xor(r_ne, o);
                            const int t_s = __shfl_xor(r_s, o);
                            const bool take = t_s >= 0 && (r_s < 0 || t_ne < r_ne || (t_ne == r_ne && t_s > r_s));
                            if (take) { r_ne = t_ne; r_s = t_s; }
                        }
                        if (c_s < 0 || r_ne < c_ne || (r_ne == c_ne && r_s > c_s)) {          // against what the passes before found for it (their s is smaller)
                            c_ne = r_ne; c_s = r_s;
                            if (mine && s == r_s && nout < MIRP_MAX_MIRNA_PER_WINDOW) {   // exactly one lane owns the winner
                                const PStruct bp = sts[r_s];
                                MirpMirna r;
                                r.window = w; r.tid = W.tid; r.fold_s = b_fold_s; r.fold_e = b_fold_e; r.mat_s = m.start; r.mat_e = m.end;
                                r.star_s = b_star_s; r.star_e = b_star_e; r.strand = m.strand; r.has_star = b_has_star;
                                r.line = bp.line; r.ss_off = bp.off; r.ss_len = bp.len; r.reserved = b_imp;
                                r.total_depth_mature = b_tm; r.total_depth_star = b_ts;
                                out[(size_t)w * MIRP_MAX_MIRNA_PER_WINDOW + nout] = r;
                            }
                        }
                    }
                    // the mature's last pair lies in this pass: its row, if it has one, is final
                    if ((ii + 1) * nst <= pb + 64 && c_s >= 0 && nout < MIRP_MAX_MIRNA_PER_WINDOW) nout++;
                }
            }
        }
        if (lane == 0) { n_out[w] = nout; }
        if (REASONS && lane == 0) {
            const unsigned int ridx = atomicAdd(rcount, 1u);
            if (ridx < rcap) {
                int* r = rpool + (size_t)ridx * rstride;
                for (int q = 0; q < rstride; q++) r[q] = 0;
                r[0] = w; r[1] = -1; r[2] = nst; r[3] = any_in_range ? 1 : 0; r[4] = nout;
            }
        }
        // any lane may have raised a capacity flag
        {
            int f = st_flag;
            for (int o = 32; o > 0; o >>= 1) { int t = __shfl_xor(f, o); f = t > f ? t : f; }
            if (lane == 0) status[w] = f;
        }
        PCLK(6)
        PCLK_FLUSH
        __syncthreads();
    }
}

#ifndef MIRP_PRED_LCAP
#define MIRP_PRED_LCAP 48
#endif
PredictCaps predict_default_caps(int max_lines, int ss_stride) {
    PredictCaps c;
    c.p_cap = std::max(6, ss_stride / 56 + 1);
#ifdef MIRP_PRED_SCAP_BY_LCAP          // (experiment: structures sized from the staged lines)
    { const int lc = max_lines <= 96 ? std::min(max_lines, MIRP_PRED_LCAP) : max_lines; c.s_cap = 2 * lc > 96 ? 2 * lc : 96; }
#else
    c.s_cap = 2 * max_lines > PW_MIN_STRUCTS ? 2 * max_lines : PW_MIN_STRUCTS;
#endif
    c.m_cap = 64;
    // lines staged per window: the main launch (max_lines = 96) takes 40 -- 99.98 % of the benchmark's windows have fewer printed lines of >= 55
    // characters (profiles/tools/nl_hist.py), the rest is run again; launches over the full-capacity side buffers stage everything
    c.l_cap = max_lines <= 96 ? std::min(max_lines, MIRP_PRED_LCAP) : max_lines;
    return c;
}

size_t predict_lds_bytes(int max_lines, int ss_stride, PredictCaps caps, bool text_in_lds) {
    size_t b = text_in_lds ? (((size_t)caps.l_cap * ssw_words(ss_stride) * 8 + 15) & ~(size_t)15) : 0;
    b += sizeof(PStruct) * ((size_t)caps.s_cap + 64 * (size_t)caps.p_cap);
    b += sizeof(int) * (size_t)caps.m_cap;
    b += sizeof(unsigned short) * ((size_t)max_lines + (size_t)caps.l_cap);
    return (b + 15) & ~(size_t)15;
}
size_t predict_lds_bytes(int max_lines, int ss_stride, PredictCaps caps) { return predict_lds_bytes(max_lines, ss_stride, caps, true); }
size_t predict_lds_bytes(int max_lines, int ss_stride) { return predict_lds_bytes(max_lines, ss_stride, predict_default_caps(max_lines, ss_stride)); }
// what has to fit whatever the lines' number and length (structures, pieces, matures): the staged text itself moves to global memory when it does not
size_t predict_lds_bytes_min(int max_lines, int ss_stride, PredictCaps caps) { return predict_lds_bytes(max_lines, ss_stride, caps, false); }
size_t predict_lds_bytes_min(int max_lines, int ss_stride) { return predict_lds_bytes(max_lines, ss_stride, predict_default_caps(max_lines, ss_stride), false); }

template <bool REASONS, bool GTEXT>
static hipError_t launch_predict_as(hipStream_t stream, int grid, size_t lds, const MirpWindow* windows, int n_windows, const MirpMature* matures,
                                    const MirpAln* alns, long long n_alns, const MirpFoldLine* lines, const char* ss, int ss_stride, int max_lines,
                                    const int* n_lines, MirpPredictParams pp, MirpMirna* out, int* n_out, int* status, unsigned int* rcount, int* rpool,
                                    unsigned int rcap, int rstride, const int* wsel, int n_sel, const int* skip, const int* wslot, PredictCaps caps, int* need, unsigned long long* gtext) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)predict_kernel<REASONS, GTEXT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((predict_kernel<REASONS, GTEXT>), dim3(grid), dim3(64), lds, stream, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride,
                       max_lines, n_lines, pp, out, n_out, status, REASONS ? rcount : nullptr, REASONS ? rpool : nullptr, REASONS ? rcap : 0u, REASONS ? rstride : 0,
                       wsel, n_sel, skip, wslot, caps, need, gtext);
    return hipGetLastError();
}

hipError_t launch_predict(hipStream_t stream, int grid, const MirpWindow* windows, int n_windows, const MirpMature* matures,
                          const MirpAln* alns, long long n_alns, const MirpFoldLine* lines, const char* ss, int ss_stride, int max_lines,
                          const int* n_lines, MirpPredictParams pp, MirpMirna* out, int* n_out, int* status, unsigned int* rcount, int* rpool,
                          unsigned int rcap, int rstride, const int* wsel, int n_sel, const int* skip, const int* wslot, const PredictCaps* caps_in, int* need) {
    const PredictCaps caps = caps_in ? *caps_in : predict_default_caps(max_lines, ss_stride);
    size_t lds = predict_lds_bytes(max_lines, ss_stride, caps);
#ifdef MIRP_PRED_LDS_PAD
    lds += MIRP_PRED_LDS_PAD;      // timing experiment: fewer resident windows per CU
#endif
    if (lds <= 160 * 1024) {
        if (rpool)
            return launch_predict_as<true, false>(stream, grid, lds, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, out, n_out, status,
                                                  rcount, rpool, rcap, rstride, wsel, n_sel, skip, wslot, caps, need, nullptr);
        return launch_predict_as<false, false>(stream, grid, lds, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, out, n_out, status,
                                               rcount, rpool, rcap, rstride, wsel, n_sel, skip, wslot, caps, need, nullptr);
    }
    // the staged text does not fit in LDS: a scratch area per workgroup in global memory (a few workgroups: the area is l_cap lines of ss_stride / 4 bytes each),
    // allocated and released around the launch -- the path of PRECURSOR_LEN in the thousands, not of the benchmark
    lds = predict_lds_bytes(max_lines, ss_stride, caps, false);
    const size_t per = (size_t)caps.l_cap * ssw_words(ss_stride) * 8;
    grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)2 << 30) / std::max<size_t>(per, 1)));
    unsigned long long* gtext = nullptr;
    hipError_t e = hipMalloc((void**)&gtext, per * (size_t)grid + 16);
    if (e != hipSuccess) return e;
    if (rpool)
        e = launch_predict_as<true, true>(stream, grid, lds, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, out, n_out, status,
                                          rcount, rpool, rcap, rstride, wsel, n_sel, skip, wslot, caps, need, gtext);
    else
        e = launch_predict_as<false, true>(stream, grid, lds, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, out, n_out, status,
                                           rcount, rpool, rcap, rstride, wsel, n_sel, skip, wslot, caps, need, gtext);
    const hipError_t e2 = hipStreamSynchronize(stream);
    (void)hipFree(gtext);
    return e != hipSuccess ? e : e2;
}

// records of the first pass that belong to windows which are run again: r[0] = -1 (the host drops them)
__global__ void reasons_invalidate_kernel(int* __restrict__ rpool, unsigned int n, int rstride, const unsigned char* __restrict__ flagged) {
    for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        int* r = rpool + (size_t)k * rstride;
        if (r[0] >= 0 && flagged[r[0]]) r[0] = -1;
    }
}

// One launch of the filter plus, when windows exceeded a capacity, a second launch over just those windows with capacities sized from what they
// reported (need[]) and their number of candidate matures.  scope: the launch covers the windows wsel[0..n_sel) (slots wslot or k) or, with
// wsel == nullptr, every window except skip[w] >= 0.  Returns 0, or a negative code with *err set (LDS budget exceeded: -5).
// jobs_rec (optional): {launches, the largest ceil(windows / workgroups)} of the caller's record (mirp_ctx::jobs_per_slot[4]), updated per launch.
int run_predict_launch(hipStream_t stream, int n_cu, const MirpWindow* windows, int n_windows, const MirpMature* matures, const MirpAln* alns, long long n_alns,
                       const MirpFoldLine* lines, const char* ss, int ss_stride, int max_lines, const int* n_lines, MirpPredictParams pp, MirpMirna* out, int* n_out,
                       int* status, unsigned int* rcount, int* rpool, unsigned int rcap, int rstride, const int* wsel, int n_sel, const int* skip, std::string* err,
                       int* need_buf, long long* jobs_rec) {
    const int n_iter = wsel ? n_sel : n_windows;
    if (n_iter <= 0) return 0;
    // need_buf: 12 * n_windows bytes of the caller's (the resident pipeline keeps one; an allocation and a release per call cost more than the
    // filter's own device work on a small batch), else allocated here
    int* need = need_buf;
    if (!need && hipMalloc((void**)&need, 12 * (size_t)n_windows) != hipSuccess) { *err = "device allocation failed (predict)"; return -6; }
    struct Free { int* p; int* a = nullptr; int* b = nullptr; unsigned char* f = nullptr; ~Free() { if (p) (void)hipFree(p); if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (f) (void)hipFree(f); } } guard{need_buf ? nullptr : need};
    if (hipMemsetAsync(need, 0, 12 * (size_t)n_windows, stream) != hipSuccess) { *err = "memset failed"; return -2; }
#ifndef MIRP_PRED_GRID
#define MIRP_PRED_GRID 64
#endif
    const int grid = std::min(n_iter, n_cu * MIRP_PRED_GRID);
    if (jobs_rec) { jobs_rec[0]++; jobs_rec[1] = std::max(jobs_rec[1], ((long long)n_iter + grid - 1) / grid); }
    if (launch_predict(stream, grid, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, out, n_out, status, rcount, rpool, rcap, rstride,
                       wsel, n_sel, skip, nullptr, nullptr, need) != hipSuccess) { *err = "predict kernel launch failed"; return -2; }
    std::vector<int> h_status((size_t)n_windows), h_sel, h_skip;
    unsigned int n1 = 0;
    if (hipMemcpyAsync(h_status.data(), status, 4 * (size_t)n_windows, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        (rcount && hipMemcpyAsync(&n1, rcount, 4, hipMemcpyDeviceToHost, stream) != hipSuccess) || hipStreamSynchronize(stream) != hipSuccess) {
        *err = "predict kernel execution failed"; return -2;
    }
#ifdef MIRP_DIAG
    if (std::getenv("MIRP_PREDICT_CLOCKS")) predict_clocks_print();
#endif
    if (wsel) { h_sel.resize((size_t)n_sel); if (hipMemcpy(h_sel.data(), wsel, 4 * (size_t)n_sel, hipMemcpyDeviceToHost) != hipSuccess) { *err = "D2H failed"; return -2; } }
    else if (skip) { h_skip.resize((size_t)n_windows); if (hipMemcpy(h_skip.data(), skip, 4 * (size_t)n_windows, hipMemcpyDeviceToHost) != hipSuccess) { *err = "D2H failed"; return -2; } }
    std::vector<int> rw, rs;          // windows to run again, their slots
    for (int it = 0; it < n_iter; it++) {
        const int w = wsel ? h_sel[(size_t)it] : it;
        if (!wsel && skip && h_skip[(size_t)it] >= 0) continue;
        if (h_status[(size_t)w] == 2 || h_status[(size_t)w] == 3) { rw.push_back(w); rs.push_back(it); }
    }
    if (rw.empty()) return 0;
    std::vector<MirpWindow> h_w((size_t)n_windows);
    if (hipMemcpy(h_w.data(), windows, sizeof(MirpWindow) * (size_t)n_windows, hipMemcpyDeviceToHost) != hipSuccess) { *err = "D2H failed"; return -2; }
    if (hipMalloc((void**)&guard.a, 4 * rw.size()) != hipSuccess || hipMalloc((void**)&guard.b, 4 * rw.size()) != hipSuccess) { *err = "device allocation failed (predict)"; return -6; }
    // (not gated on the first pass's record count: a re-run round can write the first records of a window that the next round voids)
    if (rpool && hipMalloc((void**)&guard.f, (size_t)n_windows) != hipSuccess) { *err = "device allocation failed (predict)"; return -6; }
    PredictCaps caps = predict_default_caps(max_lines, ss_stride);
    std::vector<int> h_need(3 * (size_t)n_windows);
    // A flagged window says what it needs (need[]), but what it says can be short of the truth: a line that was not staged contributed neither its
    // structures nor its pieces.  So the windows that are still flagged after a re-run go round again with what they report then; every round
    // stages at least the lines the one before asked for, so the third has seen everything.
    for (int round = 0; round < 3 && !rw.empty(); round++) {
        if (hipMemcpy(h_need.data(), need, 12 * (size_t)n_windows, hipMemcpyDeviceToHost) != hipSuccess) { *err = "D2H failed"; return -2; }
        for (int w : rw) {
            caps.s_cap = std::max(caps.s_cap, h_need[3 * (size_t)w]);
            caps.p_cap = std::max(caps.p_cap, h_need[3 * (size_t)w + 1]);
            caps.l_cap = std::max(caps.l_cap, std::min(h_need[3 * (size_t)w + 2], max_lines));
            caps.m_cap = std::max(caps.m_cap, h_w[(size_t)w].n_matures);
        }
        if (predict_lds_bytes_min(max_lines, ss_stride, caps) > 160 * 1024) {
            *err = "a window has more structures / candidate matures than the filter kernel can hold in LDS (" + std::to_string(caps.s_cap) + " structures, " +
                   std::to_string(caps.m_cap) + " matures)";
            return -5;
        }
        if (hipMemcpy(guard.a, rw.data(), 4 * rw.size(), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(guard.b, rs.data(), 4 * rs.size(), hipMemcpyHostToDevice) != hipSuccess) {
            *err = "H2D failed"; return -2;
        }
        if (rpool) {          // records written so far for the windows of THIS round are void (truncated by a capacity)
            std::vector<unsigned char> fl((size_t)n_windows, 0);
            for (int w : rw) fl[(size_t)w] = 1;
            if (hipMemcpy(guard.f, fl.data(), (size_t)n_windows, hipMemcpyHostToDevice) != hipSuccess) { *err = "H2D failed"; return -2; }
            unsigned int n2 = 0;
            if (hipMemcpy(&n2, rcount, 4, hipMemcpyDeviceToHost) != hipSuccess) { *err = "D2H failed"; return -2; }
            const unsigned int nn = std::min(n2, rcap);
            if (nn > 0)
                hipLaunchKernelGGL(reasons_invalidate_kernel, dim3((nn + 255) / 256 > 4096 ? 4096 : (nn + 255) / 256), dim3(256), 0, stream, rpool, nn, rstride, (const unsigned char*)guard.f);
        }
        const int grid2 = std::min((int)rw.size(), n_cu * 4);
        if (jobs_rec) { jobs_rec[0]++; jobs_rec[1] = std::max(jobs_rec[1], ((long long)rw.size() + grid2 - 1) / grid2); }
        if (launch_predict(stream, grid2, windows, n_windows, matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, out, n_out, status,
                           rcount, rpool, rcap, rstride, guard.a, (int)rw.size(), nullptr, guard.b, &caps, need) != hipSuccess) { *err = "predict kernel launch failed (re-run)"; return -2; }
        if (hipMemcpyAsync(h_status.data(), status, 4 * (size_t)n_windows, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            *err = "predict kernel execution failed (re-run)"; return -2;
        }
        std::vector<int> rw2, rs2;
        for (size_t k = 0; k < rw.size(); k++)
            if (h_status[(size_t)rw[k]] == 2 || h_status[(size_t)rw[k]] == 3) { rw2.push_back(rw[k]); rs2.push_back(rs[k]); }
        rw.swap(rw2); rs.swap(rs2);
    }
    return 0;
}

}  // namespace mirp
