// Device side of the homolog search (mirp_homolog_scan, mirp_homolog.cpp): the placements of short known sequences in the resident
// alignment index within v mismatches, the windows around them and the structure rules of the predict stage on a window and a given interval.
//
//   scan      the seeds of align_kernels.hip (align_device.h: the two halves of the oriented sequence, with v >= 2 also every single-substitution
//             variant of a half), launch_excl_scan over the seed ranges = a flat candidate space, one candidate per thread.  hm_verify_kernel<0>
//             counts the placements of every query (all strata: a candidate within v mismatches counts, from its canonical finder only);
//             hm_cut_kernel drops the queries with more than max_placements; launch_excl_scan gives every query its offset; hm_verify_kernel<1>
//             writes query << 35 | gpos << 3 | strand << 2 | mismatches at these offsets, and mirp_device_sort_u64 by the whole key puts them in
//             (query, contig in reference order, offset, + before -) order.  The keys of the queries [q0, q1] with gpos in [g0, g1) make one pass
//             (pass_plan.h) when all of them exceed the key capacity.
//   windows   hm_winlen_kernel: contig, clipped window and interval of every placement of a chunk; launch_excl_scan; hm_winseq_kernel: the letters
//             on the placement's strand, as the fold reads them.
//   evaluate  homolog_eval_kernel, one wave per window: phase 1 of predict_kernel (the structure list from the fold's lines, staged in LDS at 2 bits
//             per character), then one lane per structure runs get_maturestar_info on the interval; wave reductions find the passing structure of
//             lowest normalised energy and the structure of lowest normalised energy overall, ties to the lowest index.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "align_device.h"
#include "predict_device.h"
#include "pass_plan.h"
#include "site_keys.h"

namespace mirp {

// ---------------------------------------------------------------- scan
__global__ void hm_seedcount_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ roff, long long n, AlParams P, int* __restrict__ cnt) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const unsigned char* rd = codes + roff[r];
        const int L = (int)(roff[r + 1] - roff[r]);
        int c = 0;
        for (int s = 0; s < 2; s++)
            for (int h = 0; h < (P.v ? 2 : 1); h++) {
                int hoff, hlen, bp;
                al_half(L, P.v, h, &hoff, &hlen);
                c += al_nseeds(rd, L, s, hoff, hlen, P.e, &bp);
            }
        cnt[r] = c;
    }
}

// the seeds of every query (all letters are A C G T: the exact half, and with e = 1 its 3 x length single-substitution variants) and their SA ranges
__global__ void hm_seedfill_kernel(AlRef R, const unsigned char* __restrict__ codes, const long long* __restrict__ roff, long long n, AlParams P,
                                   const long long* __restrict__ sscan, AlSeed* __restrict__ seeds, int* __restrict__ ccnt, int* __restrict__ overflow) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const unsigned char* rd = codes + roff[r];
        const int L = (int)(roff[r + 1] - roff[r]);
        long long o = sscan[r];
        for (int s = 0; s < 2; s++)
            for (int h = 0; h < (P.v ? 2 : 1); h++) {
                int hoff, hlen, bp;
                al_half(L, P.v, h, &hoff, &hlen);
                const int ns = al_nseeds(rd, L, s, hoff, hlen, P.e, &bp);
                const int m = hlen < 16 ? hlen : 16;
                for (int k = 0; k < ns; k++) {
                    int vpos = -1, vbase = 0;
                    if (k > 0) {
                        vpos = (k - 1) / 3;
                        const unsigned rb = al_oriented(rd, L, s, hoff + vpos);
                        vbase = (int)((rb + 1 + (k - 1) % 3) & 3u);
                    }
                    unsigned key = 0;
                    for (int i = 0; i < m; i++) key = (key << 2) | (i == vpos ? (unsigned)vbase : al_oriented(rd, L, s, hoff + i));
                    long long lo, hi;
                    al_range(R, key, m, &lo, &hi);
                    AlSeed sd;
                    sd.lo = lo; sd.read = (unsigned)r; sd.strand = (unsigned char)s; sd.half = (unsigned char)h; sd.vbase = (unsigned char)vbase; sd.pad = 0;
                    sd.vpos = vpos;
                    seeds[o] = sd;
                    const long long c = hi - lo;
                    if (c > 0x7fffffffll) { atomicOr(overflow, 1); ccnt[o] = 0x7fffffff; }
                    else ccnt[o] = (int)c;
                    o++;
                }
            }
    }
}

// One candidate of [c0, c1) per thread; its seed comes from a binary search over the seed scan.  PASS 0: placements per query.  PASS 1: the keys of
// the kept queries q0 .. q1 with gpos in [g0, g1) at off[q] - off[q0] (off == nullptr: one query, from 0) + the query's cursor; a key past `cap` is
// not written (its pass is asked again over a shorter range), the cursor counts it all the same.
template <int PASS>
__global__ void hm_verify_kernel(AlRef R, const unsigned char* __restrict__ codes, const long long* __restrict__ roff, const AlSeed* __restrict__ seeds,
                                 long long n_seeds, const long long* __restrict__ cscan, long long c0, long long c1, AlParams P, unsigned* __restrict__ cnt,
                                 const int* __restrict__ slots, const long long* __restrict__ off, long long q0, long long q1, unsigned long long g0,
                                 unsigned long long g1, unsigned* __restrict__ cursor, unsigned long long* __restrict__ out, long long cap) {
    for (long long c = c0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; c < c1; c += (long long)gridDim.x * blockDim.x) {
        long long a = 0, z = n_seeds;                 // last seed with cscan <= c
        while (z - a > 1) { const long long md = (a + z) >> 1; if (cscan[md] <= c) a = md; else z = md; }
        const AlSeed sd = seeds[a];
        const long long q = (long long)sd.read;
        if (PASS == 1 && (q < q0 || q > q1 || slots[q] == 0)) continue;
        const unsigned long long pos = R.sa[sd.lo + (c - cscan[a])];
        const long long rb = roff[q];
        const int L = (int)(roff[q + 1] - rb);
        const int mm = al_check(R, codes + rb, L, sd, pos, P);
        if (mm < 0) continue;
        if (PASS == 0) {
            atomicAdd(&cnt[q], 1u);
        } else {
            int hoff, hlen;
            al_half(L, P.v, sd.half, &hoff, &hlen);
            const unsigned long long g = pos - hoff;
            if (g < g0 || g >= g1) continue;
            const long long slot = (long long)atomicAdd(&cursor[q], 1u) + (off ? off[q] - off[q0] : 0);
            if (slot < cap) out[slot] = ((unsigned long long)q << 35) | (g << 3) | ((unsigned long long)sd.strand << 2) | (unsigned long long)mm;
        }
    }
}

// slots[q] = the placements of query q, 0 when they exceed max_placements; small[0] += placements kept, small[1] += queries dropped
__global__ void hm_cut_kernel(const unsigned* __restrict__ cnt, long long n, int max_placements, int* __restrict__ slots, unsigned long long* __restrict__ small) {
    unsigned long long kept = 0, dropped = 0;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
        const unsigned k = cnt[q];
        const bool over = k > (unsigned)max_placements;
        slots[q] = over ? 0 : (int)k;
        kept += over ? 0 : k;
        dropped += over;
    }
    for (int o = 32; o > 0; o >>= 1) { kept += __shfl_xor(kept, o, 64); dropped += __shfl_xor(dropped, o, 64); }
    if ((threadIdx.x & 63) == 0) { if (kept) atomicAdd(&small[0], kept); if (dropped) atomicAdd(&small[1], dropped); }
}

// ---------------------------------------------------------------- windows
__global__ void hm_winlen_kernel(const unsigned long long* __restrict__ keys, long long n, const long long* __restrict__ roff,
                                 const unsigned long long* __restrict__ cstart, int n_contigs, int precursor_len, HmWin* __restrict__ win, int* __restrict__ lens) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const long long q = (long long)(key >> 35);
        const unsigned long long g = (key >> 3) & 0xffffffffull;
        const int L = (int)(roff[q + 1] - roff[q]);
        const int a = site_contig(cstart, n_contigs, g);
        const long long cs = (long long)cstart[a], ce = (long long)cstart[a + 1];
        const long long F = (precursor_len - L) / 2;
        const long long lo = (long long)g - F > cs ? (long long)g - F : cs, hi = (long long)g + L + F < ce ? (long long)g + L + F : ce;
        HmWin w;
        w.tid = a; w.ws = (int)(lo - cs) + 1; w.we = (int)(hi - cs) + 1; w.m0 = (int)((long long)g - cs) + 1; w.m1 = w.m0 + L;
        w.strand = (int)((key >> 2) & 1); w.query = (int)q; w.mm = (int)(key & 3);
        win[i] = w;
        lens[i] = (int)(hi - lo);
    }
}

// the letters of window i at seqs + offs[i]: the genome's on the plus strand, their reverse complement on the minus strand; N where ambiguous
__global__ void hm_winseq_kernel(AlRef R, const HmWin* __restrict__ win, long long n, const unsigned long long* __restrict__ cstart,
                                 const long long* __restrict__ offs, unsigned char* __restrict__ seqs) {
    const long long total = offs[n];
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < total; x += (long long)gridDim.x * blockDim.x) {
        long long a = 0, z = n;                     // last window with offs <= x
        while (z - a > 1) { const long long md = (a + z) >> 1; if (offs[md] <= x) a = md; else z = md; }
        const HmWin w = win[a];
        const int j = (int)(x - offs[a]), len = w.we - w.ws;
        const unsigned long long g = cstart[w.tid] + (unsigned long long)(w.ws - 1) + (unsigned long long)(w.strand ? len - 1 - j : j);
        const bool amb = (R.amb[g >> 5] >> (g & 31)) & 1u;
        const unsigned b = al_base(R.pk, g);
        seqs[x] = amb ? 'N' : "ACGT"[w.strand ? 3u - b : b];
    }
}

// ---------------------------------------------------------------- evaluate
// Capacities of one launch, as predict_kernel's: p_cap pieces per line, s_cap structures per window, l_cap staged lines per window.  A window that
// needs more is flagged (status 2) with what it needs and run again with capacities sized for it.
struct HmCaps { int p_cap, s_cap, l_cap; };

// wsel == nullptr: the windows [0, n_windows); else the windows wsel[0 .. n_sel).  Window w's fold output is at slot w.  need[3 w] = structures,
// need[3 w + 1] = pieces of one line, need[3 w + 2] = lines to stage that the window has.  gtext != nullptr: the staged text lives in a global
// scratch area of the workgroup instead of LDS.
__global__ void __launch_bounds__(64) homolog_eval_kernel(const HmWin* __restrict__ win, int n_windows, const MirpFoldLine* __restrict__ lines,
                                                          const char* __restrict__ ss, int ss_stride, int max_lines, const int* __restrict__ n_lines,
                                                          int minlen, HmEval* __restrict__ out, char* __restrict__ out_ss,
                                                          const int* __restrict__ wsel, int n_sel, HmCaps caps, int* __restrict__ need,
                                                          unsigned long long* __restrict__ gtext) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int wpl = ssw_words(ss_stride);                                 // 64-bit words per staged line (32 characters each)
    const int max_structs = caps.s_cap, P_CAP = caps.p_cap, L_CAP = caps.l_cap;
    unsigned long long* textw = gtext ? gtext + (size_t)blockIdx.x * L_CAP * wpl : (unsigned long long*)smem;
    PStruct* sts = (PStruct*)(smem + (gtext ? (size_t)0 : (((size_t)L_CAP * wpl * 8 + 15) & ~(size_t)15)));   // s_cap
    PStruct* slot = sts + max_structs;                                    // 64 * p_cap
    int* cnts = (int*)(slot + 64 * P_CAP);                                // 64
    unsigned short* lslot = (unsigned short*)(cnts + 64);                 // max_lines: staged slot of a line, 0xffff = not staged
    unsigned short* lline = lslot + max_lines;                            // l_cap: line of a staged slot
    const int lane = threadIdx.x;
    const int n_iter = wsel ? n_sel : n_windows;
    for (int it = blockIdx.x; it < n_iter; it += gridDim.x) {
        const int w = wsel ? wsel[it] : it;
        const HmWin W = win[w];
        const int nl = n_lines[w] < max_lines ? n_lines[w] : max_lines;
        const MirpFoldLine* wl = lines + (size_t)w * max_lines;
        int st_flag = 0, need_pieces = 0;
        // which lines are staged: the printed ones of at least minlen characters (MP:1568-1570), in line order
        int n_used = 0;
        for (int lb = 0; lb < nl; lb += 64) {
            const int k = lb + lane;
            bool used = false;
            if (k < nl) { const MirpFoldLine ln = wl[k]; used = ln.printed && ln.len >= minlen; }
            const unsigned long long bal = __ballot(used);
            const int u = n_used + (int)__popcll(bal & ((1ull << lane) - 1ull));
            if (k < nl) lslot[k] = (used && u < L_CAP) ? (unsigned short)u : (unsigned short)0xffff;
            if (used && u < L_CAP) lline[u] = (unsigned short)k;
            if (used && u >= L_CAP) st_flag = 2;
            n_used += (int)__popcll(bal);
        }
        __syncthreads();
        // stage their text as '(' and ')' bit planes (lane = one word = 32 characters)
        {
            const char* src = ss + (size_t)w * max_lines * ss_stride;
            const int nu = n_used < L_CAP ? n_used : L_CAP;
            for (int x = lane; x < nu * wpl; x += 64) {
                const int us = x / wpl, wi = x - us * wpl, ln = lline[us];
                textw[x] = d_stage_word(src + (size_t)ln * ss_stride, ss_stride, wi);
            }
        }
        __syncthreads();
        // ---- phase 1: structures (lane per line, chunks of 64 lines), as predict_kernel's
        int nst = 0;
        for (int lb = 0; lb < nl; lb += 64) {
            int k = lb + lane, cnt = 0;
            if (k < nl) {
                MirpFoldLine ln = wl[k];
                const int us = lslot[k];
                SSW s; s.w = textw + (size_t)(us == 0xffff ? 0 : us) * wpl; s.o = 0;
                if (ln.printed && ln.len >= minlen && us != 0xffff) {
                    if (ssw_is_stem_loop(s, ln.len)) {
                        PStruct p; p.line = (unsigned short)k; p.off = 0; p.len = (unsigned short)ln.len; p.type = 0;
                        slot[lane * P_CAP + cnt++] = p;
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
                                        if (cnt < P_CAP) {
                                            PStruct p; p.line = (unsigned short)k; p.off = (unsigned short)ps; p.len = (unsigned short)pl; p.type = (unsigned short)type;
                                            slot[lane * P_CAP + cnt++] = p;
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
            cnts[lane] = cnt;
            __syncthreads();
            // ordered compaction (line order, piece order)
            int base = nst;
            for (int l = 0; l < 64; l++) { if (l < lane) base += cnts[l]; }
            for (int c = 0; c < cnt; c++) { if (base + c < max_structs) sts[base + c] = slot[lane * P_CAP + c]; else st_flag = 2; }
            int tot = 0;
            for (int l = 0; l < 64; l++) tot += cnts[l];
            nst += tot;
            __syncthreads();
        }
        {          // what this window needs, for the re-run of flagged windows: structures in all, pieces of its richest line, lines to stage
            int np = need_pieces;
            for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(np, o); np = t > np ? t : np; }
            if (lane == 0) { need[3 * (size_t)w] = nst; need[3 * (size_t)w + 1] = np; need[3 * (size_t)w + 2] = n_used; }
        }
        const int nst_all = nst;
        if (nst > max_structs) nst = max_structs;
        // ---- phase 2: lane per structure on the interval; every lane keeps its own lowest normalised energy (its s only grows, so the first of
        // equals stays), once among the structures that pass and once among all
        double p_ne = 0.0, a_ne = 0.0;
        int p_s = -1, a_s = -1, a_code = 0;
        MStar p_ms;
        p_ms.code = 0; p_ms.star_s = p_ms.star_e = p_ms.fold_s = p_ms.fold_e = 0;
        for (int sb = 0; sb < nst; sb += 64) {
            const int s = sb + lane;
            if (s < nst) {
                const PStruct p = sts[s];
                const MirpFoldLine ln = wl[p.line];
                const double ne = ((double)ln.energy / 100.0) / (double)ln.len;
                SSW str; str.w = textw + (size_t)lslot[p.line] * wpl; str.o = p.off;
                MStar ms;
                ssw_maturestar(str, p.len, W.m0, W.m1, ln.start + p.off, W.ws, W.we, W.strand, ms);
                if (a_s < 0 || ne < a_ne) { a_ne = ne; a_s = s; a_code = ms.code; }
                if (ms.code == 0 && (p_s < 0 || ne < p_ne)) { p_ne = ne; p_s = s; p_ms = ms; }
            }
        }
        // wave arg-min over (ne ascending, s ascending) among the lanes that have a candidate
        double r_ne = p_ne, q_ne = a_ne;
        int r_s = p_s, q_s = a_s, q_code = a_code;
        for (int o = 32; o > 0; o >>= 1) {
            const double t_ne = __shfl_xor(r_ne, o);
            const int t_s = __shfl_xor(r_s, o);
            if (t_s >= 0 && (r_s < 0 || t_ne < r_ne || (t_ne == r_ne && t_s < r_s))) { r_ne = t_ne; r_s = t_s; }
            const double u_ne = __shfl_xor(q_ne, o);
            const int u_s = __shfl_xor(q_s, o), u_code = __shfl_xor(q_code, o);
            if (u_s >= 0 && (q_s < 0 || u_ne < q_ne || (u_ne == q_ne && u_s < q_s))) { q_ne = u_ne; q_s = u_s; q_code = u_code; }
        }
        int f = st_flag;
        for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(f, o); f = t > f ? t : f; }
        if (r_s >= 0) {
            const PStruct bp = sts[r_s];
            const char* src = ss + ((size_t)w * max_lines + bp.line) * ss_stride + bp.off;
            char* dst = out_ss + (size_t)w * ss_stride;
            for (int j = lane; j < (int)bp.len; j += 64) dst[j] = src[j];
        }
        if (r_s >= 0 ? p_s == r_s : lane == 0) {          // exactly one lane writes the record: the winner's owner, or lane 0 without a winner
            HmEval e = {};
            e.n_structs = nst_all; e.best = r_s; e.code = r_s >= 0 ? 0 : q_s >= 0 ? q_code : -1; e.status = f;
            if (r_s >= 0) {
                const PStruct bp = sts[r_s];
                const MirpFoldLine ln = wl[bp.line];
                SSW str; str.w = textw + (size_t)lslot[bp.line] * wpl; str.o = bp.off;
                const int fst = ln.start + bp.off;
                const int l0 = W.strand == 0 ? W.m0 - W.ws - fst + 1 : W.we - W.m1 - fst + 1, l1 = l0 + (W.m1 - W.m0);
                ssw_duplex_stats(str, bp.len, l0, l1, &e.prime5, &e.total_bps, &e.total_dots);
                e.star_s = p_ms.star_s; e.star_e = p_ms.star_e; e.fold_s = p_ms.fold_s; e.fold_e = p_ms.fold_e;
                e.energy = ln.energy; e.line_len = ln.len; e.ss_len = bp.len;
            }
            out[w] = e;
        }
        __syncthreads();
    }
}

static size_t hm_eval_lds(int max_lines, int ss_stride, HmCaps caps, bool text_in_lds) {
    size_t b = text_in_lds ? (((size_t)caps.l_cap * ssw_words(ss_stride) * 8 + 15) & ~(size_t)15) : 0;
    b += sizeof(PStruct) * ((size_t)caps.s_cap + 64 * (size_t)caps.p_cap);
    b += sizeof(int) * 64;
    b += sizeof(unsigned short) * ((size_t)max_lines + (size_t)caps.l_cap);
    return (b + 15) & ~(size_t)15;
}

}  // namespace mirp

using namespace mirp;

static inline int hm_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

static AlRef hm_ref(const mirp_ctx* c) {
    return AlRef{(const unsigned*)c->a_pk.p, (const unsigned*)c->a_amb.p, (const unsigned*)c->a_cst.p, (const unsigned*)c->a_sa.p,
                 (const long long*)c->a_bkt.p, (unsigned long long)c->a_total};
}

// The placements of the nq queries (codes 0..3 at roff[0 .. nq]) in output order, as keys.  stats: [0] placements kept, [1] queries dropped by
// max_placements, [2] key passes.
int mirp_device_homolog_scan(mirp_ctx* c, const unsigned char* codes, const long long* roff, long long nq, int v, int max_placements,
                             std::vector<unsigned long long>& keys, long long stats[3]) {
    keys.clear();
    stats[0] = stats[1] = stats[2] = 0;
    if (!c->a_ready) return fail(c, -1, "mirp_homolog_scan: no index (mirp_align_index first)");
    if (nq <= 0) return 0;
    hipStream_t st = c->stream;
    const AlParams P{v, v / 2, 0, max_placements, 0};
    const AlRef R = hm_ref(c);
    const long long nb = roff[nq];
    if (c->a_codes.ensure((size_t)nb + 16) || c->a_roff.ensure(8 * (size_t)(nq + 1)) || c->a_small.ensure(64) || c->a_rcnt.ensure(4 * (size_t)nq) ||
        c->a_rscan.ensure(8 * (size_t)(nq + 1)))
        return fail(c, -6, "device allocation failed (homologs: queries)");
    HIPCHK(c, hipMemcpyAsync(c->a_codes.p, codes, (size_t)nb, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->a_roff.p, roff, 8 * (size_t)(nq + 1), hipMemcpyHostToDevice, st));
    unsigned long long* d_small = (unsigned long long*)c->a_small.p;    // [0] placements kept, [1] queries dropped, [4] overflow flag
    HIPCHK(c, hipMemsetAsync(d_small, 0, 64, st));
    const unsigned char* d_codes = (const unsigned char*)c->a_codes.p;
    const long long* d_roff = (const long long*)c->a_roff.p;
    const int g = hm_grid(nq);
    // ---- seeds
    long long* d_rscan = (long long*)c->a_rscan.p;
    hipLaunchKernelGGL(hm_seedcount_kernel, dim3(g), dim3(256), 0, st, d_codes, d_roff, nq, P, (int*)c->a_rcnt.p);
    launch_excl_scan(st, (const int*)c->a_rcnt.p, d_rscan, nq);
    std::vector<long long> h_rscan((size_t)nq + 1);
    HIPCHK(c, hipMemcpyAsync(h_rscan.data(), d_rscan, 8 * (size_t)(nq + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const long long S = h_rscan[(size_t)nq];
    if (c->a_seeds.ensure(sizeof(AlSeed) * (size_t)std::max<long long>(S, 1)) || c->a_ccnt.ensure(4 * (size_t)std::max<long long>(S, 1)) ||
        c->a_cscan.ensure(8 * (size_t)(S + 1)))
        return fail(c, -6, "device allocation failed (homologs: seeds)");
    AlSeed* d_seeds = (AlSeed*)c->a_seeds.p;
    long long* d_cscan = (long long*)c->a_cscan.p;
    hipLaunchKernelGGL(hm_seedfill_kernel, dim3(g), dim3(256), 0, st, R, d_codes, d_roff, nq, P, (const long long*)d_rscan, d_seeds, (int*)c->a_ccnt.p,
                       (int*)(d_small + 4));
    if (S > 0) launch_excl_scan(st, (const int*)c->a_ccnt.p, d_cscan, S);
    else HIPCHK(c, hipMemsetAsync(d_cscan, 0, 8, st));
    std::vector<long long> h_cscan((size_t)S + 1);
    unsigned long long ovf = 0;
    HIPCHK(c, hipMemcpyAsync(&ovf, d_small + 4, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_cscan.data(), d_cscan, 8 * (size_t)(S + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (ovf) return fail(c, -5, "a seed matches 2^31 or more index positions");
    const long long TC = h_cscan[(size_t)S];
    // ---- count, cut, offsets
    if (c->a_lvl.ensure(4 * (size_t)nq) || c->a_slots.ensure(4 * (size_t)nq) || c->a_off.ensure(8 * (size_t)(nq + 1)) || c->a_cursor.ensure(4 * (size_t)nq))
        return fail(c, -6, "device allocation failed (homologs: counts)");
    unsigned* d_cnt = (unsigned*)c->a_lvl.p;
    int* d_slots = (int*)c->a_slots.p;
    long long* d_off = (long long*)c->a_off.p;
    unsigned* d_cursor = (unsigned*)c->a_cursor.p;
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, 4 * (size_t)nq, st));
    if (TC > 0)
        hipLaunchKernelGGL(hm_verify_kernel<0>, dim3(hm_grid(TC)), dim3(256), 0, st, R, d_codes, d_roff, (const AlSeed*)d_seeds, S, (const long long*)d_cscan, 0ll, TC, P,
                           d_cnt, (const int*)nullptr, (const long long*)nullptr, 0ll, 0ll, 0ull, 0ull, (unsigned*)nullptr, (unsigned long long*)nullptr, 0ll);
    hipLaunchKernelGGL(hm_cut_kernel, dim3(g), dim3(256), 0, st, (const unsigned*)d_cnt, nq, max_placements, d_slots, d_small);
    launch_excl_scan(st, (const int*)d_slots, d_off, nq);
    std::vector<int> h_slots((size_t)nq);
    unsigned long long sm[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h_slots.data(), d_slots, 4 * (size_t)nq, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(sm, d_small, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    stats[0] = (long long)sm[0];
    stats[1] = (long long)sm[1];
    if (sm[0] == 0) return 0;
    // ---- key passes
    const long long cap = c->hm_cap > 0 ? c->hm_cap : (1ll << 24);
    const long long buf = std::min<long long>(cap, (long long)sm[0]);
    if (c->a_items.ensure(8 * (size_t)buf) || c->a_itmp.ensure(8 * (size_t)buf)) return fail(c, -6, "device allocation failed (homologs: keys)");
    unsigned long long* d_keys = (unsigned long long*)c->a_items.p;
    int qbits = 0;
    while ((1ll << qbits) < nq) qbits++;
    const int sort_bits = std::min(64, (35 + qbits + 7) / 8 * 8);
    try { keys.reserve((size_t)sm[0]); } catch (...) { return fail(c, -7, "host allocation failed (homologs: keys)"); }
    // one pass: the candidates of the queries q0 .. q1 whose position lies in [g0, g1); *got = the keys it found (those beyond `cap` are not kept)
    auto pass = [&](long long q0, long long q1, unsigned long long g0, unsigned long long g1, bool by_offsets, long long* got) -> int {
        const long long c0 = h_cscan[(size_t)h_rscan[(size_t)q0]], c1 = h_cscan[(size_t)h_rscan[(size_t)q1 + 1]];
        HIPCHK(c, hipMemsetAsync(d_cursor + q0, 0, 4 * (size_t)(q1 - q0 + 1), st));
        if (c1 > c0)
            hipLaunchKernelGGL(hm_verify_kernel<1>, dim3(hm_grid(c1 - c0)), dim3(256), 0, st, R, d_codes, d_roff, (const AlSeed*)d_seeds, S, (const long long*)d_cscan, c0,
                               c1, P, (unsigned*)nullptr, (const int*)d_slots, by_offsets ? (const long long*)d_off : (const long long*)nullptr, q0, q1, g0, g1, d_cursor,
                               d_keys, buf);
        long long n = 0;
        if (by_offsets) {
            for (long long q = q0; q <= q1; q++) n += h_slots[(size_t)q];
        } else {
            unsigned k = 0;
            HIPCHK(c, hipMemcpyAsync(&k, d_cursor + q0, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            n = (long long)k;
        }
        *got = n;
        stats[2]++;
        if (n > buf || n == 0) return 0;
        if (int rc = mirp_device_sort_u64(c, d_keys, (unsigned long long*)c->a_itmp.p, n, 0, sort_bits)) return rc;
        const size_t at = keys.size();
        keys.resize(at + (size_t)n);
        HIPCHK(c, hipMemcpyAsync(keys.data() + at, d_keys, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        return 0;
    };
    const int rc = plan_passes(
        nq, [&](long long q) { return (long long)h_slots[(size_t)q]; }, buf, (unsigned long long)c->a_total,
        [&](long long first, long long last, long long) -> int { long long got = 0; return pass(first, last, 0ull, ~0ull, true, &got); },
        [&](long long q, unsigned long long lo, unsigned long long hi, long long* got) -> int { return pass(q, q, lo, hi, false, got); });
    if (rc == PLAN_POSITION_OVER_CAP) return fail(c, -5, "mirp_homolog_scan: the key capacity is smaller than the placements at one position");
    return rc;
}

// Windows, fold and evaluation of the n placements keys[0 .. n): win[i], ev[i] and, for a placement with a passing structure, at text[text_off[i]]
// the we - ws letters of its window on its strand followed by the ev[i].ss_len characters of the structure.  max_lines: structure lines the fold keeps per window at first; a chunk with a window that needs more
// is folded again with room for it.  stats += {fold chunks, evaluation re-runs, folds repeated for more lines, evaluation launches with the staged
// text in global memory}; seconds += {windows, fold, evaluation + download}.
int mirp_device_homolog_eval(mirp_ctx* c, const unsigned long long* keys, long long n, int precursor_len, int max_lines, HmWin* win, HmEval* ev,
                             std::vector<char>& text, long long* text_off, long long stats[4], double seconds[3]) {
    if (n <= 0) return 0;
    hipStream_t st = c->stream;
    const AlRef R = hm_ref(c);
    const int ni = (int)n;
    double t = mirp::now();
    if (c->hm_keys.ensure(8 * (size_t)n) || c->hm_win.ensure(sizeof(HmWin) * (size_t)n) || c->hm_lens.ensure(4 * (size_t)n) || c->hm_offs.ensure(8 * (size_t)(n + 1)))
        return fail(c, -6, "device allocation failed (homologs: windows)");
    HIPCHK(c, hipMemcpyAsync(c->hm_keys.p, keys, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HmWin* d_win = (HmWin*)c->hm_win.p;
    long long* d_offs = (long long*)c->hm_offs.p;
    hipLaunchKernelGGL(hm_winlen_kernel, dim3(hm_grid(n)), dim3(256), 0, st, (const unsigned long long*)c->hm_keys.p, n, (const long long*)c->a_roff.p,
                       (const unsigned long long*)c->a_cstart.p, c->a_n_contigs, precursor_len, d_win, (int*)c->hm_lens.p);
    launch_excl_scan(st, (const int*)c->hm_lens.p, d_offs, n);
    std::vector<long long> h_offs((size_t)n + 1);
    HIPCHK(c, hipMemcpyAsync(win, d_win, sizeof(HmWin) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_offs.data(), d_offs, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const long long total = h_offs[(size_t)n];
    if (c->hm_seqs.ensure((size_t)total + 16)) return fail(c, -6, "device allocation failed (homologs: window letters)");
    if (total > 0)
        hipLaunchKernelGGL(hm_winseq_kernel, dim3(hm_grid(total)), dim3(256), 0, st, R, (const HmWin*)d_win, n, (const unsigned long long*)c->a_cstart.p,
                           (const long long*)d_offs, (unsigned char*)c->hm_seqs.p);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    int n_max = 1;
    for (long long i = 0; i < n; i++) n_max = std::max(n_max, (int)(h_offs[(size_t)i + 1] - h_offs[(size_t)i]));
    seconds[0] += mirp::now() - t;
    const int stride = ((n_max + 3 + 7) / 8) * 8;
    std::vector<int> h_status((size_t)n), h_nl((size_t)n);
    for (;;) {
        // ---- fold: the output stays on the device for the evaluation
        t = mirp::now();
        const size_t per_win = (size_t)max_lines * stride;
        if (c->blines.ensure(sizeof(MirpFoldLine) * (size_t)n * max_lines) || c->bss.ensure((size_t)n * per_win) || c->bnlines.ensure(4 * (size_t)n) ||
            c->bmfe.ensure(4 * (size_t)n) || c->bstatus.ensure(4 * (size_t)n))
            return fail(c, -6, "device allocation failed (homologs: fold output)");
        if (int rc = mirp_run_fold(c, (const unsigned char*)c->hm_seqs.p, (const long long*)d_offs, nullptr, ni, n_max, precursor_len, max_lines, stride,
                                   (MirpFoldLine*)c->blines.p, (char*)c->bss.p, (int*)c->bnlines.p, (int*)c->bmfe.p, (int*)c->bstatus.p))
            return rc;
        HIPCHK(c, hipMemcpyAsync(h_status.data(), c->bstatus.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_nl.data(), c->bnlines.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        seconds[1] += mirp::now() - t;
        stats[0]++;
        int more = 0;
        for (long long i = 0; i < n; i++) {
            if (h_status[(size_t)i] < 0) return fail(c, -2, "mirp_homolog_scan: the fold of a window failed (status " + std::to_string(h_status[(size_t)i]) + ")");
            if (h_status[(size_t)i] == 1) more = std::max(more, h_nl[(size_t)i]);
        }
        if (!more) break;
        if (more <= max_lines) return fail(c, -2, "mirp_homolog_scan: a window is flagged for more structure lines than it reports");
        max_lines = more;
        stats[2]++;
    }
    // ---- evaluation
    t = mirp::now();
    if (c->hm_eval.ensure(sizeof(HmEval) * (size_t)n) || c->hm_ss.ensure((size_t)n * stride) || c->hm_need.ensure(12 * (size_t)n) ||
        c->hm_sel.ensure(4 * (size_t)n))
        return fail(c, -6, "device allocation failed (homologs: evaluation)");
    HmCaps caps;
    caps.p_cap = std::max(6, stride / 56 + 1);
    caps.s_cap = std::max(2 * max_lines, 192);
    caps.l_cap = std::min(max_lines, 48);
    if (c->hm_eval_caps[0] > 0) { caps.p_cap = c->hm_eval_caps[0]; caps.s_cap = c->hm_eval_caps[1]; caps.l_cap = std::min(max_lines, c->hm_eval_caps[2]); }
    HIPCHK(c, hipMemsetAsync(c->hm_need.p, 0, 12 * (size_t)n, st));
    std::vector<int> sel;
    std::vector<int> h_need;
    for (int round = 0;; round++) {
        const int n_iter = round ? (int)sel.size() : ni;
        size_t lds = hm_eval_lds(max_lines, stride, caps, true);
        unsigned long long* gtext = nullptr;
        TmpDevice T;
        int grid = std::min(n_iter, c->n_cu * 32);
        if (lds > 160 * 1024) {          // the staged text does not fit in LDS: a scratch area per workgroup in global memory
            lds = hm_eval_lds(max_lines, stride, caps, false);
            if (lds > 160 * 1024) return fail(c, -5, "mirp_homolog_scan: a window has more structures than the evaluation kernel can hold in LDS");
            const size_t per = (size_t)caps.l_cap * ssw_words(stride) * 8;
            grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)1 << 30) / std::max<size_t>(per, 1)));
            gtext = (unsigned long long*)T.get(per * (size_t)grid + 16);
            if (!gtext) return fail(c, -6, "device allocation failed (homologs: staged text)");
            stats[3]++;
        }
        c->note_jobs_per_slot(3, n_iter, grid);
        if (lds > 64 * 1024) HIPCHK(c, hipFuncSetAttribute((const void*)homolog_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(homolog_eval_kernel, dim3(grid), dim3(64), lds, st, (const HmWin*)d_win, ni, (const MirpFoldLine*)c->blines.p, (const char*)c->bss.p, stride,
                           max_lines, (const int*)c->bnlines.p, 55, (HmEval*)c->hm_eval.p, (char*)c->hm_ss.p, round ? (const int*)c->hm_sel.p : (const int*)nullptr,
                           n_iter, caps, (int*)c->hm_need.p, gtext);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(ev, c->hm_eval.p, sizeof(HmEval) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        sel.clear();
        for (long long i = 0; i < n; i++)
            if (ev[i].status == 2) sel.push_back((int)i);
        if (sel.empty()) break;
        // A flagged window says what it needs, but a line that was not staged contributed neither its structures nor its pieces: the windows still
        // flagged after a re-run go round again with what they report then; every round stages at least the lines the one before asked for.
        if (round == 3) return fail(c, -2, "mirp_homolog_scan: a window is still over the evaluation kernel's capacities after three re-runs");
        h_need.resize(3 * (size_t)n);
        HIPCHK(c, hipMemcpy(h_need.data(), c->hm_need.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
        for (int w : sel) {
            caps.s_cap = std::max(caps.s_cap, h_need[3 * (size_t)w]);
            caps.p_cap = std::max(caps.p_cap, h_need[3 * (size_t)w + 1]);
            caps.l_cap = std::max(caps.l_cap, std::min(h_need[3 * (size_t)w + 2], max_lines));
        }
        HIPCHK(c, hipMemcpy(c->hm_sel.p, sel.data(), 4 * sel.size(), hipMemcpyHostToDevice));
        stats[1]++;
    }
    // the letters and the structure text of the windows with a passing structure
    std::vector<char> h_ss((size_t)n * stride), h_seqs((size_t)total);
    HIPCHK(c, hipMemcpy(h_ss.data(), c->hm_ss.p, h_ss.size(), hipMemcpyDeviceToHost));
    if (total > 0) HIPCHK(c, hipMemcpy(h_seqs.data(), c->hm_seqs.p, (size_t)total, hipMemcpyDeviceToHost));
    for (long long i = 0; i < n; i++) {
        text_off[i] = (long long)text.size();
        if (ev[i].best < 0) continue;
        text.insert(text.end(), h_seqs.begin() + h_offs[(size_t)i], h_seqs.begin() + h_offs[(size_t)i + 1]);
        text.insert(text.end(), h_ss.begin() + (size_t)i * stride, h_ss.begin() + (size_t)i * stride + ev[i].ss_len);
    }
    seconds[2] += mirp::now() - t;
    return 0;
}
