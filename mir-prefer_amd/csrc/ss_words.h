// The structure rules of the predict stage on words instead of characters: the structure list of a window (a8, MP:1541-1724) and get_maturestar_info with
// its duplex rules (a9, MP:1727-1999), shared by predict_kernel.hip and homolog_kernels.hip.  No dependencies: the header compiles under hipcc (host and
// device) and under a plain host compiler, which is how tests/tools/ss_words_check.cpp compares every rule with its character-by-character restatement.
//
// Staged text: a line is a row of 64-bit words, word j = the characters 32 j .. 32 j + 31, the low half their '(' bits, the high half their ')' bits
// (two 1-bit planes, interleaved per 32 characters so that one 8-byte read fetches both).  A line of n characters takes 8 ceil(n / 32) bytes -- 80 at 300
// characters, against 76 at 2 bits per character in 32-bit words -- and find / rfind / count are a mask and one ctz / clz / popcount per 32 characters.
// No rule reads memory per character; where a rule is sequential (the partner walk inside the word where the depth returns to zero, the bifurcation state
// machine) it walks the set bits of a word it holds in registers.  '.' does not change any rule's state, so those walks skip it.
// A view (SSW) is a row and a character offset: index 0 is the view's start.  Every rule masks the bits outside [0, len) of its view and reads no word
// that holds none of the view's characters.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSW_HD __host__ __device__ inline
#define SSW_HD_SMALL __host__ __device__ __attribute__((always_inline)) inline
#else
#define SSW_HD inline
#define SSW_HD_SMALL inline
#endif
#ifndef SSW_PATH_HIT          // the check program counts the two paths of the duplex rule through this
#define SSW_PATH_HIT(k)
#endif

namespace mirp {

struct SSW {
    const unsigned long long* w;
    int o;
    SSW_HD_SMALL SSW operator+(int d) const { SSW r; r.w = w; r.o = o + d; return r; }
};

SSW_HD_SMALL int ssw_words(int n_chars) { return (n_chars + 31) >> 5; }          // 64-bit words of a row of n_chars characters
SSW_HD_SMALL int ssw_popc(unsigned v) { return __builtin_popcount(v); }
SSW_HD_SMALL int ssw_ctz(unsigned v) { return __builtin_ctz(v); }                 // v != 0
SSW_HD_SMALL int ssw_top(unsigned v) { return 31 - __builtin_clz(v); }            // v != 0

// Staging: the '(' and ')' bits of four characters (one 32-bit read of the text), at bit q of the word's planes.
SSW_HD_SMALL void ssw_pack4(unsigned four, int q, unsigned& op, unsigned& cl) {
    for (int b = 0; b < 4; b++) {
        const unsigned ch = (four >> (8 * b)) & 0xffu;
        op |= (ch == '(' ? 1u : 0u) << (q + b);
        cl |= (ch == ')' ? 1u : 0u) << (q + b);
    }
}
SSW_HD_SMALL unsigned long long ssw_word(unsigned op, unsigned cl) { return (unsigned long long)op | ((unsigned long long)cl << 32); }

// word j of the row, masked to the absolute character range [A, B), which word j must intersect; m = the mask itself
SSW_HD_SMALL void ssw_load(SSW s, int j, int A, int B, unsigned& op, unsigned& cl, unsigned& m) {
    const unsigned long long v = s.w[j];
    const int lo = A - 32 * j, hi = B - 32 * j;
    m = (hi >= 32 ? 0xffffffffu : (1u << hi) - 1u) & (lo <= 0 ? 0xffffffffu : ~((1u << lo) - 1u));
    op = (unsigned)v & m;
    cl = (unsigned)(v >> 32) & m;
}
SSW_HD_SMALL unsigned ssw_pick(char c, unsigned op, unsigned cl, unsigned m) { return c == '(' ? op : (c == ')' ? cl : m & ~(op | cl)); }

// n <= 32 characters from index pos of the view (n >= 1), at bit 0
SSW_HD_SMALL void ssw_fetch(SSW s, int pos, int n, unsigned& op, unsigned& cl) {
    const int K = s.o + pos, j = K >> 5, sh = K & 31;
    unsigned long long v = s.w[j];
    op = (unsigned)v >> sh;
    cl = (unsigned)(v >> 32) >> sh;
    if (sh + n > 32) {
        v = s.w[j + 1];
        op |= (unsigned)v << (32 - sh);
        cl |= (unsigned)(v >> 32) << (32 - sh);
    }
    const unsigned m = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    op &= m; cl &= m;
}

// str.find / str.rfind / str.count of one character over [a, b), 0 <= a, b <= the view's length; an empty range gives -1 / -1 / 0
SSW_HD int ssw_find(SSW s, char c, int a, int b) {
    if (a >= b) return -1;
    const int A = s.o + a, B = s.o + b;
    for (int j = A >> 5; j <= (B - 1) >> 5; j++) {
        unsigned op, cl, m;
        ssw_load(s, j, A, B, op, cl, m);
        const unsigned sel = ssw_pick(c, op, cl, m);
        if (sel) return 32 * j + ssw_ctz(sel) - s.o;
    }
    return -1;
}
SSW_HD int ssw_rfind(SSW s, char c, int a, int b) {
    if (a >= b) return -1;
    const int A = s.o + a, B = s.o + b;
    for (int j = (B - 1) >> 5; j >= A >> 5; j--) {
        unsigned op, cl, m;
        ssw_load(s, j, A, B, op, cl, m);
        const unsigned sel = ssw_pick(c, op, cl, m);
        if (sel) return 32 * j + ssw_top(sel) - s.o;
    }
    return -1;
}
SSW_HD int ssw_count(SSW s, char c, int a, int b) {
    if (a >= b) return 0;
    const int A = s.o + a, B = s.o + b;
    int n = 0;
    for (int j = A >> 5; j <= (B - 1) >> 5; j++) {
        unsigned op, cl, m;
        ssw_load(s, j, A, B, op, cl, m);
        n += ssw_popc(ssw_pick(c, op, cl, m));
    }
    return n;
}
SSW_HD_SMALL void ssw_clip(int len, int& a, int& b) {   // Python slice bounds
    if (a < 0) { a += len; if (a < 0) a = 0; }
    if (b < 0) { b += len; if (b < 0) b = 0; }
    if (a > len) a = len;
    if (b > len) b = len;
}

// partner of the bracket at x inside s[0, len); -1 if unmatched, if s[x] is '.' or if x lies outside.  A depth walk per word: a word whose closes cannot
// bring the depth to zero is two popcounts, the word where it can is walked bracket by bracket in registers.
SSW_HD int ssw_partner(SSW s, int len, int x) {
    if (x < 0 || x >= len) return -1;
    const int A = s.o, B = s.o + len, X = s.o + x, j0 = X >> 5;
    const unsigned long long v0 = s.w[j0];
    const unsigned bit = 1u << (X & 31);
    int depth = 0;
    if ((unsigned)v0 & bit) {
        for (int j = j0; j <= (B - 1) >> 5; j++) {
            unsigned p, q, m;
            ssw_load(s, j, X, B, p, q, m);
            const int nq = ssw_popc(q);
            if (depth - nq > 0) { depth += ssw_popc(p) - nq; continue; }
            for (unsigned r = p | q; r; r &= r - 1) {
                const int b = ssw_ctz(r);
                if ((p >> b) & 1u) depth++;
                else if (--depth == 0) return 32 * j + b - s.o;
            }
        }
    } else if ((unsigned)(v0 >> 32) & bit) {
        for (int j = j0; j >= A >> 5; j--) {
            unsigned p, q, m;
            ssw_load(s, j, A, X + 1, p, q, m);
            const int np = ssw_popc(p);
            if (depth - np > 0) { depth += ssw_popc(q) - np; continue; }
            for (unsigned r = p | q; r;) {
                const int b = ssw_top(r);
                r &= ~(1u << b);
                if ((q >> b) & 1u) depth++;
                else if (--depth == 0) return 32 * j + b - s.o;
            }
        }
    }
    return -1;
}

// does no ')' of s[0, len) close below depth 0 (the reference pops an empty stack there)
SSW_HD bool ssw_no_underflow(SSW s, int len) {
    if (len <= 0) return true;
    const int A = s.o, B = s.o + len;
    int depth = 0;
    for (int j = A >> 5; j <= (B - 1) >> 5; j++) {
        unsigned p, q, m;
        ssw_load(s, j, A, B, p, q, m);
        const int nq = ssw_popc(q);
        if (depth >= nq) { depth += ssw_popc(p) - nq; continue; }
        for (unsigned r = p | q; r; r &= r - 1) {
            if ((p >> ssw_ctz(r)) & 1u) depth++;
            else { if (depth == 0) return false; depth--; }
        }
    }
    return true;
}

SSW_HD bool ssw_is_stem_loop(SSW s, int len) {   // MP:1602-1608, minloop 3
    const int lo = ssw_rfind(s, '(', 0, len), fc = ssw_find(s, ')', 0, len);
    return fc - lo - 1 >= 3;
}

// MP:1611-1659.  The state machine runs over the brackets of each word in registers.
SSW_HD bool ssw_good_bifurcation(SSW s, int len) {
    int depth = 0, bif = 0, last_pop = 0, first_bi_last = 0, second_bi_first = 0, last_pos = 0;
    if (len > 0) {
        const int A = s.o, B = s.o + len;
        for (int j = A >> 5; j <= (B - 1) >> 5; j++) {
            unsigned p, q, m;
            ssw_load(s, j, A, B, p, q, m);
            for (unsigned r = p | q; r; r &= r - 1) {
                const int b = ssw_ctz(r), idx = 32 * j + b - s.o;
                if ((p >> b) & 1u) {
                    if (idx != 0) {
                        if (depth == 0) { if (last_pop) return false; }
                        else if (last_pop) {
                            if (bif >= 1) return false;
                            bif = 1; first_bi_last = last_pos; second_bi_first = idx;
                        }
                    }
                    depth++; last_pop = 0; last_pos = idx;
                } else {
                    last_pop = 1;
                    if (depth == 0) return false;
                    depth--; last_pos = idx;
                }
            }
        }
    }
    const int a = ssw_partner(s, len, second_bi_first), b = ssw_partner(s, len, first_bi_last);
    if (a < 0 || b < 0) return false;
    if ((double)(a - b) / len < 0.5)
        if ((double)b / len > 0.25)
            if ((double)a / len < 0.75) return true;
    return false;
}

// The duplex string of stat_duplex: s[m0, m0 + ml) followed by s[s0, s0 + L - ml), in chunks of 32 characters.
struct SSWCat {
    SSW s; int m0, ml, s0, L;
    SSW_HD_SMALL void chunk(int c, unsigned& op, unsigned& cl) const {          // characters [32 c, 32 c + 32) of the concatenation, masked to L
        const int i = 32 * c, n = L - i < 32 ? L - i : 32;
        if (i < ml) {
            const int n1 = ml - i < n ? ml - i : n;
            ssw_fetch(s, m0 + i, n1, op, cl);
            if (n1 < n) { unsigned a, b; ssw_fetch(s, s0, n - n1, a, b); op |= a << n1; cl |= b << n1; }
        } else ssw_fetch(s, s0 + i - ml, n, op, cl);
    }
};
// the same string held in registers: at most 64 characters
struct SSWCat64 {
    unsigned op0, cl0, op1, cl1;
    SSW_HD_SMALL void chunk(int c, unsigned& op, unsigned& cl) const { op = c ? op1 : op0; cl = c ? cl1 : cl0; }
};

// stat_duplex + pass_stat_duplex (MP:1815-1873) over a duplex string of L characters in nch chunks.  Returns the MS code.
template <class Src>
SSW_HD int ssw_duplex_stats(Src src, int L) {
    const int nch = (L + 31) >> 5;
    int openpos = -1, closepos = -1;
    for (int c = 0; c < nch && (openpos < 0 || closepos < 0); c++) {
        unsigned op, cl;
        src.chunk(c, op, cl);
        if (op && openpos < 0) openpos = 32 * c + ssw_ctz(op);
        if (cl && closepos < 0) closepos = 32 * c + ssw_ctz(cl);
    }
    const bool swap = openpos > closepos;          // the bracket that comes first opens
    // first make sure no close pops an empty stack (the reference would raise IndexError)
    {
        int depth = 0;
        for (int c = 0; c < nch; c++) {
            unsigned p, q;
            if (swap) src.chunk(c, q, p); else src.chunk(c, p, q);
            const int nq = ssw_popc(q);
            if (depth >= nq) { depth += ssw_popc(p) - nq; continue; }
            for (unsigned r = p | q; r; r &= r - 1) {
                if ((p >> ssw_ctz(r)) & 1u) depth++;
                else { if (depth == 0) return 12; depth--; }
            }
        }
    }
    // Pairs (open idx -> close idx), visited in increasing open idx.  Opens are matched LIFO: each open finds its close with a depth walk over the words.
    int nloops = 0, nbulges = 0, totalloop = 0, maxbulge = 0;
    int prev_o = -1, prev_c = -1;
    for (int ci = 0; ci < nch; ci++) {
        unsigned P, Q;
        if (swap) src.chunk(ci, Q, P); else src.chunk(ci, P, Q);
        for (unsigned opens = P; opens; opens &= opens - 1) {
            const int b0 = ssw_ctz(opens), i = 32 * ci + b0;
            int depth = 0, c = -1;
            for (int cj = ci; cj < nch && c < 0; cj++) {
                unsigned p, q;
                if (cj == ci) { const unsigned from = ~((1u << b0) - 1u); p = P & from; q = Q & from; }
                else if (swap) src.chunk(cj, q, p);
                else src.chunk(cj, p, q);
                const int nq = ssw_popc(q);
                if (depth - nq > 0) { depth += ssw_popc(p) - nq; continue; }
                for (unsigned r = p | q; r; r &= r - 1) {
                    const int b = ssw_ctz(r);
                    if ((p >> b) & 1u) depth++;
                    else if (--depth == 0) { c = 32 * cj + b; break; }
                }
            }
            if (c < 0) continue;   // never closed: not in dict_bp
            if (prev_o >= 0) {
                if (!((i - prev_o == 1) && (prev_c - c == 1))) {
                    const int mb = i - prev_o - 1, sb = prev_c - c - 1;
                    if (mb == sb) { nloops++; totalloop += mb; }
                    else { nbulges++; const int mx = mb > sb ? mb : sb; if (mx > maxbulge) maxbulge = mx; }
                }
            }
            prev_o = i; prev_c = c;
        }
    }
    if (nloops + nbulges > 5) return 8;
    if (maxbulge > 2) return 9;
    if (totalloop > 5) return 10;
    if (nbulges > 2) return 11;
    return 0;
}

// mature_duplex = s[m0, m1), star_duplex = s[s0, s1), m0 <= m1, s0 <= s1, inside the view.  A duplex of at most 64 characters (every miRNA-sized one) is read
// once into registers; a longer one (nothing bounds the star segment) is read through the words of the two segments.
SSW_HD int ssw_duplex_code(SSW s, int m0, int m1, int s0, int s1) {
    SSWCat cat; cat.s = s; cat.m0 = m0; cat.ml = m1 - m0; cat.s0 = s0; cat.L = cat.ml + (s1 - s0);
    if (cat.L <= 64) {
        SSW_PATH_HIT(0)
        SSWCat64 r; r.op0 = r.cl0 = r.op1 = r.cl1 = 0u;
        if (cat.L > 0) cat.chunk(0, r.op0, r.cl0);
        if (cat.L > 32) cat.chunk(1, r.op1, r.cl1);
        return ssw_duplex_stats(r, cat.L);
    }
    SSW_PATH_HIT(1)
    return ssw_duplex_stats(cat, cat.L);
}

struct MStar { int code, star_s, star_e, fold_s, fold_e; };

// get_maturestar_info (MP:1876-1999). strand 0 '+', 1 '-'.
SSW_HD void ssw_maturestar(SSW ss, int len, int m0, int m1, int foldstart, int rs, int re, int strand, MStar& o) {
    o.code = 0; o.star_s = o.star_e = 0;
    if (!ssw_no_underflow(ss, len)) { o.code = 1; return; }
    int l0, l1, fg0, fg1;
    if (strand == 0) { l0 = m0 - rs - foldstart + 1; l1 = m1 - rs - foldstart + 1; fg0 = rs + foldstart - 1; fg1 = fg0 + len; }
    else { l0 = re - m1 - foldstart + 1; l1 = re - m0 - foldstart + 1; fg0 = re - foldstart - len + 1; fg1 = re - foldstart + 1; }
    o.fold_s = fg0; o.fold_e = fg1;
    if (!(m0 >= fg0 && m1 <= fg1)) { o.code = 2; return; }
    int a = l0, b = l1; ssw_clip(len, a, b);
    int firstbp = ssw_find(ss, '(', a, b);
    const int firstcl = ssw_find(ss, ')', a, b);
    if (firstbp != -1 && firstcl != -1) { o.code = 3; return; }
    if ((b > a ? b - a : 0) - ssw_count(ss, '.', a, b) < 14) { o.code = 4; return; }
    char sym = '(';
    if (firstbp == -1) { firstbp = firstcl; sym = ')'; }
    if (firstbp == -1) { o.code = 4; return; }
    const int lastbp = ssw_rfind(ss, sym, a, b);
    const int p_last = ssw_partner(ss, len, lastbp), p_first = ssw_partner(ss, len, firstbp);
    if (p_last < 0 || p_first < 0) { o.code = 12; return; }
    const int star_start = p_last - (l1 - 1 - lastbp) + 2, star_end = p_first + (firstbp - l0) + 2 + 1;
    if (l0 <= star_start) {
        if (star_start - l1 < 3) { o.code = 5; return; }
        if (star_end > len) { o.code = 6; return; }
    }
    if (star_start <= l0) {
        if (l0 - star_end < 3) { o.code = 5; return; }
        if (star_start < 0) { o.code = 6; return; }
    }
    int ra = l0, rb = l1 - 2; ssw_clip(len, ra, rb);
    const int mend = ssw_rfind(ss, sym, ra, rb);
    const int p_mend = mend >= 0 ? ssw_partner(ss, len, mend) : -1;
    if (mend < 0 || p_mend < 0) { o.code = 12; return; }
    int md0 = l0, md1 = mend + 1, sd0 = p_mend, sd1 = p_first + 1;
    ssw_clip(len, md0, md1); ssw_clip(len, sd0, sd1);
    if (md1 < md0) md1 = md0;
    if (sd1 < sd0) sd1 = sd0;
    const int total_bps = (md1 - md0) - ssw_count(ss, '.', md0, md1);
    if (total_bps < 14) { o.code = 4; return; }
    int sa = star_start, sb = star_end; ssw_clip(len, sa, sb);
    if (ssw_find(ss, '(', sa, sb) != -1 && ssw_find(ss, ')', sa, sb) != -1) { o.code = 7; return; }
    const int dc = ssw_duplex_code(ss, md0, md1, sd0, sd1);
    if (dc) { o.code = dc; return; }
    if (strand == 0) { o.star_s = rs + foldstart - 1 + star_start; o.star_e = rs + foldstart - 1 + star_end; }
    else { o.star_s = re - foldstart - star_end + 1; o.star_e = re - foldstart - star_start + 1; }
}

// mature / star duplex figures of a passing structure (the values get_maturestar_info returns beside the star, MP:1876-1999): prime5 = the mature
// [l0, l1) of the view lies in the 5' arm, total_bps = the paired characters of the mature side of the duplex, total_dots = the unpaired ones of both
// sides.  Called on a structure that ssw_maturestar passed with the same interval, so the first bracket, mend and their partners exist.
SSW_HD void ssw_duplex_stats(SSW ss, int len, int l0, int l1, int* prime5, int* total_bps, int* total_dots) {
    int a = l0, b = l1; ssw_clip(len, a, b);
    char sym = '(';
    *prime5 = 1;
    int firstbp = ssw_find(ss, '(', a, b);
    if (firstbp == -1) { firstbp = ssw_find(ss, ')', a, b); sym = ')'; *prime5 = 0; }
    const int p_first = ssw_partner(ss, len, firstbp);
    int ra = l0, rb = l1 - 2; ssw_clip(len, ra, rb);
    const int mend = ssw_rfind(ss, sym, ra, rb);
    const int p_mend = ssw_partner(ss, len, mend);
    int md0 = l0, md1 = mend + 1, sd0 = p_mend, sd1 = p_first + 1;
    ssw_clip(len, md0, md1); ssw_clip(len, sd0, sd1);
    if (md1 < md0) md1 = md0;
    if (sd1 < sd0) sd1 = sd0;
    const int mdots = ssw_count(ss, '.', md0, md1);
    *total_dots = mdots + ssw_count(ss, '.', sd0, sd1);
    *total_bps = (md1 - md0) - mdots;
}

}  // namespace mirp
