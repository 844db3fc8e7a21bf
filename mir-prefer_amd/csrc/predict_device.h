// The structure rules of the predict stage as device code, shared by predict_kernel.hip and homolog_kernels.hip: the dot-bracket text staged at 2 bits
// per character, the structure list of a window (a8, MP:1541-1724) and get_maturestar_info with its duplex rules (a9, MP:1727-1999).
#pragma once
#include <hip/hip_runtime.h>

namespace mirp {

// One structure piece of a window: line index, offset and length inside the line, kind (0 stem-loop, 1 good bifurcation).
// start and normalised energy are recomputed from the line record.
struct PStruct { unsigned short line, off, len, type; };

// Dot-bracket text staged in LDS at 2 bits per character (16 characters per word): a window's lines then take <= 9 KB instead of
// 34 KB, which is what bounds the number of resident windows per CU.  0 '.', 1 '(', 2 ')'.
struct SS {
    const unsigned* w;
    int o;
    __device__ __forceinline__ char operator[](int i) const {
        const int k = o + i;
        const unsigned c = (w[k >> 4] >> ((k & 15) * 2)) & 3u;
        return c == 0 ? '.' : (c == 1 ? '(' : ')');
    }
    __device__ __forceinline__ SS operator+(int d) const { SS r; r.w = w; r.o = o + d; return r; }
};

__device__ __forceinline__ int d_find(SS s, char c, int a, int b) { for (int i = a; i < b; i++) if (s[i] == c) return i; return -1; }
__device__ __forceinline__ int d_rfind(SS s, char c, int a, int b) { for (int i = b - 1; i >= a; i--) if (s[i] == c) return i; return -1; }
__device__ __forceinline__ int d_count(SS s, char c, int a, int b) { int n = 0; for (int i = a; i < b; i++) n += (s[i] == c); return n; }
__device__ __forceinline__ void d_clip(int len, int& a, int& b) {   // Python slice bounds
    if (a < 0) { a += len; if (a < 0) a = 0; }
    if (b < 0) { b += len; if (b < 0) b = 0; }
    if (a > len) a = len;
    if (b > len) b = len;
}

// partner of bracket at x inside s[0,len); -1 if unmatched
__device__ int d_partner(SS s, int len, int x) {
    int depth = 0;
    if (s[x] == '(') {
        for (int i = x; i < len; i++) { if (s[i] == '(') depth++; else if (s[i] == ')') { if (--depth == 0) return i; } }
    } else if (s[x] == ')') {
        for (int i = x; i >= 0; i--) { if (s[i] == ')') depth++; else if (s[i] == '(') { if (--depth == 0) return i; } }
    }
    return -1;
}

__device__ bool d_is_stem_loop(SS s, int len) {   // MP:1602-1608, minloop 3
    int lo = d_rfind(s, '(', 0, len), fc = d_find(s, ')', 0, len);
    return fc - lo - 1 >= 3;
}

// MP:1611-1659
__device__ bool d_good_bifurcation(SS s, int len) {
    int depth = 0, bif = 0, last_pop = 0, first_bi_last = 0, second_bi_first = 0, last_pos = 0;
    for (int idx = 0; idx < len; idx++) {
        char ch = s[idx];
        if (ch == '(') {
            if (idx != 0) {
                if (depth == 0) { if (last_pop) return false; }
                else if (last_pop) {
                    if (bif >= 1) return false;
                    bif = 1; first_bi_last = last_pos; second_bi_first = idx;
                }
            }
            depth++; last_pop = 0; last_pos = idx;
        } else if (ch == ')') {
            last_pop = 1;
            if (depth == 0) return false;
            depth--; last_pos = idx;
        }
    }
    int a = d_partner(s, len, second_bi_first), b = d_partner(s, len, first_bi_last);
    if (a < 0 || b < 0) return false;
    if ((double)(a - b) / len < 0.5)
        if ((double)b / len > 0.25)
            if ((double)a / len < 0.75) return true;
    return false;
}

// stat_duplex + pass_stat_duplex (MP:1815-1873) on mature_duplex = s[m0,m1), star_duplex = s[s0,s1). Returns MS code.
__device__ int d_duplex_code(SS s, int m0, int m1, int s0, int s1) {
    const int ml = m1 - m0, L = ml + (s1 - s0);
#define DCH(i) ((i) < ml ? s[m0 + (i)] : s[s0 + (i) - ml])
    int openpos = -1, closepos = -1;
    for (int i = 0; i < L && (openpos < 0 || closepos < 0); i++) {
        char ch = DCH(i);
        if (ch == '(' && openpos < 0) openpos = i;
        if (ch == ')' && closepos < 0) closepos = i;
    }
    char oc = '(', cc = ')';
    if (openpos > closepos) { oc = ')'; cc = '('; }
    // Pairs (open idx -> close idx), visited in increasing open idx.  Opens are matched LIFO.
    // Walk the opens in order and find each one's close with a depth counter (no arrays needed).
    int nloops = 0, nbulges = 0, totalloop = 0, maxbulge = 0;
    int prev_o = -1, prev_c = -1;
    // first make sure no close pops an empty stack (the reference would raise IndexError)
    {
        int depth = 0;
        for (int i = 0; i < L; i++) { char ch = DCH(i); if (ch == oc) depth++; else if (ch == cc) { if (depth == 0) return 12; depth--; } }
    }
    for (int i = 0; i < L; i++) {
        if (DCH(i) != oc) continue;
        int depth = 0, c = -1;
        for (int j = i; j < L; j++) { char ch = DCH(j); if (ch == oc) depth++; else if (ch == cc) { if (--depth == 0) { c = j; break; } } }
        if (c < 0) continue;   // never closed: not in dict_bp
        if (prev_o >= 0) {
            if (!((i - prev_o == 1) && (prev_c - c == 1))) {
                int mb = i - prev_o - 1, sb = prev_c - c - 1;
                if (mb == sb) { nloops++; totalloop += mb; }
                else { nbulges++; maxbulge = max(maxbulge, max(mb, sb)); }
            }
        }
        prev_o = i; prev_c = c;
    }
#undef DCH
    if (nloops + nbulges > 5) return 8;
    if (maxbulge > 2) return 9;
    if (totalloop > 5) return 10;
    if (nbulges > 2) return 11;
    return 0;
}

struct MStar { int code, star_s, star_e, fold_s, fold_e; };

// get_maturestar_info (MP:1876-1999). strand 0 '+', 1 '-'.
__device__ void d_maturestar(SS ss, int len, int m0, int m1, int foldstart, int rs, int re, int strand, MStar& o) {
    o.code = 0; o.star_s = o.star_e = 0;
    { int depth = 0; for (int i = 0; i < len; i++) { if (ss[i] == '(') depth++; else if (ss[i] == ')') { if (depth == 0) { o.code = 1; return; } depth--; } } }
    int l0, l1, fg0, fg1;
    if (strand == 0) { l0 = m0 - rs - foldstart + 1; l1 = m1 - rs - foldstart + 1; fg0 = rs + foldstart - 1; fg1 = fg0 + len; }
    else { l0 = re - m1 - foldstart + 1; l1 = re - m0 - foldstart + 1; fg0 = re - foldstart - len + 1; fg1 = re - foldstart + 1; }
    o.fold_s = fg0; o.fold_e = fg1;
    if (!(m0 >= fg0 && m1 <= fg1)) { o.code = 2; return; }
    int a = l0, b = l1; d_clip(len, a, b);
    bool has_o = d_find(ss, '(', a, b) != -1, has_c = d_find(ss, ')', a, b) != -1;
    if (has_o && has_c) { o.code = 3; return; }
    if ((b > a ? b - a : 0) - d_count(ss, '.', a, b) < 14) { o.code = 4; return; }
    char sym = '(';
    int firstbp = d_find(ss, '(', a, b), lastbp = d_rfind(ss, '(', a, b);
    if (firstbp == -1) { firstbp = d_find(ss, ')', a, b); lastbp = d_rfind(ss, ')', a, b); sym = ')'; }
    if (firstbp == -1) { o.code = 4; return; }
    int p_last = d_partner(ss, len, lastbp), p_first = d_partner(ss, len, firstbp);
    if (p_last < 0 || p_first < 0) { o.code = 12; return; }
    int star_start = p_last - (l1 - 1 - lastbp) + 2, star_end = p_first + (firstbp - l0) + 2 + 1;
    if (l0 <= star_start) {
        if (star_start - l1 < 3) { o.code = 5; return; }
        if (star_end > len) { o.code = 6; return; }
    }
    if (star_start <= l0) {
        if (l0 - star_end < 3) { o.code = 5; return; }
        if (star_start < 0) { o.code = 6; return; }
    }
    int ra = l0, rb = l1 - 2; d_clip(len, ra, rb);
    int mend = d_rfind(ss, sym, ra, rb);
    int p_mend = mend >= 0 ? d_partner(ss, len, mend) : -1;
    if (mend < 0 || p_mend < 0) { o.code = 12; return; }
    int md0 = l0, md1 = mend + 1, sd0 = p_mend, sd1 = p_first + 1;
    d_clip(len, md0, md1); d_clip(len, sd0, sd1);
    if (md1 < md0) md1 = md0;
    if (sd1 < sd0) sd1 = sd0;
    int total_bps = (md1 - md0) - d_count(ss, '.', md0, md1);
    if (total_bps < 14) { o.code = 4; return; }
    int sa = star_start, sb = star_end; d_clip(len, sa, sb);
    if (d_find(ss, '(', sa, sb) != -1 && d_find(ss, ')', sa, sb) != -1) { o.code = 7; return; }
    int dc = d_duplex_code(ss, md0, md1, sd0, sd1);
    if (dc) { o.code = dc; return; }
    if (strand == 0) { o.star_s = rs + foldstart - 1 + star_start; o.star_e = rs + foldstart - 1 + star_end; }
    else { o.star_s = re - foldstart - star_end + 1; o.star_e = re - foldstart - star_start + 1; }
}

}  // namespace mirp
