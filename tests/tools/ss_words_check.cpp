// Check program of mir-prefer_amd/csrc/ss_words.h (tests/test_ss_words_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it):
// every structure rule on words against its character-by-character restatement, result by result.  The restatement is the rule set the filter kernel ran
// and the homolog evaluation ran before the word rules, moved here unchanged (the two attribute macros below make it host code).  Every packed row is a heap block of exactly the words its
// line needs, so a rule that reads a word beyond its view's line is a sanitizer error.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

static thread_local long long g_path_hit[2] = {0, 0};
#define SSW_PATH_HIT(k) g_path_hit[k]++;
#include "../../mir-prefer_amd/csrc/ss_words.h"

// ------------------------------------------------------------------------------------------------ the restatement (character by character)
namespace ref {
using std::max;
#define __device__
#define __forceinline__ inline

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

// mature / star duplex figures of a passing structure (the values get_maturestar_info returns beside the star, MP:1876-1999)
__device__ void hm_duplex_stats(SS ss, int len, int l0, int l1, int* prime5, int* total_bps, int* total_dots) {
    int a = l0, b = l1; d_clip(len, a, b);
    char sym = '(';
    *prime5 = 1;
    int firstbp = d_find(ss, '(', a, b);
    if (firstbp == -1) { firstbp = d_find(ss, ')', a, b); sym = ')'; *prime5 = 0; }
    const int p_first = d_partner(ss, len, firstbp);
    int ra = l0, rb = l1 - 2; d_clip(len, ra, rb);
    const int mend = d_rfind(ss, sym, ra, rb);
    const int p_mend = d_partner(ss, len, mend);
    int md0 = l0, md1 = mend + 1, sd0 = p_mend, sd1 = p_first + 1;
    d_clip(len, md0, md1); d_clip(len, sd0, sd1);
    if (md1 < md0) md1 = md0;
    if (sd1 < sd0) sd1 = sd0;
    const int mdots = d_count(ss, '.', md0, md1);
    *total_dots = mdots + d_count(ss, '.', sd0, sd1);
    *total_bps = (md1 - md0) - mdots;
}
#undef __device__
#undef __forceinline__
}  // namespace ref

// ------------------------------------------------------------------------------------------------ harness
using mirp::SSW;

static thread_local long long g_checks = 0, g_code_hist[16] = {0}, g_dstats = 0, g_dstats_3p = 0;
static thread_local std::mt19937 g_rng(20240611u);
static int rnd(int lo, int hi) { return lo + (int)(g_rng() % (unsigned)(hi - lo + 1)); }          // inclusive

[[noreturn]] static void fail(const char* what, const std::string& host, int off, int len, long long a, long long b, long long got, long long want) {
    std::fprintf(stderr, "MISMATCH %s: view offset %d length %d args (%lld, %lld): words %lld, characters %lld\nline: %s\n", what, off, len, a, b, got, want,
                 host.size() <= 400 ? host.c_str() : "(long)");
    std::exit(1);
}
#define CHECK(what, a, b, got, want) do { g_checks++; const long long g_ = (got), w_ = (want); if (g_ != w_) fail(what, L.host, off, len, (a), (b), g_, w_); } while (0)

// a line in both stagings, each in a heap block of exactly its size
struct Line {
    std::string host;
    unsigned* w2;                  // 2 bits per character
    unsigned long long* w1;        // bit planes
    explicit Line(const std::string& h) : host(h) {
        const int n = (int)h.size(), n2 = (n + 15) >> 4, n1 = mirp::ssw_words(n);
        w2 = (unsigned*)std::malloc(sizeof(unsigned) * (size_t)(n2 ? n2 : 1));
        w1 = (unsigned long long*)std::malloc(sizeof(unsigned long long) * (size_t)(n1 ? n1 : 1));
        for (int k = 0; k < n2; k++) w2[k] = 0;
        for (int i = 0; i < n; i++) w2[i >> 4] |= (h[i] == '(' ? 1u : (h[i] == ')' ? 2u : 0u)) << ((i & 15) * 2);
        for (int k = 0; k < n1; k++) {          // as the kernels' stager does: four characters per read, eight reads per word
            unsigned op = 0, cl = 0;
            for (int q = 0; q < 8; q++) {
                unsigned four = 0;
                for (int b = 0; b < 4; b++) { const int i = 32 * k + 4 * q + b; if (i < n) four |= (unsigned)(unsigned char)h[i] << (8 * b); }
                mirp::ssw_pack4(four, 4 * q, op, cl);
            }
            w1[k] = mirp::ssw_word(op, cl);
        }
    }
    ~Line() { std::free(w2); std::free(w1); }
    Line(const Line&) = delete;
    ref::SS r(int off) const { ref::SS s; s.w = w2; s.o = off; return s; }
    SSW v(int off) const { SSW s; s.w = w1; s.o = off; return s; }
};

static void check_range(const Line& L, int off, int len, int a, int b) {
    const ref::SS R = L.r(off); const SSW V = L.v(off);
    for (const char c : {'(', ')', '.'}) {
        CHECK("find", a, b, mirp::ssw_find(V, c, a, b), ref::d_find(R, c, a, b));
        CHECK("rfind", a, b, mirp::ssw_rfind(V, c, a, b), ref::d_rfind(R, c, a, b));
        CHECK("count", a, b, mirp::ssw_count(V, c, a, b), ref::d_count(R, c, a, b));
    }
}
static void check_slice(const Line& L, int off, int len, int a0, int b0) {          // Python slice bounds, then the scans over the clipped range
    int a = a0, b = b0, ra = a0, rb = b0;
    mirp::ssw_clip(len, a, b); ref::d_clip(len, ra, rb);
    CHECK("clip a", a0, b0, a, ra);
    CHECK("clip b", a0, b0, b, rb);
    check_range(L, off, len, a, b);
}
static void check_duplex(const Line& L, int off, int len, int m0, int m1, int s0, int s1) {
    CHECK("duplex_code", (long long)m0 * 100000 + m1, (long long)s0 * 100000 + s1, mirp::ssw_duplex_code(L.v(off), m0, m1, s0, s1), ref::d_duplex_code(L.r(off), m0, m1, s0, s1));
}
static void check_maturestar(const Line& L, int off, int len, int m0, int m1, int foldstart, int rs, int re, int strand) {
    mirp::MStar g; ref::MStar w;
    g.fold_s = g.fold_e = w.fold_s = w.fold_e = -12345;          // code 1 leaves them unset in both
    mirp::ssw_maturestar(L.v(off), len, m0, m1, foldstart, rs, re, strand, g);
    ref::d_maturestar(L.r(off), len, m0, m1, foldstart, rs, re, strand, w);
    CHECK("maturestar code", m0, m1, g.code, w.code);
    CHECK("maturestar star_s", m0, m1, g.star_s, w.star_s);
    CHECK("maturestar star_e", m0, m1, g.star_e, w.star_e);
    CHECK("maturestar fold_s", m0, m1, g.fold_s, w.fold_s);
    CHECK("maturestar fold_e", m0, m1, g.fold_e, w.fold_e);
    g_code_hist[w.code & 15]++;
}
// The five positions the duplex figures are made of, as the restatement finds them; false where one of them does not exist.  The kernel asks for the
// figures only of a structure that get_maturestar_info passed, where all five exist; the restatement reads character firstbp, mend or a partner without
// looking at its sign, so both functions are called only where these are >= 0 and the restatement's reads stay inside the line.
struct DuplexPos { int l0, l1m2, mend, p_mend, p_first; };
static bool duplex_positions(ref::SS R, int len, int l0, int l1, DuplexPos* out) {
    int a = l0, b = l1; ref::d_clip(len, a, b);
    char sym = '(';
    int firstbp = ref::d_find(R, '(', a, b);
    if (firstbp == -1) { firstbp = ref::d_find(R, ')', a, b); sym = ')'; }
    if (firstbp < 0) return false;
    const int p_first = ref::d_partner(R, len, firstbp);
    int ra = l0, rb = l1 - 2; ref::d_clip(len, ra, rb);
    const int mend = ref::d_rfind(R, sym, ra, rb);
    if (mend < 0 || p_first < 0) return false;
    const int p_mend = ref::d_partner(R, len, mend);
    if (p_mend < 0) return false;
    if (out) { out->l0 = l0; out->l1m2 = l1 - 2; out->mend = mend; out->p_mend = p_mend; out->p_first = p_first; }
    return true;
}
static bool check_duplex_stats(const Line& L, int off, int len, int l0, int l1) {
    if (!duplex_positions(L.r(off), len, l0, l1, nullptr)) return false;
    int g[3] = {-7, -7, -7}, w[3] = {-7, -7, -7};
    mirp::ssw_duplex_stats(L.v(off), len, l0, l1, &g[0], &g[1], &g[2]);
    ref::hm_duplex_stats(L.r(off), len, l0, l1, &w[0], &w[1], &w[2]);
    CHECK("duplex_stats prime5", l0, l1, g[0], w[0]);
    CHECK("duplex_stats total_bps", l0, l1, g[1], w[1]);
    CHECK("duplex_stats total_dots", l0, l1, g[2], w[2]);
    g_dstats++;
    g_dstats_3p += w[0] == 0;
    return true;
}
// a mature of 18 .. 24 characters anywhere in the view, both strands; window coordinates chosen so that the local coordinates fall where wanted
static void check_maturestar_at(const Line& L, int off, int len, int l0, int ml, int strand) {
    const int foldstart = rnd(1, 40), rs = rnd(100, 5000), re = rs + foldstart + len + rnd(0, 60);
    int m0, m1;
    if (strand == 0) { m0 = l0 + rs + foldstart - 1; m1 = m0 + ml; }
    else { m1 = re - foldstart + 1 - l0; m0 = m1 - ml; }
    check_maturestar(L, off, len, m0, m1, foldstart, rs, re, strand);
}
static void check_view_basic(const Line& L, int off, int len) {
    const ref::SS R = L.r(off); const SSW V = L.v(off);
    check_range(L, off, len, 0, len);
    for (int x = 0; x < len; x++) CHECK("partner", x, 0, mirp::ssw_partner(V, len, x), ref::d_partner(R, len, x));
    CHECK("is_stem_loop", 0, 0, mirp::ssw_is_stem_loop(V, len), ref::d_is_stem_loop(R, len));
    if (len > 0) CHECK("good_bifurcation", 0, 0, mirp::ssw_good_bifurcation(V, len), ref::d_good_bifurcation(R, len));
}
// everything on one view; n_extra random ranges, slices, duplexes and matures beside the fixed ones
static void check_view(const Line& L, int off, int len, int n_extra) {
    check_view_basic(L, off, len);
    check_range(L, off, len, len, len);
    check_range(L, off, len, 0, 0);
    check_slice(L, off, len, -3, len + 5);
    check_slice(L, off, len, -len - 4, -1);
    check_slice(L, off, len, len + 2, len + 9);
    check_slice(L, off, len, 2, 1);
    for (int k = 0; k < n_extra; k++) {
        const int a = rnd(0, len), b = rnd(0, len);
        check_range(L, off, len, a < b ? a : b, a < b ? b : a);
        check_slice(L, off, len, rnd(-len - 3, len + 3), rnd(-len - 3, len + 3));
        if (len >= 2) {
            const int c1 = rnd(0, len), c2 = rnd(0, len), c3 = rnd(0, len), c4 = rnd(0, len);
            check_duplex(L, off, len, std::min(c1, c2), std::max(c1, c2), std::min(c3, c4), std::max(c3, c4));
        }
        check_maturestar_at(L, off, len, rnd(-3, len), rnd(18, 24), k & 1);
    }
}

static const int kOffsets[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65};
static std::string random_text(int n) { std::string s((size_t)n, '.'); for (char& c : s) c = ".()"[g_rng() % 3]; return s; }
static std::string embed(const std::string& s, int off, int tail) { return random_text(off) + s + random_text(tail); }

static std::string balanced(int n, int p_dot) {          // a balanced dot-bracket string of n characters
    std::string s((size_t)n, '.');
    int depth = 0;
    for (int i = 0; i < n; i++) {
        const int left = n - i;
        if (depth >= left) { s[(size_t)i] = ')'; depth--; continue; }
        const int r = rnd(0, 99);
        if (r < p_dot) continue;
        if (depth > 0 && (r & 1)) { s[(size_t)i] = ')'; depth--; }
        else if (depth + 1 <= left - 1) { s[(size_t)i] = '('; depth++; }
    }
    return s;
}
// a hairpin: 5' tail, an arm of n_pairs '(' with bulges, a loop, the mirrored arm with its own bulges, 3' tail
static std::string hairpin(int n_pairs, int loop, int p_bulge, int t5, int t3, std::vector<int>* opens = nullptr) {
    std::string s((size_t)t5, '.');
    for (int k = 0; k < n_pairs; k++) { if (opens) opens->push_back((int)s.size()); s += '('; if (rnd(0, 99) < p_bulge) s += std::string((size_t)rnd(1, 3), '.'); }
    s += std::string((size_t)loop, '.');
    for (int k = 0; k < n_pairs; k++) { s += ')'; if (rnd(0, 99) < p_bulge) s += std::string((size_t)rnd(1, 3), '.'); }
    s += std::string((size_t)t3, '.');
    return s;
}

struct Tally { long long views = 0, checks = 0, codes[16] = {0}, dstats = 0, dstats_3p = 0; };
static void exhaustive_at(int off, Tally* out) {
    g_rng.seed(977u + (unsigned)off);
    long long n = 0;
    for (int len = 0; len <= 11; len++) {
        long long total = 1;
        for (int k = 0; k < len; k++) total *= 3;
        std::string s((size_t)len, '.');
        const std::string head = random_text(off), tails[3] = {"", random_text(rnd(1, 40)), random_text(rnd(1, 40))};
        for (long long code = 0; code < total; code++) {
            long long c = code;
            for (int k = 0; k < len; k++) { s[(size_t)k] = ".()"[c % 3]; c /= 3; }
            const Line L(head + s + tails[code % 3]);
            n++;
            if (s.find_first_of("()") != std::string::npos)          // the duplex figures over every interval that holds a bracket
                for (int l0 = -2; l0 <= len + 2; l0++) for (int l1 = l0; l1 <= len + 2; l1++) check_duplex_stats(L, off, len, l0, l1);
            if (len <= 7) {
                check_view(L, off, len, 1);
                for (int a = 0; a <= len; a++) for (int b = a; b <= len; b++) check_range(L, off, len, a, b);
                for (int a = -len - 2; a <= len + 2; a++) check_slice(L, off, len, a, (int)((code + a + 64) % (2 * len + 5)) - len - 2);
            } else {
                check_view_basic(L, off, len);
                const int a = rnd(0, len), b = rnd(0, len);
                check_range(L, off, len, std::min(a, b), std::max(a, b));
                check_duplex(L, off, len, 0, a, b, len);
                check_maturestar_at(L, off, len, rnd(-2, 3), rnd(4, 11), (int)(code & 1));
            }
        }
    }
    out->views = n; out->checks = g_checks; out->dstats = g_dstats; out->dstats_3p = g_dstats_3p;
    for (int c = 0; c < 16; c++) out->codes[c] = g_code_hist[c];
}

int main() {
    // 1. every string over . ( ) up to length 11, at every view offset, inside a longer random line (every third one ends with the view): a thread per offset
    std::vector<std::thread> workers;
    Tally tallies[sizeof(kOffsets) / sizeof(kOffsets[0])];
    for (size_t k = 0; k < sizeof(kOffsets) / sizeof(kOffsets[0]); k++) workers.emplace_back(exhaustive_at, kOffsets[k], &tallies[k]);
    // 2. seeded random balanced and unbalanced strings at the word-boundary lengths and at line lengths of the filter
    {
        const int lens[] = {15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 325, 350, 3000};
        for (const int n : lens) {
            const int reps = n >= 3000 ? 2 : n >= 300 ? 6 : 12;
            for (int rep = 0; rep < reps; rep++) {
                for (int kind = 0; kind < 2; kind++) {
                    const std::string s = kind ? random_text(n) : balanced(n, rep % 3 == 0 ? 20 : 60);
                    for (const int off : kOffsets) {
                        if (n >= 3000 && off != 0 && off != 17 && off != 33) continue;
                        const Line L(embed(s, off, rep & 1 ? 0 : rnd(1, 70)));
                        check_view(L, off, n, n >= 300 ? 60 : 25);
                    }
                    // views into the line itself: pieces at odd offsets, as filter_ss cuts them
                    const Line L(s);
                    for (int k = 0; k < 8; k++) { const int off = rnd(0, n - 1), len = rnd(1, n - off); check_view(L, off, len, 6); }
                }
            }
        }
    }
    // 3. hairpin loops and partner pairs across one and across two word boundaries
    {
        for (int start = 20; start <= 70; start++) {
            for (const int span : {3, 4, 5, 8, 30, 31, 32, 33, 34, 40, 62, 63, 64, 65, 66, 70, 100}) {          // span: dots between the innermost pair
                for (const int pairs : {1, 2, 5}) {
                    const std::string s = std::string((size_t)start, '.') + std::string((size_t)pairs, '(') + std::string((size_t)span, '.') + std::string((size_t)pairs, ')') + "..";
                    const Line L(s);
                    check_view(L, 0, (int)s.size(), 4);
                    check_view(L, start > 3 ? start - 3 : 0, (int)s.size() - (start > 3 ? start - 3 : 0), 2);
                    for (int l0 = start - 26; l0 <= (int)s.size(); l0++)          // the duplex figures with the interval over either arm
                        for (const int w : {18, 21, 26}) { if (l0 >= 0) check_duplex_stats(L, 0, (int)s.size(), l0, l0 + w); }
                    // two hairpins side by side: a bifurcation whose branch point pairs straddle the boundaries
                    const std::string t = "((" + s + s.substr((size_t)start) + "))";
                    const Line T(t);
                    check_view(T, 0, (int)t.size(), 2);
                    for (int l0 = 0; l0 <= (int)t.size(); l0 += 3) check_duplex_stats(T, 0, (int)t.size(), l0, l0 + 21);
                }
            }
        }
    }
    // 4. duplexes of 20 .. 200 characters: matures on hairpins with long and short arms, both sides of the 64-character register path
    {
        const long long h0 = g_path_hit[0], h1 = g_path_hit[1];
        long long by_len[2] = {0, 0};
        for (int rep = 0; rep < 1500; rep++) {
            std::vector<int> opens;
            const int pairs = rnd(16, 90), t5 = rnd(0, 40);
            const std::string s = hairpin(pairs, rnd(3, 12), rep % 4 == 0 ? 0 : rnd(2, 25), t5, rnd(0, 40), &opens);
            const int off = kOffsets[rep % 11];
            const Line L(embed(s, off, rep % 3 ? rnd(1, 30) : 0));
            const int len = (int)s.size();
            // direct: mature segment on the 5' arm, star segment its partner range; total 20 .. 200 characters
            const int k0 = rnd(0, pairs - 10), k1 = rnd(k0 + 9, std::min(pairs - 1, k0 + 95));
            const int m0 = opens[(size_t)k0], m1 = opens[(size_t)k1] + 1;
            const int s0 = ref::d_partner(L.r(off), len, opens[(size_t)k1]), s1 = ref::d_partner(L.r(off), len, opens[(size_t)k0]) + 1;
            const int total = (m1 - m0) + (s1 - s0);
            if (total >= 20 && total <= 200) {
                by_len[total > 64]++;
                check_duplex(L, off, len, m0, m1, s0, s1);
                check_duplex(L, off, len, s0, s1, m0, m1);          // the close bracket comes first: roles swap
                check_duplex(L, off, len, m0, m1, s0 + 1, s1);      // an unclosed open
                check_duplex(L, off, len, m0 + 1, m1, s0, s1);      // a close that pops the empty stack
            }
            // through get_maturestar_info: matures of 18 .. 24 on either arm and either strand, and long "matures" whose duplex passes 64 characters
            for (int q = 0; q < 6; q++) check_maturestar_at(L, off, len, rnd(t5 > 2 ? t5 - 2 : 0, len - 18), rnd(18, 24), q & 1);
            for (int q = 0; q < 2; q++) check_maturestar_at(L, off, len, opens[(size_t)k0], rnd(34, 80), q & 1);
        }
        std::printf("duplex inputs of 20 .. 200 characters: %lld of at most 64, %lld longer; register path taken %lld times, word path %lld times\n", by_len[0], by_len[1],
                    g_path_hit[0] - h0, g_path_hit[1] - h1);
        if (by_len[0] == 0 || by_len[1] == 0 || g_path_hit[0] == h0 || g_path_hit[1] == h1) { std::fprintf(stderr, "a side of the 64-character path was not hit\n"); return 1; }
    }
    // 5. the duplex figures (ssw_duplex_stats) on hairpins in lines of 60 .. 3,000 characters: an interval of 18 .. 26 characters on either arm, the line
    // shifted so that l0, l1 - 2, mend, p_mend and p_first in turn land on character 31, 32, 33, 63, 64, 65 and in the last word of the line
    {
        static const int kTargets[6] = {31, 32, 33, 63, 64, 65};
        long long hit[2][5][7] = {};
        for (int rep = 0; rep < 700; rep++) {
            const int pairs = rep % 2 ? rnd(3, 14) : rep % 8 ? rnd(15, 120) : rnd(121, 1400);
            const std::string core = hairpin(pairs, rnd(3, 12), rep % 3 == 0 ? 0 : rnd(2, 20), 0, rnd(0, 30));
            const int C = (int)core.size();
            if (C > 3000) continue;
            const Line K(core);
            for (int arm = 0; arm < 2; arm++) {
                std::vector<int> br;
                for (int i = 0; i < C; i++) if (core[(size_t)i] == (arm ? ')' : '(')) br.push_back(i);
                for (int tries = 0; tries < 3; tries++) {
                    const int w = rnd(18, 26), b0 = br[(size_t)rnd(0, (int)br.size() - 1)];
                    const int l0 = std::max(0, tries == 0 ? b0 - rnd(0, 3) : tries == 1 ? br.front() - rnd(0, w - 3) : br.back() - rnd(2, w - 3)), l1 = l0 + w;
                    DuplexPos P;
                    if (!duplex_positions(K.r(0), C, l0, l1, &P)) continue;
                    const int X[5] = {P.l0, P.l1m2, P.mend, P.p_mend, P.p_first};
                    for (int q = 0; q < 5; q++) {
                        for (int t = 0; t < 7; t++) {
                            int shift = -1;
                            if (t < 6) {
                                if (X[q] <= kTargets[t] && kTargets[t] - X[q] + C <= 3000) shift = kTargets[t] - X[q];
                                if (shift >= 0 && shift + C < 60) shift = -1;          // the line is shorter than 60 characters
                            } else {
                                for (int k = 0; k < 40 && shift < 0; k++) {
                                    const int sft = rnd(std::max(0, 60 - C), 3000 - C), N = sft + C;
                                    if (sft + X[q] >= 32 * ((N - 1) >> 5)) shift = sft;
                                }
                            }
                            if (shift < 0) continue;
                            const Line L(std::string((size_t)shift, '.') + core);
                            const int len = shift + C, off = 0;
                            DuplexPos Q;
                            const bool same = duplex_positions(L.r(0), len, l0 + shift, l1 + shift, &Q);
                            CHECK("duplex positions after the shift", l0, l1, same && Q.mend == P.mend + shift && Q.p_mend == P.p_mend + shift && Q.p_first == P.p_first + shift, 1);
                            if (check_duplex_stats(L, 0, len, l0 + shift, l1 + shift)) hit[ref::d_find(K.r(0), '(', l0, std::min(l1, C)) < 0][q][t]++;
                            check_duplex_stats(L, 0, len, l0 + shift - 1, l1 + shift);
                            check_duplex_stats(L, 0, len, l0 + shift + 1, l1 + shift + 1);
                        }
                    }
                }
            }
        }
        for (int a = 0; a < 2; a++) for (int q = 0; q < 5; q++) for (int t = 0; t < 7; t++)
            if (hit[a][q][t] == 0) {
                std::fprintf(stderr, "duplex figures: arm %d, position %d (l0, l1 - 2, mend, p_mend, p_first) never landed on target %d (31 32 33 63 64 65 last word)\n", a, q, t);
                return 1;
            }
    }
    {
        long long views = 0;
        for (size_t k = 0; k < workers.size(); k++) {
            workers[k].join();
            views += tallies[k].views; g_checks += tallies[k].checks; g_dstats += tallies[k].dstats; g_dstats_3p += tallies[k].dstats_3p;
            for (int c = 0; c < 16; c++) g_code_hist[c] += tallies[k].codes[c];
        }
        std::printf("exhaustive: %lld views\n", views);
    }
    std::printf("get_maturestar_info codes seen:");
    for (int c = 0; c < 13; c++) std::printf(" %d:%lld", c, g_code_hist[c]);
    std::printf("\nduplex figures: %lld comparisons, %lld with prime5 == 0\n", g_dstats, g_dstats_3p);
    std::printf("OK %lld comparisons\n", g_checks);
    return 0;
}
