// C-ABI of the homolog search (mirp_homolog_scan): the known sequences are checked and coded here, homolog_kernels.hip places them
// in the resident alignment index, cuts the windows, and evaluates what the fold leaves on the device; the placements come back chunk by chunk and
// are merged into loci and ordered here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>
#include "mirp_ctx.h"

namespace {

template <class T>
T* hm_copy_out(const T* src, size_t n) {
    T* p = (T*)std::malloc(sizeof(T) * std::max<size_t>(n, 1));
    if (p && n) std::memcpy(p, src, sizeof(T) * n);
    return p;
}

}  // namespace

extern "C" int mirp_set_homolog_capacity(mirp_ctx* c, int64_t keys, int64_t chunk, int32_t fold_lines, int32_t pieces, int32_t structures, int32_t staged_lines) {
    if (!c) return -1;
    const int set = (pieces > 0) + (structures > 0) + (staged_lines > 0);
    if (keys < 0 || chunk < 0 || chunk > 0x7fffffffll || fold_lines < 0 || pieces < 0 || structures < 0 || staged_lines < 0 || (set != 0 && set != 3))
        return fail(c, -1, "mirp_set_homolog_capacity: bad argument");
    c->hm_cap = keys;
    c->hm_chunk = chunk;
    c->hm_lines = fold_lines;
    c->hm_eval_caps[0] = pieces; c->hm_eval_caps[1] = structures; c->hm_eval_caps[2] = staged_lines;
    return 0;
}

extern "C" int mirp_homolog_last_stats(mirp_ctx* c, int64_t stats[24], double seconds[5]) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_homolog_last_stats: bad argument");
    for (int i = 0; i < 24; i++) stats[i] = c->hm_stats[i];
    if (seconds)
        for (int i = 0; i < 5; i++) seconds[i] = c->hm_sec[i];
    return 0;
}

extern "C" int mirp_homolog_contigs(mirp_ctx* c, char** names, int64_t* names_bytes, int64_t** lens, int32_t* n_contigs) {
    if (!c) return -1;
    if (!names || !names_bytes || !lens || !n_contigs) return fail(c, -1, "mirp_homolog_contigs: bad argument");
    *names = nullptr; *names_bytes = 0; *lens = nullptr; *n_contigs = 0;
    if (!c->a_ready) return fail(c, -1, "mirp_homolog_contigs: no index (mirp_align_index first)");
    std::string blob;
    for (const std::string& s : c->a_contig_names) { blob += s; blob += '\0'; }
    static_assert(sizeof(long long) == sizeof(int64_t), "the lengths are handed over as they are");
    char* o_n = hm_copy_out(blob.data(), blob.size());
    int64_t* o_l = (int64_t*)hm_copy_out(c->a_contig_lens.data(), c->a_contig_lens.size());
    if (!o_n || !o_l) { std::free(o_n); std::free(o_l); return fail(c, -7, "mirp_homolog_contigs: host allocation failed"); }
    *names = o_n; *names_bytes = (int64_t)blob.size(); *lens = o_l; *n_contigs = (int32_t)c->a_contig_names.size();
    return 0;
}

extern "C" int mirp_homolog_scan(mirp_ctx* c, const char* q_blob, const int64_t* q_off, int32_t n_q, const MirpHomologOpts* o, MirpHomologRec** recs,
                                 int64_t* n_recs, char** text, int32_t** also) {
    if (!c) return -1;
    c->reset_jobs_per_slot(3);
    if (n_q < 0 || !o || !recs || !n_recs || !text || !also || (n_q > 0 && (!q_blob || !q_off))) return fail(c, -1, "mirp_homolog_scan: bad argument");
    *recs = nullptr; *n_recs = 0; *text = nullptr; *also = nullptr;
    for (int i = 0; i < 24; i++) c->hm_stats[i] = 0;          // a refused call leaves no statistics of an earlier one
    for (int i = 0; i < 5; i++) c->hm_sec[i] = 0;
    if (o->max_mismatches < 0 || o->max_mismatches > 3 || o->precursor_len < 60 || o->precursor_len > 3000 || o->max_placements < 1 || o->reserved != 0)
        return fail(c, -1, "mirp_homolog_scan: bad options");
    if (n_q > (1 << 24)) return fail(c, -10, "mirp_homolog_scan: more than 16,777,216 known sequences");
    if (!c->a_ready) return fail(c, -1, "mirp_homolog_scan: no index (mirp_align_index first)");
    // ---- the queries as codes 0..3
    unsigned char code[256];
    std::memset(code, 4, sizeof code);
    code['A'] = code['a'] = 0; code['C'] = code['c'] = 1; code['G'] = code['g'] = 2; code['T'] = code['t'] = code['U'] = code['u'] = 3;
    std::vector<unsigned char> codes;
    std::vector<long long> roff((size_t)n_q + 1, 0);
    char msg[160];
    for (int q = 0; q < n_q; q++) {
        const long long L = q_off[q + 1] - q_off[q];
        if (L < 18 || L > 26) {
            std::snprintf(msg, sizeof msg, "mirp_homolog_scan: known sequence %d: a length outside 18..26", q + 1);
            return fail(c, -10, msg);
        }
        for (long long p = 0; p < L; p++) {
            const unsigned char k = code[(unsigned char)q_blob[q_off[q] + p]];
            if (k > 3) {
                std::snprintf(msg, sizeof msg, "mirp_homolog_scan: known sequence %d: a letter other than A C G T U", q + 1);
                return fail(c, -10, msg);
            }
            codes.push_back(k);
        }
        roff[(size_t)q + 1] = (long long)codes.size();
    }
    HIPCHK(c, hipSetDevice(c->device));
    long long* S = c->hm_stats;
    S[0] = n_q;
    // ---- placements
    double t = mirp::now();
    std::vector<unsigned long long> keys;
    long long st3[3];
    if (int rc = mirp_device_homolog_scan(c, codes.data(), roff.data(), n_q, o->max_mismatches, o->max_placements, keys, st3)) return rc;
    c->hm_sec[0] = mirp::now() - t;
    S[1] = st3[1]; S[2] = (long long)keys.size(); S[5] = st3[2];
    if ((long long)keys.size() != st3[0]) return fail(c, -2, "mirp_homolog_scan: the key passes returned another number of placements than the count");
    // ---- windows, fold, evaluation: chunks of placements bounded by the fold's output
    const int lines0 = c->hm_lines > 0 ? c->hm_lines : 96;
    const long long stride_est = ((long long)o->precursor_len + 3 + 7) / 8 * 8;
    long long chunk = std::max<long long>(1, std::min<long long>(1 << 15, (1ll << 30) / (lines0 * stride_est)));
    if (c->hm_chunk > 0) chunk = c->hm_chunk;
    const size_t n = keys.size();
    std::vector<HmWin> win(n);
    std::vector<HmEval> ev(n);
    std::vector<long long> text_off(n);
    std::vector<char> wtext;
    double sec3[3] = {0, 0, 0};
    long long est4[4] = {0, 0, 0, 0};
    for (size_t p0 = 0; p0 < n; p0 += (size_t)chunk) {
        const long long m = (long long)std::min<size_t>((size_t)chunk, n - p0);
        if (int rc = mirp_device_homolog_eval(c, keys.data() + p0, m, o->precursor_len, lines0, win.data() + p0, ev.data() + p0, wtext, text_off.data() + p0, est4, sec3))
            return rc;
        S[6]++;
    }
    S[7] = est4[0]; S[8] = est4[1]; S[9] = est4[3];
    for (int i = 0; i < 3; i++) c->hm_sec[1 + i] = sec3[i];
    // ---- merge: placements at one (contig, strand, interval) are one locus, named by the fewest mismatches, then the earlier query
    t = mirp::now();
    std::vector<size_t> pass;
    for (size_t i = 0; i < n; i++) {
        const HmEval& e = ev[i];
        if (e.best >= 0) { pass.push_back(i); continue; }
        if (e.code < 0) S[23]++;
        else if (e.code >= 1 && e.code <= 12) S[10 + e.code]++;
    }
    S[3] = (long long)pass.size();
    auto site = [&](size_t i) { return std::make_tuple(win[i].tid, win[i].strand, win[i].m0, win[i].m1); };
    std::stable_sort(pass.begin(), pass.end(), [&](size_t a, size_t b) {
        if (site(a) != site(b)) return site(a) < site(b);
        return win[a].mm < win[b].mm;          // the placements arrive in query order: among equal mismatches the earlier query stays first
    });
    std::vector<MirpHomologRec> out;
    std::vector<int32_t> al;
    std::vector<char> txt;
    for (size_t a = 0; a < pass.size();) {
        size_t z = a + 1;
        while (z < pass.size() && site(pass[z]) == site(pass[a])) z++;
        const size_t i = pass[a];
        const HmWin& w = win[i];
        const HmEval& e = ev[i];
        MirpHomologRec r;
        std::memset(&r, 0, sizeof r);
        r.query = w.query; r.contig = w.tid; r.strand = w.strand; r.mismatches = w.mm;
        r.mat_s = w.m0; r.mat_e = w.m1; r.star_s = e.star_s; r.star_e = e.star_e; r.fold_s = e.fold_s; r.fold_e = e.fold_e; r.win_s = w.ws; r.win_e = w.we;
        r.prime5 = e.prime5; r.total_bps = e.total_bps; r.total_dots = e.total_dots; r.energy = e.energy; r.line_len = e.line_len; r.ss_len = e.ss_len;
        r.n_also = (int32_t)(z - a - 1);
        r.also_off = (int64_t)(al.size() / 2);
        std::vector<std::pair<int, int>> others;
        for (size_t k = a + 1; k < z; k++) others.emplace_back(win[pass[k]].query, win[pass[k]].mm);
        std::sort(others.begin(), others.end());
        for (const auto& x : others) { al.push_back(x.first); al.push_back(x.second); }
        r.text_off = text_off[i];          // into wtext for now
        out.push_back(r);
        a = z;
    }
    std::stable_sort(out.begin(), out.end(), [](const MirpHomologRec& a, const MirpHomologRec& b) {
        return std::make_tuple(a.contig, a.fold_s, a.strand, a.mat_s, a.mat_e) < std::make_tuple(b.contig, b.fold_s, b.strand, b.mat_s, b.mat_e);
    });
    for (MirpHomologRec& r : out) {
        const size_t len = (size_t)(r.win_e - r.win_s) + (size_t)r.ss_len;
        const size_t at = txt.size();
        txt.insert(txt.end(), wtext.begin() + r.text_off, wtext.begin() + r.text_off + (long long)len);
        r.text_off = (int64_t)at;
    }
    S[4] = (long long)out.size();
    c->hm_sec[4] = mirp::now() - t;
    if (out.empty()) return 0;
    MirpHomologRec* o_r = hm_copy_out(out.data(), out.size());
    char* o_t = hm_copy_out(txt.data(), txt.size());
    int32_t* o_a = hm_copy_out(al.data(), al.size());
    if (!o_r || !o_t || !o_a) {
        std::free(o_r); std::free(o_t); std::free(o_a);
        return fail(c, -7, "mirp_homolog_scan: host allocation failed");
    }
    *recs = o_r; *n_recs = (int64_t)out.size(); *text = o_t; *also = o_a;
    return 0;
}
