// C-ABI of the known-miRNA annotation (mirp_annotate_scan): the query FASTA and the known FASTA files are parsed with §14's parser
// (the known files in its skip-length mode), filtered by --species, packed as one 64-bit word of 2-bit codes plus an unknown mask each;
// annotate_kernels.hip finds, orders and cuts the hits; the lines of both files are written here from the downloaded keys (8 bytes per hit: the
// text needs nothing the host does not hold, and the summary joins each query's first line with its hit count in the same walk).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_fasta.h"
#include "mirp_mirna.h"

namespace {


const long long kMaxKnown = 1ll << 24;

bool alnum(unsigned char ch) { return (ch >= '0' && ch <= '9') || (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); }

// (mir|let|lin)-?([0-9]+) at w[p ..], letters in either case -> the family, or "" without a match
std::string family_at(const std::string& w, size_t p) {
    if (p + 3 > w.size()) return "";
    char t[4] = {0, 0, 0, 0};
    for (int i = 0; i < 3; i++) t[i] = (char)(w[p + i] | 0x20);
    const bool mir = !std::strcmp(t, "mir"), let = !std::strcmp(t, "let"), lin = !std::strcmp(t, "lin");
    if (!mir && !let && !lin) return "";
    size_t a = p + 3;
    if (a < w.size() && w[a] == '-') a++;
    size_t z = a;
    while (z < w.size() && w[z] >= '0' && w[z] <= '9') z++;
    if (z == a) return "";
    return std::string(mir ? "miR" : let ? "let-" : "lin-") + w.substr(a, z - a);
}

// ^(?:[A-Za-z0-9]+-)?(mir|let|lin)-?([0-9]+), case-insensitive; without a match the id itself
std::string family_of(const std::string& w) {
    size_t r = 0;
    while (r < w.size() && alnum((unsigned char)w[r])) r++;
    if (r > 0 && r < w.size() && w[r] == '-') {
        const std::string f = family_at(w, r + 1);
        if (!f.empty()) return f;
    }
    const std::string f = family_at(w, 0);
    return f.empty() ? w : f;
}

AnPacked pack(const unsigned char* cd, int L) {
    AnPacked p{0ull, 0u, L};
    for (int i = 0; i < L; i++) {
        if (cd[i] > 3) p.unk |= 1u << i;
        else p.word |= (unsigned long long)cd[i] << (2 * i);
    }
    return p;
}

}  // namespace

extern "C" int mirp_annotate_scan(mirp_ctx* c, const char* query_path, const char* const* known_paths, int32_t n_known, const MirpAnnotateOpts* o,
                                  const char* out_path, const char* summary_path, int64_t stats[12], double seconds[6]) {
    if (!c) return -1;
    if (!query_path || !known_paths || n_known < 1 || !o || !out_path || !summary_path || (o->n_species > 0 && !o->species))
        return fail(c, -1, "mirp_annotate_scan: bad argument");
    if (o->max_offset < 0 || o->max_offset > 4 || o->max_mismatches < 0 || o->max_mismatches > 6 || o->max_lines < 0 || o->n_species < 0)
        return fail(c, -1, "mirp_annotate_scan: bad options");
    HIPCHK(c, hipSetDevice(c->device));
    mirp::OutFile fh(out_path), fs(summary_path);   // every return before the commits discards both: a refused or failed run has no output, not even an old one
    double sec[6] = {0, 0, 0, 0, 0, 0};
    double t = mirp::now();
    mirp::Mirnas Q, A;
    long long skipped = 0;
    if (int rc = mirp::parse_mirnas(c, query_path, Q)) return rc;
    for (int f = 0; f < n_known; f++)
        if (int rc = mirp::parse_mirnas(c, known_paths[f], A, &skipped)) return rc;
    // the kept known sequences: the printed id is the first word of the header; --species keeps the ids that start with a listed prefix and '-'
    std::vector<std::string> species;
    const char* sp = o->species;
    for (int i = 0; i < o->n_species; i++) {
        species.emplace_back(sp);
        sp += species.back().size() + 1;
        if (species.back().empty()) return fail(c, -1, "mirp_annotate_scan: an empty species prefix");
    }
    std::vector<long long> src;                     // kept known -> record of A
    std::vector<std::string> kid, kfam;
    for (long long r = 0; r < (long long)A.lens.size(); r++) {
        const char* a = A.names.data() + A.noff[(size_t)r];
        const char* b = A.names.data() + A.noff[(size_t)r + 1];
        const char* z = a;
        while (z < b && !mirp::fa_ws((unsigned char)*z)) z++;
        std::string id(a, z);
        bool keep = species.empty();
        for (const std::string& s : species)
            if (id.size() > s.size() && id.compare(0, s.size(), s) == 0 && id[s.size()] == '-') { keep = true; break; }
        if (!keep) continue;
        if ((long long)src.size() >= kMaxKnown) return fail(c, -10, "more than 16,777,216 known sequences are kept");
        src.push_back(r);
        kfam.push_back(family_of(id));
        kid.push_back(std::move(id));
    }
    const long long nq = (long long)Q.lens.size(), nk = (long long)src.size();
    std::vector<AnPacked> pq((size_t)nq), pk((size_t)nk);
    long long lq[33] = {0}, lk[33] = {0};
    for (long long i = 0; i < nq; i++) { pq[(size_t)i] = pack(Q.codes.data() + 32 * i, Q.lens[(size_t)i]); lq[Q.lens[(size_t)i]]++; }
    for (long long i = 0; i < nk; i++) { pk[(size_t)i] = pack(A.codes.data() + 32 * src[(size_t)i], A.lens[(size_t)src[(size_t)i]]); lk[pk[(size_t)i].len]++; }
    const int E = o->max_offset;
    long long evals = 0;                            // pairs x admissible shifts: 2 E + 1 - |Lq - Lk| shifts have both offsets within E
    for (int a = 12; a <= 32; a++)
        for (int b = 12; b <= 32; b++) evals += lq[a] * lk[b] * std::max(0, 2 * E + 1 - std::abs(a - b));
    sec[0] = mirp::now() - t;

    if (!fh.open()) return fail(c, -8, std::string("cannot write ") + out_path);
    if (!fs.open()) return fail(c, -8, std::string("cannot write ") + summary_path);
    std::string text = "query\tknown\tfamily\tdistance\tmismatches\toffset5\toffset3\tquery_5to3\tpairs\tknown_5to3\n", summ;
    auto flush = [&](std::string& s, mirp::OutFile& f, const char* path) -> int {
        if (!f.write(s.data(), s.size())) return fail(c, -8, std::string("cannot write ") + path);
        s.clear();
        return 0;
    };
    std::vector<unsigned> hits;
    long long next_q = 0, cur_q = -1, n_class[4] = {0, 0, 0, 0};
    const char* RNA = "ACGUN";
    char num[96];
    auto qname = [&](std::string& s, long long q) { s.append(Q.names, (size_t)Q.noff[(size_t)q], (size_t)(Q.noff[(size_t)q + 1] - Q.noff[(size_t)q])); };
    auto novel_until = [&](long long q1) {
        for (; next_q < q1; next_q++) {
            qname(summ, next_q);
            std::snprintf(num, sizeof num, "\t%d\tnovel\t.\t.\t.\t.\t.\t.\t0\n", Q.lens[(size_t)next_q]);
            summ += num;
            n_class[3]++;
        }
    };
    const MirpAnSink sink = [&](long long qbase, const unsigned long long* keys, size_t n) -> int {
        for (size_t i = 0; i < n; i++) {
            const unsigned long long key = keys[i];
            const long long q = qbase + (long long)(key >> 35), k = (long long)(key >> 4) & 0xffffff;
            const int dist = (int)(key >> 31) & 15, mm = (int)(key >> 28) & 7, d = (int)(key & 15) - 4;
            const int Lq = Q.lens[(size_t)q], Lk = pk[(size_t)k].len, off3 = Lq + d - Lk;
            if (q != cur_q) {
                novel_until(q);
                const int cls = dist == 0 ? 0 : mm == 0 ? 1 : 2;
                qname(summ, q);
                std::snprintf(num, sizeof num, "\t%d\t%s\t", Lq, cls == 0 ? "identical" : cls == 1 ? "isomir" : "homolog");
                summ += num;
                summ += kid[(size_t)k];
                summ += '\t';
                summ += kfam[(size_t)k];
                std::snprintf(num, sizeof num, "\t%d\t%d\t%d\t%d\t%u\n", dist, mm, d, off3, hits[(size_t)q]);
                summ += num;
                n_class[cls]++;
                cur_q = q;
                next_q = q + 1;
            }
            qname(text, q);
            text += '\t';
            text += kid[(size_t)k];
            text += '\t';
            text += kfam[(size_t)k];
            std::snprintf(num, sizeof num, "\t%d\t%d\t%d\t%d\t", dist, mm, d, off3);
            text += num;
            const unsigned char* qc = Q.codes.data() + 32 * q;
            const unsigned char* kc = A.codes.data() + 32 * src[(size_t)k];
            const int c0 = std::min(d, 0), c1 = std::max(Lq + d, Lk);          // the columns, as positions of the known sequence
            for (int x = c0; x < c1; x++) text += x - d >= 0 && x - d < Lq ? RNA[qc[x - d]] : '-';
            text += '\t';
            for (int x = c0; x < c1; x++) {
                const bool hq = x - d >= 0 && x - d < Lq, hk = x >= 0 && x < Lk;
                text += !(hq && hk) ? '.' : qc[x - d] < 4 && qc[x - d] == kc[x] ? '|' : 'x';
            }
            text += '\t';
            for (int x = c0; x < c1; x++) text += x >= 0 && x < Lk ? RNA[kc[x]] : '-';
            text += '\n';
            if (text.size() > (1u << 22))
                if (int rc = flush(text, fh, out_path)) return rc;
            if (summ.size() > (1u << 22))
                if (int rc = flush(summ, fs, summary_path)) return rc;
        }
        return 0;
    };
    long long st3[3];
    double dsec[5];
    int rc = mirp_device_annotate(c, pq, pk, E, o->max_mismatches, o->max_lines, hits, sink, st3, dsec);
    if (!rc) {
        novel_until(nq);
        rc = flush(text, fh, out_path);
        if (!rc) rc = flush(summ, fs, summary_path);
    }
    if (rc) return rc;
    if (!fh.commit() || !fs.commit()) {
        fh.discard();
        return fail(c, -8, std::string("cannot write ") + out_path);
    }
    for (int i = 0; i < 5; i++) sec[1 + i] = dsec[i];
    if (stats) {
        stats[0] = nq;
        stats[1] = nk;
        stats[2] = skipped;
        stats[3] = nq * nk;
        stats[4] = evals;
        stats[5] = st3[0];
        for (int i = 0; i < 4; i++) stats[6 + i] = n_class[i];
        stats[10] = st3[1];
        stats[11] = st3[2];
    }
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}
