// The tailed SAM tokenizer of the isomiR counts (mirp_tokenize_sams_tailed): threaded, no device.  Where the ingest (mirp_ingest.cpp)
// keeps POS and len(SEQ) of every record, this one keeps the templated footprint and the 3' non-templated tail that `align --tail` reported: a record is
// (tid, strand, POS, m of `<m>M`, depth, sample) in the MirpAln layout plus a tail code.  The @SQ table, the sample names, the flag filter, the read-id
// depth, CRLF and the refusals with their messages are the ingest's (sam_text.h); a CIGAR that is neither `<m>M` nor a 3' soft clip, and a tail of more
// than 8 letters, skip the record and are counted.  Records stay in (sample, file) order: the scan (isomir_kernels.hip) needs no order.
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../include/mirprefer.h"
#include "sam_text.h"

namespace {

using namespace samtext;

struct IsoChunk {
    std::vector<MirpAln> recs;
    std::vector<uint32_t> tails;
    long long skip_cigar = 0, skip_long = 0;
    std::string err;
};

// A 0 C 1 G 2 T 3 (U counts as T), anything else N 4; either case
inline int tail_digit(char ch) {
    switch (ch) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 4;
    }
}

// code of the t digits d[0 .. t) (sequenced order), t 1..8: (5^t - 5) / 4 + 1 + the digits as a base-5 number; 0 for t = 0
inline uint32_t tail_code(const int* d, int t) {
    if (t == 0) return 0;
    uint32_t pw = 1, v = 0;
    for (int i = 0; i < t; i++) { v = v * 5 + (uint32_t)d[i]; pw *= 5; }
    return (pw - 5) / 4 + 1 + v;
}

// digits then one op letter at *p; false when there is no digit, no letter, or the number passes 10^9
inline bool cigar_op(const char*& p, const char* ce, long* len, char* op) {
    const char* d0 = p;
    long v = 0;
    while (p < ce && *p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); p++; if (v > 1000000000L) return false; }
    if (p == d0 || p >= ce) return false;
    *len = v;
    *op = *p++;
    return true;
}

void parse_chunk(const char* b, const char* e, const NameTable* tab, int sample, IsoChunk* out) {
    const char* s = b;
    out->recs.reserve((size_t)(e - b) / 64 + 16);
    out->tails.reserve((size_t)(e - b) / 64 + 16);
    int last_tid = -1;
    const char* last_name = nullptr;
    size_t last_len = 0;
    while (s < e) {
        const char* le = (const char*)memchr(s, '\n', (size_t)(e - s));
        if (!le) le = e;
        const char* lend = (le > s && le[-1] == '\r') ? le - 1 : le;
        const char* line = s;
        s = le + 1;
        if (lend <= line || *line == '@') continue;
        const char* f[11];
        const char* fe[11];
        int nf = 0;
        const char* q = line;
        while (nf < 11) {
            f[nf] = q;
            const char* t = (const char*)memchr(q, '\t', (size_t)(lend - q));
            if (!t) t = lend;
            fe[nf++] = t;
            if (t >= lend) break;
            q = t + 1;
        }
        if (nf < 10) continue;
        long flag = 0;
        if (!parse_uint(f[1], fe[1], &flag)) { out->err = "SAM flag is not a number"; return; }
        if (flag & 0x704) continue;
        const long depth = read_id_depth(f[0], fe[0]);
        if (depth < 0) { out->err = "Read Id format is not right. Read id must be in \"samplename_rA_xN\" format."; return; }
        const size_t nl = (size_t)(fe[2] - f[2]);
        int tid;
        if (last_name && nl == last_len && std::memcmp(last_name, f[2], nl) == 0) tid = last_tid;
        else {
            tid = tab->find(f[2], nl);
            if (tid < 0) { out->err = "alignment refers to a sequence that is not in the @SQ header: " + std::string(f[2], fe[2]); return; }
            last_tid = tid; last_name = f[2]; last_len = nl;
        }
        long pos = 0;
        if (!parse_uint(f[3], fe[3], &pos) || pos > 0x7ffffff0L) { out->err = "SAM position is not a number"; return; }
        const char* seq = f[9];
        const long rl = (long)(fe[9] - f[9]);
        if (rl > 65535) { out->err = "read longer than 65535"; return; }
        const char* c = f[5];
        const char* ce = fe[5];
        if (ce - c == 1 && *c == '*') { out->err = "alignment without a CIGAR string"; return; }
        const bool minus = (flag & 16) != 0;
        const bool no_seq = rl == 1 && *seq == '*';
        // `<m>M`, or a 3' clip: `<m>M<t>S` on +, `<t>S<m>M` on -
        long m = 0, t = 0, l1 = 0, l2 = 0;
        char o1 = 0, o2 = 0;
        const char* p = c;
        bool ok = cigar_op(p, ce, &l1, &o1);
        if (ok && p == ce) { ok = o1 == 'M'; m = l1; }
        else if (ok) {
            ok = cigar_op(p, ce, &l2, &o2) && p == ce;
            if (ok && !minus && o1 == 'M' && o2 == 'S') { m = l1; t = l2; }
            else if (ok && minus && o1 == 'S' && o2 == 'M') { t = l1; m = l2; }
            else ok = false;
            if (t < 1) ok = false;
        }
        if (ok && (m < 1 || m > 65535)) ok = false;
        if (ok && !no_seq && rl != m + t) ok = false;
        if (ok && t > 0 && no_seq) ok = false;
        if (!ok) { out->skip_cigar++; continue; }
        int dg[8];
        int tl = 0;
        if (t > 0) {
            if (t > 8) { out->skip_long++; continue; }
            tl = (int)t;
            if (!minus) for (int i = 0; i < tl; i++) dg[i] = tail_digit(seq[m + i]);
            else for (int i = 0; i < tl; i++) { const int d = tail_digit(seq[tl - 1 - i]); dg[i] = d < 4 ? 3 - d : 4; }      // reverse complement of SEQ[:t]
        } else if (nf == 11 && fe[10] < lend) {          // optional fields: the first XT:Z: (the --tail-trim form)
            const char* a = fe[10] + 1;
            while (a <= lend) {
                const char* z = (const char*)memchr(a, '\t', (size_t)(lend - a));
                if (!z) z = lend;
                if (z - a >= 5 && std::memcmp(a, "XT:Z:", 5) == 0) {
                    if (z - (a + 5) > 8) tl = -1;
                    else for (const char* x = a + 5; x < z; x++) dg[tl++] = tail_digit(*x);
                    break;
                }
                a = z + 1;
            }
            if (tl < 0) { out->skip_long++; continue; }
        }
        MirpAln r;
        r.tid = tid; r.pos = (int32_t)pos; r.depth = (uint32_t)depth; r.len = (uint16_t)m;
        r.strand = minus ? 1 : 0; r.sample = (uint8_t)sample;
        out->recs.push_back(r);
        out->tails.push_back(tail_code(dg, tl));
    }
}

char* pack_names(const std::vector<std::string>& v) {
    size_t nb = 0;
    for (auto& s : v) nb += s.size() + 1;
    char* out = (char*)std::malloc(std::max<size_t>(nb, 1));
    if (!out) return nullptr;
    char* w = out;
    for (auto& s : v) { std::memcpy(w, s.c_str(), s.size() + 1); w += s.size() + 1; }
    return out;
}

}  // namespace

extern "C" void mirp_free_tailed_sam_data(MirpTailedSamData* d) {
    if (!d) return;
    std::free(d->contig_names); std::free(d->contig_len); std::free(d->sample_names); std::free(d->alns); std::free(d->tails);
    std::memset(d, 0, sizeof(*d));
}

extern "C" int mirp_tokenize_sams_tailed(const char* const* paths, int32_t n_paths, int32_t n_threads, MirpTailedSamData* out, char* errbuf, size_t errbuf_len) {
    auto bail = [&](const std::string& m) {
        if (errbuf && errbuf_len) std::snprintf(errbuf, errbuf_len, "%s", m.c_str());
        if (out) mirp_free_tailed_sam_data(out);
        return -1;
    };
    if (out) std::memset(out, 0, sizeof(*out));
    if (!paths || n_paths < 1 || !out) return bail("mirp_tokenize_sams_tailed: bad argument");
    if (n_paths > MIRP_MAX_SAMPLES) return bail("mirp_tokenize_sams_tailed: too many samples");
    if (n_threads < 1) n_threads = usable_cpus();
    NameTable tab;
    std::vector<int64_t> lens;
    std::vector<std::string> samples;
    std::vector<std::vector<IsoChunk>> per_file((size_t)n_paths);
    for (int fi = 0; fi < n_paths; fi++) {
        Mapped m;
        if (!m.open(paths[fi])) return bail(std::string("cannot open ") + paths[fi]);
        const char* e = m.p + m.n;
        std::string sname;
        const char* s = read_header(m.p, e, fi == 0, &tab, &lens, &sname);
        if (fi == 0) {
            if (tab.names.empty()) return bail("Can not get the sequence length from the input SAM files. Make sure SAM files have headers.");
            tab.build();
        }
        samples.push_back(sname);
        const std::vector<const char*> cuts = cut_body(s, e, n_threads);
        const int nt = (int)cuts.size() - 1;
        per_file[fi].resize(nt);
        std::vector<std::thread> th;
        for (int k = 0; k < nt; k++) th.emplace_back(parse_chunk, cuts[k], cuts[k + 1], &tab, fi, &per_file[fi][k]);
        for (auto& t : th) t.join();
        for (auto& c : per_file[fi]) if (!c.err.empty()) return bail(c.err);
    }
    size_t n = 0;
    for (auto& f : per_file) for (auto& c : f) { n += c.recs.size(); out->skipped_cigar += c.skip_cigar; out->skipped_long_tail += c.skip_long; }
    out->alns = (MirpAln*)std::malloc(std::max<size_t>(n, 1) * sizeof(MirpAln));
    out->tails = (uint32_t*)std::malloc(std::max<size_t>(n, 1) * sizeof(uint32_t));
    out->contig_names = pack_names(tab.names);
    out->sample_names = pack_names(samples);
    out->contig_len = (int64_t*)std::malloc(std::max<size_t>(lens.size(), 1) * sizeof(int64_t));
    if (!out->alns || !out->tails || !out->contig_names || !out->sample_names || !out->contig_len) return bail("out of memory");
    size_t o = 0;
    for (auto& f : per_file)
        for (auto& c : f) {
            if (!c.recs.empty()) {
                std::memcpy(out->alns + o, c.recs.data(), c.recs.size() * sizeof(MirpAln));
                std::memcpy(out->tails + o, c.tails.data(), c.tails.size() * sizeof(uint32_t));
            }
            o += c.recs.size();
        }
    for (size_t k = 0; k < lens.size(); k++) out->contig_len[k] = lens[k];
    out->n_contigs = (int32_t)tab.names.size();
    out->n_samples = (int32_t)samples.size();
    out->n_alns = (int64_t)n;
    return 0;
}
