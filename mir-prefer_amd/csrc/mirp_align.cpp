// C-ABI of the read alignment (mirp_align_index, mirp_align_reads): the FASTA parsing, the 2-bit packing of the reference, the SAM
// header and the batching of the reads on the host; align_kernels.hip does the index, the search and the SAM records on the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>
#include "mirp_fasta.h"

namespace {


// base codes: A C G T in either case 0..3, anything else 4
struct Codes {
    unsigned char t[256];
    Codes() {
        std::memset(t, 4, sizeof t);
        t['A'] = t['a'] = 0; t['C'] = t['c'] = 1; t['G'] = t['g'] = 2; t['T'] = t['t'] = 3;
    }
};
const Codes kCodes;

}  // namespace

int mirp::read_whole(mirp_ctx* c, const char* path, std::string& buf) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(c, -8, std::string("cannot open ") + path);
    fseeko(f, 0, SEEK_END);
    const long long n = (long long)ftello(f);
    fseeko(f, 0, SEEK_SET);
    try { buf.resize((size_t)n); } catch (...) { std::fclose(f); return fail(c, -7, std::string("host allocation failed reading ") + path); }
    const size_t got = n > 0 ? std::fread(&buf[0], 1, (size_t)n, f) : 0;
    std::fclose(f);
    if ((long long)got != n) return fail(c, -8, std::string("cannot read ") + path);
    return 0;
}

int mirp::pack_fasta(mirp_ctx* c, const char* const* paths, int n_paths, PackedFasta& out) {
    std::vector<unsigned>& pk = out.pk;
    std::vector<unsigned>& amb = out.amb;
    std::vector<unsigned>& cst = out.cst;
    std::vector<std::string>& names = out.names;
    std::vector<long long>& lens = out.lens;
    pk.clear(); amb.clear(); cst.clear(); names.clear(); lens.clear();
    std::unordered_set<std::string> seen;
    unsigned long long pos = 0;           // bases so far
    const unsigned long long limit = 1ull << 32;
    std::string buf;
    for (int fi = 0; fi < n_paths; fi++) {
        if (int rc = read_whole(c, paths[fi], buf)) return rc;
        bool open = false;
        std::string name;
        unsigned long long start = 0;
        auto finish = [&]() -> int {
            if (!open) return 0;
            open = false;
            if (pos == start) {
                std::fprintf(stderr, "Warning: contig %s in %s has length 0 and is dropped.\n", name.c_str(), paths[fi]);
                return 0;
            }
            if (!seen.insert(name).second) return fail(c, -10, std::string(paths[fi]) + ": duplicate contig name " + name);
            cst[start >> 5] |= 1u << (start & 31);
            names.push_back(name);
            lens.push_back((long long)(pos - start));
            return 0;
        };
        const int rc = for_lines(buf, [&](const char* raw, const char* a, const char* b) -> int {
            if (*raw == '>') {
                if (int r = finish()) return r;
                name = first_word(raw, b);
                if (name.empty()) return fail(c, -10, std::string(paths[fi]) + ": a header without a contig name");
                open = true;
                start = pos;
                return 0;
            }
            if (!open) return 0;                    // text before the first header is not part of any contig
            const long long n = b - a;
            if (pos + (unsigned long long)n >= limit) return fail(c, -10, "the reference has 2^32 bases or more (positions are 32-bit)");
            const size_t need_pk = (size_t)((pos + n + 15) >> 4) + 2, need_bm = (size_t)((pos + n + 31) >> 5) + 2;
            if (pk.size() < need_pk) pk.resize(std::max(need_pk, pk.size() * 2), 0u);
            if (amb.size() < need_bm) { amb.resize(std::max(need_bm, amb.size() * 2), 0u); cst.resize(amb.size(), 0u); }
            for (const char* q = a; q < b; q++, pos++) {
                const unsigned k = kCodes.t[(unsigned char)*q];
                if (k < 4) pk[pos >> 4] |= k << (2 * (pos & 15));
                else amb[pos >> 5] |= 1u << (pos & 31);
            }
            return 0;
        });
        if (rc) return rc;
        if (int r = finish()) return r;
    }
    const long long total = (long long)pos;
    pk.resize((size_t)((total + 15) / 16 + 2), 0u);
    amb.resize((size_t)((total + 31) / 32 + 2), 0u);
    cst.resize(amb.size(), 0u);
    for (size_t w = (size_t)(total >> 5); w < amb.size(); w++) {          // every position past the end is ambiguous
        const long long lo = (long long)w * 32;
        amb[w] |= lo >= total ? 0xffffffffu : ~((1u << (total - lo)) - 1u);
    }
    out.blob.clear();
    out.noff.assign(1, 0);
    out.cstart.assign(1, 0);
    for (size_t i = 0; i < names.size(); i++) {
        out.blob += names[i];
        out.noff.push_back((long long)out.blob.size());
        out.cstart.push_back(out.cstart.back() + (unsigned long long)lens[i]);
    }
    out.total = total;
    return 0;
}

// Parses the reference FASTA files (in order), packs them and builds the device-resident index.  seconds = {read + parse + pack, upload, keys, sort,
// positions + buckets}.  Contigs of length 0 are dropped with a warning on stderr; duplicate names, empty names and 2^32 bases or more are refused.
extern "C" int mirp_align_index(mirp_ctx* c, const char* const* paths, int32_t n_paths, int32_t* n_contigs, int64_t* total_out, double seconds[5]) {
    if (!c) return -1;
    if (!paths || n_paths < 1) return fail(c, -1, "mirp_align_index: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    c->a_ready = false;
    double sec[5] = {0, 0, 0, 0, 0};
    double t = mirp::now();
    mirp::PackedFasta ref;
    if (int rc = mirp::pack_fasta(c, paths, n_paths, ref)) return rc;
    std::vector<std::string>().swap(c->a_contig_names);
    sec[0] = mirp::now() - t;
    double dsec[4] = {0, 0, 0, 0};
    if (int rc = mirp_device_align_index(c, ref.pk.data(), ref.amb.data(), ref.cst.data(), ref.total, ref.cstart, ref.blob, ref.noff, dsec)) return rc;
    for (int i = 0; i < 4; i++) sec[1 + i] = dsec[i];
    c->a_contig_names = ref.names;
    c->a_contig_lens = ref.lens;
    if (n_contigs) *n_contigs = (int32_t)ref.names.size();
    if (total_out) *total_out = ref.total;
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}

// Aligns the reads of one FASTA file against the resident index and writes the SAM file.  stats = {reads, aligned, unaligned,
// suppressed by -m, records written}; seconds = {read + parse, upload, seeds, verify, sort, emit + download + write}.  Refusals (a read longer than
// 1,024 nt, more than 2^31 - 1 reads, a header without a name) happen before out_path is opened; on a later error the partial file is removed.
extern "C" int mirp_align_reads(mirp_ctx* c, const char* reads_path, const char* out_path, const char* pg_cl, int32_t v, int32_t k, int32_t m,
                                int32_t filter_unmapped, int64_t stats[5], double seconds[6]) {
    if (!c) return -1;
    if (!reads_path || !out_path || !pg_cl || v < 0 || v > 3 || k < 1 || m < 0) return fail(c, -1, "mirp_align_reads: bad argument");
    if (!c->a_ready) return fail(c, -1, "mirp_align_reads: no index (mirp_align_index first)");
    HIPCHK(c, hipSetDevice(c->device));
    double sec[6] = {0, 0, 0, 0, 0, 0};
    double t = mirp::now();
    std::string buf;
    if (int rc = mirp::read_whole(c, reads_path, buf)) return rc;
    std::vector<unsigned char> codes;
    std::vector<long long> roff(1, 0), qoff(1, 0);
    std::string qn;
    codes.reserve(buf.size() / 2);
    bool open = false;
    const long long max_reads = 0x7fffffffll;
    int rc = mirp::for_lines(buf, [&](const char* raw, const char* a, const char* b) -> int {
        if (*raw == '>') {
            if (open) roff.push_back((long long)codes.size());
            if ((long long)qoff.size() > max_reads) return fail(c, -10, std::string(reads_path) + ": more than 2^31 - 1 reads in one file");
            const std::string name = mirp::first_word(raw, b);
            if (name.empty()) return fail(c, -10, std::string(reads_path) + ": a read header without a name");
            qn += name;
            qoff.push_back((long long)qn.size());
            open = true;
            return 0;
        }
        if (!open) return 0;
        for (const char* q = a; q < b; q++) codes.push_back(kCodes.t[(unsigned char)*q]);
        if ((long long)codes.size() - roff.back() > 1024) {
            const size_t r = qoff.size() - 2;
            return fail(c, -10, std::string(reads_path) + ": read " + qn.substr((size_t)qoff[r], (size_t)(qoff[r + 1] - qoff[r])) +
                                    " is longer than 1,024 nt (not supported)");
        }
        return 0;
    });
    if (rc) return rc;
    if (open) roff.push_back((long long)codes.size());
    std::string().swap(buf);
    const long long n = (long long)roff.size() - 1;
    sec[0] = mirp::now() - t;

    mirp::OutFile out(out_path);
    if (!out.open()) return fail(c, -8, std::string("cannot write ") + out_path);
    std::string head = "@HD\tVN:1.0\tSO:unsorted\n";
    for (size_t i = 0; i < c->a_contig_names.size(); i++)
        head += "@SQ\tSN:" + c->a_contig_names[i] + "\tLN:" + std::to_string(c->a_contig_lens[i]) + "\n";
    head += std::string("@PG\tID:mir_prefer_amd.align\tCL:\"") + pg_cl + "\"\n";
    auto sink = [&](const char* p, size_t len) -> int { return out.write(p, len) ? 0 : fail(c, -8, std::string("cannot write ") + out_path); };
    rc = sink(head.data(), head.size());
    long long st4[4] = {0, 0, 0, 0};
    double dsec[5] = {0, 0, 0, 0, 0};
    // batches: bounded reads, bases and seeds (with e = 1 a read has up to 2 * (2 + 4 L) seeds)
    long long r0 = 0;
    c->a_batches = 0;
    while (!rc && r0 < n) {
        long long r1 = r0, seeds = 0;
        while (r1 < n && r1 - r0 < (1ll << 22) && roff[r1] - roff[r0] < (1ll << 28)) {
            const long long L = roff[r1 + 1] - roff[r1];
            const long long s = v == 0 ? 2 : v == 1 ? 4 : 2 * (2 + 4 * L);
            if (r1 > r0 && seeds + s > (1ll << 26)) break;
            seeds += s;
            r1++;
        }
        std::vector<long long> rb(roff.begin() + r0, roff.begin() + r1 + 1), qb(qoff.begin() + r0, qoff.begin() + r1 + 1);
        for (auto& x : rb) x -= roff[r0];
        for (auto& x : qb) x -= qoff[r0];
        rc = mirp_device_align_batch(c, codes.data() + roff[r0], rb.data(), qn.data() + qoff[r0], qb.data(), r1 - r0, v, k, m, filter_unmapped, sink, st4,
                                     dsec);
        r0 = r1;
        c->a_batches++;
    }
    if (rc) return rc;
    if (!out.commit()) return fail(c, -8, std::string("cannot write ") + out_path);
    for (int i = 0; i < 5; i++) sec[1 + i] = dsec[i];
    if (stats) {
        stats[0] = n;
        for (int i = 0; i < 4; i++) stats[1 + i] = st4[i];
    }
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}

extern "C" int64_t mirp_align_last_batches(const mirp_ctx* c) { return c ? c->a_batches : -1; }
