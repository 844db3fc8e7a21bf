// C-ABI of the read alignment (mirp_align_index, mirp_align_reads): the FASTA parsing, the 2-bit packing of the reference, the SAM
// header and the batching of the reads on the host; align_kernels.hip does the index, the search and the SAM records on the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

namespace {

// depth of a read for the placement: the number after the last _x of a QNAME that matches _x[0-9]+$, if it is <= 2^32 - 1; otherwise 1
unsigned depth_of(const char* q, size_t len) {
    size_t i = len;
    while (i > 0 && q[i - 1] >= '0' && q[i - 1] <= '9') i--;
    if (i == len || i < 2 || q[i - 1] != 'x' || q[i - 2] != '_') return 1u;
    while (i < len - 1 && q[i] == '0') i++;
    if (len - i > 10) return 1u;
    unsigned long long d = 0;
    for (; i < len; i++) d = d * 10 + (unsigned long long)(q[i] - '0');
    return d <= 0xffffffffull ? (unsigned)d : 1u;
}

void swap_buf(DevBuf& a, DevBuf& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

// the hits of a batch of pass 1 that stay resident for pass 2
struct KeptBatch {
    DevBuf items, off, best, supp;
    long long n_items = 0;
    bool kept = false;
};

// mirp_align_reads (place == nullptr, tail == nullptr), mirp_align_reads_placed and mirp_align_reads_tailed (never both).  stats[8], seconds[8];
// with tail, stats[5..6] = {tailed, suppressed in the tail pass} and sec[6] = the tail pass
int align_file(mirp_ctx* c, const char* reads_path, const char* out_path, const char* pg_cl, int v, int k, int m, int filter_unmapped,
               const MirpAlignPlaceOpts* place, const MirpAlignTailOpts* tail, const char* tails_path, long long stats[8], double sec[8]) {
    double t = mirp::now();
    std::string buf;
    if (int rc = mirp::read_whole(c, reads_path, buf)) return rc;
    std::vector<unsigned char> codes;
    std::vector<long long> roff(1, 0), qoff(1, 0);
    std::vector<unsigned> depth;
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
            if (place || tail) depth.push_back(depth_of(name.data(), name.size()));
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

    // batches: bounded reads, bases and seeds (with e = 1 a read has up to 2 * (2 + 4 L) seeds)
    std::vector<long long> cut(1, 0);
    for (long long r0 = 0; r0 < n;) {
        long long r1 = r0, seeds = 0;
        while (r1 < n && r1 - r0 < (1ll << 22) && roff[r1] - roff[r0] < (1ll << 28)) {
            const long long L = roff[r1 + 1] - roff[r1];
            const long long s = v == 0 ? 2 : v == 1 ? 4 : 2 * (2 + 4 * L);
            if (r1 > r0 && seeds + s > (1ll << 26)) break;
            seeds += s;
            r1++;
        }
        cut.push_back(r1);
        r0 = r1;
    }
    const size_t nbatch = cut.size() - 1;
    c->a_batches = (long long)nbatch;
    std::vector<long long> rb, qb;
    double dsec[6] = {0, 0, 0, 0, 0, 0};
    auto upload = [&](size_t b) -> int {
        const long long r0 = cut[b], r1 = cut[b + 1];
        rb.assign(roff.begin() + r0, roff.begin() + r1 + 1);
        qb.assign(qoff.begin() + r0, qoff.begin() + r1 + 1);
        for (auto& x : rb) x -= roff[r0];
        for (auto& x : qb) x -= qoff[r0];
        return mirp_device_align_upload(c, codes.data() + roff[r0], rb.data(), qn.data() + qoff[r0], qb.data(), place || tail ? depth.data() + r0 : nullptr, r1 - r0, dsec);
    };

    // ---- placement, pass 1: the hits of every batch, the unique reads of the whole file
    long long st7[7] = {0, 0, 0, 0, 0, 0, 0};      // aligned, unaligned, suppressed, records, unique, by density, at random
    std::vector<KeptBatch> kept(place ? nbatch : 0);
    long long n_unique = 0;
    if (place) {
        const double t1 = mirp::now();
        const long long cap = c->a_place_cap > 0 ? c->a_place_cap : (1ll << 28);
        long long resident = 0;
        c->a_place_realigned = 0;
        for (size_t b = 0; b < nbatch; b++) {
            const long long nb = cut[b + 1] - cut[b];
            long long NI = 0;
            if ((rc = upload(b)) || (rc = mirp_device_align_hits(c, nb, v, m, filter_unmapped, nullptr, &NI, dsec))) return rc;
            unsigned long long cnt[3] = {0, 0, 0};
            HIPCHK(c, hipMemcpy(cnt, c->a_small.p, sizeof cnt, hipMemcpyDeviceToHost));
            for (int i = 0; i < 3; i++) st7[i] += (long long)cnt[i];
            t = mirp::now();
            if ((rc = mirp_device_place_unique(c, nb, &n_unique))) return rc;
            sec[6] += mirp::now() - t;
            if (nbatch == 1) break;                     // pass 2 follows on the same resident hits
            if (resident + NI <= cap) {
                swap_buf(kept[b].items, c->a_items); swap_buf(kept[b].off, c->a_off); swap_buf(kept[b].best, c->a_best); swap_buf(kept[b].supp, c->a_supp);
                kept[b].n_items = NI;
                kept[b].kept = true;
                resident += NI;
            } else {
                c->a_place_realigned++;
            }
        }
        t = mirp::now();
        unsigned long long depth_sum = 0;
        if ((rc = mirp_device_place_prepare(c, n_unique, &depth_sum))) return rc;
        sec[6] += mirp::now() - t;
        sec[7] = mirp::now() - t1;
        if (depth_sum >= ((1ull << 63) + (unsigned long long)m - 1) / (unsigned long long)m)      // m * depth_sum >= 2^63
            return fail(c, -10, std::string(reads_path) + ": -m times the total depth of the uniquely mapped reads is 2^63 or more (placement weights would overflow)");
    }

    mirp::OutFile out(out_path);
    std::unique_ptr<mirp::OutFile> tails_out(tail ? new mirp::OutFile(tails_path) : nullptr);       // both files go if either fails
    if (!out.open()) return fail(c, -8, std::string("cannot write ") + out_path);
    if (tail && !tails_out->open()) return fail(c, -8, std::string("cannot write ") + tails_path);
    if (tail && (rc = mirp_device_align_tail_clear(c))) return rc;
    std::string head = "@HD\tVN:1.0\tSO:unsorted\n";
    for (size_t i = 0; i < c->a_contig_names.size(); i++)
        head += "@SQ\tSN:" + c->a_contig_names[i] + "\tLN:" + std::to_string(c->a_contig_lens[i]) + "\n";
    head += std::string("@PG\tID:mir_prefer_amd.align\tCL:\"") + pg_cl + "\"\n";
    auto sink = [&](const char* p, size_t len) -> int { return out.write(p, len) ? 0 : fail(c, -8, std::string("cannot write ") + out_path); };
    rc = sink(head.data(), head.size());
    for (size_t b = 0; !rc && b < nbatch; b++) {
        const long long nb = cut[b + 1] - cut[b];
        long long NI = 0;
        unsigned long long cnt[8];
        if (!place) {
            if ((rc = upload(b)) || (rc = mirp_device_align_hits(c, nb, v, m, filter_unmapped, tail, &NI, dsec)) ||
                (rc = mirp_device_align_emit(c, nb, NI, v, k, m, filter_unmapped, 0, tail, sink, cnt, dsec)))
                break;
            for (int i = 0; i < 4; i++) st7[i] += (long long)cnt[i];
            if (tail) {             // the end-to-end pass counted these reads as unaligned
                unsigned long long tl[2] = {0, 0};
                HIPCHK(c, hipMemcpy(tl, (const unsigned long long*)c->a_small.p + 8, sizeof tl, hipMemcpyDeviceToHost));
                st7[0] += (long long)tl[0];
                st7[1] -= (long long)(tl[0] + tl[1]);
                st7[2] += (long long)tl[1];
                st7[4] += (long long)tl[0];
                st7[5] += (long long)tl[1];
            }
            continue;
        }
        // ---- placement, pass 2: the batch's hits again (resident, or aligned a second time), the weights, the picks, one record per read
        if (nbatch > 1) {
            if ((rc = upload(b))) break;
            if (kept[b].kept) {
                swap_buf(kept[b].items, c->a_items); swap_buf(kept[b].off, c->a_off); swap_buf(kept[b].best, c->a_best); swap_buf(kept[b].supp, c->a_supp);
                NI = kept[b].n_items;
            } else if ((rc = mirp_device_align_hits(c, nb, v, m, filter_unmapped, nullptr, &NI, dsec))) {
                break;
            }
        } else {
            HIPCHK(c, hipMemcpy(&NI, (const long long*)c->a_off.p + nb, 8, hipMemcpyDeviceToHost));
        }
        t = mirp::now();
        if ((rc = mirp_device_place_pick(c, nb, NI, place->mode, place->window, place->seed, n_unique))) break;
        sec[6] += mirp::now() - t;
        if ((rc = mirp_device_align_emit(c, nb, NI, v, k, m, filter_unmapped, place->mode, nullptr, sink, cnt, dsec))) break;
        st7[3] += (long long)cnt[3];
        for (int i = 0; i < 3; i++) st7[4 + i] += (long long)cnt[5 + i];
    }
    if (rc) return rc;
    if (tail) {                     // the summary of the whole file: one row per tail string among its tailed reads
        std::vector<MirpTailRow> rows;
        if ((rc = mirp_device_align_tail_rows(c, rows))) return rc;
        std::string text = "tail\tlength\treads\tdepth\n";
        for (const MirpTailRow& r : rows)
            text += r.tail + "\t" + std::to_string(r.tail.size()) + "\t" + std::to_string(r.reads) + "\t" + std::to_string(r.depth) + "\n";
        if (!tails_out->write(text.data(), text.size())) return fail(c, -8, std::string("cannot write ") + tails_path);
    }
    if (!out.commit()) return fail(c, -8, std::string("cannot write ") + out_path);
    if (tail && !tails_out->commit()) { out.discard(); return fail(c, -8, std::string("cannot write ") + tails_path); }
    for (int i = 0; i < 5; i++) sec[1 + i] = dsec[i];
    if (tail) sec[6] = dsec[5];
    stats[0] = n;
    for (int i = 0; i < 7; i++) stats[1 + i] = st7[i];
    return 0;
}

}  // namespace

// Aligns the reads of one FASTA file against the resident index and writes the SAM file.  stats = {reads, aligned, unaligned,
// suppressed by -m, records written}; seconds = {read + parse, upload, seeds, verify, sort, emit + download + write}.  Refusals (a read longer than
// 1,024 nt, more than 2^31 - 1 reads, a header without a name) happen before out_path is opened; on a later error the partial file is removed.
extern "C" int mirp_align_reads(mirp_ctx* c, const char* reads_path, const char* out_path, const char* pg_cl, int32_t v, int32_t k, int32_t m,
                                int32_t filter_unmapped, int64_t stats[5], double seconds[6]) {
    if (!c) return -1;
    c->text_pieces = 0;
    if (!reads_path || !out_path || !pg_cl || v < 0 || v > 3 || k < 1 || m < 0) return fail(c, -1, "mirp_align_reads: bad argument");
    if (!c->a_ready) return fail(c, -1, "mirp_align_reads: no index (mirp_align_index first)");
    HIPCHK(c, hipSetDevice(c->device));
    long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = align_file(c, reads_path, out_path, pg_cl, v, k, m, filter_unmapped, nullptr, nullptr, nullptr, st, sec)) return rc;
    if (stats) for (int i = 0; i < 5; i++) stats[i] = st[i];
    if (seconds) std::memcpy(seconds, sec, 6 * sizeof(double));
    return 0;
}

// mirp_align_reads with the placement of multi-mapped reads (DESIGN.md §12 "Placement"): one record per read.  place == NULL or mode 0: exactly
// mirp_align_reads.  stats = mirp_align_reads' five, then {unique, placed by density, placed at random}; seconds = mirp_align_reads' six, then
// {unique list + sort + prefix + weights + picks, the whole of pass 1}.  With a mode, m must be 1..10000 and k is not consulted; a file whose
// m * (total depth of its unique reads) is 2^63 or more is refused (-10) before out_path is opened.
extern "C" int mirp_align_reads_placed(mirp_ctx* c, const char* reads_path, const char* out_path, const char* pg_cl, int32_t v, int32_t k, int32_t m,
                                       int32_t filter_unmapped, const MirpAlignPlaceOpts* place, int64_t stats[8], double seconds[8]) {
    if (!c) return -1;
    c->text_pieces = 0;
    const bool on = place && place->mode != 0;
    if (!reads_path || !out_path || !pg_cl || v < 0 || v > 3 || k < 1 || m < 0) return fail(c, -1, "mirp_align_reads_placed: bad argument");
    if (on && (place->mode < 1 || place->mode > 2 || place->window < 0 || place->window > 10000 || m < 1 || m > 10000))
        return fail(c, -1, "mirp_align_reads_placed: bad placement argument (mode 0..2, window 0..10000, m 1..10000)");
    if (!c->a_ready) return fail(c, -1, "mirp_align_reads: no index (mirp_align_index first)");
    HIPCHK(c, hipSetDevice(c->device));
    long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = align_file(c, reads_path, out_path, pg_cl, v, k, m, filter_unmapped, on ? place : nullptr, nullptr, nullptr, st, sec)) return rc;
    if (stats) for (int i = 0; i < 8; i++) stats[i] = st[i];
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}

// mirp_align_reads with the search for 3' non-templated tails among the reads it leaves without a hit (DESIGN.md §12 "Tails").  tail == NULL or
// max_tail 0: exactly mirp_align_reads, and tails_path is not touched.  stats = mirp_align_reads' five (aligned includes the tailed reads, suppressed
// those suppressed in the tail pass), then {tailed, suppressed in the tail pass}; seconds = mirp_align_reads' six, then the tail pass.
extern "C" int mirp_align_reads_tailed(mirp_ctx* c, const char* reads_path, const char* out_path, const char* tails_path, const char* pg_cl, int32_t v,
                                       int32_t k, int32_t m, int32_t filter_unmapped, const MirpAlignTailOpts* tail, int64_t stats[7], double seconds[7]) {
    if (!c) return -1;
    c->text_pieces = 0;
    const bool on = tail && tail->max_tail != 0;
    if (!reads_path || !out_path || !pg_cl || v < 0 || v > 3 || k < 1 || m < 0) return fail(c, -1, "mirp_align_reads_tailed: bad argument");
    if (on && (!tails_path || tail->max_tail < 1 || tail->max_tail > 8 || tail->min_templated < 12 || tail->min_templated > 1024 || tail->trim < 0 ||
               tail->trim > 1))
        return fail(c, -1, "mirp_align_reads_tailed: bad tail argument (max_tail 0..8, min_templated 12..1024, trim 0..1, a path for the summary)");
    if (!c->a_ready) return fail(c, -1, "mirp_align_reads: no index (mirp_align_index first)");
    HIPCHK(c, hipSetDevice(c->device));
    long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = align_file(c, reads_path, out_path, pg_cl, v, k, m, filter_unmapped, nullptr, on ? tail : nullptr, tails_path, st, sec)) return rc;
    if (stats) for (int i = 0; i < 7; i++) stats[i] = st[i];
    if (seconds) std::memcpy(seconds, sec, 7 * sizeof(double));
    return 0;
}

extern "C" int64_t mirp_align_last_batches(const mirp_ctx* c) { return c ? c->a_batches : -1; }

extern "C" int mirp_set_align_place_capacity(mirp_ctx* c, int64_t items) {
    if (!c) return -1;
    if (items < 0) return fail(c, -1, "mirp_set_align_place_capacity: bad argument");
    c->a_place_cap = items;
    return 0;
}

extern "C" int64_t mirp_align_place_last_realigned(const mirp_ctx* c) { return c ? c->a_place_realigned : -1; }

