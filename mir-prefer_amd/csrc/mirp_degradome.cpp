// C-ABI of the degradome (PARE) cleavage scan (mirp_degradome_scan): the miRNA FASTA and the transcripts are parsed and packed as
// for mirp_target_scan, the @SQ contigs of the resident alignments are matched to the transcripts, degradome_kernels.hip finds the hits, and the
// lines are written here from the downloaded hit records (a few thousand after the evidence filter; the text needs nothing the host does not hold).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "mirp_fasta.h"
#include "mirp_mirna.h"

namespace {


// pair class of miRNA code mc (0..3 A C G U, 4 unknown) with target base y (0..3 A C G U): 0 Watson-Crick, 1 G:U, 2 mismatch
int pair_class(unsigned mc, unsigned y) {
    if (mc > 3) return 2;
    if (mc + y == 3) return 0;
    return (mc == 2 && y == 3) || (mc == 3 && y == 2) ? 1 : 2;
}

}  // namespace

extern "C" int mirp_degradome_scan(mirp_ctx* c, const char* mirna_path, const char* transcripts_path, const MirpDegradomeOpts* o, const char* out_path,
                                   int64_t stats[15], double seconds[6]) {
    if (!c) return -1;
    if (!mirna_path || !transcripts_path || !o || !out_path || (o->n_contigs > 0 && (!o->contig_names || !o->contig_len)))
        return fail(c, -1, "mirp_degradome_scan: bad argument");
    if (o->max_half_score < 0 || o->max_half_score > 16 || o->max_category < 0 || o->max_category > 4 || o->n_contigs < 0 || !(o->alpha > 0.0) || !(o->alpha <= 1.0))
        return fail(c, -1, "mirp_degradome_scan: bad options");
    HIPCHK(c, hipSetDevice(c->device));
    double sec[6] = {0, 0, 0, 0, 0, 0};
    double t = mirp::now();
    mirp::Mirnas M;
    mirp::PackedFasta ref;
    mirp::OutFile out(out_path);                    // every return before commit() discards: a refused input has no output, not even an old one
    if (int rc = mirp::parse_mirnas(c, mirna_path, M)) return rc;
    if (int rc = mirp::pack_fasta(c, &transcripts_path, 1, ref)) return rc;
    // every @SQ contig is a transcript of the FASTA with the same length
    const int n_f = (int)ref.names.size();
    std::unordered_map<std::string, int> by_name;
    for (int f = 0; f < n_f; f++) by_name.emplace(ref.names[(size_t)f], f);
    std::vector<int> f2s((size_t)n_f, -1);
    std::vector<unsigned long long> sqstart((size_t)o->n_contigs, 0);
    std::vector<long long> sqlen((size_t)o->n_contigs, 0);
    const char* nm = o->contig_names;
    for (int s = 0; s < o->n_contigs; s++) {
        const std::string name(nm);
        nm += name.size() + 1;
        const auto it = by_name.find(name);
        if (it == by_name.end()) return fail(c, -10, "contig " + name + " of the SAM header is not in " + transcripts_path);
        const int f = it->second;
        if (ref.lens[(size_t)f] != o->contig_len[s])
            return fail(c, -10, "contig " + name + " has " + std::to_string(ref.lens[(size_t)f]) + " bases in " + transcripts_path + " but LN:" +
                                    std::to_string((long long)o->contig_len[s]) + " in the SAM header");
        if (f2s[(size_t)f] < 0) f2s[(size_t)f] = s;          // (a name twice in the header: the ingest refuses that)
        sqstart[(size_t)s] = ref.cstart[(size_t)f];
        sqlen[(size_t)s] = ref.lens[(size_t)f];
    }
    const long long n_mi = (long long)M.lens.size();
    const bool cleave = o->cleavage_site != 0;
    std::vector<TgMirna> mi((size_t)n_mi), mia((size_t)n_mi);
    for (long long m = 0; m < n_mi; m++) {
        mi[(size_t)m] = mirp::make_mirna(M.codes.data() + 32 * m, M.lens[(size_t)m], cleave, false);
        mia[(size_t)m] = mirp::make_mirna(M.codes.data() + 32 * m, M.lens[(size_t)m], cleave, true);
    }
    ref.pk.resize((size_t)(2 * ((ref.total + 31) / 32 + 2)), 0u);          // whole 64-bit words, one past the last window
    sec[0] = mirp::now() - t;

    if (!out.open()) return fail(c, -8, std::string("cannot write ") + out_path);
    std::string text = "miRNA\ttarget\tcleavage\tstart\tend\tscore\tcategory\treads\ttranscript_max\tsites\tpvalue\tmismatches\tgu\tmirna_5to3\tpairs\ttarget_3to5\n";
    auto flush = [&]() -> int {
        if (!out.write(text.data(), text.size())) return fail(c, -8, std::string("cannot write ") + out_path);
        text.clear();
        return 0;
    };
    const unsigned* pk = ref.pk.data();
    auto base = [&](unsigned long long q) { return (pk[q >> 4] >> (2 * (q & 15))) & 3u; };
    const char* RNA = "ACGUN";
    const MirpDgSink sink = [&](int mbase, const MirpDgHit* hits, size_t n, const unsigned long long* sites, const double* pval) -> int {
        char num[64];
        for (size_t i = 0; i < n; i++) {
            const unsigned long long key = hits[i].key, g = key & 0xffffffffull;
            const int mloc = (int)(key >> 40), cat = (int)(key >> 37) & 7, half = (int)(key >> 32) & 31;
            const long long m = (long long)mbase + mloc;
            const int L = M.lens[(size_t)m];
            const unsigned char* mc = M.codes.data() + 32 * m;
            int a = 0, z = n_f;                 // transcript: last cstart <= g
            while (z - a > 1) { const int md = (a + z) >> 1; if (ref.cstart[(size_t)md] <= g) a = md; else z = md; }
            const long long p = (long long)(g - ref.cstart[(size_t)a]) + 1;
            const unsigned long long g1 = g + 9;            // the base paired with miRNA position 1; position i pairs with g1 - (i - 1)
            int nmm = 0, ngu = 0;
            for (int i = 1; i <= L; i++) {
                const int k = pair_class(mc[i - 1], base(g1 - (unsigned)(i - 1)));
                nmm += k == 2;
                ngu += k == 1;
            }
            text.append(M.names, (size_t)M.noff[(size_t)m], (size_t)(M.noff[(size_t)m + 1] - M.noff[(size_t)m]));
            text += '\t';
            text += ref.names[(size_t)a];
            std::snprintf(num, sizeof num, "\t%lld\t%lld\t%lld\t%d.%d\t%d\t", p, p + 10 - L, p + 9, half >> 1, half & 1 ? 5 : 0, cat);
            text += num;
            std::snprintf(num, sizeof num, "%llu\t%llu\t%llu\t", hits[i].reads, hits[i].tmax, sites[(size_t)mloc * 17 + half]);
            text += num;
            std::snprintf(num, sizeof num, "%.3e\t%d\t%d\t", pval[((size_t)mloc * 5 + cat) * 17 + half], nmm, ngu);
            text += num;
            for (int i = 0; i < L; i++) text += RNA[mc[i]];
            text += '\t';
            for (int i = 1; i <= L; i++) {
                const int k = pair_class(mc[i - 1], base(g1 - (unsigned)(i - 1)));
                text += k == 0 ? '|' : k == 1 ? 'o' : 'x';
            }
            text += '\t';
            for (int i = 1; i <= L; i++) text += RNA[base(g1 - (unsigned)(i - 1))];
            text += '\n';
            if (text.size() > (1u << 22))
                if (int rc = flush()) return rc;
        }
        return 0;
    };
    long long st2[12];
    double dsec[6];
    int rc = mirp_device_degradome(c, (const unsigned long long*)ref.pk.data(), ref.amb.data(), ref.cst.data(), ref.total, ref.cstart, f2s, sqstart, sqlen, mi, mia,
                                   o->max_half_score, o->max_category, o->alpha, sink, st2, dsec);
    if (!rc) rc = flush();
    if (rc) return rc;
    if (!out.commit()) return fail(c, -8, std::string("cannot write ") + out_path);
    for (int i = 0; i < 5; i++) sec[1 + i] = dsec[i];
    if (stats) {
        stats[0] = n_mi;
        stats[1] = n_f;
        stats[2] = ref.total;
        for (int i = 0; i < 12; i++) stats[3 + i] = st2[i];
    }
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}
