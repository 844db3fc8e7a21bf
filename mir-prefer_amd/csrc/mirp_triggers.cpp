// C-ABI of the miRNA triggers of PHAS loci (mirp_trigger_scan): the argument checks, the miRNA FASTA and its masks (mirp_mirna.h,
// the cleavage rule always on) and the genome packing (mirp_fasta.h) on the host; trigger_kernels.hip finds the sites in the locus intervals and
// runs the phasing test in the windows their cuts anchor.  The caller (triggers.py) computes kmin, maps the contigs and writes the files.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_fasta.h"
#include "mirp_mirna.h"
#include "trigger_device.h"

extern "C" int mirp_trigger_scan(mirp_ctx* c, const char* mirna_path, const char* const* genome_paths, int32_t n_genome, const MirpTriggerLocus* loci,
                                 int64_t n_loci, const MirpTriggerOpts* o, const int32_t* kmin, MirpTrigger** triggers, int64_t* n_triggers,
                                 int64_t* site_counts, int64_t stats[6], double seconds[5]) {
    if (!c) return -1;
    if (!mirna_path || !genome_paths || n_genome < 1 || n_loci < 0 || (n_loci > 0 && (!loci || !site_counts)) || !o || !kmin || !triggers || !n_triggers)
        return fail(c, -1, "mirp_trigger_scan: bad argument");
    for (int32_t i = 0; i < n_genome; i++)
        if (!genome_paths[i]) return fail(c, -1, "mirp_trigger_scan: bad argument");
    if (o->length < 1 || o->length > 1024 || o->cycles < 1 || o->cycles > 64 || o->min_phased < 1 || o->min_depth < 1 || o->max_half_score < 0 ||
        o->max_half_score > 16 || o->drift < 0 || o->drift > 2)
        return fail(c, -1, "mirp_trigger_scan: bad options");
    for (int64_t q = 0; q < n_loci; q++)
        if (loci[q].tid < 0 || loci[q].contig < 0 || loci[q].start < 1 || loci[q].start > loci[q].end)
            return fail(c, -1, "mirp_trigger_scan: bad locus " + std::to_string(q));
    *triggers = nullptr;
    *n_triggers = 0;
    double sec[5] = {0, 0, 0, 0, 0};
    const double t = mirp::now();
    mirp::Mirnas M;
    mirp::PackedFasta ref;
    if (int rc = mirp::parse_mirnas(c, mirna_path, M)) return rc;
    if (int rc = mirp::pack_fasta(c, genome_paths, n_genome, ref)) return rc;
    for (int64_t q = 0; q < n_loci; q++)
        if ((size_t)loci[q].contig >= ref.lens.size() || loci[q].end > ref.lens[(size_t)loci[q].contig])
            return fail(c, -1, "mirp_trigger_scan: bad locus " + std::to_string(q));
    const long long n_mi = (long long)M.lens.size();
    std::vector<TgMirna> mi((size_t)n_mi);
    std::vector<unsigned char> mlen((size_t)n_mi);
    for (long long m = 0; m < n_mi; m++) {
        mi[(size_t)m] = mirp::make_mirna(M.codes.data() + 32 * m, M.lens[(size_t)m], true, false);
        mi[(size_t)m].smin = 0;
        mi[(size_t)m].smax = o->max_half_score;
        mlen[(size_t)m] = (unsigned char)M.lens[(size_t)m];
    }
    ref.pk.resize((size_t)(2 * ((ref.total + 31) / 32 + 2)), 0u);          // whole 64-bit words, one past the last window
    sec[0] = mirp::now() - t;
    HIPCHK(c, hipSetDevice(c->device));
    long long st[6] = {0, 0, 0, 0, 0, 0};
    if (int rc = mirp_device_trigger_scan(c, (const unsigned long long*)ref.pk.data(), ref.amb.data(), ref.cst.data(), ref.total, ref.cstart, mi, mlen, loci,
                                          n_loci, *o, kmin, triggers, n_triggers, site_counts, st, sec + 1))
        return rc;
    if (stats)
        for (int i = 0; i < 6; i++) stats[i] = st[i];
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}
