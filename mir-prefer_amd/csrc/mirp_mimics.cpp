// C-ABI of the endogenous-target-mimic search (mirp_mimic_scan): the miRNA FASTA parse and masks of the target-site search
// (mirp_mirna.h), the seed table, the target packing (shared with mirp_align_index) and the output file on the host; mimic_kernels.hip scans,
// sorts, cuts and writes the lines on the device.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include "mirp_fasta.h"
#include "mirp_mirna.h"

namespace {

const int kSeedKeys = 1 << 14;

// the 14-bit code of miRNA positions 2..8 (position 2 in the low bits, A C G U = 0..3), -1 with an unknown letter among them
int seed_key(const unsigned char* cd) {
    int key = 0;
    for (int i = 2; i <= 8; i++) {
        if (cd[i - 1] > 3) return -1;
        key |= (int)cd[i - 1] << (2 * (i - 2));
    }
    return key;
}

}  // namespace

extern "C" int mirp_mimic_scan(mirp_ctx* c, const char* mirna_path, const char* const* target_paths, int32_t n_targets, const MirpMimicOpts* o,
                               const char* out_path, int64_t stats[8], double seconds[5]) {
    if (!c) return -1;
    c->text_pieces = 0;
    if (!mirna_path || !target_paths || n_targets < 1 || !o || !out_path) return fail(c, -1, "mirp_mimic_scan: bad argument");
    if (o->max_imperfect < 0 || o->max_imperfect > 6 || o->loop_len < 2 || o->loop_len > 6 || o->max_sites < 0 || (o->both_strands != 0 && o->both_strands != 1))
        return fail(c, -1, "mirp_mimic_scan: bad options");
    HIPCHK(c, hipSetDevice(c->device));
    double sec[5] = {0, 0, 0, 0, 0};
    double t = mirp::now();
    mirp::Mirnas M;
    mirp::PackedFasta ref;
    mirp::OutFile out(out_path);                    // every return before commit() discards: a refused input has no output, not even an old one
    if (int rc = mirp::parse_mirnas(c, mirna_path, M)) return rc;
    if (int rc = mirp::pack_fasta(c, target_paths, n_targets, ref)) return rc;
    const long long n_mi = (long long)M.lens.size();
    // the miRNAs with a usable seed, stably sorted by its key: bucket k = entries [start[k], start[k + 1])
    std::vector<int> key((size_t)n_mi);
    std::vector<unsigned> mid, slot((size_t)n_mi, ~0u), start((size_t)kSeedKeys + 1, 0u);
    for (long long m = 0; m < n_mi; m++) {
        key[(size_t)m] = seed_key(M.codes.data() + 32 * m);
        if (key[(size_t)m] >= 0) { mid.push_back((unsigned)m); start[(size_t)key[(size_t)m] + 1]++; }
    }
    std::stable_sort(mid.begin(), mid.end(), [&](unsigned a, unsigned b) { return key[a] < key[b]; });
    std::partial_sum(start.begin(), start.end(), start.begin());
    std::vector<TgMirna> mi(mid.size());
    for (size_t e = 0; e < mid.size(); e++) {
        const unsigned m = mid[e];
        slot[m] = (unsigned)e;
        mi[e] = mirp::make_mirna(M.codes.data() + 32 * (size_t)m, M.lens[m], false, false);
    }
    ref.pk.resize((size_t)(2 * ((ref.total + 31) / 32 + 2)), 0u);          // whole 64-bit words, two past the last span
    sec[0] = mirp::now() - t;

    auto sink = [&](const char* p, size_t len) -> int { return out.write(p, len) ? 0 : fail(c, -8, std::string("cannot write ") + out_path); };
    const std::string head = "miRNA\ttarget\tstart\tend\tstrand\timperfect\tmismatches\tgu\tmirna_5to3\tpairs\ttarget_3to5\tloop\n";
    int rc = sink(head.data(), head.size());
    long long st4[4] = {0, 0, 0, 0};
    double dsec[4] = {0, 0, 0, 0};
    if (!rc)
        rc = mirp_device_mimic_scan(c, (const unsigned long long*)ref.pk.data(), ref.amb.data(), ref.cst.data(), ref.total, ref.cstart, ref.blob, ref.noff, mi, mid,
                                    slot, start, M.codes, M.lens, M.names, M.noff, *o, sink, st4, dsec);
    if (rc) return rc;
    if (!out.commit()) return fail(c, -8, std::string("cannot write ") + out_path);
    for (int i = 0; i < 4; i++) sec[1 + i] = dsec[i];
    if (stats) {
        stats[0] = n_mi;
        stats[1] = n_mi - (long long)mid.size();
        stats[2] = (long long)ref.names.size();
        stats[3] = ref.total;
        stats[4] = st4[2];
        stats[5] = st4[3];
        stats[6] = st4[0];
        stats[7] = st4[1];
    }
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}
