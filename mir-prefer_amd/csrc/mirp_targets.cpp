// C-ABI of the plant miRNA target-site search (mirp_target_scan): the miRNA FASTA parse and the per-miRNA masks, the target packing
// (shared with mirp_align_index) and the output file on the host; targets_kernels.hip scans, sorts, cuts and writes the lines on the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_fasta.h"
#include "mirp_mirna.h"

namespace {


// miRNA letters: A C G U in either case 0..3, T = U, anything else 4 (unknown)
struct RnaCodes {
    unsigned char t[256];
    RnaCodes() {
        std::memset(t, 4, sizeof t);
        t['A'] = t['a'] = 0; t['C'] = t['c'] = 1; t['G'] = t['g'] = 2; t['U'] = t['u'] = t['T'] = t['t'] = 3;
    }
};
const RnaCodes kRna;

const long long kMaxMirnas = 1ll << 24;

}  // namespace

namespace mirp {

// the miRNA FASTA of §14; refusals name the 1-based record.  skipped: lengths outside 12..32 are dropped and counted, not refused (§19)
int parse_mirnas(mirp_ctx* c, const char* path, Mirnas& M, long long* skipped) {
    std::string buf;
    if (int rc = mirp::read_whole(c, path, buf)) return rc;
    long long rec = 0, len = 0;
    bool open = false;
    auto refuse = [&](const std::string& why) { return fail(c, -10, std::string(path) + ": record " + std::to_string(rec) + ": " + why); };
    auto finish = [&]() -> int {
        if (!open) return 0;
        open = false;
        if ((len < 12 || len > 32) && skipped) {
            M.noff.pop_back();
            M.names.resize((size_t)M.noff.back());
            M.codes.resize(M.codes.size() - 32);
            ++*skipped;
            return 0;
        }
        if (len < 12 || len > 32) return refuse("the sequence has " + std::to_string(len) + " nt (12..32 allowed)");
        M.lens.push_back((int)len);
        return 0;
    };
    auto ascii = [&](const char* a, const char* b) -> int {
        for (const char* q = a; q < b; q++)
            if ((unsigned char)*q >= 0x80) return refuse("a byte >= 0x80");
        return 0;
    };
    int rc = mirp::for_lines(buf, [&](const char* raw, const char* a, const char* b) -> int {
        if (*raw == '>') {
            if (int r = finish()) return r;
            rec++;
            if (rec > kMaxMirnas && !skipped) return refuse("more than 16,777,216 miRNAs");
            const char* h = raw + 1;
            while (h < b && mirp::fa_ws((unsigned char)*h)) h++;
            if (h == b) return refuse("a header without a name");
            if (int r = ascii(h, b)) return r;
            for (const char* q = h; q < b; q++) M.names.push_back(*q == '\t' ? ' ' : *q);
            M.noff.push_back((long long)M.names.size());
            M.codes.resize(M.codes.size() + 32, 4);
            open = true;
            len = 0;
            return 0;
        }
        if (!open) return 0;                 // text before the first header is ignored
        if (int r = ascii(a, b)) return r;
        unsigned char* cd = M.codes.data() + M.codes.size() - 32;
        for (const char* q = a; q < b; q++, len++)
            if (len < 32) cd[len] = kRna.t[(unsigned char)*q];
        return 0;
    });
    if (rc) return rc;
    return finish();
}

// the masks of one miRNA (codes cd[0 .. L), position i = 1 .. L at cd[i - 1]) for both strands; -c sets the cleavage masks.  anchored: the plus
// strand's masks for a window whose last base pairs with miRNA position 1 (position i at j = 32 - i; the degradome scan), s[1] unused
TgMirna make_mirna(const unsigned char* cd, int L, bool cleavage, bool anchored) {
    TgMirna m;
    std::memset(&m, 0, sizeof m);
    m.L = L;
    m.lmask = L == 32 ? 0xffffffffu : (1u << L) - 1u;
    if (anchored) m.lmask <<= 32 - L;
    for (int i = 1; i <= L; i++) {
        const unsigned k = cd[i - 1];
        for (int s = 0; s < 2; s++) {
            TgStrand& S = m.s[s];
            if (anchored && s) continue;
            const int j = anchored ? 32 - i : s ? i - 1 : L - i;      // window position paired with miRNA position i
            const unsigned bit = 1u << j;
            if (k > 3) S.unk |= bit;
            else {
                const unsigned x = s ? k : 3u - k;       // the forward target base of a Watson-Crick pair (A C G T = 0..3)
                if (x & 1) S.pl |= bit;
                if (x & 2) S.ph |= bit;
                if (k == 2) S.g1 |= bit;                 // miRNA G: G:U with target U (forward T on +, A on -)
                if (k == 3) S.g2 |= bit;                 // miRNA U: G:U with target G (forward G on +, C on -)
            }
            if (i >= 2 && i <= 13) S.seed |= bit;
            if (cleavage && (i == 10 || i == 11)) S.cleave |= bit;
        }
    }
    return m;
}

}  // namespace mirp

using mirp::Mirnas;
using mirp::make_mirna;
using mirp::parse_mirnas;

extern "C" int mirp_set_target_capacity(mirp_ctx* c, int64_t keys) {
    if (!c) return -1;
    if (keys < 0 || keys == 1) return fail(c, -1, "mirp_set_target_capacity: bad argument");
    c->tg_cap = keys;
    return 0;
}

extern "C" int mirp_target_scan(mirp_ctx* c, const char* mirna_path, const char* const* target_paths, int32_t n_targets, const MirpTargetOpts* o,
                                const char* out_path, int64_t stats[6], double seconds[5]) {
    if (!c) return -1;
    c->text_pieces = 0;
    c->reset_jobs_per_slot(0);
    c->reset_jobs_per_slot(1);
    if (!mirna_path || !target_paths || n_targets < 1 || !o || !out_path) return fail(c, -1, "mirp_target_scan: bad argument");
    if (o->max_half_score < 0 || o->max_half_score > 16 || o->max_sites < 0 || (o->energy != 0 && o->energy != 1) ||
        (o->accessibility != 0 && o->accessibility != 1))
        return fail(c, -1, "mirp_target_scan: bad options");
    HIPCHK(c, hipSetDevice(c->device));
    double sec[5] = {0, 0, 0, 0, 0};
    double t = mirp::now();
    Mirnas M;
    mirp::PackedFasta ref;
    mirp::OutFile out(out_path);                    // every return before commit() discards: a refused input has no output, not even an old one
    if (int rc = parse_mirnas(c, mirna_path, M)) return rc;
    if (int rc = mirp::pack_fasta(c, target_paths, n_targets, ref)) return rc;
    const long long n_mi = (long long)M.lens.size();
    std::vector<TgMirna> mi((size_t)n_mi);
    for (long long m = 0; m < n_mi; m++) mi[(size_t)m] = make_mirna(M.codes.data() + 32 * m, M.lens[(size_t)m], o->cleavage_site != 0, false);
    ref.pk.resize((size_t)(2 * ((ref.total + 31) / 32 + 2)), 0u);          // whole 64-bit words, one past the last window
    sec[0] = mirp::now() - t;

    auto sink = [&](const char* p, size_t len) -> int { return out.write(p, len) ? 0 : fail(c, -8, std::string("cannot write ") + out_path); };
    const std::string head = std::string("miRNA\ttarget\tstart\tend\tstrand\tscore\tmismatches\tgu\tmirna_5to3\tpairs\ttarget_3to5") + (o->bulge ? "\tbulge" : "") +
                             (o->energy ? "\tmfe\tmfe_perfect\tmfe_ratio\tduplex" : "") + (o->accessibility ? "\tupe\n" : "\n");
    int rc = sink(head.data(), head.size());
    long long st2[2] = {0, 0};
    double dsec[4] = {0, 0, 0, 0};
    if (!rc)
        rc = mirp_device_target_scan(c, (const unsigned long long*)ref.pk.data(), ref.amb.data(), ref.cst.data(), ref.total, ref.cstart, ref.blob, ref.noff, mi,
                                     M.codes, M.names, M.noff, *o, sink, st2, dsec);
    if (rc) return rc;
    if (!out.commit()) return fail(c, -8, std::string("cannot write ") + out_path);
    for (int i = 0; i < 4; i++) sec[1 + i] = dsec[i];
    if (stats) {
        stats[0] = n_mi;
        stats[1] = (long long)ref.names.size();
        stats[2] = ref.total;
        stats[3] = ref.total * n_mi * (o->both_strands ? 2 : 1);
        stats[4] = st2[0];
        stats[5] = st2[1];
    }
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}
