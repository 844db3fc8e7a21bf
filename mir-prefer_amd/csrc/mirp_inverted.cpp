// C-ABI of the inverted-repeat search (mirp_inverted_scan): the contigs are checked, coded and packed here, inverted_kernels.hip
// scans the band, picks the candidates, traces them back and selects; the repeats, their ops and the ops' offsets are handed over as
// library-owned arrays.  Only candidate keys, records and ops leave the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mirp_ctx.h"

namespace {

template <class T>
T* iv_copy_out(const T* src, size_t n) {
    T* p = (T*)std::malloc(sizeof(T) * std::max<size_t>(n, 1));
    if (p && n) std::memcpy(p, src, sizeof(T) * n);
    return p;
}

}  // namespace

extern "C" int mirp_set_inverted_capacity(mirp_ctx* c, int64_t bytes) {
    if (!c) return -1;
    if (bytes < 0) return fail(c, -1, "mirp_set_inverted_capacity: bad argument");
    c->iv_cap = bytes;
    return 0;
}

extern "C" int mirp_inverted_last_stats(mirp_ctx* c, int64_t stats[12], double seconds[5]) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_inverted_last_stats: bad argument");
    for (int i = 0; i < 12; i++) stats[i] = c->iv_stats[i];
    if (seconds)
        for (int i = 0; i < 5; i++) seconds[i] = c->iv_sec[i];
    return 0;
}

extern "C" int mirp_inverted_scan(mirp_ctx* c, const char* blob, const int64_t* off, int32_t n_contigs, const MirpInvertedOpts* o, MirpInvertedRec** recs,
                                  int64_t* n_recs, char** ops, int64_t** ops_off) {
    if (!c) return -1;
    if (n_contigs < 0 || !o || !recs || !n_recs || !ops || !ops_off || (n_contigs > 0 && (!blob || !off)))
        return fail(c, -1, "mirp_inverted_scan: bad argument");
    *recs = nullptr; *n_recs = 0; *ops = nullptr; *ops_off = nullptr;
    for (int i = 0; i < 12; i++) c->iv_stats[i] = 0;          // a refused call leaves no statistics of an earlier one
    for (int i = 0; i < 5; i++) c->iv_sec[i] = 0;
    if (o->max_span < 8 || o->max_span > MIRP_INVERTED_MAX_SPAN || o->min_score < 1 || o->match < 1 || o->match > 10 || o->mismatch < 1 || o->mismatch > 10 ||
        o->gap < 1 || o->gap > 50 || o->reserved != 0)
        return fail(c, -1, "mirp_inverted_scan: bad options");
    unsigned char code[256];
    std::memset(code, 4, sizeof code);
    const char* in = "AaCcGgTtUu";
    const unsigned char cd[] = {0, 0, 1, 1, 2, 2, 3, 3, 3, 3};
    for (int k = 0; k < 10; k++) code[(unsigned char)in[k]] = cd[k];
    // every contig starts at a multiple of 16 rows and is followed by at least one padding row
    IvGenome G;
    G.pstart.resize((size_t)n_contigs + 1);
    G.pend.resize((size_t)n_contigs + 1);
    long long rows = 0, bases = 0;
    for (int k = 0; k < n_contigs; k++) {
        const long long L = off[k + 1] - off[k];
        if (L < 0) return fail(c, -1, "mirp_inverted_scan: bad offsets");
        G.pstart[(size_t)k] = rows;
        G.pend[(size_t)k] = rows + L;
        rows += (L / 16 + 1) * 16;
        bases += L;
    }
    G.pstart[(size_t)n_contigs] = G.pend[(size_t)n_contigs] = rows;
    G.rows = rows;
    // the words past the last row are padding as far as the scan reads: the strip a tile ends in, the band, the block of 16 levels it ends in and
    // the two words the scan loads ahead
    const long long n_words = (rows + MIRP_INVERTED_STRIP + MIRP_INVERTED_MAX_SPAN + 128) / 16;
    G.words.assign((size_t)n_words, 0x4444444444444444ull);
    for (int k = 0; k < n_contigs; k++) {
        const unsigned char* src = (const unsigned char*)blob + off[k];
        const long long L = off[k + 1] - off[k], at = G.pstart[(size_t)k];
        for (long long p = 0; p < L; p++) {
            const unsigned char ch = src[p];
            if (ch >= 0x80) {
                char msg[128];
                std::snprintf(msg, sizeof msg, "mirp_inverted_scan: contig %d: a byte >= 0x80", k + 1);
                return fail(c, -10, msg);
            }
            const unsigned long long v = code[ch];
            if (v != 4) {
                unsigned long long& w = G.words[(size_t)((at + p) >> 4)];
                const int sh = 4 * (int)((at + p) & 15);
                w = (w & ~(15ull << sh)) | (v << sh);
            }
        }
    }
    c->iv_stats[0] = n_contigs;
    c->iv_stats[1] = bases;
    for (int k = 0; k < n_contigs; k++) {          // cells of row i (1-based) of a contig of L bases: min(max_span - 1, L - i)
        const long long L = off[k + 1] - off[k], D1 = o->max_span - 1;
        const long long full = std::max(0ll, L - D1);          // rows with a full band
        const long long rest = L - full;                         // rows i = full + 1 .. L hold L - i = rest - 1 .. 0 cells
        c->iv_stats[2] += full * D1 + rest * (rest - 1) / 2;
    }
    if (rows == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<MirpInvertedRec> r;
    std::vector<char> text;
    std::vector<long long> at;
    if (int rc = mirp_device_inverted(c, G, *o, r, text, at)) return rc;
    if (r.empty()) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "the ops' offsets are handed over as they are");
    MirpInvertedRec* out_r = iv_copy_out(r.data(), r.size());
    char* out_t = iv_copy_out(text.data(), text.size());
    int64_t* out_at = (int64_t*)iv_copy_out(at.data(), at.size());
    if (!out_r || !out_t || !out_at) {
        std::free(out_r); std::free(out_t); std::free(out_at);
        return fail(c, -7, "mirp_inverted_scan: host allocation failed");
    }
    *recs = out_r; *n_recs = (int64_t)r.size(); *ops = out_t; *ops_off = out_at;
    return 0;
}
