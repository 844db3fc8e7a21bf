// C-ABI of the gapped local alignment of queries with known sequences (mirp_hairpin_align): both sides are checked and coded
// here, hairpin_kernels.hip scores every pair, orders and cuts the hits and traces the kept ones back; the hits, their ops and the ops' offsets
// are handed over as library-owned arrays.  Only hit records and ops leave the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"

namespace {

const int kMaxLen = 3000;
const long long kMaxKnown = 1ll << 24;

// checks one side and codes it: A C G U/T = 0..3 in either case, anything else `unknown`; every sequence starts at a multiple of `align` and is
// padded to one with `pad`
int hp_code(mirp_ctx* c, const char* side, const char* blob, const int64_t* off, int32_t n, unsigned char unknown, int align, unsigned char pad, HpSeqs& out) {
    unsigned char code[256];
    std::memset(code, unknown, sizeof code);
    const char* in = "AaCcGgUuTt";
    const unsigned char cd[] = {0, 0, 1, 1, 2, 2, 3, 3, 3, 3};
    for (int k = 0; k < 10; k++) code[(unsigned char)in[k]] = cd[k];
    char msg[160];
    out.at.resize((size_t)n);
    out.len.resize((size_t)n);
    long long total = 0;
    for (int q = 0; q < n; q++) {
        const long long L = off[q + 1] - off[q];
        const char* why = L <= 0 ? "an empty sequence" : L > kMaxLen ? "a sequence longer than 3,000 nt" : nullptr;
        if (why) {
            std::snprintf(msg, sizeof msg, "mirp_hairpin_align: %s record %d: %s", side, q + 1, why);
            return fail(c, -10, msg);
        }
        out.at[(size_t)q] = total;
        out.len[(size_t)q] = (int)L;
        total += (L + align - 1) / align * align;
    }
    out.codes.assign((size_t)total, pad);
    for (int q = 0; q < n; q++) {
        unsigned char* dst = out.codes.data() + out.at[(size_t)q];
        for (long long p = 0; p < out.len[(size_t)q]; p++) {
            const unsigned char ch = (unsigned char)blob[off[q] + p];
            if (ch >= 0x80) {
                std::snprintf(msg, sizeof msg, "mirp_hairpin_align: %s record %d: a byte >= 0x80", side, q + 1);
                return fail(c, -10, msg);
            }
            dst[p] = code[ch];
        }
    }
    return 0;
}

template <class T>
T* hp_copy_out(const T* src, size_t n) {
    T* p = (T*)std::malloc(sizeof(T) * std::max<size_t>(n, 1));
    if (p && n) std::memcpy(p, src, sizeof(T) * n);
    return p;
}

}  // namespace

extern "C" int mirp_set_hairpin_capacity(mirp_ctx* c, int64_t bytes) {
    if (!c) return -1;
    if (bytes < 0) return fail(c, -1, "mirp_set_hairpin_capacity: bad argument");
    c->hp_cap = bytes;
    return 0;
}

extern "C" int mirp_hairpin_last_stats(mirp_ctx* c, int64_t stats[8], double seconds[5], int64_t* hits_per_query) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_hairpin_last_stats: bad argument");
    for (int i = 0; i < 8; i++) stats[i] = c->hp_stats[i];
    if (seconds)
        for (int i = 0; i < 5; i++) seconds[i] = c->hp_sec[i];
    if (hits_per_query)          // stats[0] entries
        for (size_t q = 0; q < c->hp_per_query.size() && (long long)q < c->hp_stats[0]; q++) hits_per_query[q] = c->hp_per_query[q];
    return 0;
}

extern "C" int mirp_hairpin_align(mirp_ctx* c, const char* q_blob, const int64_t* q_off, int32_t n_q, const char* k_blob, const int64_t* k_off, int32_t n_k,
                                  const MirpHairpinOpts* o, MirpHairpinHit** hits, int64_t* n_hits, char** ops, int64_t** ops_off) {
    if (!c) return -1;
    c->reset_jobs_per_slot(2);
    if (n_q < 0 || n_k < 0 || !o || !hits || !n_hits || !ops || !ops_off || (n_q > 0 && (!q_blob || !q_off)) || (n_k > 0 && (!k_blob || !k_off)))
        return fail(c, -1, "mirp_hairpin_align: bad argument");
    *hits = nullptr; *n_hits = 0; *ops = nullptr; *ops_off = nullptr;
    c->hp_per_query.clear();          // a refused call leaves no statistics of an earlier one
    for (int i = 0; i < 8; i++) c->hp_stats[i] = 0;
    for (int i = 0; i < 5; i++) c->hp_sec[i] = 0;
    if (o->match < 1 || o->match > 10 || o->mismatch < 1 || o->mismatch > 10 || o->gap_open < 0 || o->gap_open > 20 || o->gap_extend < 1 || o->gap_extend > 10 ||
        o->min_score < 1 || o->max_lines < 0)
        return fail(c, -1, "mirp_hairpin_align: bad options");
    if (n_k > kMaxKnown) return fail(c, -10, "mirp_hairpin_align: more than 16,777,216 known sequences");
    HpSeqs Q, K;
    if (int rc = hp_code(c, "query", q_blob, q_off, n_q, 4, MIRP_HAIRPIN_STRIP, 6, Q)) return rc;
    if (int rc = hp_code(c, "known", k_blob, k_off, n_k, 5, 1, 7, K)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<MirpHairpinHit> h;
    std::vector<char> text;
    std::vector<long long> at;
    if (int rc = mirp_device_hairpin(c, Q, K, *o, h, text, at)) return rc;
    if (h.empty()) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "the ops' offsets are handed over as they are");
    MirpHairpinHit* out_h = hp_copy_out(h.data(), h.size());
    char* out_t = hp_copy_out(text.data(), text.size());
    int64_t* out_at = (int64_t*)hp_copy_out(at.data(), at.size());
    if (!out_h || !out_t || !out_at) {
        std::free(out_h); std::free(out_t); std::free(out_at);
        return fail(c, -7, "mirp_hairpin_align: host allocation failed");
    }
    *hits = out_h; *n_hits = (int64_t)h.size(); *ops = out_t; *ops_off = out_at;
    return 0;
}
