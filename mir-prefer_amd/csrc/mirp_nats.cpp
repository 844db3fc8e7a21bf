// C-ABI of the search for natural antisense transcripts (mirp_nats_scan): the transcripts are checked, coded and packed here, both
// senses; nats_kernels.hip makes the k-mer records, joins them into candidates, scans the bands, traces back and selects; the regions, their ops
// and the ops' offsets are handed over as library-owned arrays.  Only counters, candidates, end cells, records and ops leave the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mirp_ctx.h"

namespace {

template <class T>
T* nt_copy_out(const T* src, size_t n) {
    T* p = (T*)std::malloc(sizeof(T) * std::max<size_t>(n, 1));
    if (p && n) std::memcpy(p, src, sizeof(T) * n);
    return p;
}

inline void nt_put(std::vector<unsigned long long>& words, long long at, unsigned long long v) {
    unsigned long long& w = words[(size_t)(at >> 4)];
    const int sh = 4 * (int)(at & 15);
    w = (w & ~(15ull << sh)) | (v << sh);
}

}  // namespace

extern "C" int mirp_set_nats_capacity(mirp_ctx* c, int64_t bytes) {
    if (!c) return -1;
    if (bytes < 0) return fail(c, -1, "mirp_set_nats_capacity: bad argument");
    c->nt_cap = bytes;
    return 0;
}

extern "C" int mirp_nats_last_stats(mirp_ctx* c, int64_t stats[16], double seconds[6]) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_nats_last_stats: bad argument");
    for (int i = 0; i < 16; i++) stats[i] = c->nt_stats[i];
    if (seconds)
        for (int i = 0; i < 6; i++) seconds[i] = c->nt_sec[i];
    return 0;
}

extern "C" int mirp_nats_scan(mirp_ctx* c, const char* blob, const int64_t* off, int32_t n_seqs, const MirpNatsOpts* o, MirpNatsRec** recs, int64_t* n_recs,
                              char** ops, int64_t** ops_off) {
    if (!c) return -1;
    if (n_seqs < 0 || !o || !recs || !n_recs || !ops || !ops_off || (n_seqs > 0 && (!blob || !off))) return fail(c, -1, "mirp_nats_scan: bad argument");
    *recs = nullptr; *n_recs = 0; *ops = nullptr; *ops_off = nullptr;
    for (int i = 0; i < 16; i++) c->nt_stats[i] = 0;          // a refused call leaves no statistics of an earlier one
    for (int i = 0; i < 6; i++) c->nt_sec[i] = 0;
    c->reset_jobs_per_slot(8);
    const bool band_ok = o->band == 16 || o->band == 32 || o->band == 64 || o->band == 128 || o->band == 256;
    if (o->seed < 12 || o->seed > 24 || !band_ok || o->max_occ < 1 || o->max_occ > 10000 || o->min_seeds < 1 || o->match < 1 || o->match > 10 ||
        o->mismatch < 1 || o->mismatch > 10 || o->gap < 1 || o->gap > 50 || o->min_score < 1 || o->min_length < 1 || o->reserved != 0)
        return fail(c, -1, "mirp_nats_scan: bad options");
    if (n_seqs > (1 << 25)) return fail(c, -10, "mirp_nats_scan: more than 2^25 transcripts");
    unsigned char code[256];
    std::memset(code, 4, sizeof code);
    const char* in = "AaCcGgTtUu";
    const unsigned char cd[] = {0, 0, 1, 1, 2, 2, 3, 3, 3, 3};
    for (int k = 0; k < 10; k++) code[(unsigned char)in[k]] = cd[k];
    // every kept transcript starts at a multiple of 16 nibbles, with MIRP_NATS_GAP padding nibbles before the first and after every one
    NtSeqs T;
    T.len.assign((size_t)n_seqs, 0);
    T.pos.assign((size_t)n_seqs, 0);
    long long at = MIRP_NATS_GAP, bases = 0, skipped = 0;
    for (int s = 0; s < n_seqs; s++) {
        const long long L = off[s + 1] - off[s];
        if (L < 0) return fail(c, -1, "mirp_nats_scan: bad offsets");
        const unsigned char* src = (const unsigned char*)blob + off[s];
        for (long long p = 0; p < L; p++)
            if (src[p] >= 0x80) {
                char msg[128];
                std::snprintf(msg, sizeof msg, "mirp_nats_scan: transcript %d: a byte >= 0x80", s + 1);
                return fail(c, -10, msg);
            }
        if (L == 0 || L > MIRP_NATS_MAX_LEN) { skipped++; continue; }
        T.len[(size_t)s] = (int)L;
        T.pos[(size_t)s] = at;
        at += (L + 15) / 16 * 16 + MIRP_NATS_GAP;
        bases += L;
    }
    c->nt_stats[0] = n_seqs;
    c->nt_stats[1] = skipped;
    c->nt_stats[2] = bases;
    if (bases == 0) return 0;
    const size_t n_words = (size_t)(at / 16);
    T.fwd.assign(n_words, 0x4444444444444444ull);
    T.rc.assign(n_words, 0x5555555555555555ull);
    T.wseq.assign(n_words, -1);
    for (int s = 0; s < n_seqs; s++) {
        const long long L = T.len[(size_t)s], first = T.pos[(size_t)s];
        if (L == 0) continue;
        const unsigned char* src = (const unsigned char*)blob + off[s];
        for (long long w = first / 16; w < (first + L + 15) / 16; w++) T.wseq[(size_t)w] = s;
        for (long long p = 0; p < L; p++) {
            const unsigned long long v = code[src[p]];
            if (v == 4) continue;          // (an unknown letter keeps the padding's code in either array)
            nt_put(T.fwd, first + p, v);
            nt_put(T.rc, first + (L - 1 - p), 3 - v);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<MirpNatsRec> r;
    std::vector<char> text;
    std::vector<long long> text_at;
    if (int rc = mirp_device_nats(c, T, *o, r, text, text_at)) return rc;
    if (r.empty()) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "the ops' offsets are handed over as they are");
    MirpNatsRec* out_r = nt_copy_out(r.data(), r.size());
    char* out_t = nt_copy_out(text.data(), text.size());
    int64_t* out_at = (int64_t*)nt_copy_out(text_at.data(), text_at.size());
    if (!out_r || !out_t || !out_at) {
        std::free(out_r); std::free(out_t); std::free(out_at);
        return fail(c, -7, "mirp_nats_scan: host allocation failed");
    }
    *recs = out_r; *n_recs = (int64_t)r.size(); *ops = out_t; *ops_off = out_at;
    return 0;
}
