// C-ABI of the two-strand fold (mirp_duplex_batch): the strands are checked and coded here and walked in passes of at most
// `capacity` pairs; a pass uploads its coded strands and offsets, duplex_kernels.hip folds them (one wave per pair) and the energy and the two
// masks of paired positions per pair come back, from which the records and the structure texts are written on the host.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"

namespace {

const long long kDefaultCapacity = 1ll << 20;
const int kMaxLen = 64;

struct DxCodes {
    unsigned char t[256];
    DxCodes() {       // the fold's codes: N A C G U = 0..4
        std::memset(t, 0, sizeof t);
        t['A'] = t['a'] = 1; t['C'] = t['c'] = 2; t['G'] = t['g'] = 3; t['U'] = t['u'] = t['T'] = t['t'] = 4;
    }
};
const DxCodes kDx;

inline int lowest(unsigned long long m) { return __builtin_ctzll(m) + 1; }
inline int highest(unsigned long long m) { return 64 - __builtin_clzll(m); }

}  // namespace

extern "C" int mirp_set_duplex_capacity(mirp_ctx* c, int64_t pairs) {
    if (!c) return -1;
    if (pairs < 0) return fail(c, -1, "mirp_set_duplex_capacity: bad argument");
    c->dx_cap = pairs;
    return 0;
}

extern "C" int mirp_duplex_last_stats(mirp_ctx* c, int64_t stats[3]) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_duplex_last_stats: bad argument");
    for (int i = 0; i < 3; i++) stats[i] = c->dx_stats[i];
    return 0;
}

extern "C" int mirp_duplex_batch(mirp_ctx* c, const char* a_blob, const int64_t* a_off, const char* b_blob, const int64_t* b_off, int32_t n, MirpDuplexRec* recs,
                                 char* structures) {
    if (!c) return -1;
    c->reset_jobs_per_slot(0);
    if (n < 0 || (n > 0 && (!a_blob || !a_off || !b_blob || !b_off || !recs))) return fail(c, -1, "mirp_duplex_batch: bad argument");
    char msg[160];
    for (int q = 0; q < n; q++)
        for (int s = 0; s < 2; s++) {
            const long long L = s ? b_off[q + 1] - b_off[q] : a_off[q + 1] - a_off[q];
            if (L < 1 || L > kMaxLen) {
                std::snprintf(msg, sizeof msg, "mirp_duplex_batch: pair %d: strand %c has %lld nt (1..64 allowed)", q + 1, s ? 'b' : 'a', L);
                return fail(c, -10, msg);
            }
        }
    c->dx_stats[0] = n; c->dx_stats[1] = 0; c->dx_stats[2] = 0;
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const long long cap = std::min<long long>(c->dx_cap > 0 ? c->dx_cap : kDefaultCapacity, 1ll << 24);
    if (c->dx_small.ensure(16)) return fail(c, -6, "mirp_duplex_batch: device allocation failed");
    HIPCHK(c, hipMemsetAsync(c->dx_small.p, 0, 8, st));
    std::vector<unsigned char> ha, hb;
    std::vector<long long> hao, hbo;
    std::vector<int> mfe;
    std::vector<unsigned long long> ma, mb;
    long long text_at = 0;
    for (long long q0 = 0; q0 < n; q0 += cap) {
        const long long m = std::min<long long>(cap, n - q0);
        const long long na = a_off[q0 + m] - a_off[q0], nb = b_off[q0 + m] - b_off[q0];
        ha.resize((size_t)na); hb.resize((size_t)nb); hao.resize((size_t)m + 1); hbo.resize((size_t)m + 1);
        int max_la = 1, max_lb = 1;
        for (long long q = 0; q <= m; q++) { hao[(size_t)q] = a_off[q0 + q] - a_off[q0]; hbo[(size_t)q] = b_off[q0 + q] - b_off[q0]; }
        for (long long q = 0; q < m; q++) {
            max_la = std::max(max_la, (int)(hao[(size_t)q + 1] - hao[(size_t)q]));
            max_lb = std::max(max_lb, (int)(hbo[(size_t)q + 1] - hbo[(size_t)q]));
        }
        for (long long p = 0; p < na; p++) ha[(size_t)p] = kDx.t[(unsigned char)a_blob[a_off[q0] + p]];
        for (long long p = 0; p < nb; p++) hb[(size_t)p] = kDx.t[(unsigned char)b_blob[b_off[q0] + p]];
        if (c->dx_a.ensure((size_t)na + 16) || c->dx_b.ensure((size_t)nb + 16) || c->dx_aoff.ensure(8 * ((size_t)m + 1)) || c->dx_boff.ensure(8 * ((size_t)m + 1)) ||
            c->dx_mfe.ensure(4 * (size_t)m) || c->dx_ma.ensure(8 * (size_t)m) || c->dx_mb.ensure(8 * (size_t)m))
            return fail(c, -6, "mirp_duplex_batch: device allocation failed (a pass)");
        HIPCHK(c, hipMemcpyAsync(c->dx_a.p, ha.data(), (size_t)na, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->dx_b.p, hb.data(), (size_t)nb, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->dx_aoff.p, hao.data(), 8 * ((size_t)m + 1), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->dx_boff.p, hbo.data(), 8 * ((size_t)m + 1), hipMemcpyHostToDevice, st));
        if (int rc = mirp_device_duplex_pairs(c, (const unsigned char*)c->dx_a.p, (const long long*)c->dx_aoff.p, (const unsigned char*)c->dx_b.p,
                                              (const long long*)c->dx_boff.p, m, max_la, max_lb, (int*)c->dx_mfe.p, (unsigned long long*)c->dx_ma.p,
                                              (unsigned long long*)c->dx_mb.p, (unsigned long long*)c->dx_small.p))
            return rc;
        mfe.resize((size_t)m); ma.resize((size_t)m); mb.resize((size_t)m);
        HIPCHK(c, hipMemcpyAsync(mfe.data(), c->dx_mfe.p, 4 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(ma.data(), c->dx_ma.p, 8 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(mb.data(), c->dx_mb.p, 8 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (long long q = 0; q < m; q++) {
            const unsigned long long x = ma[(size_t)q], y = mb[(size_t)q];
            MirpDuplexRec& r = recs[q0 + q];
            r.mfe = mfe[(size_t)q];
            r.pairs = __builtin_popcountll(x);
            r.a_first = x ? lowest(x) : 0; r.a_last = x ? highest(x) : 0;
            r.b_first = y ? lowest(y) : 0; r.b_last = y ? highest(y) : 0;
            if (structures) {
                const int la = (int)(hao[(size_t)q + 1] - hao[(size_t)q]), lb = (int)(hbo[(size_t)q + 1] - hbo[(size_t)q]);
                char* t = structures + text_at;
                for (int i = 0; i < la; i++) t[i] = (x >> i) & 1 ? '(' : '.';
                t[la] = '&';
                for (int j = 0; j < lb; j++) t[la + 1 + j] = (y >> j) & 1 ? ')' : '.';
                t[la + 1 + lb] = 0;
                text_at += la + lb + 2;
            }
        }
        c->dx_stats[1]++;
    }
    unsigned long long ev = 0;
    HIPCHK(c, hipMemcpy(&ev, c->dx_small.p, 8, hipMemcpyDeviceToHost));
    c->dx_stats[2] = (long long)ev;
    return 0;
}
