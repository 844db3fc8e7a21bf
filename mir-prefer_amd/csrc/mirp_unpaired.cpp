// C-ABI of the accessibility of intervals (mirp_unpaired_batch): the windows are checked and coded here and walked in call order
// in passes of at most `capacity` windows (pass_plan.h, a window a bin).  A pass uploads its codes, offsets and intervals, orders its windows by
// length class, launches unpaired_kernels.hip once per class (so that a 51-nt window does not pay for the slab of a 128-nt one) and brings the
// records back.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"

namespace {

const long long kDefaultCapacity = 1ll << 20;

struct UpCodes {
    unsigned char t[256];
    UpCodes() {       // the fold's codes: N A C G U = 0..4
        std::memset(t, 0, sizeof t);
        t['A'] = t['a'] = 1; t['C'] = t['c'] = 2; t['G'] = t['g'] = 3; t['U'] = t['u'] = t['T'] = t['t'] = 4;
    }
};
const UpCodes kUp;

}  // namespace

extern "C" int mirp_set_unpaired_capacity(mirp_ctx* c, int64_t windows) {
    if (!c) return -1;
    if (windows < 0) return fail(c, -1, "mirp_set_unpaired_capacity: bad argument");
    c->up_cap = windows;
    return 0;
}

extern "C" int mirp_unpaired_last_stats(mirp_ctx* c, int64_t stats[3]) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_unpaired_last_stats: bad argument");
    for (int i = 0; i < 3; i++) stats[i] = c->up_stats[i];
    return 0;
}

extern "C" int mirp_set_target_flanks(mirp_ctx* c, int32_t up, int32_t down) {
    if (!c) return -1;
    if (up < 0 || down < 0 || (long long)up + down > 95) return fail(c, -1, "mirp_set_target_flanks: flanks are >= 0 and at most 95 together");
    c->tg_up = up;
    c->tg_down = down;
    return 0;
}

extern "C" int mirp_unpaired_batch(mirp_ctx* c, const char* blob, const int64_t* off, const int32_t* lo, const int32_t* hi, int32_t n, MirpUnpairedRec* recs) {
    if (!c) return -1;
    c->reset_jobs_per_slot(1);
    if (n < 0 || (n > 0 && (!blob || !off || !lo || !hi || !recs))) return fail(c, -1, "mirp_unpaired_batch: bad argument");
    char msg[160];
    long long cells = 0;
    for (int q = 0; q < n; q++) {
        const long long L = off[q + 1] - off[q];
        const char* why = L <= 0 ? "an empty sequence" : L > MIRP_UNPAIRED_MAX ? "a sequence longer than 128 nt" : nullptr;
        if (!why && !(1 <= lo[q] && lo[q] <= hi[q] && hi[q] <= L)) why = "an interval outside 1 <= lo <= hi <= length";
        for (long long p = off[q]; !why && p < off[q + 1]; p++)
            if ((unsigned char)blob[p] >= 0x80) why = "a byte >= 0x80";
        if (why) {
            std::snprintf(msg, sizeof msg, "mirp_unpaired_batch: record %d: %s", q + 1, why);
            return fail(c, -10, msg);
        }
        cells += L * (L - 1) / 2;
    }
    c->up_stats[0] = n; c->up_stats[1] = 0; c->up_stats[2] = cells;
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const long long cap = std::min<long long>(c->up_cap > 0 ? c->up_cap : kDefaultCapacity, 1ll << 24);
    std::vector<unsigned char> codes;
    std::vector<long long> offs;
    std::vector<int> order;
    auto flush = [&](long long first, long long last, long long) -> int {
        const long long m = last - first + 1, letters = off[last + 1] - off[first];
        codes.resize((size_t)letters); offs.resize((size_t)m + 1); order.resize((size_t)m);
        for (long long p = 0; p < letters; p++) codes[(size_t)p] = kUp.t[(unsigned char)blob[off[first] + p]];
        for (long long q = 0; q <= m; q++) offs[(size_t)q] = off[first + q] - off[first];
        for (long long q = 0; q < m; q++) order[(size_t)q] = (int)q;
        auto cls = [&](int q) { return mirp_unpaired_class((int)(offs[(size_t)q + 1] - offs[(size_t)q])); };
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cls(a) < cls(b); });
        if (c->up_codes.ensure((size_t)letters + 16) || c->up_offs.ensure(8 * ((size_t)m + 1)) || c->up_lo.ensure(4 * (size_t)m) || c->up_hi.ensure(4 * (size_t)m) ||
            c->up_order.ensure(4 * (size_t)m) || c->up_recs.ensure(sizeof(MirpUnpairedRec) * (size_t)m))
            return fail(c, -6, "mirp_unpaired_batch: device allocation failed (a pass)");
        HIPCHK(c, hipMemcpyAsync(c->up_codes.p, codes.data(), (size_t)letters, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->up_offs.p, offs.data(), 8 * ((size_t)m + 1), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->up_lo.p, lo + first, 4 * (size_t)m, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->up_hi.p, hi + first, 4 * (size_t)m, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->up_order.p, order.data(), 4 * (size_t)m, hipMemcpyHostToDevice, st));
        for (long long a = 0; a < m;) {
            const int k = cls(order[(size_t)a]);
            long long b = a;
            while (b < m && cls(order[(size_t)b]) == k) b++;
            if (int rc = mirp_device_unpaired_batch(c, (const unsigned char*)c->up_codes.p, (const long long*)c->up_offs.p, (const int*)c->up_lo.p,
                                                    (const int*)c->up_hi.p, (const int*)c->up_order.p + a, b - a, k, (MirpUnpairedRec*)c->up_recs.p))
                return rc;
            a = b;
        }
        HIPCHK(c, hipMemcpyAsync(recs + first, c->up_recs.p, sizeof(MirpUnpairedRec) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->up_stats[1]++;
        return 0;
    };
    auto count = [](long long) { return 1ll; };
    auto range = [&](long long, unsigned long long, unsigned long long, long long*) -> int { return fail(c, -5, "mirp_unpaired_batch: pass plan"); };
    return mirp::plan_passes(n, count, cap, 1, flush, range);
}
