// C-ABI of the shuffle test of precursor MFEs (mirp_randfold, mirp_shuffle_batch): the sequences are checked and coded here, put in
// an order (for the fold: the sequences of at most 300 nt first, which the LDS-resident kernels fold at span 300, then the longer ones, which the
// generic kernels fold at the span of the longest), and walked in passes of at most `capacity` jobs.  A pass is three steps on the device:
// rf_shuffle_kernel writes the pass's sequences and offsets into the buffers mirp_run_fold reads, mirp_run_fold folds them with one structure line
// of capacity (the MFE is written whether or not the lines fit: status 1 is expected), rf_stats_kernel adds the MFEs to the records.  Only the
// records come back.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"

namespace {


const int kMaxLen = 3000;                  // PRECURSOR_LEN's limit in the reference, what the fold path serves
const int kLdsLen = 300;                   // up to here at span 300 on the LDS-resident kernels
const long long kMaxJobs = 1ll << 40;
const long long kDefaultCapacity = 1ll << 18;

struct RfHost {
    int n = 0, n_short = 0;
    long long jps = 1;
    std::vector<int> perm, lens;           // position -> index in the call, its length
    std::vector<long long> cum;            // letters before position i
    RfPlan plan;
    long long jobs() const { return (long long)n * jps; }
    long long row(long long j) const {     // first byte of job j's row in the job space
        if (j >= jobs()) return cum[(size_t)n] * jps;
        const long long qi = j / jps;
        return cum[(size_t)qi] * jps + (j - qi * jps) * lens[(size_t)qi];
    }
};

// checks, codes and uploads the sequences; by_length: the order of the fold (short ones first), else the order of the call
int rf_prepare(mirp_ctx* c, const char* what, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpRandfoldOpts* o, bool by_length, RfHost& H,
               std::vector<MirpRandfoldRec>* recs) {
    char msg[160];
    if (o->n_shuffles < 1 || o->n_shuffles > 100000 || (o->dinucleotide != 0 && o->dinucleotide != 1) || o->capacity < 0)
        return fail(c, -1, std::string(what) + ": bad options");
    if ((long long)n_seqs * ((long long)o->n_shuffles + 1) > kMaxJobs) {
        std::snprintf(msg, sizeof msg, "%s: %d sequences x (%d shuffles + 1) are more than 2^40 folds", what, n_seqs, o->n_shuffles);
        return fail(c, -10, msg);
    }
    H.n = n_seqs;
    const long long base = n_seqs > 0 ? offsets[0] : 0;
    const long long total = n_seqs > 0 ? offsets[n_seqs] - base : 0;
    std::vector<long long> rel((size_t)n_seqs + 1, 0);
    for (int q = 0; q < n_seqs; q++) {
        const long long L = offsets[q + 1] - offsets[q];
        const char* why = L <= 0 ? "an empty sequence" : L > kMaxLen ? "a sequence longer than 3,000 nt" : nullptr;
        if (why) {
            std::snprintf(msg, sizeof msg, "%s: record %d: %s", what, q + 1, why);
            return fail(c, -10, msg);
        }
        rel[(size_t)q + 1] = offsets[q + 1] - base;
    }
    static const struct Table {
        unsigned char t[256];
        Table() {
            std::memset(t, 4, sizeof t);
            t['A'] = t['a'] = 0; t['C'] = t['c'] = 1; t['G'] = t['g'] = 2; t['U'] = t['u'] = t['T'] = t['t'] = 3;
        }
    } code;
    std::vector<unsigned char> codes((size_t)total + 1);
    if (recs) recs->assign((size_t)n_seqs, MirpRandfoldRec{0, 0, 0, 0, INT_MAX, 0, 0, 0});
    for (int q = 0; q < n_seqs; q++) {
        int gc = 0;
        for (long long p = rel[(size_t)q]; p < rel[(size_t)q + 1]; p++) {
            const unsigned char ch = (unsigned char)seqs[base + p];
            if (ch >= 0x80) {
                std::snprintf(msg, sizeof msg, "%s: record %d: a byte >= 0x80", what, q + 1);
                return fail(c, -10, msg);
            }
            const unsigned char cd = code.t[ch];
            codes[(size_t)p] = cd;
            gc += cd == 1 || cd == 2;
        }
        if (recs) { (*recs)[(size_t)q].len = (int)(rel[(size_t)q + 1] - rel[(size_t)q]); (*recs)[(size_t)q].gc = gc; }
    }
    H.perm.clear();
    for (int pass = 0; pass < (by_length ? 2 : 1); pass++) {
        for (int q = 0; q < n_seqs; q++) {
            const bool is_short = rel[(size_t)q + 1] - rel[(size_t)q] <= kLdsLen;
            if (!by_length || is_short == (pass == 0)) H.perm.push_back(q);
        }
        if (pass == 0) H.n_short = by_length ? (int)H.perm.size() : 0;
    }
    H.lens.resize((size_t)n_seqs);
    H.cum.assign((size_t)n_seqs + 1, 0);
    for (int i = 0; i < n_seqs; i++) {
        H.lens[(size_t)i] = (int)(rel[(size_t)H.perm[(size_t)i] + 1] - rel[(size_t)H.perm[(size_t)i]]);
        H.cum[(size_t)i + 1] = H.cum[(size_t)i] + H.lens[(size_t)i];
    }
    if (n_seqs == 0) return 0;
    hipStream_t st = c->stream;
    if (c->rf_codes.ensure((size_t)total + 16) || c->rf_offs.ensure(8 * ((size_t)n_seqs + 1)) || c->rf_perm.ensure(4 * (size_t)n_seqs) ||
        c->rf_cum.ensure(8 * ((size_t)n_seqs + 1)))
        return fail(c, -6, std::string(what) + ": device allocation failed (sequences)");
    HIPCHK(c, hipMemcpyAsync(c->rf_codes.p, codes.data(), (size_t)total, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->rf_offs.p, rel.data(), 8 * ((size_t)n_seqs + 1), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->rf_perm.p, H.perm.data(), 4 * (size_t)n_seqs, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->rf_cum.p, H.cum.data(), 8 * ((size_t)n_seqs + 1), hipMemcpyHostToDevice, st));
    if (recs) {
        if (c->rf_rec.ensure(sizeof(MirpRandfoldRec) * (size_t)n_seqs) || c->rf_bad.ensure(16)) return fail(c, -6, std::string(what) + ": device allocation failed (records)");
        HIPCHK(c, hipMemcpyAsync(c->rf_rec.p, recs->data(), sizeof(MirpRandfoldRec) * (size_t)n_seqs, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(c->rf_bad.p, 0, 16, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));          // the host vectors go out of scope
    H.plan.d_codes = (const unsigned char*)c->rf_codes.p;
    H.plan.d_offs = (const long long*)c->rf_offs.p;
    H.plan.d_perm = (const int*)c->rf_perm.p;
    H.plan.d_cum = (const long long*)c->rf_cum.p;
    H.plan.seed = o->seed;
    H.plan.dinucleotide = o->dinucleotide;
    return 0;
}

// the buffers of a pass of n jobs and `bytes` letters
int rf_pass_buffers(mirp_ctx* c, const char* what, int n, long long bytes, bool di) {
    if (c->rf_seq.ensure((size_t)bytes + 16) || c->rf_soffs.ensure(8 * ((size_t)n + 1)) || (di && c->rf_slab.ensure((size_t)bytes + 16)))
        return fail(c, -6, std::string(what) + ": device allocation failed (a pass's sequences)");
    return 0;
}

}  // namespace

extern "C" int mirp_randfold(mirp_ctx* c, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpRandfoldOpts* o, MirpRandfoldRec** recs,
                             int64_t stats[4], double seconds[5]) {
    if (!c) return -1;
    if (!seqs || !offsets || n_seqs < 0 || !o || !recs) return fail(c, -1, "mirp_randfold: bad argument");
    *recs = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    double sec[5] = {0, 0, 0, 0, 0};
    long long passes = 0, fallbacks = 0;
    double t = mirp::now();
    RfHost H;
    std::vector<MirpRandfoldRec> h_rec;
    if (int rc = rf_prepare(c, "mirp_randfold", seqs, offsets, n_seqs, o, true, H, &h_rec)) return rc;
    sec[0] = mirp::now() - t;
    H.jps = (long long)o->n_shuffles + 1;
    H.plan.jps = H.jps;
    H.plan.k_first = 0;
    H.plan.has_native = 1;
    const long long cap = std::min<long long>(o->capacity > 0 ? o->capacity : kDefaultCapacity, 1ll << 24);
    hipStream_t st = c->stream;
    for (int g = 0; g < 2 && n_seqs > 0; g++) {
        const int q0 = g == 0 ? 0 : H.n_short, q1 = g == 0 ? H.n_short : H.n;
        if (q0 == q1) continue;
        const int span = g == 0 ? kLdsLen : *std::max_element(H.lens.begin() + q0, H.lens.begin() + q1);
        for (long long j0 = q0 * H.jps; j0 < q1 * H.jps; j0 += cap) {
            const int n = (int)std::min<long long>(cap, q1 * H.jps - j0);
            const long long base = H.row(j0), bytes = H.row(j0 + n) - base;
            const int n_max = *std::max_element(H.lens.begin() + (j0 / H.jps), H.lens.begin() + ((j0 + n - 1) / H.jps) + 1);
            const int stride = ((n_max + 3 + 7) / 8) * 8;
            if (int rc = rf_pass_buffers(c, "mirp_randfold", n, bytes, o->dinucleotide != 0)) return rc;
            if (c->rf_lines.ensure(sizeof(MirpFoldLine) * (size_t)n) || c->rf_ss.ensure((size_t)n * stride) || c->rf_nlines.ensure(4 * (size_t)n) ||
                c->rf_mfe.ensure(4 * (size_t)n) || c->rf_status.ensure(4 * (size_t)n))
                return fail(c, -6, "mirp_randfold: device allocation failed (a pass's fold output)");
            t = mirp::now();
            mirp_device_rf_shuffle(c, H.plan, j0, n, base, (unsigned char*)c->rf_seq.p, (long long*)c->rf_soffs.p, (unsigned char*)c->rf_slab.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(st));
            sec[1] += mirp::now() - t;
            t = mirp::now();
            if (int rc = mirp_run_fold(c, (const unsigned char*)c->rf_seq.p, (const long long*)c->rf_soffs.p, nullptr, n, n_max, span, 1, stride,
                                       (MirpFoldLine*)c->rf_lines.p, (char*)c->rf_ss.p, (int*)c->rf_nlines.p, (int*)c->rf_mfe.p, (int*)c->rf_status.p))
                return rc;
            HIPCHK(c, hipStreamSynchronize(st));
            fallbacks += c->last_fallback;
            sec[2] += mirp::now() - t;
            t = mirp::now();
            mirp_device_rf_stats(c, H.plan, j0, n, (const int*)c->rf_mfe.p, (const int*)c->rf_status.p, (MirpRandfoldRec*)c->rf_rec.p, (int*)c->rf_bad.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(st));
            sec[3] += mirp::now() - t;
            passes++;
        }
    }
    t = mirp::now();
    MirpRandfoldRec* out = (MirpRandfoldRec*)std::calloc(std::max(n_seqs, 1), sizeof(MirpRandfoldRec));
    if (!out) return fail(c, -7, "mirp_randfold: host allocation failed (records)");
    if (n_seqs > 0) {
        int bad = 0;
        if (hipMemcpy(out, c->rf_rec.p, sizeof(MirpRandfoldRec) * (size_t)n_seqs, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(&bad, c->rf_bad.p, 4, hipMemcpyDeviceToHost) != hipSuccess) {
            std::free(out);
            return fail(c, -2, "mirp_randfold: D2H copy failed");
        }
        if (bad < 0) {
            std::free(out);
            return fail(c, -5, "mirp_randfold: the fold reported status " + std::to_string(bad) + " for a sequence");
        }
    }
    sec[4] = mirp::now() - t;
    *recs = out;
    if (stats) { stats[0] = n_seqs; stats[1] = H.jobs(); stats[2] = passes; stats[3] = fallbacks; }
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}

extern "C" int mirp_shuffle_batch(mirp_ctx* c, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpRandfoldOpts* o, int32_t k0, int32_t n_k,
                                  char** out, int64_t* n_bytes) {
    if (!c) return -1;
    if (!seqs || !offsets || n_seqs < 0 || !o || !out || !n_bytes || k0 < 0 || n_k < 1 || (long long)k0 + n_k > 100000)
        return fail(c, -1, "mirp_shuffle_batch: bad argument");
    *out = nullptr;
    *n_bytes = 0;
    HIPCHK(c, hipSetDevice(c->device));
    RfHost H;
    if (int rc = rf_prepare(c, "mirp_shuffle_batch", seqs, offsets, n_seqs, o, false, H, nullptr)) return rc;
    H.jps = n_k;
    H.plan.jps = H.jps;
    H.plan.k_first = k0;
    H.plan.has_native = 0;
    const long long total = H.row(H.jobs());
    char* h = (char*)std::malloc((size_t)std::max<long long>(total, 1));
    if (!h) return fail(c, -7, "mirp_shuffle_batch: host allocation failed");
    auto bail = [&](int rc) { std::free(h); return rc; };
    const long long cap = std::min<long long>(o->capacity > 0 ? o->capacity : kDefaultCapacity, 1ll << 24);
    for (long long j0 = 0; j0 < H.jobs(); j0 += cap) {
        const int n = (int)std::min<long long>(cap, H.jobs() - j0);
        const long long base = H.row(j0), bytes = H.row(j0 + n) - base;
        if (int rc = rf_pass_buffers(c, "mirp_shuffle_batch", n, bytes, o->dinucleotide != 0)) return bail(rc);
        mirp_device_rf_shuffle(c, H.plan, j0, n, base, (unsigned char*)c->rf_seq.p, (long long*)c->rf_soffs.p, (unsigned char*)c->rf_slab.p);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h + base, c->rf_seq.p, (size_t)bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return bail(fail(c, -2, "mirp_shuffle_batch: shuffle kernel or D2H copy failed"));
    }
    *out = h;
    *n_bytes = total;
    return 0;
}
