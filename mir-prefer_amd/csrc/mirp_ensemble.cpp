// C-ABI of the partition function of whole sequences (mirp_ensemble): the sequences are checked and coded here; their MFEs come
// from mirp_run_fold with one structure line of capacity and the default model, as randfold takes them (the sequences of at most 300 nt at span
// 300 on the LDS-resident kernels, the longer ones at the span of the longest); then the sequences are walked in call order in passes whose table
// slabs fit the capacity (pass_plan.h over slab bytes).  A pass is the inside and outside kernels, the reduction to records and centroid texts and,
// when the pairs are wanted, a count per row, a prefix on the host and the fill of the pair list.  Only records, texts and the pairs at or above
// the cutoff leave the device.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"

namespace {

const int kMaxLen = 3000;                  // randfold's limit: what the pipeline can emit as a precursor
const int kLdsLen = 300;                   // the MFE fold: up to here at span 300 on the LDS-resident kernels
const long long kDefaultCapacity = 1ll << 34;

struct EnCodes {
    unsigned char code[256], letter[256];
    EnCodes() {       // the fold's codes N A C G U = 0..4 and the letters mirp_run_fold reads
        std::memset(code, 0, sizeof code);
        std::memset(letter, 'N', sizeof letter);
        const char* in = "AaCcGgUuTt";
        const unsigned char cd[] = {1, 1, 2, 2, 3, 3, 4, 4, 4, 4};
        for (int k = 0; k < 10; k++) { code[(unsigned char)in[k]] = cd[k]; letter[(unsigned char)in[k]] = (unsigned char)"NACGU"[cd[k]]; }
    }
};
const EnCodes kEn;

// the MFEs of the sequences (letters ACGUN, offsets rel) in call order into h_mfe
int en_mfes(mirp_ctx* c, const std::vector<unsigned char>& letters, const std::vector<long long>& rel, int n_seqs, std::vector<int>& h_mfe) {
    h_mfe.assign((size_t)n_seqs, 0);
    hipStream_t st = c->stream;
    for (int g = 0; g < 2; g++) {
        std::vector<int> idx;
        std::vector<unsigned char> blob;
        std::vector<long long> offs(1, 0);
        int n_max = 0;
        for (int q = 0; q < n_seqs; q++) {
            const int L = (int)(rel[(size_t)q + 1] - rel[(size_t)q]);
            if ((L <= kLdsLen) != (g == 0)) continue;
            idx.push_back(q);
            blob.insert(blob.end(), letters.begin() + rel[(size_t)q], letters.begin() + rel[(size_t)q + 1]);
            offs.push_back((long long)blob.size());
            n_max = std::max(n_max, L);
        }
        const int m = (int)idx.size();
        if (m == 0) continue;
        const int span = g == 0 ? kLdsLen : n_max;
        const int stride = ((n_max + 3 + 7) / 8) * 8;
        if (c->en_seq.ensure(blob.size() + 16) || c->en_soffs.ensure(8 * ((size_t)m + 1)) || c->en_lines.ensure(sizeof(MirpFoldLine) * (size_t)m) ||
            c->en_ss.ensure((size_t)m * stride) || c->en_nlines.ensure(4 * (size_t)m) || c->en_mfe.ensure(4 * (size_t)std::max(m, n_seqs)) ||
            c->en_status.ensure(4 * (size_t)m))
            return fail(c, -6, "mirp_ensemble: device allocation failed (the MFE fold)");
        HIPCHK(c, hipMemcpyAsync(c->en_seq.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->en_soffs.p, offs.data(), 8 * ((size_t)m + 1), hipMemcpyHostToDevice, st));
        if (int rc = mirp_run_fold(c, (const unsigned char*)c->en_seq.p, (const long long*)c->en_soffs.p, nullptr, m, n_max, span, 1, stride,
                                   (MirpFoldLine*)c->en_lines.p, (char*)c->en_ss.p, (int*)c->en_nlines.p, (int*)c->en_mfe.p, (int*)c->en_status.p))
            return rc;
        std::vector<int> mfe((size_t)m), status((size_t)m);
        HIPCHK(c, hipMemcpyAsync(mfe.data(), c->en_mfe.p, 4 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(status.data(), c->en_status.p, 4 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (int k = 0; k < m; k++) {
            if (status[(size_t)k] < 0) return fail(c, -5, "mirp_ensemble: the fold reported status " + std::to_string(status[(size_t)k]) + " for a sequence");
            h_mfe[(size_t)idx[(size_t)k]] = mfe[(size_t)k];
        }
    }
    HIPCHK(c, hipMemcpy(c->en_mfe.p, h_mfe.data(), 4 * (size_t)n_seqs, hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

extern "C" int mirp_set_ensemble_capacity(mirp_ctx* c, int64_t bytes) {
    if (!c) return -1;
    if (bytes < 0) return fail(c, -1, "mirp_set_ensemble_capacity: bad argument");
    c->en_cap = bytes;
    return 0;
}

extern "C" int mirp_ensemble_last_stats(mirp_ctx* c, int64_t stats[3]) {
    if (!c) return -1;
    if (!stats) return fail(c, -1, "mirp_ensemble_last_stats: bad argument");
    for (int i = 0; i < 3; i++) stats[i] = c->en_stats[i];
    return 0;
}

extern "C" int mirp_ensemble(mirp_ctx* c, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpEnsembleOpts* o, MirpEnsembleRec* recs,
                             char* centroids, MirpBpp** bpp, int64_t* n_bpp) {
    if (!c) return -1;
    if (n_seqs < 0 || !o || (n_seqs > 0 && (!seqs || !offsets || !recs || !centroids))) return fail(c, -1, "mirp_ensemble: bad argument");
    const bool want = o->want_bpp != 0;
    if (want && (!bpp || !n_bpp || !(o->bpp_cutoff >= 0.0 && o->bpp_cutoff <= 1.0))) return fail(c, -1, "mirp_ensemble: bad options");
    if (bpp) *bpp = nullptr;
    if (n_bpp) *n_bpp = 0;
    char msg[160];
    const long long base = n_seqs > 0 ? offsets[0] : 0;
    std::vector<long long> rel((size_t)n_seqs + 1, 0);
    for (int q = 0; q < n_seqs; q++) {
        const long long L = offsets[q + 1] - offsets[q];
        const char* why = L <= 0 ? "an empty sequence" : L > kMaxLen ? "a sequence longer than 3,000 nt" : nullptr;
        if (why) {
            std::snprintf(msg, sizeof msg, "mirp_ensemble: record %d: %s", q + 1, why);
            return fail(c, -10, msg);
        }
        rel[(size_t)q + 1] = offsets[q + 1] - base;
    }
    const long long total = rel[(size_t)n_seqs];
    std::vector<unsigned char> letters((size_t)total), codes((size_t)total);
    long long cells = 0;
    for (int q = 0; q < n_seqs; q++) {
        for (long long p = rel[(size_t)q]; p < rel[(size_t)q + 1]; p++) {
            const unsigned char ch = (unsigned char)seqs[base + p];
            if (ch >= 0x80) {
                std::snprintf(msg, sizeof msg, "mirp_ensemble: record %d: a byte >= 0x80", q + 1);
                return fail(c, -10, msg);
            }
            letters[(size_t)p] = kEn.letter[ch];
            codes[(size_t)p] = kEn.code[ch];
        }
        const long long L = rel[(size_t)q + 1] - rel[(size_t)q];
        cells += L * (L - 1) / 2;
    }
    c->en_stats[0] = n_seqs; c->en_stats[1] = 0; c->en_stats[2] = cells;
    if (n_seqs == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;

    // the MFEs, always with the default model
    std::vector<int> h_mfe;
    const int model = c->fold_model;
    c->fold_model = MIRP_FOLD_MODEL_VIENNA_212;
    const int rc_mfe = en_mfes(c, letters, rel, n_seqs, h_mfe);
    c->fold_model = model;
    if (rc_mfe) return rc_mfe;

    if (c->en_codes.ensure((size_t)total + 16) || c->en_recs.ensure(sizeof(MirpEnsembleRec) * (size_t)n_seqs))
        return fail(c, -6, "mirp_ensemble: device allocation failed (sequences)");
    HIPCHK(c, hipMemcpy(c->en_codes.p, codes.data(), (size_t)total, hipMemcpyHostToDevice));

    const long long cap = c->en_cap > 0 ? c->en_cap : kDefaultCapacity;
    auto slab_bytes = [&](long long q) { return (long long)(8 * mirp_ensemble_slab_doubles((int)(rel[(size_t)q + 1] - rel[(size_t)q]))); };
    std::vector<MirpBpp> pairs;
    std::vector<EnJob> jobs;
    std::vector<int> row_cnt;
    std::vector<long long> row_at;
    auto flush = [&](long long first, long long last, long long) -> int {
        const int m = (int)(last - first + 1);
        const long long letters0 = rel[(size_t)first], n_letters = rel[(size_t)last + 1] - letters0;
        jobs.clear();
        std::vector<long long> slab_off((size_t)m + 1, 0);
        for (int k = 0; k < m; k++) slab_off[(size_t)k + 1] = slab_off[(size_t)k] + (long long)mirp_ensemble_slab_doubles((int)(rel[(size_t)(first + k) + 1] - rel[(size_t)(first + k)]));
        int n_ring = 0, max_ring_n = 0;
        for (int ring = 1; ring >= 0; ring--) {
            for (int k = 0; k < m; k++) {
                const long long q = first + k;
                const int L = (int)(rel[(size_t)q + 1] - rel[(size_t)q]);
                if ((L <= MIRP_ENSEMBLE_RING_N) != (ring == 1)) continue;
                if (ring == 1) max_ring_n = std::max(max_ring_n, L);
                jobs.push_back(EnJob{rel[(size_t)q], slab_off[(size_t)k], rel[(size_t)q] - letters0 + k, rel[(size_t)q] - letters0, L, (int)q});
            }
            if (ring == 1) n_ring = (int)jobs.size();
        }
        if (c->en_jobs.ensure(sizeof(EnJob) * (size_t)m) || c->en_slab.ensure(8 * (size_t)slab_off[(size_t)m]) || c->en_texts.ensure((size_t)n_letters + m + 16))
            return fail(c, -6, "mirp_ensemble: device allocation failed (a pass's slabs)");
        HIPCHK(c, hipMemcpyAsync(c->en_jobs.p, jobs.data(), sizeof(EnJob) * (size_t)m, hipMemcpyHostToDevice, st));
        if (int rc = mirp_device_ensemble_fold(c, (const unsigned char*)c->en_codes.p, (const EnJob*)c->en_jobs.p, n_ring, m, max_ring_n, (double*)c->en_slab.p)) return rc;
        if (int rc = mirp_device_ensemble_reduce(c, (const EnJob*)c->en_jobs.p, m, (double*)c->en_slab.p, (const int*)c->en_mfe.p, (MirpEnsembleRec*)c->en_recs.p,
                                                 (char*)c->en_texts.p))
            return rc;
        HIPCHK(c, hipMemcpyAsync(recs + first, (const MirpEnsembleRec*)c->en_recs.p + first, sizeof(MirpEnsembleRec) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(centroids + letters0 + first, c->en_texts.p, (size_t)n_letters + m, hipMemcpyDeviceToHost, st));
        if (want) {
            if (c->en_rowcnt.ensure(4 * (size_t)n_letters) || c->en_rowat.ensure(8 * (size_t)n_letters))
                return fail(c, -6, "mirp_ensemble: device allocation failed (a pass's pair counts)");
            if (int rc = mirp_device_ensemble_bpp(c, (const EnJob*)c->en_jobs.p, m, (const double*)c->en_slab.p, o->bpp_cutoff, (int*)c->en_rowcnt.p, nullptr, nullptr))
                return rc;
            row_cnt.resize((size_t)n_letters);
            row_at.resize((size_t)n_letters);
            HIPCHK(c, hipMemcpyAsync(row_cnt.data(), c->en_rowcnt.p, 4 * (size_t)n_letters, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            long long found = 0;
            for (long long r = 0; r < n_letters; r++) { row_at[(size_t)r] = found; found += row_cnt[(size_t)r]; }
            if (found > 0) {
                if (c->en_bpp.ensure(sizeof(MirpBpp) * (size_t)found)) return fail(c, -6, "mirp_ensemble: device allocation failed (a pass's pairs)");
                HIPCHK(c, hipMemcpyAsync(c->en_rowat.p, row_at.data(), 8 * (size_t)n_letters, hipMemcpyHostToDevice, st));
                if (int rc = mirp_device_ensemble_bpp(c, (const EnJob*)c->en_jobs.p, m, (const double*)c->en_slab.p, o->bpp_cutoff, nullptr,
                                                      (const long long*)c->en_rowat.p, (MirpBpp*)c->en_bpp.p))
                    return rc;
                const size_t at = pairs.size();
                pairs.resize(at + (size_t)found);
                HIPCHK(c, hipMemcpyAsync(pairs.data() + at, c->en_bpp.p, sizeof(MirpBpp) * (size_t)found, hipMemcpyDeviceToHost, st));
            }
        }
        HIPCHK(c, hipStreamSynchronize(st));
        c->en_stats[1]++;
        return 0;
    };
    // a sequence whose slab alone exceeds the capacity counts as one that just fits: it gets a pass of its own
    auto count = [&](long long q) { return std::min(slab_bytes(q), cap); };
    auto range = [&](long long, unsigned long long, unsigned long long, long long*) -> int { return fail(c, -5, "mirp_ensemble: pass plan"); };
    if (int rc = mirp::plan_passes(n_seqs, count, cap, 1, flush, range)) return rc;
    if (want && !pairs.empty()) {
        MirpBpp* out = (MirpBpp*)std::malloc(sizeof(MirpBpp) * pairs.size());
        if (!out) return fail(c, -7, "mirp_ensemble: host allocation failed (pairs)");
        std::memcpy(out, pairs.data(), sizeof(MirpBpp) * pairs.size());
        *bpp = out;
        *n_bpp = (int64_t)pairs.size();
    }
    return 0;
}
