// Device side of the known-miRNA annotation (mirp_annotate_scan, mirp_annotate.cpp), with the semantics of DESIGN.md §19.
//
// Sequences: the host packs each as AnPacked (one 64-bit word of 2-bit codes, a 32-bit mask of unknown letters, the length); an_planes_kernel
// turns that, once per sequence, into AnSeq: the two bit planes of the codes (as §14 holds its windows) and n = the positions that hold a known
// letter, 16 bytes.  Queries and known sequences share the format.
//
// Pair (q, k), shift d: q position i lies on k position i + d.  One lane holds one sequence A of the larger side; the other side's sequences B
// arrive one after the other through wave-uniform (scalar) loads, and B is the one that is shifted, by s (B position j on A position j + s; s = -d
// when A is the query, d when A is the known sequence), so the shifts of the three planes and of B's length mask are scalar instructions:
//     diff = ((al ^ bl') | (ah ^ bh') | ~(an & bn')) & av & bv'     mismatching overlap positions (an unknown letter mismatches everything)
//     mm = popc(diff), |offset3| = |La - Lb - s|, |offset5| = |s|, distance = mm + |offset5| + |offset3|
//     rank = distance << 7 | mm << 4 | |d| << 1 | (d > 0)             the order in which shifts are preferred; the minimum over admissible s
// A pair is a hit when some s in -E .. E has |offset3| <= E and mm <= M.  The minimum stays in a register.
//
//   count  an_scan_kernel<1>: hits per query (cnt[q]): the bins of plan_passes (pass_plan.h) and the summary's `hits` column.
//   keys   an_scan_kernel<0>: queries [q0, q1) (at most 2^16, a group) against known [k0, k1), hits whose (distance, mm) bin lies in [blo, bhi]
//          append the key qloc << 35 | distance << 31 | mm << 28 | known << 4 | d + 4 to a buffer of `cap` keys and count them.
//   bins   an_scan_kernel<2>: hits of one query per (distance, mm) bin, for a query whose hits alone exceed `cap`: planned again by these bins.
//   order  mirp_device_sort_u64 on bits 4 .. 51: per query, (distance, mismatches, known) = the output order.
//   cut    an_cut_kernel: -k by the key's rank in its query's run (the runs' starts come from the counts), kept keys compacted in order.
// The lines are written on the host from the kept keys (mirp_annotate.cpp).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"
#include "targets_device.h"
#include "wave_atomic.h"

namespace mirp {

#define AN_GROUP (1 << 16)      // queries per group (the key holds 16 bits of query index)
#define AN_NBIN 128             // (distance, mm) bins: distance << 3 | mm, distance <= 14, mm <= 6

struct AnSeq { unsigned l, h, n; int len; };

__global__ void an_planes_kernel(const AnPacked* __restrict__ in, long long n, AnSeq* __restrict__ out) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const AnPacked p = in[i];
    AnSeq s;
    s.l = tg_even(p.word);
    s.h = tg_even(p.word >> 1);
    s.n = (p.len >= 32 ? 0xffffffffu : (1u << p.len) - 1u) & ~p.unk;
    s.len = p.len;
    out[i] = s;
}

// the preferred admissible shift of lane sequence (al, ah, an, av, La) against B, as a rank; 0xffffffff when no shift is admissible
template <bool LANE_Q>
__device__ __forceinline__ unsigned an_best(unsigned al, unsigned ah, unsigned an, unsigned av, int La, const AnSeq& B, int E, int M) {
    const unsigned bv = B.len >= 32 ? 0xffffffffu : (1u << B.len) - 1u;
    const int delta = La - B.len;
    unsigned best = 0xffffffffu;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int s = -E; s <= E; s++) {
        const unsigned r = (unsigned)(s < 0 ? -s : s);
        const unsigned bl = s < 0 ? B.l >> r : B.l << r, bh = s < 0 ? B.h >> r : B.h << r, bn = s < 0 ? B.n >> r : B.n << r, bs = s < 0 ? bv >> r : bv << r;
        const unsigned diff = ((al ^ bl) | (ah ^ bh) | ~(an & bn)) & av & bs;
        const unsigned mm = (unsigned)__popc(diff);
        const int e3 = delta - s;
        const unsigned o3 = (unsigned)(e3 < 0 ? -e3 : e3);
        const unsigned low = (r << 7) | (r << 1) | (unsigned)((LANE_Q ? -s : s) > 0);          // the shift's share of the rank, wave-uniform
        const unsigned rank = mm * 144u + ((o3 << 7) + low);                                   // (mm + o3 + r) << 7 | mm << 4 | r << 1 | (d > 0) for mm <= 7
        const bool ok = o3 <= (unsigned)E && mm <= (unsigned)M;
        best = min(best, ok ? rank : 0xffffffffu);
    }
    return best;
}

// Lanes: sequences a0 + blockIdx.x * 256 + threadIdx.x < a1 of `lane`; the uniform side: sequences [u0, u1) of `uni`, `chunk` per blockIdx.y.
// LANE_Q: the lanes are the queries.  qbase: the group's first query.  MODE 0: keys[0 .. cap), counter[0] = hits (also past cap); MODE 1:
// cnt[query] += hits; MODE 2: hist[bin] += hits.
template <int MODE, bool LANE_Q>
__global__ __launch_bounds__(256) void an_scan_kernel(const AnSeq* __restrict__ lane, long long a0, long long a1, const AnSeq* __restrict__ uni, long long u0,
                                                      long long u1, long long chunk, int E, int M, unsigned blo, unsigned bspan, long long qbase,
                                                      unsigned long long* __restrict__ keys, unsigned long long cap, unsigned long long* __restrict__ counter,
                                                      unsigned* __restrict__ cnt, unsigned long long* __restrict__ hist) {
    const long long a = a0 + (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned al = 0, ah = 0, an = 0, av = 0;
    int La = 0;                                    // a lane past a1: no shift is admissible (|La - Lb - s| >= 8)
    if (a < a1) {
        const AnSeq A = lane[a];
        al = A.l; ah = A.h; an = A.n; La = A.len;
        av = La >= 32 ? 0xffffffffu : (1u << La) - 1u;
    }
    const long long j0 = u0 + (long long)blockIdx.y * chunk;
    const long long j1 = j0 + chunk < u1 ? j0 + chunk : u1;
    unsigned mine = 0;
    for (long long j = j0; j < j1; j++) {
        const unsigned rank = an_best<LANE_Q>(al, ah, an, av, La, uni[j], E, M);
        const unsigned bin = rank >> 4;
        const bool hit = rank != 0xffffffffu && bin - blo <= bspan;
        if (MODE == 0) {
            if (hit) {
                const unsigned long long i = atomicAdd(counter, 1ull);
                const unsigned long long q = (unsigned long long)((LANE_Q ? a : j) - qbase), k = (unsigned long long)(LANE_Q ? j : a);
                const int s = (int)((rank >> 1) & 7u), d = rank & 1u ? s : -s;
                if (i < cap) keys[i] = (q << 35) | ((unsigned long long)bin << 28) | (k << 4) | (unsigned long long)(d + 4);
            }
        } else if (MODE == 1) {
            if (LANE_Q) mine += hit;
            else {
                const unsigned long long b = __ballot(hit);
                if (b && (threadIdx.x & 63) == 0) atomicAdd(&cnt[j], (unsigned)__popcll(b));
            }
        } else {
            cl_wave_atomic<0>(hist, hit ? (long long)bin : -1ll, 1ull);
        }
    }
    if (MODE == 1 && LANE_Q && mine) atomicAdd(&cnt[a], mine);
}

// sorted keys[0 .. n): key i of query qloc has rank i - run[qloc] in its run and is kept when that is below out[qloc + 1] - out[qloc]
__global__ void an_cut_kernel(const unsigned long long* __restrict__ keys, long long n, const long long* __restrict__ run, const long long* __restrict__ out,
                              unsigned long long* __restrict__ kept) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const long long q = (long long)(key >> 35), r = i - run[q];
        if (r < out[q + 1] - out[q]) kept[out[q] + r] = key;
    }
}

}  // namespace mirp

namespace {

struct AnRun {
    mirp_ctx* c;
    const mirp::AnSeq* d_q;
    const mirp::AnSeq* d_k;
    long long nq, nk, cap, K;
    long long held = 0;                        // keys tg_keys / tg_ktmp hold: min(cap, all hits)
    int E, M;
    const MirpAnSink* sink;
    std::vector<unsigned long long> h_keys;
    long long stats[3] = {0, 0, 0};            // hits, keys kept, passes
    double sec[4] = {0, 0, 0, 0};              // counting scan, key scans, sort + cut, download + write

    // queries [q0, q1) against known [k0, k1); one lane per sequence of the larger side, the other side split over blockIdx.y so that the grid
    // fills the device
    template <int MODE>
    void launch(long long q0, long long q1, long long k0, long long k1, unsigned blo, unsigned bhi, long long qbase) {
        using namespace mirp;
        const bool lane_q = q1 - q0 >= k1 - k0;
        const long long a0 = lane_q ? q0 : k0, a1 = lane_q ? q1 : k1, u0 = lane_q ? k0 : q0, u1 = lane_q ? k1 : q1;
        const long long gx = (a1 - a0 + 255) / 256;
        long long gy = std::max<long long>(1, std::min<long long>({(long long)c->n_cu * 16 / gx, (u1 - u0 + 255) / 256, 65535ll}));
        const long long chunk = (u1 - u0 + gy - 1) / gy;
        gy = (u1 - u0 + chunk - 1) / chunk;
        const dim3 grid((unsigned)gx, (unsigned)gy);
        unsigned long long* keys = (unsigned long long*)c->tg_keys.p;
        unsigned long long* counter = (unsigned long long*)c->tg_small.p;
        unsigned* cnt = (unsigned*)c->an_cnt.p;
        unsigned long long* hist = (unsigned long long*)c->tg_hist.p;
        if (lane_q)
            hipLaunchKernelGGL((an_scan_kernel<MODE, true>), grid, dim3(256), 0, c->stream, d_q, a0, a1, d_k, u0, u1, chunk, E, M, blo, bhi - blo, qbase, keys,
                               (unsigned long long)held, counter, cnt, hist);
        else
            hipLaunchKernelGGL((an_scan_kernel<MODE, false>), grid, dim3(256), 0, c->stream, d_k, a0, a1, d_q, u0, u1, chunk, E, M, blo, bhi - blo, qbase, keys,
                               (unsigned long long)held, counter, cnt, hist);
    }

    // the keys of queries [q0, q1), bins [blo, bhi], known [k0, k1) into tg_keys; -> hits (maybe > cap)
    int scan_keys(long long q0, long long q1, long long k0, long long k1, unsigned blo, unsigned bhi, long long* hits) {
        const double t = mirp::now();
        hipStream_t st = c->stream;
        HIPCHK(c, hipMemsetAsync(c->tg_small.p, 0, 8, st));
        launch<0>(q0, q1, k0, k1, blo, bhi, q0);
        unsigned long long h = 0;
        HIPCHK(c, hipMemcpyAsync(&h, c->tg_small.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        *hits = (long long)h;
        sec[1] += mirp::now() - t;
        return 0;
    }

    // sorts the n <= cap keys of the last scan of the group [q0, q1) and hands the kept ones to the sink.  run / out (q1 - q0 + 1 entries each):
    // the runs' first indices and the kept keys' first indices; null: one query, whose first `keep` keys are kept
    int finish(long long q0, long long q1, long long n, const std::vector<long long>* run, const std::vector<long long>* out, long long keep) {
        using namespace mirp;
        hipStream_t st = c->stream;
        stats[2]++;
        if (n == 0) return 0;
        double t = mirp::now();
        unsigned long long* d_keys = (unsigned long long*)c->tg_keys.p;
        int qbits = 0;
        while ((1ll << qbits) < q1 - q0) qbits++;
        if (int rc = mirp_device_sort_u64(c, d_keys, (unsigned long long*)c->tg_ktmp.p, n, 4, (31 + qbits + 7) / 8 * 8)) return rc;
        const unsigned long long* src = d_keys;
        if (run && out->back() != n) {
            const size_t m = run->size();
            if (c->an_run.ensure(8 * m) || c->an_out.ensure(8 * m) || c->an_kept.ensure(8 * (size_t)std::max<long long>(out->back(), 1)))
                return fail(c, -6, "device allocation failed (annotate: cut)");
            HIPCHK(c, hipMemcpyAsync(c->an_run.p, run->data(), 8 * m, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(c->an_out.p, out->data(), 8 * m, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(an_cut_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 16384)), dim3(256), 0, st, (const unsigned long long*)d_keys, n,
                               (const long long*)c->an_run.p, (const long long*)c->an_out.p, (unsigned long long*)c->an_kept.p);
            src = (const unsigned long long*)c->an_kept.p;
            keep = out->back();
        } else if (run) {
            keep = n;
        }
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        sec[2] += mirp::now() - t;
        t = mirp::now();
        if (keep > 0) {
            if ((long long)h_keys.size() < keep) h_keys.resize((size_t)keep);
            HIPCHK(c, hipMemcpy(h_keys.data(), src, 8 * (size_t)keep, hipMemcpyDeviceToHost));
            if (int rc = (*sink)(q0, h_keys.data(), (size_t)keep)) return rc;
            stats[1] += keep;
        }
        sec[3] += mirp::now() - t;
        return 0;
    }

    // one pass over queries [q0, q1) whose hits (cnt) sum to total <= cap
    int pass(long long q0, long long q1, const unsigned* cnt, long long total) {
        long long got = 0;
        if (int rc = scan_keys(q0, q1, 0, nk, 0, AN_NBIN - 1, &got)) return rc;
        if (got != total) return fail(c, -5, "annotate: a pass found a different number of hits than counted");
        std::vector<long long> run((size_t)(q1 - q0 + 1)), out((size_t)(q1 - q0 + 1));
        run[0] = out[0] = 0;
        for (long long q = q0; q < q1; q++) {
            const long long n = cnt[q];
            run[(size_t)(q - q0 + 1)] = run[(size_t)(q - q0)] + n;
            out[(size_t)(q - q0 + 1)] = out[(size_t)(q - q0)] + (K > 0 ? std::min(n, K) : n);
        }
        return finish(q0, q1, got, &run, &out, 0);
    }

    // one query with more hits than cap: passes of consecutive (distance, mm) bins, one bin over cap by ranges of known indices
    int oversize(long long q, long long total) {
        hipStream_t st = c->stream;
        double t = mirp::now();
        HIPCHK(c, hipMemsetAsync(c->tg_hist.p, 0, 8 * AN_NBIN, st));
        launch<2>(q, q + 1, 0, nk, 0, AN_NBIN - 1, q);
        unsigned long long hist[AN_NBIN];
        HIPCHK(c, hipMemcpyAsync(hist, c->tg_hist.p, sizeof hist, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        sec[0] += mirp::now() - t;
        long long sum = 0, emitted = 0;
        for (int b = 0; b < AN_NBIN; b++) sum += (long long)hist[b];
        if (sum != total) return fail(c, -5, "annotate: the bins of a query hold a different number of hits than counted");
        // the bins are (distance, mm), the positions of a bin over cap are the known indices; -k: the walk ends once the pending
        // pass holds the lines the query still lacks
        const auto left = [&]() { return K > 0 ? K - emitted : (1ll << 62); };
        const auto keep = [&](long long got) {
            const long long n = std::min(got, left());
            emitted += n;
            return n;
        };
        const auto flush = [&](long long ba, long long bb, long long expected) -> int {
            long long got = 0;
            if (int rc = scan_keys(q, q + 1, 0, nk, (unsigned)ba, (unsigned)bb, &got)) return rc;
            if (got != expected) return fail(c, -5, "annotate: a pass found a different number of hits than counted");
            return finish(q, q + 1, got, nullptr, nullptr, keep(got));
        };
        const auto range = [&](long long b, unsigned long long p, unsigned long long p1, long long* got) -> int {
            if (int rc = scan_keys(q, q + 1, (long long)p, (long long)p1, (unsigned)b, (unsigned)b, got)) return rc;
            return *got > cap ? 0 : finish(q, q + 1, *got, nullptr, nullptr, keep(*got));
        };
        const int rc = mirp::plan_passes(AN_NBIN, [&](long long b) { return (long long)hist[b]; }, cap, (unsigned long long)nk, flush, range, 0,
                                         [&](long long pend) { return pend >= left(); });
        return rc == mirp::PLAN_POSITION_OVER_CAP ? fail(c, -5, "annotate: one known sequence holds more hits of one query than a pass") : rc;
    }
};

}  // namespace

int mirp_device_annotate(mirp_ctx* c, const std::vector<AnPacked>& q, const std::vector<AnPacked>& k, int max_offset, int max_mismatches, long long max_lines,
                         std::vector<unsigned>& hits_per_query, const MirpAnSink& sink, long long stats[3], double seconds[5]) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long nq = (long long)q.size(), nk = (long long)k.size();
    for (int i = 0; i < 3; i++) stats[i] = 0;
    for (int i = 0; i < 5; i++) seconds[i] = 0;
    hits_per_query.assign((size_t)nq, 0u);
    if (nq == 0 || nk == 0) return 0;
    const long long cap = c->tg_cap > 0 ? c->tg_cap : (1ll << 26);
    double t = mirp::now();
    if (c->an_pack.ensure(sizeof(AnPacked) * (size_t)std::max(nq, nk)) || c->an_q.ensure(sizeof(AnSeq) * (size_t)nq) || c->an_k.ensure(sizeof(AnSeq) * (size_t)nk) ||
        c->an_cnt.ensure(4 * (size_t)nq) || c->tg_small.ensure(64) || c->tg_hist.ensure(8 * AN_NBIN))
        return fail(c, -6, "device allocation failed (annotate)");
    HIPCHK(c, hipMemcpyAsync(c->an_pack.p, q.data(), sizeof(AnPacked) * (size_t)nq, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(an_planes_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, (const AnPacked*)c->an_pack.p, nq, (AnSeq*)c->an_q.p);
    HIPCHK(c, hipMemcpyAsync(c->an_pack.p, k.data(), sizeof(AnPacked) * (size_t)nk, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(an_planes_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, (const AnPacked*)c->an_pack.p, nk, (AnSeq*)c->an_k.p);
    HIPCHK(c, hipMemsetAsync(c->an_cnt.p, 0, 4 * (size_t)nq, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    seconds[0] = mirp::now() - t;

    AnRun run;
    run.c = c;
    run.d_q = (const AnSeq*)c->an_q.p;
    run.d_k = (const AnSeq*)c->an_k.p;
    run.nq = nq; run.nk = nk; run.cap = cap; run.K = max_lines;
    run.E = max_offset; run.M = max_mismatches;
    run.sink = &sink;
    t = mirp::now();
    run.launch<1>(0, nq, 0, nk, 0, AN_NBIN - 1, 0);
    HIPCHK(c, hipMemcpyAsync(hits_per_query.data(), c->an_cnt.p, 4 * (size_t)nq, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    run.sec[0] += mirp::now() - t;
    const unsigned* cnt = hits_per_query.data();
    long long total = 0;
    for (long long i = 0; i < nq; i++) total += cnt[i];
    run.stats[0] = total;
    if (total > 0) {
        const long long hold = std::min(cap, total);
        if (c->tg_keys.ensure(8 * (size_t)hold) || c->tg_ktmp.ensure(8 * (size_t)hold)) return fail(c, -6, "device allocation failed (annotate: keys)");
        run.held = hold;
    }
    // the bins are the queries, at most AN_GROUP indices to a pass; a query over cap is one position, which oversize() plans by its
    // own bins and finishes
    const auto flush = [&](long long qa, long long qb, long long expected) { return run.pass(qa, qb + 1, cnt, expected); };
    const auto range = [&](long long i, unsigned long long, unsigned long long, long long* got) {
        *got = 0;
        return run.oversize(i, cnt[i]);
    };
    if (int rc = plan_passes(nq, [&](long long i) { return (long long)cnt[i]; }, cap, 1, flush, range, AN_GROUP)) return rc;
    for (int i = 0; i < 3; i++) stats[i] = run.stats[i];
    for (int i = 0; i < 4; i++) seconds[1 + i] = run.sec[i];
    return 0;
}
