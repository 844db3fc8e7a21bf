// The chunk plan and the ring layout of the fold overlap (run_chunked in mirp_fold.cpp; DESIGN.md §17, rounds 9 and 10).  Host only: no HIP, no context,
// nothing of the project, so that a CPU test can compile it alone.  A batch of n_work windows is cut into chunks (fold_overlap_plan); the epilogue of
// chunk k runs beside the fill of chunk k + 1, and the archive is a ring of slots that hold one chunk each (fold_overlap_ring).  An empty plan means
// the serial path.
#pragma once
#include <cstddef>
#include <vector>

namespace mirp {

enum { FOLD_SCHEDULE_ORDERED = 0,      // round 9: fills in order on one stream, a dense pass per chunk; every boundary costs a tail of idle CUs
       FOLD_SCHEDULE_TAILFREE = 1 };   // round 10: fills of neighbouring chunks on two streams, a boundary costs nothing

constexpr int FOLD_OVERLAP_CHUNKS = 4;          // ordered schedule, automatic: this many equal chunks (more where the slot capacity forces them)
constexpr int FOLD_OVERLAP_MIN_ROUNDS = 8;      // automatic: a batch of fewer rounds of the fill grid than this runs serially
// Tail-free schedule, automatic.  An epilogue at one workgroup per CU, running beside a fill, needs FOLD_OVERLAP_EPI_RATIO of the time its own chunk's
// fill took: 0.69 on the product build (8.90 ms beside a fill, behind a fill of 12.83 ms for the same 5,120 windows; the other chunks of that batch
// gave 0.68 and 0.57).  It has to end before the next fill does or it delays the epilogues behind it, so
// chunk[k + 1] >= ratio * chunk[k].  The plan tapers by FOLD_OVERLAP_TAPER = 0.75: the ratio plus 0.06, half the spread the ratio showed between
// chunks of one batch, for a chunk whose windows are slower to trace back than to fill.  It tapers down to FOLD_OVERLAP_LAST_ROUNDS rounds of the
// fill grid: the last chunk's epilogue has no fill to hide behind, and a chunk of less than two rounds is mostly launch and ramp.
#ifndef MIRP_FOLD_EPI_RATIO_PERMILLE
#define MIRP_FOLD_EPI_RATIO_PERMILLE 690
#endif
#ifndef MIRP_FOLD_TAPER_PERMILLE
#define MIRP_FOLD_TAPER_PERMILLE 750
#endif
#ifndef MIRP_FOLD_LAST_ROUNDS
#define MIRP_FOLD_LAST_ROUNDS 2
#endif
constexpr int FOLD_OVERLAP_EPI_RATIO_PERMILLE = MIRP_FOLD_EPI_RATIO_PERMILLE;
constexpr int FOLD_OVERLAP_TAPER_PERMILLE = MIRP_FOLD_TAPER_PERMILLE;
constexpr int FOLD_OVERLAP_LAST_ROUNDS = MIRP_FOLD_LAST_ROUNDS;
static_assert(FOLD_OVERLAP_TAPER_PERMILLE >= FOLD_OVERLAP_EPI_RATIO_PERMILLE && FOLD_OVERLAP_TAPER_PERMILLE <= 1000, "the taper is the measured ratio plus a margin");

// n_work      windows of the batch
// round       windows of one round of the persistent fill grid (2 per CU)
// cap         windows a slot of the ring holds at most
// request     mirp_set_fold_overlap: -1 automatic, 0 off, N > 0 equal chunks of N windows (at most cap), the remainder last, whatever the batch size
// schedule    FOLD_SCHEDULE_*: only the automatic plan depends on it
// Returns the chunk sizes in order: positive, none above cap, their sum n_work.  Empty: the serial path (off, nothing to fold, an automatic batch
// of fewer than FOLD_OVERLAP_MIN_ROUNDS rounds or one that a single chunk holds).
inline std::vector<int> fold_overlap_plan(long long n_work, long long round, long long cap, long long request, int schedule) {
    std::vector<int> plan;
    if (n_work <= 0 || request == 0 || request < -1) return plan;
    if (round < 1) round = 1;
    if (cap < 1) cap = 1;
    auto equal = [&](long long chunk) {
        for (long long b0 = 0; b0 < n_work; b0 += chunk) plan.push_back((int)(chunk < n_work - b0 ? chunk : n_work - b0));
    };
    if (request > 0) {
        equal(request < cap ? request : cap);
        return plan;
    }
    if (n_work < (long long)FOLD_OVERLAP_MIN_ROUNDS * round) return plan;
    const long long cap_r = cap >= round ? cap / round * round : cap;      // whole rounds per chunk where a slot holds one
    if (schedule == FOLD_SCHEDULE_ORDERED) {
        long long chunk = ((n_work + FOLD_OVERLAP_CHUNKS - 1) / FOLD_OVERLAP_CHUNKS + round - 1) / round * round;
        if (chunk > cap_r) chunk = cap_r;
        equal(chunk);
    } else {
        // built from the end: the last chunk, then each chunk before it as large as the taper and the slot allow, until the batch is covered; the
        // first chunk takes what is left (it is the one chunk that may be smaller than the taper asks: nothing runs beside its fill)
        std::vector<long long> back;
        long long t = FOLD_OVERLAP_LAST_ROUNDS * round < cap_r ? FOLD_OVERLAP_LAST_ROUNDS * round : cap_r, sum = 0;
        while (sum + t < n_work) {
            back.push_back(t);
            sum += t;
            const long long up = t * 1000 / FOLD_OVERLAP_TAPER_PERMILLE;      // rounded down: t >= taper * up; whole rounds do not matter where no grid drains alone
            t = up < cap_r ? up : cap_r;
        }
        back.push_back(n_work - sum);
        for (size_t k = back.size(); k-- > 0;) plan.push_back((int)back[k]);
    }
    if (plan.size() < 2) plan.clear();
    return plan;
}

// The archive of a chunked fold: FOLD_RING_SLOTS slots side by side, chunk k in slot k % FOLD_RING_SLOTS, which it takes over from chunk
// k - FOLD_RING_SLOTS once that chunk's epilogue is done.  A slot is as large as its largest chunk: cap[s] windows from window at[s] of the archive on.
constexpr int FOLD_RING_SLOTS = 3;
struct FoldRing {
    size_t cap[FOLD_RING_SLOTS], at[FOLD_RING_SLOTS + 1];
    size_t windows() const { return at[FOLD_RING_SLOTS]; }      // of the whole ring
};
inline FoldRing fold_overlap_ring(const std::vector<int>& plan) {
    FoldRing r = {};
    for (size_t k = 0; k < plan.size(); k++)
        if ((size_t)plan[k] > r.cap[k % FOLD_RING_SLOTS]) r.cap[k % FOLD_RING_SLOTS] = (size_t)plan[k];
    for (int s = 0; s < FOLD_RING_SLOTS; s++) r.at[s + 1] = r.at[s] + r.cap[s];
    return r;
}

}  // namespace mirp
