// The plan of the key passes of a scan whose keys go through a buffer of bounded capacity (targets, degradome, annotate).  Host
// only: no HIP, no context.  The caller has counted the hits of every bin, the bins being numbered in output order, and supplies the kernels,
// sorts and sinks as callables; the plan is the walk over the counts and knows nothing about keys.
#pragma once
#include <climits>

namespace mirp {

// what plan_passes returns when one position of one bin alone holds more than `cap` keys: no pass can take them
constexpr int PLAN_POSITION_OVER_CAP = INT_MIN;

struct PlanNoStop { bool operator()(long long) const { return false; } };

// count(i)                          hits of bin i, 0 <= i < n_bins; a bin without hits neither opens nor closes a pass
// flush(first, last, expected)      one pass over the bins first .. last (both with hits), which hold `expected` <= cap hits together
// range(bin, lo, hi, &got)          positions [lo, hi) of [0, span) of one bin that alone exceeds cap: reports the hits found and, when got <= cap,
//                                   has finished them as a pass; on got > cap the plan halves the length (never below 1, never growing back) and asks again
// group_limit                       > 0: a pass ends before a bin whose index is that far from the pass's first
// stop(pending)                     true ends the walk; asked before every bin with hits, after a flush and before every range (pending = 0 there)
// Consecutive bins are packed into one pass while their hits stay at or below cap; the pending pass is flushed before a bin that would exceed it
// (a bin that alone exceeds it included) and once at the end.  A nonzero return of a callable ends the walk and is returned.
template <class Count, class Flush, class Range, class Stop = PlanNoStop>
int plan_passes(long long n_bins, Count count, long long cap, unsigned long long span, Flush flush, Range range, long long group_limit = 0,
                Stop stop = Stop()) {
    long long first = -1, last = -1, pend = 0;
    auto flush_pending = [&]() -> int {
        if (first < 0) return 0;
        const long long a = first, n = pend;
        first = -1;
        pend = 0;
        return flush(a, last, n);
    };
    for (long long i = 0; i < n_bins; i++) {
        const long long cnt = count(i);
        if (cnt == 0) continue;
        if (stop(pend)) break;
        if (pend + cnt > cap || (group_limit > 0 && first >= 0 && i - first >= group_limit))
            if (int rc = flush_pending()) return rc;
        if (stop(pend)) break;
        if (cnt <= cap) {
            if (first < 0) first = i;
            last = i;
            pend += cnt;
            continue;
        }
        unsigned long long len = span;
        for (unsigned long long p = 0; p < span && !stop(pend);) {
            const unsigned long long p1 = len < span - p ? p + len : span;
            long long got = 0;
            if (int rc = range(i, p, p1, &got)) return rc;
            if (got <= cap) { p = p1; continue; }
            if (p1 - p == 1) return PLAN_POSITION_OVER_CAP;
            len = len / 2 > 1 ? len / 2 : 1;
        }
    }
    return flush_pending();
}

}  // namespace mirp
