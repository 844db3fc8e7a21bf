"""CPU tests of the pass planner (mir-prefer_amd/csrc/pass_plan.h): a small driver that includes the header and nothing else of the
project is compiled with the host C++ compiler and prints one line per call of its callables.  The printed sequences are compared with a Python
restatement of the four loops the planner replaced (the target search's, the degradome scan's and the two of the annotation, as they stood
before it) and with sequences worked out by hand.

A scenario is cap, span, the group limit (0: none), the budget K (0: none), the call that fails (0: none) and, for every bin, the positions of its
keys.  The driver's count of a bin is the number of its positions, a range query answers with the positions in [lo, hi), a pass or a finished
range keeps min(hits, K - kept so far) lines, and the walk stops when the pending pass holds what K still lacks.  Lines: `P first last expected`,
`R bin lo hi got` with ` *` when the range was finished (got <= cap), and `E rc` at the end (`E over`: one position over the capacity)."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "pass_plan.h"

int main() {
    long long cap, span, limit, K, fail_at, n;
    while (std::scanf("%lld %lld %lld %lld %lld %lld", &cap, &span, &limit, &K, &fail_at, &n) == 6) {
        std::vector<std::vector<long long>> bins((size_t)n);
        for (auto& b : bins) {
            long long m = 0;
            if (std::scanf("%lld", &m) != 1) return 2;
            b.resize((size_t)m);
            for (auto& x : b)
                if (std::scanf("%lld", &x) != 1) return 2;
        }
        long long calls = 0, kept = 0;
        const auto left = [&]() { return K > 0 ? K - kept : (1ll << 62); };
        const auto keep = [&](long long got) { kept += got < left() ? got : left(); };
        const auto count = [&](long long i) { return (long long)bins[(size_t)i].size(); };
        const auto flush = [&](long long first, long long last, long long expected) -> int {
            std::printf("P %lld %lld %lld\n", first, last, expected);
            if (++calls == fail_at) return 7;
            keep(expected);
            return 0;
        };
        const auto range = [&](long long bin, unsigned long long lo, unsigned long long hi, long long* got) -> int {
            *got = 0;
            for (long long x : bins[(size_t)bin]) *got += (unsigned long long)x >= lo && (unsigned long long)x < hi;
            std::printf("R %lld %llu %llu %lld%s\n", bin, lo, hi, *got, *got <= cap ? " *" : "");
            if (++calls == fail_at) return 7;
            if (*got <= cap) keep(*got);
            return 0;
        };
        const int rc = limit == 0 && K == 0 ? mirp::plan_passes(n, count, cap, (unsigned long long)span, flush, range)
                                            : mirp::plan_passes(n, count, cap, (unsigned long long)span, flush, range, limit,
                                                                [&](long long pend) { return pend >= left(); });
        if (rc == mirp::PLAN_POSITION_OVER_CAP) std::printf("E over\n");
        else std::printf("E %d\n", rc);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pass_plan")
    (d / "driver.cpp").write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "mir-prefer_amd", "csrc"), str(d / "driver.cpp"), "-o", str(d / "driver")])

    def run(scenarios):
        """scenarios: (cap, span, limit, K, fail_at, bins) each -> the printed lines of each"""
        text = "".join("%d %d %d %d %d %d\n" % (cap, span, limit, K, fail_at, len(bins)) + "".join(" ".join(map(str, [len(b)] + list(b))) + "\n" for b in bins)
                       for cap, span, limit, K, fail_at, bins in scenarios)
        out = subprocess.run([str(d / "driver")], input=text.encode(), capture_output=True, timeout=60, check=True).stdout.decode().split("\n")[:-1]
        res, cur = [], []
        for ln in out:
            cur.append(ln)
            if ln.startswith("E "):
                res.append(cur)
                cur = []
        assert not cur and len(res) == len(scenarios)
        return res
    return run


# ------------------------------------------------------------------------------------------ the four loops as they stood before the planner
class Failed(Exception):
    pass


class OnePosition(Exception):
    """a range of one position still exceeds the capacity: the target search refused it, the other loops did not end"""


class Events(list):
    def __init__(self, fail_at):
        super().__init__()
        self.fail_at = fail_at

    def add(self, line):
        self.append(line)
        if len(self) == self.fail_at:
            raise Failed


def _in(pos, lo, hi):
    return sum(1 for x in pos if lo <= x < hi)


def _ranges(ev, i, pos, cap, span, go_on, finished):
    """the position loop shared by three of the loops, word for word: the length is halved, with a floor of 1, and never grows back"""
    length, p = span, 0
    while p < span and go_on():
        p1 = min(span, p + length)
        got = _in(pos, p, p1)
        ev.add("R %d %d %d %d%s" % (i, p, p1, got, " *" if got <= cap else ""))
        if got > cap and p1 - p == 1:
            raise OnePosition
        if got > cap:
            length = max(1, length // 2)
            continue
        finished(got)
        p = p1


def walk_targets(ev, bins, cap, span):
    """TgRun::group (targets_kernels.hip): bins (miRNA, half-score), ranges of offsets"""
    ma = mb = -1
    pend = 0

    def flush():
        nonlocal ma, pend
        if ma < 0:
            return
        a, n = ma, pend
        ma, pend = -1, 0
        ev.add("P %d %d %d" % (a, mb, n))
    for i, pos in enumerate(bins):
        cnt = len(pos)
        if cnt == 0:
            continue
        if pend + cnt > cap:
            flush()
        if cnt <= cap:
            if ma < 0:
                ma = i
            mb = i
            pend += cnt
            continue
        _ranges(ev, i, pos, cap, span, lambda: True, lambda got: None)
    flush()


# the group loop of mirp_device_degradome (degradome_kernels.hip): bins (miRNA, category, half-score) behind the pbins masks, ranges of packed
# positions.  The walk is the target search's; it had no refusal for one position over the capacity and did not end there.
walk_degradome = walk_targets


def walk_annotate_bins(ev, bins, cap, span, K):
    """AnRun::oversize (annotate_kernels.hip): bins (distance, mismatches), ranges of known indices, the -k budget"""
    ba = bb = -1
    pend = kept = 0

    def left():
        return K - kept if K > 0 else 1 << 62

    def keep(got):
        nonlocal kept
        kept += min(got, left())

    def flush():
        nonlocal ba, pend
        if ba < 0:
            return
        a, n = ba, pend
        ba, pend = -1, 0
        ev.add("P %d %d %d" % (a, bb, n))
        keep(n)
    b = 0
    while b < len(bins) and pend < left():
        pos = bins[b]
        b += 1
        n = len(pos)
        if n == 0:
            continue
        if pend + n > cap:
            flush()
        if left() <= 0:
            break
        if n <= cap:
            if ba < 0:
                ba = b - 1
            bb = b - 1
            pend += n
            continue
        _ranges(ev, b - 1, pos, cap, span, lambda: left() > 0, keep)
    flush()


def walk_annotate_queries(ev, bins, cap, limit):
    """the query loop of mirp_device_annotate: bins are queries, a pass spans fewer than `limit` indices, and a query over the capacity goes to
    oversize(), which finishes its hits itself: one range over the single position, which finds none of them"""
    qa = qb = -1
    pend = 0

    def flush():
        nonlocal qa, pend
        if qa < 0:
            return
        a, n = qa, pend
        qa, pend = -1, 0
        ev.add("P %d %d %d" % (a, qb, n))
    for i, pos in enumerate(bins):
        n = len(pos)
        if n == 0:
            continue
        if qa >= 0 and (pend + n > cap or i - qa >= limit):
            flush()
        if n > cap:
            ev.add("R %d 0 1 0 *" % i)
            continue
        if qa < 0:
            qa = i
        qb = i
        pend += n
    flush()


def restate(cap, span, limit, K, fail_at, bins, walk=None):
    ev = Events(fail_at)
    try:
        if walk is not None:
            walk(ev, bins, cap, span)
        elif limit:
            walk_annotate_queries(ev, bins, cap, limit)
        else:
            walk_annotate_bins(ev, bins, cap, span, K)
        return ev + ["E 0"]
    except Failed:
        return ev + ["E 7"]
    except OnePosition:
        return ev + ["E over"]


def _check(driver, scenarios, literal=None):
    got = driver(scenarios)
    for s, g in zip(scenarios, got):
        cap, span, limit, K, fail_at, bins = s
        if limit == 0 and K == 0:
            assert g == restate(*s, walk=walk_targets) == restate(*s, walk=walk_degradome), s
            assert g == restate(*s), s                       # annotate's bins without -k walk the same way
        else:
            assert g == restate(*s), s
    if literal is not None:
        assert got == literal
    return got


def at0(*counts):
    return [[0] * n for n in counts]


# ---------------------------------------------------------------------------------------------------------------------------- the cases
def test_no_bins_and_all_counts_zero(driver):
    _check(driver, [(4, 8, 0, 0, 0, []), (4, 8, 0, 0, 0, at0(0, 0, 0)), (4, 8, 3, 2, 0, at0(0, 0))], [["E 0"]] * 3)


def test_three_bins_of_two_at_capacity_four(driver):
    _check(driver, [(4, 8, 0, 0, 0, at0(2, 2, 2))], [["P 0 1 4", "P 2 2 2", "E 0"]])


def test_a_sum_equal_to_the_capacity_and_one_more(driver):
    _check(driver, [(5, 8, 0, 0, 0, at0(2, 3)), (5, 8, 0, 0, 0, at0(3, 3)), (5, 8, 0, 0, 0, at0(5)), (5, 8, 0, 0, 0, at0(1, 1, 1, 1, 1, 1))],
           [["P 0 1 5", "E 0"], ["P 0 0 3", "P 1 1 3", "E 0"], ["P 0 0 5", "E 0"], ["P 0 4 5", "P 5 5 1", "E 0"]])


def test_an_oversize_bin_is_split_by_halved_ranges(driver):
    _check(driver, [(2, 8, 0, 0, 0, [[3], [0, 1, 7], [5]])],
           [["P 0 0 1", "R 1 0 8 3", "R 1 0 4 2 *", "R 1 4 8 1 *", "P 2 2 1", "E 0"]])


def test_the_length_does_not_grow_back(driver):
    # keys at 0 1 2 | 9: the length falls to 2 on the left and the empty right half is still walked two positions at a time
    _check(driver, [(2, 16, 0, 0, 0, [[0, 1, 2, 9]])],
           [["R 0 0 16 4", "R 0 0 8 3", "R 0 0 4 3", "R 0 0 2 2 *", "R 0 2 4 1 *", "R 0 4 6 0 *", "R 0 6 8 0 *", "R 0 8 10 1 *", "R 0 10 12 0 *",
             "R 0 12 14 0 *", "R 0 14 16 0 *", "E 0"]])


def test_one_position_over_the_capacity_is_an_error(driver):
    got = driver([(2, 8, 0, 0, 0, [[5, 5, 5]]), (2, 8, 0, 5, 0, [[5, 5, 5]])])
    want = ["R 0 0 8 3", "R 0 0 4 0 *", "R 0 4 8 3", "R 0 4 6 3", "R 0 4 5 0 *", "R 0 5 6 3", "E over"]
    assert got == [want, want]
    assert restate(2, 8, 0, 0, 0, [[5, 5, 5]], walk=walk_targets) == want        # the target search refused it in the same place


def test_zero_count_bins_inside_and_at_the_ends(driver):
    _check(driver, [(4, 8, 0, 0, 0, at0(0, 1, 0, 2, 0, 0)), (4, 8, 0, 0, 0, at0(0, 0, 3, 0, 2, 0, 1, 0))],
           [["P 1 3 3", "E 0"], ["P 2 2 3", "P 4 6 3", "E 0"]])


def test_group_limit(driver):
    _check(driver, [(10, 1, 3, 0, 0, at0(1, 0, 0, 1)), (10, 1, 3, 0, 0, at0(1, 0, 1, 1)), (10, 1, 4, 0, 0, at0(1, 0, 0, 1))],
           [["P 0 0 1", "P 3 3 1", "E 0"], ["P 0 2 2", "P 3 3 1", "E 0"], ["P 0 3 2", "E 0"]])


def test_a_query_over_the_capacity_is_handed_over_between_two_passes(driver):
    # its hits stand outside the span of one position: the caller's range callable finishes them itself and reports none
    _check(driver, [(3, 1, 100, 0, 0, [[0], [0], [1, 1, 1, 1], [0]])], [["P 0 1 2", "R 2 0 1 0 *", "P 3 3 1", "E 0"]])


def test_budget(driver):
    _check(driver, [(4, 8, 0, 4, 0, at0(3, 3, 3)), (10, 8, 0, 2, 0, at0(3, 3)), (4, 8, 0, 3, 0, at0(3, 3, 3))],
           [["P 0 0 3", "P 1 1 3", "E 0"], ["P 0 0 3", "E 0"], ["P 0 0 3", "E 0"]])
    # inside an oversize bin: the ranges end when the budget is spent
    _check(driver, [(2, 8, 0, 3, 0, [[0, 1, 2, 3, 4, 5, 6, 7]])], [["R 0 0 8 8", "R 0 0 4 4", "R 0 0 2 2 *", "R 0 2 4 2 *", "E 0"]])


def test_a_failing_callable_stops_the_walk(driver):
    _check(driver, [(4, 8, 0, 0, 2, at0(2, 2, 2, 3)), (2, 8, 0, 0, 2, [[3], [0, 1, 7], [5]]), (2, 8, 0, 0, 3, [[3], [0, 1, 7], [5]])],
           [["P 0 1 4", "P 2 2 2", "E 7"], ["P 0 0 1", "R 1 0 8 3", "E 7"], ["P 0 0 1", "R 1 0 8 3", "R 1 0 4 2 *", "E 7"]])


def test_random_scenarios(driver):
    rng = random.Random(20261)
    scenarios = []
    for _ in range(200):
        cap = rng.randint(2, 8)
        mode = rng.randrange(4)
        n = rng.randint(0, 12)
        counts = [rng.choice((0, 0, 1, 2, cap - 1, cap, cap + 1, 2 * cap + 1, rng.randint(0, 3 * cap))) for _ in range(n)]
        fail_at = rng.choice((0, 0, 0, rng.randint(1, 6)))
        if mode == 3:                               # the query loop: one position, the hits of a query over the capacity outside it
            scenarios.append((cap, 1, rng.randint(1, 5), 0, fail_at, [[1 if c > cap else 0] * c for c in counts]))
            continue
        span = rng.randint(1, 64)
        bins = [[rng.randrange(span) for _ in range(c)] for c in counts]
        scenarios.append((cap, span, 0, rng.randint(1, 20) if mode == 2 else 0, fail_at, bins))
    over = [s for s in scenarios if restate(*s, walk=walk_targets if s[2] == 0 and s[3] == 0 else None)[-1] == "E over"]
    assert len(over) <= len(scenarios) // 4
    got = _check(driver, [s for s in scenarios if s not in over])
    assert sum(1 for g in got for ln in g if ln.startswith("R ") and not ln.endswith("*")) > 50 and sum(1 for g in got if g[-1] == "E 7") > 10
