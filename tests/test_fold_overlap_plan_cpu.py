"""CPU tests of the chunk plan of the fold overlap (mir-prefer_amd/csrc/fold_overlap_plan.h): a small driver that includes the
header and nothing else of the project is compiled with the host C++ compiler.  It prints the header's constants, then for every input line
`n_work round cap request schedule` the chunk sizes of the plan on one line (an empty line: the serial path); started with the argument `ring` it
prints the plan's ring layout instead (fold_overlap_ring): the number of slots, their capacities and their first windows, the last being the total."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "fold_overlap_plan.h"

int main(int argc, char**) {
    std::printf("%d %d %d %d %d\n", mirp::FOLD_OVERLAP_CHUNKS, mirp::FOLD_OVERLAP_MIN_ROUNDS, mirp::FOLD_OVERLAP_EPI_RATIO_PERMILLE,
                mirp::FOLD_OVERLAP_TAPER_PERMILLE, mirp::FOLD_OVERLAP_LAST_ROUNDS);
    long long n, round, cap, request;
    int schedule;
    while (std::scanf("%lld %lld %lld %lld %d", &n, &round, &cap, &request, &schedule) == 5) {
        const std::vector<int> plan = mirp::fold_overlap_plan(n, round, cap, request, schedule);
        if (argc > 1) {
            const mirp::FoldRing ring = mirp::fold_overlap_ring(plan);
            std::printf("%d", mirp::FOLD_RING_SLOTS);
            for (int s = 0; s < mirp::FOLD_RING_SLOTS; s++) std::printf(" %zu", ring.cap[s]);
            for (int s = 0; s <= mirp::FOLD_RING_SLOTS; s++) std::printf(" %zu", ring.at[s]);
            std::printf(" %zu\n", ring.windows());
            continue;
        }
        for (size_t k = 0; k < plan.size(); k++) std::printf("%s%d", k ? " " : "", plan[k]);
        std::printf("\n");
    }
    return 0;
}
"""

ORDERED, TAILFREE = 0, 1


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("fold_overlap_plan")
    (d / "driver.cpp").write_text(DRIVER)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "mir-prefer_amd", "csrc"), str(d / "driver.cpp"), "-o", str(d / "driver")])

    def run(cases, ring=False):
        """cases: (n_work, round, cap, request, schedule) each -> (the header's constants, the chunk sizes of each, or with `ring` the ring's numbers)"""
        text = "".join("%d %d %d %d %d\n" % c for c in cases)
        out = subprocess.run([str(d / "driver")] + (["ring"] if ring else []), input=text.encode(), capture_output=True, timeout=60, check=True).stdout.decode().split("\n")[:-1]
        assert len(out) == 1 + len(cases)
        return tuple(int(x) for x in out[0].split()), [[int(x) for x in ln.split()] for ln in out[1:]]
    return run


GRID = [c for c in itertools.product((1, 2, 39, 40, 511, 512, 4095, 4096, 4097, 5000, 19686, 70244, 300001), (1, 8, 512), (1, 100, 4097, 7680, 1 << 20),
                                     (-1, 0, 1, 2, 64, 5120, 1 << 21), (ORDERED, TAILFREE))]


def test_sizes_are_positive_sum_to_the_batch_and_fit_a_slot(plan):
    _, got = plan(GRID)
    n_plans = 0
    for (n, rnd, cap, req, sched), sizes in zip(GRID, got):
        if not sizes:
            continue
        n_plans += 1
        assert all(s > 0 for s in sizes) and sum(sizes) == n, (n, rnd, cap, req, sched, sizes)
        assert max(sizes) <= cap, (n, rnd, cap, req, sched, sizes)
    assert n_plans > len(GRID) // 3


def test_a_request_gives_equal_chunks_with_the_remainder_last(plan):
    cases = [c for c in GRID if c[3] > 0]
    _, got = plan(cases)
    for (n, rnd, cap, req, sched), sizes in zip(cases, got):
        size = min(req, cap)
        assert sizes == [size] * (n // size) + ([n % size] if n % size else []), (n, rnd, cap, req, sched)
        assert len(sizes) == -(-n // size)


def test_the_empty_plan(plan):
    (_, min_rounds, _, _, _), _ = plan([])
    assert min_rounds == 8
    cases = [c for c in GRID if c[3] <= 0]
    _, got = plan(cases)
    for (n, rnd, cap, req, sched), sizes in zip(cases, got):
        if req == 0 or n < min_rounds * rnd:
            assert sizes == [], (n, rnd, cap, req, sched)      # off, or an automatic batch below 8 rounds of the fill grid
        assert len(sizes) != 1                                  # automatic: fewer than two chunks is the serial path
    _, got = plan([(0, 512, 7680, -1, TAILFREE), (0, 512, 7680, 64, TAILFREE), (-5, 512, 7680, 64, ORDERED), (4095, 512, 7680, -1, TAILFREE), (4096, 512, 7680, -1, TAILFREE),
                   (4096, 512, 1 << 20, -1, ORDERED)])
    assert got[:4] == [[], [], [], []] and len(got[4]) >= 2 and got[5] == [1024] * 4


def test_the_tailfree_plan_lets_every_epilogue_end_before_the_next_fill(plan):
    """chunk[k + 1] >= r * chunk[k] for the shipped r (the epilogue's time beside a fill over that chunk's fill time), with the margin the header states."""
    cases = [c for c in GRID if c[3] == -1 and c[4] == TAILFREE] + [(n, 512, 7680, -1, TAILFREE) for n in range(4096, 90000, 997)]
    (_, _, ratio, taper, last_rounds), got = plan(cases)
    assert 0 < ratio <= taper <= 1000
    n_plans = 0
    for (n, rnd, cap, req, sched), sizes in zip(cases, got):
        for a, b in zip(sizes, sizes[1:]):
            assert 1000 * b >= taper * a >= ratio * a, (n, rnd, cap, sizes)
        if sizes:
            n_plans += 1
            assert sizes[-1] <= max(last_rounds * rnd, 1)       # the exposed epilogue is the smallest chunk's
    assert n_plans >= 80


def test_mode_0_reproduces_the_plan_of_round_9(plan):
    _, got = plan([(19686, 512, 7680, -1, ORDERED), (70244, 512, 7680, -1, ORDERED), (19686, 512, 4000, -1, ORDERED)])
    assert got[0] == [5120, 5120, 5120, 4326]
    assert len(got[1]) == 10 and got[1] == [7680] * 9 + [70244 - 9 * 7680]
    assert got[2] == [3584] * 5 + [19686 - 5 * 3584]      # whole rounds under the slot capacity


def test_the_tailfree_plan_of_the_benchmark_batches(plan):
    """The two batches the design log quotes: the plan tapers from the slot capacity (or what the batch leaves) down to the last chunk."""
    (_, _, _, taper, last_rounds), got = plan([(19686, 512, 7680, -1, TAILFREE), (70244, 512, 7680, -1, TAILFREE)])
    for n, sizes in zip((19686, 70244), got):
        assert sum(sizes) == n and sizes[-1] == last_rounds * 512 and max(sizes) <= 7680
        assert sizes[1:] == sorted(sizes[1:], reverse=True)


def test_the_ring_holds_every_chunk_in_slot_k_mod_3_without_overlap(plan):
    """fold_overlap_ring over every plan of GRID: chunk k sits in slot k % 3 and fits it, the slots lie side by side, and the whole ring is the sum of
    the per-slot maxima, at most three slots of the capacity."""
    _, plans = plan(GRID)
    _, rings = plan(GRID, ring=True)
    n_plans = 0
    for (n, rnd, cap, req, sched), sizes, ring in zip(GRID, plans, rings):
        slots, caps, at, total = ring[0], ring[1:4], ring[4:8], ring[8]
        assert slots == 3 and len(ring) == 9
        per_slot = [max(sizes[s::3], default=0) for s in range(3)]
        assert caps == per_slot, (n, rnd, cap, req, sched)
        for k, size in enumerate(sizes):
            assert at[k % 3] + size <= at[k % 3] + caps[k % 3] == at[k % 3 + 1]       # chunk k: slot k % 3, inside it, and the next slot starts behind it
        assert at[0] == 0 and all(at[s] + caps[s] <= at[s + 1] for s in range(3))     # no two slots overlap
        assert total == at[3] == sum(per_slot)
        if sizes:
            n_plans += 1
            assert total <= 3 * cap, (n, rnd, cap, req, sched)
    assert n_plans > len(GRID) // 3
