"""GPU tests of the accessibility of intervals (mirp_unpaired_batch, unpaired_kernels.hip): the device's efe, efe_open and upe
against the masked restatement of tests/test_unpaired_cpu.py (pinned there to the filtered enumeration of every structure) over §24's pinned
values, the lengths around the wave and the two-cells-per-lane boundary and the longest window, intervals at either end, over the whole window,
over a single base and across a hairpin's stem, 200 seeded windows with planted hairpins and N letters, and the G/C 128-mer; the single-base
identity against the device's own pair probabilities (mirp_ensemble); bit-equality over call compositions and forced pass capacities; the
refusals and the statistics.  Tolerance (§24, from §23): 1e-8 kcal/mol on all three values.  The restatement runs in worker processes that are
started fresh (spawn), never forked from a process that holds a device context."""
import math
import multiprocessing
import random

import numpy as np
import pytest

from tests.test_ensemble_cpu import KT, planted_hairpin, random_seq, seeded
from tests.test_unpaired_cpu import GC128, HAIRPIN20, PINS, upe_job

pytestmark = pytest.mark.gpu
TOL = 1e-8
FIELDS = ("efe", "efe_open", "upe")


def intervals_of(n):
    """first base, last base, whole window, a single base inside, four bases a quarter in (across the stem of a planted hairpin)"""
    out = [(1, 1), (n, n), (1, n), ((n + 1) // 2, (n + 1) // 2), (n // 4 + 1, min(n, n // 4 + 4))]
    return sorted(set(out))


def _shapes():
    rng = random.Random(2408)
    seqs = [random_seq(rng, n, "GC") if n < 12 else planted_hairpin(rng, n) for n in (1, 4, 5, 8, 31, 32, 33, 63, 64, 65, 127, 128)]
    return [(s, lo, hi) for s in seqs for lo, hi in intervals_of(len(s))]


def _seeded():
    rng = random.Random(2409)
    out = []
    for k, s in enumerate(seeded(2410, 200, 20, 128)):
        n = len(s)
        if k % 5 == 4:                      # N letters, other ambiguity codes and lower case
            t = list(s)
            for _ in range(1 + n // 15):
                t[rng.randrange(n)] = rng.choice("NRYn")
            s = "".join(t)
            if k % 10 == 9:
                s = s.lower().replace("u", "t")
        width = rng.choice((1, 4, 20, 21, 22, 33))
        lo = rng.randint(1, max(1, n - width + 1))
        out.append((s, lo, min(n, lo + width - 1)))
    return out


SHAPES = _shapes()
SEEDED = _seeded()
BITS = [(s, lo, hi) for (s, lo, hi) in _seeded()[3::4]][:50]


@pytest.fixture(scope="module")
def restated():
    """(sequence, lo, hi) -> restate_upe, computed once per window in a pool of fresh processes"""
    cache = {}
    with multiprocessing.get_context("spawn").Pool(14) as pool:
        def many(jobs):
            todo = sorted({j for j in jobs if j not in cache}, key=lambda j: len(j[0]), reverse=True)
            for j, res in zip(todo, pool.map(upe_job, todo, chunksize=1)):
                cache[j] = res
            return [cache[j] for j in jobs]
        yield many


def run(ctx, jobs, **kw):
    return ctx.unpaired_batch([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], **kw)


def compare(jobs, recs, want, label):
    worst = dict.fromkeys(FIELDS, 0.0)
    for j, r, w in zip(jobs, recs, want):
        for f in FIELDS:
            worst[f] = max(worst[f], abs(float(r[f]) - w[f]))
    print("%s: %d windows, largest deviations %s kcal/mol" % (label, len(jobs), ", ".join("%s %.3g" % (f, worst[f]) for f in FIELDS)))
    for j, r, w in zip(jobs, recs, want):
        for f in FIELDS:
            assert abs(float(r[f]) - w[f]) <= TOL, (j, f, float(r[f]), w[f])
        assert float(r["upe"]) >= -TOL


def test_pins(gpu_ctx, restated):
    jobs = [(s, lo, hi) for s, lo, hi, _, _, _ in PINS]
    recs = run(gpu_ctx, jobs)
    for (s, lo, hi, efe_open, efe, upe), r in zip(PINS, recs):
        print("%s [%d,%d]: efe_open %.12f efe %.12f upe %.12f" % (s if len(s) < 30 else "G/C 128-mer", lo, hi, r["efe_open"], r["efe"], r["upe"]))
        assert abs(r["efe_open"] - efe_open) <= TOL and abs(r["efe"] - efe) <= TOL and abs(r["upe"] - upe) <= TOL, (s, lo, hi)
    compare(jobs, recs, restated(jobs), "pins")
    assert recs[4]["efe"] == 0.0 and recs[4]["efe_open"] == 0.0 and recs[4]["upe"] == 0.0          # AAAA


def test_lengths_and_intervals(gpu_ctx, restated):
    assert sorted({len(s) for s, _, _ in SHAPES}) == [1, 4, 5, 8, 31, 32, 33, 63, 64, 65, 127, 128]
    compare(SHAPES, run(gpu_ctx, SHAPES), restated(SHAPES), "shapes")
    stem = [(HAIRPIN20, 3, 6), (HAIRPIN20, 15, 19), (HAIRPIN20, 1, 20), (HAIRPIN20, 20, 20)]
    recs = run(gpu_ctx, stem)
    compare(stem, recs, restated(stem), "across a stem")
    assert recs[0]["upe"] > 10 and recs[1]["upe"] > 10 and abs(recs[2]["efe_open"]) <= TOL


def test_seeded_windows(gpu_ctx, restated):
    assert len(SEEDED) == 200 and min(len(j[0]) for j in SEEDED) >= 20 and max(len(j[0]) for j in SEEDED) == 128
    assert sum("N" in j[0].upper() for j in SEEDED) >= 30
    recs = run(gpu_ctx, SEEDED)
    compare(SEEDED, recs, restated(SEEDED), "seeded")
    assert sum(r["upe"] > 1.0 for r in recs) >= 40 and sum(r["efe"] < -5.0 for r in recs) >= 40


def test_gc_128mer(gpu_ctx, restated):
    jobs = [(GC128, 1, 21), (GC128, 63, 66), (GC128, 108, 128), (GC128, 1, 128)]
    recs = run(gpu_ctx, jobs)
    compare(jobs, recs, restated(jobs), "G/C 128-mer")
    assert recs[0]["efe"] < -190 and recs[1]["upe"] < 1e-3 and abs(recs[3]["efe_open"]) <= TOL


def test_single_base_is_the_device_s_unpaired_probability(gpu_ctx):
    seqs = seeded(2411, 12, 30, 70)
    _, _, bpp = gpu_ctx.ensemble(seqs, bpp_cutoff=0)
    jobs, want = [], []
    for q, s in enumerate(seqs):
        rows = np.zeros(len(s))
        mine = bpp[bpp["seq"] == q]
        np.add.at(rows, mine["i"] - 1, mine["p"])
        np.add.at(rows, mine["j"] - 1, mine["p"])
        for a in random.Random(q).sample(range(len(s)), 4):
            jobs.append((s, a + 1, a + 1))
            want.append(0.0 - KT * math.log(1.0 - rows[a]))
    recs = run(gpu_ctx, jobs)
    worst = max(abs(float(r["upe"]) - w) for r, w in zip(recs, want))
    print("single base against mirp_ensemble: largest difference %.3g kcal/mol" % worst)
    assert worst <= TOL


def test_bit_equality_over_compositions_and_capacities(gpu_ctx):
    assert len(BITS) == 50
    together = run(gpu_ctx, BITS)
    assert gpu_ctx.unpaired_last_stats()["passes"] == 1
    for k in (0, 7, 49):
        alone = run(gpu_ctx, [BITS[k]])
        for f in FIELDS:
            assert alone[f][0].tobytes() == together[f][k].tobytes(), (k, f)
    order = list(range(50))
    random.Random(2412).shuffle(order)
    shuffled = run(gpu_ctx, [BITS[k] for k in order] + SHAPES[-5:])
    for at, k in enumerate(order):
        for f in FIELDS:
            assert shuffled[f][at].tobytes() == together[f][k].tobytes(), (k, f)
    for cap, passes in ((1, 50), (7, 8), (49, 2)):
        split = run(gpu_ctx, BITS, capacity=cap)
        assert gpu_ctx.unpaired_last_stats()["passes"] == passes
        for f in FIELDS:
            assert split[f].tobytes() == together[f].tobytes(), (cap, f)


def test_refusals(gpu_ctx):
    from mir_prefer_amd import capi
    ok = ("GGGAAACCC", 1, 3)
    bad = [(("", 1, 1), "an empty sequence"), (("A" * 129, 1, 1), "longer than 128"), ((b"ACG\x80U", 1, 1), "0x80"), (("ACGU", 0, 2), "interval"),
           (("ACGU", 3, 2), "interval"), (("ACGU", 2, 5), "interval")]
    for job, what in bad:
        with pytest.raises(capi.MirpError) as e:
            run(gpu_ctx, [ok, ok, job, ok])
        assert "-10" in str(e.value) and "record 3" in str(e.value) and what in str(e.value), str(e.value)
    assert gpu_ctx.lib.mirp_unpaired_batch(gpu_ctx.h, b"", None, None, None, -1, None) == -1
    assert len(run(gpu_ctx, [])) == 0 and gpu_ctx.unpaired_last_stats() == dict(windows=0, passes=0, cells=0)
    assert gpu_ctx.lib.mirp_set_target_flanks(gpu_ctx.h, 90, 6) == -1 and gpu_ctx.lib.mirp_set_target_flanks(gpu_ctx.h, -1, 0) == -1
    assert gpu_ctx.lib.mirp_set_target_flanks(gpu_ctx.h, 17, 13) == 0
    assert len(run(gpu_ctx, [ok])) == 1          # the context still works


def test_last_stats(gpu_ctx):
    jobs = [("A" * 128, 5, 9), (HAIRPIN20, 3, 6), ("ACGU", 1, 4), ("G", 1, 1)]
    run(gpu_ctx, jobs, capacity=3)
    assert gpu_ctx.unpaired_last_stats() == dict(windows=4, passes=2, cells=128 * 127 // 2 + 190 + 6 + 0)
