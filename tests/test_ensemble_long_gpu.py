"""GPU tests of the partition function's slab kernels (en_inside_kernel<false> / en_outside_kernel<false>) where they differ from the
301..400 nt that tests/test_ensemble_gpu.py restates: six sequences of 700, 1,027, 1,028, 1,029, 1,100 and 1,400 nt with real structure against the
recorded restatement (tests/golden/ensemble_long.json.gz, pinned by tests/test_ensemble_long_cpu.py).  With 1,024 threads a diagonal of n - d cells
gives a thread a second cell from n = 1,029 on: 700 nt stays below the thread count, 1,027 and 1,028 nt are the last lengths with one cell per thread,
1,029 nt has exactly one second cell, (1024, 1028), which the sequence closes with a triloop hairpin, 1,100 nt has 2,628 and 1,400 nt about 70,000,
among them a hairpin loop of 210 N; the exterior sweeps and the initial fill stride the same way.  Every sequence of 1,100 nt and more has a
centroid pair at i >= 1024.  The second test puts slab jobs before ring jobs in call order and across a pass boundary.
Tolerances (§23): 1e-8 kcal/mol for efe, 1e-8 absolute for p, the row sums, diversity and centroid_dist, 1e-8 relative for mfe_freq."""
import random

import numpy as np
import pytest

from tests.test_ensemble_cpu import planted_hairpin
from tests.test_ensemble_gpu import _per_sequence
from tests.test_ensemble_long_cpu import LENGTHS, STORED_FROM, load

pytestmark = pytest.mark.gpu
TOL = dict(efe=1e-8, p=1e-8, row=1e-8, mfe_freq=1e-8, diversity=1e-8, centroid_dist=1e-8)


@pytest.fixture(scope="module")
def entries():
    return load()["sequences"]


@pytest.fixture(scope="module")
def one_call(gpu_ctx, entries):
    """the six sequences in fixture order, every p: (records, centroid texts, pair list, where each sequence's pairs begin)"""
    recs, cens, bpp = gpu_ctx.ensemble([e["seq"] for e in entries], bpp_cutoff=0.0)
    assert gpu_ctx.ensemble_last_stats()["passes"] == 1
    key = (bpp["seq"].astype(np.int64) << 24) | (bpp["i"].astype(np.int64) << 12) | bpp["j"]
    assert np.all(np.diff(key) > 0), "ordered by (seq, i, j)"
    return recs, cens, bpp, np.searchsorted(bpp["seq"], np.arange(len(entries) + 1))


def matrix(n, i, j, p):
    m = np.zeros((n + 1, n + 1))
    m[i, j] = p
    return m


@pytest.mark.parametrize("q", range(len(LENGTHS)), ids=[str(n) for n in LENGTHS])
def test_long_sequences_against_the_recorded_restatement(one_call, entries, q):
    recs, cens, bpp, bounds = one_call
    assert len(recs) == len(cens) == len(entries) == len(LENGTHS) and bounds[-1] == len(bpp)
    e, g = entries[q], recs[q]
    n, w = e["n"], e["record"]
    mine = bpp[bounds[q]:bounds[q + 1]]
    # complete: strictly ordered, (n - 4)(n - 3) / 2 entries, each a cell with j - i >= 4
    assert len(mine) == (n - 4) * (n - 3) // 2 and mine["i"].min() >= 1 and mine["j"].max() <= n and (mine["j"] - mine["i"]).min() >= 4
    got = matrix(n, mine["i"], mine["j"], mine["p"])
    dev = {"efe": abs(float(g["efe"]) - w["efe"]), "mfe_freq": abs(float(g["mfe_freq"]) - w["mfe_freq"]) / w["mfe_freq"],
           "diversity": abs(float(g["diversity"]) - w["diversity"]), "centroid_dist": abs(float(g["centroid_dist"]) - w["centroid_dist"]),
           "p": float(np.abs(got[e["i"], e["j"]] - e["p"]).max()),
           "row": float(np.abs((got.sum(axis=0) + got.sum(axis=1))[1:] - e["row"]).max())}
    rest = got.copy()
    rest[e["i"], e["j"]] = 0.0
    print("n = %d: largest deviations %s; largest p not stored %.6g" % (n, ", ".join("%s %.2e" % kv for kv in dev.items()), rest.max()))
    assert (int(g["len"]), int(g["mfe"]), int(g["centroid_pairs"])) == (n, w["mfe"], w["centroid_pairs"]), (n, g, w)
    assert cens[q] == e["centroid"].encode(), n
    for k, v in dev.items():
        assert v <= TOL[k], (n, k, v)
    assert rest.max() < STORED_FROM + TOL["p"], n


def _pairs_at(entry, got_bpp, cutoff):
    """the pair list of one sequence at a cutoff against the stored pairs, as test_the_pair_list does: at or above cutoff + tol listed and equal within
    tol, at or below cutoff - tol absent, and nothing listed that is not stored (every restated p >= 5e-4 is)"""
    assert cutoff - TOL["p"] > STORED_FROM
    key = entry["i"] * 4096 + entry["j"]
    got_key = got_bpp["i"].astype(np.int64) * 4096 + got_bpp["j"]
    assert np.all(np.diff(got_key) > 0) and got_bpp["p"].min() >= cutoff
    at = np.searchsorted(key, got_key)
    assert at.max() < len(key) and np.array_equal(key[at], got_key), "a listed pair that the restatement has below 5e-4"
    assert np.abs(got_bpp["p"] - entry["p"][at]).max() <= TOL["p"]
    listed = np.zeros(len(key), dtype=bool)
    listed[at] = True
    assert listed[entry["p"] >= cutoff + TOL["p"]].all() and not listed[entry["p"] <= cutoff - TOL["p"]].any()
    return int(listed.sum())


def test_slab_jobs_before_ring_jobs_keep_their_bits(gpu_ctx, entries):
    rng = random.Random(2337)
    e1029, e700 = entries[LENGTHS.index(1029)], entries[LENGTHS.index(700)]
    seqs = [e1029["seq"], planted_hairpin(rng, 40), e700["seq"], planted_hairpin(rng, 300), planted_hairpin(rng, 301)]
    assert [len(s) for s in seqs] == [1029, 40, 700, 300, 301]
    got = gpu_ctx.ensemble(seqs, bpp_cutoff=1e-3)
    assert gpu_ctx.ensemble_last_stats()["passes"] == 1
    whole = _per_sequence(got, len(seqs))
    for q, s in enumerate(seqs):
        assert _per_sequence(gpu_ctx.ensemble([s], bpp_cutoff=1e-3), 1)[0] == whole[q], q
    # 40 MB: the 1,029-mer's slab (38.2 MB) and the 40-mer, then the 700-mer (17.7 MB) before the two of 300 and 301 nt
    assert _per_sequence(gpu_ctx.ensemble(seqs, bpp_cutoff=1e-3, capacity=40_000_000), len(seqs)) == whole
    assert gpu_ctx.ensemble_last_stats()["passes"] == 2
    recs, cens, bpp = got
    bounds = np.searchsorted(bpp["seq"], np.arange(len(seqs) + 1))
    for q, e in ((0, e1029), (2, e700)):
        assert cens[q] == e["centroid"].encode() and int(recs["centroid_pairs"][q]) == e["record"]["centroid_pairs"], q
        assert _pairs_at(e, bpp[bounds[q]:bounds[q + 1]], 1e-3) > 500, q
