"""GPU tests of the partition function (mirp_ensemble, ensemble_kernels.hip) and of the `ensemble` command: the device's records,
centroid texts and pair probabilities against the restatement of tests/test_ensemble_cpu.py (pinned there to the enumeration of every structure
and to the CPU oracle) over §23's pinned values, the lengths around the wave, ring and LDS / slab boundaries, 212 seeded sequences, the range
cases of 3,000 nt, bit-equality over call compositions and forced pass capacities, the pair list's cutoff and order, the refusals, and whole runs
of the command.  Tolerances (§23): 1e-8 kcal/mol for efe, 1e-8 absolute for p, diversity and centroid_dist, 1e-8 relative for mfe_freq.  Every
sequence compared through a threshold (p > 0.5, the list's cutoff) has no restated p within 1e-6 of it: asserted, never skipped.  The restatement
runs in worker processes that are started fresh (spawn), never forked from a process that holds a device context."""
import multiprocessing
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.test_ensemble_cpu import MULTI, planted_hairpin, qualifies, random_seq, range_hairpin, restate_job, seeded
from tests.test_targets_cpu import ROOT

pytestmark = pytest.mark.gpu
TOL = 1e-8
HAIRPIN20 = "GGGAGCUCGAAAGAGCUCCC"


def _shapes():
    rng = random.Random(2308)
    return [random_seq(rng, n, "GC") if n < 12 else planted_hairpin(rng, n) for n in (1, 4, 5, 8, 31, 32, 33, 63, 64, 65, 299, 300, 301)]


SHAPES = _shapes()
SEEDED = seeded(2310, 200, 20, 150) + seeded(2311, 12, 250, 400)
PAIRLIST = SEEDED[:20] + SEEDED[21:24] + SEEDED[25:42]          # (20 and 24 have a p within 1e-6 of the cutoff 0.001)
BITS = seeded(2312, 50, 20, 150)
FILE = seeded(2313, 10, 30, 120) + [MULTI, "AAAA"]
H300 = range_hairpin()


@pytest.fixture(scope="module")
def restated():
    """sequence -> (restate(), record), computed once per sequence in a pool of fresh processes"""
    cache = {}
    with multiprocessing.get_context("spawn").Pool(14) as pool:
        def many(seqs):
            todo = sorted({s for s in seqs if s not in cache}, key=len, reverse=True)
            for s, res in zip(todo, pool.map(restate_job, todo, chunksize=1)):
                cache[s] = res
            return [cache[s] for s in seqs]
        yield many


def dense(n, triples):
    m = np.zeros((n, n))
    for i, j, p in triples:
        m[i, j] = p
    return m


def compare(seqs, got, want, worst=None):
    """records, centroids and every p of a call with bpp_cutoff = 0 against the restatement; returns the largest deviations seen"""
    recs, cens, bpp = got
    worst = worst if worst is not None else dict(efe=0.0, p=0.0, diversity=0.0, centroid_dist=0.0, mfe_freq=0.0)
    assert len(recs) == len(cens) == len(seqs)
    assert np.all(np.diff(bpp["seq"].astype(np.int64) * (1 << 40) + bpp["i"].astype(np.int64) * (1 << 20) + bpp["j"]) > 0), "ordered by (seq, i, j)"
    bounds = np.searchsorted(bpp["seq"], np.arange(len(seqs) + 1))
    for q, (s, (r, w)) in enumerate(zip(seqs, want)):
        assert qualifies(r), (q, s)
        g = recs[q]
        n = len(s)
        assert (int(g["len"]), int(g["mfe"]), int(g["centroid_pairs"])) == (n, w["mfe"], w["centroid_pairs"]), (q, s, g, w)
        assert cens[q] == r["centroid"].encode(), (q, s, cens[q], r["centroid"])
        dev = {"efe": abs(float(g["efe"]) - w["efe"]), "diversity": abs(float(g["diversity"]) - w["diversity"]),
               "centroid_dist": abs(float(g["centroid_dist"]) - w["centroid_dist"]), "mfe_freq": abs(float(g["mfe_freq"]) - w["mfe_freq"]) / w["mfe_freq"]}
        mine = bpp[bounds[q]:bounds[q + 1]]
        assert len(mine) == max(n - 4, 0) * max(n - 3, 0) // 2, (q, s, len(mine))
        dev["p"] = float(np.abs(dense(n, zip(mine["i"] - 1, mine["j"] - 1, mine["p"])) - dense(n, [(i, j, v) for (i, j), v in r["p"].items()])).max()) if n else 0.0
        for k, v in dev.items():
            assert v <= TOL, (q, s, k, v)
            worst[k] = max(worst[k], v)
    return worst


# ---------------------------------------------------------------------------------------------------- the device against §23 and the restatement
def test_pins_on_the_device(gpu_ctx):
    recs, cens, bpp = gpu_ctx.ensemble(["AAAA", MULTI, HAIRPIN20], bpp_cutoff=0.1)
    assert cens == [b"....", b"............", b"((((((((....))))))))"]
    assert recs["len"].tolist() == [4, 12, 20] and recs["mfe"].tolist() == [0, 0, -1570] and recs["centroid_pairs"].tolist() == [0, 0, 8]
    assert recs["efe"][0] == 0.0 and recs["mfe_freq"][0] == 1.0 and recs["diversity"][0] == 0.0 and recs["centroid_dist"][0] == 0.0
    for q, (efe, freq, div, cd) in ((1, (-0.13219990016918653, 0.8069459981825868, 0.5758179863781583, 0.32860363993015557)),
                                    (2, (-15.733592149971926, 0.9469544100141003, 0.1020938120333924, 0.053694485438679135))):
        assert abs(recs["efe"][q] - efe) <= TOL and abs(recs["mfe_freq"][q] - freq) <= TOL * freq
        assert abs(recs["diversity"][q] - div) <= TOL and abs(recs["centroid_dist"][q] - cd) <= TOL
    assert [(int(b["seq"]), int(b["i"]), int(b["j"])) for b in bpp][:2] == [(1, 1, 12), (1, 2, 11)] and len(bpp) == 2 + 8
    assert abs(bpp["p"][0] - 0.1356745407608117) <= TOL and abs(bpp["p"][1] - 0.14273259353299395) <= TOL
    assert gpu_ctx.ensemble_last_stats() == {"sequences": 3, "passes": 1, "cells": 6 + 66 + 190}
    # the fold model of the context neither changes the result nor is changed
    try:
        gpu_ctx.set_fold_model("vienna-1.8.5")
        again = gpu_ctx.ensemble(["AAAA", MULTI, HAIRPIN20], bpp_cutoff=0.1)
        assert again[0].tobytes() == recs.tobytes() and again[2].tobytes() == bpp.tobytes()
    finally:
        gpu_ctx.set_fold_model("vienna-2.1.2")
    assert gpu_ctx.ensemble([])[0].shape == (0,)


def test_shapes(gpu_ctx, restated):
    assert [len(s) for s in SHAPES] == [1, 4, 5, 8, 31, 32, 33, 63, 64, 65, 299, 300, 301]
    got = gpu_ctx.ensemble(SHAPES, bpp_cutoff=0.0)
    print("largest deviations (shapes):", compare(SHAPES, got, restated(SHAPES)))
    assert got[0]["efe"][:2].tolist() == [0.0, 0.0] and got[1][0] == b"." and got[1][1] == b"...."


def test_seeded_sequences(gpu_ctx, restated):
    assert len(SEEDED) == 212 and sum(len(s) >= 250 for s in SEEDED) == 12
    got = gpu_ctx.ensemble(SEEDED, bpp_cutoff=0.0)
    print("largest deviations (212 seeded):", compare(SEEDED, got, restated(SEEDED)))
    assert sum(int(c) > 5 for c in got[0]["centroid_pairs"]) > 60


def test_range(gpu_ctx, restated):
    short, long_, full = "A" + H300, "A" * 2700 + H300, "G" * 1498 + "AAAA" + "C" * 1498
    assert len(long_) == len(full) == 3000
    recs, cens, bpp = gpu_ctx.ensemble([short, long_, full], bpp_cutoff=1e-6)
    compare([short], gpu_ctx.ensemble([short], bpp_cutoff=0.0), restated([short]))
    assert abs(recs["efe"][1] - recs["efe"][0]) <= TOL and recs["mfe"][1] == recs["mfe"][0] and recs["efe"][0] < -200
    assert cens[1] == b"." * 2699 + cens[0] and cens[0].count(b"(") > 100
    a, b = bpp[bpp["seq"] == 0], bpp[bpp["seq"] == 1]
    pa = {(int(x["i"]) + 2699, int(x["j"]) + 2699): float(x["p"]) for x in a}
    pb = {(int(x["i"]), int(x["j"])): float(x["p"]) for x in b}
    assert len(pa) > 100
    for k in set(pa) | set(pb):
        if k in pa and k in pb:
            assert abs(pa[k] - pb[k]) <= TOL, k
        else:                            # below the cutoff in the other call
            assert pa.get(k, pb.get(k)) < 1e-6 + TOL, k
    for f in ("diversity", "centroid_dist"):
        assert abs(recs[f][1] - recs[f][0]) <= TOL
    g = recs[2]
    assert all(np.isfinite(float(g[f])) for f in ("efe", "mfe_freq", "diversity", "centroid_dist"))
    assert g["efe"] <= g["mfe"] / 100 and g["mfe"] < -300000 and 0 < g["mfe_freq"] <= 1
    rows = np.zeros(3001)
    c = bpp[bpp["seq"] == 2]
    np.add.at(rows, c["i"], c["p"])
    np.add.at(rows, c["j"], c["p"])
    assert rows.max() <= 1 + 1e-9 and rows.max() > 0.9


def _per_sequence(got, n):
    recs, cens, bpp = got
    bounds = np.searchsorted(bpp["seq"], np.arange(n + 1))
    # the fields one by one: the bytes of a multi-field view keep the padding, which holds seq, the position in the call
    return [(recs[q].tobytes(), cens[q], b"".join(bpp[bounds[q]:bounds[q + 1]][f].tobytes() for f in ("i", "j", "p"))) for q in range(n)]


def test_bit_equality(gpu_ctx):
    n = len(BITS)
    assert n == 50
    whole = _per_sequence(gpu_ctx.ensemble(BITS, bpp_cutoff=0.001), n)
    assert gpu_ctx.ensemble_last_stats()["passes"] == 1
    for q, s in enumerate(BITS):
        assert _per_sequence(gpu_ctx.ensemble([s], bpp_cutoff=0.001), 1)[0] == whole[q], (q, s)
    order = list(range(n))
    random.Random(5).shuffle(order)
    mixed = _per_sequence(gpu_ctx.ensemble([BITS[q] for q in order] + ["G" * 350 + "AAAA" + "C" * 350], bpp_cutoff=0.001), n)
    assert [mixed[k] for k in range(n)] == [whole[q] for q in order]
    for cap in (400_000, 1_500_000, 5_000_000):
        assert _per_sequence(gpu_ctx.ensemble(BITS, bpp_cutoff=0.001, capacity=cap), n) == whole, cap
        assert gpu_ctx.ensemble_last_stats()["passes"] > 1, cap


def test_the_pair_list(gpu_ctx, restated):
    seqs = PAIRLIST
    assert len(seqs) == 40
    want = restated(seqs)
    for cutoff in (0.001, 0.05):
        recs, cens, bpp = gpu_ctx.ensemble(seqs, bpp_cutoff=cutoff)
        keys = [(int(b["seq"]), int(b["i"]), int(b["j"])) for b in bpp]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        got = dict(zip(keys, bpp["p"].tolist()))
        assert min(got.values()) >= cutoff
        for q, (r, _) in enumerate(want):
            assert qualifies(r, (cutoff,))
            for (i, j), v in r["p"].items():
                if v >= cutoff + TOL:
                    assert abs(got[(q, i + 1, j + 1)] - v) <= TOL, (q, i, j)
                elif v <= cutoff - TOL:
                    assert (q, i + 1, j + 1) not in got, (q, i, j)
        assert set(k for k in got) <= {(q, i + 1, j + 1) for q, (r, _) in enumerate(want) for (i, j) in r["p"]}


def test_refusals(gpu_ctx):
    from mir_prefer_amd import capi
    for seqs, record in (([b"ACGU", b"", b"GGGG"], 2), ([b"ACGU", b"GG", b"A" * 3001], 3), ([b"AC\x80U", b"GG"], 1), ([b"GGGAAACCC", b"AC\xffU"], 2)):
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.ensemble(seqs, bpp_cutoff=0.5)
        assert "(-10)" in str(e.value) and "record %d:" % record in str(e.value), str(e.value)
    recs, cens, bpp = gpu_ctx.ensemble([b"A" * 3000, b"acgtNNxx"], bpp_cutoff=0.5)
    assert recs["len"].tolist() == [3000, 8] and recs["efe"].tolist() == [0.0, 0.0] and len(bpp) == 0 and cens[1] == b"........"
    assert gpu_ctx.ensemble([], bpp_cutoff=0.5)[2].shape == (0,)


# ---------------------------------------------------------------------------------------------------- the command
def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.ensemble"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _same_print(fmt, v, tol):
    """the printed value when it does not depend on an error of tol, else None"""
    lo, hi = fmt % (v - tol), fmt % (v + tol)
    return lo if lo == hi else None


def test_the_command(restated, tmp_path):
    from mir_prefer_amd import ensemble
    names = ["seq%d" % k for k in range(len(FILE))]
    fa = tmp_path / "pre.fa"
    fa.write_text("".join(">%s some text\n%s\n%s\n" % (nm, s[:25], s[25:]) for nm, s in zip(names, FILE)))
    want = restated(FILE)
    assert all(qualifies(r, (0.05,)) for r, _ in want)
    r = _cli([str(fa)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    out = tmp_path / "pre.fa.ensemble.tsv"
    lines = out.read_text().split("\n")
    assert lines[0] + "\n" == ensemble.HEADER and lines[-1] == "" and len(lines) == len(FILE) + 2
    assert not (tmp_path / "pre.fa.ensemble.bpp.tsv").exists()
    decided = 0
    for nm, s, (rr, w), line in zip(names, FILE, want, lines[1:]):
        ref = ensemble.table_line(nm, w, rr["centroid"]).rstrip("\n").split("\t")
        got = line.split("\t")
        assert len(got) == 8 and got[:3] == ref[:3] and got[7] == ref[7], (got, ref)
        for col, fmt, v, tol in ((3, "%.2f", w["efe"], TOL), (4, "%.6g", w["mfe_freq"], TOL * w["mfe_freq"]), (5, "%.2f", w["diversity"], TOL),
                                 (6, "%.2f", w["centroid_dist"], TOL)):
            if v == 0 or _same_print(fmt, v, tol) is not None:          # (an exact 0, as of AAAA where Z = 1, is exact on the device too: 0.00)
                assert got[col] == ref[col], (nm, col, got, ref)
                decided += 1
    assert decided >= 4 * len(FILE) - 2
    # -p, -c and -o; the outputs of an earlier run go first
    r = _cli(["-p", "-c", "0.05", "-o", "t/x.tsv", str(fa)], tmp_path)
    assert r.returncode == 255 and b"Error: " in r.stderr and not list(tmp_path.glob("t/*"))          # no such directory
    (tmp_path / "t").mkdir()
    r = _cli(["-p", "-c", "0.05", "-o", "t/x.tsv", str(fa)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "t" / "x.tsv").read_text() == out.read_text()
    rows = [ln.split("\t") for ln in (tmp_path / "t" / "x.bpp.tsv").read_text().split("\n")[:-1]]
    got = {(nm, int(i), int(j)): p for nm, i, j, p in rows}
    assert [(names.index(nm), int(i), int(j)) for nm, i, j, _ in rows] == sorted((names.index(nm), int(i), int(j)) for nm, i, j, _ in rows)
    n_want = 0
    for nm, (rr, _) in zip(names, want):
        for (i, j), v in rr["p"].items():
            if v >= 0.05 + TOL:
                n_want += 1
                if _same_print("%.6f", v, TOL) is not None:
                    assert got[(nm, i + 1, j + 1)] == "%.6f" % v, (nm, i, j)
            elif v <= 0.05 - TOL:
                assert (nm, i + 1, j + 1) not in got
    assert len(got) == n_want > 50
    # a refused run leaves no file, not even an earlier run's
    bad = tmp_path / "t" / "bad.fa"
    bad.write_text(">a\nGGGAAACCC\n>b\n\n>c\nACGU\n")
    for nm in ("bad.fa.ensemble.tsv", "bad.fa.ensemble.bpp.tsv"):
        (tmp_path / "t" / nm).write_text("old\n")
    r = _cli(["-p", str(bad)], tmp_path)
    assert r.returncode == 255 and b"Error: " in r.stderr and b"record 2" in r.stderr, r.stderr.decode()
    assert sorted(p.name for p in (tmp_path / "t").iterdir()) == ["bad.fa", "x.bpp.tsv", "x.tsv"]
    assert _cli([str(tmp_path / "none.fa")], tmp_path).returncode == 255
