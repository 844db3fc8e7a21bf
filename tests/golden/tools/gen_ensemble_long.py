#!/usr/bin/env python3
"""Dev-only: the recorded reference of the partition function at 700..1,400 nt, tests/golden/ensemble_long.json.gz.

The six sequences of tests/test_ensemble_long_cpu.py's recipes go through restate() / record_of() of tests/test_ensemble_cpu.py (the inside /
outside program on x87 extended doubles, pinned there to the enumeration of every structure) with the CPU oracle's MFE, one fresh (spawned)
process per sequence: about n^2 * 70 us each, two and a half minutes in all on six cores, under 300 MB per process.  Stored per sequence: the recipe, the
letters, n, ln Z, the record's fields, the centroid text, min_gap (the smallest |p - 0.5|), every pair with p >= 5e-4 as 1-based i, j and p rounded
to 14 decimals, and row[x] = the sum of p over the pairs that hold position x, taken from the whole matrix.

What the recipes are for is asserted here, before anything is written: min_gap >= 1e-6 everywhere; a pair with p > 0.5 and i >= 1024 (0-based)
in the sequences of 1,100 nt and more; p(1024, 1028) >= 1e-6 in the 1,029-mer.  A recipe that fails gets another seed, never a skip.

    python tests/golden/tools/gen_ensemble_long.py            # writes the file
    python tests/golden/tools/gen_ensemble_long.py --verify   # recomputes and compares with the committed file
"""
import gzip
import json
import multiprocessing
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(GOLD, "ensemble_long.json.gz")
LIMIT = 421_000          # bytes: the largest fixture committed before this one


def job(recipe):
    """recipe -> the fixture's entry; a module-level function so that a spawned worker can run it"""
    import numpy as np
    from tests.test_ensemble_cpu import record_of, restate
    from tests.test_ensemble_long_cpu import SLAB_THREADS, STORED_FROM, build, normalised
    from tests.test_randfold_cpu import oracle_mfe
    t0 = time.time()
    s = build(recipe)
    r = restate(s)
    n = r["n"]
    rec = record_of(r, oracle_mfe((normalised(s).encode(), "vienna-2.1.2")))
    row = np.zeros(n)
    for (i, j), v in r["p"].items():
        row[i] += v
        row[j] += v
    stored = sorted((i + 1, j + 1, round(v, 14)) for (i, j), v in r["p"].items() if v >= STORED_FROM)
    assert r["min_gap"] >= 1e-6, (n, r["min_gap"])
    entry = dict(recipe=recipe, seq=s, n=n, lnz=r["lnz"], record=rec, centroid=r["centroid"], min_gap=r["min_gap"], nonzero_pairs=len(r["p"]),
                 pairs_i=[x[0] for x in stored], pairs_j=[x[1] for x in stored], pairs_p=[x[2] for x in stored], row=[round(float(v), 14) for v in row])
    if n >= 1100:
        assert any(v > 0.5 and i >= SLAB_THREADS for (i, j), v in r["p"].items()), n
    if n == 1029:
        entry["p_spilled_cell"] = r["p"].get((SLAB_THREADS, SLAB_THREADS + 4), 0.0)
        assert entry["p_spilled_cell"] >= 1e-6, entry["p_spilled_cell"]
    print("n = %d: %.0f s, efe %.4f, mfe %d, %d non-zero p, %d stored, min_gap %.3g" % (n, time.time() - t0, rec["efe"], rec["mfe"], len(r["p"]), len(stored),
                                                                                     r["min_gap"]), flush=True)
    return entry


def close(a, b, path=""):
    """equal texts and integers; floats to 1e-12 (relative above 1)"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(close(a[k], b[k], path + "/" + k) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(close(x, y, path) for x, y in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        ok = abs(a - b) <= 1e-12 * max(1.0, abs(a))
    else:
        ok = a == b
    if not ok:
        print("differs at %s: %r != %r" % (path, a, b))
    return ok


def main():
    from tests.test_ensemble_long_cpu import LENGTHS, RECIPES
    verify = sys.argv[1:] == ["--verify"]
    assert verify or not sys.argv[1:], __doc__
    order = sorted(range(len(RECIPES)), key=lambda k: -LENGTHS[k])          # the longest first
    with multiprocessing.get_context("spawn").Pool(min(6, os.cpu_count() or 1), maxtasksperchild=1) as pool:
        done = pool.map(job, [RECIPES[k] for k in order], chunksize=1)
    entries = [None] * len(RECIPES)
    for k, e in zip(order, done):
        entries[k] = e
    assert [e["n"] for e in entries] == LENGTHS
    fx = dict(generator="tests/golden/tools/gen_ensemble_long.py: restate() and record_of() of tests/test_ensemble_cpu.py, the MFE from oracle/lfold.c",
              stored_from=5e-4, sequences=entries)
    fx = json.loads(json.dumps(fx))
    if verify:
        with gzip.open(PATH, "rt") as f:
            old = json.load(f)
        if not close(old, fx):
            sys.exit("the recomputed reference differs from " + PATH)
        print("verified", PATH)
        return
    with open(PATH, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as f:
        f.write(json.dumps(fx, separators=(",", ":")).encode())
    size = os.path.getsize(PATH)
    print("wrote", PATH, size, "bytes")
    assert size < LIMIT, "raise the stored-pair threshold"


if __name__ == "__main__":
    main()
