#!/usr/bin/env python3
"""Timing of the accessibility of intervals (mirp_unpaired_batch and targets -u) on seeded inputs.

    python profiles/tools/unpaired_time.py [--out build/unpaired_time/unpaired_time.json] [--cases a,b] [--repeats 3] [--ensemble-windows 2000]
                                           [--targets a,b,c] [--dir /tmp/targets_time]

Cases, random windows, seed 1, the interval 21 nt starting at base 18 (a default window of targets -u):
  a  100,000 windows of 51..63 nt
  b  10,000 windows of 128 nt
Each case runs once to load the code objects and then --repeats times in the same context; the later calls are reported: median, smallest and
largest of the wall time, the windows per second and the cells per second of the whole call (upload, the kernel's launches by length class,
download).  The point of comparison is mirp_ensemble, which the library already had, on the first --ensemble-windows windows of the same bytes,
alternating with calls of unpaired_batch on those windows alone: it runs one inside and one outside pass where the new call runs two inside
passes in one; `ratio` is the ensemble's wall time over the new call's.
--targets runs the three cases of profiles/tools/targets_time.py (its inputs, made on first use) without and with -u, alternating in the same
context, --repeats times after a warm-up pair, and reports the phases of both and the sites per second that the sort + cut phase gained."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": (100000, 51, 63), "b": (10000, 128, 128)}


def make_windows(n, lo, hi, seed=1):
    rng = np.random.RandomState(seed)
    acgu = np.frombuffer(b"ACGU", dtype=np.uint8)
    return [acgu[rng.randint(0, 4, size=int(L))].tobytes() for L in rng.randint(lo, hi + 1, size=n)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "unpaired_time", "unpaired_time.json"))
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ensemble-windows", type=int, default=2000)
    ap.add_argument("--targets", default="", help="cases of targets_time.py to run without and with -u, e.g. a,b,c")
    ap.add_argument("--dir", default="/tmp/targets_time")
    args = ap.parse_args()
    from mir_prefer_amd import capi
    ctx = capi.Context(0)
    result = {"cases": {}, "targets": {}}
    try:
        for case in [c for c in args.cases.split(",") if c]:
            n, lo, hi = CASES[case]
            seqs = make_windows(n, lo, hi)
            los, his = [18] * n, [38] * n
            walls = []
            for _ in range(1 + args.repeats):
                t = time.time()
                recs = ctx.unpaired_batch(seqs, los, his)
                walls.append(time.time() - t)
            assert (recs["upe"] >= -1e-9).all() and (recs["efe"] <= 1e-9).all()
            stats = ctx.unpaired_last_stats()
            m = min(n, args.ensemble_windows)
            small, base = [], []
            for _ in range(1 + args.repeats):
                t = time.time()
                sub = ctx.unpaired_batch(seqs[:m], los[:m], his[:m])
                small.append(time.time() - t)
                t = time.time()
                ens = ctx.ensemble(seqs[:m])[0]
                base.append(time.time() - t)
            assert np.abs(ens["efe"] - sub["efe"]).max() <= 1e-8 and sub.tobytes() == recs[:m].tobytes()
            row = {"windows": n, "cells": stats["cells"], "passes": stats["passes"], "first_wall_s": walls[0], "wall_s": spread(walls[1:]),
                   "windows_per_s": spread([n / w for w in walls[1:]]), "cells_per_s": spread([stats["cells"] / w for w in walls[1:]]),
                   "mean_upe": float(recs["upe"].mean()), "compared_windows": m, "unpaired_s": spread(small[1:]), "ensemble_s": spread(base[1:]),
                   "ratio": spread([b / s for b, s in zip(base[1:], small[1:])])}
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
        if args.targets:
            import targets_time
            paths = targets_time.make_inputs(args.dir)
            for case in args.targets.split(","):
                mk, tk, both = targets_time.CASES[case]
                out = os.path.join(args.dir, "case_%s_upe.tsv" % case)
                runs = {False: [], True: []}
                for _ in range(1 + args.repeats):
                    for u in (False, True):
                        t = time.time()
                        res = ctx.target_scan(paths[mk], [paths[k] for k in tk], out, max_half_score=8, both_strands=both, accessibility=u)
                        res["wall_s"] = time.time() - t
                        runs[u].append(res)
                phases = ("parse", "upload", "scan", "sort_cut", "emit_write")
                row = {"sites": runs[True][-1]["sites"], "passes": runs[True][-1]["passes"]}
                for u, key in ((False, "plain"), (True, "upe")):
                    row[key] = {"wall_s": spread([r["wall_s"] for r in runs[u][1:]])}
                    row[key].update({p: spread([r["seconds"][i] for r in runs[u][1:]]) for i, p in enumerate(phases)})
                gained = row["upe"]["sort_cut"]["median"] - row["plain"]["sort_cut"]["median"]
                row["sites_per_s_of_the_gain"] = row["sites"] / gained if gained > 0 else None
                result["targets"][case] = row
                print("targets", case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
