#!/usr/bin/env python3
"""Timing of the gapped alignment of precursors with known hairpins (mirp_hairpin_align) on seeded inputs.

    python profiles/tools/hairpins_time.py [--out build/hairpins_time/hairpins_time.json] [--cases a,b] [--repeats 3] [--numpy-queries N]

Cases, random sequences, seed 1: 500 queries of 80..250 nt against
  a  10,000 known sequences of 60..200 nt
  b  38,000 known sequences of 60..200 nt
One query in 10 is a copy of a known sequence with substitutions or with indels.  Each case runs once to load the code objects and then --repeats
times in the same context; the later calls are reported: median, smallest and largest of the wall time and of each stage (upload, scoring, filter
+ sort + cut, traceback, download) and the cells per second of the scoring stage.  --numpy-queries N times the tests' restatement
(tests/test_hairpins_cpu.restate) on the first N queries against the same known sequences, for context."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = {"a": 10000, "b": 38000}
STAGES = ("upload", "scoring", "filter_sort_cut", "traceback", "download")


def make_inputs(n_known, n_queries=500, seed=1):
    rng = np.random.RandomState(seed)
    acgu = np.frombuffer(b"ACGU", dtype=np.uint8)

    def seq(n):
        return acgu[rng.randint(0, 4, size=int(n))].tobytes()
    known = [seq(L) for L in rng.randint(60, 201, size=n_known)]
    queries = [seq(L) for L in rng.randint(80, 251, size=n_queries)]
    for q in range(0, n_queries, 10):
        s = bytearray(known[rng.randint(0, n_known)])
        if (q // 10) % 2:
            for _ in range(max(1, len(s) // 12)):
                s[rng.randint(0, len(s))] = acgu[rng.randint(0, 4)]
        else:
            for _ in range(rng.randint(1, 4)):
                at, g = rng.randint(1, len(s) - 7), rng.randint(1, 7)
                s = s[:at] + (bytearray(seq(g)) if rng.randint(0, 2) else bytearray()) + s[at + (g if rng.randint(0, 2) else 0):]
        queries[q] = bytes(s)
    return queries, known


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "hairpins_time", "hairpins_time.json"))
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-queries", type=int, default=0)
    args = ap.parse_args()
    from mir_prefer_amd import capi
    ctx = capi.Context(0)
    result = {"cases": {}}
    try:
        for case in args.cases.split(","):
            queries, known = make_inputs(CASES[case])
            walls, stages = [], []
            for _ in range(1 + args.repeats):
                t = time.time()
                recs, cigars = ctx.hairpin_align(queries, known)
                walls.append(time.time() - t)
                stages.append(ctx.hairpin_last_stats())
            st = stages[-1]
            row = {"queries": len(queries), "known": len(known), "cells": st["cells"], "hits": st["hits"], "score_passes": st["score_passes"],
                   "trace_passes": st["trace_passes"], "first_wall_s": walls[0], "wall_s": spread(walls[1:]),
                   "stage_s": {name: spread([s["seconds"][x] for s in stages[1:]]) for x, name in enumerate(STAGES)},
                   "scoring_cells_per_s": spread([s["cells"] / s["seconds"][1] for s in stages[1:]])}
            if args.numpy_queries > 0:
                from tests.test_hairpins_cpu import restate
                n = min(args.numpy_queries, len(queries))
                t = time.time()
                hits, per = restate(queries[:n], known)
                dt = time.time() - t
                want = [(h["query"], h["known"], h["score"], h["cigar"]) for h in hits]
                got = [(int(r["query"]), int(r["known"]), int(r["score"]), c) for r, c in zip(recs, cigars) if r["query"] < n]
                assert got == want, "the device and the restatement differ"
                row["numpy"] = {"queries": n, "seconds": dt, "cells_per_s": sum(len(q) for q in queries[:n]) * sum(len(k) for k in known) / dt}
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
