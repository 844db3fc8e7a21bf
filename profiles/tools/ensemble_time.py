#!/usr/bin/env python3
"""Timing of the partition function of precursors (mirp_ensemble) on seeded inputs.

    python profiles/tools/ensemble_time.py [--out build/ensemble_time/ensemble_time.json] [--cases a,b] [--repeats 3] [--pairs]

Cases, random sequences, seed 1:
  a  500 precursors of 80..250 nt
  b  20 sequences of 1000 nt
Each case runs once to load the code objects and then --repeats times in the same context; the later calls are reported: median, smallest and
largest of the wall time and the sequences per second of the whole call (the MFE fold, the inside and outside kernels, the reduction, the
download; with --pairs also the pair list at the cutoff 0.001).  The yardstick is the MFE fold the library already had: alternating with those
calls, in the same process, fold_batch_summary folds the very same bytes with one structure line of capacity; `ratio` is the ensemble wall time
over that.  The kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` (a run of its own)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = {"a": (500, 80, 250), "b": (20, 1000, 1000)}


def make_sequences(n, lo, hi, seed=1):
    rng = np.random.RandomState(seed)
    acgu = np.frombuffer(b"ACGU", dtype=np.uint8)
    return [acgu[rng.randint(0, 4, size=int(L))].tobytes() for L in rng.randint(lo, hi + 1, size=n)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ensemble_time", "ensemble_time.json"))
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", action="store_true")
    args = ap.parse_args()
    from mir_prefer_amd import capi
    ctx = capi.Context(0)
    result = {"pairs": args.pairs, "cases": {}}
    try:
        for case in args.cases.split(","):
            n, lo, hi = CASES[case]
            seqs = make_sequences(n, lo, hi)
            blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
            offs = np.zeros(n + 1, dtype=np.int64)
            np.cumsum([len(s) for s in seqs], out=offs[1:])
            walls, base = [], []
            for _ in range(1 + args.repeats):
                t = time.time()
                recs, cens, bpp = ctx.ensemble(seqs, bpp_cutoff=0.001 if args.pairs else None)
                walls.append(time.time() - t)
                t = time.time()
                mfes = ctx.fold_batch_summary(blob, offs, max(300, hi), max_lines=1)[1]
                base.append(time.time() - t)
            assert (recs["mfe"] == np.asarray(mfes)).all() and (recs["efe"] * 100 <= recs["mfe"] + 1e-6).all()
            stats = ctx.ensemble_last_stats()
            row = {"sequences": n, "letters": int(offs[-1]), "cells": stats["cells"], "passes": stats["passes"], "first_wall_s": walls[0],
                   "wall_s": spread(walls[1:]), "sequences_per_s": spread([n / w for w in walls[1:]]), "cells_per_s": spread([stats["cells"] / w for w in walls[1:]]),
                   "fold_batch_summary_s": spread(base[1:]), "ratio": spread([w / b for w, b in zip(walls[1:], base[1:])]),
                   "pairs_listed": None if bpp is None else int(len(bpp))}
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
