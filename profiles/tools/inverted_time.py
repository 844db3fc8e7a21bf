"""Times the inverted-repeat search (mirp_inverted_scan) on a synthetic genome.

    python profiles/tools/inverted_time.py [--out build/inverted_time/inverted_time.json] [--mb 120] [--span 2000] [--slice 50000]

Input: the genome shape of phasing_time.py, six contigs of --mb / 6 Mb of uniform random letters (seeded), with --planted repeats (arms 20..300,
loops 0..600, about 3 % substitutions) and 0.5 % of the bases in microsatellites of unit 1..6 and 30..300 nt.  One warm-up call, then three.
Reports the seconds of every stage, the scan's cells per second against its own vector-issue bound (7.86e13 lane-instructions per second over the
instructions per cell named in DESIGN.md §30), the numpy restatement's cells per second on the first --slice bases of the same genome, and the
counts of candidates, traced and dropped candidates and accepted repeats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ISSUE_RATE = 7.86e13          # lane-instructions per second of the device
INSTRUCTIONS_PER_CELL = 8.08  # vector instructions per cell of an unchecked block of iv_scan_kernel: 2,068 in 16 levels x 16 rows


def make_genome(mb, planted, seed=30):
    rng = np.random.RandomState(seed)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    n = int(mb * 1e6) // 6
    contigs = []
    for k in range(6):
        g = letters[rng.randint(0, 4, n)]
        for _ in range(planted // 6):
            arm, loop = int(rng.randint(20, 301)), int(rng.randint(0, 601))
            pos = int(rng.randint(0, n - 2 * arm - loop))
            right = comp[g[pos:pos + arm][::-1]].copy()
            hit = rng.random_sample(arm) < 0.03
            right[hit] = letters[rng.randint(0, 4, int(hit.sum()))]
            g[pos + arm + loop:pos + 2 * arm + loop] = right
        budget = n // 200
        while budget > 0:
            unit, length = letters[rng.randint(0, 4, int(rng.randint(1, 7)))], int(rng.randint(30, 301))
            pos = int(rng.randint(0, n - length))
            g[pos:pos + length] = np.resize(unit, length)
            budget -= length
        contigs.append(g.tobytes())
    return contigs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "inverted_time", "inverted_time.json"))
    ap.add_argument("--mb", type=float, default=120)
    ap.add_argument("--planted", type=int, default=3000)
    ap.add_argument("--span", type=int, default=2000)
    ap.add_argument("--slice", type=int, default=50000)
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    from mir_prefer_amd import capi
    t = time.time()
    contigs = make_genome(args.mb, args.planted)
    result = {"mb": args.mb, "span": args.span, "planted": args.planted, "make_genome_s": round(time.time() - t, 2), "runs": []}
    ctx = capi.Context(0)
    try:
        for run in range(4):
            t = time.time()
            recs, _ = ctx.inverted_scan(contigs, max_span=args.span)
            wall = time.time() - t
            st = ctx.inverted_last_stats()
            rate = st["cells"] / st["seconds"][1]
            entry = dict(st, wall_s=wall, warm_up=run == 0, scan_cells_per_s=rate, scan_fraction_of_issue_bound=rate / (ISSUE_RATE / INSTRUCTIONS_PER_CELL),
                         records=len(recs))
            result["runs"].append(entry)
            print(json.dumps(entry), flush=True)
    finally:
        ctx.close()
    result["issue_bound_cells_per_s"] = ISSUE_RATE / INSTRUCTIONS_PER_CELL
    if not args.skip_restatement:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import inverted_restatement as R
        s = R.letters(contigs[0][:args.slice])
        t = time.time()
        R.h_levels(s, args.span, 3, 4, 12)
        dt = time.time() - t
        cells = sum(min(args.span - 1, len(s) - i) for i in range(1, len(s) + 1))
        result["restatement"] = {"bases": len(s), "cells": cells, "seconds": dt, "cells_per_s": cells / dt}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result.get("restatement", {})))


if __name__ == "__main__":
    main()
