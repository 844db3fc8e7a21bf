#!/usr/bin/env python3
"""Timing of the two-strand fold (mirp_duplex_batch) and of `targets -e` on seeded inputs.

    python profiles/tools/duplex_time.py [--pairs 1000000] [--repeat 3] [--dir /tmp/targets_time] [--cases a,b,c] [--skip-targets]
                                         [--out build/duplex_time/duplex_time.json] [--kernel-stats kernel_stats.csv]

Part 1: `--pairs` random 21 x 23 strand pairs and as many near-complement pairs (the reverse complement of a with up to three substituted,
inserted or deleted bases and a flank on each side, 23 nt) through capi.Context.duplex_batch: one warm-up call, then --repeat calls of each kind,
alternating.  Reported per kind: duplexes per second and loop evaluations per second (mirp_duplex_last_stats) over the whole call (host clock:
coding, upload, kernel, download, records), lowest and highest of the repeats.
Part 2: the three cases of profiles/tools/targets_time.py (§14) without and with -e, alternating in this one process after a warm-up run of
each: the phases of `seconds` and, per case, the ratio of the -e run's total and "sort + cut" phase to the plain run's.
Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`; --kernel-stats reads that CSV and the JSON this tool wrote and
gives duplexes and loop evaluations per second of duplex_kernel time."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_pairs(n, seed=1):
    """-> (random a, random b, near-complement b) as lists of bytes; a 21 nt, b 23 nt"""
    rng = np.random.RandomState(seed)
    acgu = np.frombuffer(b"ACGU", dtype=np.uint8)
    a = rng.randint(0, 4, size=(n, 21))
    b = rng.randint(0, 4, size=(n, 23))
    near = np.empty((n, 23), dtype=np.int64)
    near[:, 1:22] = (3 - a)[:, ::-1]
    near[:, 0] = rng.randint(0, 4, n)
    near[:, 22] = rng.randint(0, 4, n)
    rows = np.arange(n)
    for _ in range(3):                                       # up to three edits: a substitution, or a shift of the tail (an insertion / a deletion)
        kind, at = rng.randint(0, 4, n), rng.randint(2, 21, n)
        sub = kind == 1
        near[rows[sub], at[sub]] = rng.randint(0, 4, int(sub.sum()))
        for q in rows[kind == 2]:
            near[q, at[q] + 1:] = near[q, at[q]:-1]
            near[q, at[q]] = rng.randint(0, 4)
        for q in rows[kind == 3]:
            near[q, at[q]:-1] = near[q, at[q] + 1:]
            near[q, -1] = rng.randint(0, 4)
    return ([x.tobytes() for x in acgu[a]], [x.tobytes() for x in acgu[b]], [x.tobytes() for x in acgu[near]])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/targets_time")
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--skip-targets", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "duplex_time", "duplex_time.json"))
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: kernel-time rates")
    args = ap.parse_args()
    if args.kernel_stats:
        done = json.load(open(args.out))
        ns = 0.0
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "duplex_kernel<mirp::DxPairs>" in row["Name"]:
                    ns += float(row["TotalDurationNs"])
        calls = 1 + 2 * len(done["batch"]["random"]["wall_s_runs"])
        n = done["batch"]["pairs"]
        ev = done["batch"]["warm_up_evaluations"] + sum(done["batch"][k]["evaluations"] * len(done["batch"][k]["wall_s_runs"]) for k in ("random", "near"))
        ks = {"duplex_kernel_s": ns * 1e-9, "duplexes": n * calls, "evaluations": ev,
              "duplexes_per_s_kernel": n * calls / (ns * 1e-9) if ns else None, "evaluations_per_s_kernel": ev / (ns * 1e-9) if ns else None}
        print(json.dumps(ks, indent=1))
        json.dump(ks, open(args.out.replace(".json", "_kernels.json"), "w"), indent=1)
        return 0
    from mir_prefer_amd import capi
    result = {"batch": {"pairs": args.pairs}, "targets": {}}
    a, b, near = make_pairs(args.pairs)
    ctx = capi.Context(0)
    try:
        ctx.duplex_batch(a, b, structures=False)             # loads the code object
        result["batch"]["warm_up_evaluations"] = ctx.duplex_last_stats()["evaluations"]
        runs = {"random": [], "near": []}
        for _ in range(max(1, args.repeat)):
            for kind, bb in (("random", b), ("near", near)):
                t = time.time()
                recs, _ = ctx.duplex_batch(a, bb, structures=False)
                runs[kind].append((time.time() - t, ctx.duplex_last_stats(), int((recs["mfe"] < 0).sum()), float(recs["mfe"].mean()) / 100.0))
        for kind, rs in runs.items():
            walls = [r[0] for r in rs]
            ev = rs[0][1]["evaluations"]
            result["batch"][kind] = {"wall_s_runs": walls, "evaluations": ev, "passes": rs[0][1]["passes"], "bound": rs[0][2], "mean_mfe_kcal": rs[0][3],
                                     "duplexes_per_s": [args.pairs / max(walls), args.pairs / min(walls)],
                                     "evaluations_per_s": [ev / max(walls), ev / min(walls)]}
            print(kind, json.dumps(result["batch"][kind]), flush=True)
        if not args.skip_targets:
            import targets_time
            t0 = time.time()
            paths = targets_time.make_inputs(args.dir)
            print("inputs ready in %.1f s" % (time.time() - t0), flush=True)
            for case in args.cases.split(","):
                mk, tk, both = targets_time.CASES[case]
                out = os.path.join(args.dir, "case_%s_energy.tsv" % case)
                runs = {False: [], True: []}
                for _ in range(1 + max(1, args.repeat)):
                    for e in (False, True):
                        t = time.time()
                        res = ctx.target_scan(paths[mk], [paths[k] for k in tk], out, max_half_score=8, both_strands=both, energy=e)
                        res["wall_s"] = time.time() - t
                        runs[e].append(res)
                row = {}
                for e, name in ((False, "plain"), (True, "energy")):
                    rs = runs[e][1:]
                    row[name] = {"sites": rs[0]["sites"], "passes": rs[0]["passes"], "evaluations": rs[0]["evaluations"],
                                 "seconds_runs": [dict(zip(("parse", "upload", "scan", "sort_cut", "emit_write"), r["seconds"])) for r in rs],
                                 "total_s_runs": [sum(r["seconds"]) for r in rs], "wall_s_runs": [r["wall_s"] for r in rs]}
                lo = {name: (min(row[name]["total_s_runs"]), min(s["sort_cut"] for s in row[name]["seconds_runs"])) for name in row}
                row["energy_over_plain_total"] = lo["energy"][0] / lo["plain"][0]
                row["energy_over_plain_sort_cut"] = lo["energy"][1] / lo["plain"][1] if lo["plain"][1] > 0 else None
                result["targets"][case] = row
                print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
