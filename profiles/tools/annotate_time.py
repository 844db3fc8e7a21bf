#!/usr/bin/env python3
"""Timing of the known-miRNA annotation (mirp_annotate_scan) on seeded inputs.

    python profiles/tools/annotate_time.py [--dir /tmp/annotate_time] [--out build/annotate_time/annotate_time.json] [--cases a,b,c]
                                           [--repeats 5] [--valu-per-eval 31.6] [--numpy-queries 20] [--kernel-stats kernel_stats.csv]

Cases (the issue's three), each against 50,000 known sequences of 18..24 nt, -e 2 -m 2:
  a  300 queries (a pipeline's mature.fa)
  b  10^5 queries (a small collapsed library)
  c  10^6 queries (a collapsed library)
One query in 50 is a copy, a shifted copy or a 1-2-substitution copy of a known sequence; the rest are random.  Each case runs once to load the
code objects and then --repeats times in the same context; the calls after the first are reported: median, smallest and largest of the wall time
and of the counting scan (host clock around the launch and its synchronise).  The rate is evaluations (pairs x shifts with both offsets within
-e) over the counting scan, which visits every pair once; the key scans repeat the work for the query ranges that hold hits and are listed with
their own seconds.  The VALU issue bound is 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz over the VALU instructions one evaluation issues
(--valu-per-eval, counted in the ISA of an_scan_kernel, DESIGN.md §19: 16 per shift and 7 per pair, all 5 shifts run for every pair and 2.76 of
them are evaluations at these lengths, hence 31.6).  --numpy-queries N also times the tests' numpy restatement on N queries
of case a on this machine's CPUs, for context.  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`; --kernel-stats
reads that CSV and sums the an_scan_kernel rows."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LANE_OPS = 256 * 4 * 32 * 2.4e9        # VALU lane-operations per second
CASES = {"a": 300, "b": 100_000, "c": 1_000_000}
N_KNOWN = 50_000


def random_records(rng, n, prefix):
    """n random sequences of 18..24 nt as one [n, 24] letter matrix and their lengths"""
    acgu = np.frombuffer(b"ACGU", dtype=np.uint8)
    return acgu[rng.randint(0, 4, size=(n, 24))], rng.randint(18, 25, size=n)


def write_records(path, prefix, letters, lens):
    with open(path, "wb") as f:
        f.write(b"".join(b">%s%d\n%s\n" % (prefix, i, letters[i, :lens[i]].tobytes()) for i in range(len(lens))))


def make_inputs(d, cases, seed=1):
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(seed)
    paths = {"known": os.path.join(d, "known_50k.fa")}
    kl, kn = random_records(rng, N_KNOWN, b"k")
    if not os.path.exists(paths["known"]):
        write_records(paths["known"], b"ath-miR", kl, kn)
    for case in cases:
        n = CASES[case]
        paths[case] = os.path.join(d, "query_%s.fa" % case)
        ql, qn = random_records(np.random.RandomState(seed + 1 + ord(case)), n, b"q")
        r2 = np.random.RandomState(seed + 100 + ord(case))
        for i in range(0, n, 50):                    # relatives of known sequences
            k = int(r2.randint(0, N_KNOWN))
            s, L = kl[k].copy(), int(kn[k])
            kind = (i // 50) % 3
            if kind == 1:
                s[:L - 1] = s[1:L]
            elif kind == 2:
                for p in r2.randint(0, L, size=1 + (i // 150) % 2):
                    s[p] = b"ACGU"[(b"ACGU".index(bytes([s[p]])) + 1) % 4]
            ql[i], qn[i] = s, L
        if not os.path.exists(paths[case]):
            write_records(paths[case], b"read_", ql, qn)
    return paths


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default="/tmp/annotate_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "annotate_time", "annotate_time.json"))
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--valu-per-eval", type=float, default=31.6)
    ap.add_argument("--numpy-queries", type=int, default=0)
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: the scan kernels' time")
    args = ap.parse_args()
    result = {"valu_issue_bound_lane_ops_per_s": LANE_OPS, "valu_per_eval": args.valu_per_eval, "valu_bound_evals_per_s": LANE_OPS / args.valu_per_eval,
              "cases": {}}
    if args.kernel_stats:
        scan_ns = 0.0
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "an_scan_kernel" in row["Name"]:
                    scan_ns += float(row["TotalDurationNs"])
        print(json.dumps({"scan_kernel_s": scan_ns * 1e-9}))
        return 0
    cases = args.cases.split(",")
    t0 = time.time()
    paths = make_inputs(args.dir, cases)
    print("inputs ready in %.1f s" % (time.time() - t0), flush=True)
    if args.numpy_queries:
        from tests.test_annotate_cpu import KnownMatrix, hits_numpy, parse_known
        from tests.test_targets_cpu import parse_mirnas
        known, _ = parse_known([open(paths["known"], "rb").read()])
        queries = parse_mirnas(open(paths[cases[0]], "rb").read())[:args.numpy_queries]
        K = KnownMatrix(known)
        lens = np.array([len(c) for _, c in known])
        evals = sum(int(np.maximum(0, 5 - np.abs(lens - len(q))).sum()) for _, q in queries)
        t = time.time()
        for _, q in queries:
            hits_numpy(q, K, 2, 2)
        dt = time.time() - t
        result["numpy"] = {"queries": len(queries), "evaluations": evals, "seconds": dt, "evals_per_s": evals / dt}
        print("numpy", json.dumps(result["numpy"]), flush=True)
    from mir_prefer_amd import capi
    ctx = capi.Context(0)
    try:
        for case in cases:
            out = os.path.join(args.dir, "case_%s.annot.tsv" % case)
            runs = []
            for _ in range(1 + args.repeats):
                t = time.time()
                res = ctx.annotate_scan(paths[case], [paths["known"]], out, out[:-4] + ".summary.tsv")
                res["wall_s"] = time.time() - t
                runs.append(res)
            r = runs[1]
            later = runs[1:]
            names = ("parse", "upload", "count_scan", "key_scans", "sort_cut", "download_write")
            row = {x: r[x] for x in r if x != "seconds"}
            row.update(first_wall_s=runs[0]["wall_s"], wall_s=spread([x["wall_s"] for x in later]),
                       seconds={n: spread([x["seconds"][i] for x in later]) for i, n in enumerate(names)})
            cs = row["seconds"]["count_scan"]["median"]
            row["evals_per_s_count_scan"] = r["evaluations"] / cs if cs > 0 else None
            row["share_of_valu_bound"] = row["evals_per_s_count_scan"] / result["valu_bound_evals_per_s"] if cs > 0 else None
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
