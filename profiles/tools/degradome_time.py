#!/usr/bin/env python3
"""Timing of the degradome cleavage scan (mirp_degradome_scan) on seeded inputs.

    python profiles/tools/degradome_time.py [--dir /tmp/degradome_time] [--out build/degradome_time/degradome_time.json] [--cases a,c]
                                            [--kernel-stats kernel_stats.csv] [--valu-per-eval 24]

Inputs: a 70 Mb transcriptome of 35,000 transcripts (1-3 kb), 50,000 random 21-nt miRNAs of which the first 1,000 are planted once each, and a
degradome of 10 M sense records over about 5 M units (random positions with geometric depths, two records per unit) with a peak of depth 1,000 on
each planted site's cleavage position.  The records are loaded with load_alignments (the SAM ingest is timed by bench.py --full, not here).
Cases:
  a  the first 1,000 miRNAs, -s 4
  c  all 50,000 miRNAs, -s 4
Each case runs twice in one context (the first loads the code objects); the second is reported with its phases.  Rates: the counting scan in
evaluations (transcript offsets x miRNAs) over its phase, next to mirp_target_scan's scan phase on the same files in the same session (the same
kernel); the anchored scan in evaluations (kept units x miRNAs) over its counting phase, against the VALU issue bound 256 CUs x 4 SIMDs x 32 lanes
x 2.4 GHz over the VALU instructions one evaluation issues (--valu-per-eval, counted in the ISA of dg_scan_kernel).  Kernel times come from a run
of its own under `rocprofv3 --kernel-trace --stats`; --kernel-stats reads that CSV."""
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
LANE_OPS = 256 * 4 * 32 * 2.4e9        # VALU lane-operations per second
N_TX = 35000


def make_inputs(d, seed=1):
    from targets_time import write_fasta
    from mir_prefer_amd.synth import ALN_DTYPE
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    paths = {"tx": os.path.join(d, "transcripts_70M.fa"), "m1k": os.path.join(d, "mirna_1k.fa"), "m50k": os.path.join(d, "mirna_50k.fa")}
    mir = acgt[rng.randint(0, 4, size=(50000, 21))]
    mir_txt = np.where(mir == ord("T"), ord("U"), mir).astype(np.uint8)
    lens = rng.randint(1000, 3001, size=N_TX)
    lens = (lens * (70_000_000 / lens.sum())).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    seq = acgt[rng.randint(0, 4, size=int(lens.sum()))]
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    peaks = []
    for i in range(1000):                       # miRNA i: a perfect site at offset 100 of transcript 35 i; cleavage position o + L - 9 (1-based)
        t = 35 * i
        seq[off[t] + 100:off[t] + 121] = comp[mir[i][::-1]]
        peaks.append((t, 100 + 21 - 9))
    if not os.path.exists(paths["tx"]):
        write_fasta(paths["tx"], [(b"tx%05d" % i, seq[off[i]:off[i + 1]].tobytes()) for i in range(N_TX)])
    for key, n in (("m1k", 1000), ("m50k", 50000)):
        if not os.path.exists(paths[key]):
            with open(paths[key], "wb") as f:
                f.write(b"".join(b">mir%05d\n%s\n" % (i, mir_txt[i].tobytes()) for i in range(n)))
    g = rng.randint(0, int(lens.sum()), size=5_200_000)
    tid = np.searchsorted(off, g, side="right") - 1
    recs = np.zeros(2 * len(g) + len(peaks), ALN_DTYPE)
    recs["tid"][:2 * len(g)] = np.repeat(tid, 2)
    recs["pos"][:2 * len(g)] = np.repeat(g - off[tid] + 1, 2)
    recs["depth"][:2 * len(g)] = np.minimum(rng.geometric(0.4, 2 * len(g)), 500)
    for k, (t, p) in enumerate(peaks):
        recs[2 * len(g) + k] = (t, p, 1000, 20, 0, 0)
    recs["len"] = 20
    recs = recs[np.lexsort((recs["pos"], recs["tid"]))]
    return paths, ["tx%05d" % i for i in range(N_TX)], lens, recs


CASES = {"a": "m1k", "c": "m50k"}
PHASES = ("parse", "upload", "units", "site_counts", "anchored_counts", "keys_sort_write")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default="/tmp/degradome_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "degradome_time", "degradome_time.json"))
    ap.add_argument("--cases", default="a,c")
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: kernel times by kernel family")
    ap.add_argument("--valu-per-eval", type=float, default=24.0)
    args = ap.parse_args()
    result = {"valu_per_eval": args.valu_per_eval, "valu_bound_evals_per_s": LANE_OPS / args.valu_per_eval, "cases": {}}
    if args.kernel_stats:
        fam = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                key = next((k for k in ("dg_scan_kernel", "tg_scan_kernel", "dg_", "radix", "scan") if k in name), "other")
                fam[key] = fam.get(key, 0.0) + float(row["TotalDurationNs"]) * 1e-9
        print(json.dumps(fam, indent=1))
        return 0
    from mir_prefer_amd import capi
    t0 = time.time()
    paths, names, lens, recs = make_inputs(args.dir)
    print("inputs ready in %.1f s: %d records" % (time.time() - t0, len(recs)), flush=True)
    ctx = capi.Context(0)
    try:
        ctx.load_genome([(n, np.full(1, 65, np.uint8)) for n in names])
        ctx.load_alignments(recs)
        for case in args.cases.split(","):
            mk = CASES[case]
            out = os.path.join(args.dir, "case_%s.tsv" % case)
            runs = []
            for _ in range(2):
                t = time.time()
                res = ctx.degradome_scan(paths[mk], paths["tx"], out, names, lens, max_half_score=8)
                res["wall_s"] = time.time() - t
                runs.append(res)
            r = runs[1]
            sec = dict(zip(PHASES, r["seconds"]))
            tg = [ctx.target_scan(paths[mk], [paths["tx"]], out + ".targets", max_half_score=8) for _ in range(2)][1]
            row = {"mirnas": r["mirnas"], "bases": r["bases"], "records": r["records"], "units": r["units"],
                   "categories": [r["c%d" % k] for k in range(5)], "evaluations": r["evaluations"], "hits": r["hits"], "passes": r["passes"],
                   "wall_s": r["wall_s"], "first_wall_s": runs[0]["wall_s"], "seconds": sec,
                   "counting_scan_evals_per_s": r["bases"] * r["mirnas"] / sec["site_counts"],
                   "targets_scan_evals_per_s": tg["evaluations"] / tg["seconds"][2], "targets_sites": tg["sites"],
                   "anchored_evals_per_s": r["evaluations"] / sec["anchored_counts"]}
            row["anchored_share_of_valu_bound"] = row["anchored_evals_per_s"] / result["valu_bound_evals_per_s"]
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
