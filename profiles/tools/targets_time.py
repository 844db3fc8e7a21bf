#!/usr/bin/env python3
"""Timing of the plant miRNA target-site search (mirp_target_scan) on seeded inputs.

    python profiles/tools/targets_time.py [--dir /tmp/targets_time] [--out build/targets_time/targets_time.json] [--cases a,b,c]
                                          [--kernel-stats kernel_stats.csv] [--valu-per-eval 23]

Cases (the issue's three):
  a  1,000 21-nt miRNAs x a 70 Mb transcriptome (35,000 transcripts of 1-3 kb), plus strand, -s 4
  b  the same miRNAs x a 120 Mb genome (6 chromosomes with N runs), -b, -s 4
  c  50,000 21-nt miRNAs x the 70 Mb transcriptome, plus strand, -s 4
Each case runs twice in one context (the first loads the code objects); the second is reported with its phases.  The rate is evaluations
(target offsets x miRNAs x strands) over the scan phase (host clock around the scan launches and their synchronise).  Kernel times come from a run of
its own under `rocprofv3 --kernel-trace --stats`; --kernel-stats reads that CSV and gives the scan kernels' evaluations per second of kernel time
against the VALU issue bound: 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz over the VALU instructions one evaluation issues (--valu-per-eval,
counted in the ISA of tg_scan_kernel)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LANE_OPS = 256 * 4 * 32 * 2.4e9        # VALU lane-operations per second


def write_fasta(path, records, width=80):
    with open(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + name + b"\n")
            s = np.frombuffer(seq, dtype=np.uint8)
            n = len(s) // width * width
            body = np.concatenate([s[:n].reshape(-1, width), np.full((len(s) // width, 1), 10, np.uint8)], axis=1).tobytes()
            f.write(body + (seq[n:] + b"\n" if n < len(s) else b""))


def make_inputs(d, seed=1):
    os.makedirs(d, exist_ok=True)
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    paths = {"tx": os.path.join(d, "transcripts_70M.fa"), "genome": os.path.join(d, "genome_120M.fa"), "m1k": os.path.join(d, "mirna_1k.fa"),
             "m50k": os.path.join(d, "mirna_50k.fa")}
    mir = acgt[rng.randint(0, 4, size=(50000, 21))]
    mir_txt = np.where(mir == ord("T"), ord("U"), mir).astype(np.uint8)
    if not os.path.exists(paths["tx"]):
        lens = rng.randint(1000, 3001, size=35000)
        lens = (lens * (70_000_000 / lens.sum())).astype(np.int64)
        seq = acgt[rng.randint(0, 4, size=int(lens.sum()))]
        # plant a perfect site of each of the first 1,000 miRNAs (reverse complement) in the transcripts
        comp = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
        for i, o in enumerate(rng.choice(len(seq) // 100 - 1, size=1000, replace=False) * 100):
            seq[o:o + 21] = np.array([comp[c] for c in mir[i][::-1]], np.uint8)
        off = np.concatenate([[0], np.cumsum(lens)])
        write_fasta(paths["tx"], [(b"tx%05d" % i, seq[off[i]:off[i + 1]].tobytes()) for i in range(len(lens))])
    if not os.path.exists(paths["genome"]):
        recs = []
        for c in range(6):
            s = acgt[rng.randint(0, 4, size=20_000_000)]
            for _ in range(20):
                a = int(rng.randint(0, len(s) - 50000))
                s[a:a + int(rng.randint(100, 50000))] = ord("N")
            recs.append((b"chr%d" % (c + 1), s.tobytes()))
        write_fasta(paths["genome"], recs)
    for key, n in (("m1k", 1000), ("m50k", 50000)):
        if not os.path.exists(paths[key]):
            with open(paths[key], "wb") as f:
                f.write(b"".join(b">mir%05d\n%s\n" % (i, mir_txt[i].tobytes()) for i in range(n)))
    return paths


CASES = {"a": ("m1k", ["tx"], False), "b": ("m1k", ["genome"], True), "c": ("m50k", ["tx"], False)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default="/tmp/targets_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "targets_time", "targets_time.json"))
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: kernel-time rates")
    ap.add_argument("--valu-per-eval", type=float, default=23.0)
    args = ap.parse_args()
    result = {"valu_issue_bound_lane_ops_per_s": LANE_OPS, "valu_per_eval": args.valu_per_eval,
              "valu_bound_evals_per_s": LANE_OPS / args.valu_per_eval, "cases": {}}
    if args.kernel_stats:
        evals = 0
        prev = args.out if os.path.exists(args.out) else None
        if prev:
            evals = sum(c["evaluations"] * 2 for c in json.load(open(prev))["cases"].values())     # every case ran twice
        scan_ns = 0.0
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "tg_scan_kernel" in row["Name"]:
                    scan_ns += float(row["TotalDurationNs"])
        result["kernel_stats"] = {"scan_kernel_s": scan_ns * 1e-9, "evaluations": evals,
                                  "evals_per_s_kernel": evals / (scan_ns * 1e-9) if scan_ns and evals else None}
        if result["kernel_stats"]["evals_per_s_kernel"]:
            result["kernel_stats"]["share_of_valu_bound"] = result["kernel_stats"]["evals_per_s_kernel"] / result["valu_bound_evals_per_s"]
        print(json.dumps(result["kernel_stats"], indent=1))
        out = args.out.replace(".json", "_kernels.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        json.dump(result, open(out, "w"), indent=1)
        return 0
    from mir_prefer_amd import capi
    t0 = time.time()
    paths = make_inputs(args.dir)
    print("inputs ready in %.1f s" % (time.time() - t0), flush=True)
    ctx = capi.Context(0)
    try:
        for case in args.cases.split(","):
            mk, tk, both = CASES[case]
            out = os.path.join(args.dir, "case_%s.tsv" % case)
            runs = []
            for _ in range(2):
                t = time.time()
                res = ctx.target_scan(paths[mk], [paths[k] for k in tk], out, max_half_score=8, both_strands=both)
                res["wall_s"] = time.time() - t
                runs.append(res)
            r = runs[1]
            sec = dict(zip(("parse", "upload", "scan", "sort_cut", "emit_write"), r["seconds"]))
            row = {"mirnas": r["mirnas"], "targets": r["targets"], "bases": r["bases"], "strands": 2 if both else 1, "evaluations": r["evaluations"],
                   "sites": r["sites"], "passes": r["passes"], "wall_s": r["wall_s"], "first_wall_s": runs[0]["wall_s"], "seconds": sec,
                   "evals_per_s_scan_phase": r["evaluations"] / sec["scan"] if sec["scan"] > 0 else None}
            row["share_of_valu_bound"] = row["evals_per_s_scan_phase"] / result["valu_bound_evals_per_s"] if row["evals_per_s_scan_phase"] else None
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
