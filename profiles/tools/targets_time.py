#!/usr/bin/env python3
"""Timing of the plant miRNA target-site search (mirp_target_scan) on seeded inputs.

    python profiles/tools/targets_time.py [--dir /tmp/targets_time] [--out build/targets_time/targets_time.json] [--cases a,b,c]
                                          [--bulge] [--repeat N] [--kernel-stats kernel_stats.csv] [--valu-per-eval 23] [--valu-per-eval-bulge 64]

Cases (the issue's three):
  a  1,000 21-nt miRNAs x a 70 Mb transcriptome (35,000 transcripts of 1-3 kb), plus strand, -s 4
  b  the same miRNAs x a 120 Mb genome (6 chromosomes with N runs), -b, -s 4
  c  50,000 21-nt miRNAs x the 70 Mb transcriptome, plus strand, -s 4
Each case runs twice in one context (the first loads the code objects); the second is reported with its phases.  --repeat N reports N runs
after the first instead, with the lowest and highest scan time.  --bulge runs every case without and with bulged sites (target_scan(bulge=True),
tg_bulge_scan_kernel), alternating in the same context, and reports the bulge run next to the plain one with the ratio of their scan times.  The rate is evaluations
(target offsets x miRNAs x strands) over the scan phase (host clock around the scan launches and their synchronise).  Kernel times come from a run of
its own under `rocprofv3 --kernel-trace --stats`; --kernel-stats reads that CSV and gives the scan kernels' evaluations per second of kernel time
against the VALU issue bound: 256 CUs x 4 SIMDs x 32 lanes per cycle x 2.4 GHz over the VALU instructions one evaluation issues (--valu-per-eval,
counted in the ISA of tg_scan_kernel), and the same for tg_bulge_scan_kernel with its own count (--valu-per-eval-bulge), each
kernel on its own."""
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
    ap.add_argument("--valu-per-eval-bulge", type=float, default=64.0, help="VALU instructions per evaluation of tg_bulge_scan_kernel")
    ap.add_argument("--bulge", action="store_true", help="every case without and with bulged sites, alternating")
    ap.add_argument("--repeat", type=int, default=1, help="reported runs per case and mode after the warm-up run")
    args = ap.parse_args()
    result = {"valu_issue_bound_lane_ops_per_s": LANE_OPS, "valu_per_eval": args.valu_per_eval,
              "valu_bound_evals_per_s": LANE_OPS / args.valu_per_eval, "cases": {}}
    if args.kernel_stats:
        # evaluations of every run of the JSON this tool wrote (a JSON without scan_s_runs is from the version that ran every case twice), per kernel
        evals = {"tg_scan_kernel": 0, "tg_bulge_scan_kernel": 0}
        if os.path.exists(args.out):
            for c in json.load(open(args.out))["cases"].values():
                runs = 1 + len(c.get("scan_s_runs", [0]))
                evals["tg_scan_kernel"] += c["evaluations"] * runs
                if "bulge" in c:
                    evals["tg_bulge_scan_kernel"] += c["bulge"]["evaluations"] * runs
        scan_ns = {k: 0.0 for k in evals}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for k in evals:
                    if "::" + k + "<" in row["Name"]:
                        scan_ns[k] += float(row["TotalDurationNs"])
        result["kernel_stats"] = {}
        for k, valu in (("tg_scan_kernel", args.valu_per_eval), ("tg_bulge_scan_kernel", args.valu_per_eval_bulge)):
            if not scan_ns[k]:
                continue
            ks = {"scan_kernel_s": scan_ns[k] * 1e-9, "evaluations": evals[k], "valu_per_eval": valu,
                  "evals_per_s_kernel": evals[k] / (scan_ns[k] * 1e-9) if evals[k] else None}
            if ks["evals_per_s_kernel"]:
                ks["share_of_valu_bound"] = ks["evals_per_s_kernel"] / (LANE_OPS / valu)
            result["kernel_stats"][k] = ks
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
            modes = (False, True) if args.bulge else (False,)
            runs = {b: [] for b in modes}
            for _ in range(1 + max(1, args.repeat)):
                for b in modes:
                    t = time.time()
                    res = ctx.target_scan(paths[mk], [paths[k] for k in tk], out, max_half_score=8, both_strands=both, bulge=b)
                    res["wall_s"] = time.time() - t
                    runs[b].append(res)

            def report(rs):
                r = rs[1]
                sec = dict(zip(("parse", "upload", "scan", "sort_cut", "emit_write"), r["seconds"]))
                row = {"mirnas": r["mirnas"], "targets": r["targets"], "bases": r["bases"], "strands": 2 if both else 1, "evaluations": r["evaluations"],
                       "sites": r["sites"], "passes": r["passes"], "wall_s": r["wall_s"], "first_wall_s": rs[0]["wall_s"], "seconds": sec,
                       "evals_per_s_scan_phase": r["evaluations"] / sec["scan"] if sec["scan"] > 0 else None}
                row["share_of_valu_bound"] = row["evals_per_s_scan_phase"] / result["valu_bound_evals_per_s"] if row["evals_per_s_scan_phase"] else None
                scans = [x["seconds"][2] for x in rs[1:]]
                row["scan_s_runs"], row["scan_s_min"], row["scan_s_max"] = scans, min(scans), max(scans)
                return row
            row = report(runs[False])
            if args.bulge:
                row["bulge"] = report(runs[True])
                row["bulge"]["scan_ratio_to_plain"] = row["bulge"]["scan_s_min"] / row["scan_s_min"] if row["scan_s_min"] > 0 else None
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
