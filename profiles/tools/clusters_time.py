#!/usr/bin/env python3
"""Timing of the small-RNA clusters (mirp_cluster_scan) on the input of phasing_time.py.

    python profiles/tools/clusters_time.py [--dir /tmp/phasing_time] [--out build/clusters_time/clusters_time.json] [--records 10000000]
                                           [--kernel-stats kernel_stats.csv] [--skip-restatement]

Input: the two SAM files of phasing_time.py (about 10 M records against a 120 Mb genome of six 20 Mb contigs; written there if missing).  One
context ingests them once per round and runs the cluster scan at the default -m 0.5rpm --pad 75 and at -m 20 --pad 75; of two rounds the second
is reported: the ingest, the mirp_cluster_scan call (wall), the host write of the three files (calls included), and the numpy restatement of the
clusters (tests/test_clusters_cpu.py) on the same records.  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`;
--kernel-stats reads that CSV and gives the cluster kernels' time per scan: the cl_* kernels and the (hash-record) radix sort are the scan's
alone, the int32 scans are shared with the ingest's sort and are listed apart."""
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
SETTINGS = (("0.5rpm", 75), ("20", 75))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default="/tmp/phasing_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "clusters_time", "clusters_time.json"))
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: kernel time per scan")
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    if args.kernel_stats:
        n_scans = 2 * len(SETTINGS)
        own, scans = {}, {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                base = name.split("(")[0].split("<")[0].split("::")[-1]
                t = float(row["TotalDurationNs"]) * 1e-9
                if base.startswith("cl_") or (base.startswith("sort_") and "MirpHashRec" in name):
                    own[name] = t
                elif base.startswith("excl_scan"):
                    scans[name] = t
        res = {"cluster_kernels_s": own, "per_scan_s": sum(own.values()) / n_scans, "shared_scan_kernels_s": scans,
               "shared_scan_per_scan_upper_bound_s": sum(scans.values()) / n_scans}
        print(json.dumps(res, indent=1))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(res, open(args.out.replace(".json", "_kernels.json"), "w"), indent=1)
        return 0
    from mir_prefer_amd import capi, clusters
    from phasing_time import make_records, write_sams
    os.makedirs(args.dir, exist_ok=True)
    t0 = time.time()
    paths = write_sams(args.dir, make_records(args.records))
    print("inputs ready in %.1f s: %d bytes of SAM" % (time.time() - t0, sum(os.path.getsize(p) for p in paths)), flush=True)
    result = {"scans": {}}
    ctx = capi.Context(0)
    try:
        for rnd in range(2):
            t = time.time()
            names, lens, samples, alns, _, sec = ctx.ingest_sams(paths)
            ingest = {"wall_s": time.time() - t, "tokenize_s": sec["tokenize_s"], "upload_filter_s": sec["upload_filter_s"], "sort_s": sec["sort_s"],
                      "download_s": sec["download_s"]}
            total = int(alns["depth"].sum(dtype=np.uint64))
            for m, pad in SETTINGS:
                T = clusters.threshold(clusters.parse_min_coverage(m), total)
                t = time.time()
                got, counts, st = ctx.cluster_scan(T, pad, lens, len(paths))
                t_scan = time.time() - t
                t = time.time()
                files = clusters.format_files(names, got, counts, list(samples))
                for p, body in zip(clusters.output_paths(os.path.join(args.dir, "m%s" % m)), files):
                    with open(p, "wb") as f:
                        f.write(body)
                t_host = time.time() - t
                if rnd == 1:
                    result["scans"][m] = dict(st, T=T, pad=pad, scan_s=t_scan, host_write_s=t_host, records_per_s_scan_call=st["records"] / t_scan)
                    print(m, json.dumps(result["scans"][m]), flush=True)
            if rnd == 1:
                result["records"] = int(len(alns))
                result["ingest"] = ingest
                print("ingest", json.dumps(ingest), flush=True)
    finally:
        ctx.close()
    if not args.skip_restatement:
        from tests.test_clusters_cpu import clusters_numpy
        m, pad = SETTINGS[0]
        sc = result["scans"][m]
        t = time.time()
        want, _, st = clusters_numpy(alns, lens, len(paths), sc["T"], pad)
        result["numpy_restatement_s"] = time.time() - t
        assert st["clusters"] == sc["clusters"] and st["assigned"] == sc["assigned"]
        print("numpy restatement: %.2f s" % result["numpy_restatement_s"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
