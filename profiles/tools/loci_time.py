#!/usr/bin/env python3
"""Timing of the reads on given loci (mirp_locus_scan) on the input of clusters_time.py.

    python profiles/tools/loci_time.py [--out build/loci_time/loci_time.json] [--records 10000000] [--skip-restatement]

Input: the records of phasing_time.py (about 10 M against a 120 Mb genome of six 20 Mb contigs), loaded as they are (sample = the file that
clusters_time.py would have written them to), so no SAM text is written.  One context runs, twice each and reporting the second round,
  - mirp_cluster_scan at the default -m 0.5rpm --pad 75,
  - mirp_locus_scan with the clusters of that scan as loci (unstranded), and
  - mirp_locus_scan with two loci per contig that span it whole (one without a strand, one on the plus strand, -s).
It then times the numpy statement of the scan (tests/loci_restatement.py) on the same arrays and fails if a device result differs from it.  The
pad is no smaller than the longest record, so the first locus scan must also reproduce the sums of the cluster scan."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "loci_time", "loci_time.json"))
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    from mir_prefer_amd import capi, clusters
    from phasing_time import CONTIG_LEN, N_CONTIGS, make_records
    from tests.loci_restatement import scan_numpy
    t0 = time.time()
    recs = make_records(args.records)
    recs["sample"] = np.arange(len(recs)) % 2
    lens = [CONTIG_LEN] * N_CONTIGS
    total = int(recs["depth"].sum(dtype=np.uint64))
    T = clusters.threshold(clusters.parse_min_coverage("0.5rpm"), total)
    print("inputs ready in %.1f s: %d records, %d reads, T %d" % (time.time() - t0, len(recs), total, T), flush=True)
    wide = np.zeros(2 * N_CONTIGS, capi.LOCUS_DTYPE)
    wide["tid"], wide["strand"], wide["start"], wide["end"] = np.arange(2 * N_CONTIGS) // 2, [2, 0] * N_CONTIGS, 1, CONTIG_LEN
    result = {"records": int(len(recs)), "T": T}
    ctx = capi.Context(0)
    try:
        ctx.load_genome([("chr%d" % (i + 1), np.full(4, 65, np.uint8)) for i in range(N_CONTIGS)])
        ctx.load_alignments(recs)
        for rnd in range(2):
            t = time.time()
            cl, cl_counts, cl_stats = ctx.cluster_scan(T, 75, lens, 2)
            t_cluster = time.time() - t
            arr = np.zeros(len(cl), capi.LOCUS_DTYPE)
            arr["tid"], arr["strand"], arr["start"], arr["end"] = cl["tid"], 2, cl["start"], cl["end"]
            t = time.time()
            got, counts, stats = ctx.locus_scan(arr, lens, 2)
            t_loci = time.time() - t
            slots = ctx.last_jobs_per_slot(5)
            t = time.time()
            wgot, wcounts, wstats = ctx.locus_scan(wide, lens, 2, True)
            t_wide = time.time() - t
            wslots = ctx.last_jobs_per_slot(5)
            t = time.time()
            for q in range(0, len(arr), max(len(arr) // 200, 1)):
                ctx.locus_scan(arr[q:q + 1], lens, 2)
            t_one = (time.time() - t) / len(range(0, len(arr), max(len(arr) // 200, 1)))
        result["cluster_scan"] = dict(cl_stats, wall_s=t_cluster)
        result["locus_scan_on_the_clusters"] = dict(stats, wall_s=t_loci, jobs_per_slot=slots, records_per_s=len(recs) / t_loci)
        result["locus_scan_contig_wide"] = dict(wstats, wall_s=t_wide, jobs_per_slot=wslots, records_per_s=len(recs) / t_wide)
        result["locus_scan_one_locus_wall_s"] = t_one
    finally:
        ctx.close()
    print(json.dumps(result, indent=1), flush=True)
    # the cluster scan's own sums: with pad >= the longest record no record overlaps two clusters, so the two definitions coincide
    assert int(recs["len"].max()) <= 75
    assert got.tobytes() == cl.tobytes() and (counts == cl_counts).all(), "the locus scan on the clusters differs from the cluster scan"
    if not args.skip_restatement:
        t = time.time()
        want, wantc, st = scan_numpy(recs, arr, lens, 2)
        result["numpy_restatement_on_the_clusters_s"] = time.time() - t
        assert got.tobytes() == want.tobytes() and (counts == wantc).all() and all(stats[k] == st[k] for k in st), "device result differs (clusters as loci)"
        t = time.time()
        want, wantc, st = scan_numpy(recs, wide, lens, 2, True)
        result["numpy_restatement_contig_wide_s"] = time.time() - t
        assert wgot.tobytes() == want.tobytes() and (wcounts == wantc).all() and all(wstats[k] == st[k] for k in st), "device result differs (contig-wide loci)"
        print("numpy restatement: %.2f s on the clusters, %.2f s contig-wide; both equal the device results"
              % (result["numpy_restatement_on_the_clusters_s"], result["numpy_restatement_contig_wide_s"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
