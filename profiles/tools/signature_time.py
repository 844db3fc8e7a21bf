#!/usr/bin/env python3
"""Timing of the duplex and overlap-signature scan (mirp_signature_scan) on the input of clusters_time.py.

    python profiles/tools/signature_time.py [--out build/signature_time/signature_time.json] [--records 10000000] [--skip-restatement]

Input: the records of phasing_time.py (about 10 M against a 120 Mb genome of six 20 Mb contigs, with planted phased duplexes), loaded as they
are, so no SAM text is written.  One context runs, twice each and reporting the second round,
  - mirp_cluster_scan at the default -m 0.5rpm --pad 75, whose clusters are the loci of the first case,
  - mirp_signature_scan at its defaults with those clusters as loci, and
  - mirp_signature_scan with one locus per contig that spans it whole (--contigs).
It then times the numpy statement of the scan (tests/signature_restatement.py) on the same arrays and fails if a device result differs from
it.  The times are host-clock walls of whole calls, downloads included: the sorts, scans and kernels of a call are not separated."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "signature_time", "signature_time.json"))
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    from mir_prefer_amd import capi, clusters
    from phasing_time import CONTIG_LEN, N_CONTIGS, make_records
    from tests.signature_restatement import scan_numpy
    t0 = time.time()
    recs = make_records(args.records)
    lens = [CONTIG_LEN] * N_CONTIGS
    total = int(recs["depth"].sum(dtype=np.uint64))
    T = clusters.threshold(clusters.parse_min_coverage("0.5rpm"), total)
    print("inputs ready in %.1f s: %d records, %d reads, T %d" % (time.time() - t0, len(recs), total, T), flush=True)
    wide = np.zeros(N_CONTIGS, capi.LOCUS_DTYPE)
    wide["tid"], wide["strand"], wide["start"], wide["end"] = np.arange(N_CONTIGS), 2, 1, CONTIG_LEN
    result = {"records": int(len(recs)), "T": T}
    ctx = capi.Context(0)
    try:
        ctx.load_genome([("chr%d" % (i + 1), np.full(4, 65, np.uint8)) for i in range(N_CONTIGS)])
        ctx.load_alignments(recs)
        for rnd in range(2):
            cl, _, _ = ctx.cluster_scan(T, 75, lens, 1)
            arr = np.zeros(len(cl), capi.LOCUS_DTYPE)
            arr["tid"], arr["strand"], arr["start"], arr["end"] = cl["tid"], 2, cl["start"], cl["end"]
            t = time.time()
            got = ctx.signature_scan(arr, lens)
            t_loci = time.time() - t
            slots = ctx.last_jobs_per_slot(7)
            t = time.time()
            wgot = ctx.signature_scan(wide, lens)
            t_wide = time.time() - t
            wslots = ctx.last_jobs_per_slot(7)
        result["signature_scan_on_the_clusters"] = dict(got[3], loci=len(arr), wall_s=t_loci, jobs_per_slot=slots, records_per_s=len(recs) / t_loci,
                                                        loci_with_a_duplex=int((got[0]["duplexes"] > 0).sum()), duplexes=int(got[0]["duplexes"].sum()))
        result["signature_scan_contig_wide"] = dict(wgot[3], loci=len(wide), wall_s=t_wide, jobs_per_slot=wslots, records_per_s=len(recs) / t_wide,
                                                    duplexes=int(wgot[0]["duplexes"].sum()), peak_overlaps=(1 + wgot[1].argmax(1)).tolist())
    finally:
        ctx.close()
    print(json.dumps(result, indent=1), flush=True)
    if not args.skip_restatement:
        for name, loci, dev in (("on_the_clusters", arr, got), ("contig_wide", wide, wgot)):
            t = time.time()
            want = scan_numpy(recs, loci, lens)
            result["numpy_restatement_%s_s" % name] = time.time() - t
            assert dev[0].tobytes() == want[0].tobytes() and (dev[1] == want[1]).all() and dev[2].tobytes() == want[2].tobytes() and dev[3] == want[3], \
                "device result differs (%s)" % name
        print("numpy restatement: %.2f s on the clusters, %.2f s contig-wide; both equal the device results"
              % (result["numpy_restatement_on_the_clusters_s"], result["numpy_restatement_contig_wide_s"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
