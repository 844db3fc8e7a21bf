#!/usr/bin/env python3
"""Timing of the isomiR counts (mirp_isomir_scan) on synthetic records.

    python profiles/tools/isomirs_time.py [--records 10000000] [--loci 10000] [--samples 3] [--dir /tmp/isomirs_time]
                                          [--out build/isomirs_time/isomirs_time.json] [--kernel-stats kernel_stats.csv] [--skip-restatement]
                                          [--skip-tokenizer]

10^4 loci of 20..24 nt on both strands of six 20 Mb contigs; 10^7 records, nine in ten drawn around a locus (offsets up to max + 2, a tail for one
in four), the rest background; depths 1..1000; three samples.  One context runs the scan at the default --max5 2 --max3 4 three times; the fastest
call is reported (wall, upload of the records included), beside the numpy restatement (tests/isomir_restatement.py, scan_numpy) on the same arrays
and the tailed tokenizer on SAM files holding the same number of records (a block of 10^5 lines repeated).  Kernel times come from a run of its own
under `rocprofv3 --kernel-trace --stats`; --kernel-stats reads that CSV and gives the time per scan of the iso_* kernels and the hash-record sort."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ROUNDS = 3
CONTIG_LEN = 20_000_000
N_CONTIGS = 6


def make_inputs(n, nl, samples, seed=1):
    from mir_prefer_amd.synth import ALN_DTYPE
    rng = np.random.default_rng(seed)
    tid = rng.integers(0, N_CONTIGS, nl)
    start = np.sort(rng.integers(100, CONTIG_LEN - 200, nl))
    end = start + rng.integers(19, 24, nl)
    strand = rng.integers(0, 2, nl)
    of = rng.integers(0, nl, n)
    bg = rng.random(n) < 0.1
    d5, d3 = rng.integers(-4, 5, n), rng.integers(-6, 7, n)
    sg = 1 - 2 * strand[of]
    l5, l3 = np.where(strand[of] == 0, start[of], end[of]), np.where(strand[of] == 0, end[of], start[of])
    r5, r3 = l5 + sg * d5, l3 + sg * d3
    alns = np.zeros(n, dtype=ALN_DTYPE)
    alns["tid"] = np.where(bg, rng.integers(0, N_CONTIGS, n), tid[of])
    alns["pos"] = np.where(bg, rng.integers(1, CONTIG_LEN - 100, n), np.minimum(r5, r3))
    alns["len"] = np.where(bg, rng.integers(18, 27, n), np.abs(r3 - r5) + 1)
    alns["strand"] = strand[of]
    alns["depth"] = rng.integers(1, 1001, n)
    alns["sample"] = rng.integers(0, samples, n)
    tails = np.where(rng.random(n) < 0.25, rng.integers(1, 156, n), 0).astype(np.uint32)        # tails of 1..3 letters
    loci = list(zip(tid.tolist(), strand.tolist(), start.tolist(), end.tolist()))
    return alns, tails, loci


def write_sams(folder, n, samples):
    rng = np.random.default_rng(2)
    head = "".join("@SQ\tSN:chr%d\tLN:%d\n" % (t, CONTIG_LEN) for t in range(N_CONTIGS))
    paths = []
    per = n // samples
    for s in range(samples):
        lines = []
        for k in range(100_000):
            m, t = int(rng.integers(19, 25)), int(rng.choice((0, 0, 0, 1, 2)))
            minus = bool(rng.integers(0, 2))
            cigar = "%dM" % m if not t else ("%dS%dM" % (t, m) if minus else "%dM%dS" % (m, t))
            lines.append("S%d_r%d_x%d\t%d\tchr%d\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tXA:i:0\tMD:Z:%d\tNM:i:0%s\n"
                         % (s, k, int(rng.integers(1, 1000)), 16 if minus else 0, int(rng.integers(0, N_CONTIGS)), int(rng.integers(1, CONTIG_LEN - 100)),
                            cigar, "A" * (m + t), "I" * (m + t), m, "\tXT:Z:" + "T" * t if t else ""))
        block = "".join(lines).encode()
        path = os.path.join(folder, "S%d.sam" % s)
        with open(path, "wb") as f:
            f.write(head.encode())
            for _ in range(max(per // 100_000, 1)):
                f.write(block)
        paths.append(path)
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--loci", type=int, default=10_000)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/isomirs_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "isomirs_time", "isomirs_time.json"))
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: kernel time per scan")
    ap.add_argument("--skip-restatement", action="store_true")
    ap.add_argument("--skip-tokenizer", action="store_true")
    args = ap.parse_args()
    if args.kernel_stats:
        own, scans = {}, {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                base = name.split("(")[0].split("<")[0].split("::")[-1]
                t = float(row["TotalDurationNs"]) * 1e-9
                if base.startswith("iso_") or (base.startswith("sort_") and "MirpHashRec" in name):
                    own[name] = t / ROUNDS
                elif base.startswith("excl_scan"):
                    scans[name] = t / ROUNDS
        res = {"per_scan_s": own, "per_scan_total_s": sum(own.values()), "int32_scans_per_scan_s": sum(scans.values())}
        print(json.dumps(res, indent=1))
        return 0
    from mir_prefer_amd import capi
    from tests import isomir_restatement as R
    from tests.test_isomirs_gpu import as_result, loci_array
    t0 = time.time()
    alns, tails, loci = make_inputs(args.records, args.loci, args.samples)
    print("inputs ready in %.1f s" % (time.time() - t0), flush=True)
    result = {"records": args.records, "loci": args.loci, "samples": args.samples}
    ctx = capi.Context(0)
    la = loci_array(loci)
    walls = []
    for _ in range(ROUNDS):
        t0 = time.time()
        got = ctx.isomir_scan(alns, tails, la, 2, 4, args.samples)
        walls.append(time.time() - t0)
    ctx.close()
    result["scan_wall_s"] = walls
    result["stats"] = got[4]
    print("mirp_isomir_scan walls %s, stats %s" % (["%.4f" % w for w in walls], got[4]), flush=True)
    if not args.skip_restatement:
        t0 = time.time()
        want = R.scan_numpy(alns, tails, loci, 2, 4, args.samples)
        result["numpy_restatement_s"] = time.time() - t0
        result["equal"] = as_result(*got) == want
        print("numpy restatement %.2f s, equal to the device: %s" % (result["numpy_restatement_s"], result["equal"]), flush=True)
    if not args.skip_tokenizer:
        os.makedirs(args.dir, exist_ok=True)
        paths = write_sams(args.dir, args.records, args.samples)
        result["sam_bytes"] = sum(os.path.getsize(p) for p in paths)
        capi.tokenize_sams_tailed(paths)                      # page cache
        t0 = time.time()
        out = capi.tokenize_sams_tailed(paths)
        result["tokenizer_s"] = time.time() - t0
        result["tokenizer_records"] = len(out[3])
        print("tailed tokenizer %.3f s for %d records, %d bytes" % (result["tokenizer_s"], len(out[3]), result["sam_bytes"]), flush=True)
        for p in paths:
            os.remove(p)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
