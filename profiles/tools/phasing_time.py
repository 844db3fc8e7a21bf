#!/usr/bin/env python3
"""Timing of the phased siRNA (PHAS) loci (mirp_phase_scan) on seeded inputs.

    python profiles/tools/phasing_time.py [--dir /tmp/phasing_time] [--out build/phasing_time/phasing_time.json] [--records 10000000]
                                          [--kernel-stats kernel_stats.csv] [--skip-restatement]

Input: two SAM files against a 120 Mb genome (six contigs of 20 Mb), about 10 M records: 40 % of length 21, 15 % of length 24, the rest 18..26
spread uniformly, on both strands, depths geometric; plus 300 planted 21-phased and 100 planted 24-phased loci on both strands.  One context runs
the ingest and the scans (-l 21 and -l 24, defaults otherwise) twice; the second round is reported: tokenize, ingest (upload + filter, sort,
download), scan (the mirp_phase_scan call), host merge + write, and the numpy restatement of the windows (tests/test_phasing_cpu.py) on the same
records.  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`; --kernel-stats reads that CSV and gives the kernels'
time per scan and anchors per second of kernel time."""
import argparse
import csv
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N_CONTIGS, CONTIG_LEN = 6, 20_000_000


def make_records(n, seed=1):
    from mir_prefer_amd.synth import ALN_DTYPE
    rng = np.random.RandomState(seed)
    r = np.zeros(n, ALN_DTYPE)
    r["tid"] = rng.randint(0, N_CONTIGS, n)
    r["pos"] = rng.randint(1, CONTIG_LEN - 40, n)
    r["len"] = np.where(rng.rand(n) < 0.55, np.where(rng.rand(n) < 0.4 / 0.55, 21, 24), rng.randint(18, 27, n))
    r["strand"] = rng.randint(0, 2, n)
    r["depth"] = np.minimum(rng.geometric(0.35, n), 100000)
    rows = []
    for L, count in ((21, 300), (24, 100)):
        for _ in range(count):
            tid, x0 = int(rng.randint(0, N_CONTIGS)), int(rng.randint(10, CONTIG_LEN - 20 * L))
            for j in range(int(rng.randint(6, 13))):
                rows += [(tid, x0 + j * L, int(rng.randint(3, 200)), L, 0), (tid, x0 + j * L - 2, int(rng.randint(3, 200)), L, 1)]
    p = np.zeros(len(rows), ALN_DTYPE)
    a = np.array(rows, np.int64)
    p["tid"], p["pos"], p["depth"], p["len"], p["strand"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]
    r = np.concatenate([r, p])
    return r[np.lexsort((r["pos"], r["tid"]))]


def write_sams(d, recs):
    paths = [os.path.join(d, "s%d.sam" % i) for i in range(2)]
    if all(os.path.exists(p) for p in paths):
        return paths
    head = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:chr%d\tLN:%d\n" % (c + 1, CONTIG_LEN) for c in range(N_CONTIGS))
    seq = {L: "A" * L for L in range(10, 40)}
    for f, p in enumerate(paths):
        sub = recs[f::2]
        with open(p, "w") as out:
            out.write(head)
            cols = zip(sub["tid"].tolist(), sub["pos"].tolist(), sub["depth"].tolist(), sub["len"].tolist(), sub["strand"].tolist())
            buf = []
            for i, (t, pos, dep, L, s) in enumerate(cols):
                buf.append("s%d_r%d_x%d\t%d\tchr%d\t%d\t255\t%dM\t*\t0\t0\t%s\t*\n" % (f, i, dep, 16 * s, t + 1, pos, L, seq[L]))
                if len(buf) == 1 << 16:
                    out.write("".join(buf))
                    buf = []
            out.write("".join(buf))
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default="/tmp/phasing_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "phasing_time", "phasing_time.json"))
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of this tool: kernel time per scan")
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    if args.kernel_stats:
        prev = json.load(open(args.out))
        anchors = sum(c["anchors"] for c in prev["scans"].values()) * 2          # every scan ran twice
        rows = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if row["Name"].split("(")[0].split("<")[0].split("::")[-1].startswith("ph_"):
                    rows[row["Name"]] = float(row["TotalDurationNs"]) * 1e-9
        tot = sum(rows.values())
        res = {"phase_kernels_s": rows, "phase_kernel_total_s": tot, "per_scan_s": tot / (2 * len(prev["scans"])),
               "anchors_per_s_kernel": anchors / tot if tot else None}
        print(json.dumps(res, indent=1))
        json.dump(res, open(args.out.replace(".json", "_kernels.json"), "w"), indent=1)
        return 0
    from mir_prefer_amd import capi, phasing
    os.makedirs(args.dir, exist_ok=True)
    t0 = time.time()
    recs = make_records(args.records)
    paths = write_sams(args.dir, recs)
    print("inputs ready in %.1f s: %d records, %d bytes of SAM" % (time.time() - t0, len(recs), sum(os.path.getsize(p) for p in paths)), flush=True)
    result = {"records": int(len(recs)), "scans": {}}
    ctx = capi.Context(0)
    try:
        for rnd in range(2):
            t = time.time()
            names, lens, _, alns, _, sec = ctx.ingest_sams(paths)
            ingest = {"wall_s": time.time() - t, "tokenize_s": sec["tokenize_s"], "upload_filter_s": sec["upload_filter_s"], "sort_s": sec["sort_s"],
                      "download_s": sec["download_s"]}
            assert len(alns) == len(recs)
            for L in (21, 24):
                hg = phasing.Hypergeom(10, L)
                t = time.time()
                kmin = hg.kmin(Fraction(1, 1000))
                t_kmin = time.time() - t
                t = time.time()
                wins, st = ctx.phase_scan(L, 10, kmin)
                t_scan = time.time() - t
                t = time.time()
                loci = phasing.merge_loci(phasing.window_tuples(wins), lens, 10, L, hg)
                with open(os.path.join(args.dir, "l%d.phas.tsv" % L), "wb") as f:
                    f.write(phasing.format_tsv(names, loci))
                t_host = time.time() - t
                if rnd == 1:
                    result["scans"]["l%d" % L] = {"records_of_length": st["records"], "units": st["units"], "anchors": st["anchors"],
                                                  "passing_windows": int(len(wins)), "loci": len(loci), "kmin_s": t_kmin, "scan_s": t_scan,
                                                  "host_merge_write_s": t_host, "anchors_per_s_scan_call": st["anchors"] / t_scan}
                    print("l%d" % L, json.dumps(result["scans"]["l%d" % L]), flush=True)
            if rnd == 1:
                result["ingest"] = ingest
                print("ingest", json.dumps(ingest), flush=True)
    finally:
        ctx.close()
    sc = result["scans"]["l21"]
    result["share_of_wall_l21"] = {"ingest": result["ingest"]["wall_s"] / (result["ingest"]["wall_s"] + sc["scan_s"] + sc["host_merge_write_s"]),
                                   "scan": sc["scan_s"] / (result["ingest"]["wall_s"] + sc["scan_s"] + sc["host_merge_write_s"])}
    if not args.skip_restatement:
        from tests.test_phasing_cpu import windows_numpy
        t = time.time()
        want = windows_numpy(recs, 21, 10)
        result["numpy_restatement_l21_s"] = time.time() - t
        result["numpy_restatement_l21_windows"] = len(want)
        assert len(want) == sc["passing_windows"]
        print("numpy restatement: %.2f s" % result["numpy_restatement_l21_s"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
