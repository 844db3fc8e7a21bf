#!/usr/bin/env python3
"""Timing of the miRNA triggers of PHAS loci (mirp_trigger_scan) on the input of phasing_time.py.

    python profiles/tools/triggers_time.py [--dir /tmp/triggers_time] [--out build/triggers_time/triggers_time.json] [--records 10000000]
                                           [--mirnas 1000] [--restate-loci 200] [--kernel-stats kernel_stats.csv]

Input: phasing_time.py's records and SAM files (six contigs of 20 Mb), a random genome of those contigs, and --mirnas random 21-nt miRNAs; the
phasing scan (-l 21, defaults) gives the loci, and a perfect site of miRNA q % mirnas is written on the best register of every fifth locus q
before the genome file is written, so that the scan has triggers to find.  The steps run as child processes, each under its own time limit, and
the first one that fails ends the run:

    scan       one context: ingest, mirp_phase_scan, the genome and phas.tsv files, then mirp_trigger_scan three times (the last is reported)
    targets    the existing route on the same input: `targets -b -c` with the same miRNAs on the loci's sequences (.phas.fa)
    restate    the numpy restatement (tests/trigger_restatement.py) on the first --restate-loci loci, compared with the device's lines for them

Kernel times come from a run of the scan step of its own under `rocprofv3 --kernel-trace --stats`:
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/tools/triggers_time.py --step scan
and --kernel-stats reads that CSV and gives the time of tr_scan_kernel and tr_window_kernel per call."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"scan": 600, "targets": 300, "restate": 600}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _paths(d):
    return {k: os.path.join(d, v) for k, v in (("genome", "genome.fa"), ("mirna", "mirnas.fa"), ("phas", "l21.phas.tsv"), ("fa", "l21.phas.fa"),
                                               ("trig", "l21.phas.triggers.tsv"), ("summ", "l21.phas.triggers.summary.tsv"))}


def step_scan(args, result):
    import phasing_time
    from mir_prefer_amd import capi, phasing, triggers
    P = _paths(args.dir)
    t0 = time.time()
    recs = phasing_time.make_records(args.records)
    sams = phasing_time.write_sams(args.dir, recs)
    rng = np.random.RandomState(2)
    names = ["chr%d" % (c + 1) for c in range(phasing_time.N_CONTIGS)]
    seqs = [ACGT[rng.randint(0, 4, phasing_time.CONTIG_LEN)] for _ in names]
    mirs = [ACGT[rng.randint(0, 4, 21)].tobytes() for _ in range(args.mirnas)]
    with open(P["mirna"], "wb") as f:
        f.write(b"".join(b">mir%d\n%s\n" % (i, m.replace(b"T", b"U")) for i, m in enumerate(mirs)))
    print("inputs ready in %.1f s: %d records" % (time.time() - t0, len(recs)), flush=True)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    ctx = capi.Context(0)
    try:
        t = time.time()
        n_names, lens, _, alns, _, sec = ctx.ingest_sams(sams)
        result["ingest"] = {"wall_s": time.time() - t, "tokenize_s": sec["tokenize_s"]}
        assert n_names == names
        hg = phasing.Hypergeom(10, 21)
        kmin = hg.kmin(Fraction(1, 1000))
        wins, _ = ctx.phase_scan(21, 10, kmin)
        loci = phasing.merge_loci(phasing.window_tuples(wins), lens, 10, 21, hg)
        planted = 0
        for q, (tid, start, end, _, w, _) in enumerate(loci):
            o = int(w[1]) - 21 + 9                                       # a plus site whose cut is the best window's register
            if q % 5 == 0 and o > 0 and o + 21 < phasing_time.CONTIG_LEN:
                seqs[tid][o:o + 21] = np.frombuffer(mirs[q % args.mirnas].translate(comp)[::-1], np.uint8)
                planted += 1
        with open(P["genome"], "wb") as f:
            for n, s in zip(names, seqs):
                f.write(b">" + n.encode() + b"\n" + s.tobytes() + b"\n")
        with open(P["phas"], "wb") as f:
            f.write(phasing.format_tsv(names, loci))
        with open(P["fa"], "wb") as f:
            f.write(phasing.format_fasta(names, loci, seqs))
        rows = triggers.parse_phas(open(P["phas"], "rb").read())
        t = time.time()
        genome = capi.read_fasta(P["genome"])
        result["read_genome_s"] = time.time() - t
        for rnd in range(3):
            t = time.time()
            tsv, summ, st = triggers.scan(ctx, P["mirna"], P["genome"], rows, names, genome, 21, 10, Fraction(1, 1000))
            wall = time.time() - t
        sec = st.pop("seconds")
        result["scan"] = dict(st, loci=len(rows), planted=planted, module_call_s=wall, mirp_trigger_scan_s=sum(sec),
                              seconds=dict(zip(("parse_pack", "upload", "sites_sort", "units", "windows_download"), sec)),
                              evaluations=2 * st["interval_bases"] * st["mirnas"])
        open(P["trig"], "wb").write(tsv)
        open(P["summ"], "wb").write(summ)
    finally:
        ctx.close()
    print(json.dumps(result["scan"]), flush=True)


def step_targets(args, result):
    P = _paths(args.dir)
    t = time.time()
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets", "-b", "-c", "-o", os.path.join(args.dir, "route.targets.tsv"), P["mirna"], P["fa"]],
                       capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT))
    result["targets_route"] = {"wall_s": time.time() - t, "rc": r.returncode, "stderr": r.stderr.decode().strip()[-300:]}
    if r.returncode != 0:
        raise SystemExit("targets failed: " + r.stderr.decode())
    print(json.dumps(result["targets_route"]), flush=True)


def step_restate(args, result):
    import phasing_time
    from mir_prefer_amd import capi, triggers
    from tests.test_targets_cpu import parse_mirnas
    from tests.trigger_restatement import restate_numpy
    P = _paths(args.dir)
    recs = phasing_time.make_records(args.records)
    rows = triggers.parse_phas(open(P["phas"], "rb").read())[:args.restate_loci]
    genome = capi.read_fasta(P["genome"])
    names = [n for n, _ in genome]
    mirnas = parse_mirnas(open(P["mirna"], "rb").read())
    t = time.time()
    tsv, summ = restate_numpy(recs, names, [s for _, s in genome], mirnas, rows)
    result["numpy_restatement"] = {"loci": len(rows), "wall_s": time.time() - t, "lines": tsv.count(b"\n") - 1}
    loci = {b"%s:%d-%d" % (r[0].encode(), r[1], r[2]) for r in rows}
    got = [ln for ln in open(P["trig"], "rb").read().split(b"\n")[1:-1] if ln.split(b"\t")[0] in loci]
    assert got == tsv.split(b"\n")[1:-1], "the device's lines of these loci differ from the restatement"
    print(json.dumps(result["numpy_restatement"]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", default="/tmp/triggers_time")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "triggers_time", "triggers_time.json"))
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--mirnas", type=int, default=1000)
    ap.add_argument("--restate-loci", type=int, default=200)
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats CSV of a run of `--step scan`: kernel time per mirp_trigger_scan call")
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if args.kernel_stats:
        rows = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                name = row["Name"].split("(")[0].split("<")[0].split("::")[-1]
                if name.startswith("tr_"):
                    rows[name] = rows.get(name, 0.0) + float(row["TotalDurationNs"]) * 1e-9 / 3          # the step calls the scan three times
        print(json.dumps({"kernel_s_per_call": rows}, indent=1))
        json.dump({"kernel_s_per_call": rows}, open(args.out.replace(".json", "_kernels.json"), "w"), indent=1)
        return 0
    if args.step:
        result = {}
        {"scan": step_scan, "targets": step_targets, "restate": step_restate}[args.step](args, result)
        json.dump(result, open(args.out.replace(".json", "_%s.json" % args.step), "w"), indent=1)
        return 0
    result = {"records": args.records, "mirnas": args.mirnas}
    for step in ("scan", "targets", "restate"):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", args.dir, "--out", args.out,
               "--records", str(args.records), "--mirnas", str(args.mirnas), "--restate-loci", str(args.restate_loci)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (step, rc), flush=True)
            return 1
        result.update(json.load(open(args.out.replace(".json", "_%s.json" % step))))
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
