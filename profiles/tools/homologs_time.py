#!/usr/bin/env python3
"""Timing of the homolog search (mirp_homolog_scan) on a seeded genome of 120 Mb: 10,000 random 21-nt queries plus the known
sequences of planted hairpins, at -v 1 and -v 3.

    python profiles/tools/homologs_time.py [--genome-mb 120] [--queries 10000] [--planted 200] [--out build/homologs_time/homologs_time.json]

Genome: align_time.py's (random bases in 8 contigs, 2,000 copied segments of 1-5 kb, 200 runs of 100 N), with the hairpins of
tests/homolog_restatement.py planted into it.  Every timed call runs after a first call of the same kind (code objects loaded).  Reports the
seconds of the scan, the windows, the fold and the evaluation, and placements/s (over the scan) and windows/s (over the fold)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PHASES = ("scan", "windows", "fold", "evaluation_download", "merge")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=int, default=120)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--planted", type=int, default=200)
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "homologs_time"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from align_time import make_genome
    from mir_prefer_amd import capi
    from tests import homolog_restatement as hr
    os.makedirs(a.dir, exist_ok=True)
    total = a.genome_mb * 1_000_000
    gpath = os.path.join(a.dir, "genome.fa")
    t = time.time()
    make_genome(gpath, total, 1)
    # plant the hairpins by patching the FASTA text in place: lines of 100 bases + newline, 8 contigs of equal length with a header each
    rng = random.Random(4)
    queries, seen = [], set()
    clen = total // 8
    with open(gpath, "r+b") as f:
        for k in range(a.planted):
            hp, known, _ = hr.planted_hairpin(rng, 3)
            c, at = rng.randrange(8), rng.randrange(1000, clen - 1000)
            head = sum(len(b">chr%d\n" % (i + 1)) for i in range(c + 1)) + c * (clen + clen // 100)
            for j, ch in enumerate(hp):          # base p of a contig stands at head + p + p // 100
                f.seek(head + at + j + (at + j) // 100)
                f.write(ch.encode())
            if known not in seen:
                seen.add(known)
                queries.append(known)
    while len(queries) < a.planted + a.queries:
        q = hr.random_seq(rng, 21)
        if q not in seen:
            seen.add(q)
            queries.append(q)
    res = {"genome_bases": total, "queries": len(queries), "planted": a.planted, "make_inputs_s": time.time() - t}
    ctx = capi.Context(0)
    t = time.time()
    idx = ctx.align_index([gpath])
    res["index_s"] = time.time() - t
    res["index_phases_s"] = idx["seconds"]
    ctx.homolog_scan(queries[:64], max_mismatches=1)
    for v in (1, 3):
        ctx.homolog_scan(queries[:64], max_mismatches=v)
        t = time.time()
        recs, _, _ = ctx.homolog_scan(queries, max_mismatches=v)
        wall = time.time() - t
        st = ctx.homolog_last_stats()
        sec = dict(zip(PHASES, st.pop("seconds")))
        res["v%d" % v] = {"wall_s": wall, "phases_s": sec, **st, "placements_per_s": st["placements"] / max(sec["scan"], 1e-9),
                          "windows_per_s": st["placements"] / max(sec["fold"], 1e-9)}
        print(json.dumps({"v": v, **res["v%d" % v]}), flush=True)
    ctx.close()
    out = a.out or os.path.join(a.dir, "homologs_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    os.unlink(gpath)


if __name__ == "__main__":
    main()
