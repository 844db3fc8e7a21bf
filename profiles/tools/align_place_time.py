#!/usr/bin/env python3
"""Timing of the placement of multi-mapped reads (mirp_align_reads_placed; DESIGN.md §12 "Placement") on the inputs of align_time.py: the seeded
120 Mb genome and 6.7 M distinct 18-26-nt reads, one context, every timed call after a first call of the same kind, host clock around the call.

    python profiles/tools/align_place_time.py [--genome-mb 120] [--reads 6700000] [--repeats 3] [--out build/align_time/align_place_time.json]
    python profiles/tools/align_place_time.py --plain-only --root <another checkout>     (the unchanged -v 0 -k 20 call of that checkout's build)
    python profiles/tools/align_place_time.py --once                                      (one call of each kind: for a run under rocprofv3)

(a) `-v 0 -k 20` without placement, --repeats times: mean, min and max, the tool's run-to-run spread.
(b) `--place u` at -v 0 and -v 1 (m 50, window 50, seed 0) with the split first pass / placement / emit, and `--place r` at -v 0.
(c) (b) with the resident capacity forced to 1 item, so that every batch is aligned twice."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PHASES = ["read_parse", "upload", "seeds", "verify", "sort", "emit_download_write", "placement", "first_pass"]


def timed(ctx, rpath, sam, **kw):
    t = time.time()
    r = ctx.align_reads(rpath, sam, "align_place_time", **kw)
    wall = time.time() - t
    sec = r.pop("seconds")
    return {"wall_s": wall, "phases_s": dict(zip(PHASES, sec)), **r, "sam_bytes": os.path.getsize(sam)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=int, default=120)
    ap.add_argument("--reads", type=int, default=6_700_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the checkout whose mir_prefer_amd package and library are timed")
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "align_time"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.abspath(a.root))
    import align_time
    from mir_prefer_amd import capi
    os.makedirs(a.dir, exist_ok=True)
    gpath, rpath, sam = os.path.join(a.dir, "genome.fa"), os.path.join(a.dir, "reads.fa"), os.path.join(a.dir, "placed.sam")
    res = {"root": os.path.abspath(a.root), "genome_bases": a.genome_mb * 1_000_000}
    if not (os.path.exists(gpath) and os.path.exists(rpath)):           # a second run with the same --dir times the same files
        g = align_time.make_genome(gpath, a.genome_mb * 1_000_000, 1)
        align_time.make_reads(rpath, g, a.reads, 2)
        del g
    res["reads_bytes"] = os.path.getsize(rpath)
    ctx = capi.Context(0)
    ctx.align_index([gpath])
    if not a.once:
        ctx.align_reads(rpath, sam, "align_place_time", v=0, k=20)
    runs = [timed(ctx, rpath, sam, v=0, k=20) for _ in range(1 if a.once else a.repeats)]
    walls = [r["wall_s"] for r in runs]
    res["plain_v0_k20"] = {"walls_s": walls, "mean_s": sum(walls) / len(walls), "min_s": min(walls), "max_s": max(walls), "last": runs[-1]}
    print(json.dumps({"plain_v0_k20": res["plain_v0_k20"]}), flush=True)
    if not a.plain_only:
        for cap, tag in ((0, "resident"), (1, "realigned")):
            ctx.set_align_place_capacity(cap)
            for mode, v in (("u", 0), ("u", 1), ("r", 0)):
                if cap and mode == "r":
                    continue
                kw = dict(v=v, k=20, m=50, place=mode, window=50, seed=0)
                if not cap and not a.once:
                    timed(ctx, rpath, sam, **kw)
                r = timed(ctx, rpath, sam, **kw)
                r["batches"], r["realigned"] = ctx.align_last_batches(), ctx.align_place_last_realigned()
                res["place_%s_v%d_%s" % (mode, v, tag)] = r
                print(json.dumps({"call": "place_%s_v%d_%s" % (mode, v, tag), **r}), flush=True)
        ctx.set_align_place_capacity(0)
    ctx.close()
    os.unlink(sam)
    out = a.out or os.path.join(a.dir, "align_place_time.json")
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
