"""Dev tool: the fold stage of a bench workload under given fold-overlap switches, one JSON line per setting; the library is the tree's own or the one
named by MIRP_LIB.  Run it from several trees (or with several libraries) back to back in one session to compare.

    fold_overlap_time.py [--workload config1|config2] [--folds 8] [--tree NAME] SETTING ...

SETTING is `overlap:tailfree`, e.g. `a:a` (automatic, -1), `0:x` (serial path), `5120:0` (equal chunks of 5,120 windows, fills in order), `2560:1`;
`x` leaves a switch alone (a library without it).  k0 / k1 are mirp_last_fold_kernel_ms: first fill's start to last fill's end, and the rest."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from mir_prefer_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="config1")
ap.add_argument("--folds", type=int, default=8)
ap.add_argument("--tree", default=os.path.basename(ROOT))
ap.add_argument("settings", nargs="+")
a = ap.parse_args()
specs, n_samples, background, _, _ = bench.workload_specs(a.workload, 1)
contigs, alns, _ = bench.build_shard(specs, set(range(len(specs))), n_samples, background)
order = np.argsort(np.array([n for n, _ in contigs], dtype=object), kind="stable").astype(np.int32)
ctx = capi.Context(0)
ctx.load_genome(contigs)
ctx.load_alignments(alns)
_, _, nwin = ctx.candidate(bench.CUT, bench.GAP, bench.L, order)
ctx.fold(bench.L)      # one-off costs
for s in a.settings:
    ov, tf = ("-1" if v == "a" else v for v in s.split(":"))
    if ov != "x":
        ctx.set_fold_overlap(int(ov))
    if tf != "x":
        ctx.set_fold_overlap_tailfree(int(tf))
    ctx.fold(bench.L)
    fold, k0, k1 = [], [], []
    for _ in range(a.folds):
        ctx.fold(bench.L)
        fold.append(ctx.last_timings()["fold_ms"])
        k = ctx.last_fold_kernel_ms()
        k0.append(k[0]); k1.append(k[1])
    print(json.dumps({"lib": os.path.basename(capi.LIB_PATH), "tree": a.tree, "workload": a.workload, "overlap": ov, "tailfree": tf, "windows": int(nwin),
                      "chunks": ctx.last_fold_overlap_chunks() if hasattr(ctx, "last_fold_overlap_chunks") else -1, "dense": ctx.last_fold_dense(),
                      "fallbacks": ctx.last_fold_fallbacks(), "fold_ms_min": round(min(fold), 3), "fold_ms_med": round(float(np.median(fold)), 3),
                      "fold_ms_max": round(max(fold), 3), "k0_med": round(float(np.median(k0)), 3), "k1_med": round(float(np.median(k1)), 3)}), flush=True)
ctx.close()
