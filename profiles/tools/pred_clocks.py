"""Dev tool: phase clocks of the filter kernel (predict_kernel) on the benchmark workload.
needs the diagnostics build: make -C mir-prefer_amd/csrc DIAG=1, then MIRP_LIB=mir-prefer_amd/libmirprefer_diag.so python <this file>"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from mir_prefer_amd import synth, capi
ds = synth.make_dataset([30427671], 12000, n_samples=1, seed=2, contig_names=["Chr1"])
ctx = capi.Context(0)
ctx.load_genome(ds.contigs); ctx.load_alignments(ds.sorted_alns())
ctx.candidate(10, 100, 300, np.zeros(1, dtype=np.int32))
ctx.fold(300)
ctx.predict(1, 18, 23, False, True)
os.environ["MIRP_PREDICT_CLOCKS"] = "1"
out = ctx.predict(1, 18, 23, False, True)
print("%s: predict %.3f ms, %d loci" % (os.path.basename(capi.LIB_PATH), ctx.last_timings()["predict_ms"], len(out["result"])), flush=True)
