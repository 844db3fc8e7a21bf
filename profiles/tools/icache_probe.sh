cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
rocprofv3 -L 2>/dev/null | grep -oE "\b(SQC?_[A-Z_0-9]*(ICACHE|IFETCH|INST_CACHE|INSTR)[A-Z_0-9]*)\b" | sort -u | head -40
OUT=${1:-/tmp/icache_probe}          # rocprofv3 output folder (and $OUT.log); --full: the vienna-1.8.5 launches (fold_lds_kernel<1, ...) come from the `configs` block
timeout 300 rocprofv3 --kernel-trace --pmc SQ_IFETCH SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQ_WAVE_CYCLES SQ_BUSY_CYCLES --output-format csv -d "$OUT" -- python3 bench.py --full --steps 2 --warmup 0 --no-cpu-baseline > "$OUT.log" 2>&1
tail -2 "$OUT.log" | cut -c1-300
OUT="$OUT" python3 - <<'PY'
import csv, glob, collections, os
for f in glob.glob(os.path.join(os.environ["OUT"], "**", "*counter_collection.csv"), recursive=True):
    agg = collections.defaultdict(float); n = collections.Counter()
    for r in csv.DictReader(open(f)):
        if "fold_lds_kernel" in r["Kernel_Name"] and "epilogue" not in r["Kernel_Name"] and (", true" in r["Kernel_Name"] or "<1" in r["Kernel_Name"]):
            agg[r["Counter_Name"]] += float(r["Counter_Value"]); n[r["Counter_Name"]] += 1
    for k in agg: print(k, agg[k] / max(1, n[k]), n[k])
PY
