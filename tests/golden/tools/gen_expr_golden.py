#!/usr/bin/env python3
"""Dev-only (build container): golden vectors for the expression rules of the predict stage (row a10 of SURVEY.md section 8), from DIRECT calls
of the reference's own functions through the py3 shim (ref_shim.py; nothing of the reference is copied):

  * `geometry`: get_maturestar_info (MP:1876-1999) of every (structure, mature) pair of the planted windows of tests/expression_cases.py -- the
    fail string, or star and fold coordinates.  The case builder places its reads on these, so it runs here on the reference's answers.
  * `pairs`: check_expression_new (MP:2037-2163) of every pair that has coordinates, with ALLOW_3NT_OVERHANG off and on, on a dict_map_info built
    in memory from the case's records exactly as gen_mapinfo_each_sample (MP:2002-2031) would: reads with startpos >= start and
    startpos + len <= end of the window, {sample: {"+"/"-": {startpos: [(seq, depth)]}}}.  Kept: every non-dict item of the result and the
    numbers of the per-sample dicts; or the exception class where the reference raises (a precursor without a read divides by zero).
  * `cases`, `records`: the inputs themselves, so that a golden that no longer matches the builder is noticed.

Regenerate (byte for byte):   python3 tests/golden/tools/gen_expr_golden.py
Output: tests/golden/expr_rules.json.gz"""
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(GOLD, "expr_rules.json.gz")


def main():
    if not os.path.exists(os.path.join(os.environ.get("MIRP_ORACLE_BIN", "/tmp/ora/bin"), "samtools")):
        os.environ["MIRP_ORACLE_BIN"] = tempfile.mkdtemp()          # no binary runs here: the shim only needs a place for its PATH links
    import ref_shim
    from tests import expression_cases as ec
    g = ref_shim.load_reference()
    geometry = {}

    def ref_geometry(ss, m0, m1, foldstart, ws, we, strand):
        key = ec.geometry_key(ss, m0, m1, foldstart, ws, we, strand)
        if key not in geometry:
            r = g["get_maturestar_info"](ss, (m0, m1), foldstart, foldstart + len(ss), ws, we, "+-"[strand])
            geometry[key] = r if isinstance(r, str) else [int(r[0]), int(r[1]), int(r[2]), int(r[3])]
        r = geometry[key]
        return r if isinstance(r, str) else tuple(r)

    cases, rec = ec.build(ref_geometry)
    # the structure list the builder states for every line is the reference's (is_stem_loop / filter_ss / has_one_good_bifurcation, MP:1574-1589)
    for c in cases:
        for (ss, start, energy), pieces in zip(c["lines"], c["pieces"]):
            if g["is_stem_loop"](ss, 3):
                want = [(0, len(ss))]
            else:
                want = [(s, len(x)) for s, x in g["filter_ss"](ss)[0] if g["is_stem_loop"](x, 3) or g["has_one_good_bifurcation"](x)]
            assert [tuple(p) for p in pieces] == want, (c["name"], pieces, want)
    pairs = {}
    for c in cases:
        w = c["window"]
        names = ["s%d" % k for k in range(c["n_samples"])]
        info = {n: {"+": {}, "-": {}} for n in names}
        for pos, ln, strand, sample, depth in ec.member_reads(rec, w["tid"], w["ws"], w["we"]):
            info[names[sample]]["+-"[strand]].setdefault(pos, []).append(("A" * ln, depth))
        for line, off, ln, ne, fstart in ec.structures_of(c):
            ss = c["lines"][line][0][off:off + ln]
            for m0, m1, strand, depth in c["matures"]:
                if not (ec.MIN_MATURE <= m1 - m0 <= ec.MAX_MATURE):
                    continue
                geo = ref_geometry(ss, m0, m1, fstart, w["ws"], w["we"], strand)
                if isinstance(geo, str):
                    continue
                star_s, star_e, fold_s, fold_e = geo
                for allow in (0, 1):
                    key = ec.pair_key(c["index"], m0, m1, geo, strand, allow)
                    if key in pairs:
                        continue
                    try:
                        r = g["check_expression_new"](info, names, fold_s, fold_e, (m0, m1), depth, (star_s, star_e), "+-"[strand], bool(allow))
                    except Exception as e:
                        pairs[key] = {"raises": type(e).__name__}
                        continue
                    out = {k: v for k, v in r.items() if not isinstance(v, dict)}
                    out["samples"] = [{k: v for k, v in r[n].items() if k != "reads_maps"} for n in names]
                    pairs[key] = out
    out = {"generator": "reference functions through tests/golden/tools/ref_shim.py: get_maturestar_info (MP:1876-1999), check_expression_new "
                        "(MP:2037-2163), is_stem_loop, filter_ss, has_one_good_bifurcation (MP:1602-1724), on the planted cases of tests/expression_cases.py",
           "cases": cases, "records": [[int(x) for x in r] for r in rec.tolist()], "geometry": geometry, "pairs": pairs}
    with open(PATH, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
            f.write(json.dumps(out, sort_keys=True, separators=(",", ":")).encode())
    print("wrote", PATH, os.path.getsize(PATH), "bytes;", len(cases), "cases,", len(rec), "records,", len(geometry), "geometries,", len(pairs), "pairs")


if __name__ == "__main__":
    main()
