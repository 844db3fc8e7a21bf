"""Planted cases for the expression half of the filter kernel, and a plain-Python restatement of it.

`build(geometry)` returns a deterministic list of named cases: one window each, with its structure lines, candidate matures and a handful of
alignment records placed relative to the coordinates get_maturestar_info gives (mature, star, fold region).  `geometry` is the function that
supplies those coordinates: the generator (tests/golden/tools/gen_expr_golden.py) passes the reference's own get_maturestar_info, the tests pass
a lookup in the golden it wrote (tests/golden/expr_rules.json.gz) -- a geometry the golden does not hold raises, so a stale golden is noticed.

The restatement (`expression`, `decide`, `window_truth`) follows the reference's text -- check_expression_new (MP:2037-2163, MP =
miR_PREFeR.py) and the decision tree of check_loci (MP:2241-2343) -- with Python integers and floats.  It is the truth of
tests/test_expression_rules_cpu.py (against direct reference calls and the C oracle) and of tests/test_expression_rules_gpu.py."""
import gzip
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALN_DTYPE = np.dtype([("tid", "<i4"), ("pos", "<i4"), ("depth", "<u4"), ("len", "<u2"), ("strand", "u1"), ("sample", "u1")])
MIN_MATURE, MAX_MATURE, MINLEN = 18, 24, 55
MAX_LINES, STRIDE = 96, 120
MAX_MIRNA = 8          # MIRP_MAX_MIRNA_PER_WINDOW
I32_MAX = 2 ** 31 - 1
MS_CODE = {"FAIL_STRUCTURE_MATCHED_BASES": 1, "FAIL_STRUCTURE_MATURE_NOT_IN_FOLD_REGION": 2, "FAIL_STRUCTURE_MATURE_NOT_IN_ONE_ARM": 3,
           "FAIL_STRUCTURE_MATURE_MATCH_SMALL_THAN_14": 4, "FAIL_STRUCTURE_MATURE_STAR_OVERLAP": 5, "FAIL_STRUCTURE_STAR_OUT_OF_FOLD_REGION": 6,
           "FAIL_STRUCTURE_STAR_NOT_IN_ONE_ARM": 7, "FAIL_STRUCTURE_TOO_MANY_BULGE_OR_LOOP": 8, "FAIL_STRUCTURE_MAX_BULGE_LARGE_THAN_2": 9,
           "FAIL_STRUCTURE_TOTAL_LOOP_SIZE_LARGER_THAN_5": 10, "FAIL_STRUCTURE_NUM_BULGE_MORE_THAN_2": 11}
PER_SAMPLE = ("reads_pre", "reads_mature", "reads_star", "reads_antisense", "reads_mature_isoform", "reads_mature_inside",
              "bases_with_reads_start", "ratio_bases_with_reads_start", "reads_star_imperfect")


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
def member_reads(records, tid, ws, we):
    """The reads gen_mapinfo_each_sample keeps for a window (MP:2021): those of the contig that start at or after ws and end at or before we."""
    r = records[records["tid"] == tid]
    pos, ln = r["pos"].astype(np.int64), r["len"].astype(np.int64)
    r = r[(pos >= ws) & (pos + ln <= we)]
    return [(int(x["pos"]), int(x["len"]), int(x["strand"]), int(x["sample"]), int(x["depth"])) for x in r]


def expression(reads, n_samples, fold_s, fold_e, m0, m1, star_s, star_e, strand, allow_3nt):
    """check_expression_new (MP:2037-2163) on `reads` = member_reads(...): the reference's result dict without its read lists, the per-sample
    dicts as the list `samples`; {"raises": "ZeroDivisionError"} where the reference divides by a depth of zero (MP:2156)."""
    mature_len, star_len, pre_len = m1 - m0, star_e - star_s, fold_e - fold_s
    S = [dict(reads_pre=0, reads_mature=0, reads_star=0, reads_antisense=0, reads_mature_isoform=0, reads_mature_inside=0,
              bases_with_reads_start=0) for _ in range(n_samples)]
    if allow_3nt:
        for s in S:
            s["reads_star_imperfect"] = [0, 0, 0]
    starts = set()          # (start position, sample) with a read on the locus strand: one count each, credited to the LAST sample (MP:2068)
    for pos, ln, st, sm, depth in reads:
        if not (fold_s <= pos < fold_e):          # MP:2064
            continue
        d = S[sm]
        if st != strand:
            d["reads_antisense"] += depth
            continue
        starts.add((pos, sm))
        d["reads_pre"] += depth
        if pos == m0 and ln == mature_len:
            d["reads_mature"] += depth
        if pos == star_s and ln == star_len:
            d["reads_star"] += depth
        if abs(pos - m0) <= 3 and abs(ln - mature_len) <= 3:
            d["reads_mature_isoform"] += depth
        if pos >= m0 and pos + ln <= m1:
            d["reads_mature_inside"] += depth
        if allow_3nt:
            if pos == star_s and ln == star_len + 1:
                d["reads_star_imperfect"][0] += depth
            elif pos - 1 == star_s and ln == star_len - 1:
                d["reads_star_imperfect"][1] += depth
            elif pos - 1 == star_s and ln == star_len:
                d["reads_star_imperfect"][2] += depth
    S[n_samples - 1]["bases_with_reads_start"] = len(starts)
    o = {"samplenames": ["s%d" % k for k in range(n_samples)]}
    o["total_depth_just_this_strand"] = sum(s["reads_pre"] for s in S)
    o["total_depth_anti"] = sum(s["reads_antisense"] for s in S)
    o["total_depth_mature"] = sum(s["reads_mature"] for s in S)
    o["total_depth_isoform"] = sum(s["reads_mature_isoform"] for s in S)
    star = sum(s["reads_star"] for s in S)
    o["total_depth_star"] = star
    imp = [sum(s["reads_star_imperfect"][i] for s in S) if allow_3nt else 0 for i in range(3)]
    o["total_depth_imperfect_star"] = imp
    o["mature_depth_each_sample"] = [s["reads_mature"] for s in S]
    for s in S:
        s["ratio_bases_with_reads_start"] = float(s["bases_with_reads_start"]) / pre_len
    o["mature_star_distance"] = star_s - m1 if star_s > m1 else m0 - star_e
    max_imp = 0
    if star == 0 and allow_3nt:
        max_imp = max(imp)
        if max_imp == 0:
            o["imperfect_star_start"] = 0
            o["max_imperfect_star"] = 0
        else:
            which = imp.index(max_imp)
            o["imperfect_star_start"] = star_s + (0 if which == 0 else 1)
            o["imperfect_star_end"] = star_e + (0 if which == 1 else 1)
            o["max_imperfect_star"] = max_imp
            o["imperfect_star_which"] = which
    o["samples"] = S
    this = o["total_depth_just_this_strand"]
    if this == 0:
        return {"raises": "ZeroDivisionError"}
    o["mature_star_ratio_total"] = float(o["total_depth_mature"] + max(star, max_imp)) / this
    o["mature_star_ratio_total_both_strand"] = float(o["total_depth_mature"] + max(star, max_imp)) / (this + o["total_depth_anti"])
    o["mature_iso_star_ratio_total"] = float(o["total_depth_isoform"] + max(star, max_imp)) / this
    if "max_imperfect_star" in o:
        o["total_depth_star"] = max(star, max_imp)
    return o


def counters(reads, n_samples, fold_s, fold_e, m0, m1, star_s, star_e, strand, allow_3nt):
    """The numbers of a pair that exist whether or not the reference's divisions go through (the nine counters of a -d record, the per-sample mature
    depths): the same loop as `expression`, kept apart from it so that a record can be stated for the no-read exception too."""
    c = dict(this=0, anti=0, mature=0, iso=0, star=0, imp=[0, 0, 0], each=[0] * n_samples)
    for pos, ln, st, sm, depth in reads:
        if not (fold_s <= pos < fold_e):
            continue
        if st != strand:
            c["anti"] += depth
            continue
        c["this"] += depth
        if pos == m0 and ln == m1 - m0:
            c["mature"] += depth
            c["each"][sm] += depth
        if pos == star_s and ln == star_e - star_s:
            c["star"] += depth
        if abs(pos - m0) <= 3 and abs(ln - (m1 - m0)) <= 3:
            c["iso"] += depth
        if allow_3nt:
            if pos == star_s and ln == star_e - star_s + 1:
                c["imp"][0] += depth
            elif pos - 1 == star_s and ln == star_e - star_s - 1:
                c["imp"][1] += depth
            elif pos - 1 == star_s and ln == star_e - star_s:
                c["imp"][2] += depth
    return c


def decide(e, allow_no_star):
    """The pass / fail tree of check_loci (MP:2279-2341) on a result of `expression` -> the flag word of mirp_predict_reasons."""
    if "raises" in e:
        return 256
    if e["mature_star_distance"] <= 4:
        return 1
    if e["total_depth_star"] > 0:
        return 2 if e["mature_star_ratio_total"] < 0.2 else 128
    if not allow_no_star:
        return 4
    if any(s["ratio_bases_with_reads_start"] > 0.5 for s in e["samples"]):
        return 8
    each = e["mature_depth_each_sample"]
    expressed_all = len([x for x in each if x > 0]) == len(each)
    if e["mature_iso_star_ratio_total"] >= 0.8 and (expressed_all or e["total_depth_mature"] >= 1000):
        return 128
    return (16 if e["mature_iso_star_ratio_total"] < 0.8 else 0) | (32 if e["total_depth_mature"] <= 100 else 0) | (0 if expressed_all else 64)


def structures_of(case):
    """[(line, ss_off, ss_len, normalised energy, fold start)] in the order of get_structures_next_extendregion (MP:1568-1589)."""
    out = []
    for k, (ss, start, energy) in enumerate(case["lines"]):
        if len(ss) < MINLEN:
            continue
        ne = (energy / 100.0) / len(ss)
        for off, ln in case["pieces"][k]:
            out.append((k, off, ln, ne, start + off))
    return out


def window_truth(case, geometry, records, allow_3nt, allow_no_star):
    """What check_loci yields for the case's window: {"n_structs", "any_in_range", "pairs": {(mature index, structure index): pair}, "mirnas": [...]}.
    pair = {"code", "flags", "geom", "expr", "counters"}; a miRNA entry is a dict with MirpMirna's field names (depths already saturated)."""
    w = case["window"]
    sts = structures_of(case)
    mats = case["matures"]
    out = {"n_structs": len(sts), "any_in_range": int(any(MIN_MATURE <= m[1] - m[0] <= MAX_MATURE for m in mats)), "pairs": {}, "mirnas": []}
    if not sts or not out["any_in_range"]:
        return out
    reads = member_reads(records, w["tid"], w["ws"], w["we"])
    cache = {}
    order = sorted(range(len(mats)), key=lambda k: -mats[k][3])          # stable, depth descending (MP:2241)
    for mi in order:
        m0, m1, strand, _ = mats[mi]
        if m1 - m0 < MIN_MATURE or m1 - m0 > MAX_MATURE:
            continue
        lowest, best = 0.0, None
        for si, (line, off, ln, ne, fstart) in enumerate(sts):
            ss = case["lines"][line][0][off:off + ln]
            key = (ss, m0, m1, fstart, strand)
            if key not in cache:
                g = geometry(ss, m0, m1, fstart, w["ws"], w["we"], strand)
                if isinstance(g, str):
                    cache[key] = {"code": MS_CODE[g], "flags": 0, "geom": None}
                else:
                    star_s, star_e, fold_s, fold_e = g
                    e = expression(reads, case["n_samples"], fold_s, fold_e, m0, m1, star_s, star_e, strand, allow_3nt)
                    c = counters(reads, case["n_samples"], fold_s, fold_e, m0, m1, star_s, star_e, strand, allow_3nt)
                    c["distance"] = star_s - m1 if star_s > m1 else m0 - star_e
                    cache[key] = {"code": 0, "flags": decide(e, allow_no_star), "geom": (star_s, star_e, fold_s, fold_e), "expr": e, "counters": c}
            p = cache[key]
            out["pairs"][(mi, si)] = p
            if ne > lowest or p["flags"] != 128:          # MP:2251; the kernel evaluates such a pair all the same, it just cannot win
                continue
            e = p["expr"]
            star_s, star_e, fold_s, fold_e = p["geom"]
            has_star = e["total_depth_star"] > 0
            reserved = 0
            if "max_imperfect_star" in e:
                reserved = 1 | ((e["imperfect_star_which"] + 1) << 1 | 8 if "imperfect_star_which" in e else 0)
                if has_star:
                    star_s, star_e = e["imperfect_star_start"], e["imperfect_star_end"]
            best = dict(window=case["index"], tid=w["tid"], fold_s=fold_s, fold_e=fold_e, mat_s=m0, mat_e=m1, star_s=star_s, star_e=star_e,
                        strand=strand, has_star=int(has_star), line=line, ss_off=off, ss_len=ln, reserved=reserved,
                        total_depth_mature=min(e["total_depth_mature"], I32_MAX), total_depth_star=min(e["total_depth_star"], I32_MAX),
                        depth64=(e["total_depth_mature"], e["total_depth_star"]))
            lowest = ne
        if best is not None and len(out["mirnas"]) < MAX_MIRNA:
            out["mirnas"].append(best)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry
def hand_hairpin(loop, pairs=30):
    """`pairs` stacked pairs around a loop of `loop` bases, a stem-loop for loop >= 3."""
    return "(" * pairs + "." * loop + ")" * pairs


def local_to_genome(l0, l1, strand, ws, we, foldstart):
    """Inverse of pos_genome_2_local (MP:1727-1768) for a mature at [l0, l1) of a structure that starts at 1-based offset foldstart of the window."""
    if strand == 0:
        return ws + foldstart - 1 + l0, ws + foldstart - 1 + l1
    return we - foldstart + 1 - l1, we - foldstart + 1 - l0


def golden_hairpins():
    """Four stem-loops from the passing `whole == 0` cases of struct_rules.json.gz: (strand, arm of the mature) in every combination, at most 88
    characters, mature and star at least 5 apart and the star clear of the fold's ends -> [(ss, l0, l1, strand)]."""
    with gzip.open(os.path.join(GOLD, "struct_rules.json.gz"), "rt") as f:
        g = json.load(f)
    picks = {}
    for c in g["maturestar"]:
        r = c["result"].get("ok")
        if c["whole"] != 0 or not isinstance(r, list) or not (MINLEN <= len(c["ss"]) <= 88):
            continue
        m0, m1 = c["mature"]
        star_s, star_e, fold_s, fold_e = r[:4]
        dist = star_s - m1 if star_s > m1 else m0 - star_e
        if dist < 5 or min(star_s, m0) - fold_s < 5 or fold_e - max(star_e, m1) < 5 or not (20 <= m1 - m0 <= 22):
            continue
        strand = 1 if c["strand"] == "-" else 0
        key = (strand, bool(r[5]))
        if key in picks:
            continue
        if strand == 0:
            l0 = m0 - c["regionstart"] - c["foldstart"] + 1
        else:
            l0 = c["regionend"] - m1 - c["foldstart"] + 1
        picks[key] = (c["ss"], l0, l0 + m1 - m0, strand)
    assert len(picks) == 4
    return [picks[k] for k in sorted(picks)]


class Geom:
    """One placed hairpin: window, line start, mature; star and fold region from `geometry`."""

    def __init__(self, name, ss, l0, l1, strand, foldstart, tail, ws, geometry):
        n = len(ss)
        self.name, self.ss, self.strand, self.foldstart, self.n = name, ss, strand, foldstart, n
        self.ws, self.we = ws, ws + foldstart - 1 + n + tail
        self.m0, self.m1 = local_to_genome(l0, l1, strand, self.ws, self.we, foldstart)
        g = geometry(ss, self.m0, self.m1, foldstart, self.ws, self.we, strand)
        assert not isinstance(g, str), (name, g)
        self.star_s, self.star_e, self.fold_s, self.fold_e = g
        self.ml, self.sl = self.m1 - self.m0, self.star_e - self.star_s
        self.distance = self.star_s - self.m1 if self.star_s > self.m1 else self.m0 - self.star_e

    def free_starts(self, length=18):
        """Start positions of the fold region at which a read of `length` stays in the window and touches neither the isoform box nor the star
        or its imperfect variants, in ascending order."""
        return [p for p in range(max(self.fold_s, self.ws), self.fold_e)
                if p + length <= self.we and abs(p - self.m0) > 3 and p not in (self.star_s, self.star_s + 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# read templates: name -> function(Geom) -> (n_samples, [(pos, len, depth, sample, same strand?)])
def _mature(g, depth, sample=0):
    return (g.m0, g.ml, depth, sample, True)


def _star(g, depth, sample=0):
    return (g.star_s, g.sl, depth, sample, True)


def _other(g, depth, k=0, sample=0, same=True):
    return (g.free_starts()[k], 18, depth, sample, same)


def _both(g, total):
    return [_mature(g, total - total // 2, 0), _mature(g, total // 2, 1)]


def _starts(g, n_starts):
    """No star, 1,000 mature reads in two samples (2 starts), then other starts up to n_starts: three positions read in both samples (2 each),
    the rest in one; antisense reads on further positions, which count nothing."""
    free = g.free_starts()
    reads = _both(g, 1000)
    left, k = n_starts - 2, 0
    while left > 0:
        if k < 3 and left >= 2:
            reads += [(free[k], 18, 1, 0, True), (free[k], 18, 1, 1, True)]
            left -= 2
        else:
            reads.append((free[k], 18, 1, k & 1, True))
            left -= 1
        k += 1
    reads += [(p, 18, 7, 0, False) for p in free[k:k + 5]]
    return reads


def _boundary(g):
    """A passing star pair plus one read on each side of every membership boundary, depths in powers of two so that the sum names the members."""
    reads = [_mature(g, 4096), _star(g, 2048)]
    d = 1
    for pos, ln in ((g.ws - 1, 18), (g.ws, 18), (g.we - 18, 18), (g.we - 18, 19), (g.fold_s - 1, 18), (g.fold_s, 18), (g.fold_e - 1, 15), (g.fold_e, 15),
                    (g.fold_e - 1, g.we - g.fold_e + 1), (g.fold_e - 1, g.we - g.fold_e + 2)):
        if ln >= 1:
            reads.append((pos, ln, d, 0, True))
        d *= 2
    return reads


TEMPLATES = {
    "star_2_of_10": lambda g: (2, [_mature(g, 1), _star(g, 1), _other(g, 8)]),
    "star_1_of_10": lambda g: (2, [_star(g, 1), _other(g, 9)]),
    "star_2_of_11": lambda g: (2, [_mature(g, 1), _star(g, 1), _other(g, 9)]),
    "nostar_pass": lambda g: (2, _both(g, 40) + [_other(g, 3)]),
    "starts_half": lambda g: (2, _starts(g, g.n // 2)),
    "starts_half_plus_1": lambda g: (2, _starts(g, g.n // 2 + 1)),
    "iso_4_of_5": lambda g: (2, _both(g, 4) + [_other(g, 1)]),
    "iso_3_of_4": lambda g: (2, _both(g, 3) + [_other(g, 1)]),
    "iso_400_of_500": lambda g: (2, _both(g, 400) + [_other(g, 100)]),
    "iso_400_of_501": lambda g: (2, _both(g, 400) + [_other(g, 101)]),
    "mature_100_one_sample": lambda g: (2, [_mature(g, 100)]),
    "mature_101_one_sample": lambda g: (2, [_mature(g, 101)]),
    "mature_100_low_ratio": lambda g: (2, _both(g, 100) + [_other(g, 30)]),
    "mature_101_low_ratio": lambda g: (2, _both(g, 101) + [_other(g, 30)]),
    "mature_999_one_sample": lambda g: (2, [_mature(g, 999)]),
    "mature_1000_one_sample": lambda g: (2, [_mature(g, 1000)]),
    "flags_16_32_64": lambda g: (2, [_mature(g, 50), _other(g, 50)]),
    "isoform_box": lambda g: (2, _both(g, 80) + [(g.m0 - 3, g.ml - 3, 1, 0, True), (g.m0 - 3, g.ml + 3, 2, 1, True), (g.m0 + 3, g.ml - 3, 4, 0, True),
                                                  (g.m0 + 3, g.ml + 3, 8, 1, True), (g.m0 - 4, g.ml, 16, 0, True), (g.m0 + 4, g.ml, 32, 0, True),
                                                  (g.m0, g.ml - 4, 64, 0, True), (g.m0, g.ml + 4, 128, 0, True)]),
    "imperfect_0": lambda g: (2, [_mature(g, 10), (g.star_s, g.sl + 1, 3, 0, True)]),
    "imperfect_1": lambda g: (2, [_mature(g, 10), (g.star_s + 1, g.sl - 1, 3, 1, True)]),
    "imperfect_2": lambda g: (2, [_mature(g, 10), (g.star_s + 1, g.sl, 3, 0, True)]),
    "imperfect_tie_0_1": lambda g: (2, [_mature(g, 10), (g.star_s, g.sl + 1, 3, 0, True), (g.star_s + 1, g.sl - 1, 3, 0, True), (g.star_s + 1, g.sl, 1, 0, True)]),
    "imperfect_tie_1_2": lambda g: (2, [_mature(g, 10), (g.star_s, g.sl + 1, 1, 0, True), (g.star_s + 1, g.sl - 1, 2, 0, True), (g.star_s + 1, g.sl - 1, 1, 1, True),
                                        (g.star_s + 1, g.sl, 3, 0, True)]),
    "imperfect_beside_perfect": lambda g: (2, [_mature(g, 10), _star(g, 2), (g.star_s, g.sl + 1, 5, 0, True), (g.star_s + 1, g.sl - 1, 5, 0, True),
                                               (g.star_s + 1, g.sl, 5, 0, True)]),
    "imperfect_too_few": lambda g: (2, [_mature(g, 1), (g.star_s + 1, g.sl, 1, 0, True), _other(g, 9)]),
    "only_antisense": lambda g: (2, [(g.m0, g.ml, 50, 0, False), _other(g, 5, same=False)]),
    "no_reads": lambda g: (2, []),
    "boundaries": lambda g: (2, _boundary(g)),
    "deep_no_star": lambda g: (3, [_mature(g, 1200000000, 0), _mature(g, 1200000000, 1), _other(g, 5, sample=2)]),
    "deep_star": lambda g: (3, [_mature(g, 1200000000, 0), _mature(g, 1200000000, 1), _star(g, 1100000000, 0), _star(g, 1100000000, 2)]),
}
CLOSE_TEMPLATES = ("star_2_of_10", "nostar_pass")          # on the hairpins whose mature and star are 4 apart: flag 1 whatever the reads
SAMPLE_COUNTS = (1, 2, 32, 33, 64, 65, 255)
SAMPLE_EDGES = (0, 31, 32, 63, 64)


def _sample_reads(g, n_samples, missing):
    """No star; 999 mature reads spread over every sample but `missing` (None: over all of them), which has an isoform read in their place."""
    have = [s for s in range(n_samples) if s != missing]
    reads = []
    if have:
        each, rest = 999 // len(have), 999 % len(have)
        reads = [_mature(g, each + (rest if k == 0 else 0), s) for k, s in enumerate(have)]
    if missing is not None:
        reads.append((g.m0 + 1, g.ml, 2, missing, True))
    return reads


def build(geometry):
    """-> (cases, records).  A case: {"name", "index", "n_samples", "window": {tid, ws, we, strand}, "lines": [(ss, start, energy)], "pieces":
    [[(off, len)] per line], "matures": [(start, end, strand, depth)], "tags": {...}}; records: ALN_DTYPE, (tid, pos)-sorted, of all cases."""
    cases, reads = [], []
    cursor = [10000, 1010000]          # next free coordinate per contig; contig 1's windows lie beyond all of contig 0's (decoys, below)

    def place(name, ss, l0, l1, strand, foldstart, tail):
        k = len(cases)
        tid = k & 1
        gap = 1 if (k >> 1) & 1 else 37          # every other window of a contig follows its neighbour at once: that one's reads lie directly before ws / after we
        g = Geom(name, ss, l0, l1, strand, foldstart, tail, cursor[tid] + gap, geometry)
        cursor[tid] = g.we
        return tid, g

    def add(name, tid, g, n_samples, rd, lines=None, pieces=None, matures=None, tags=None):
        lines = lines if lines is not None else [(g.ss, g.foldstart, -3000)]
        c = {"name": name, "index": len(cases), "n_samples": n_samples, "window": {"tid": tid, "ws": g.ws, "we": g.we, "strand": g.strand},
             "lines": lines, "pieces": pieces if pieces is not None else [[(0, len(l[0]))] for l in lines],
             "matures": matures if matures is not None else [(g.m0, g.m1, g.strand, 100)], "tags": dict(tags or {}, geom=g.name)}
        cases.append(c)
        for pos, ln, depth, sample, same in rd:
            reads.append((tid, pos, depth, ln, g.strand if same else 1 - g.strand, sample))
        # a read of the OTHER contig at the mature's own position and length
        reads.append((1 - tid, g.m0, 100000, g.ml, g.strand, 0))
        return c

    hp = golden_hairpins()
    shapes = []          # (name, ss, l0, l1, strand, foldstart, tail)
    for k, (ss, l0, l1, strand) in enumerate(hp):
        shapes.append(("golden%d" % k, ss, l0, l1, strand, 1 if k & 1 else 8, 0 if k & 1 else 30))
    far, close = hand_hairpin(5), hand_hairpin(4)
    for strand in (0, 1):
        shapes.append(("hand5_5p_%d" % strand, far, 9, 31, strand, 1, 30))           # 5' arm, one unpaired base at the loop
        shapes.append(("hand5_3p_%d" % strand, far, 36, 58, strand, 8, 0))           # 3' arm
    close_shapes = []
    for strand in (0, 1):
        close_shapes.append(("hand4_5p_%d" % strand, close, 9, 31, strand, 3, 12))
        close_shapes.append(("hand4_3p_%d" % strand, close, 35, 57, strand, 3, 12))

    for sh in shapes:
        for tname, fn in TEMPLATES.items():
            tid, g = place(sh[0], *sh[1:])
            assert g.distance >= 5, (sh[0], g.distance)
            ns, rd = fn(g)
            add("%s/%s" % (sh[0], tname), tid, g, ns, rd, tags={"template": tname})
    for sh in close_shapes:
        for tname in CLOSE_TEMPLATES:
            tid, g = place(sh[0], *sh[1:])
            assert g.distance == 4, (sh[0], g.distance)
            ns, rd = TEMPLATES[tname](g)
            add("%s/%s" % (sh[0], tname), tid, g, ns, rd, tags={"template": tname, "close": True})

    # ---- samples: the sample without mature reads at every word edge of the kernel's sample set
    # (every sample's mature read is a start position of its own, MP:2066-2068: 254 of them need a precursor of 510 nt and more to stay at or
    # below one half -- the hairpin with a long dangling end, still a stem-loop)
    long_shape = ("long5_5p", far + "." * 455, 9, 31, 0, 1, 0)
    for ns in SAMPLE_COUNTS:
        for missing in [None] + sorted(set(e for e in SAMPLE_EDGES + (ns - 1,) if e < ns)):
            tid, g = place(*long_shape)
            add("samples/%d/%s" % (ns, missing), tid, g, ns, _sample_reads(g, ns, missing), tags={"samples": ns, "missing": missing})

    # ---- selection among structures
    passing = lambda g: [_mature(g, 10), _star(g, 2)]
    sh = shapes[4]
    tid, g = place(*sh)
    add("select/70_equal", tid, g, 2, passing(g), lines=[(g.ss, g.foldstart, -3000)] * 70, tags={"select": "last"})
    tid, g = place(*sh)
    add("select/70_lower_at_5", tid, g, 2, passing(g), lines=[(g.ss, g.foldstart, -3100 if k == 5 else -3000) for k in range(70)], tags={"select": 5})
    tid, g = place(*sh)
    add("select/energy_0", tid, g, 2, passing(g), lines=[(g.ss, g.foldstart, 0)], tags={"select": "zero"})
    tid, g = place(*sh)
    add("select/energy_positive", tid, g, 2, passing(g), lines=[(g.ss, g.foldstart, 100)], tags={"select": "positive"})
    tid, g = place(*sh)
    add("select/positive_after_negative", tid, g, 2, passing(g), lines=[(g.ss, g.foldstart, -100), (g.ss, g.foldstart, 100)], tags={"select": "positive_last"})
    # a bifurcated line: two stem-loops side by side, which filter_ss cuts into two pieces of the same normalised energy.  The pieces hold one
    # stem each, so a mature lies in one of them and no mature passes on both; the tie the pieces take part in is set up with a second line of
    # the same length and energy that holds the first stem alone.  Structure order: that line, piece 0, piece 1 -> piece 0 wins for the mature in
    # the first stem (the later of two equals, and not the last structure), piece 1 for the mature in the second.
    stem = hand_hairpin(5, 25)
    two = stem + "..." + stem
    for strand in (0, 1):
        k = len(cases)
        tid = k & 1
        ws = cursor[tid] + 11
        we = ws + len(two) + 9
        cursor[tid] = we
        ma = local_to_genome(4, 26, strand, ws, we, 1)
        mb = local_to_genome(len(stem) + 3 + 4, len(stem) + 3 + 26, strand, ws, we, 1)
        ga = geometry(two[:len(stem) + 3], ma[0], ma[1], 1, ws, we, strand)
        gb = geometry(two[len(stem):], mb[0], mb[1], 1 + len(stem), ws, we, strand)
        assert not isinstance(ga, str) and not isinstance(gb, str)
        c = {"name": "select/bifurcated_%d" % strand, "index": k, "n_samples": 2, "window": {"tid": tid, "ws": ws, "we": we, "strand": strand},
             "lines": [(stem + "." * (len(two) - len(stem)), 1, -4000), (two, 1, -4000)],
             "pieces": [[(0, len(two))], [(0, len(stem) + 3), (len(stem), len(two) - len(stem))]],
             "matures": [(mb[0], mb[1], strand, 90), (ma[0], ma[1], strand, 100)], "tags": {"select": "bifurcated", "geom": "two_stems"}}
        cases.append(c)
        for (m0, m1), (s0, s1) in ((ma, ga[:2]), (mb, gb[:2])):
            reads.append((tid, m0, 10, m1 - m0, strand, 0))
            reads.append((tid, s0, 2, s1 - s0, strand, 1))
        reads.append((1 - tid, ma[0], 100000, ma[1] - ma[0], strand, 0))

    # ---- matures
    def variants(g, shifts, lens):
        return [(g.m0 + dx, g.m0 + dx + ln) for dx in shifts for ln in lens]

    def variant_reads(vs, depth_of):
        return [(a, b - a, depth_of(k), s, True) for k, (a, b) in enumerate(vs) for s in (0, 1)]

    for sh in (shapes[0], shapes[3], shapes[4]):
        def two_matures(g):
            b = (g.m0 + 1, g.m1 + 1)
            rd = [_mature(g, 10), _star(g, 2), (b[0], g.ml, 10, 1, True)]
            gb = geometry(g.ss, b[0], b[1], g.foldstart, g.ws, g.we, g.strand)
            if not isinstance(gb, str):
                rd.append((gb[0], gb[1] - gb[0], 2, 1, True))
            return b, rd

        tid, g = place(*sh)
        b, rd = two_matures(g)
        add("matures/equal_depths", tid, g, 2, rd, matures=[(b[0], b[1], g.strand, 100), (g.m0, g.m1, g.strand, 100)], tags={"matures": "equal"})
        tid, g = place(*sh)
        b, rd = two_matures(g)
        add("matures/out_of_range_between", tid, g, 2, rd,
            matures=[(g.m0, g.m1, g.strand, 100), (g.m0, g.m0 + 26, g.strand, 90), (b[0], b[1], g.strand, 80)], tags={"matures": "between"})
        tid, g = place(*sh)
        b, rd = two_matures(g)
        add("matures/none_in_range", tid, g, 2, rd, matures=[(g.m0, g.m0 + 26, g.strand, 90), (g.m0, g.m0 + 17, g.strand, 80)], tags={"matures": "none"})
        # twelve variants inside one another's isoform box, read in both samples: every one passes without a star, the first eight are kept
        tid, g = place(*sh)
        vs = variants(g, (0, -1, -2, -3), (g.ml, g.ml - 1, g.ml - 2))
        depth = [50 + ((7 * k) % 12) for k in range(12)]          # distinct, not in input order
        add("matures/twelve", tid, g, 2, variant_reads(vs, lambda k: 5), matures=[(a, b_, g.strand, depth[k]) for k, (a, b_) in enumerate(vs)],
            tags={"matures": "twelve"})
        # seventy matures (more than the kernel's table of 64) on seventy lines (more than it stages): shifts -4 .. 5, lengths 18 .. 24
        heavy = lambda k: 1000 if 0 <= vs[k][0] - g.m0 <= 3 and g.ml - 1 <= vs[k][1] - vs[k][0] <= g.ml else 1
        if sh is shapes[0]:          # once: 4,900 pairs
            tid, g = place(*sh)
            vs = variants(g, range(-4, 6), range(18, 25))
            add("matures/seventy_on_70_lines", tid, g, 2, variant_reads(vs, heavy), lines=[(g.ss, g.foldstart, -3000 - (k % 3)) for k in range(70)],
                matures=[(a, b_, g.strand, 500 - ((37 * k) % 70)) for k, (a, b_) in enumerate(vs)], tags={"matures": "seventy"})
        tid, g = place(*sh)
        vs = variants(g, range(-4, 6), range(18, 25))
        add("matures/seventy", tid, g, 2, variant_reads(vs, heavy),
            matures=[(a, b_, g.strand, 500 - ((37 * k) % 70)) for k, (a, b_) in enumerate(vs)], tags={"matures": "seventy_one_line"})

    assert cursor[0] < 1000000
    rec = np.array(reads, dtype=ALN_DTYPE)
    rec = rec[np.lexsort((np.arange(len(rec)), rec["pos"], rec["tid"]))]
    return cases, rec


# ---------------------------------------------------------------------------------------------------------------------------------
# the golden
def geometry_key(ss, m0, m1, foldstart, ws, we, strand):
    return "%s|%d|%d|%d|%d|%d|%d" % (ss, m0, m1, foldstart, ws, we, strand)


_golden = None


def load_golden():
    global _golden
    if _golden is None:
        with gzip.open(os.path.join(GOLD, "expr_rules.json.gz"), "rt") as f:
            _golden = json.load(f)
    return _golden


def golden_geometry(ss, m0, m1, foldstart, ws, we, strand):
    """get_maturestar_info's answer as the golden recorded it: the fail string, or (star_s, star_e, fold_s, fold_e)."""
    g = load_golden()["geometry"][geometry_key(ss, m0, m1, foldstart, ws, we, strand)]
    return g if isinstance(g, str) else tuple(g)


_built = None


def planted():
    """(cases, records) built on the golden's geometry, once per process; the golden's own copy of the inputs must equal what is built now."""
    global _built
    if _built is None:
        cases, rec = build(golden_geometry)
        g = load_golden()
        assert g["cases"] == json.loads(json.dumps(cases)), "tests/golden/expr_rules.json.gz is stale: run tests/golden/tools/gen_expr_golden.py"
        assert g["records"] == [[int(x) for x in r] for r in rec.tolist()], "tests/golden/expr_rules.json.gz is stale"
        _built = (cases, rec)
    return _built


def batch(cases):
    """The arrays mirp_predict_batch takes for `cases`: windows, matures, fold output (every window at MAX_LINES lines of `stride` bytes: STRIDE, or
    what the longest line needs)."""
    from mir_prefer_amd import records
    n = len(cases)
    W = np.zeros(n, dtype=records.WINDOW_DTYPE)
    M = np.zeros(sum(len(c["matures"]) for c in cases), dtype=records.MATURE_DTYPE)
    lines = np.zeros((n, MAX_LINES), dtype=[("start", "<i4"), ("len", "<i4"), ("energy", "<i4"), ("printed", "<i4")])
    stride = max([STRIDE] + [(len(l[0]) + 7) // 8 * 8 for c in cases for l in c["lines"]])
    ss = np.zeros((n, MAX_LINES, stride), dtype=np.uint8)
    nl = np.zeros(n, dtype=np.int32)
    off = 0
    for k, c in enumerate(cases):
        w = c["window"]
        W[k] = (w["tid"], w["ws"], w["we"], w["strand"], w["ws"], w["we"], 0, 0, 0, len(c["matures"]), 0, off, 0, w["we"] - w["ws"], 0)
        for m in c["matures"]:
            M[off] = m
            off += 1
        nl[k] = len(c["lines"])
        for j, (s, start, energy) in enumerate(c["lines"]):
            b = s.encode()
            lines[k, j] = (start, len(b), energy, 1)
            ss[k, j, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return W, M, {"lines": lines, "ss": ss, "n_lines": nl, "stride": stride, "max_lines": MAX_LINES}


_truth = {}


def truth(allow_3nt, allow_no_star):
    """window_truth of every planted case under one parameter combination, computed once per process and shared by the tests."""
    key = (int(allow_3nt), int(allow_no_star))
    if key not in _truth:
        cases, rec = planted()
        _truth[key] = [window_truth(c, golden_geometry, rec, key[0], key[1]) for c in cases]
    return _truth[key]


def pair_key(index, m0, m1, geo, strand, allow_3nt):
    """Key of a pair in the golden's `pairs` (the generator writes the same)."""
    return "%d|%d|%d|%d|%d|%d|%d|%d|%d" % ((index, m0, m1) + tuple(geo) + (strand, int(allow_3nt)))
