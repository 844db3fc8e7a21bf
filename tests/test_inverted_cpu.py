"""CPU tests of the inverted-repeat search: the two restatements of tests/inverted_restatement.py against each other and against a
witness that shares no code with them, the definition's pins, ties, candidate rule and selection, and the host side of mir_prefer_amd.inverted
(options, writers, the header's declarations).  The device is compared with the restatement in test_inverted_gpu.py."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import inverted_restatement as R
from tests.test_targets_cpu import ROOT

S6 = dict(min_score=6, max_span=8)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def plant(genome, rng, pos, arm, loop, subs=0, deleted=False):
    left = [rng.choice("ACGT") for _ in range(arm)]
    right = list(revcomp("".join(left)))
    for _ in range(subs):
        p = rng.randrange(3, arm - 3)
        right[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[right[p]]
    if deleted:
        del right[arm // 2]
    genome[pos:pos + arm] = left
    genome[pos + arm + loop:pos + arm + loop + len(right)] = right


def brief(recs):
    return [(r["contig"], r["score"], r["left_start"], r["left_end"], r["right_start"], r["right_end"], R.structure(r["ops"])) for r in recs]


# ---------------------------------------------------------------------------------------------------- the recurrence
def test_cells_and_levels_agree():
    rng = random.Random(1)
    for trial in range(60):
        n = rng.choice((1, 2, 3, 7, 8, 9, 30, 64, 65, 150))
        s = rand_seq(rng, n, rng.choice(("AT", "ACGT", "ACGTN", "CG")))
        o = dict(max_span=rng.choice((8, 9, 16, 40, 200)), match=rng.randint(1, 10), mismatch=rng.randint(1, 10), gap=rng.randint(1, 50),
                 min_score=rng.choice((1, 6, 20)))
        H = R.h_cells(s, o["max_span"], o["match"], o["mismatch"], o["gap"])
        L = R.h_levels(s, o["max_span"], o["match"], o["mismatch"], o["gap"])
        for i in range(1, n + 1):
            for j in range(i + 1, n + 1):
                want = H.get((i, j), 0)
                assert (int(L[j - i + 1, i - 1]) if j - i < o["max_span"] else 0) == want
        assert R.rows_of_cells(H, n, o["max_span"]) == R.rows_of_levels(L, n)
        a, b = {}, {}
        assert R.find([s], "cells", a, **o) == R.find([s], "levels", b, **o) and a == b


def witness(s, i, j, match, mismatch, gap):
    """the best sum over every outward path that ends at (i, j), by walking all of them inwards; the empty path scores 0"""
    pairs = ("AT", "TA", "CG", "GC")

    def walk(a, b):
        if b <= a:
            return 0
        here = match if s[a - 1] + s[b - 1] in pairs else -mismatch
        return max(0, here + walk(a + 1, b - 1), walk(a + 1, b) - gap, walk(a, b - 1) - gap)

    # the three moves out of (i, j) itself: a path through (i, j) has one of them as its last step
    if j <= i:
        return 0
    here = match if s[i - 1] + s[j - 1] in pairs else -mismatch
    return max(0, here + walk(i + 1, j - 1), walk(i + 1, j) - gap, walk(i, j - 1) - gap)


def all_paths_best(s, i, j, match, mismatch, gap):
    """the same by explicit enumeration: every sequence of moves from (i, j) inwards, every prefix of it a path"""
    pairs = ("AT", "TA", "CG", "GC")
    best, stack = 0, [(i, j, 0)]
    while stack:
        a, b, score = stack.pop()
        best = max(best, score)
        if b <= a:
            continue
        stack.append((a + 1, b - 1, score + (match if s[a - 1] + s[b - 1] in pairs else -mismatch)))
        stack.append((a + 1, b, score - gap))
        stack.append((a, b - 1, score - gap))
    return best


def test_h_is_the_best_outward_path():
    rng = random.Random(2)
    for trial in range(120):
        n = rng.randint(2, 9)
        s = rand_seq(rng, n, "ACGTN" if trial % 2 else "AT")
        match, mismatch, gap = rng.randint(1, 10), rng.randint(1, 10), rng.randint(1, 12)
        H = R.h_cells(s, 4096, match, mismatch, gap)
        for i in range(1, n + 1):
            for j in range(i + 1, n + 1):
                assert H[(i, j)] == all_paths_best(s, i, j, match, mismatch, gap) == witness(s, i, j, match, mismatch, gap), (s, i, j)


def test_reverse_complement_mirrors_h():
    rng = random.Random(3)
    for trial in range(20):
        n = rng.randint(2, 60)
        s = rand_seq(rng, n, "ACGTN")
        t = s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))
        D = rng.choice((8, 20, 100))
        H, G = R.h_cells(s, D, 3, 4, 5), R.h_cells(t, D, 3, 4, 5)
        assert all(G[(n + 1 - j, n + 1 - i)] == h for (i, j), h in H.items()) and len(G) == len(H)


def rescore(s, rec, match, mismatch, gap):
    a, b, score = rec["left_start"], rec["right_end"], 0
    for op in rec["ops"]:
        if op in "=X":
            assert (op == "=") == ((s[a - 1], s[b - 1]) in R.PAIRS)
            score += match if op == "=" else -mismatch
            a, b = a + 1, b - 1
        elif op == "L":
            score, a = score - gap, a + 1
        else:
            score, b = score - gap, b - 1
    assert (a - 1, b + 1) == (rec["left_end"], rec["right_start"]) or rec["ops"][-1] in "LR"
    return score


def test_structures_rescore_and_end_in_pairs():
    rng = random.Random(4)
    seen = set()
    for trial in range(30):
        g = [rng.choice("ACGT") for _ in range(400)]
        for k in range(3):
            plant(g, rng, 20 + 130 * k, rng.randint(15, 40), rng.randint(0, 40), subs=rng.randint(0, 3), deleted=bool(k % 2))
        s = "".join(g)
        o = dict(max_span=150, match=rng.randint(2, 5), mismatch=rng.randint(1, 6), gap=rng.randint(1, 8), min_score=12)
        for rec in R.find([s], **o):
            assert rescore(s, rec, o["match"], o["mismatch"], o["gap"]) == rec["score"]
            assert rec["ops"][0] == "=" and rec["ops"][-1] == "="
            assert rec["left_start"] <= rec["left_end"] < rec["right_start"] <= rec["right_end"]
            assert rec["right_end"] - rec["left_start"] + 1 <= o["max_span"]
            seen.update(rec["ops"])
    assert seen == set("=XLR")


# ---------------------------------------------------------------------------------------------------- pins and ties
def test_pins():
    for engine in ("cells", "levels"):
        assert brief(R.find(["ACGT"], engine, **S6)) == [(0, 6, 1, 2, 3, 4, "2=")]
        # GGGAAACCC is 9 nt: at a span of 9 it scores 9 with a loop of 3; at 8 the cell (1, 9) does not exist and the inner part is reported
        assert brief(R.find(["GGGAAACCC"], engine, min_score=6, max_span=9)) == [(0, 9, 1, 3, 7, 9, "3=")]
        assert brief(R.find(["GGGAAACCC"], engine, **S6)) == [(0, 6, 1, 2, 7, 8, "2=")]
        assert brief(R.find(["GGGNCCC"], engine, **S6)) == [(0, 9, 1, 3, 5, 7, "3=")]          # the N is the loop
        assert brief(R.find(["gggnccu", "ACGU"], engine, **S6)) == [(0, 6, 1, 2, 5, 6, "2="), (1, 6, 1, 2, 3, 4, "2=")]
    text = R.tsv_text(["c"], R.find(["ACGT"], **S6))
    assert text == R.TSV_HEADER + "IR_1\tc\t1\t4\t6\t1\t2\t3\t4\t0\t2\t0\t0\t100.00\t2=\n"
    with pytest.raises(ValueError):
        R.find([b"AC\x80T"], **S6)


def test_ties():
    # the row's end: the smallest d among the cells that reach r(i)
    for engine in ("cells", "levels"):
        _, r, dstar, _ = R.scan_contig("GCAC", engine, **S6)
        assert (r[1], dstar[1]) == (3, 1)          # G.C at d = 1 and at d = 3
        _, r, dstar, _ = R.scan_contig("AAAA", engine, **S6)
        assert r[1:] == [0, 0, 0, 0] and dstar[1:] == [0, 0, 0, 0]
    # the traceback: the diagonal before the left base, the left base before the right base (match 2, mismatch 1, gap 1)
    for s, score, ops in (("AATA", 1, "X="), ("ATAA", 1, "X="), ("ATTA", 1, "L="), ("AAATATA", 2, "X=L=")):
        H = R.h_cells(s, 8, 2, 1, 1)
        rec = R.traceback(lambda i, j: H.get((i, j), 0), s, 1, len(s), 2, 1, 1)
        assert (rec["score"], rec["ops"]) == (score, ops)
    # the selection: score descending, then contig, left_start, right_end; a later one yields when an arm shares a position
    def cand(contig, score, ls, le, rs, re_):
        return dict(contig=contig, score=score, left_start=ls, left_end=le, right_start=rs, right_end=re_)
    c = [cand(1, 9, 1, 3, 7, 9), cand(0, 9, 3, 5, 8, 10), cand(0, 9, 1, 3, 20, 22), cand(0, 9, 1, 3, 12, 14), cand(0, 12, 30, 33, 40, 43),
         cand(0, 9, 34, 36, 37, 39), cand(0, 9, 33, 35, 50, 52), cand(0, 9, 44, 45, 60, 61)]
    assert R.select(c) == [c[3], c[4], c[5], c[7], c[0]]


# ---------------------------------------------------------------------------------------------------- candidates and selection
def test_one_mismatch_yields_the_outer_end():
    arm = "ACGGATCCGTAAGCTTGCAT"
    right = list(revcomp(arm))
    right[12] = {"A": "C", "C": "A", "G": "T", "T": "G"}[right[12]]
    s = "CC" + arm + "CACACACA" + "".join(right) + "CC"
    for engine in ("cells", "levels"):
        _, r, dstar, rows = R.scan_contig(s, engine, max_span=100, min_score=15)
        assert 3 in rows and r[3] == 3 * 19 - 4 and 3 + dstar[3] == len(s) - 2
        out = R.find([s], engine, max_span=100, min_score=15)
        assert brief(out) == [(0, 53, 3, 22, 31, 50, "7=1X12=")]


def planted_genome():
    rng = random.Random(7)
    g = [rng.choice("ACGT") for _ in range(3000)]
    spots = ((100, 25, 0, 0, False), (600, 60, 40, 2, False), (1400, 120, 150, 3, True), (2300, 40, 250, 1, False))
    for pos, arm, loop, subs, deleted in spots:
        plant(g, rng, pos, arm, loop, subs, deleted)
    return "".join(g), spots


def test_planted_repeats_are_found_and_nothing_else():
    s, spots = planted_genome()
    st = {}
    out = R.find([s], stats=st, max_span=400)
    assert len(out) == 4 and st["candidates"] < st["rows_above"]
    for rec, (pos, arm, loop, subs, deleted) in zip(out, spots):
        assert abs(rec["left_start"] - (pos + 1)) <= 3 and abs(rec["right_end"] - (pos + 2 * arm + loop - deleted)) <= 3
        assert rec["mismatches"] <= subs and rec["gaps"] == int(deleted)
    assert out == R.find([s], "cells", max_span=400)


def test_microsatellite_is_one_record():
    st = {}
    out = R.find(["AT" * 60], stats=st, max_span=400)
    assert brief(out) == [(0, 180, 1, 60, 61, 120, "60=")] and st["candidates"] > 10
    assert brief(R.find(["AT" * 60], "cells", max_span=400)) == brief(out)


def test_nested_repeat_survives():
    rng = random.Random(8)
    inner_arm, outer_arm = rand_seq(rng, 20), rand_seq(rng, 30)
    inner = inner_arm + "CACAC" + revcomp(inner_arm)
    s = "CC" + outer_arm + "AC" + inner + "CA" * 25 + revcomp(outer_arm) + "CC"          # (off the middle: the outer alignment cannot run through it)
    out = R.find([s], max_span=200, min_score=30)
    assert [(r["score"], r["left_start"], r["right_end"]) for r in out] == [(90, 3, len(s) - 2), (60, 35, 79)]
    assert out[0]["left_end"] < out[1]["left_start"] and out[1]["right_end"] < out[0]["right_start"]


# ---------------------------------------------------------------------------------------------------- the host side of the command
def as_array(recs):
    from mir_prefer_amd import capi
    return np.array([(r["contig"], r["score"], r["left_start"], r["left_end"], r["right_start"], r["right_end"], r["matches"], r["mismatches"], r["gaps"], 0)
                     for r in recs], dtype=capi.INVERTED_DTYPE)


def test_writers_and_gffmask_round_trip(tmp_path):
    from mir_prefer_amd import gffmask, inverted
    s, _ = planted_genome()
    contigs = [s.lower(), "AT" * 60, "GGGuNACCC"]
    names = ["chr1", "sat|2", "tiny"]
    recs = R.find(contigs, max_span=400, min_score=12)
    assert len(recs) >= 6 and {r["contig"] for r in recs} == {0, 1, 2}
    arr, structures = as_array(recs), [R.structure(r["ops"]) for r in recs]
    assert inverted.tsv_table(names, arr, structures) == R.tsv_text(names, recs)
    assert inverted.gff_table(names, arr) == R.gff_text(names, recs)
    assert inverted.fasta_table(names, [c.encode() for c in contigs], arr) == R.fasta_text(names, contigs, recs)
    assert inverted.tsv_table(names, arr[:0], []) == inverted.TSV_HEADER == R.TSV_HEADER
    assert inverted.gff_table(names, arr[:0]) == "##gff-version 3\n" and inverted.fasta_table(names, contigs, arr[:0]) == ""
    lines = R.tsv_text(names, recs).splitlines()[1:]
    assert [l.split("\t")[0] for l in lines] == ["IR_%d" % (k + 1) for k in range(len(recs))]
    assert [(r["contig"], r["left_start"], r["right_end"]) for r in recs] == sorted((r["contig"], r["left_start"], r["right_end"]) for r in recs)
    fasta = R.fasta_text(names, contigs, recs).splitlines()
    assert fasta[-2] == ">IR_%d tiny:1-9 score=12" % len(recs) and fasta[-1] == "GGGUNACCC"
    gff = tmp_path / "x.gff3"
    gff.write_text(inverted.gff_table(names, arr))
    assert all(len(l.split()) == 9 for l in gff.read_text().splitlines()[1:])
    got = gffmask.keep_regions_include(str(gff), minlen=0)
    assert sorted(got) == sorted((names[r["contig"]], r["left_start"] - 1, r["right_end"]) for r in recs)
    assert inverted.output_names("b") == ("b.tsv", "b.gff3", "b.fa")


def test_option_errors_need_no_binding(tmp_path, capsys):
    from mir_prefer_amd import inverted
    f = str(tmp_path / "g.fa")
    o, genomes, base = inverted.parse_args([f, f + "2"])
    assert (o.max_span, o.min_score, o.match, o.mismatch, o.gap, o.device) == (2000, 50, 3, 4, 12, 0)
    assert genomes == [f, f + "2"] and base == f + ".inverted"
    assert inverted.parse_args(["-d", "8", "-s", "1", "--gap", "50", "-o", "out", f])[2] == "out"
    bad = [[], ["-d", "7", f], ["-d", "4097", f], ["-s", "0", f], ["--match", "0", f], ["--match", "11", f], ["--mismatch", "0", f], ["--mismatch", "11", f],
           ["--gap", "0", f], ["--gap", "51", f], ["--device", "-1", f], ["-o", "", f], ["-x", f], ["-d", "x", f]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            inverted.parse_args(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    probe = "import sys\nfrom mir_prefer_amd import inverted\ntry:\n    inverted.main(['-d', '5', %r])\nfinally:\n    print('capi' in ' '.join(sys.modules))\n" % f
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and b"Error: " not in r.stderr and r.stdout.strip() == b"False", (r.stdout, r.stderr)
    # a missing file is reported before a device is opened; the outputs of an earlier run are gone all the same
    stale = [f + ".inverted" + ext for ext in (".tsv", ".gff3", ".fa")]
    for path in stale:
        open(path, "w").write("old\n")
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.inverted", f], cwd=str(tmp_path), capture_output=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 255 and r.stderr.startswith(b"Error: file ") and not any(os.path.exists(path) for path in stale)


def test_abi_entries_are_declared():
    from mir_prefer_amd import capi
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_inverted_scan(", "mirp_set_inverted_capacity(", "mirp_inverted_last_stats(", "MirpInvertedOpts", "MirpInvertedRec"):
        assert name in header
    assert capi.ABI_VERSION == 17
    m = re.search(r"typedef struct \{([^}]*)\} MirpInvertedRec;", header)
    fields = [f.strip() for part in m.group(1).split(";") for f in re.sub(r"int(32|64)_t", "", part).split(",") if f.strip()]
    assert fields == list(capi.INVERTED_DTYPE.names) and capi.INVERTED_DTYPE.itemsize == 56
    m = re.search(r"typedef struct \{([^}]*)\} MirpInvertedOpts;", header)
    fields = [f.strip() for f in m.group(1).replace("int32_t", "").replace(";", "").split(",")]
    import ctypes
    assert fields == [f for f, _ in capi.InvertedOpts._fields_] and ctypes.sizeof(capi.InvertedOpts) == 24
    for name, value in (("TILE", capi.INVERTED_TILE), ("STRIP", capi.INVERTED_STRIP), ("MAX_SPAN", capi.INVERTED_MAX_SPAN)):
        assert int(re.search(r"#define MIRP_INVERTED_%s\s+(\d+)" % name, header).group(1)) == value
    assert capi.INVERTED_TILE % capi.INVERTED_STRIP == 0 and capi.INVERTED_MAX_SPAN == 4096
    assert len(capi.INVERTED_STATS) == 11


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_kernels_use_no_scratch(tmp_path):
    import shutil
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "mir-prefer_amd", "csrc", "inverted_kernels.hip"), "-o", str(tmp_path / "inverted_kernels.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    report, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    for kernel in ("iv_scan_kernel", "iv_cand_kernel", "iv_trace_kernel"):
        mine = [v for k, v in report.items() if kernel in k]
        assert len(mine) == 1 and mine[0]["ScratchSize"] == 0, (kernel, mine)
