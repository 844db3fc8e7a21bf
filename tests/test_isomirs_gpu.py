"""GPU tests of the isomiR counts (isomir_kernels.hip, mirp_isomir_scan, `python -m mir_prefer_amd.isomirs`): all three files byte for
byte against the plain-Python restatement (tests/isomir_restatement.py) on seeded random annotations and SAM files at five settings, a hotspot locus
whose sums pass 2^32 and whose keys span many waves, 300,000 small loci (more records and loci than the capped grids have lanes), the edges (a contig
of 2^31 - 1 bases, 255 samples, no records, nothing assigned, a contig without loci) and the chain reads collapse -> align --tail -> isomirs."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from mir_prefer_amd import align, capi, isomirs, reads
from mir_prefer_amd.capi import ISO_LOCUS_DTYPE
from mir_prefer_amd.synth import ALN_DTYPE
from tests import isomir_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(2, 4), (0, 0), (15, 15), (0, 15), (7, 1)]
GRID_LANES = 1024 * 256            # ISO_MAX_BLOCKS x ISO_NT of isomir_kernels.hip


def as_result(iso, sums, lc, ic, stats):
    """What Context.isomir_scan returns, in the shape of the restatement's result."""
    return {"isomirs": [tuple(r) for r in iso.tolist()], "sums": [list(r) for r in sums.tolist()], "locus_counts": lc.tolist(),
            "isomir_counts": ic.tolist(), "stats": (stats["records"], stats["assigned"], stats["depth"], stats["isomirs"])}


def loci_array(loci):
    arr = np.zeros(len(loci), dtype=ISO_LOCUS_DTYPE)
    for f, col in zip(("tid", "strand", "start", "end"), zip(*loci)):
        arr[f] = col
    return arr


def summary_numbers(err):
    line = [l for l in err.split("\n") if l.startswith("isomirs: ") and "records kept" in l][-1]
    v = [int(w) for w in line.replace(",", " ").split() if w.isdigit()]
    return {"records": v[0], "cigar": v[1], "long_tail": v[2], "kept": v[3], "dropped": v[4], "assigned": v[5], "depth": v[6], "isomirs": v[7]}


# ---------------------------------------------------------------------------------------------------- 1. random
CONTIGS = [("chrA", 40000), ("chrB", 30000), ("chrC", 20000), ("chrD", 6000)]


def random_world(tmp, seed=11):
    rng = random.Random(seed)
    loci, places = [], set()

    def add(contig, start, end, strand):
        if start < 1 or end > dict(CONTIGS)[contig] or start > end or (contig, strand, start, end) in places:
            return
        places.add((contig, strand, start, end))
        loci.append((contig, start, end, strand))
    for contig, ln in CONTIGS:
        add(contig, 1, 21, "+")
        add(contig, 1, 22, "-")
        add(contig, ln - 20, ln, "-")
        add(contig, ln - 21, ln, "+")
        for _ in range(200):
            start, strand = rng.randrange(30, ln - 60), rng.choice("+-")
            end = start + rng.randrange(19, 25)
            add(contig, start, end, strand)
            kind = rng.randrange(6)
            if kind == 0:                                   # nested, and one shifted by a base on each side
                add(contig, start + rng.randrange(1, 4), end - rng.randrange(1, 4), strand)
                add(contig, start + 1, end + 1, strand)
            elif kind == 1:                                 # the same 5' end, another 3' end
                d = rng.randrange(1, 6)
                add(contig, *((start, end + d) if strand == "+" else (start - d, end)), strand)
            elif kind == 2:                                 # the same place on the other strand
                add(contig, start, end, "-" if strand == "+" else "+")
    rng.shuffle(loci)
    gff = ["##gff-version 3\n"]
    for k, (contig, start, end, strand) in enumerate(loci):
        gff.append("%s\t.\tmiRNA_primary_transcript\t%d\t%d\t.\t%s\t.\tID=pri%d\n" % (contig, max(start - 40, 1), end + 40, strand, k))
        gff.append("%s\t.\tmiRNA\t%d\t%d\t.\t%s\t.\tID=M%d%s\n" % (contig, start, end, strand, k, ";Name=miR%d" % k if k % 3 else ""))
    gff.append("chrZ\t.\tmiRNA\t5\t25\t.\t+\t.\tID=elsewhere\n")
    gff_path = os.path.join(tmp, "m.gff3")
    open(gff_path, "w").write("".join(gff))
    head = "@HD\tVN:1.0\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    sams = []
    for fi, sample in enumerate(("root", "leaf_2", "flower")):
        lines = [head]
        for k in range(6700 + 13 * fi):
            rid = "%s_r%d_x%d" % (sample, k, rng.choice((1, 2, 5, 40, 1000, rng.randrange(1, 100000))))
            if rng.random() < 0.08:                         # background
                contig, ln = rng.choice(CONTIGS)
                m = rng.randrange(18, 27)
                lines.append("%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t*\n" % (rid, rng.choice((0, 16)), contig, rng.randrange(1, ln - 30), m, "A" * m))
                continue
            contig, start, end, strand = rng.choice(loci)
            big = rng.random() < 0.25
            d5 = rng.randrange(-17, 18) if big else rng.choice((0, 0, 0, 0, 1, -1, 2, -2, 3))
            d3 = rng.randrange(-17, 18) if big else rng.choice((0, 0, 0, -1, -2, 1, 2, -5, 4, 5))
            if strand == "+":
                p, q = start + d5, end + d3
            else:
                p, q = start - d3, end - d5
            m = q - p + 1
            if p < 1 or m < 1:
                continue
            t = rng.choice((0, 0, 0, 1, 1, 2, 2, 3, 5, 8))
            tail = "".join(rng.choice("TTTAAACGNtu") for _ in range(t))
            body = "".join(rng.choice("ACGT") for _ in range(m))
            flag = 16 if strand == "-" else 0
            form = rng.random()
            if form < 0.03:
                flag |= rng.choice((4, 256, 512, 1024))
            if form > 0.94:                                 # skipped forms
                cigar, seq, opts = rng.choice((("%dM1I%dM" % (m - 2, 1), body, ""), ("2S%dM" % m if flag == 0 else "%dM2S" % m, "GG" + body, ""),
                                               ("%dM" % m, body, "\tXT:Z:ACGTACGTT"), ("%dM9S" % m if flag == 0 else "9S%dM" % m,
                                                                                      body + "A" * 9 if flag == 0 else "A" * 9 + body, "")))
            elif t and rng.random() < 0.5:                  # the soft-clipped form of align --tail: SEQ holds the tail as the strand stores it
                norm = R.norm_tail(tail)
                stored = tail if not flag & 16 else "".join({"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}[c] for c in reversed(norm))
                cigar, seq = ("%dM%dS" % (m, t), body + stored) if not flag & 16 else ("%dS%dM" % (t, m), stored + body)
                opts = "\tXT:Z:%s" % norm
            else:                                           # the --tail-trim form, or no tail
                cigar, seq, opts = "%dM" % m, body, ("\tNM:i:0\tXT:Z:%s" % tail if t else "")
            lines.append("%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t%s%s\n" % (rid, flag, contig, p, cigar, seq, "I" * len(seq), opts))
        path = os.path.join(tmp, "s%d.sam" % fi)
        open(path, "w").write("".join(lines))
        sams.append(path)
    grng = random.Random(seed + 1)
    seqs = {c: "".join(grng.choice("ACGTacgtN") for _ in range(ln)).encode() for c, ln in CONTIGS}
    fa = os.path.join(tmp, "g.fa")
    open(fa, "wb").write(b"".join(b">" + c.encode() + b"\n" + seqs[c] + b"\n" for c, _ in CONTIGS))
    return gff_path, sams, fa, seqs


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("isomirs"))
    gff, sams, fa, seqs = random_world(tmp)
    names, lens, samples, recs, skipped = R.parse_sams(sams)
    kept, dropped = R.keep_loci(R.read_gff(gff), names, lens)
    tid_of = {n: t for t, n in enumerate(names)}
    loci = [(tid_of[l[2]], 0 if l[5] == "+" else 1, l[3], l[4]) for l in kept]
    return {"tmp": tmp, "gff": gff, "sams": sams, "fa": fa, "seqs": seqs, "names": names, "lens": lens, "samples": samples, "recs": recs,
            "skipped": skipped, "kept": kept, "dropped": dropped, "loci": loci}


@pytest.mark.parametrize("max5, max3", SETTINGS)
def test_random_files_equal_the_restatement(gpu_ctx, world, capsys, max5, max3):
    w = world
    assert len(w["recs"]) % 64 != 0 and len(w["recs"]) > 15000 and len(w["loci"]) > 800 and w["dropped"] == 1
    assert w["skipped"]["cigar"] > 100 and w["skipped"]["long_tail"] > 100 and w["samples"] == ["root", "leaf_2", "flower"]
    want = R.scan_plain(w["recs"], w["loci"], max5, max3, 3)
    with_g = (max5, max3) == (2, 4)
    files = R.files(want, w["kept"], w["samples"], w["seqs"] if with_g else None)
    assert want["stats"][1] > (300 if max5 == 0 and max3 == 0 else 5000) and want["stats"][3] > 200
    base = os.path.join(w["tmp"], "out_%d_%d" % (max5, max3))
    argv = ["--max5", str(max5), "--max3", str(max3), "-o", base + ".tsv"] + (["-g", w["fa"]] if with_g else []) + [w["gff"]] + w["sams"]
    got = []
    for _ in range(2):                                      # twice: no result depends on scheduling
        assert isomirs.main(argv) == 0
        got.append(tuple(open(p, "rb").read() for p in isomirs.output_paths(base)))
        st = summary_numbers(capsys.readouterr().err)
    assert got[0] == got[1]
    for g, f, what in zip(got[0], files, ("tsv", "counts", "isomirs")):
        assert g == f, what
    assert st == {"records": len(w["recs"]), "cigar": w["skipped"]["cigar"], "long_tail": w["skipped"]["long_tail"], "kept": len(w["kept"]),
                  "dropped": 1, "assigned": want["stats"][1], "depth": want["stats"][2], "isomirs": want["stats"][3]}
    # the library call itself, and the numpy restatement the larger tests lean on
    names, lens, samples, alns, tails, skipped = capi.tokenize_sams_tailed(w["sams"])
    assert as_result(*gpu_ctx.isomir_scan(alns, tails, loci_array(w["loci"]), max5, max3, 3)) == want
    assert R.scan_numpy(alns, tails, w["loci"], max5, max3, 3) == want


# ---------------------------------------------------------------------------------------------------- 2. hotspot
def test_hotspot_locus_sums_past_32_bits(gpu_ctx):
    rng = np.random.default_rng(5)
    n = 2_100_000
    loci = [(0, 0, 5000, 5020), (0, 0, 900, 921), (1, 1, 300, 320), (0, 1, 5000, 5020)]
    combos = [(d5, d3, R.tail_code(t)) for d5 in (-1, 0, 1) for d3 in (-2, -1, 0, 1) for t in ("", "T", "TT", "A")][:40]
    pick = rng.integers(0, len(combos), n)
    c = np.array(combos, dtype=np.int64)[pick]
    alns = np.zeros(n + 3, dtype=ALN_DTYPE)
    alns["tid"][:n] = 0
    alns["pos"][:n] = 5000 + c[:, 0]
    alns["len"][:n] = (5020 + c[:, 1]) - (5000 + c[:, 0]) + 1
    alns["depth"][:n] = rng.integers(1 << 30, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    alns["sample"][:n] = rng.integers(0, 3, n)
    tails = np.zeros(n + 3, dtype=np.uint32)
    tails[:n] = c[:, 2]
    alns[n:] = [(0, 900, 7, 22, 0, 1), (1, 301, 9, 21, 1, 2), (0, 5000, 11, 21, 1, 0)]
    order = rng.permutation(n + 3)
    alns, tails = alns[order], tails[order]
    want = R.scan_numpy(alns, tails, loci, 2, 4, 3)
    got = as_result(*gpu_ctx.isomir_scan(alns, tails, loci_array(loci), 2, 4, 3))
    assert got == want
    assert want["stats"][1:] == (n + 3, int(alns["depth"].sum(dtype=np.uint64)), 43) and want["sums"][0][8] == 40
    assert min(r[4] for r in want["isomirs"][:40]) > 1 << 40 and min(min(row) for row in want["isomir_counts"][:40]) > 1 << 32
    assert want["sums"][1][:2] == [7, 7] and want["sums"][2][0] == 9 and want["sums"][2][3] == 9 and want["sums"][3][1] == 11


# ---------------------------------------------------------------------------------------------------- 3. many small
def test_many_small_loci_pass_the_grid(gpu_ctx):
    rng = np.random.default_rng(9)
    nl = 300_000
    start = 10 + 30 * np.arange(nl, dtype=np.int64)
    strand = (np.arange(nl) % 3 == 1).astype(np.int64)
    loci = list(zip([0] * nl, strand.tolist(), start.tolist(), (start + 20).tolist()))
    per = rng.integers(1, 4, nl)
    of = np.repeat(np.arange(nl), per)
    n = len(of)
    assert n > 2 * GRID_LANES and nl > GRID_LANES and n % 64 != 0          # every resident lane takes a third record, and a second locus
    d5, d3 = rng.integers(-2, 3, n), rng.integers(-3, 3, n)
    sg = 1 - 2 * strand[of]
    l5, l3 = np.where(strand[of] == 0, start[of], start[of] + 20), np.where(strand[of] == 0, start[of] + 20, start[of])
    r5, r3 = l5 + sg * d5, l3 + sg * d3
    alns = np.zeros(n, dtype=ALN_DTYPE)
    alns["pos"], alns["len"] = np.minimum(r5, r3), np.abs(r3 - r5) + 1
    alns["strand"], alns["depth"], alns["sample"] = strand[of], rng.integers(1, 50, n), rng.integers(0, 2, n)
    tails = rng.choice(np.array([0, 0, 0, R.tail_code("T"), R.tail_code("A"), R.tail_code("TN")], dtype=np.uint32), n)
    order = rng.permutation(n)
    alns, tails = alns[order], tails[order]
    want = R.scan_numpy(alns, tails, loci, 2, 4, 2)
    got = as_result(*gpu_ctx.isomir_scan(alns, tails, loci_array(loci), 2, 4, 2))
    assert want["stats"][1] == n and all(s[8] >= 1 for s in want["sums"])
    for key in ("stats", "isomirs", "sums", "locus_counts", "isomir_counts"):
        assert got[key] == want[key], key


# ---------------------------------------------------------------------------------------------------- 4. edges
def recs_of(alns, tails):
    return [(r[0], r[4], r[1], r[3], r[2], r[5], int(t)) for r, t in zip(alns.tolist(), tails.tolist())]


def test_last_base_of_the_longest_contig(gpu_ctx):
    LN = (1 << 31) - 1
    loci = [(0, 1, LN - 20, LN), (0, 0, LN - 21, LN), (0, 0, 1, 21)]
    rows = [(0, LN - 20, 3, 21, 1, 0), (0, LN - 20, 4, 23, 1, 0), (0, LN - 22, 5, 23, 1, 0), (0, LN - 21, 6, 22, 0, 0), (0, LN - 21, 7, 37, 0, 0),
            (0, LN, 8, 1, 1, 0), (0, LN, 9, 65535, 0, 0), (0, 1, 10, 21, 0, 0), (0, 0, 11, 22, 0, 0), (0, LN - 35, 12, 36, 1, 0)]
    alns = np.array(rows, dtype=ALN_DTYPE)
    tails = np.array([0, 4, 0, 0, 24, 0, 0, 488280, 0, 0], dtype=np.uint32)
    for max5, max3 in ((2, 4), (15, 15), (0, 0)):
        want = R.scan_plain(recs_of(alns, tails), loci, max5, max3, 1)
        assert as_result(*gpu_ctx.isomir_scan(alns, tails, loci_array(loci), max5, max3, 1)) == want
    want = R.scan_plain(recs_of(alns, tails), loci, 15, 15, 1)
    assert want["isomirs"] == [(0, -2, 0, 4, 4), (0, 0, 0, 0, 3), (0, 0, 2, 0, 5), (0, 0, 15, 0, 12), (1, 0, 0, 0, 6), (1, 0, 15, 24, 7),
                               (2, -1, 0, 0, 11), (2, 0, 0, 488280, 10)]


def test_255_samples_and_a_contig_without_loci(gpu_ctx):
    loci = [(0, 0, 101, 121), (2, 1, 50, 70)]
    rows = [(0, 101 + (s % 3) - 1, s + 1, 21, 0, s) for s in range(255)] + [(1, 101, 5, 21, 0, 0), (2, 50, 6, 21, 1, 254), (3, 50, 6, 21, 1, 1)]
    alns = np.array(rows, dtype=ALN_DTYPE)
    tails = np.array([s % 7 for s in range(len(rows))], dtype=np.uint32)
    want = R.scan_plain(recs_of(alns, tails), loci, 2, 4, 255)
    got = gpu_ctx.isomir_scan(alns, tails, loci_array(loci), 2, 4, 255)
    assert as_result(*got) == want and got[2].shape == (2, 255) and want["stats"][1] == 256
    with pytest.raises(capi.MirpError) as e:
        gpu_ctx.isomir_scan(alns, tails, loci_array(loci), 2, 4, 254)
    assert "sample index" in str(e.value)
    for bad in (dict(max5=16), dict(max3=-1), dict(n_samples=0), dict(n_samples=256)):
        with pytest.raises(capi.MirpError):
            gpu_ctx.isomir_scan(alns, tails, loci_array(loci), **dict(dict(max5=2, max3=4, n_samples=255), **bad))
    with pytest.raises(capi.MirpError):
        gpu_ctx.isomir_scan(alns, tails, loci_array([(0, 0, 5, 4)]), 2, 4, 255)


def test_no_records_and_nothing_assigned(gpu_ctx, tmp_path, capsys):
    gff = tmp_path / "m.gff3"
    gff.write_text("chr1\t.\tmiRNA\t101\t121\t.\t+\t.\tID=a;Name=x\nchr1\t.\tmiRNA\t301\t321\t.\t-\t.\tID=b\n")
    head = "@SQ\tSN:chr1\tLN:1000\n"
    empty, far = tmp_path / "e_1.sam", tmp_path / "f_1.sam"
    empty.write_text(head)
    far.write_text(head + "lib_r1_x5\t0\tchr1\t500\t255\t21M\t*\t0\t0\t%s\t*\n" % ("A" * 21))
    zero = (isomirs.TSV_HEADER + "a\tx\tchr1\t101\t121\t+" + "\t0" * 9 + "\t.\t.\t.\t0\nb\t.\tchr1\t301\t321\t-" + "\t0" * 9 + "\t.\t.\t.\t0\n").encode()
    for sams, names, records in (([empty], ["", ], 0), ([empty, far], ["", "lib"], 1)):
        base = str(tmp_path / ("z%d" % records))
        assert isomirs.main(["-o", base, str(gff)] + [str(s) for s in sams]) == 0
        got = [open(p, "rb").read() for p in isomirs.output_paths(base)]
        files, st, _ = R.restate(str(gff), [str(s) for s in sams], 2, 4)
        assert got == list(files) and got[0] == zero
        assert got[1] == ("name\t" + "\t".join(names) + "\na" + "\t0" * len(names) + "\nb" + "\t0" * len(names) + "\n").encode()
        assert got[2] == ("name\td5\td3\ttail\treads\tseq\t" + "\t".join(names) + "\n").encode()
        assert summary_numbers(capsys.readouterr().err) == dict(st, records=records) and st["assigned"] == 0
    res = gpu_ctx.isomir_scan(np.zeros(0, dtype=ALN_DTYPE), np.zeros(0, np.uint32), loci_array([(0, 0, 101, 121)]), 2, 4, 2)
    assert as_result(*res) == R.scan_plain([], [(0, 0, 101, 121)], 2, 4, 2) and res[3].shape == (0, 2)


# ---------------------------------------------------------------------------------------------------- 5. chain and command line
def run_cli(args, cwd):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.isomirs"] + args, cwd=str(cwd), capture_output=True, timeout=300,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_chain_collapse_align_tail_isomirs(tmp_path):
    rng = random.Random(21)
    g1 = [rng.choice("ACGT") for _ in range(700)]
    g2 = [rng.choice("ACGT") for _ in range(500)]
    g1[320:323] = "CCG"                                      # behind miR_plus (300..320, 1-based): a TT or A tail is not templated
    g2[146:149] = "CGG"                                      # behind miR_minus on its strand (150..170 on -): the bases before 150
    g1, g2 = "".join(g1), "".join(g2)
    (tmp_path / "g.fa").write_text(">c1\n%s\n>c2\n%s\n" % (g1, g2))
    (tmp_path / "m.gff3").write_text("c1\tmiR-PREFeR\tmiRNA-precursor\t250\t400\t.\t+\t.\tID=miRNA-precursor_0;NAME=miRNA-precursor_0;Other=\n"
                                     "c1\tmiR-PREFeR\tmiRNA\t300\t320\t.\t+\t.\tID=miRNA_0;NAME=miRNA_0;Other=\n"
                                     "c2\tmiR-PREFeR\tmiRNA\t150\t170\t.\t-\t.\tID=miRNA_1;NAME=miRNA_1;Other=\n")
    mature = g1[299:320]
    minus = revcomp(g2[149:170])
    kinds = [(mature, 9), (mature + "TT", 4), (mature + "A", 3), (mature[:-2], 2), (mature[1:], 5), (minus, 6), (minus + "TT", 2)]
    for name, scale in (("S1", 1), ("S2", 3)):
        reads_ = [seq for seq, count in kinds for _ in range(count * scale)]
        rng.shuffle(reads_)
        (tmp_path / (name + ".fa")).write_text("".join(">read%d\n%s\n" % (k, s) for k, s in enumerate(reads_)))
    (tmp_path / "names.txt").write_text("S1\nS2\n")
    fas = [str(tmp_path / "S1.fa"), str(tmp_path / "S2.fa")]
    assert reads.main(["collapse", str(tmp_path / "names.txt")] + fas) == 0
    proc = [f + ".processed" for f in fas]
    assert align.main(["--tail", "3", "-v", "0", "-r", str(tmp_path / "g.fa")] + proc) == 0
    sams = [p + ".sam" for p in proc]
    gff = str(tmp_path / "m.gff3")
    r = run_cli(["-g", str(tmp_path / "g.fa"), "-o", str(tmp_path / "clip"), gff] + sams, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    clip = [open(p, "rb").read() for p in isomirs.output_paths(str(tmp_path / "clip"))]
    seqs = {"c1": g1.encode(), "c2": g2.encode()}
    files, st, res = R.restate(gff, sams, 2, 4, seqs)
    assert clip == list(files)
    rna = mature.replace("T", "U")
    lines = clip[2].decode().split("\n")
    assert "miRNA_0\t0\t0\tTT\t16\t%suu\t4\t12" % rna in lines and "miRNA_0\t0\t0\tA\t12\t%sa\t3\t9" % rna in lines
    assert "miRNA_0\t0\t0\t.\t36\t%s\t9\t27" % rna in lines and "miRNA_0\t0\t-2\t.\t8\t%s\t2\t6" % rna[:-2] in lines
    assert "miRNA_0\t1\t0\t.\t20\t%s\t5\t15" % rna[1:] in lines
    assert "miRNA_1\t0\t0\t.\t24\t%s\t6\t18" % minus.replace("T", "U") in lines and "miRNA_1\t0\t0\tTT\t8\t%suu\t2\t6" % minus.replace("T", "U") in lines
    assert clip[0].decode().split("\n")[1] == "miRNA_0\tmiRNA_0\tc1\t300\t320\t+\t92\t36\t20\t8\t0\t28\t16\t12\t5\t0\t0\t.\t36"
    assert clip[1] == b"name\tS1\tS2\nmiRNA_0\t23\t69\nmiRNA_1\t8\t24\n"
    assert st["assigned"] == 14 and st["cigar"] == 0 and b"14 records assigned" in r.stderr
    # the same reads through --tail-trim: other SAM records, identical files
    assert align.main(["--tail", "3", "--tail-trim", "-v", "0", "-r", str(tmp_path / "g.fa")] + proc) == 0
    assert b"\t21M2S\t" not in open(sams[0], "rb").read() and b"XT:Z:TT" in open(sams[0], "rb").read()
    r = run_cli(["-g", str(tmp_path / "g.fa"), "-o", str(tmp_path / "trim.tsv"), gff] + sams, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert [open(p, "rb").read() for p in isomirs.output_paths(str(tmp_path / "trim"))] == clip
    # a refused GFF leaves no file, not even the earlier run's
    (tmp_path / "bad.gff3").write_text("c1\t.\tmiRNA\t300\t320\t.\t+\t.\tID=a\nc1\t.\tmiRNA\t300\t320\t.\t+\t.\tID=b\n")
    r = run_cli(["-o", str(tmp_path / "trim"), str(tmp_path / "bad.gff3")] + sams, tmp_path)
    assert r.returncode == 255 and r.stderr.startswith(b"Error: ") and not any(os.path.exists(p) for p in isomirs.output_paths(str(tmp_path / "trim")))
    (tmp_path / "far.gff3").write_text("c9\t.\tmiRNA\t300\t320\t.\t+\t.\tID=a\n")
    for bad in ("far.gff3", "long.gff3"):
        if bad == "long.gff3":
            (tmp_path / bad).write_text("c2\t.\tmiRNA\t480\t501\t.\t+\t.\tID=a\n")
        r = run_cli(["-o", str(tmp_path / "clip"), str(tmp_path / bad)] + sams, tmp_path)
        assert r.returncode == 255 and r.stderr.startswith(b"Error: "), r.stderr
    assert not any(os.path.exists(p) for p in isomirs.output_paths(str(tmp_path / "clip")))
    r = run_cli(["-g", str(tmp_path / "S1.fa"), "-o", str(tmp_path / "g"), gff] + sams, tmp_path)
    assert r.returncode == 255 and b"is not in" in r.stderr and not os.path.exists(str(tmp_path / "g.tsv"))
