"""CPU tests of the reads-on-given-loci verb: worked examples of the counting rule as literals (a record that hangs over a locus
start by one base and one that misses it by one, nested and duplicate loci, -s with +, - and . loci, a locus without reads, the contig clipping);
every accepted and refused line form of the three loci formats, -t and the loci dropped for an unknown contig; the two restatements of
tests/loci_restatement.py against each other on seeded inputs and the module's own readers and file writer against them; the struct layouts
against the C header, the new symbol and the unchanged ABI version; and the option errors of the command line, which exit 2 without opening
a device."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from mir_prefer_amd import capi, loci, phasing
from tests import loci_restatement as R
from tests.test_clusters_cpu import ROOT, make_records, random_records, random_seqs


def L(*rows):
    """(tid, strand char, start, end) -> LOCUS_DTYPE"""
    arr = np.zeros(len(rows), capi.LOCUS_DTYPE)
    for q, (tid, strand, start, end) in enumerate(rows):
        arr[q] = (tid, "+-.".index(strand), start, end)
    return arr


def both(rows, loci_rows, lens, n_samples=1, stranded=False):
    """The two restatements of the scan agree; -> (rows as CLUSTER_DTYPE, counts, stats)."""
    alns = make_records(rows)
    arr = L(*loci_rows)
    got, counts, stats = R.scan_numpy(alns, arr, lens, n_samples, stranded)
    plain, pairs = R.scan_plain(alns, arr, lens, n_samples, stranded)
    assert stats["pairs"] == pairs
    for q, c in enumerate(plain):
        assert (int(got["reads"][q]), int(got["plus_reads"][q]), got["sizes"][q].tolist(), counts[q].tolist(), int(got["placements"][q])) == \
            (c["reads"], c["plus"], c["sizes"], c["samples"], len(c["pl"])), q
        if c["pl"]:
            (mp, ms, ml), mr = min(c["pl"].items(), key=lambda kv: (-kv[1], kv[0]))
            assert (int(got["major_pos"][q]), int(got["major_strand"][q]), int(got["major_len"][q]), int(got["major_reads"][q])) == (mp, ms, ml, mr)
        else:
            assert (int(got["major_pos"][q]), int(got["major_strand"][q]), int(got["major_len"][q]), int(got["major_reads"][q])) == (0, 0, 0, 0)
    return got, counts, stats


# ---------------------------------------------------------------------------------------------------- the rule
def test_one_base_of_overlap_counts_and_one_base_short_does_not():
    # the record [80, 100] ends on the first base of [100, 200]; [79, 99] ends one base before it
    got, _, st = both([(0, 80, 3, 21, 0), (0, 79, 5, 21, 0), (0, 200, 7, 21, 1), (0, 201, 11, 21, 1)], [(0, ".", 100, 200)], [1000])
    assert int(got["reads"][0]) == 3 + 7 and int(got["plus_reads"][0]) == 3 and st["pairs"] == 2 and int(got["placements"][0]) == 2
    assert (int(got["major_pos"][0]), int(got["major_strand"][0]), int(got["major_len"][0]), int(got["major_reads"][0])) == (200, 1, 21, 7)


def test_nested_overlapping_and_duplicate_loci_all_count():
    rows = [(0, 100, 2, 21, 0, 0), (0, 150, 3, 24, 1, 1), (0, 300, 5, 22, 0, 0), (1, 100, 9, 21, 0, 1)]
    got, counts, st = both(rows, [(0, ".", 90, 400), (0, ".", 140, 160), (0, ".", 160, 310), (0, ".", 140, 160), (1, ".", 1, 99), (0, ".", 1, 1000)],
                           [1000, 500], n_samples=2)
    assert got["reads"].tolist() == [10, 3, 8, 3, 0, 10] and counts.tolist() == [[7, 3], [0, 3], [5, 3], [0, 3], [0, 0], [7, 3]]
    assert got["placements"].tolist() == [3, 1, 2, 1, 0, 3] and st["pairs"] == 3 + 1 + 2 + 1 + 0 + 3
    assert got[1:2].tobytes() == got[3:4].tobytes()                           # the duplicate has the same row
    assert got["sizes"][0].tolist() == [0, 0, 2, 5, 0, 3, 0]


def test_stranded_counts_own_strand_or_none():
    rows = [(0, 100, 2, 21, 0), (0, 105, 3, 21, 1)]
    loc = [(0, "+", 90, 130), (0, "-", 90, 130), (0, ".", 90, 130)]
    assert both(rows, loc, [500], stranded=True)[0]["reads"].tolist() == [2, 3, 5]
    assert both(rows, loc, [500], stranded=False)[0]["reads"].tolist() == [5, 5, 5]
    got = both(rows, loc, [500], stranded=True)[0]
    assert got["placements"].tolist() == [1, 1, 2] and got["major_pos"].tolist() == [100, 105, 105]


def test_spans_are_clipped_to_the_contig():
    # pos 0 covers [1, 20]; a record at LN + 1 and one wholly before position 1 have no span; one past the end is clipped to LN
    rows = [(0, 0, 2, 21, 0), (0, 501, 3, 21, 0), (0, -30, 5, 21, 0), (0, 495, 7, 21, 1), (1, 1, 11, 21, 0), (7, 10, 13, 21, 0)]
    got, _, st = both(rows, [(0, ".", 1, 1), (0, ".", 20, 21), (0, ".", 21, 30), (0, ".", 500, 500), (1, ".", 1, 300), (0, ".", 1, 500)], [500, 300])
    assert got["reads"].tolist() == [2, 2, 0, 7, 11, 9] and st["pairs"] == 6
    assert int(got["major_pos"][0]) == 0                                       # the placement keeps POS as the file has it


def test_major_placement_ties_are_section_16s():
    def major(rows):
        g = both(rows, [(0, ".", 1, 400)], [500])[0][0]
        return [int(g[f]) for f in ("major_pos", "major_strand", "major_len", "major_reads")]
    assert major([(0, 100, 5, 21, 0), (0, 101, 6, 21, 0)]) == [101, 0, 21, 6]
    assert major([(0, 100, 3, 21, 0), (0, 100, 3, 21, 0), (0, 101, 6, 21, 0)]) == [100, 0, 21, 6]
    assert major([(0, 101, 6, 21, 0), (0, 100, 6, 24, 1)]) == [100, 1, 24, 6]
    assert major([(0, 100, 6, 21, 1), (0, 100, 6, 24, 0)]) == [100, 0, 24, 6]
    assert major([(0, 100, 6, 24, 0), (0, 100, 6, 21, 0)]) == [100, 0, 21, 6]


def test_worked_files(tmp_path):
    names, lens, samples = ["chrB", "chrA"], [1000, 600], ["s0", "s1"]
    alns = make_records([(0, 100, 8, 21, 0, 0), (0, 100, 2, 21, 0, 1), (0, 110, 2, 24, 1, 1), (1, 5, 4, 30, 1, 0)])
    kept = [("a", "gene", "chrB", 90, 125, "+"), ("b", ".", "chrA", 1, 10, "."), ("empty", "PHAS", "chrA", 100, 200, "-")]
    seqs = {"chrB": b"N" * 99 + b"acgtacgtacgtacgtacgtaGG" + b"N" * 878, "chrA": b"ttttGCGCGCGC" * 50}
    want_tsv = (R.HEADER +
                b"a\tgene\tchrB\t90\t125\t+\t12\t10\t+\t21\t2\t100\t+\t21\t10\tACGUACGUACGUACGUACGUA\t0\t0\t10\t0\t0\t2\t0\n"
                b"b\t.\tchrA\t1\t10\t.\t4\t0\t-\tN\t1\t5\t-\t30\t4\tGCGCGCAAAAGCGCGCGCAAAAGCGCGCGC\t0\t0\t0\t0\t0\t0\t4\n"
                b"empty\tPHAS\tchrA\t100\t200\t-\t0\t0\t.\tN\t0\t0\t.\t0\t0\t*\t0\t0\t0\t0\t0\t0\t0\n")
    want_cnt = b"name\ts0\ts1\na\t8\t4\nb\t4\t0\nempty\t0\t0\n"
    assert R.files_plain(alns, kept, names, lens, samples, False, seqs) == (want_tsv, want_cnt)
    rows, counts, _ = R.scan_numpy(alns, R.locus_array(kept, names), lens, 2)
    assert loci.format_files(kept, rows, counts, samples, seqs) == (want_tsv, want_cnt)
    assert loci.format_files(kept, rows, counts, samples)[0].split(b"\n")[1].split(b"\t")[15] == b"*"
    assert loci.TSV_HEADER == R.HEADER and (loci.locus_array(kept, names) == R.locus_array(kept, names)).all()


@pytest.mark.parametrize("seed", range(4))
def test_restatements_agree_on_random_inputs(seed):
    rng = np.random.RandomState(100 + seed)
    lens = [3000, 700, 150, 5000]
    names = ["chr%d" % i for i in range(4)]
    alns = random_records(rng, lens, 3, 300, 20)
    kept = random_loci(rng, names, lens, 60)
    seqs = dict(zip(names, random_seqs(rng, lens)))
    for stranded in (False, True):
        arr = R.locus_array(kept, names)
        rows, counts, stats = R.scan_numpy(alns, arr, lens, 3, stranded)
        want = R.files_plain(alns, kept, names, lens, ["a", "b", "a"], stranded, seqs)
        assert loci.format_files(kept, rows, counts, ["a", "b", "a"], seqs) == want
        assert stats["pairs"] == R.scan_plain(alns, arr, lens, 3, stranded)[1] and stats["max_len"] == int(alns["len"].max())
    assert int((rows["placements"] == 0).sum()) > 0 and int((rows["placements"] > 3).sum()) > 5


def random_loci(rng, names, lens, n):
    """Loci of every shape: short and long, nested in and equal to an earlier one, contig-wide, at both contig ends, of all three strands."""
    out = []
    for k in range(n):
        t = int(rng.randint(0, len(lens)))
        kind = k % 6
        if kind == 0 and out:
            _, _, contig, a, b, _ = out[int(rng.randint(0, len(out)))]
            t = names.index(contig)
            a, b = (a, b) if rng.randint(0, 2) else (a + (b - a) // 3, b - (b - a) // 3)
        elif kind == 1:
            a, b = 1, lens[t]
        elif kind == 2:
            a = int(rng.randint(1, 30))
            b = a + int(rng.randint(0, 40))
        elif kind == 3:
            b = lens[t]
            a = b - int(rng.randint(0, 40))
        else:
            a = int(rng.randint(1, lens[t] + 1))
            b = min(lens[t], a + int(rng.randint(0, 300)))
        out.append(("L%d" % k, "t%d" % (k % 3), names[t], a, b, "+-."[int(rng.randint(0, 3))]))
    return out


# ---------------------------------------------------------------------------------------------------- the loci files
GFF = ("##gff-version 3\n"
       "# a comment\n"
       "\n"
       "chr1\tsrc\tgene\t10\t200\t.\t+\t.\tID=g1;Name=x\n"
       "chr1\tsrc\tmRNA\t10\t200\t.\t+\t.\tID=m1;Parent=g1\r\n"
       "chr1\tsrc\texon\t10\t50\t.\t-\t.\tParent=m1\n"
       "chr2\tsrc\tgene\t5\t5\t.\t?\t.\tName=n; ID=g2 ;ID=other\n"
       "chr1\tsrc\tgene\t10\t200\t.\t.\t.\t.\n"
       "##FASTA\n"
       ">chr1\nACGT\n"
       "chr1\tsrc\tgene\tx\ty\t.\t+\t.\tID=never\n")


def test_gff3_lines(tmp_path):
    p = tmp_path / "a.gff3"
    p.write_text(GFF)
    want = [("g1", "gene", "chr1", 10, 200, "+"), ("m1", "mRNA", "chr1", 10, 200, "+"), ("chr1:10-50:-", "exon", "chr1", 10, 50, "-"),
            ("g2", "gene", "chr2", 5, 5, "."), ("chr1:10-200:.", "gene", "chr1", 10, 200, ".")]
    assert loci.read_gff(str(p)) == want == R.read_gff(str(p))
    assert loci.read_loci(str(p)) == want and loci.read_loci(str(p), "gff3", ["gene"]) == [want[0], want[3], want[4]]
    assert loci.read_gff(str(p), ["exon", "mRNA"]) == want[1:3] == R.read_gff(str(p), ["exon", "mRNA"])
    assert loci.read_gff(str(p), ["none"]) == []


@pytest.mark.parametrize("line,why", [
    ("chr1\tsrc\tgene\t10\t200\t.\t+\t.\n", "9 columns"),
    ("chr1\tsrc\n", "9 columns"),
    ("chr1\tsrc\tgene\t1.5\t200\t.\t+\t.\tID=a\n", "whole numbers"),
    ("chr1\tsrc\tgene\t10\t\t.\t+\t.\tID=a\n", "whole numbers"),
    ("chr1\tsrc\tgene\t0\t200\t.\t+\t.\tID=a\n", "before position 1"),
    ("chr1\tsrc\tgene\t201\t200\t.\t+\t.\tID=a\n", "behind its end"),
    ("chr1\tsrc\tgene\t10\t200\t.\t*\t.\tID=a\n", "strand"),
    ("chr1\tsrc\tgene\t10\t200\t.\t\t.\tID=a\n", "strand"),
    ("chr1\tsrc\texon\t10\t20\t.\t+\t.\tID=ok\n", "occurs twice"),
])
def test_gff3_refusals_name_file_and_line(tmp_path, line, why):
    p = tmp_path / "bad.gff3"
    p.write_text("##gff-version 3\nchr1\tsrc\tgene\t1\t9\t.\t+\t.\tID=ok\n" + line)
    with pytest.raises(ValueError) as e:
        loci.read_gff(str(p))
    assert why in str(e.value) and "%s line 3" % p in str(e.value)
    if why == "occurs twice":
        assert "-t" in str(e.value) and len(loci.read_gff(str(p), ["gene"])) == 1
    with pytest.raises(R.Refused) as e:
        R.read_gff(str(p))
    assert "line 3" in str(e.value)


def test_same_place_with_two_names_is_fine(tmp_path):
    p = tmp_path / "a.gff3"
    p.write_text("c\ts\tgene\t1\t9\t.\t+\t.\tID=a\nc\ts\tgene\t1\t9\t.\t+\t.\tID=b\n")
    assert [l[0] for l in loci.read_gff(str(p))] == ["a", "b"]


BED = ("track name=x\n"
       "browser position chr1:1-100\n"
       "# comment\n"
       "\n"
       "chr1\t0\t10\n"
       "chr1\t9\t10\tnamed\t0\t-\n"
       "chr1\t20\t30\t.\t0\t+\r\n"
       "chr2\t5\t6\tfour\n"
       "chr2\t7\t9\tfive\t100\n"
       "chr2\t7\t9\tsix\t100\t.\t7\t9\n")


def test_bed_lines(tmp_path):
    p = tmp_path / "a.bed"
    p.write_text(BED)
    want = [("chr1:1-10", ".", "chr1", 1, 10, "."), ("named", ".", "chr1", 10, 10, "-"), ("chr1:21-30", ".", "chr1", 21, 30, "+"),
            ("four", ".", "chr2", 6, 6, "."), ("five", ".", "chr2", 8, 9, "."), ("six", ".", "chr2", 8, 9, ".")]
    assert loci.read_loci(str(p)) == want == R.read_bed(str(p))
    q = tmp_path / "a.txt"
    q.write_text(BED)
    assert loci.read_loci(str(q), "bed") == want
    with pytest.raises(ValueError):
        loci.read_loci(str(q))                                                    # auto takes it as GFF3


@pytest.mark.parametrize("line,why", [
    ("chr1\t5\n", "3 columns"),
    ("chr1 5 9\n", "3 columns"),
    ("chr1\tx\t9\n", "whole numbers"),
    ("chr1\t-1\t9\n", "before position 1"),
    ("chr1\t9\t9\n", "behind its end"),
    ("chr1\t5\t9\tn\t0\tx\n", "strand"),
    ("chr1\t5\t9\tok\n", "occurs twice"),
    ("chr1\t0\t4\n", "occurs twice"),
])
def test_bed_refusals_name_file_and_line(tmp_path, line, why):
    p = tmp_path / "bad.bed"
    p.write_text("chr1\t0\t4\tok\nchr1\t0\t4\n" + line)
    with pytest.raises(ValueError) as e:
        loci.read_bed(str(p))
    assert why in str(e.value) and "%s line 3" % p in str(e.value)
    with pytest.raises(R.Refused):
        R.read_bed(str(p))


def test_phas_lines(tmp_path):
    row = b"%s\t%d\t%d\t3\t%d\t21\t10\t1e-5\t100\t200\n"
    p = tmp_path / "x.phas.tsv"
    p.write_bytes(phasing.HEADER + row % (b"chr1", 100, 310, 121) + row % (b"chr 2", 5, 215, 5))
    want = [("chr1:100-310", "PHAS", "chr1", 100, 310, "."), ("chr 2:5-215", "PHAS", "chr 2", 5, 215, ".")]
    assert loci.read_loci(str(p)) == want == R.read_phas(str(p)) and loci.read_loci(str(p), "phas") == want
    for body, why, line in ((b"chr1\t100\n", "line 2: not a line of a phasing output", 2),
                            (row % (b"chr1", 100, 310, 121) + row % (b"chr1", 100, 310, 100), "occurs twice", 3),
                            (row % (b"chr1", 0, 310, 121), "before position 1", 2),
                            (row % (b"chr1", 311, 310, 121), "behind its end", 2)):
        p.write_bytes(phasing.HEADER + body)
        with pytest.raises(ValueError) as e:
            loci.read_phas(str(p))
        assert why in str(e.value) and str(p) in str(e.value) and "line %d" % line in str(e.value)
    p.write_bytes(b"not a header\n")
    with pytest.raises(ValueError) as e:
        loci.read_phas(str(p))
    assert "line 1: not the header line" in str(e.value)


def test_keep_loci_drops_unknown_contigs_and_refuses_the_rest():
    all_loci = [("a", ".", "chr1", 1, 100, "."), ("b", ".", "nope", 1, 10, "+"), ("c", ".", "chr2", 50, 50, "-"), ("d", ".", "nope2", 1, 1, ".")]
    kept, dropped = loci.keep_loci(all_loci, ["chr2", "chr1", "chr2"], [50, 100, 10])
    assert kept == [all_loci[0], all_loci[2]] and dropped == 2 and R.keep(all_loci, ["chr2", "chr1", "chr2"], [50, 100, 10]) == (kept, 2)
    assert loci.locus_array(kept, ["chr2", "chr1", "chr2"]).tolist() == [(1, 2, 1, 100), (0, 1, 50, 50)]
    with pytest.raises(ValueError) as e:
        loci.keep_loci(all_loci, ["chr2", "chr1"], [49, 100])
    assert "locus c ends at 50, beyond the end of sequence chr2 (LN:49)" in str(e.value)
    with pytest.raises(ValueError) as e:
        loci.keep_loci(all_loci, ["other"], [49])
    assert "no locus" in str(e.value)
    many = [("n", ".", "c", 1, 1, ".")] * ((1 << 24) + 1)
    with pytest.raises(ValueError) as e:
        loci.keep_loci(many, ["c"], [5])
    assert "more than 16777216 loci" in str(e.value)
    assert len(loci.keep_loci(many[:-1], ["c"], [5])[0]) == 1 << 24


# ---------------------------------------------------------------------------------------------------- the ABI
def test_abi_entries_are_declared(tmp_path):
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_locus_scan(", "MirpLocusSpan", "MirpLocusOpts", "MIRP_LOCI_CHUNK", "MIRP_LOCI_MAX"):
        assert name in header
    assert capi.ABI_VERSION == 17
    assert int(re.search(r"#define MIRP_LOCI_CHUNK\s+(\d+)", header).group(1)) == capi.LOCI_CHUNK
    assert int(re.search(r"#define MIRP_LOCI_MAX\s+(\d+)", header).group(1)) == capi.LOCI_MAX == loci.MAX_LOCI == 1 << 24
    assert capi.LOCI_CHUNK % 64 == 0 and len(capi.LOCUS_STATS) == 5
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the struct layout with")
    lf, of = ["tid", "strand", "start", "end"], ["contig_len", "n_contigs", "n_samples", "stranded", "reserved"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirprefer.h"\nint main(void) {\n'
                   ' printf("%zu %zu", sizeof(MirpLocusSpan), sizeof(MirpLocusOpts));\n' +
                   "".join(' printf(" %%zu", offsetof(MirpLocusSpan, %s));\n' % f for f in lf) +
                   "".join(' printf(" %%zu", offsetof(MirpLocusOpts, %s));\n' % f for f in of) + ' printf("\\n");\n return 0;\n}\n')
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got[:2] == [capi.LOCUS_DTYPE.itemsize, ctypes.sizeof(capi.LocusOpts)] == [24, 24]
    assert got[2:6] == [capi.LOCUS_DTYPE.fields[f][1] for f in lf] and list(capi.LOCUS_DTYPE.names) == lf
    assert got[6:] == [getattr(capi.LocusOpts, f).offset for f in of] and [f for f, _ in capi.LocusOpts._fields_] == of


def test_the_library_exports_the_symbol():
    lib = capi.load_library()
    assert lib.mirp_locus_scan.restype is ctypes.c_int and lib.mirp_abi_version() == 17
    # arguments are checked before a device is touched: a null context is refused
    assert lib.mirp_locus_scan(None, None, 0, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "mir-prefer_amd", "csrc", "loci_kernels.hip"), "-o", str(tmp_path / "loci_kernels.o")]
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
    for kernel, instances in (("lc_maxlen_kernel", 1), ("lc_range_kernel", 2), ("lc_count_kernel", 1), ("lc_key_kernel", 1), ("lc_run_kernel", 1),
                              ("lc_table_kernel", 1), ("lc_major_kernel", 2), ("lc_out_kernel", 1)):
        mine = [v for k, v in report.items() if kernel in k]
        assert len(mine) == instances and all(v["ScratchSize"] == 0 and v["VGPRs"] <= 64 for v in mine), (kernel, mine)


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.loci"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))


def test_option_errors_exit_2_before_a_device(tmp_path, capsys):
    sam, gff, bed = tmp_path / "a.sam", tmp_path / "l.gff3", tmp_path / "l.bed"
    sam.write_bytes(b"@SQ\tSN:c\tLN:100\n")
    gff.write_text("c\ts\tgene\t1\t9\t.\t+\t.\tID=a\n")
    bed.write_text("c\t0\t9\n")
    s, g = str(sam), str(gff)
    bad = [[], [g], ["--format", "gtf", g, s], ["--format", "", g, s], ["-t", "", g, s], ["-t", "gene,,exon", g, s], ["-t", "gene", str(bed), s],
           ["-t", "gene", "--format", "phas", g, s], ["--device", "-1", g, s], ["--device", "x", g, s], ["-o", "", g, s], ["-g", "", g, s], ["-x", g, s]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            loci.parse_args(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    for args in (bad[0], bad[2], bad[6]):
        r = run_cli(args, tmp_path)
        assert r.returncode == 2 and b"Error: " not in r.stderr, (args, r.stderr)
    assert not list(tmp_path.glob("*.tsv"))
    o, path, sams, types, base = loci.parse_args(["-t", "gene,exon", "-t", "mRNA", "-s", g, s, s + "2"])
    assert (path, sams, types, base, o.stranded, o.format, o.device) == (g, [s, s + "2"], ["gene", "exon", "mRNA"], s + ".loci", True, "auto", 0)
    assert loci.parse_args(["-o", "x/out.tsv", g, s])[4] == "x/out" and loci.parse_args(["-o", "out", g, s])[2:4] == ([s], None)
    assert loci.parse_args(["-t", "gene", "--format", "gff3", str(bed), s])[3] == ["gene"]
    assert loci.output_paths("b") == ["b.tsv", "b.counts.tsv"]
    assert [loci.file_format("auto", n) for n in ("a.bed", "a.phas.tsv", "a.tsv", "a.gff3", "a.BED")] == ["bed", "phas", "gff3", "gff3", "gff3"]
    with pytest.raises(SystemExit) as e:
        loci.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--format", "--type", "--stranded", "--output", "--genome", "--device"):
        assert opt in text


def test_missing_and_refused_inputs_exit_255_and_leave_no_output(tmp_path):
    sam, gff = tmp_path / "a.sam", tmp_path / "l.gff3"
    sam.write_bytes(b"@SQ\tSN:c\tLN:100\n")
    gff.write_text("c\ts\tgene\t1\t9\t.\t+\t.\tID=a\nc\ts\tgene\t9\t1\t.\t+\t.\tID=b\n")
    stale = loci.output_paths(str(sam) + ".loci")
    for args, why in (([str(gff), str(sam), str(tmp_path / "nope.sam")], "nope.sam does not exist"),
                      ([str(tmp_path / "nope.gff3"), str(sam)], "nope.gff3 does not exist"),
                      (["-g", str(tmp_path / "nope.fa"), str(gff), str(sam)], "nope.fa does not exist"),
                      ([str(gff), str(sam)], "l.gff3 line 2: locus b has its start behind its end")):
        for p in stale:
            open(p, "w").write("stale\n")
        r = run_cli(args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr)
        if "nope.sam" not in why and "nope.gff3" not in why and "nope.fa" not in why:
            assert not any(os.path.exists(p) for p in stale)
    probe = ("import sys\nfrom mir_prefer_amd import loci\nrc = loci.main([%r, %r])\nprint(rc, 'mir_prefer_amd.capi' in sys.modules)\n"
             % (str(gff), str(sam)))
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.stdout.split() == [b"255", b"False"], (r.stdout, r.stderr)            # a refused loci file never loads the library
