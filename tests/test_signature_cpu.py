"""CPU tests of the signature verb: the worked examples of the definition as literals against both restatements of
tests/signature_restatement.py (one duplex, the pair shifted by one base either way, the other near misses, the locus edges, the contig
join, min() in both directions past 32 bits, the ties of the major duplex, --min-reads); the two restatements against each other on seeded
inputs and the module's file writer against them; the option errors of the command line, which exit 2 without opening a device, among them
--contigs together with a loci file and a loci file missing without --contigs; the struct layouts against the C header, the new symbol and
the unchanged ABI version; and that no new kernel uses scratch."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from mir_prefer_amd import capi, signature
from tests import signature_restatement as R
from tests.test_clusters_cpu import ROOT, make_records, random_records, random_seqs
from tests.test_loci_cpu import L, random_loci


def both(rows, loci_rows, lens, **kw):
    """The two restatements of the scan agree; -> (rows, H, sites, stats) of the numpy one."""
    alns = make_records(rows)
    arr = L(*loci_rows)
    got, H, sites, stats = R.scan_numpy(alns, arr, lens, **kw)
    plain = R.scan_plain(alns, arr, **kw)
    o = R.options(**kw)
    want_sites = []
    for q, c in enumerate(plain):
        paired = [min(dp, dm) for _, _, dp, dm in c["duplexes"]]
        assert (int(got["reads"][q]), int(got["plus_reads"][q]), H[q].tolist(), int(got["duplexes"][q]), int(got["duplex_reads"][q])) == \
            (c["reads"], c["plus"], c["H"], len(paired), sum(paired)), q
        major = c["duplexes"][paired.index(max(paired))] if paired else (0, 0, 0, 0)
        assert tuple(int(got[f][q]) for f in ("major_pos", "major_len", "major_plus", "major_minus")) == major, q
        want_sites += [(q, p, dp, dm, ln, 0) for (p, ln, dp, dm), m in zip(c["duplexes"], paired) if m >= o["min_reads"]]
    assert sites.tolist() == want_sites and stats["sites"] == len(want_sites) and not got["reserved"].any()
    return got, H, sites, stats


def hist(H, q=0):
    """{overlap: H} of the overlaps that are not zero"""
    return {k + 1: int(v) for k, v in enumerate(H[q]) if v}


# ---------------------------------------------------------------------------------------------------- the rule
def test_one_duplex():
    got, H, sites, st = both([(0, 100, 5, 21, 0), (0, 98, 3, 21, 1)], [(0, ".", 1, 1000)], [1000], min_reads=1)
    assert hist(H) == {19: 3} and got[["reads", "plus_reads", "duplexes", "duplex_reads"]].tolist() == [(8, 5, 1, 3)]
    assert got[["major_pos", "major_len", "major_plus", "major_minus"]].tolist() == [(100, 21, 5, 3)]
    assert sites.tolist() == [(0, 100, 5, 3, 21, 0)] and st == {"records": 2, "kept": 2, "u_entries": 1, "v_entries": 1, "jobs": 1, "sites": 1}


@pytest.mark.parametrize("minus,overlap", [((99, 21), 20), ((97, 21), 18), ((98, 22), 20)])
def test_near_misses_shift_the_overlap_and_are_no_duplex(minus, overlap):
    got, H, sites, _ = both([(0, 100, 5, 21, 0), (0, minus[0], 3, minus[1], 1)], [(0, ".", 1, 1000)], [1000], min_reads=1)
    assert hist(H) == {overlap: 3} and int(got["duplexes"][0]) == 0 and len(sites) == 0 and int(got["reads"][0]) == 8


def test_overhang_selects_the_matching_pair():
    rows = [(0, 100, 5, 21, 0), (0, 100, 2, 21, 1), (0, 99, 3, 21, 1), (0, 98, 4, 21, 1), (0, 97, 6, 21, 1)]
    for o, minus in ((0, 2), (1, 3), (2, 4), (3, 6)):
        got, H, sites, _ = both(rows, [(0, ".", 1, 1000)], [1000], overhang=o, min_reads=1)
        assert sites.tolist() == [(0, 100, 5, minus, 21, 0)] and hist(H) == {21: 2, 20: 3, 19: 4, 18: 5}
    assert int(both(rows, [(0, ".", 1, 1000)], [1000], overhang=4, min_reads=1)[0]["duplexes"][0]) == 0


def test_min_in_both_directions_past_32_bits():
    top = (1 << 32) - 1
    for a, b in ((0, 1), (1, 0)):                                               # two '+' against one '-', and the reverse
        pos = {0: 100, 1: 98}
        rows = [(0, pos[a], top, 21, a), (0, pos[a], top, 21, a), (0, pos[b], 7, 21, b)]
        got, H, sites, _ = both(rows, [(0, ".", 1, 1000)], [1000])
        assert hist(H) == {19: 7} and int(got["reads"][0]) == 2 * top + 7 and int(got["duplex_reads"][0]) == 7
        assert sorted(sites[["plus_reads", "minus_reads"]].tolist()[0]) == [7, 2 * top]
    rows = [(0, 100, top, 21, 0)] * 3 + [(0, 98, top, 21, 1)] * 2
    got, H, sites, _ = both(rows, [(0, ".", 1, 1000)], [1000])
    assert hist(H) == {19: 2 * top} and int(got["major_plus"][0]) == 3 * top and int(got["major_minus"][0]) == 2 * top > 1 << 32


def test_locus_edges_are_five_prime_ends():
    # '+' 5' ends at 100 and 200, '-' 5' ends at 118 (pos 98) and 218 (pos 198)
    rows = [(0, 100, 5, 21, 0), (0, 98, 3, 21, 1), (0, 200, 9, 21, 0), (0, 198, 4, 21, 1)]
    loc = [(0, ".", 100, 118), (0, ".", 101, 118), (0, ".", 100, 117), (0, ".", 99, 119), (0, ".", 1, 1000), (0, ".", 119, 199), (0, ".", 100, 118),
           (0, ".", 110, 210), (0, ".", 200, 217), (0, ".", 200, 218)]
    got, H, sites, _ = both(rows, loc, [1000], min_reads=1)
    assert got["reads"].tolist() == [8, 3, 5, 8, 21, 0, 8, 12, 9, 13] and got["plus_reads"].tolist() == [5, 0, 5, 5, 14, 0, 5, 9, 9, 9]
    assert got["duplexes"].tolist() == [1, 0, 0, 1, 2, 0, 1, 0, 0, 1] and got["duplex_reads"].tolist() == [3, 0, 0, 3, 7, 0, 3, 0, 0, 4]
    assert [hist(H, q) for q in range(10)] == [{19: 3}, {}, {}, {19: 3}, {19: 7}, {}, {19: 3}, {}, {}, {19: 4}]
    # order (locus, p, L); the duplex shared by loci 0, 3, 4 and 6 is listed under each
    assert sites[["locus", "pos"]].tolist() == [(0, 100), (3, 100), (4, 100), (4, 200), (6, 100), (9, 200)]
    assert got[0:1].tobytes() == got[6:7].tobytes()                             # the duplicate has the same row


def test_contig_join_never_pairs():
    K = 30
    rows = [(0, 500, 5, 21, 0)] + [(1, y - 20, 3, 21, 1) for y in range(1, K + 1)]   # '+' at the last base of contig 0, '-' 5' ends at 1..K of contig 1
    got, H, sites, _ = both(rows, [(0, ".", 1, 500), (1, ".", 1, 300), (1, ".", 1, 1)], [500, 300])
    assert not H.any() and not got["duplexes"].any() and got["reads"].tolist() == [5, 3 * K, 3] and got["plus_reads"].tolist() == [5, 0, 0]


def test_length_filter():
    rows = [(0, 100, 5, 19, 0), (0, 100, 6, 20, 0), (0, 100, 7, 25, 0), (0, 100, 8, 26, 0),
            (0, 98, 1, 19, 1), (0, 98, 2, 20, 1), (0, 98, 3, 25, 1), (0, 98, 4, 26, 1)]
    got, H, sites, st = both(rows, [(0, ".", 1, 1000)], [1000], min_reads=1)
    assert int(got["reads"][0]) == 6 + 7 + 2 + 3 and st["kept"] == 4 and sites[["len", "plus_reads", "minus_reads"]].tolist() == [(20, 6, 2), (25, 7, 3)]
    assert hist(H) == {18: 2, 23: 3}                                            # U(100) = 13 against V(117) = 2 and V(122) = 3
    got, H, sites, st = both(rows, [(0, ".", 1, 1000)], [1000], min_reads=1, min_len=19, max_len=26)
    assert int(got["reads"][0]) == 36 and st["kept"] == 8 and len(sites) == 4


def test_max_overlap_cuts_the_walk():
    rows = [(0, 100, 5, 21, 0), (0, 100 + 30 - 21, 3, 21, 1), (0, 100 + 31 - 21, 4, 21, 1), (0, 80, 2, 21, 1)]   # '-' 5' ends at 129 (k = 30), 130 (k = 31), 100 (k = 1)
    assert hist(both(rows, [(0, ".", 1, 1000)], [1000])[1]) == {1: 2, 30: 3}
    assert hist(both(rows, [(0, ".", 1, 1000)], [1000], max_overlap=31)[1]) == {1: 2, 30: 3, 31: 4}
    assert hist(both(rows, [(0, ".", 1, 1000)], [1000], max_overlap=1)[1]) == {1: 2}
    assert hist(both(rows, [(0, ".", 1, 129)], [1000])[1]) == {1: 2, 30: 3} and hist(both(rows, [(0, ".", 1, 128)], [1000])[1]) == {1: 2}


def test_major_duplex_ties():
    def major(rows):
        g = both(rows, [(0, ".", 1, 900)], [1000], min_reads=1)[0][0]
        return [int(g[f]) for f in ("major_pos", "major_len", "major_plus", "major_minus")]
    assert major([(0, 100, 5, 21, 0), (0, 98, 3, 21, 1), (0, 200, 3, 21, 0), (0, 198, 9, 21, 1)]) == [100, 21, 5, 3]       # m = 3 twice: the smaller p
    assert major([(0, 100, 5, 24, 0), (0, 98, 3, 24, 1), (0, 100, 3, 21, 0), (0, 98, 9, 21, 1)]) == [100, 21, 3, 9]        # the same p: the shorter L
    assert major([(0, 100, 5, 21, 0), (0, 98, 3, 21, 1), (0, 200, 4, 21, 0), (0, 198, 9, 21, 1)]) == [200, 21, 4, 9]       # the larger m wins


def test_min_reads_lists_from_m():
    rows = [(0, 100, 5, 21, 0), (0, 98, 9, 21, 1)]
    for mr, n in ((4, 1), (5, 1), (6, 0)):
        got, _, sites, _ = both(rows, [(0, ".", 1, 900)], [1000], min_reads=mr)
        assert len(sites) == n and int(got["duplexes"][0]) == 1 and int(got["duplex_reads"][0]) == 5


def test_host_columns():
    H = [0] * 30
    assert signature.host_columns(0, H, 0) == (0, 0, "NA", "NA") == R.host_columns(0, H, 0)
    H[18], H[3] = 7, 7
    peak, top, z, frac = signature.host_columns(20, H, 5)
    assert (peak, top, frac) == (4, 7, "0.5000") and z == "%.3f" % ((7 - 14 / 30) / (((28 * (14 / 30) ** 2 + 2 * (7 - 14 / 30) ** 2) / 30) ** 0.5))
    assert signature.host_columns(3, [4] * 30, 1) == (1, 4, "NA", "0.6667")
    assert signature.host_columns(10, [0, 9], 5) == (2, 9, "1.000", "1.0000")


def test_worked_files():
    names = ["chrB", "chrA"]
    alns = make_records([(0, 100, 8, 21, 0, 0), (0, 100, 2, 21, 0, 1), (0, 98, 6, 21, 1, 1), (0, 300, 4, 24, 0, 0), (0, 298, 4, 24, 1, 0), (1, 5, 4, 30, 1, 0)])
    kept = [("a", "gene", "chrB", 90, 330, "+"), ("b", ".", "chrA", 1, 100, "."), ("a2", "PHAS", "chrB", 100, 118, "-")]
    seqs = {"chrB": b"N" * 97 + b"ttacgtacgtacgtacgtacgtaGG" + b"N" * 878, "chrA": b"ttttGCGCGCGC" * 50}
    z = "%.3f" % ((6 - 10 / 30) / (((28 * (10 / 30) ** 2 + (6 - 10 / 30) ** 2 + (4 - 10 / 30) ** 2) / 30) ** 0.5))
    want_tsv = (R.HEADER +
                b"a\tgene\tchrB\t90\t330\t24\t14\t10\t19\t6\t" + z.encode() + b"\t2\t10\t0.8333\t100\t21\t10\t6\tACGUACGUACGUACGUACGUA\n"
                b"b\t.\tchrA\t1\t100\t0\t0\t0\t0\t0\tNA\t0\t0\tNA\t0\t0\t0\t0\t*\n"
                b"a2\tPHAS\tchrB\t100\t118\t16\t10\t6\t19\t6\t5.385\t1\t6\t0.7500\t100\t21\t10\t6\tACGUACGUACGUACGUACGUA\n")
    want_ovl = (b"name\t" + b"\t".join(b"%d" % k for k in range(1, 31)) + b"\n" +
                b"a" + b"".join(b"\t%d" % {19: 6, 22: 4}.get(k, 0) for k in range(1, 31)) + b"\n" +
                b"b" + b"\t0" * 30 + b"\n" + b"a2" + b"".join(b"\t%d" % {19: 6}.get(k, 0) for k in range(1, 31)) + b"\n")
    want_dup = (R.DUPLEX_HEADER + b"a\tchrB\t100\t21\t10\t6\t6\tACGUACGUACGUACGUACGUA\tCGUACGUACGUACGUACGUAA\n"
                b"a2\tchrB\t100\t21\t10\t6\t6\tACGUACGUACGUACGUACGUA\tCGUACGUACGUACGUACGUAA\n")
    assert R.files_plain(alns, kept, names, seqs) == (want_tsv, want_ovl, want_dup)
    rows, H, sites, _ = R.scan_numpy(alns, R.locus_array(kept, names), [1000, 600])
    assert signature.format_files(kept, rows, H, sites, 2, seqs) == (want_tsv, want_ovl, want_dup)
    bare = signature.format_files(kept, rows, H, sites, 2)
    assert bare[0].split(b"\n")[1].split(b"\t")[18] == b"*" and bare[2].split(b"\n")[1].split(b"\t")[7:] == [b"*", b"*"] and bare[1] == want_ovl
    assert signature.TSV_HEADER == R.HEADER and signature.DUPLEX_HEADER == R.DUPLEX_HEADER


def duplex_records(rng, lens, n_dup, n_noise):
    """Planted duplexes of 20..25 nt with overhangs 0..3 and depths around --min-reads on top of random_records' noise and hot spots."""
    rows = []
    for _ in range(n_dup):
        t = int(rng.randint(0, len(lens)))
        ln, o = int(rng.randint(20, 26)), int(rng.choice([2, 2, 2, 0, 1, 3]))
        p = int(rng.randint(5, lens[t] - 30))
        rows += [(t, p, int(rng.randint(1, 12)), ln, 0, 0), (t, p - o, int(rng.randint(1, 12)), ln + int(rng.randint(0, 8) == 0), 1, 0)]
    noise = random_records(rng, lens, 1, n_noise, max(n_dup // 10, 1))
    return make_records(rows + [tuple(r) for r in noise.tolist()])


@pytest.mark.parametrize("seed", range(4))
def test_restatements_agree_on_random_inputs(seed):
    rng = np.random.RandomState(200 + seed)
    lens = [3000, 700, 150, 5000]
    names = ["chr%d" % i for i in range(4)]
    alns = duplex_records(rng, lens, 150, 300)
    kept = random_loci(rng, names, lens, 60)
    seqs = dict(zip(names, random_seqs(rng, lens)))
    arr = R.locus_array(kept, names)
    for kw in ({"min_len": 18, "max_len": 30, "max_overlap": 64, "overhang": 0, "min_reads": 1}, {"max_overlap": 1, "overhang": 3, "min_reads": 9}, {}):
        rows, H, sites, stats = both([tuple(r) for r in alns.tolist()], [tuple(x) for x in zip(arr["tid"].tolist(), ["."] * len(arr), arr["start"].tolist(),
                                                                                                arr["end"].tolist())], lens, **kw)
        o = R.options(**kw)
        assert signature.format_files(kept, rows, H, sites, o["overhang"], seqs) == R.files_plain(alns, kept, names, seqs, **kw)
    assert int((rows["duplexes"] == 0).sum()) > 0 and int((rows["duplexes"] > 3).sum()) > 5 and H.any()


# ---------------------------------------------------------------------------------------------------- the ABI
def test_abi_entries_are_declared(tmp_path):
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_signature_scan(", "MirpSignatureOpts", "MirpSignatureRow", "MirpDuplexSite", "MIRP_SIGNATURE_CHUNK", "MIRP_SIGNATURE_MAX_OVERLAP"):
        assert name in header
    assert capi.ABI_VERSION == 17
    assert int(re.search(r"#define MIRP_SIGNATURE_CHUNK\s+(\d+)", header).group(1)) == capi.SIGNATURE_CHUNK == R.CHUNK == 4096
    assert int(re.search(r"#define MIRP_SIGNATURE_MAX_OVERLAP\s+(\d+)", header).group(1)) == capi.SIGNATURE_MAX_OVERLAP == signature.MAX_OVERLAP == 64
    assert len(capi.SIGNATURE_STATS) == 6
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the struct layout with")
    structs = (("MirpSignatureOpts", [f for f, _ in capi.SignatureOpts._fields_]), ("MirpSignatureRow", list(capi.SIGNATURE_ROW_DTYPE.names)),
               ("MirpDuplexSite", list(capi.DUPLEX_SITE_DTYPE.names)))
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirprefer.h"\nint main(void) {\n' +
                   "".join(' printf("%%zu ", sizeof(%s));\n' % s + "".join(' printf("%%zu ", offsetof(%s, %s));\n' % (s, f) for f in fs) for s, fs in structs) +
                   ' printf("\\n");\n return 0;\n}\n')
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    want = [ctypes.sizeof(capi.SignatureOpts)] + [getattr(capi.SignatureOpts, f).offset for f in structs[0][1]]
    for dt, (_, fs) in zip((capi.SIGNATURE_ROW_DTYPE, capi.DUPLEX_SITE_DTYPE), structs[1:]):
        want += [dt.itemsize] + [dt.fields[f][1] for f in fs]
    assert got == want and (want[0], capi.SIGNATURE_ROW_DTYPE.itemsize, capi.DUPLEX_SITE_DTYPE.itemsize) == (40, 64, 40)
    assert structs[0][1] == ["contig_len", "n_contigs", "min_len", "max_len", "max_overlap", "overhang", "reserved", "min_reads"]
    assert structs[1][1] == ["reads", "plus_reads", "duplexes", "duplex_reads", "major_pos", "major_plus", "major_minus", "major_len", "reserved"]
    assert structs[2][1] == ["locus", "pos", "plus_reads", "minus_reads", "len", "reserved"]


def test_the_library_exports_the_symbol():
    lib = capi.load_library()
    assert lib.mirp_signature_scan.restype is ctypes.c_int and lib.mirp_abi_version() == 17
    # arguments are checked before a device is touched: a null context is refused
    assert lib.mirp_signature_scan(None, None, 0, None, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "mir-prefer_amd", "csrc", "signature_kernels.hip"),
           "-o", str(tmp_path / "signature_kernels.o")]
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
    for kernel, instances in (("sg_key_kernel", 1), ("sg_run_kernel", 1), ("sg_ends_kernel", 1), ("sg_place_kernel", 1), ("sg_pair_kernel", 1),
                              ("lc_range_kernel", 1), ("sg_overlap_kernel", 1), ("sg_duplex_kernel", 2), ("sg_out_kernel", 1), ("sg_emit_kernel", 1)):
        mine = [v for k, v in report.items() if kernel in k]
        assert len(mine) == instances and all(v["ScratchSize"] == 0 and v["VGPRs"] <= 64 for v in mine), (kernel, mine)
    assert len(report) == 11


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.signature"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))


def test_option_errors_exit_2_before_a_device(tmp_path, capsys):
    sam, gff, bed = tmp_path / "a.sam", tmp_path / "l.gff3", tmp_path / "l.bed"
    sam.write_bytes(b"@SQ\tSN:c\tLN:100\n")
    gff.write_text("c\ts\tgene\t1\t9\t.\t+\t.\tID=a\n")
    bed.write_text("c\t0\t9\n")
    s, g = str(sam), str(gff)
    bad = [[], [g], [s], ["--contigs"], ["--contigs", g, s], ["--contigs", str(bed), s], ["--contigs", "--format", "gff3", s], ["--contigs", "-t", "gene", s],
           ["--format", "gtf", g, s], ["-t", "", g, s], ["-t", "gene", str(bed), s], ["--min-len", "0", g, s], ["--min-len", "26", g, s],
           ["--max-len", "65536", g, s], ["--max-overlap", "0", g, s], ["--max-overlap", "65", g, s], ["--overhang", "-1", g, s], ["--overhang", "9", g, s],
           ["--overhang", "3", "--min-len", "3", "--max-len", "30", g, s], ["--min-reads", "0", g, s], ["--min-reads", "x", g, s], ["--device", "-1", g, s],
           ["-o", "", g, s], ["-g", "", g, s], ["-x", g, s]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            signature.parse_args(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    for args in (bad[1], bad[4], bad[13], bad[18]):
        r = run_cli(args, tmp_path)
        assert r.returncode == 2 and b"Error: " not in r.stderr, (args, r.stderr)
    assert not list(tmp_path.glob("*.tsv"))
    o, path, sams, types, base = signature.parse_args(["-t", "gene,exon", "-t", "mRNA", g, s, s + "2"])
    assert (path, sams, types, base, o.format, o.device, o.contigs) == (g, [s, s + "2"], ["gene", "exon", "mRNA"], s + ".signature", "auto", 0, False)
    assert (o.min_len, o.max_len, o.max_overlap, o.overhang, o.min_reads) == (20, 25, 30, 2, 5)
    o, path, sams, types, base = signature.parse_args(["--contigs", "--min-len", "3", "--max-len", "65535", "--overhang", "2", "--max-overlap", "64", s, s + "2"])
    assert (path, sams, types, base, o.contigs, o.min_len, o.max_len, o.max_overlap) == (None, [s, s + "2"], None, s + ".signature", True, 3, 65535, 64)
    assert signature.parse_args(["-o", "x/out.tsv", g, s])[4] == "x/out" and signature.parse_args(["--overhang", "8", "--min-len", "9", g, s])[0].overhang == 8
    assert signature.output_paths("b") == ["b.tsv", "b.overlaps.tsv", "b.duplexes.tsv"]
    with pytest.raises(SystemExit) as e:
        signature.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--format", "--type", "--contigs", "--min-len", "--max-len", "--max-overlap", "--overhang", "--min-reads", "--output", "--genome", "--device"):
        assert opt in text


def test_contig_loci():
    assert signature.contig_loci(["b", "a", "b", "e"], [50, 100, 10, 0]) == [("b", "contig", "b", 1, 50, "."), ("a", "contig", "a", 1, 100, ".")]
    with pytest.raises(ValueError):
        signature.contig_loci(["e"], [0])


def test_missing_and_refused_inputs_exit_255_and_leave_no_output(tmp_path):
    sam, gff = tmp_path / "a.sam", tmp_path / "l.gff3"
    sam.write_bytes(b"@SQ\tSN:c\tLN:100\n")
    gff.write_text("c\ts\tgene\t1\t9\t.\t+\t.\tID=a\nc\ts\tgene\t9\t1\t.\t+\t.\tID=b\n")
    stale = signature.output_paths(str(sam) + ".signature")
    for args, why in (([str(gff), str(sam), str(tmp_path / "nope.sam")], "nope.sam does not exist"),
                      ([str(tmp_path / "nope.gff3"), str(sam)], "nope.gff3 does not exist"),
                      (["--contigs", str(tmp_path / "nope.sam")], "nope.sam does not exist"),
                      (["-g", str(tmp_path / "nope.fa"), str(gff), str(sam)], "nope.fa does not exist"),
                      ([str(gff), str(sam)], "l.gff3 line 2: locus b has its start behind its end")):
        for p in stale:
            open(p, "w").write("stale\n")
        r = run_cli(args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr)
        if "nope" not in why:
            assert not any(os.path.exists(p) for p in stale)
    probe = ("import sys\nfrom mir_prefer_amd import signature\nrc = signature.main([%r, %r])\nprint(rc, 'mir_prefer_amd.capi' in sys.modules)\n"
             % (str(gff), str(sam)))
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.stdout.split() == [b"255", b"False"], (r.stdout, r.stderr)            # a refused loci file never loads the library
