"""CPU tests of the small-RNA clusters: a plain-Python dict restatement and a numpy restatement of all three files agree on
seeded inputs; hand cases at each boundary of the definition (pad, the first-cluster rule, the strand and Dicer calls, the major-placement ties,
the rpm ceiling, major_rna); the GFF3 read back by gffmask; the MirpCluster dtype against the C struct; and the option errors of the command
line, which exit 2 without opening a device."""
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd import clusters, gffmask
from mir_prefer_amd.capi import CLUSTER_DTYPE
from mir_prefer_amd.synth import ALN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMP = bytes.maketrans(b"ATGCU", b"UACGA")


# ---------------------------------------------------------------------------------------------------- restatements
def restate_plain(alns, names, lens, sample_names, T, pad, seqs=None):
    """The definition of §16 word by word with dicts: per-position coverage, islands, clusters, the first-cluster assignment, the sums, the
    calls and the three files."""
    cov = {}
    for r in alns.tolist():
        tid, pos, depth, ln = r[0], r[1], r[2], r[3]
        for p in range(max(pos, 1), min(pos + ln - 1, lens[tid]) + 1):
            cov[(tid, p)] = cov.get((tid, p), 0) + depth
    islands = []
    for tid, p in sorted(k for k, v in cov.items() if v >= T):
        if islands and islands[-1][0] == tid and islands[-1][2] == p - 1:
            islands[-1][2] = p
        else:
            islands.append([tid, p, p])
    cl = []
    for tid, a, b in islands:
        if cl and cl[-1]["tid"] == tid and a - cl[-1]["end"] - 1 <= pad:
            cl[-1]["end"] = b
        else:
            cl.append({"tid": tid, "start": a, "end": b, "reads": 0, "plus": 0, "sizes": [0] * 7, "samples": [0] * len(sample_names), "pl": {}})
    for r in alns.tolist():
        tid, pos, depth, ln, strand, sample = r
        for c in cl:
            if c["tid"] == tid and pos <= c["end"] and pos + ln - 1 >= c["start"]:
                c["reads"] += depth
                c["plus"] += depth if strand == 0 else 0
                c["sizes"][0 if ln < 20 else 6 if ln > 24 else ln - 19] += depth
                c["samples"][sample] += depth
                c["pl"][(pos, strand, ln)] = c["pl"].get((pos, strand, ln), 0) + depth
                break
    tsv = [b"name\tcontig\tstart\tend\treads\tplus_reads\tstrand\tdicer_call\tplacements\tmajor_pos\tmajor_strand\tmajor_len\tmajor_reads\t"
           b"major_rna\tshort\tr20\tr21\tr22\tr23\tr24\tlong\n"]
    cnt = [b"name" + b"".join(b"\t" + s.encode() for s in sample_names) + b"\n"]
    gff = [b"##gff-version 3\n"]
    for k, c in enumerate(cl):
        name = b"Cluster_%d" % (k + 1)
        reads, plus = c["reads"], c["plus"]
        sc = b"+" if 5 * plus >= 4 * reads else b"-" if 5 * plus <= reads else b"."
        d = c["sizes"][1:6]
        best = [20 + i for i in range(5) if d[i] == max(d)]
        dc = b"N" if 5 * sum(d) < 4 * reads or len(best) > 1 else str(best[0]).encode()
        (mp, ms, ml), mr = min(c["pl"].items(), key=lambda kv: (-kv[1], kv[0]))
        if seqs is None:
            rna = b"*"
        else:
            s = bytes(seqs[c["tid"]][max(mp - 1, 0):mp - 1 + ml]).upper()
            rna = s.translate(_COMP)[::-1] if ms else s.replace(b"T", b"U")
        tsv.append(b"\t".join([name, names[c["tid"]].encode()] + [str(x).encode() for x in (c["start"], c["end"], reads, plus)] + [sc, dc] +
                              [str(x).encode() for x in (len(c["pl"]), mp)] + [b"+-"[ms:ms + 1], str(ml).encode(), str(mr).encode(), rna] +
                              [str(x).encode() for x in c["sizes"]]) + b"\n")
        cnt.append(name + b"".join(b"\t%d" % x for x in c["samples"]) + b"\n")
        gff.append(b"%s\tmir_prefer_amd\tsRNA_cluster\t%d\t%d\t.\t%s\t.\tID=%s;DicerCall=%s;Reads=%d\n" % (names[c["tid"]].encode(), c["start"], c["end"],
                                                                                                        sc, name, dc, reads))
    return b"".join(tsv), b"".join(cnt), b"".join(gff)


def clusters_numpy(alns, lens, n_samples, T, pad):
    """The clusters as capi.cluster_scan returns them (CLUSTER_DTYPE array, [clusters, samples] counts, stats), vectorised: sorted coverage
    events and their cumulative sum, searchsorted assignment, np.add.at sums, np.unique placements."""
    lens = np.asarray(lens, np.int64)
    tid = alns["tid"].astype(np.int64)
    pos = alns["pos"].astype(np.int64)
    ln = alns["len"].astype(np.int64)
    dep = alns["depth"].astype(np.int64)
    s = np.maximum(pos, 1)
    e = np.minimum(pos + ln, lens[tid] + 1)
    ok = s < e
    sk, ek = (tid << 32) + s, (tid << 32) + e
    keys = np.concatenate([sk[ok], ek[ok]])
    delta = np.concatenate([dep[ok], -dep[ok]])
    order = np.argsort(keys, kind="stable")
    keys, cum = keys[order], np.cumsum(delta[order])
    last = np.ones(len(keys), bool)
    last[:-1] = keys[1:] != keys[:-1]
    ukey, ucov = keys[last], cum[last]
    prev = np.concatenate([[0], ucov[:-1]])
    istart = ukey[(ucov >= T) & (prev < T)]
    iend = ukey[(ucov < T) & (prev >= T)] - 1
    head = np.ones(len(istart), bool)
    if len(istart) > 1:
        head[1:] = ((istart[1:] >> 32) != (iend[:-1] >> 32)) | (istart[1:] - iend[:-1] - 1 > pad)
    cstart = istart[head]
    cend = iend[np.concatenate([head[1:], [True]])] if len(istart) else iend
    nc = len(cstart)
    c = np.searchsorted(cend, sk, "left")
    cc = np.minimum(c, max(nc - 1, 0))
    asg = ok & (c < nc) & (cstart[cc] <= (tid << 32) + np.minimum(pos + ln, lens[tid] + 1) - 1) if nc else np.zeros(len(alns), bool)
    ci = c[asg]
    out = np.zeros(nc, CLUSTER_DTYPE)
    out["tid"] = cstart >> 32
    out["start"], out["end"] = cstart & 0xffffffff, cend & 0xffffffff
    for field, w in (("reads", dep), ("plus_reads", np.where(alns["strand"] == 0, dep, 0))):
        v = np.zeros(nc, np.int64)
        np.add.at(v, ci, w[asg])
        out[field] = v
    cls = np.where(ln < 20, 0, np.where(ln > 24, 6, ln - 19))
    sizes = np.zeros((nc, 7), np.int64)
    np.add.at(sizes, (ci, cls[asg]), dep[asg])
    out["sizes"] = sizes
    counts = np.zeros((nc, n_samples), np.int64)
    np.add.at(counts, (ci, alns["sample"][asg].astype(np.int64)), dep[asg])
    pk = np.zeros(int(asg.sum()), [("c", "<i8"), ("pos", "<i8"), ("strand", "<i8"), ("len", "<i8")])
    pk["c"], pk["pos"], pk["strand"], pk["len"] = ci, pos[asg], alns["strand"][asg], ln[asg]
    up, inv = np.unique(pk, return_inverse=True)
    psum = np.zeros(len(up), np.int64)
    np.add.at(psum, inv.ravel(), dep[asg])
    out["placements"] = np.bincount(up["c"], minlength=nc) if nc else []
    o = np.lexsort((up["len"], up["strand"], up["pos"], -psum, up["c"]))
    first = o[np.concatenate([[True], up["c"][o][1:] != up["c"][o][:-1]])] if len(o) else o
    out["major_pos"], out["major_strand"], out["major_len"], out["major_reads"] = up["pos"][first], up["strand"][first], up["len"][first], psum[first]
    stats = {"records": len(alns), "total": int(dep.sum()), "islands": len(istart), "clusters": nc, "assigned": int(asg.sum())}
    return out, counts, stats


def restate_numpy(alns, names, lens, sample_names, T, pad, seqs=None):
    got, counts, _ = clusters_numpy(alns, lens, len(sample_names), T, pad)
    return clusters.format_files(names, got, counts, sample_names, seqs)


# ---------------------------------------------------------------------------------------------------- inputs
def make_records(rows):
    """rows of (tid, pos, depth, len, strand[, sample]) -> ALN_DTYPE array sorted stably by (tid, pos)."""
    a = np.zeros(len(rows), ALN_DTYPE)
    if rows:
        r = np.array([tuple(x) + (0,) * (6 - len(x)) for x in rows], dtype=np.int64)
        a["tid"], a["pos"], a["depth"], a["len"], a["strand"], a["sample"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5]
    return a[np.lexsort((a["pos"], a["tid"]))]


def random_records(rng, lens, n_samples, n_noise, n_hot, lengths=(15, 18, 20, 21, 21, 22, 23, 24, 24, 24, 26, 30)):
    """Hot spots (many reads piled on a few placements, both strands, several sizes), noise of mixed lengths, multi-mapped copies and
    reads that run past the contig end (up to POS = LN + 1, which the ingest accepts) or start at position 0."""
    rows = []
    for _ in range(n_hot):
        tid = int(rng.randint(0, len(lens)))
        c = int(rng.randint(1, lens[tid]))
        for _ in range(int(rng.randint(3, 40))):
            rows.append((tid, min(max(0, c + int(rng.randint(-60, 60))), lens[tid] + 1), int(rng.randint(1, 50)), int(rng.choice(lengths)), int(rng.randint(0, 2)),
                         int(rng.randint(0, n_samples))))
    for _ in range(n_noise):
        tid = int(rng.randint(0, len(lens)))
        rows.append((tid, int(rng.randint(0, lens[tid] + 2)), int(rng.randint(1, 8)), int(rng.choice(lengths)), int(rng.randint(0, 2)),
                     int(rng.randint(0, n_samples))))
    for i in rng.randint(0, len(rows), size=len(rows) // 10):
        tid = int(rng.randint(0, len(lens)))
        rows.append((tid, int(rng.randint(1, lens[tid])),) + tuple(rows[i][2:]))
    return make_records(rows)


def random_seqs(rng, lens):
    return [bytes(np.frombuffer(b"ACGTacgtNR", np.uint8)[rng.randint(0, 10, ln)]) for ln in lens]


# ---------------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("seed", range(6))
def test_numpy_restatement_agrees_with_the_plain_one(seed):
    rng = np.random.RandomState(seed)
    lens = [3000, 700, 150, 5000]
    names = ["chr%d" % i for i in range(len(lens))]
    samples = ["s0", "s1", "s0"]
    alns = random_records(rng, lens, 3, 400, 25)
    seqs = random_seqs(rng, lens)
    total = int(alns["depth"].sum())
    for spec, pad in ((("reads", 1), 75), (("reads", 20), 0), (("rpm", Fraction(5000)), 30), (("rpm", Fraction(1, 2)), 75), (("reads", 60), 200)):
        T = clusters.threshold(spec, total)
        want = restate_plain(alns, names, lens, samples, T, pad, seqs if pad == 30 else None)
        assert restate_numpy(alns, names, lens, samples, T, pad, seqs if pad == 30 else None) == want, (seed, spec, pad)
        if spec == ("reads", 20):
            assert want[0].count(b"\n") > 3


# ---------------------------------------------------------------------------------------------------- hand cases
def _both(rows, lens, T=1, pad=75, samples=("s",), seqs=None):
    alns = make_records(rows)
    names = ["chr%d" % i for i in range(len(lens))]
    a = restate_plain(alns, names, lens, list(samples), T, pad, seqs)
    assert restate_numpy(alns, names, lens, list(samples), T, pad, seqs) == a
    return [ln.split(b"\t") for ln in a[0].split(b"\n")[1:-1]], [ln.split(b"\t") for ln in a[1].split(b"\n")[1:-1]], a


def test_gap_of_pad_merges_pad_plus_one_does_not():
    rows = [(0, 100, 1, 20, 0), (0, 130, 1, 20, 0)]                  # islands [100, 119] and [130, 149]: gap 10
    got = _both(rows, [1000], pad=10)[0]
    assert [g[:4] for g in got] == [[b"Cluster_1", b"chr0", b"100", b"149"]]
    got = _both(rows, [1000], pad=9)[0]
    assert [g[:4] for g in got] == [[b"Cluster_1", b"chr0", b"100", b"119"], [b"Cluster_2", b"chr0", b"130", b"149"]]
    got = _both([(0, 100, 1, 20, 0), (0, 120, 1, 20, 0)], [1000], pad=0)[0]        # abutting islands are one island
    assert [g[:4] for g in got] == [[b"Cluster_1", b"chr0", b"100", b"139"]]
    got = _both([(0, 100, 1, 20, 0), (1, 110, 1, 20, 0)], [1000, 1000], pad=1000)[0]   # never across contigs
    assert len(got) == 2


def test_a_read_spanning_two_clusters_counts_only_in_the_left_one():
    rows = [(0, 100, 5, 20, 0), (0, 300, 5, 20, 1), (0, 110, 2, 200, 1)]
    got, cnt, _ = _both(rows, [1000], T=5, pad=10)
    assert [g[2:6] for g in got] == [[b"100", b"119", b"7", b"5"], [b"300", b"319", b"5", b"0"]]
    assert [g[14:21] for g in got][0] == [b"0", b"5", b"0", b"0", b"0", b"0", b"2"]
    assert cnt == [[b"Cluster_1", b"7"], [b"Cluster_2", b"5"]]


def test_a_read_from_far_left_still_counts():
    rows = [(0, 10, 1, 5000, 0), (0, 4000, 9, 21, 1)]
    got = _both(rows, [9000], T=5)[0]
    assert [g[2:6] for g in got] == [[b"4000", b"4020", b"10", b"1"]]


def test_strand_call_boundaries():
    def call(plus, minus):
        rows = [(0, 100, plus, 21, 0)] * (plus > 0) + [(0, 100, minus, 21, 1)] * (minus > 0)
        return _both(rows, [500])[0][0][6]
    assert [call(8, 2), call(7, 3), call(2, 8), call(3, 7), call(5, 5), call(10, 0), call(0, 10)] == [b"+", b".", b"-", b".", b".", b"+", b"-"]


def test_dicer_call_boundaries():
    def call(sizes):
        rows = [(0, 100 + i, d, ln, 0) for i, (ln, d) in enumerate(sizes.items()) if d]
        return _both(rows, [500])[0][0][7]
    assert call({21: 8, 30: 2}) == b"21"                 # exactly 80 % in 20..24
    assert call({21: 7, 30: 3}) == b"N"
    assert call({21: 79, 18: 21}) == b"N" and call({21: 80, 18: 20}) == b"21"
    assert call({21: 4, 24: 4, 30: 2}) == b"N"            # a tie between sizes
    assert call({21: 4, 24: 5, 30: 1}) == b"24" and call({20: 6, 22: 3, 23: 1}) == b"20"


def test_major_placement_ties():
    def major(rows):
        g = _both(rows, [500])[0][0]
        return g[9:13]
    assert major([(0, 100, 5, 21, 0), (0, 101, 6, 21, 0)]) == [b"101", b"+", b"21", b"6"]
    assert major([(0, 100, 3, 21, 0), (0, 100, 3, 21, 0), (0, 101, 6, 21, 0)]) == [b"100", b"+", b"21", b"6"]   # sums, not records
    assert major([(0, 101, 6, 21, 0), (0, 100, 6, 24, 1)]) == [b"100", b"-", b"24", b"6"]     # smallest pos
    assert major([(0, 100, 6, 21, 1), (0, 100, 6, 24, 0)]) == [b"100", b"+", b"24", b"6"]     # + before -
    assert major([(0, 100, 6, 24, 0), (0, 100, 6, 21, 0)]) == [b"100", b"+", b"21", b"6"]     # the shorter len
    got = _both([(0, 100, 6, 24, 0), (0, 100, 6, 21, 0), (0, 100, 1, 21, 0)], [500])[0][0]
    assert got[8] == b"2" and got[12] == b"7"


def test_rpm_ceiling():
    assert clusters.threshold(("rpm", Fraction(1, 2)), 4_000_000) == 2                 # exact multiple
    assert clusters.threshold(("rpm", Fraction(1, 2)), 4_000_001) == 3                 # just above
    assert clusters.threshold(("rpm", Fraction(1, 2)), 1) == 1 and clusters.threshold(("rpm", Fraction(1, 2)), 0) == 1
    assert clusters.threshold(("rpm", Fraction(3, 10)), 10 ** 7) == 3 and clusters.threshold(("rpm", Fraction(3, 10)), 10 ** 7 + 1) == 4
    assert clusters.threshold(("reads", 20), 10 ** 9) == 20


def test_major_rna_on_both_strands():
    seq = b"NNacgTNacGTuRtACGTACGT"
    rows = [(0, 3, 9, 8, 0), (1, 3, 9, 8, 1)]
    got = _both(rows, [len(seq), len(seq)], seqs=[seq, seq])[0]
    assert got[0][13] == b"ACGUNACG" and got[1][13] == b"CGUNACGU"           # "acgTNacG": upper case, T -> U / reverse complement
    assert clusters.placement_rna(b"acgtun", 1, 1, 6) == b"NAACGU" and clusters.placement_rna(b"xTt", 2, 0, 2) == b"UU"
    assert clusters.placement_rna(b"RYK", 1, 1, 3) == b"KYR"                        # IUPAC codes are copied unchanged
    assert clusters.placement_rna(b"ACGT", 0, 0, 3) == b"AC"                          # within the contig only


def test_no_island_and_no_record():
    alns = make_records([(0, 100, 1, 21, 0)])
    a = restate_plain(alns, ["c"], [500], ["a", "b"], 2, 75)
    assert a == (clusters.TSV_HEADER, b"name\ta\tb\n", clusters.GFF_HEADER) == restate_numpy(alns, ["c"], [500], ["a", "b"], 2, 75)
    assert restate_numpy(make_records([]), ["c"], [500], ["a"], 1, 75)[0] == clusters.TSV_HEADER


def test_gff3_reads_back_through_gffmask(tmp_path):
    rows = [(0, 100, 3, 21, 0), (0, 150, 3, 24, 1), (0, 2000, 3, 21, 0), (1, 50, 3, 300, 1)]
    _, _, files = _both(rows, [5000, 800])
    (tmp_path / "c.gff3").write_bytes(files[2])
    assert gffmask.keep_regions_include(str(tmp_path / "c.gff3"), minlen=0) == [("chr0", 99, 173), ("chr0", 1999, 2020), ("chr1", 49, 349)]
    assert gffmask.keep_regions_include(str(tmp_path / "c.gff3")) == [("chr0", 99, 173), ("chr1", 49, 349)]
    assert files[2].split(b"\n")[1] == b"chr0\tmir_prefer_amd\tsRNA_cluster\t100\t173\t.\t.\t.\tID=Cluster_1;DicerCall=N;Reads=6"


def test_cluster_dtype_has_the_c_struct_size(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the struct layout with")
    fields = ["tid", "major_strand", "major_len", "reserved", "start", "end", "reads", "plus_reads", "placements", "major_pos", "major_reads", "sizes"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirprefer.h"\nint main(void) {\n printf("%zu", sizeof(MirpCluster));\n' +
                   "".join(' printf(" %%zu", offsetof(MirpCluster, %s));\n' % f for f in fields) +
                   ' printf(" %zu %zu\\n", sizeof(MirpClusterOpts), offsetof(MirpClusterOpts, n_samples));\n return 0;\n}\n')
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got[0] == CLUSTER_DTYPE.itemsize == 128
    assert got[1:13] == [CLUSTER_DTYPE.fields[f][1] for f in fields]
    from mir_prefer_amd import capi
    import ctypes
    assert got[13:] == [ctypes.sizeof(capi.ClusterOpts), capi.ClusterOpts.n_samples.offset]


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.clusters"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    sam = tmp_path / "a.sam"
    sam.write_bytes(b"@SQ\tSN:c\tLN:100\n")
    s = str(sam)
    bad = [[], ["-m", "0", s], ["-m", "-1", s], ["-m", "1.5", s], ["-m", "x", s], ["-m", "", s], ["-m", "0rpm", s], ["-m", "0.0rpm", s],
           ["-m", "-1rpm", s], ["-m", "rpm", s], ["-m", "1/2rpm", s], ["-m", "0.5 rpm", s], ["-m", "0.5RPM", s], ["--pad", "-1", s],
           ["--pad", "1000001", s], ["--pad", "x", s], ["--device", "-1", s], ["-o", "", s], ["-g", "", s], ["-x", s]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "a.sam").write_bytes(b"@SQ\tSN:c\tLN:100\n")
    for ext in (".tsv", ".counts.tsv", ".gff3"):
        (tmp_path / ("a.sam.clusters" + ext)).write_bytes(b"stale\n")
    r = run_cli([str(tmp_path / "a.sam"), str(tmp_path / "nope.sam")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.sam" in r.stderr.decode()
    r = run_cli(["-g", str(tmp_path / "nope.fa"), str(tmp_path / "a.sam")], tmp_path)
    assert r.returncode == 255 and "nope.fa" in r.stderr.decode()


def test_helpers_of_the_command_line(capsys):
    assert [clusters.parse_min_coverage(x) for x in ("20", "1", "0", "0.5rpm", "1e-1rpm", ".5rpm", "3rpm", "2.rpm", "0rpm", "rpm", "1.5", "x")] == \
        [("reads", 20), ("reads", 1), None, ("rpm", Fraction(1, 2)), ("rpm", Fraction(1, 10)), ("rpm", Fraction(1, 2)), ("rpm", 3), ("rpm", 2), None,
         None, None, None]
    o, sams, spec, base = clusters.parse_args(["-m", "10", "--pad", "0", "a.sam", "b.sam"])
    assert (spec, o.pad, sams, base) == (("reads", 10), 0, ["a.sam", "b.sam"], "a.sam.clusters")
    assert clusters.parse_args(["a.sam"])[2:] == (("rpm", Fraction(1, 2)), "a.sam.clusters") and clusters.parse_args(["a.sam"])[0].pad == 75
    assert clusters.parse_args(["-o", "x/out.tsv", "a.sam"])[3] == "x/out" and clusters.parse_args(["-o", "out", "a.sam"])[3] == "out"
    assert clusters.output_paths("b") == ["b.tsv", "b.counts.tsv", "b.gff3"]
    with pytest.raises(SystemExit) as e:
        clusters.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--min-coverage", "--pad", "--output", "--genome", "--device"):
        assert opt in text
