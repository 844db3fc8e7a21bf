"""GPU tests of the phased siRNA (PHAS) loci (mirp_phase_scan, phasing_kernels.hip): whole TSV files against the restatements of
tests/test_phasing_cpu.py over L = 21, 22, 24 and several m, alpha, K, D on SAM input with planted loci, mixed-length noise, several files,
multi-mapped, flagged and gapped records and a contig shorter than one window; a saturated region; coordinates near 2^31; 5 M records; the
refusals; the command line; and the chain reads collapse -> align -> phasing -g -> targets -b."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd import phasing
from tests.test_phasing_cpu import HEADER, ROOT, make_records, plant_locus, random_records, restate_numpy, restate_plain, windows_numpy

pytestmark = pytest.mark.gpu

GRID = [(10, Fraction(1, 1000), 3, 1), (4, Fraction(1, 100), 2, 2), (20, Fraction(1, 10 ** 5), 5, 1), (7, Fraction(1), 1, 3)]


def _tsv(ctx, names, lens, L, m, alpha, K, D):
    hg = phasing.Hypergeom(m, L)
    wins, stats = ctx.phase_scan(L, m, hg.kmin(alpha), min_phased=K, min_depth=D)
    return phasing.format_tsv(names, phasing.merge_loci(phasing.window_tuples(wins), lens, m, L, hg)), wins, stats


def write_sams(paths, names, lens, recs, extra=(), gapped_every=7):
    """recs (ALN_DTYPE) spread round-robin over the files, ids `s<f>_r<i>_x<depth>`; every gapped_every-th record of length >= 12 gets a gapped
    CIGAR with the same SEQ length; extra = (file, flag, tid, pos, depth, len) records written as well (flagged ones, which the ingest drops)."""
    head = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(names, lens))
    bodies = [[] for _ in paths]
    for i, r in enumerate(recs.tolist()):
        tid, pos, depth, ln, strand = r[0], r[1], r[2], r[3], r[4]
        cigar = "%dM" % ln if i % gapped_every or ln < 12 else "5M3N%dM2S" % (ln - 7)
        bodies[i % len(paths)].append("s%d_r%d_x%d\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t*\n" % (i % len(paths), i, depth, 16 if strand else 0,
                                                                                           names[tid], pos, cigar, "A" * ln))
    for j, (f, flag, tid, pos, depth, ln) in enumerate(extra):
        bodies[f].append("x%d_r%d_x%d\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t*\n" % (f, j, depth, flag, names[tid], pos, ln, "C" * ln))
    for p, b in zip(paths, bodies):
        open(p, "w").write(head + "".join(b))


def mixed_records(seed, lens):
    """Planted loci of lengths 21, 22 and 24 on one or both strands, noise of mixed lengths, multi-mapped reads."""
    parts = [random_records(np.random.RandomState(seed + i), lens, L, 700, 6) for i, L in enumerate((21, 22, 24))]
    return make_records([tuple(r[:5]) for p in parts for r in p.tolist()])


@pytest.fixture(scope="module")
def sam_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("phasing_sams")
    names, lens = ["chrB", "short", "chrA", "chrC"], [3000, 150, 5000, 900]
    recs = mixed_records(40, lens)
    rng = np.random.RandomState(41)
    extra = [(int(rng.randint(0, 3)), int(flag), int(rng.randint(0, 4)), int(rng.randint(1, 140)), int(rng.randint(1, 50)), int(L))
             for flag in (4, 256, 1024, 4 | 16, 256 | 16) for L in (21, 22, 24) for _ in range(20)]
    paths = [str(d / ("s%d.sam" % i)) for i in range(3)]
    write_sams(paths, names, lens, recs, extra)
    return paths, names, lens, recs


def test_grid_matches_the_restatement(gpu_ctx, sam_input):
    paths, names, lens, recs = sam_input
    n_names, n_lens, _, alns, _, _ = gpu_ctx.ingest_sams(paths)
    assert n_names == names and n_lens.tolist() == lens and len(alns) == len(recs)
    loci = 0
    for L in (21, 22, 24):
        for m, alpha, K, D in GRID:
            got, wins, stats = _tsv(gpu_ctx, names, lens, L, m, alpha, K, D)
            want = restate_numpy(recs, names, lens, L, m, alpha, K, D)
            assert got == want, (L, m, alpha, K, D)
            assert stats["records"] == int((recs["len"] == L).sum())
            if (m, K, D) == (10, 3, 1):
                assert restate_plain(recs, names, lens, L, m, alpha, K, D) == want
            loci += want.count(b"\n") - 1
    assert loci > 30


def test_saturated_region(gpu_ctx):
    """Every coordinate of a 10 kb region on both strands: n = S for the inner anchors."""
    rng = np.random.RandomState(5)
    rows = [(0, p, int(rng.randint(1, 9)), 21, s) for p in range(1000, 11000) for s in (0, 1)]
    rows += [(0, p, 2, 24, s) for p in range(3000, 3400) for s in (0, 1)]
    recs = make_records(rows)
    gpu_ctx.load_genome([("c0", np.full(12000, 65, np.uint8))])
    gpu_ctx.load_alignments(recs)
    for L, m, alpha, K in ((21, 10, Fraction(1, 1000), 3), (21, 20, Fraction(1), 1), (24, 4, Fraction(1), 1)):
        got, wins, _ = _tsv(gpu_ctx, ["c0"], [12000], L, m, alpha, K, 1)
        assert got == restate_numpy(recs, ["c0"], [12000], L, m, alpha, K, 1), (L, m)
        if K == 1 and L == 21:
            assert int(wins["n"].max()) == 2 * m * L and int(wins["k"].max()) == 2 * m


def test_coordinates_near_2_31(gpu_ctx):
    rng = np.random.RandomState(9)
    top = (1 << 31) - 1
    rows = []
    plant_locus(rows, rng, 0, top - 187, 21, 10, strands=(1,))          # the last minus read: pos 2^31 - 1, c = 2^31 + 1
    plant_locus(rows, rng, 0, top - 194, 21, 10, strands=(0,))
    plant_locus(rows, rng, 1, top - 400, 21, 8)
    rows += [(int(rng.randint(0, 2)), int(rng.randint(top - 3000, top + 1)), int(rng.randint(1, 9)), int(rng.choice([20, 21, 22])),
              int(rng.randint(0, 2))) for _ in range(3000)]
    recs = make_records(rows)
    assert int(recs["pos"].max()) == top
    gpu_ctx.load_genome([("a", np.full(10, 65, np.uint8)), ("b", np.full(10, 65, np.uint8))])
    gpu_ctx.load_alignments(recs)
    lens = [(1 << 31) + 50, (1 << 31) + 50]
    for m, alpha, K, D in GRID:
        got, wins, _ = _tsv(gpu_ctx, ["a", "b"], lens, 21, m, alpha, K, D)
        assert phasing.window_tuples(wins) == windows_numpy(recs, 21, m, alpha, K, D)
        assert got == restate_numpy(recs, ["a", "b"], lens, 21, m, alpha, K, D)
        if alpha == 1:
            assert int(wins["start"].max()) == top + 2


def test_5m_records(gpu_ctx):
    rng = np.random.RandomState(77)
    n, n_contigs, clen = 5_000_000, 8, 12_000_000
    recs = np.zeros(n, dtype=make_records([]).dtype)
    recs["tid"] = rng.randint(0, n_contigs, n)
    recs["pos"] = rng.randint(1, clen - 30, n)
    recs["len"] = rng.choice([18, 20, 21, 22, 23, 24, 26], n, p=[0.08, 0.1, 0.4, 0.12, 0.1, 0.15, 0.05])
    recs["strand"] = rng.randint(0, 2, n)
    recs["depth"] = np.minimum(rng.geometric(0.3, n), 10 ** 6)
    rows = []
    for _ in range(300):
        plant_locus(rows, rng, int(rng.randint(0, n_contigs)), int(rng.randint(10, clen - 400)), 21, 10, depth=(5, 60))
    recs = np.concatenate([recs, make_records(rows)])
    recs = recs[np.lexsort((recs["pos"], recs["tid"]))]
    gpu_ctx.load_genome([("c%d" % i, np.full(1, 65, np.uint8)) for i in range(n_contigs)])
    gpu_ctx.load_alignments(recs)
    hg = phasing.Hypergeom(10, 21)
    wins, stats = gpu_ctx.phase_scan(21, 10, hg.kmin(Fraction(1, 1000)))
    want = windows_numpy(recs)
    assert phasing.window_tuples(wins) == want and len(want) > 1000
    assert stats["records"] == int((recs["len"] == 21).sum()) and stats["anchors"] > 10 ** 6


# ---------------------------------------------------------------------------------------------------- the command line
def _cli(module, args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _genome(path, names, seqs):
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">%s some description\n" % n.encode())
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + b"\n")


def test_cli(sam_input, tmp_path):
    paths, names, lens, recs = sam_input
    rng = np.random.RandomState(3)
    seqs = [bytes(np.frombuffer(b"ACGTacgtN", np.uint8)[rng.randint(0, 9, ln)]) for ln in lens]
    _genome(tmp_path / "g.fa", names[::-1], seqs[::-1])
    out = tmp_path / "x.phas.tsv"
    r = _cli("mir_prefer_amd.phasing", ["-l", "22", "-c", "8", "-p", "1e-4", "-k", "4", "-d", "2", "-o", str(out), "-g", str(tmp_path / "g.fa")] + paths,
             tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_numpy(recs, names, lens, 22, 8, Fraction(1, 10000), 4, 2)
    assert out.read_bytes() == want and want.count(b"\n") > 2
    fa = []
    for ln in want.split(b"\n")[1:-1]:
        f = ln.split(b"\t")
        t, a, b = names.index(f[0].decode()), int(f[1]), int(f[2])
        fa.append(b">%s:%d-%d\n%s\n" % (f[0], a, b, seqs[t][a - 1:b]))
    assert (tmp_path / "x.phas.fa").read_bytes() == b"".join(fa)
    err = r.stderr.decode().splitlines()
    assert len(err) == 1 and err[0].startswith("phasing: %d records of length 22, " % int((recs["len"] == 22).sum()))
    assert err[0].endswith(" %d loci written to %s" % (want.count(b"\n") - 1, out))
    # defaults: <first sam>.phas.tsv, no FASTA
    r = _cli("mir_prefer_amd.phasing", paths[1:], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert open(paths[1] + ".phas.tsv", "rb").read() == restate_numpy(recs[np.arange(len(recs)) % 3 != 0], names, lens)
    assert not os.path.exists(paths[1] + ".phas.fa")
    os.remove(paths[1] + ".phas.tsv")
    # no record of length L: the header only
    r = _cli("mir_prefer_amd.phasing", ["-l", "30", "-o", str(tmp_path / "e.tsv")] + paths, tmp_path)
    assert r.returncode == 0 and (tmp_path / "e.tsv").read_bytes() == HEADER


def test_refusals_leave_no_output(tmp_path):
    sam = tmp_path / "a.sam"
    write_sams([str(sam)], ["c1", "c2"], [500, 300], make_records([(0, 10 + 21 * j, 3, 21, 0) for j in range(10)]))
    _genome(tmp_path / "short.fa", ["c1", "c2"], [b"A" * 500, b"A" * 299])
    _genome(tmp_path / "missing.fa", ["c1"], [b"A" * 500])
    (tmp_path / "bad.sam").write_bytes(sam.read_bytes() + b"r_x1\t0\tnope\t5\t255\t21M\t*\t0\t0\t" + b"A" * 21 + b"\t*\n")
    cases = [([str(tmp_path / "bad.sam")], "not in the @SQ header"),
             (["-g", str(tmp_path / "short.fa"), str(sam)], "contig c2 has 299 bases"),
             (["-g", str(tmp_path / "missing.fa"), str(sam)], "contig c2 of the SAM header is not in")]
    for args, why in cases:
        outs = [args[-1] + ".phas.tsv", args[-1] + ".phas.fa"]
        for p in outs:
            open(p, "wb").write(b"stale\n")
        r = _cli("mir_prefer_amd.phasing", args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr.decode())
        assert not os.path.exists(outs[0])
        assert os.path.exists(outs[1]) != ("-g" in args)
        os.remove(outs[1]) if os.path.exists(outs[1]) else None
    r = _cli("mir_prefer_amd.phasing", [str(sam)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "a.sam.phas.tsv").read_bytes().split(b"\n")[1].split(b"\t")[:4] == [b"c1", b"10", b"366", b"8"]


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def test_chain_collapse_align_phasing_targets(tmp_path):
    """A PHAS locus whose register starts at x0, with a site complementary to a planted miRNA cut (between miRNA positions 10 and 11) at the
    locus's third register boundary: reads collapse -> align -> phasing -g -> targets -b finds the locus and puts the cut on its register."""
    rng = np.random.RandomState(12)
    L, x0 = 21, 10001
    genome = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, 30000)].tobytes())
    mirna = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, 21)].tobytes())
    s1 = x0 + 2 * L - 11                                               # site start (1-based): the cut falls on x0 + 2L
    genome[s1 - 1:s1 - 1 + 21] = _revcomp(mirna)
    other = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, 5000)].tobytes())
    _genome(tmp_path / "genome.fa", ["chr1", "chr2"], [bytes(genome), other])
    reads = []
    for j in range(10):
        c = x0 + j * L
        reads += [bytes(genome[c - 1:c - 1 + L])] * 3 + [_revcomp(bytes(genome[c - 3:c - 3 + L]))] * 2
    (tmp_path / "reads.fa").write_bytes(b"".join(b">q%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    (tmp_path / "names.txt").write_text("S1\n")
    (tmp_path / "mir.fa").write_bytes(b">mir-t\n" + mirna.replace(b"T", b"U") + b"\n")
    for module, args in (("mir_prefer_amd.reads", ["collapse", "names.txt", "reads.fa"]),
                         ("mir_prefer_amd.align", ["-f", "-r", "genome.fa", "reads.fa.processed"]),
                         ("mir_prefer_amd.phasing", ["-g", "genome.fa", "reads.fa.processed.sam"]),
                         ("mir_prefer_amd.targets", ["-b", "-s", "0", "mir.fa", "reads.fa.processed.sam.phas.fa"])):
        r = _cli(module, args, tmp_path)
        assert r.returncode == 0, (module, r.stderr.decode())
    loci = [ln.split(b"\t") for ln in (tmp_path / "reads.fa.processed.sam.phas.tsv").read_bytes().split(b"\n")[1:-1]]
    assert len(loci) == 1 and loci[0][:2] == [b"chr1", str(x0).encode()] and loci[0][5:7] == [b"20", b"20"]
    start, end = int(loci[0][1]), int(loci[0][2])
    sites = [ln.split(b"\t") for ln in (tmp_path / "mir.fa.targets.tsv").read_bytes().split(b"\n")[1:-1]]
    assert [s[:6] for s in sites] == [[b"mir-t", b"chr1:%d-%d" % (start, end), str(s1 - start + 1).encode(), str(s1 - start + 21).encode(), b"+", b"0.0"]]
    cut = start - 1 + int(sites[0][2]) + 11                           # first locus base 3' of the cut, genome coordinate
    assert (cut - start) % L == 0 and start < cut <= end
