"""GPU tests of the small-RNA clusters (mirp_cluster_scan, clusters_kernels.hip): all three files against the restatements of
tests/test_clusters_cpu.py over several -m / --pad settings on three SAM files with flagged, gapped and multi-mapped records; a hotspot cluster
of 2.1 M records whose sums pass 2^32; 10^6 small clusters; a contig of length 2^31 - 1 with reads at its last base; a threshold no position
reaches; -g and its refusals; the command line and the no-leftover rule; and the chain reads collapse -> align -> clusters -> pipeline with the
clusters' GFF3 as GFF_FILE_INCLUDE."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mir_prefer_amd import clusters
from tests.test_clusters_cpu import ROOT, clusters_numpy, make_records, random_records, random_seqs, restate_numpy, restate_plain

pytestmark = pytest.mark.gpu

SETTINGS = [("1", 75), ("20", 0), ("0.5rpm", 75), ("5000rpm", 30), ("60", 200), ("2.5e3rpm", 0)]


def write_sams(paths, names, lens, recs, extra=(), gapped_every=7):
    """recs (ALN_DTYPE; sample = the file) written with ids `s<f>_r<i>_x<depth>`; every gapped_every-th record of length >= 12 gets a gapped
    CIGAR with the same SEQ length; extra = (file, flag, tid, pos, depth, len) records that the ingest drops."""
    head = "@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(names, lens))
    bodies = [[] for _ in paths]
    for i, r in enumerate(recs.tolist()):
        tid, pos, depth, ln, strand, f = r
        cigar = "%dM" % ln if i % gapped_every or ln < 12 else "5M3N%dM2S" % (ln - 7)
        bodies[f].append("s%d_r%d_x%d\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t*\n" % (f, i, depth, 16 if strand else 0, names[tid], pos, cigar, "A" * ln))
    for j, (f, flag, tid, pos, depth, ln) in enumerate(extra):
        bodies[f].insert(1, "s%d_x%d_x%d\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t*\n" % (f, j, depth, flag, names[tid], pos, ln, "C" * ln))
    for p, b in zip(paths, bodies):
        open(p, "w").write(head + "".join(b))


def _files(ctx, names, lens, samples, T, pad, seqs=None):
    got, counts, stats = ctx.cluster_scan(T, pad, lens, len(samples))
    return clusters.format_files(names, got, counts, samples, seqs), got, counts, stats


@pytest.fixture(scope="module")
def sam_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_sams")
    names, lens = ["chrB", "short", "chrA", "chrC"], [3000, 150, 5000, 900]
    recs = random_records(np.random.RandomState(40), lens, 3, 900, 40)
    rng = np.random.RandomState(41)
    extra = [(int(rng.randint(0, 3)), int(flag), int(rng.randint(0, 4)), int(rng.randint(1, 140)), int(rng.randint(1, 50)), 21)
             for flag in (4, 256, 512, 1024, 4 | 16, 256 | 16) for _ in range(20)]
    paths = [str(d / ("s%d.sam" % i)) for i in range(3)]
    write_sams(paths, names, lens, recs, extra)
    return paths, names, lens, recs


def test_settings_match_the_restatements(gpu_ctx, sam_input):
    paths, names, lens, recs = sam_input
    n_names, n_lens, samples, alns, _, _ = gpu_ctx.ingest_sams(paths)
    assert n_names == names and n_lens.tolist() == lens and len(alns) == len(recs) and list(samples) == ["s0", "s1", "s2"]
    total = int(recs["depth"].sum())
    seqs = random_seqs(np.random.RandomState(2), lens)
    n = 0
    for m, pad in SETTINGS:
        T = clusters.threshold(clusters.parse_min_coverage(m), total)
        got, arr, counts, stats = _files(gpu_ctx, names, lens, samples, T, pad, seqs if pad == 30 else None)
        want = restate_numpy(recs, names, lens, samples, T, pad, seqs if pad == 30 else None)
        assert got == want, (m, pad)
        assert got == restate_plain(recs, names, lens, samples, T, pad, seqs if pad == 30 else None), (m, pad)
        assert stats == clusters_numpy(recs, lens, 3, T, pad)[2]
        n += len(arr)
    assert n > 50


def test_hotspot_cluster_past_2_32(gpu_ctx):
    rng = np.random.RandomState(5)
    n = 2_100_000
    recs = np.zeros(n, dtype=make_records([]).dtype)
    recs["tid"] = 1
    recs["pos"] = 5000 + rng.randint(0, 6, n)
    recs["len"] = rng.choice([19, 21, 22, 24, 25], n)
    recs["strand"] = rng.randint(0, 2, n)
    recs["sample"] = rng.randint(0, 3, n)
    recs["depth"] = rng.randint(1 << 30, 1 << 32, n, dtype=np.int64)
    side = make_records([(0, 100, 7, 21, 0, 1), (1, 200, 3, 21, 1, 2), (1, 7000, 1, 24, 0, 0)])
    recs = np.concatenate([recs, side])
    recs = recs[np.lexsort((recs["pos"], recs["tid"]))]
    gpu_ctx.load_genome([("a", np.full(10, 65, np.uint8)), ("b", np.full(10, 65, np.uint8))])
    gpu_ctx.load_alignments(recs)
    lens = [1000, 10000]
    for T, pad in ((1, 75), (1, 0), (1 << 33, 75), (int(recs["depth"].astype(np.int64).sum()) // 3, 10)):
        got, arr, counts, stats = _files(gpu_ctx, ["a", "b"], lens, ["x", "y", "z"], T, pad)
        assert got == restate_numpy(recs, ["a", "b"], lens, ["x", "y", "z"], T, pad), (T, pad)
        assert stats["assigned"] >= (n if T <= 1 << 33 else 0)
    got, arr, counts, _ = _files(gpu_ctx, ["a", "b"], lens, ["x", "y", "z"], 1, 75)
    assert int(arr["reads"].max()) > 1 << 52 and int(counts.max()) > 1 << 50 and int(arr["placements"].max()) == 60


def test_a_million_small_clusters(gpu_ctx):
    rng = np.random.RandomState(8)
    n = 1_000_000
    recs = np.zeros(n, dtype=make_records([]).dtype)
    recs["tid"] = np.arange(n) % 4
    recs["pos"] = 1 + (np.arange(n) // 4) * 200 + rng.randint(0, 10, n)
    recs["len"] = rng.choice([20, 21, 24], n)
    recs["strand"] = rng.randint(0, 2, n)
    recs["depth"] = rng.randint(1, 5, n)
    recs = recs[np.lexsort((recs["pos"], recs["tid"]))]
    gpu_ctx.load_genome([("c%d" % i, np.full(1, 65, np.uint8)) for i in range(4)])
    gpu_ctx.load_alignments(recs)
    lens = [60_000_000] * 4
    got, arr, _, stats = _files(gpu_ctx, ["c0", "c1", "c2", "c3"], lens, ["s"], 1, 75)
    assert len(arr) == n and stats["assigned"] == n
    assert got == restate_numpy(recs, ["c0", "c1", "c2", "c3"], lens, ["s"], 1, 75)
    got, arr, _, _ = _files(gpu_ctx, ["c0", "c1", "c2", "c3"], lens, ["s"], 1, 200)
    assert got == restate_numpy(recs, ["c0", "c1", "c2", "c3"], lens, ["s"], 1, 200) and len(arr) < 1000


def test_contig_near_2_31(gpu_ctx):
    top = (1 << 31) - 1
    rng = np.random.RandomState(9)
    rows = [(0, top, 5, 21, 1, 0), (0, top - 20, 3, 21, 0, 1), (0, top - 200, 2, 24, 0, 0), (1, top - 5, 4, 30, 1, 1), (1, top + 0, 1, 18, 0, 0), (1, top - 30, 2, 40, 0, 0)]
    rows += [(int(rng.randint(0, 2)), int(rng.randint(top - 3000, top + 1)), int(rng.randint(1, 9)), int(rng.choice([20, 21, 22, 40])),
              int(rng.randint(0, 2)), int(rng.randint(0, 2))) for _ in range(3000)]
    recs = make_records(rows)
    gpu_ctx.load_genome([("a", np.full(10, 65, np.uint8)), ("b", np.full(10, 65, np.uint8))])
    gpu_ctx.load_alignments(recs)
    lens = [top, top - 10]
    for T, pad in ((1, 75), (5, 0), (30, 75)):
        got, arr, _, _ = _files(gpu_ctx, ["a", "b"], lens, ["p", "q"], T, pad)
        assert got == restate_numpy(recs, ["a", "b"], lens, ["p", "q"], T, pad), (T, pad)
    got, arr, _, _ = _files(gpu_ctx, ["a", "b"], lens, ["p", "q"], 1, 75)
    assert int(arr["end"][arr["tid"] == 0].max()) == top and int(arr["end"][arr["tid"] == 1].max()) == top - 10


def test_threshold_no_position_reaches(gpu_ctx, sam_input):
    paths, names, lens, recs = sam_input
    gpu_ctx.ingest_sams(paths)
    got, arr, counts, stats = _files(gpu_ctx, names, lens, ["s0", "s1", "s2"], 1 << 40, 75)
    assert got == (clusters.TSV_HEADER, b"name\ts0\ts1\ts2\n", clusters.GFF_HEADER) and len(arr) == 0 and counts.shape == (0, 3)
    assert stats == {"records": len(recs), "total": int(recs["depth"].sum()), "islands": 0, "clusters": 0, "assigned": 0}


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
    seqs = random_seqs(np.random.RandomState(3), lens)
    _genome(tmp_path / "g.fa", names[::-1], seqs[::-1])
    r = _cli("mir_prefer_amd.clusters", ["-m", "3", "--pad", "40", "-o", str(tmp_path / "x.tsv"), "-g", str(tmp_path / "g.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_numpy(recs, names, lens, ["s0", "s1", "s2"], 3, 40, seqs)
    assert [(tmp_path / f).read_bytes() for f in ("x.tsv", "x.counts.tsv", "x.gff3")] == list(want) and want[0].count(b"\n") > 10
    _, _, st = clusters_numpy(recs, lens, 3, 3, 40)
    err = r.stderr.decode().splitlines()
    assert err == ["clusters: %d records, total %d reads, T 3, %d islands, %d clusters, %d records assigned, written to %s"
                   % (len(recs), st["total"], st["islands"], st["clusters"], st["assigned"], tmp_path / "x.tsv")]
    # defaults: 0.5rpm, --pad 75, <first sam>.clusters.*; the files in another order give other columns
    r = _cli("mir_prefer_amd.clusters", [paths[2], paths[0]], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    sub = recs[recs["sample"] != 1].copy()
    sub["sample"] = np.where(sub["sample"] == 2, 0, 1)
    T = clusters.threshold(("rpm", clusters.parse_min_coverage("0.5rpm")[1]), int(sub["depth"].sum()))
    want = restate_numpy(sub, names, lens, ["s2", "s0"], T, 75)
    assert [open(paths[2] + ".clusters" + e, "rb").read() for e in (".tsv", ".counts.tsv", ".gff3")] == list(want)
    # the same file twice: two columns of the same name
    r = _cli("mir_prefer_amd.clusters", ["-m", "1", "-o", str(tmp_path / "dup"), paths[1], paths[1]], tmp_path)
    assert r.returncode == 0 and (tmp_path / "dup.counts.tsv").read_bytes().split(b"\n")[0] == b"name\ts1\ts1"


def test_refusals_leave_no_output(tmp_path):
    sam = tmp_path / "a.sam"
    recs = make_records([(0, 10 + 5 * j, 3, 21, j % 2, 0) for j in range(10)])
    write_sams([str(sam)], ["c1", "c2"], [500, 300], recs)
    _genome(tmp_path / "short.fa", ["c1", "c2"], [b"A" * 500, b"A" * 299])
    _genome(tmp_path / "missing.fa", ["c1"], [b"A" * 500])
    (tmp_path / "bad.sam").write_bytes(sam.read_bytes() + b"r_x1\t0\tnope\t5\t255\t21M\t*\t0\t0\t" + b"A" * 21 + b"\t*\n")
    cases = [([str(tmp_path / "bad.sam")], "not in the @SQ header"),
             (["-g", str(tmp_path / "short.fa"), str(sam)], "contig c2 has 299 bases"),
             (["-g", str(tmp_path / "missing.fa"), str(sam)], "contig c2 of the SAM header is not in")]
    for args, why in cases:
        outs = clusters.output_paths(args[-1] + ".clusters")
        for p in outs:
            open(p, "wb").write(b"stale\n")
        r = _cli("mir_prefer_amd.clusters", args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr.decode())
        assert not any(os.path.exists(p) for p in outs)
    _genome(tmp_path / "ok.fa", ["c2", "c1"], [b"A" * 300, b"acgt" * 125])
    r = _cli("mir_prefer_amd.clusters", ["-m", "1", "-g", str(tmp_path / "ok.fa"), str(sam)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "a.sam.clusters.tsv").read_bytes() == restate_numpy(recs, ["c1", "c2"], [500, 300], ["s0"], 1, 75, [b"acgt" * 125, b"A" * 300])[0]


def test_chain_collapse_align_clusters_pipeline(tmp_path):
    from mir_prefer_amd import capi, synth
    from tests.test_align_gpu import _synth_read
    ds = synth.make_dataset([50000, 30000], 30, n_samples=2, seed=6, contig_names=["chr2", "chr1"])
    ds.write_fasta(str(tmp_path / "genome.fa"))
    raw = []
    for si, sname in enumerate(ds.sample_names):
        p = tmp_path / (sname + ".fa")
        with open(p, "wb") as f:
            for k, a in enumerate(ds.alns[ds.alns["sample"] == si]):
                s = _synth_read(ds, a)
                for j in range(int(a["depth"])):
                    f.write(b">x%d_%d\n%s\n" % (k, j, s.tobytes()))
        raw.append(str(p))
    (tmp_path / "names.txt").write_text("".join(s + "\n" for s in ds.sample_names))
    sams = [p + ".processed.sam" for p in raw]
    for module, args in (("mir_prefer_amd.reads", ["collapse", "names.txt"] + raw),
                         ("mir_prefer_amd.align", ["-f", "-r", "genome.fa"] + [p + ".processed" for p in raw]),
                         ("mir_prefer_amd.clusters", ["-m", "10", "-o", "cl"] + sams)):
        r = _cli(module, args, tmp_path)
        assert r.returncode == 0, (module, r.stderr.decode())
    names, lens, samples, alns = capi.ingest_sams(sams)
    want = restate_numpy(alns, names, lens.tolist(), list(samples), 10, 75)
    assert [(tmp_path / f).read_bytes() for f in ("cl.tsv", "cl.counts.tsv", "cl.gff3")] == list(want) and want[0].count(b"\n") > 3
    cfg = tmp_path / "config"
    cfg.write_text("FASTA_FILE = %s\nALIGNMENT_FILE = %s\nGFF_FILE_INCLUDE = %s\nPRECURSOR_LEN = 300\nREADS_DEPTH_CUTOFF = 20\nMAX_GAP = 100\n"
                   "MIN_MATURE_LEN = 18\nMAX_MATURE_LEN = 24\nALLOW_NO_STAR_EXPRESSION = Y\nALLOW_3NT_OVERHANG = N\nOUTFOLDER = %s\nNAME_PREFIX = chain\n"
                   % (tmp_path / "genome.fa", ", ".join(sams), tmp_path / "cl.gff3", tmp_path / "out"))
    r = _cli("mir_prefer_amd.cli", ["pipeline", str(cfg)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert b"\tmiRNA-precursor\t" in (tmp_path / "out" / "chain_miRNA.gff3").read_bytes()
