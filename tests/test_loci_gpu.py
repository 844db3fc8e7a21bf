"""GPU tests of the reads-on-given-loci verb (mirp_locus_scan, loci_kernels.hip), by exact equality with the restatements of
tests/loci_restatement.py: about 1,000 overlapping, nested and repeated loci on three SAM files, stranded and not, through the binding and the
command line; candidate ranges of C - 1, C, C + 1 and 2 C + 1 records and placements (C = capi.LOCI_CHUNK); a 65,535-nt record that fixes the
search fringe, and a locus at position 1 of the contig after it; sums past 2^32; waves that serve three and more jobs; a contig of 2^31 - 1
bases, 255 samples, no records, no locus with reads, no locus, a sample index out of range; `clusters` reproduced on its own GFF3; and the chain
reads collapse -> align -> phasing -> loci --format phas, with the refusals that leave no output."""
import os

import numpy as np
import pytest

from mir_prefer_amd import capi, loci
from tests import loci_restatement as R
from tests.test_clusters_cpu import make_records, random_records, random_seqs
from tests.test_clusters_gpu import _cli, _genome, write_sams
from tests.test_loci_cpu import L, random_loci

pytestmark = pytest.mark.gpu

C = capi.LOCI_CHUNK
COUNT = 5                                            # the count kernel's family of mirp_last_jobs_per_slot


def load(ctx, recs, n_contigs):
    ctx.load_genome([("c%d" % i, np.full(4, 65, np.uint8)) for i in range(n_contigs)])
    ctx.load_alignments(recs)


def jobs_of(recs, arr):
    """The (locus, chunk of C records) jobs of a call: ceil(candidate range / C) summed over the loci."""
    key = (recs["tid"].astype(np.int64) << 32) + recs["pos"]
    M = int(recs["len"].max()) if len(recs) else 0
    t = arr["tid"].astype(np.int64) << 32
    n = np.searchsorted(key, t + arr["end"], "right") - np.searchsorted(key, t + arr["start"] - M + 1, "left")
    return int(((n + C - 1) // C).sum())


def check(ctx, recs, arr, lens, n_samples=1, stranded=False):
    """One call against the numpy statement: rows, counts and stats, exactly."""
    got, counts, stats = ctx.locus_scan(arr, lens, n_samples, stranded)
    want, wcounts, wstats = R.scan_numpy(recs, arr, lens, n_samples, stranded)
    assert got.tobytes() == want.tobytes() and (counts == wcounts).all() and counts.shape == wcounts.shape
    assert stats == dict(wstats, jobs=jobs_of(recs, arr))
    return got, counts, stats


# ---------------------------------------------------------------------------------------------------- 1: the settings sweep
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    d = tmp_path_factory.mktemp("loci_sams")
    names, lens = ["chrB", "short", "chrA"], [30000, 1500, 50000]           # @SQ order is not the lexicographic one
    recs = random_records(np.random.RandomState(70), lens, 3, 12000, 260)
    paths = [str(d / ("s%d.sam" % i)) for i in range(3)]
    write_sams(paths, names, lens, recs)
    rng = np.random.RandomState(71)
    kept = random_loci(rng, names, lens, 1000)
    seqs = dict(zip(names, random_seqs(rng, lens)))
    gff = d / "loci.gff3"
    gff.write_text("##gff-version 3\n" + "".join("%s\tsrc\t%s\t%d\t%d\t.\t%s\t.\tID=%s;Note=x\n" % (c, t, a, b, s, n) for n, t, c, a, b, s in kept)
                   + "nowhere\tsrc\tt0\t1\t5\t.\t+\t.\tID=dropped\n")
    _genome(d / "g.fa", names[::-1], [seqs[n] for n in names[::-1]])
    return d, paths, names, lens, recs, kept, seqs


def test_settings_match_the_restatements(gpu_ctx, sweep):
    d, paths, names, lens, recs, kept, seqs = sweep
    n_names, n_lens, samples, alns, _, _ = gpu_ctx.ingest_sams(paths)
    assert n_names == names and n_lens.tolist() == lens and len(alns) == len(recs) > 18000 and list(samples) == ["s0", "s1", "s2"]
    arr = loci.locus_array(kept, names)
    for stranded in (False, True):
        got, counts, stats = check(gpu_ctx, recs, arr, lens, 3, stranded)
        assert stats["pairs"] > 10 * len(recs)
        # the plain double loop on every 25th locus
        sub = kept[::25]
        files = loci.format_files(kept, got, counts, list(samples), seqs)
        want = R.files_plain(recs, sub, names, lens, list(samples), stranded, seqs)
        assert [ln for ln in files[0].split(b"\n")[1::25]][:len(sub)] == want[0].split(b"\n")[1:-1]
        assert [ln for ln in files[1].split(b"\n")[1::25]][:len(sub)] == want[1].split(b"\n")[1:-1]
    assert int((got["placements"] == 0).sum()) > 0 and int(got["placements"].max()) > 1000


def test_cli_whole_files(sweep, tmp_path):
    d, paths, names, lens, recs, kept, seqs = sweep
    arr = R.locus_array(kept, names)
    for extra, stranded, with_g in (([], False, False), (["-s", "-g", str(d / "g.fa")], True, True)):
        r = _cli("mir_prefer_amd.loci", extra + ["-o", str(tmp_path / "x.tsv"), str(d / "loci.gff3")] + paths, tmp_path)
        assert r.returncode == 0, r.stderr.decode()
        rows, counts, st = R.scan_numpy(recs, arr, lens, 3, stranded)
        want = loci.format_files(kept, rows, counts, ["s0", "s1", "s2"], seqs if with_g else None)
        assert [(tmp_path / f).read_bytes() for f in ("x.tsv", "x.counts.tsv")] == list(want)
        assert r.stderr.decode().splitlines() == [
            "loci: %d records, %d loci kept / 1 dropped (sequence not in the SAM header), %d (record, locus) pairs counted, %d loci with reads, "
            "written to %s" % (len(recs), len(kept), st["pairs"], int((rows["placements"] > 0).sum()), tmp_path / "x.tsv")]
    # -t, the default base, BED with the same intervals, and the whole file against the plain double loop
    few = [l for l in kept if l[1] == "t1"][:30]
    r = _cli("mir_prefer_amd.loci", ["-t", "t1", str(d / "loci.gff3"), paths[1], paths[0]], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    sub = recs[recs["sample"] != 2].copy()
    sub["sample"] = 1 - sub["sample"]
    t1 = [l for l in kept if l[1] == "t1"]
    rows, counts, _ = R.scan_numpy(sub, R.locus_array(t1, names), lens, 2)
    assert [open(paths[1] + ".loci" + e, "rb").read() for e in (".tsv", ".counts.tsv")] == list(loci.format_files(t1, rows, counts, ["s1", "s0"]))
    bed = tmp_path / "few.bed"
    bed.write_text("track name=few\n" + "".join("%s\t%d\t%d\t%s\t0\t%s\n" % (c, a - 1, b, n, s) for n, _, c, a, b, s in few))
    r = _cli("mir_prefer_amd.loci", ["-s", "-g", str(d / "g.fa"), "-o", str(tmp_path / "few"), str(bed)] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    few_bed = [(n, ".", c, a, b, s) for n, _, c, a, b, s in few]
    assert [(tmp_path / f).read_bytes() for f in ("few.tsv", "few.counts.tsv")] == \
        list(R.files_plain(recs, few_bed, names, lens, ["s0", "s1", "s2"], True, seqs))


# ---------------------------------------------------------------------------------------------------- 2: job boundaries
def test_ranges_around_a_multiple_of_the_chunk(gpu_ctx):
    """Contig k holds exactly m records with pos in [start - M + 1, end] of its locus, all 21 nt (M = 21): on contigs 0..3 at m distinct
    positions, so that the placement table has m rows there too; on contigs 4..7 every position twice, so that 2 m' records make m' placements."""
    sizes = [C - 1, C, C + 1, 2 * C + 1]
    rows, loc, jobs = [], [], 0
    for k, m in enumerate(sizes + sizes):
        twice = k >= 4
        n_pos = m if not twice else (m + 1) // 2
        start = 100000
        pos = [start - 20 + 3 * i for i in range(n_pos)]                      # the first one ends on the locus's first base
        end = pos[-1]                                                          # the last one starts on its last base
        for i, p in enumerate(pos):
            rows.append((k, p, 1 + i % 7, 21, i % 2, i % 3))
            if twice and (2 * i + 1 < m or m % 2 == 0):
                rows.append((k, p, 2, 21, i % 2, (i + 1) % 3))
        rows += [(k, start - 21, 9, 21, 0, 0), (k, start - 500, 9, 21, 1, 1), (k, end + 1, 9, 21, 0, 2), (k, end + 300, 9, 21, 1, 0)]
        loc += [(k, ".", start, end), (k, "+", start + 1, end - 1)]
        jobs += -(-m // C)
    recs = make_records(rows)
    lens = [400000] * 8
    arr = L(*loc)
    for k, m in enumerate(sizes + sizes):                                      # the construction: the candidate range of locus 2 k holds m records
        key = (recs["tid"].astype(np.int64) << 32) + recs["pos"]
        a, b = np.searchsorted(key, (k << 32) + 100000 - 20, "left"), np.searchsorted(key, (k << 32) + int(arr["end"][2 * k]), "right")
        assert b - a == m, (k, m, b - a)
    load(gpu_ctx, recs, 8)
    for stranded in (False, True):
        got, _, stats = check(gpu_ctx, recs, arr, lens, 3, stranded)
        assert jobs_of(recs, arr[0::2]) == jobs and stats["max_len"] == 21
        assert got["placements"][0:8:2].tolist() == sizes and got["placements"][8:16:2].tolist() == [(m + 1) // 2 for m in sizes]
    # every locus alone gives the same row
    for q in range(len(arr)):
        alone = gpu_ctx.locus_scan(arr[q:q + 1], lens, 3, True)[0]
        assert alone.tobytes() == got[q:q + 1].tobytes(), q


# ---------------------------------------------------------------------------------------------------- 3: the fringe
def test_one_long_record_sets_the_fringe(gpu_ctx):
    rng = np.random.RandomState(72)
    lens = [200000, 5000]
    rows = [(0, 1000, 5, 65535, 1, 0)]                                         # covers [1000, 66534]
    rows += [(0, int(p), int(rng.randint(1, 9)), 21, int(rng.randint(0, 2)), 0) for p in rng.randint(1, 199900, 3000)]
    rows += [(0, 199990, 3, 21, 0, 0), (0, 200000, 4, 21, 1, 0), (0, 200001, 6, 21, 1, 0)]      # at the end of the first contig
    rows += [(1, 1, 7, 21, 0, 0), (1, 0, 2, 21, 1, 0), (1, 30, 1, 21, 0, 0)]
    recs = make_records(rows)
    quiet = 66534 + 40                                                         # make [66534, quiet] free of short reads, so that only the long one is there
    recs = recs[~((recs["tid"] == 0) & (recs["len"] == 21) & (recs["pos"] > 66534 - 21) & (recs["pos"] <= quiet))]
    arr = L((0, ".", 66534, quiet), (0, ".", 66535, quiet), (1, ".", 1, 1), (1, ".", 1, 25), (0, ".", 200000, 200000), (0, "-", 1, 200000),
            (0, ".", 999, 999), (0, ".", 1000, 1000))
    load(gpu_ctx, recs, 2)
    for stranded in (False, True):
        got, _, stats = check(gpu_ctx, recs, arr, lens, 1, stranded)
        assert stats["max_len"] == 65535
        assert got["reads"][:2].tolist() == [5, 0] and got["placements"][:2].tolist() == [1, 0]
        assert (int(got["major_pos"][0]), int(got["major_len"][0]), int(got["major_strand"][0])) == (1000, 65535, 1)
        # position 1 of the second contig sees its own two records and nothing of the first contig's end
        assert got["reads"][2:5].tolist() == [9, 9, 7]
    assert got["placements"][2:5].tolist() == [2, 2, 2]


# ---------------------------------------------------------------------------------------------------- 4: sums past 2^32
def test_a_full_wave_of_depth_2_32_minus_1(gpu_ctx):
    top = (1 << 32) - 1
    rows = [(0, 500, top, 21, 0, 0)] * 40 + [(0, 500, top, 24, 1, 0)] * 24 + [(0, 900, 3, 21, 0, 0)]
    recs = make_records(rows)
    recs["depth"][:64] = top                                                   # make_records goes through int64; keep the full 32 bits
    arr = L((0, ".", 400, 600), (0, ".", 1, 1000), (0, "+", 520, 520))
    load(gpu_ctx, recs, 1)
    got, counts, _ = check(gpu_ctx, recs, arr, [1000], 1)
    assert int(got["reads"][0]) == 64 * top > 1 << 37 and int(counts[0, 0]) == 64 * top and int(got["major_reads"][0]) == 40 * top
    assert got["sizes"][0].tolist() == [0, 0, 40 * top, 0, 0, 24 * top, 0] and int(got["reads"][1]) == 64 * top + 3
    assert int(check(gpu_ctx, recs, arr, [1000], 1, True)[0]["reads"][2]) == 40 * top


# ---------------------------------------------------------------------------------------------------- 5: slot reuse
def test_waves_serve_three_jobs_and_more(gpu_ctx):
    rng = np.random.RandomState(73)
    heavy_n, small_n = 6, 12300                                               # 12,318 jobs: three and more for every one of 4,096 waves
    rows = []
    for h in range(heavy_n):                                                   # 2 C + 500 records under every heavy locus: three jobs each
        for i in range(2 * C + 500):
            rows.append((0, 10000 * (h + 1) + int(rng.randint(0, 3000)), int(rng.randint(1, 99)), int(rng.choice([20, 21, 22, 24, 30])),
                         int(rng.randint(0, 2)), int(rng.randint(0, 2))))
    small_pos = 1 + 60 * np.arange(small_n)
    small = np.zeros(small_n, make_records([]).dtype)
    small["tid"], small["pos"], small["depth"], small["len"] = 1, small_pos, rng.randint(1, 50, small_n), rng.choice([21, 24], small_n)
    small["strand"], small["sample"] = rng.randint(0, 2, small_n), rng.randint(0, 2, small_n)
    recs = np.concatenate([make_records(rows), small])
    arr = np.zeros(heavy_n + small_n, capi.LOCUS_DTYPE)                        # the heavy loci first
    arr["strand"] = 2
    arr["tid"][heavy_n:] = 1
    arr["start"][:heavy_n], arr["end"][:heavy_n] = 10000 * (1 + np.arange(heavy_n)), 10000 * (1 + np.arange(heavy_n)) + 3030
    arr["start"][heavy_n:], arr["end"][heavy_n:] = small_pos + 5, small_pos + 30
    lens = [100000, 60 * small_n + 100]
    load(gpu_ctx, recs, 2)
    got, _, stats = check(gpu_ctx, recs, arr, lens, 2)
    launches, per_slot = gpu_ctx.last_jobs_per_slot(COUNT)
    assert stats["jobs"] == 3 * heavy_n + small_n and launches == 1 and per_slot >= 3, (stats, launches, per_slot)
    assert int(got["placements"][heavy_n:].min()) == 1 == int(got["placements"][heavy_n:].max())
    # the row of a locus does not depend on the jobs its wave served before: every locus alone, in a call of its own
    for q in range(len(arr)):
        alone = gpu_ctx.locus_scan(arr[q:q + 1], lens, 2)[0]
        assert alone.tobytes() == got[q:q + 1].tobytes(), q
    assert gpu_ctx.last_jobs_per_slot(COUNT) == (1, 1)


# ---------------------------------------------------------------------------------------------------- 6: edges
def test_contig_of_2_31_minus_1(gpu_ctx):
    top = (1 << 31) - 1
    rows = [(0, top, 5, 21, 1, 0), (0, top - 20, 3, 21, 0, 1), (0, top - 21, 2, 21, 0, 0), (1, top - 15, 4, 30, 1, 1), (1, 5, 1, 18, 0, 0)]
    recs = make_records(rows)
    arr = L((0, ".", top, top), (0, ".", top - 1, top - 1), (0, ".", 1, top), (1, "-", top - 10, top - 10), (1, ".", top - 16, top - 16), (1, ".", 1, 1))
    load(gpu_ctx, recs, 2)
    got, _, _ = check(gpu_ctx, recs, arr, [top, top - 10], 2)
    assert got["reads"].tolist() == [8, 5, 10, 4, 0, 0]
    check(gpu_ctx, recs, arr, [top, top - 10], 2, True)


def test_255_samples(gpu_ctx):
    rng = np.random.RandomState(74)
    n = 3000
    rows = [(0, int(rng.randint(1, 900)), int(rng.randint(1, 9)), 21, int(rng.randint(0, 2)), i % 255) for i in range(n)]
    recs = make_records(rows)
    arr = L((0, ".", 1, 1000), (0, ".", 400, 420), (0, "+", 100, 900), (0, ".", 400, 420))
    load(gpu_ctx, recs, 1)
    _, counts, _ = check(gpu_ctx, recs, arr, [1000], 255, True)
    assert counts.shape == (4, 255) and int((counts[0] > 0).sum()) == 255
    # a counted record whose sample index is not below n_samples is refused; one that no locus counts is not looked at
    with pytest.raises(capi.MirpError) as e:
        gpu_ctx.locus_scan(arr, [1000], 254)
    assert "sample index" in str(e.value)
    far = make_records([(0, 10, 1, 21, 0, 0), (0, 500, 1, 21, 0, 7)])
    load(gpu_ctx, far, 1)
    assert gpu_ctx.locus_scan(L((0, ".", 1, 100)), [1000], 1)[0]["reads"].tolist() == [1]


def test_nothing_to_count(gpu_ctx):
    recs = make_records([(0, 100, 3, 21, 0, 0), (1, 100, 3, 21, 0, 0)])
    arr = L((0, ".", 1, 79), (0, ".", 121, 500), (0, "-", 90, 130), (1, ".", 1, 99))
    load(gpu_ctx, recs, 2)
    got, counts, stats = check(gpu_ctx, recs, arr, [500, 99], 1, True)           # no locus with reads (the second contig's record lies past LN)
    assert not got["reads"].any() and not got["placements"].any() and stats["pairs"] == 0
    assert got["start"].tolist() == [1, 121, 90, 1] and got["major_pos"].tolist() == [0, 0, 0, 0]
    none, ncounts, nstats = gpu_ctx.locus_scan(arr[:0], [500, 99], 3)           # n_loci = 0
    assert len(none) == 0 and ncounts.shape == (0, 3) and nstats == {"records": 2, "loci": 0, "jobs": 0, "pairs": 0, "max_len": 21}
    load(gpu_ctx, recs[:0], 2)                                                  # no records
    got, counts, stats = check(gpu_ctx, recs[:0], arr, [500, 99], 2)
    assert not got["reads"].any() and stats == {"records": 0, "loci": 4, "jobs": 0, "pairs": 0, "max_len": 0}
    assert gpu_ctx.last_jobs_per_slot(COUNT) == (0, 0)


def test_bad_arguments_are_refused(gpu_ctx):
    recs = make_records([(0, 100, 3, 21, 0, 0)])
    load(gpu_ctx, recs, 1)
    ok = (0, ".", 1, 500)
    for bad, lens, ns in ((L(ok, (1, ".", 1, 5)), [500], 1), (L((-1, ".", 1, 5)), [500], 1), (L((0, ".", 0, 5)), [500], 1), (L((0, ".", 6, 5)), [500], 1),
                          (L((0, ".", 1, 501)), [500], 1), (L(ok), [500], 0), (L(ok), [500], 256), (L(ok), [-1], 1), (L(ok), [1 << 31], 1)):
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.locus_scan(bad, lens, ns)
        assert "(-1)" in str(e.value), str(e.value)
    odd = L(ok)
    odd["strand"] = 3
    with pytest.raises(capi.MirpError):
        gpu_ctx.locus_scan(odd, [500], 1)
    assert gpu_ctx.locus_scan(L(ok), [500], 1)[0]["reads"].tolist() == [3]      # and nothing resident changed


# ---------------------------------------------------------------------------------------------------- 7: round trip with clusters
def test_clusters_on_their_own_gff3(sweep, tmp_path):
    d, paths, names, lens, recs, kept, seqs = sweep
    pad = int(recs["len"].max())                                               # no record can overlap two clusters
    r = _cli("mir_prefer_amd.clusters", ["-m", "20", "--pad", str(pad), "-g", str(d / "g.fa"), "-o", str(tmp_path / "cl")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    r = _cli("mir_prefer_amd.loci", ["-g", str(d / "g.fa"), "-o", str(tmp_path / "lo"), str(tmp_path / "cl.gff3")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    cl = [ln.split(b"\t") for ln in (tmp_path / "cl.tsv").read_bytes().split(b"\n")[:-1]]
    lo = [ln.split(b"\t") for ln in (tmp_path / "lo.tsv").read_bytes().split(b"\n")[:-1]]
    assert len(cl) == len(lo) > 30
    assert [row[4:] for row in cl] == [row[6:] for row in lo]                  # reads .. long
    assert [row[1:4] for row in cl] == [row[2:5] for row in lo] and [row[0] for row in cl[1:]] == [row[0] for row in lo[1:]]
    a, b = (tmp_path / "cl.counts.tsv").read_bytes(), (tmp_path / "lo.counts.tsv").read_bytes()
    assert a == b


# ---------------------------------------------------------------------------------------------------- 8: refusals, and the chain through phasing
def test_refusals_leave_no_output(tmp_path):
    sam = tmp_path / "a.sam"
    recs = make_records([(0, 10 + 5 * j, 3, 21, j % 2, 0) for j in range(10)])
    write_sams([str(sam)], ["c1", "c2"], [500, 300], recs)
    _genome(tmp_path / "short.fa", ["c1", "c2"], [b"A" * 500, b"A" * 299])
    (tmp_path / "bad.sam").write_bytes(sam.read_bytes() + b"r_x1\t0\tnope\t5\t255\t21M\t*\t0\t0\t" + b"A" * 21 + b"\t*\n")
    (tmp_path / "ok.gff3").write_text("c1\ts\tgene\t1\t60\t.\t+\t.\tID=a\nother\ts\tgene\t1\t60\t.\t+\t.\tID=b\n")
    (tmp_path / "past.gff3").write_text("c2\ts\tgene\t1\t301\t.\t+\t.\tID=a\n")
    (tmp_path / "nowhere.bed").write_text("other\t0\t10\n")
    (tmp_path / "twice.gff3").write_text("c1\ts\tgene\t1\t60\t.\t+\t.\tID=a\nc1\ts\texon\t1\t20\t.\t+\t.\tID=a\n")
    cases = [(["ok.gff3", "bad.sam"], "not in the @SQ header"), (["-g", "short.fa", "ok.gff3", "a.sam"], "contig c2 has 299 bases"),
             (["past.gff3", "a.sam"], "locus a ends at 301, beyond the end of sequence c2 (LN:300)"), (["nowhere.bed", "a.sam"], "no locus of the loci file"),
             (["twice.gff3", "a.sam"], "twice.gff3 line 2: the name a occurs twice")]
    for args, why in cases:
        args = [a if a.startswith("-") else str(tmp_path / a) for a in args]
        outs = loci.output_paths(args[-1] + ".loci")
        for p in outs:
            open(p, "wb").write(b"stale\n")
        r = _cli("mir_prefer_amd.loci", args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr.decode())
        assert not any(os.path.exists(p) for p in outs)
    r = _cli("mir_prefer_amd.loci", ["-t", "gene", str(tmp_path / "twice.gff3"), str(sam)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = R.files_plain(recs, [("a", "gene", "c1", 1, 60, "+")], ["c1", "c2"], [500, 300], list(capi.ingest_sams([str(sam)])[2]))
    assert [open(str(sam) + ".loci" + e, "rb").read() for e in (".tsv", ".counts.tsv")] == list(want)
    r = _cli("mir_prefer_amd.loci", [str(tmp_path / "ok.gff3"), str(sam)], tmp_path)
    assert r.returncode == 0 and "1 loci kept / 1 dropped" in r.stderr.decode()


def test_chain_collapse_align_phasing_loci(tmp_path):
    """The planted genome of the triggers chain test: ten registers of a 21-nt phase on chr1 and a miRNA whose cut falls on one of them."""
    from tests.test_phasing_gpu import _revcomp
    from tests.test_triggers_cpu import ACGT, lines_of
    rng = np.random.RandomState(12)
    Lp, x0 = 21, 10001
    genome = bytearray(ACGT[rng.randint(0, 4, 30000)].tobytes())
    mirna = bytes(ACGT[rng.randint(0, 4, 21)].tobytes())
    s1 = x0 + 2 * Lp - 11
    genome[s1 - 1:s1 - 1 + 21] = _revcomp(mirna)
    other = ACGT[rng.randint(0, 4, 5000)].tobytes()
    _genome(tmp_path / "genome.fa", ["chr1", "chr2"], [bytes(genome), other])
    reads = []
    for j in range(10):
        c = x0 + j * Lp
        reads += [bytes(genome[c - 1:c - 1 + Lp])] * 3 + [_revcomp(bytes(genome[c - 3:c - 3 + Lp]))] * 2
    (tmp_path / "reads.fa").write_bytes(b"".join(b">q%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    (tmp_path / "names.txt").write_text("S1\n")
    (tmp_path / "mir.fa").write_bytes(b">mir-t\n" + mirna.replace(b"T", b"U") + b"\n")
    sam = "reads.fa.processed.sam"
    for module, args in (("mir_prefer_amd.reads", ["collapse", "names.txt", "reads.fa"]),
                         ("mir_prefer_amd.align", ["-f", "-r", "genome.fa", "reads.fa.processed"]),
                         ("mir_prefer_amd.phasing", ["-g", "genome.fa", sam]),
                         ("mir_prefer_amd.triggers", ["-s", "0", "mir.fa", "genome.fa", sam + ".phas.tsv", sam]),
                         ("mir_prefer_amd.loci", ["--format", "phas", "-g", "genome.fa", "-o", "pl", sam + ".phas.tsv", sam])):
        r = _cli(module, args, tmp_path)
        assert r.returncode == 0, (module, r.stderr.decode())
    rows = lines_of((tmp_path / "pl.tsv").read_bytes())
    summary = lines_of((tmp_path / (sam + ".phas.triggers.summary.tsv")).read_bytes())
    assert [row[0] for row in rows] == [row[0] for row in summary] and len(rows) == 1
    assert rows[0][1:3] == [b"PHAS", b"chr1"] and int(rows[0][6]) == 50 and rows[0][9] == b"21" and rows[0][12:14] == [b"+", b"21"]
    names, lens, samples, alns = capi.ingest_sams([str(tmp_path / sam)])
    seqs = {"chr1": bytes(genome), "chr2": other}
    want = R.files_plain(alns, R.read_phas(str(tmp_path / (sam + ".phas.tsv"))), names, lens.tolist(), list(samples), False, seqs)
    assert [(tmp_path / f).read_bytes() for f in ("pl.tsv", "pl.counts.tsv")] == list(want)
    # the auto format takes the name's ending
    r = _cli("mir_prefer_amd.loci", ["-o", "pa", sam + ".phas.tsv", sam], tmp_path)
    assert r.returncode == 0 and (tmp_path / "pa.counts.tsv").read_bytes() == want[1]
