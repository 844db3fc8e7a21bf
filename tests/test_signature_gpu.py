"""GPU tests of the signature verb (mirp_signature_scan, signature_kernels.hip), by exact equality of rows, H, sites, stats and
file bytes with the restatements of tests/signature_restatement.py: the worked examples of the definition (one duplex, the near misses, the
overhangs, min() in both directions past 32 bits, the locus edges, nested, overlapping, duplicate and empty loci, no locus, the contig join,
the length filter, K = 1 and 64 over a dense V, the ties of the major duplex, --min-reads); U ranges and placement ranges of C - 1, C, C + 1
and 2 C + 1 rows (C = capi.SIGNATURE_CHUNK) with a list longer than a chunk; waves that serve three and more jobs; a contig of 2^31 - 1 bases;
two calls with the same bytes; about 1,000 loci over about 10^5 records; and the command line with its refusals."""
import os

import numpy as np
import pytest

from mir_prefer_amd import capi, signature
from tests import signature_restatement as R
from tests.test_clusters_cpu import make_records, random_seqs
from tests.test_clusters_gpu import _cli, _genome, write_sams
from tests.test_loci_cpu import L, random_loci
from tests.test_signature_cpu import duplex_records, hist

pytestmark = pytest.mark.gpu

C = capi.SIGNATURE_CHUNK
OVERLAP = 7                                          # the overlap kernel's family of mirp_last_jobs_per_slot


def load(ctx, recs, n_contigs):
    ctx.load_genome([("c%d" % i, np.full(4, 65, np.uint8)) for i in range(n_contigs)])
    ctx.load_alignments(recs)


def check(ctx, recs, arr, lens, **kw):
    """One call against the numpy statement: rows, H, sites and stats, exactly."""
    o = R.options(**kw)
    got, H, sites, stats = ctx.signature_scan(arr, lens, o["min_len"], o["max_len"], o["max_overlap"], o["overhang"], o["min_reads"])
    want, wH, wsites, wstats = R.scan_numpy(recs, arr, lens, **kw)
    assert got.tobytes() == want.tobytes() and H.shape == wH.shape and (H == wH).all() and sites.tobytes() == wsites.tobytes()
    assert stats == wstats
    return got, H, sites, stats


def case(ctx, rows, loci_rows, lens, **kw):
    recs = make_records(rows)
    load(ctx, recs, len(lens))
    return check(ctx, recs, L(*loci_rows), lens, **kw)


WHOLE = [(0, ".", 1, 1000)]


# ---------------------------------------------------------------------------------------------------- 1: the rule on the smallest inputs
def test_one_duplex_and_its_near_misses(gpu_ctx):
    got, H, sites, st = case(gpu_ctx, [(0, 100, 5, 21, 0), (0, 98, 3, 21, 1)], WHOLE, [1000], min_reads=1)
    assert hist(H) == {19: 3} and got[["reads", "plus_reads", "duplexes", "duplex_reads"]].tolist() == [(8, 5, 1, 3)]
    assert sites.tolist() == [(0, 100, 5, 3, 21, 0)] and st == {"records": 2, "kept": 2, "u_entries": 1, "v_entries": 1, "jobs": 1, "sites": 1}
    assert got[["major_pos", "major_len", "major_plus", "major_minus"]].tolist() == [(100, 21, 5, 3)]
    for minus, overlap in (((99, 21), 20), ((97, 21), 18), ((98, 22), 20)):       # shifted by one either way; one base longer
        got, H, sites, _ = case(gpu_ctx, [(0, 100, 5, 21, 0), (0, minus[0], 3, minus[1], 1)], WHOLE, [1000], min_reads=1)
        assert hist(H) == {overlap: 3} and int(got["duplexes"][0]) == 0 and len(sites) == 0 and int(got["reads"][0]) == 8
        assert got[["major_pos", "major_len", "major_plus", "major_minus"]].tolist() == [(0, 0, 0, 0)]
    rows = [(0, 100, 5, 21, 0), (0, 100, 2, 21, 1), (0, 99, 3, 21, 1), (0, 98, 4, 21, 1), (0, 97, 6, 21, 1)]
    for o, minus in ((0, 2), (1, 3), (2, 4), (3, 6)):                             # the overhang selects the matching pair
        _, H, sites, _ = case(gpu_ctx, rows, WHOLE, [1000], overhang=o, min_reads=1)
        assert sites.tolist() == [(0, 100, 5, minus, 21, 0)] and hist(H) == {21: 2, 20: 3, 19: 4, 18: 5}


def test_min_in_both_directions_past_32_bits(gpu_ctx):
    top = (1 << 32) - 1
    for a, b in ((0, 1), (1, 0)):
        pos = {0: 100, 1: 98}
        got, H, sites, _ = case(gpu_ctx, [(0, pos[a], top, 21, a), (0, pos[a], top, 21, a), (0, pos[b], 7, 21, b)], WHOLE, [1000])
        assert hist(H) == {19: 7} and int(got["reads"][0]) == 2 * top + 7 and int(got["duplex_reads"][0]) == 7
        assert sorted(sites[["plus_reads", "minus_reads"]].tolist()[0]) == [7, 2 * top]
    got, H, _, _ = case(gpu_ctx, [(0, 100, top, 21, 0)] * 3 + [(0, 98, top, 21, 1)] * 2, WHOLE, [1000])
    assert hist(H) == {19: 2 * top} and int(got["major_plus"][0]) == 3 * top and int(got["major_minus"][0]) == 2 * top > 1 << 32


def test_locus_edges_nested_duplicate_and_empty_loci(gpu_ctx):
    rows = [(0, 100, 5, 21, 0), (0, 98, 3, 21, 1), (0, 200, 9, 21, 0), (0, 198, 4, 21, 1)]
    loc = [(0, ".", 100, 118), (0, ".", 101, 118), (0, ".", 100, 117), (0, ".", 99, 119), (0, ".", 1, 1000), (0, ".", 119, 199), (0, ".", 100, 118),
           (0, ".", 110, 210), (0, ".", 200, 217), (0, ".", 200, 218), (1, ".", 1, 300)]
    got, H, sites, _ = case(gpu_ctx, rows, loc, [1000, 300], min_reads=1)
    assert got["reads"].tolist() == [8, 3, 5, 8, 21, 0, 8, 12, 9, 13, 0] and got["plus_reads"].tolist() == [5, 0, 5, 5, 14, 0, 5, 9, 9, 9, 0]
    assert got["duplexes"].tolist() == [1, 0, 0, 1, 2, 0, 1, 0, 0, 1, 0] and got["duplex_reads"].tolist() == [3, 0, 0, 3, 7, 0, 3, 0, 0, 4, 0]
    assert [hist(H, q) for q in range(11)] == [{19: 3}, {}, {}, {19: 3}, {19: 7}, {}, {19: 3}, {}, {}, {19: 4}, {}]
    assert sites[["locus", "pos"]].tolist() == [(0, 100), (3, 100), (4, 100), (4, 200), (6, 100), (9, 200)]
    assert got[0:1].tobytes() == got[6:7].tobytes()
    # no locus; a call with loci but no site; no records
    none, nH, nsites, nst = gpu_ctx.signature_scan(L()[:0], [1000, 300])
    assert len(none) == 0 and nH.shape == (0, 30) and len(nsites) == 0 and nst == {"records": 4, "kept": 0, "u_entries": 0, "v_entries": 0, "jobs": 0, "sites": 0}
    assert gpu_ctx.last_jobs_per_slot(OVERLAP) == (0, 0)
    _, _, sites, st = check(gpu_ctx, make_records(rows), L(*loc), [1000, 300])
    assert len(sites) == 0 and st["sites"] == 0 and gpu_ctx.last_jobs_per_slot(OVERLAP) == (1, 1)
    load(gpu_ctx, make_records(rows)[:0], 2)
    got, H, sites, st = check(gpu_ctx, make_records(rows)[:0], L(*loc), [1000, 300])
    assert not got["reads"].any() and not H.any() and st == {"records": 0, "kept": 0, "u_entries": 0, "v_entries": 0, "jobs": 0, "sites": 0}


def test_contig_join_never_pairs(gpu_ctx):
    for K in (30, 64):
        rows = [(0, 500, 5, 21, 0), (0, 498, 2, 21, 0)] + [(1, y - 20, 3, 21, 1) for y in range(1, K + 1)] + [(1, 1, 7, 21, 0)]
        got, H, sites, _ = case(gpu_ctx, rows, [(0, ".", 1, 500), (1, ".", 1, 300), (1, ".", 1, 1), (0, ".", 500, 500)], [500, 300], max_overlap=K, min_reads=1)
        assert not H[0].any() and not H[3].any() and not got["duplexes"][[0, 3]].any() and got["reads"].tolist() == [7, 3 * K + 7, 10, 5]
        assert hist(H, 1) == {k: 3 for k in range(1, K + 1)} and hist(H, 2) == {1: 3}      # the locus at the start of contig 1 sees its own '+' only


def test_length_filter(gpu_ctx):
    rows = [(0, 100, 5, 19, 0), (0, 100, 6, 20, 0), (0, 100, 7, 25, 0), (0, 100, 8, 26, 0),
            (0, 98, 1, 19, 1), (0, 98, 2, 20, 1), (0, 98, 3, 25, 1), (0, 98, 4, 26, 1)]
    got, H, sites, st = case(gpu_ctx, rows, WHOLE, [1000], min_reads=1)
    assert int(got["reads"][0]) == 18 and st["kept"] == 4 and sites[["len", "plus_reads", "minus_reads"]].tolist() == [(20, 6, 2), (25, 7, 3)]
    assert hist(H) == {18: 2, 23: 3}
    got, _, sites, st = case(gpu_ctx, rows, WHOLE, [1000], min_reads=1, min_len=19, max_len=26)
    assert int(got["reads"][0]) == 36 and st["kept"] == 8 and len(sites) == 4
    got, _, sites, st = case(gpu_ctx, rows + [(0, 300, 9, 65535, 0), (0, 298, 9, 65535, 1)], [(0, ".", 1, 70000)], [70000], min_reads=1, min_len=3,
                             max_len=65535)
    assert st["kept"] == 10 and len(sites) == 5 and int(got["reads"][0]) == 54


def test_max_overlap_1_and_64_over_a_dense_v(gpu_ctx):
    rng = np.random.RandomState(90)
    rows = [(0, f - 20, int(rng.randint(1, 9)), 21, 1) for f in range(1000, 1300)]                  # V has an entry at every position of [1000, 1299]
    rows += [(0, int(x), int(rng.randint(1, 9)), 21, 0) for x in (990, 1000, 1001, 1100, 1236, 1237, 1299, 1300)]
    rows += [(0, 5000, 5, 21, 0), (0, 5000 + 64 - 21, 3, 21, 1), (0, 6000, 5, 21, 0), (0, 6000 + 65 - 21, 3, 21, 1)]      # overlaps K and K + 1 at K = 64
    loc = [(0, ".", 1, 9000), (0, ".", 1000, 1299), (0, ".", 1100, 1150), (0, ".", 4000, 7000)]
    for K in (64, 1, 30):
        got, H, _, _ = case(gpu_ctx, rows, loc, [9000], max_overlap=K)
        assert (H[1] > 0).all() and (H[0] >= H[1]).all()                           # the walk takes K steps
    got, H, _, _ = case(gpu_ctx, rows, loc, [9000], max_overlap=64)
    assert hist(H, 3) == {64: 3}                                                    # the pair at overlap 65 is not counted
    assert hist(case(gpu_ctx, rows, loc, [9000], max_overlap=1)[1], 3) == {}


def test_major_duplex_ties_and_min_reads(gpu_ctx):
    def major(rows):
        g = case(gpu_ctx, rows, [(0, ".", 1, 900)], [1000], min_reads=1)[0][0]
        return [int(g[f]) for f in ("major_pos", "major_len", "major_plus", "major_minus")]
    assert major([(0, 100, 5, 21, 0), (0, 98, 3, 21, 1), (0, 200, 3, 21, 0), (0, 198, 9, 21, 1)]) == [100, 21, 5, 3]
    assert major([(0, 100, 5, 24, 0), (0, 98, 3, 24, 1), (0, 100, 3, 21, 0), (0, 98, 9, 21, 1)]) == [100, 21, 3, 9]
    assert major([(0, 100, 5, 21, 0), (0, 98, 3, 21, 1), (0, 200, 4, 21, 0), (0, 198, 9, 21, 1)]) == [200, 21, 4, 9]
    for mr, n in ((4, 1), (5, 1), (6, 0)):
        got, _, sites, _ = case(gpu_ctx, [(0, 100, 5, 21, 0), (0, 98, 9, 21, 1)], [(0, ".", 1, 900)], [1000], min_reads=mr)
        assert len(sites) == n and int(got["duplexes"][0]) == 1 and int(got["duplex_reads"][0]) == 5


def test_contig_of_2_31_minus_1(gpu_ctx):
    top = (1 << 31) - 1
    rows = [(0, top - 18, 5, 21, 0), (0, top - 20, 3, 21, 1), (0, top, 4, 21, 0), (0, top - 19, 2, 21, 1), (1, 5, 6, 21, 0), (1, 3, 6, 21, 1)]
    loc = [(0, ".", 1, top), (0, ".", top, top), (0, ".", top - 18, top - 1), (1, ".", 1, top - 10)]
    got, H, sites, _ = case(gpu_ctx, rows, loc, [top, top - 10], min_reads=1)
    assert got["reads"].tolist() == [12, 7, 5, 12] and hist(H, 0) == {19: 3, 1: 3} and hist(H, 1) == {1: 3} and sites[["locus", "pos"]].tolist() == [(0, top - 18), (3, 5)]


def test_bad_arguments_are_refused(gpu_ctx):
    recs = make_records([(0, 100, 5, 21, 0), (0, 98, 3, 21, 1)])
    load(gpu_ctx, recs, 1)
    ok = (0, ".", 1, 500)
    for bad, lens, kw in ((L(ok, (1, ".", 1, 5)), [500], {}), (L((-1, ".", 1, 5)), [500], {}), (L((0, ".", 0, 5)), [500], {}), (L((0, ".", 6, 5)), [500], {}),
                          (L((0, ".", 1, 501)), [500], {}), (L(ok), [-1], {}), (L(ok), [1 << 31], {}), (L(ok), [500], {"min_len": 0}),
                          (L(ok), [500], {"min_len": 26}), (L(ok), [500], {"max_len": 65536}), (L(ok), [500], {"max_overlap": 0}),
                          (L(ok), [500], {"max_overlap": 65}), (L(ok), [500], {"overhang": -1}), (L(ok), [500], {"overhang": 9}),
                          (L(ok), [500], {"overhang": 2, "min_len": 2}), (L(ok), [500], {"min_reads": 0})):
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.signature_scan(bad, lens, **kw)
        assert "(-1)" in str(e.value), str(e.value)
    odd = L(ok)
    odd["strand"] = 7                                                              # the locus strand is not looked at
    assert gpu_ctx.signature_scan(odd, [500])[0]["reads"].tolist() == [8]           # and nothing resident changed


# ---------------------------------------------------------------------------------------------------- 2: job boundaries
def test_ranges_around_a_multiple_of_the_chunk(gpu_ctx):
    """Contigs 0..3: m distinct '+' 5' positions (m U entries = m '+' placements), each with its duplex partner.  Contigs 4..7: a placement range
    of exactly m rows, floor(m / 2) duplex pairs and, for an odd m, one '+' placement without a partner."""
    sizes = [C - 1, C, C + 1, 2 * C + 1]
    rows, loc = [], []
    for k, m in enumerate(sizes + sizes):
        n_plus = m if k < 4 else (m + 1) // 2
        start = 100000
        for i in range(n_plus):
            p = start + 3 * i
            rows.append((k, p, 5 + i % 7, 21, 0))
            if k < 4 or 2 * i + 1 < m:
                rows.append((k, p - 2, 5 + i % 5, 21, 1))
        end = start + 3 * (n_plus - 1) + 18                                        # the last partner's 5' end
        rows += [(k, start - 40, 9, 21, 0), (k, start - 60, 9, 21, 1), (k, end + 1, 9, 21, 0), (k, end + 30, 9, 21, 1)]
        loc += [(k, ".", start, end), (k, ".", start, end - 1), (k, ".", start + 1, end - 3 * (n_plus // 2))]
    recs = make_records(rows)
    lens = [400000] * 8
    arr = L(*loc)
    load(gpu_ctx, recs, 8)
    got, H, sites, stats = check(gpu_ctx, recs, arr, lens)
    # the construction: U entries and placement rows of the first locus of every contig
    f = np.where(recs["strand"] == 1, recs["pos"].astype(np.int64) + recs["len"] - 1, recs["pos"])
    for k, m in enumerate(sizes + sizes):
        s, e = int(arr["start"][3 * k]), int(arr["end"][3 * k])
        on = recs["tid"] == k
        assert int((on & (recs["strand"] == 0) & (f >= s) & (f <= e)).sum()) == (m if k < 4 else (m + 1) // 2)
        assert int((on & (recs["pos"] >= s - 24) & (recs["pos"] <= e)).sum()) == (2 * m if k < 4 else m)
    assert got["duplexes"][0:12:3].tolist() == sizes and got["duplexes"][12:24:3].tolist() == [m // 2 for m in sizes]
    assert got["duplexes"][1:12:3].tolist() == [m - 1 for m in sizes]              # one base short on the right: the last partner is outside
    assert int(np.bincount(sites["locus"], minlength=len(arr))[9]) == 2 * C + 1     # a list of more sites than one chunk
    # every locus alone gives the same row, the same H and the same sites
    for q in range(len(arr)):
        a_rows, a_H, a_sites, a_stats = gpu_ctx.signature_scan(arr[q:q + 1], lens)
        if q % 3 == 0:                                                             # the U entries of the first locus of contig q / 3, in jobs of C
            m = (sizes + sizes)[q // 3]
            assert a_stats["jobs"] == -(-(m if q < 12 else (m + 1) // 2) // C), q
        mine = sites[sites["locus"] == q].copy()
        mine["locus"] = 0
        assert a_rows.tobytes() == got[q:q + 1].tobytes() and (a_H == H[q:q + 1]).all() and a_sites.tobytes() == mine.tobytes(), q


# ---------------------------------------------------------------------------------------------------- 3: slot reuse
def test_waves_serve_three_jobs_and_more(gpu_ctx):
    rng = np.random.RandomState(91)
    heavy_n, small_n = 6, 12300                                               # 12,318 jobs: three and more for every one of 4,096 waves
    span = 3 * (2 * C + 500)
    rows = []
    for h in range(heavy_n):                                                   # 2 C + 500 U entries under every heavy locus: three jobs each
        base = 50000 * (h + 1)
        for i in range(2 * C + 500):
            rows.append((0, base + 3 * i, int(rng.randint(1, 99)), int(rng.choice([21, 22, 24])), 0))
            if i % 3 == 0:
                rows.append((0, base + 3 * i - int(rng.choice([2, 2, 1])), int(rng.randint(1, 99)), int(rng.choice([21, 21, 24])), 1))
    small_pos = 1 + 60 * np.arange(small_n)
    plus = np.zeros(small_n, make_records([]).dtype)
    plus["tid"], plus["pos"], plus["depth"], plus["len"] = 1, small_pos + 10, rng.randint(1, 50, small_n), 21
    minus = plus.copy()
    minus["pos"], minus["depth"], minus["strand"] = plus["pos"] - rng.choice([2, 2, 3], small_n), rng.randint(1, 50, small_n), 1
    recs = np.concatenate([make_records(rows), make_records([tuple(r) for r in np.concatenate([plus, minus]).tolist()])])
    arr = np.zeros(heavy_n + small_n, capi.LOCUS_DTYPE)                        # the heavy loci first
    arr["strand"] = 2
    arr["tid"][heavy_n:] = 1
    arr["start"][:heavy_n], arr["end"][:heavy_n] = 50000 * (1 + np.arange(heavy_n)), 50000 * (1 + np.arange(heavy_n)) + span
    arr["start"][heavy_n:], arr["end"][heavy_n:] = small_pos + 5, small_pos + 40
    lens = [400000, 60 * small_n + 100]
    load(gpu_ctx, recs, 2)
    got, H, sites, stats = check(gpu_ctx, recs, arr, lens)
    launches, per_slot = gpu_ctx.last_jobs_per_slot(OVERLAP)
    assert stats["jobs"] == 3 * heavy_n + small_n and launches == 1 and per_slot >= 3, (stats, launches, per_slot)
    assert int(got["duplexes"][:heavy_n].min()) > 400 and 0.5 < float(got["duplexes"][heavy_n:].mean()) < 0.8 and int((H[heavy_n:].sum(1) > 0).sum()) == small_n


# ---------------------------------------------------------------------------------------------------- 4: the sweep
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    rng = np.random.RandomState(92)
    names, lens = ["chrB", "short", "chrA"], [300000, 1500, 500000]           # @SQ order is not the lexicographic one
    recs = duplex_records(rng, lens, 20000, 30000)
    kept = random_loci(rng, names, lens, 1000)
    return names, lens, recs, kept


def test_sweep_matches_both_restatements_and_is_deterministic(gpu_ctx, sweep):
    names, lens, recs, kept = sweep
    assert 90000 < len(recs) < 130000
    load(gpu_ctx, recs, 3)
    arr = R.locus_array(kept, names)
    got, H, sites, stats = check(gpu_ctx, recs, arr, lens)
    again = gpu_ctx.signature_scan(arr, lens)
    assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == H.tobytes() and again[2].tobytes() == sites.tobytes() and again[3] == stats
    assert len(sites) > 10000 and int((got["duplexes"] == 0).sum()) > 0 and int(got["duplexes"].max()) > 1000
    check(gpu_ctx, recs, arr, lens, min_len=18, max_len=30, max_overlap=64, overhang=0, min_reads=1)
    # the plain double loop on every 25th locus, through the files
    sub = list(range(0, len(kept), 25))
    pick = np.isin(sites["locus"], sub)
    renumbered = sites[pick].copy()
    renumbered["locus"] //= 25
    files = signature.format_files([kept[q] for q in sub], got[sub], H[sub], renumbered, 2)
    assert files == R.files_plain(recs, [kept[q] for q in sub], names)


# ---------------------------------------------------------------------------------------------------- 5: the command line
def test_cli_files_contigs_and_refusals(tmp_path):
    rng = np.random.RandomState(93)
    names, lens = ["chrB", "short", "chrA"], [4000, 150, 6000]
    recs = duplex_records(rng, lens, 300, 500)
    recs["sample"] = rng.randint(0, 2, len(recs))
    paths = [str(tmp_path / ("s%d.sam" % i)) for i in range(2)]
    write_sams(paths, names, lens, recs)
    kept = random_loci(rng, names, lens, 40)
    seqs = dict(zip(names, random_seqs(rng, lens)))
    gff = tmp_path / "loci.gff3"
    gff.write_text("##gff-version 3\n" + "".join("%s\tsrc\t%s\t%d\t%d\t.\t%s\t.\tID=%s;Note=x\n" % (c, t, a, b, s, n) for n, t, c, a, b, s in kept)
                   + "nowhere\tsrc\tt0\t1\t5\t.\t+\t.\tID=dropped\n")
    _genome(tmp_path / "g.fa", names[::-1], [seqs[n] for n in names[::-1]])
    outs = ("x.tsv", "x.overlaps.tsv", "x.duplexes.tsv")
    for extra, kw, with_g in (([], {}, False), (["-g", str(tmp_path / "g.fa"), "--min-len", "18", "--max-len", "30", "--max-overlap", "40", "--overhang", "0",
                                                 "--min-reads", "2"], dict(min_len=18, max_len=30, max_overlap=40, overhang=0, min_reads=2), True)):
        r = _cli("mir_prefer_amd.signature", extra + ["-o", str(tmp_path / "x.tsv"), str(gff)] + paths, tmp_path)
        assert r.returncode == 0, r.stderr.decode()
        want = R.files_plain(recs, kept, names, seqs if with_g else None, **kw)
        assert [(tmp_path / f).read_bytes() for f in outs] == list(want) and want[2].count(b"\n") > 20
        rows, _, sites, st = R.scan_numpy(recs, R.locus_array(kept, names), lens, **kw)
        o = R.options(**kw)
        assert r.stderr.decode().splitlines() == [
            "signature: %d records, %d kept (%d..%d nt), %d loci kept / 1 dropped (sequence not in the SAM header), %d loci with a duplex, "
            "%d duplexes listed, written to %s" % (len(recs), st["kept"], o["min_len"], o["max_len"], len(kept), int((rows["duplexes"] > 0).sum()),
                                                   len(sites), tmp_path / "x.tsv")]
    # -t and the default base; --contigs
    t1 = [l for l in kept if l[1] == "t1"]
    r = _cli("mir_prefer_amd.signature", ["-t", "t1", str(gff), paths[1], paths[0]], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert [open(paths[1] + ".signature" + e, "rb").read() for e in (".tsv", ".overlaps.tsv", ".duplexes.tsv")] == list(R.files_plain(recs, t1, names))
    r = _cli("mir_prefer_amd.signature", ["--contigs", "-g", str(tmp_path / "g.fa"), "-o", str(tmp_path / "w")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    whole = [(n, "contig", n, 1, ln, ".") for n, ln in zip(names, lens)]
    assert [(tmp_path / f).read_bytes() for f in ("w.tsv", "w.overlaps.tsv", "w.duplexes.tsv")] == list(R.files_plain(recs, whole, names, seqs))
    # refusals leave no output and remove an earlier run's files
    (tmp_path / "past.gff3").write_text("short\ts\tgene\t1\t151\t.\t+\t.\tID=a\n")
    (tmp_path / "nowhere.bed").write_text("other\t0\t10\n")
    (tmp_path / "twice.gff3").write_text("chrB\ts\tgene\t1\t60\t.\t+\t.\tID=a\nchrB\ts\texon\t1\t20\t.\t+\t.\tID=a\n")
    _genome(tmp_path / "short.fa", names, [seqs["chrB"], seqs["short"][:-1], seqs["chrA"]])
    for args, why in ((["past.gff3"], "locus a ends at 151, beyond the end of sequence short (LN:150)"), (["nowhere.bed"], "no locus of the loci file"),
                      (["twice.gff3"], "twice.gff3 line 2: the name a occurs twice"), (["-g", "short.fa", "loci.gff3"], "contig short has 149 bases")):
        args = [a if a.startswith("-") else str(tmp_path / a) for a in args] + [paths[0]]
        stale = signature.output_paths(paths[0] + ".signature")
        for p in stale:
            open(p, "wb").write(b"stale\n")
        r = _cli("mir_prefer_amd.signature", args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr.decode())
        assert not any(os.path.exists(p) for p in stale)
