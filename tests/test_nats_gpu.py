"""The NAT search on the device (mirp_nats_scan, nats_kernels.hip) against its restatement (tests/nats_restatement.py): exact
equality of the records, the cigars, every counter and the bytes of the three files.  The shapes are the smallest at which the kernels take
another path: transcripts around k and around the band's width, seeds in the matrix's corners, regions that drift to the band's edge and past it,
every number of diagonals per lane, a wave's second and third candidate, the longest transcript, passes of one transcript and one candidate."""
import os
import random
import subprocess
import sys

import pytest

from tests import nats_cases as C
from tests import nats_restatement as R
from tests.test_targets_cpu import ROOT

pytestmark = pytest.mark.gpu


def as_dicts(recs, cigars):
    return [dict({f: int(r[f]) for f in R.FIELDS}, cigar=cg) for r, cg in zip(recs, cigars)]


def check(ctx, seqs, want=None, capacity=0, **opts):
    """One call against the restatement: records, cigars, counters, file bytes.  -> (records as dicts, stats)"""
    from mir_prefer_amd import nats
    if want is None:
        want = R.find(seqs, **opts)
    recs, cigars = ctx.nats_scan(seqs, capacity=capacity, **opts)
    stats = ctx.nats_last_stats()
    got = as_dicts(recs, cigars)
    assert got == want[0]
    assert {f: stats[f] for f in R.STAT_NAMES} == want[1]
    names = ["t%d|x" % k for k in range(len(seqs))]
    assert nats.tsv_table(names, recs, cigars) == R.tsv_text(names, want[0])
    assert nats.pairs_table(names, recs) == R.pairs_text(names, want[0])
    assert nats.bed_table(names, recs) == R.bed_text(names, want[0])
    return got, stats


def brief(recs):
    return [(r["a"], r["b"], r["score"], r["a_start"], r["a_end"], r["b_start"], r["b_end"], r["cigar"]) for r in recs]


def test_pins(gpu_ctx):
    seqs, where = C.perfect_region()
    got, _ = check(gpu_ctx, seqs)
    assert brief(got) == [(0, 1, 360) + where + ("120=",)] and got[0]["seeds"] == 105
    seqs, o, where = C.n_in_seed()
    got, stats = check(gpu_ctx, seqs, **o)
    assert stats["seed_hits"] == 9 and got[0]["seeds"] == 9 and got[0]["cigar"] == "20=1X19="
    seqs, o = C.occurrence_edge()
    got, stats = check(gpu_ctx, seqs, max_occ=3, **o)
    assert [(r["a"], r["b"]) for r in got] == [(0, 1), (1, 2), (1, 3)] and stats["kmers_ignored"] == 0
    got, stats = check(gpu_ctx, seqs, max_occ=2, **o)
    assert got == [] and stats["kmers_ignored"] == 2 and stats["seed_hits"] == 0
    seqs, o, where = C.two_seeds()
    for min_seeds, n in ((1, 1), (2, 1), (3, 0)):
        got, stats = check(gpu_ctx, seqs, min_seeds=min_seeds, **o)
        assert len(got) == n and stats["seed_hits"] == 2 and stats["kept_candidates"] == n
    (first, second), o = C.end_cell_ties()
    assert brief(check(gpu_ctx, first, **o)[0]) == [(0, 1, 90, 21, 50, 31, 60, "30=")]
    assert brief(check(gpu_ctx, second, **o)[0]) == [(0, 1, 90, 21, 50, 69, 98, "30=")]
    (first, second), o = C.traceback_ties()
    assert [r["cigar"] for r in check(gpu_ctx, first, **o)[0]] == ["20=1I21="]
    assert [r["cigar"] for r in check(gpu_ctx, second, **o)[0]] == ["20=1D1I20="]
    seqs, o = C.two_copies_in_b()
    assert [(r["a_start"], r["b_start"]) for r in check(gpu_ctx, seqs, **o)[0]] == [(61, 41), (61, 241)]
    seqs, o = C.two_bins()
    got, stats = check(gpu_ctx, seqs, **o)
    assert len(got) == 1 and stats["above"] == 2 and stats["candidates"] == 2


@pytest.mark.parametrize("first", [0, 10, 20])
def test_seeded_inputs(gpu_ctx, first):
    for seed in range(first, first + 10):
        seqs, o = C.seeded_inputs(seed)
        check(gpu_ctx, seqs, **o)


@pytest.mark.parametrize("k", [12, 16, 24])
@pytest.mark.parametrize("W", [16, 64])
def test_lengths_around_k_and_the_band(gpu_ctx, k, W):
    o = dict(seed=k, band=W, min_score=3 * k, min_length=k)
    got, stats = check(gpu_ctx, C.length_ladder(k, W), **o)
    assert {r["a"] for r in got} >= {2, 3, 7, 8, 9} and all(r["b"] == 10 for r in got if r["a"] in (2, 3, 7, 8, 9))
    got, stats = check(gpu_ctx, C.corner_seeds(k, W), **o)
    n, m = got[0]["a_len"], got[0]["b_len"]
    assert [(r["a_start"], r["b_start"], r["bin"]) for r in got] == [(1, 1, (k - 1) // W), (n - k + 1, m - k + 1, (n + m - k - 1) // W)]
    assert got[1]["a_end"] == n and got[1]["b_end"] == m and (n + m - 2) // W - got[1]["bin"] <= 2


@pytest.mark.parametrize("W", [16, 64])
def test_regions_that_drift_to_the_edge_of_the_band(gpu_ctx, W):
    for drift in (W // 2 - 1, W // 2, W // 2 + 1, W, W + 1):
        check(gpu_ctx, C.drifting_region(W, drift), seed=12, band=W, gap=1, min_score=60, min_length=20)
        check(gpu_ctx, C.drifting_region(W, drift), seed=12, band=W, gap=2, mismatch=3, min_score=60, min_length=20)


@pytest.mark.parametrize("W", [32, 128, 256])
def test_every_number_of_diagonals_per_lane(gpu_ctx, W):
    """W = 32, 128 and 256: 2, 6 and 12 diagonals per lane (16 and 64 run everywhere else)."""
    rng = random.Random(W)
    region = C.rand_seq(rng, 150)
    copy = C.mutate(rng, region, subs=0.04, indels=[(50, 2), (100, -3)])
    A, B = C.rand_seq(rng, 330), C.rand_seq(rng, 300)
    A = A[:90] + region + A[240:]
    rc = R.revcomp(copy)
    B = B[:60] + rc + B[60 + len(rc):]
    got, _ = check(gpu_ctx, [A, B, C.rand_seq(rng, 40)], seed=12, band=W, min_score=100, min_length=50)
    assert len(got) == 1 and got[0]["score"] > 250


def test_a_wave_serves_a_second_and_a_third_candidate(gpu_ctx):
    """300 short candidates in one call: 20 x 15 pairs of transcripts that share one 12-mer each."""
    from mir_prefer_amd import capi
    rng = random.Random(300)
    regions = [[C.rand_seq(rng, 12) for _ in range(15)] for _ in range(20)]
    first = ["T".join(regions[i][j] for j in range(15)) for i in range(20)]
    second = ["A".join(R.revcomp(regions[i][j]) for i in range(20)) for j in range(15)]
    got, stats = check(gpu_ctx, first + second, seed=12, band=16, min_score=36, min_length=12)
    assert stats["kept_candidates"] >= 300 and len({(r["a"], r["b"]) for r in got}) == 300
    launches, per_slot = gpu_ctx.last_jobs_per_slot(capi.NATS_FAMILY)
    assert launches == 1 and per_slot >= 3          # a wave serves four candidates in turn


def test_the_longest_transcripts(gpu_ctx):
    """Two transcripts of 65,535 nt, a diverged region of 400 nt ending at the last base of A and at the first of B: the end cell is the matrix's
    last cell.  The numpy statement covers that band alone."""
    rng = random.Random(65535)
    region = C.rand_seq(rng, 400)
    copy = C.mutate(rng, region, subs=0.03, indels=[(120, 1), (260, -2)])
    n = R.MAX_LEN
    A = C.rand_seq(rng, n - 400) + region
    B = R.revcomp(copy) + C.rand_seq(rng, n - len(copy))
    recs, cigars = gpu_ctx.nats_scan([A, B])
    stats = gpu_ctx.nats_last_stats()
    got = as_dicts(recs, cigars)
    assert len(got) == 1 and stats["bases"] == 2 * n and stats["skipped"] == 0
    r = got[0]
    score, i_end, j_end, ops, i0, j0, cells = R.np_extend(R.np_codes(A), R.np_rc(R.np_codes(B)), r["bin"], 64, 3, 4, 12)
    assert (r["score"], r["a_start"], r["a_end"], r["b_start"], r["b_end"], r["cigar"]) == (score, i0, i_end, n + 1 - j_end, n + 1 - j0, R.np_cigar(ops))
    assert (i_end, j_end) == (n, n) and r["a_len"] == r["b_len"] == n
    assert r["matches"] + r["mismatches"] + r["gaps"] == len(ops) and r["seeds"] >= 100


def test_letters_and_refusals(gpu_ctx):
    from mir_prefer_amd import capi
    seqs, where = C.perfect_region()
    plain, _ = check(gpu_ctx, seqs)
    mixed = [seqs[0].lower().replace("t", "u"), seqs[1].replace("T", "U")]
    assert check(gpu_ctx, mixed)[0] == plain
    other = [seqs[0][:100] + "*" + seqs[0][101:], seqs[1][:120] + "R-" + seqs[1][122:]]
    got, _ = check(gpu_ctx, other)
    assert got and got != plain
    with pytest.raises(capi.MirpError, match="transcript 2: a byte >= 0x80"):
        gpu_ctx.nats_scan([seqs[0], seqs[1][:5].encode() + b"\x80" + seqs[1][6:].encode()])
    assert gpu_ctx.nats_last_stats()["transcripts"] == 0
    # an over-long and an empty transcript are skipped and keep their indices
    rng = random.Random(12)
    padded = ["", seqs[0], C.rand_seq(rng, R.MAX_LEN + 1), seqs[1]]
    got, stats = check(gpu_ctx, padded)
    assert [(r["a"], r["b"]) for r in got] == [(1, 3)] and stats["skipped"] == 2 and stats["bases"] == len(seqs[0]) + len(seqs[1])
    # nothing to find, nothing to search
    got, stats = check(gpu_ctx, [C.rand_seq(rng, 200), C.rand_seq(rng, 200)])
    assert got == [] and stats["regions"] == 0
    for empty in ([], [""], ["ACGT"], ["N" * 50, "N" * 50]):
        got, stats = check(gpu_ctx, empty)
        assert got == [] and stats["seed_hits"] == 0
    for bad in (dict(seed=11), dict(seed=25), dict(band=48), dict(max_occ=0), dict(max_occ=10001), dict(min_seeds=0), dict(match=0), dict(mismatch=11),
                dict(gap=51), dict(min_score=0), dict(min_length=0)):
        with pytest.raises(capi.MirpError, match="bad options"):
            gpu_ctx.nats_scan(seqs, **bad)


def test_passes_of_one_transcript_and_one_candidate(gpu_ctx):
    seqs, o = C.seeded_inputs(29)
    seqs = seqs + C.two_copies_in_b()[0]
    o.update(min_score=10, min_length=5)
    want = R.find(seqs, **o)
    _, whole = check(gpu_ctx, seqs, want=want, **o)
    assert whole["join_passes"] == 1 and whole["trace_passes"] == 1 and whole["above"] >= 4
    _, single = check(gpu_ctx, seqs, want=want, capacity=16, **o)
    assert single["trace_passes"] == whole["above"] and single["join_passes"] > 2
    _, between = check(gpu_ctx, seqs, want=want, capacity=16 * 40, **o)
    assert 1 < between["join_passes"] < single["join_passes"]


def test_shuffled_transcripts(gpu_ctx):
    rng = random.Random(77)
    seqs = [C.rand_seq(rng, rng.randint(150, 300)) for _ in range(8)]
    for a, b, at_a, at_b in ((0, 5, 20, 40), (2, 3, 60, 10), (1, 7, 5, 90), (4, 6, 80, 80)):
        seqs[a], seqs[b] = C.plant(rng, seqs[a], at_a, seqs[b], at_b, C.rand_seq(rng, 45))
    o = dict(seed=12, band=32, min_score=100, min_length=40)
    straight, _ = check(gpu_ctx, seqs, **o)
    assert len(straight) == 4
    order = list(range(8))
    rng.shuffle(order)
    moved, _ = check(gpu_ctx, [seqs[k] for k in order], **o)
    def sides(recs, back):
        out = []
        for r in recs:
            x = (back[r["a"]], r["a_start"], r["a_end"])
            y = (back[r["b"]], r["b_start"], r["b_end"])
            out.append((min(x, y), max(x, y), r["score"], r["seeds"], r["bin"]))
        return sorted(out)
    assert sides(moved, order) == sides(straight, list(range(8)))


def test_the_command(tmp_path):
    seqs, where = C.perfect_region()
    fa, fb = tmp_path / "a.fa", tmp_path / "b.fa"
    fa.write_text(">first one\n%s\n%s\n" % (seqs[0][:150], seqs[0][150:]))
    fb.write_text(">second\n%s\n" % seqs[1])
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *args: subprocess.run([sys.executable, "-m", "mir_prefer_amd.nats"] + list(args), cwd=str(tmp_path), capture_output=True, timeout=300, env=env)
    r = run(str(fa), str(fb))
    assert r.returncode == 0, r.stderr
    want, stats = R.find(seqs)
    names = ["first", "second"]
    base = str(fa) + ".nats"
    assert open(base + ".tsv").read() == R.tsv_text(names, want) and open(base + ".pairs.tsv").read() == R.pairs_text(names, want)
    assert open(base + ".bed").read() == R.bed_text(names, want)
    assert r.stderr.decode().startswith("nats: 2 transcripts, 0 skipped, 580 bases, 0 k-mer values ignored, 105 seed hits, 1 candidates, 1 kept, %d cells, "
                                        "1 at or above the score, 1 traced, 1 regions, 1 pairs; written to " % stats["cells"])
    r = run("-o", "out", "-s", "400", str(fa), str(fb))
    assert r.returncode == 0 and open(tmp_path / "out.tsv").read() == R.TSV_HEADER and open(tmp_path / "out.pairs.tsv").read() == R.PAIRS_HEADER
    assert open(tmp_path / "out.bed").read() == ""
    # a refused input leaves no file, not even an earlier run's; option errors exit with 2
    fc = tmp_path / "c.fa"
    fc.write_text(">second\nACGT\n")
    r = run("-o", "out", str(fa), str(fb), str(fc))
    assert r.returncode == 255 and r.stderr.startswith(b"Error: ") and b"occurs twice" in r.stderr
    assert not any(os.path.exists(str(tmp_path / ("out" + ext))) for ext in (".tsv", ".pairs.tsv", ".bed"))
    fd = tmp_path / "d.fa"
    fd.write_bytes(b">third\nAC\xc3GT\n")
    r = run(str(fa), str(fd))
    assert r.returncode == 255 and b"d.fa" in r.stderr and b"0x80" in r.stderr and not os.path.exists(base + ".tsv")
    assert run("--band", "48", str(fa)).returncode == 2
