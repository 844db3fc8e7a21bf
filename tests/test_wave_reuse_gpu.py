"""GPU tests of the second and later jobs a resident wave serves in the wave-per-job kernels (duplex_kernel, unpaired_kernel, hp_score_kernel,
homolog_eval_kernel).  Each of them gives a workgroup or wave a private slab and lets it serve several jobs in turn
without clearing the slab as a whole; the other test files never give one launch more jobs than it has slots.  Here every case makes one call so
large that every slot serves at least three jobs, which the call's own record says (capi.Context.last_jobs_per_slot), ordered so that a slot goes
from its largest, most strongly bound job to its smallest and then to mixed ones.  The truth comes twice: (a) the plain restatement of the
operation on a seeded sample of the jobs, with the tolerance its own test file uses, and (b) bit or byte equality of all jobs with the same jobs
run through the capacity knobs in passes so small that no slot serves two -- the configuration the other test files pin to the restatements.
The slot counts named below are those of a device with 256 compute units, and every large call asserts the exact ceil(jobs / slots) they give;
with more slots a call whose slots no longer serve three jobs each in the planned order fails on that assertion, it does not pass vacuously.  Further: the 15-bit score fields of the hairpin scoring at their limit (match = 10 at 3,000 nt) and the hand-over of the unpaired
slab from LDS to device memory, every length around it.  The restatements run in worker processes that are started fresh (spawn), never forked
from a process that holds a device context."""
import multiprocessing
import random
import time

import numpy as np
import pytest

from mir_prefer_amd import homologs
from tests import homolog_restatement as hr
from tests.test_duplex_cpu import duplex, fmt_mfe, near_complement, random_strand, seeded_pairs, target_strand
from tests.test_ensemble_cpu import planted_hairpin, random_seq
from tests.test_hairpins_cpu import as_records, restate
from tests.test_targets_bulge_cpu import plant_bulged
from tests.test_targets_cpu import ACGT, load_reference, plant, random_mirnas, write_fasta
from tests.test_unpaired_cpu import format_upe, site_window, upe_job

pytestmark = pytest.mark.gpu
DUPLEX, UNPAIRED, HAIRPIN, HOMOLOG = 0, 1, 2, 3          # the families of mirp_last_jobs_per_slot
DX_FIELDS = ("mfe", "pairs", "a_first", "a_last", "b_first", "b_last")
UP_FIELDS = ("efe", "efe_open", "upe")
UP_TOL = 1e-8                                            # kcal/mol (as tests/test_unpaired_gpu.py)


def duplex_job(pair):
    return duplex(*pair)


@pytest.fixture(scope="module")
def pool():
    with multiprocessing.get_context("spawn").Pool(14) as p:
        yield p


def first_differences(a, b, limit=5):
    """the first few indices at which two sequences of equal length differ (an assertion on them prints little, however long the sequences)"""
    assert len(a) == len(b)
    return [k for k, (x, y) in enumerate(zip(a, b)) if x != y][:limit]


def bits(values):
    return np.ascontiguousarray(values).view(np.uint64)


def tiled(rng, distinct, n):
    """n jobs drawn from the distinct ones, every one of them used"""
    picks = list(range(len(distinct))) + [rng.randrange(len(distinct)) for _ in range(n - len(distinct))]
    rng.shuffle(picks)
    return [distinct[k] for k in picks]


# ---------------------------------------------------------------------------------------------------- duplex
DX_SLOTS = 32768          # min(ceil(n / 4), 32 x 256 CUs) blocks of 4 waves; wave s serves the pairs s, s + 32768, ...
DX_PAIRS = 100000
assert 3 * DX_SLOTS <= DX_PAIRS < 4 * DX_SLOTS


def duplex_pairs():
    """Block 1 (a wave's first pair): 64 x 64 G/C-rich near-complements.  Block 2: strands of 1..12 nt, among them la = 1, lb = 1 and pairs that
    cannot bind.  The rest: seeded pairs as the other duplex tests fold them."""
    rng = np.random.RandomState(2101)
    pick = random.Random(2102)
    big = []
    for _ in range(512):
        a = random_strand(rng, 64, "GGGCCCAU")
        big.append((a, (near_complement(rng, a, edits=4, flank=0) + random_strand(rng, 64, "GC"))[:64]))
    small = [("A", "U"), ("G", "C"), ("AAAA", "AAAA"), ("G", "CCCCCCCCCCCC"), ("GGGGGGGGGGGG", "C"), ("NNNN", "NNNN"), ("GGGG", "CCCC")]
    for k in range(1017):
        a = random_strand(rng, int(rng.randint(1, 13)), "GCAU" if k % 3 else "AC")
        small.append((a, near_complement(rng, a, edits=1, flank=1)[:12] if k % 2 else random_strand(rng, int(rng.randint(1, 13)), "AC" if k % 3 == 0 else "ACGU")))
    mixed = seeded_pairs(2103, 4096)
    return tiled(pick, big, DX_SLOTS) + tiled(pick, small, DX_SLOTS) + tiled(pick, mixed, DX_PAIRS - 2 * DX_SLOTS)


def test_duplex_waves_serve_three_pairs(gpu_ctx, pool):
    pairs = duplex_pairs()
    assert len(pairs) == DX_PAIRS >= 3 * DX_SLOTS and all(len(a) == 64 == len(b) for a, b in pairs[:DX_SLOTS])
    assert all(1 <= len(a) <= 12 and 1 <= len(b) <= 12 for a, b in pairs[DX_SLOTS:2 * DX_SLOTS])
    a_list, b_list = [a for a, _ in pairs], [b for _, b in pairs]
    t = time.time()
    recs, ss = gpu_ctx.duplex_batch(a_list, b_list)
    wall = time.time() - t
    launches, per_slot = gpu_ctx.last_jobs_per_slot(DUPLEX)
    stats = gpu_ctx.duplex_last_stats()
    print("duplex: %d pairs in one launch, %d per wave, %.2f s; %d loop evaluations" % (len(pairs), per_slot, wall, stats["evaluations"]))
    assert launches == 1 and per_slot == 4 == -(-DX_PAIRS // DX_SLOTS) and stats["passes"] == 1          # 3 full rounds of the waves and a part of a fourth
    # (b) passes of 4,096 pairs: 1,024 blocks, every wave serves one pair
    base, ss0 = gpu_ctx.duplex_batch(a_list, b_list, capacity=4096)
    assert gpu_ctx.last_jobs_per_slot(DUPLEX) == ((DX_PAIRS + 4095) // 4096, 1)
    assert first_differences(recs.tolist(), base.tolist()) == [] and first_differences(ss, ss0) == []
    assert gpu_ctx.duplex_last_stats()["evaluations"] == stats["evaluations"] > 0
    # what the blocks hold: strongly bound pairs first, unbound ones among a wave's second pairs
    assert (recs["mfe"][:DX_SLOTS] < -3000).all() and (recs["mfe"][DX_SLOTS:2 * DX_SLOTS] == 0).sum() > 5000
    assert (recs["mfe"][DX_SLOTS:2 * DX_SLOTS] < 0).sum() > 5000
    # (a) the restatement of a seeded sample of every block
    rng = random.Random(2104)
    sample = rng.sample(range(DX_SLOTS), 30) + rng.sample(range(DX_SLOTS, 2 * DX_SLOTS), 120) + rng.sample(range(2 * DX_SLOTS, DX_PAIRS), 150)
    want = pool.map(duplex_job, [pairs[q] for q in sample], chunksize=2)
    for q, w in zip(sample, want):
        assert tuple(int(recs[q][f]) for f in DX_FIELDS) == tuple(w[f] for f in DX_FIELDS), (q, pairs[q], recs[q], w)
        assert ss[q] == w["structure"], (q, pairs[q], ss[q], w["structure"])


# ---------------------------------------------------------------------------------------------------- unpaired
def intervals_of(n):
    """first base, last base, the whole window, a single base inside, four bases a quarter in, 21 bases from the middle on"""
    return [(1, 1), (n, n), (1, n), ((n + 1) // 2, (n + 1) // 2), (n // 4 + 1, min(n, n // 4 + 4)), (n // 2, min(n, n // 2 + 20))]


def unpaired_windows(seed, lo, hi, slots, n):
    """n windows of lo..hi nt in the order a block meets them (block b serves the windows b, b + slots, ...): first the longest length with a
    G/C-rich planted hairpin, then the shortest length, every other one unable to pair, then mixed lengths, planted hairpins and random letters,
    every tenth with N; the intervals go round intervals_of."""
    rng = random.Random(seed)
    out = []
    for q in range(n):
        if q < slots:
            s = planted_hairpin(rng, hi, "GGCCAU", edits=1)
        elif q < 2 * slots:
            s = random_seq(rng, lo, "AC") if q % 2 else planted_hairpin(rng, lo)
        else:
            L = rng.randint(lo, hi)
            s = planted_hairpin(rng, L) if q % 3 else random_seq(rng, L)
            if q % 10 == 9:
                t = list(s)
                for _ in range(1 + L // 15):
                    t[rng.randrange(L)] = rng.choice("NRYn")
                s = "".join(t)
        a, b = intervals_of(len(s))[q % 6]
        out.append((s, a, b))
    return out


def run_unpaired(ctx, jobs, **kw):
    return ctx.unpaired_batch([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], **kw)


def compare_unpaired(jobs, recs, want, label):
    worst = dict.fromkeys(UP_FIELDS, 0.0)
    for r, w in zip(recs, want):
        for f in UP_FIELDS:
            worst[f] = max(worst[f], abs(float(r[f]) - w[f]))
    print("%s: %d windows restated, largest deviations %s kcal/mol" % (label, len(jobs), ", ".join("%s %.3g" % (f, worst[f]) for f in UP_FIELDS)))
    for j, r, w in zip(jobs, recs, want):
        for f in UP_FIELDS:
            assert abs(float(r[f]) - w[f]) <= UP_TOL, (j, f, float(r[f]), w[f])


# (lengths, blocks of the launch on 256 CUs, windows).  17..24 nt: a block's LDS is 20,832 bytes, 7 blocks a CU are resident and twice as many are
# launched; 49..56 nt: the largest LDS slab, 2 x 256 x 2 blocks; 57..64 nt: the slab in device memory, 4 x 256 blocks.
UNPAIRED_CASES = {"lds_24": (17, 24, 3584, 11000), "lds_56": (49, 56, 1024, 3100), "global_64": (57, 64, 1024, 3100)}


@pytest.mark.parametrize("case", sorted(UNPAIRED_CASES))
def test_unpaired_blocks_serve_three_windows(gpu_ctx, pool, case):
    lo, hi, slots, n = UNPAIRED_CASES[case]
    longest = gpu_ctx.unpaired_lds_longest()          # 56 nt by DESIGN.md §24
    assert (hi <= longest) == case.startswith("lds") and (case != "lds_56" or hi == longest) and (case != "global_64" or lo == longest + 1)
    jobs = unpaired_windows(2400 + hi, lo, hi, slots, n)
    assert 3 * slots <= n < 4 * slots and {len(j[0]) for j in jobs[2 * slots:]} == set(range(lo, hi + 1)) and sum("N" in j[0].upper() for j in jobs) > n // 50
    t = time.time()
    recs = run_unpaired(gpu_ctx, jobs)
    wall = time.time() - t
    launches, per_slot = gpu_ctx.last_jobs_per_slot(UNPAIRED)
    print("unpaired %s: %d windows in one launch, %d per block, %.3f s" % (case, n, per_slot, wall))
    assert launches == 1 and per_slot == 4 == -(-n // slots) and gpu_ctx.unpaired_last_stats()["passes"] == 1          # 3 full rounds of the blocks and a part of a fourth
    # (b) passes of 512 windows: a block each (a window's three doubles depend on nothing but the window)
    base = run_unpaired(gpu_ctx, jobs, capacity=512)
    assert gpu_ctx.last_jobs_per_slot(UNPAIRED) == ((n + 511) // 512, 1)
    for f in UP_FIELDS:
        assert np.nonzero(bits(recs[f]) != bits(base[f]))[0].tolist()[:5] == [], (case, f)
    assert (recs["efe"][:slots] < -2.0).sum() > 0.8 * slots and (recs["efe"][slots:2 * slots] == 0.0).sum() > slots // 4          # strongly bound first, then windows that cannot pair
    # (a) the masked restatement of a seeded sample of every block
    rng = random.Random(2450 + hi)
    sample = rng.sample(range(slots), 8) + rng.sample(range(slots, 2 * slots), 8) + rng.sample(range(2 * slots, n), 24)
    picked = [jobs[q] for q in sample]
    compare_unpaired(picked, recs[sample], pool.map(upe_job, picked, chunksize=1), case)


def test_unpaired_slab_hand_over(gpu_ctx, pool):
    """every length from 8 below to 8 above the longest window of the LDS slab, a planted hairpin each with two intervals, all restated"""
    longest = gpu_ctx.unpaired_lds_longest()          # 56 nt by DESIGN.md §24
    rng = random.Random(2470)
    jobs = []
    for L in range(longest - 8, longest + 9):
        s = planted_hairpin(rng, L)
        jobs += [(s, 1, L // 3), (s, L // 2, min(L, L // 2 + 20))]
    recs = run_unpaired(gpu_ctx, jobs)
    assert gpu_ctx.last_jobs_per_slot(UNPAIRED) == (3, 1)          # the classes below the longest, the longest, 8 above: a block each window
    compare_unpaired(jobs, recs, pool.map(upe_job, jobs, chunksize=1), "hand-over %d..%d nt" % (longest - 8, longest + 8))
    assert (recs["efe"] < -3.0).sum() >= 24 and (recs["upe"] > 0.5).sum() >= 17
    alone = run_unpaired(gpu_ctx, jobs, capacity=1)                # the same bits window by window
    for f in UP_FIELDS:
        assert np.nonzero(bits(alone[f]) != bits(recs[f]))[0].tolist() == [], f


# ---------------------------------------------------------------------------------------------------- targets -e -u end to end
def test_targets_energy_and_accessibility_over_100000_keys(gpu_ctx, pool, tmp_path):
    """9,000 miRNAs drawn from 300 sequences, each of which has 14 ungapped and 4 bulged sites planted: more than 100,000 keys in one pass, so that
    every wave of the duplex kernel serves 3 of them and every block of the accessibility kernel about 100; -k 6 cuts more than half of them
    inside the kernels.  The file is the one that passes of 1,000 keys write, in which no wave serves two."""
    rng = np.random.RandomState(2480)
    base = random_mirnas(rng, 300, 18, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 800000)].tobytes())
    for m in base:
        plant(rng, text, m, 14, subs=(0, 2))
        plant_bulged(rng, text, m, 4, subs=(0, 1))
    text[1000:1030] = b"N" * 30
    write_fasta(tmp_path / "t.fa", [("a", bytes(text[:300000])), ("b", bytes(text[300000:]))])
    pick = rng.randint(0, 300, 9000)
    (tmp_path / "m.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, base[p]) for i, p in enumerate(pick)))
    kw = dict(bulge=True, energy=True, accessibility=True, both_strands=True)

    def scan(name, **more):
        out = tmp_path / name
        res = gpu_ctx.target_scan(str(tmp_path / "m.fa"), [str(tmp_path / "t.fa")], str(out), **kw, **more)
        return out.read_bytes(), res, gpu_ctx.last_jobs_per_slot(DUPLEX), gpu_ctx.last_jobs_per_slot(UNPAIRED)
    uncut, res_all, _, _ = scan("uncut.tsv")
    keys = res_all["sites"]
    t = time.time()
    whole, res, dx, up = scan("whole.tsv", max_sites=6)
    wall = time.time() - t
    print("targets -e -u: %d keys, %d lines after -k 6, %d pass, %.2f s; duplex %s, unpaired %s (launches, jobs per slot)" % (
        keys, res["sites"], res["passes"], wall, dx, up))
    assert keys >= 100000 and res["passes"] == 1 and res["sites"] == whole.count(b"\n") - 1 < 0.5 * keys          # more than half are cut in the kernels
    assert dx[1] == -(-keys // DX_SLOTS) >= 4 and up[1] == -(-keys // 1024) and dx[0] == 2 and up[0] == 1          # duplex: the perfect duplexes of the group, then the keys
    assert len(set(whole.split(b"\n")) - set(uncut.split(b"\n"))) == 0
    try:
        gpu_ctx.set_target_capacity(1000)
        split, res1, dx1, up1 = scan("split.tsv", max_sites=6)
    finally:
        gpu_ctx.set_target_capacity(0)
    assert res1["passes"] > 30 and dx1[1] == 1 and up1[1] == 1 and dx1[0] > 30 and up1[0] > 30
    split_lines, whole_lines = split.split(b"\n"), whole.split(b"\n")
    assert len(split_lines) == len(whole_lines) and first_differences(split_lines, whole_lines) == []          # byte-equal files
    # 200 sampled lines: the columns against the batch calls and against the restatements
    names, seqs = load_reference([tmp_path / "t.fa"])
    contigs = {b"a": bytes(text[:300000]), b"b": bytes(text[300000:])}
    rows = [ln.split(b"\t") for ln in whole.split(b"\n")[1:-1]]
    assert whole.split(b"\n")[0].split(b"\t")[11:] == [b"bulge", b"mfe", b"mfe_perfect", b"mfe_ratio", b"duplex", b"upe"]
    sample = [rows[k] for k in random.Random(2481).sample(range(len(rows)), 200)]
    assert {f[4] for f in sample} == {b"+", b"-"} and sum(f[11] != b"." for f in sample) >= 5
    pairs = [(f[8].replace(b"-", b"").decode(), target_strand(seqs[names.index(f[1].decode())], int(f[2]) - 1, int(f[3]), f[4] == b"-")) for f in sample]
    wins = [site_window(contigs[f[1]], int(f[2]), int(f[3]), f[4].decode()) for f in sample]
    recs, ss = gpu_ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs])
    assert [f[12] for f in sample] == [fmt_mfe(int(e)) for e in recs["mfe"]] and [f[15] for f in sample] == ss
    urecs = gpu_ctx.unpaired_batch([w for w, _, _ in wins], [lo for _, lo, _ in wins], [hi for _, _, hi in wins])
    assert [f[16].decode() for f in sample] == [format_upe(float(u)) for u in urecs["upe"]]
    for f, p, w in zip(sample, pairs, pool.map(duplex_job, pairs, chunksize=4)):
        assert f[12] == fmt_mfe(w["mfe"]) and f[15] == w["structure"], (f, p, w)
    for f, j, r in zip(sample, wins, pool.map(upe_job, wins, chunksize=1)):
        x = r["upe"] * 1000
        assert abs(x - np.floor(x) - 0.5) >= 1e-6, ("a restated upe at a rounding boundary of the third decimal: take another sample seed", j, r)
        assert f[16].decode() == format_upe(r["upe"]), (f, j, r)


# ---------------------------------------------------------------------------------------------------- hairpin scoring
HP_PAR = (2, 3, 5, 2)
HP_MIN_SCORE = 32          # an exact copy of a 16-nt query; above what two random sequences of these lengths reach, but for a handful
HP_CHUNK = 3          # queries a block of the scoring kernel serves in turn in the large call (252 queries over the 92 rows the boundary buffers allow)


def hairpin_input():
    """252 queries of 16..90 nt (1 to 6 strips) and 4,096 known sequences of 300..400 nt, 82 of which hold a copy of a query, one with substitutions,
    one with an insertion or a deletion, or one extended on both sides.  The strip counts are seeded shuffles of 1..6, six queries at a time, so
    that odd and even counts stand side by side in no fixed relation to a block's run of HP_CHUNK queries; the 82 queries go round the 18
    combinations of (place in the run, strip count) and the kind of copy is drawn independently; -> (queries, known, indices of those 82, their
    queries)"""
    rng = random.Random(2500)
    queries, strips = [], []
    for k in range(42):
        strips += rng.sample(range(1, 7), 6)
    for s in strips:
        queries.append(random_seq(rng, 16 if s == 1 else rng.randint(16 * (s - 1) + 1, min(16 * s, 90))))
    known = [random_seq(rng, rng.randint(300, 400)) for _ in range(4096)]
    planted = sorted(rng.sample(range(4096), 82))
    cells = {}
    for k, s in enumerate(strips):
        cells.setdefault((k % HP_CHUNK, s), []).append(k)
    assert len(cells) == 6 * HP_CHUNK
    for c in cells.values():
        rng.shuffle(c)
    sources = [cells[c][n // len(cells)] for n, c in zip(range(82), sorted(cells) * 5)]
    for x, source in zip(planted, sources):
        q = queries[source]
        kind = rng.randrange(4)
        if kind == 1 and len(q) > 20:
            t = list(q)
            for _ in range(rng.randint(1, len(q) // 12)):
                t[rng.randrange(len(t))] = rng.choice("ACGU")
            q = "".join(t)
        elif kind == 2 and len(q) > 30:
            at, g = rng.randrange(8, len(q) - 8), rng.randint(1, 3)
            q = q[:at] + random_seq(rng, g) + q[at:] if rng.random() < 0.5 else q[:at] + q[at + g:]
        elif kind == 3:
            q = q + q[:rng.randint(1, 12)]
        at = rng.randrange(0, len(known[x]) - len(q))
        known[x] = known[x][:at] + q + known[x][at + len(q):]
    return queries, known, planted, sources


def align(ctx, queries, known, par=HP_PAR, min_score=HP_MIN_SCORE):
    recs, cigars = ctx.hairpin_align(queries, known, match=par[0], mismatch=par[1], gap_open=par[2], gap_extend=par[3], min_score=min_score)
    return [tuple(r) for r in recs.tolist()], cigars


def test_hairpin_scoring_blocks_serve_three_queries(gpu_ctx):
    queries, known, planted, sources = hairpin_input()
    assert {(len(q) + 15) // 16 for q in queries} == {1, 2, 3, 4, 5, 6} and min(map(len, queries)) == 16 and max(map(len, queries)) <= 90
    t = time.time()
    recs, cigars = align(gpu_ctx, queries, known)
    wall = time.time() - t
    launches, chunk = gpu_ctx.last_jobs_per_slot(HAIRPIN)
    stats = gpu_ctx.hairpin_last_stats()
    print("hairpin scoring: %d queries x %d known, %d queries per block, %.2f s; %d hits" % (len(queries), len(known), chunk, wall, len(recs)))
    assert launches == 1 and chunk == HP_CHUNK and stats["score_passes"] == 1
    hit_known = {r[1] for r in recs}
    assert len(recs) >= 60 and len(hit_known & set(planted)) >= 60 and len(hit_known - set(planted)) <= 10          # (a chance hit is compared as any other)
    # where the true hits fall: on the first, second and third query of a block's run, after and on every strip count, with gaps and mismatches
    true_hits = [(r, c) for r, c in zip(recs, cigars) if (r[0], r[1]) in set(zip(sources, planted))]
    cover = {(r[0] % chunk, (len(queries[r[0]]) + 15) // 16) for r, _ in true_hits}
    print("true hits %d, (place in the run, strips) covered: %s" % (len(true_hits), sorted(cover)))
    assert cover == {(p, s) for p in range(chunk) for s in range(1, 7)}
    for place in range(1, chunk):          # a later query of a run, hit after a query of an odd and of an even strip count, with a gapped and a mismatched cigar
        later = [(r, c) for r, c in true_hits if r[0] % chunk == place]
        assert {((len(queries[r[0] - 1]) + 15) // 16) % 2 for r, _ in later} == {0, 1}, place
        assert any("I" in c or "D" in c for _, c in later) and any("X" in c for _, c in later), place
    # (b) calls of 40 queries: a block each
    again, again_cigars, per_query = [], [], []
    for q0 in range(0, len(queries), 40):
        r, c = align(gpu_ctx, queries[q0:q0 + 40], known)
        assert gpu_ctx.last_jobs_per_slot(HAIRPIN) == (1, 1)
        again += [(x[0] + q0,) + x[1:] for x in r]
        again_cigars += c
        per_query += gpu_ctx.hairpin_last_stats()["per_query"]
    assert len(again) == len(recs) and first_differences(list(zip(again, again_cigars)), list(zip(recs, cigars))) == [] and per_query == stats["per_query"]
    # (a) 30 queries against the planted known sequences, pair by pair
    pick = random.Random(2501)
    some = sorted(set(pick.sample(sources, 20)) | set(pick.sample(sorted(set(range(len(queries))) - set(sources)), 10)))
    hits, _ = restate([queries[k] for k in some], [known[x] for x in planted], HP_PAR, HP_MIN_SCORE)
    w_recs, w_cigars = as_records(hits)
    want = [((some[r[0]], planted[r[1]]) + r[2:], c) for r, c in zip(w_recs, w_cigars)]
    got = [(r, c) for r, c in zip(recs, cigars) if r[0] in set(some) and r[1] in set(planted)]
    assert len(some) == 30 and len(want) >= 15 and got == want


def test_hairpin_score_fields_at_their_limit(gpu_ctx):
    """The score lives in 15-bit fields (the strip key, the filter key, the halves of the carry word): match = 10 at 3,000 nt is 30,000."""
    par = (10, 10, 20, 10)
    recs, cigars = align(gpu_ctx, ["A" * 3000], ["A" * 3000, "A" * 2999 + "C"], par, 1)
    assert [(r[0], r[1], r[2]) + r[3:7] for r in recs] == [(0, 0, 30000, 1, 3000, 1, 3000), (0, 1, 29990, 1, 2999, 1, 2999)]
    assert cigars == ["3000=", "2999="]
    rng = random.Random(3001)          # a noisy pair as test_hairpins_gpu.test_long builds it
    q = random_seq(rng, 3000)
    s = list(q)
    for _ in range(30):
        s[rng.randrange(3000)] = rng.choice("ACGU")
    s = "".join(s)
    for _ in range(5):
        at, g = rng.randrange(100, 2800), rng.randint(1, 6)
        s = s[:at] + random_seq(rng, g) + s[at:] if rng.random() < 0.5 else s[:at] + s[at + g:]
    s = (s + random_seq(rng, 3000))[:3000]
    hits, per_query = restate([q], [s, "G"], par, 1)
    w_recs, w_cigars = as_records(hits)
    recs, cigars = align(gpu_ctx, [q], [s, "G"], par, 1)
    assert recs == w_recs and cigars == w_cigars and gpu_ctx.hairpin_last_stats()["per_query"] == per_query
    assert recs[0][2] > 16384 and recs[0][9] >= 4          # bit 14 of every field is in use; gaps were opened


# ---------------------------------------------------------------------------------------------------- homolog evaluation
HM_COPIES, HM_SPACING, HM_CONTIGS = 680, 300, 5
HM_SLOTS = 8192          # min(windows, 32 x 256 CUs) blocks of the evaluation kernel


def homolog_genome():
    """25 planted precursors (hr.planted_hairpin, the known sequence an exact stretch of the arm), the longest first, each copied 680 times on
    either strand, 300 nt apart in random order over 5 contigs, every copy with up to 3 substitutions outside the site and up to 2 inside it:
    17,000 placements within 2 mismatches, and about 0.7 times as many again where the other arm, read on the other strand, is within 2
    mismatches as well.  -> (contigs, queries, the 17,000 placements [(query, contig, 0-based offset, strand, mismatches)])"""
    rng = random.Random(2600)
    nrng = np.random.RandomState(2601)
    pre = sorted((hr.planted_hairpin(rng, 0) for _ in range(25)), key=lambda x: -len(x[0]))
    assert len({k for _, k, _ in pre}) == 25
    n = 25 * HM_COPIES
    per = (n + HM_CONTIGS - 1) // HM_CONTIGS
    contigs = [bytearray(b"ACGT"[c] for c in nrng.randint(0, 4, per * HM_SPACING + 400).tolist()) for _ in range(HM_CONTIGS)]
    order = [q for q in range(25) for _ in range(HM_COPIES)]
    rng.shuffle(order)
    placements = []
    for slot, q in enumerate(order):
        hp, known, off = pre[q]
        ci, at = slot // per, 200 + (slot % per) * HM_SPACING
        t = list(hp)
        inside = rng.sample(range(off, off + 21), rng.randint(0, 2))
        outside = [p for p in rng.sample(range(len(hp)), rng.randint(0, 3)) if not off <= p < off + 21]
        for p in inside + outside:
            t[p] = rng.choice([c for c in "ACGT" if c != t[p]])
        t = "".join(t)
        strand = rng.randrange(2)
        contigs[ci][at:at + len(t)] = (hr.revcomp(t) if strand else t).encode()
        placements.append((q, ci, at + (len(t) - off - 21 if strand else off), strand, len(inside)))
    return [("chr%d" % (i + 1), c.decode()) for i, c in enumerate(contigs)], [(k, ["pln-miR%d" % (i + 1)]) for i, (_, k, _) in enumerate(pre)], placements


def test_homolog_evaluation_blocks_serve_three_windows(gpu_ctx, tmp_path):
    contigs, queries, placements = homolog_genome()
    path = str(tmp_path / "genome.fa")
    hr.write_fasta(path, contigs)
    gpu_ctx.align_index([path])
    names, _ = gpu_ctx.align_contigs()
    kw = dict(max_mismatches=2, precursor_len=300, max_placements=2 * HM_COPIES)
    t = time.time()
    recs, text, also = gpu_ctx.homolog_scan([q for q, _ in queries], **kw)
    wall = time.time() - t
    launches, per_slot = gpu_ctx.last_jobs_per_slot(HOMOLOG)
    stats = gpu_ctx.homolog_last_stats()
    print("homolog evaluation: %d placements in %d chunk, %d launches, %d windows per block, %.2f s; %d loci" % (
        stats["placements"], stats["chunks"], launches, per_slot, wall, stats["loci"]))
    assert stats["placements"] >= 25000 and stats["placements"] > len(placements) == 25 * HM_COPIES and stats["chunks"] == 1 and stats["repeat_like"] == 0
    assert launches >= 1 and per_slot == -(-stats["placements"] // HM_SLOTS) and stats["placements"] >= 3 * HM_SLOTS
    assert 2000 <= stats["loci"] and stats["passing"] < stats["placements"]          # windows with and without a passing structure
    # (b) chunks of 4,096 placements: a block each
    recs1, text1, also1 = gpu_ctx.homolog_scan([q for q, _ in queries], chunk=4096, **kw)
    stats1 = gpu_ctx.homolog_last_stats()
    assert gpu_ctx.last_jobs_per_slot(HOMOLOG)[1] == 1 and stats1["chunks"] == (stats["placements"] + 4095) // 4096
    assert len(recs) == len(recs1) and first_differences(recs.tolist(), recs1.tolist()) == []
    assert (text == text1, also.tobytes() == also1.tobytes()) == (True, True)
    varying = ("chunks", "folds", "eval_reruns", "seconds")
    assert {k: v for k, v in stats.items() if k not in varying} == {k: v for k, v in stats1.items() if k not in varying}
    # (a) 60 sampled placements against the restatement: the locus at the placement's interval, or none
    loci = {(x["contig"], x["strand"], x["mat_s"], x["mat_e"]): x for x in homologs.loci_of(recs, text, also, queries, names)}
    assert len(loci) == len(recs)
    passing = 0
    for q, ci, o, strand, mm in random.Random(2602).sample(placements, 60):
        ws, we, letters = hr.window_of(contigs[ci][1], o, 21, 300, strand)
        best, _ = hr.evaluate(letters, 300, o + 1, o + 22, ws, we, strand)
        got = loci.get((contigs[ci][0], "+-"[strand], o + 1, o + 22))
        if best is None:
            assert got is None, (q, ci, o, strand, got)
            continue
        passing += 1
        st, ms = best
        cut = lambda a, b: homologs.interval(letters, ws, we, strand, a, b)
        assert got == {"names": list(queries[q][1]), "contig": contigs[ci][0], "strand": "+-"[strand], "mat_s": o + 1, "mat_e": o + 22, "mature": cut(o + 1, o + 22),
                       "mismatches": mm, "arm": "5p" if ms.prime5 else "3p", "star_s": ms.star_s, "star_e": ms.star_e, "star": cut(ms.star_s, ms.star_e),
                       "fold_s": ms.fold_s, "fold_e": ms.fold_e, "precursor": cut(ms.fold_s, ms.fold_e), "energy": st[4], "line_len": st[5],
                       "total_bps": ms.total_bps, "total_dots": ms.total_dots, "ss": st[2], "also": []}, (q, ci, o, strand)
    assert 10 <= passing
