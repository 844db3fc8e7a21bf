"""GPU tests of the degradome (PARE) cleavage scan (mirp_degradome_scan, degradome_kernels.hip): whole TSV files against both
restatements of tests/test_degradome_cpu.py over a sweep of -s / -c / --max-category / -p on three SAM files with gapped, flagged and minus-strand
records and an @SQ order that differs from the FASTA order; every hit against mirp_target_scan on the same files; one position with 2 M records whose
sum passes 2^32; one transcript with 10^6 units next to 10^5 transcripts with one unit each; transcripts that end on and next to 32-base word
boundaries; forced key capacities; the command line and its refusals; and the chain trim -> reads collapse -> align -> degradome."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mir_prefer_amd import degradome
from mir_prefer_amd.synth import ALN_DTYPE
from tests.test_align_cpu import CODE
from tests.test_clusters_gpu import write_sams
from tests.test_degradome_cpu import (HEADER, STAT_KEYS, Case, _rows, make_records, prepare_numpy, prepare_plain, restate_numpy, restate_plain,
                                      seeded_case)
from tests.test_targets_cpu import ACGT, ROOT, parse_mirnas, random_mirnas, target_of_mirna, write_fasta

pytestmark = pytest.mark.gpu

# (max half-score, -c, --max-category, -p)
SWEEP = [(10, False, 4, 1.0), (0, False, 4, 1.0), (8, False, 4, 1.0), (16, False, 4, 1.0), (10, True, 4, 1.0), (16, True, 2, 0.05), (10, False, 0, 1.0),
         (10, False, 2, 1.0), (16, False, 4, 0.05), (16, False, 4, 1e-3), (8, True, 0, 1e-3)]


def _scan(ctx, d, case, out=None, **kw):
    out = out or (d / "out.tsv")
    res = ctx.degradome_scan(str(d / "m.fa"), str(d / "t.fa"), str(out), case.sq_names, case.sq_lens, **kw)
    return out.read_bytes(), res


def _kw(half, cleavage, max_category, alpha):
    return (dict(max_half_score=half, cleavage_site=cleavage, max_category=max_category, alpha=alpha),
            dict(max_half=half, cleavage=cleavage, max_category=max_category, alpha=alpha))


def _write_inputs(d, case, texts, mirs):
    write_fasta(d / "t.fa", [(n + " some description", t) for n, t in zip(case.fa_names, texts)])
    (d / "m.fa").write_bytes(b"".join(b">%s\n%s\n" % (n, m) for (n, _), m in zip(case.mirnas, mirs)))


@pytest.fixture(scope="module")
def sweep_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("degradome_sweep")
    case, texts, mirs = seeded_case(7)
    _write_inputs(d, case, texts, mirs)
    rng = np.random.RandomState(70)
    extra = [(int(rng.randint(0, 3)), int(flag), int(rng.randint(0, len(case.sq_names))), int(rng.randint(1, 250)), int(rng.randint(1, 50)), 21)
             for flag in (4, 256, 512, 1024, 4 | 16, 256 | 16) for _ in range(20)]
    paths = [str(d / ("deg%d.sam" % i)) for i in range(3)]
    write_sams(paths, case.sq_names, case.sq_lens, case.recs, extra)
    return d, case, paths


def test_settings_sweep_matches_both_restatements(gpu_ctx, sweep_input):
    d, case, paths = sweep_input
    names, lens, _, alns, _, _ = gpu_ctx.ingest_sams(paths)
    assert names == case.sq_names and lens.tolist() == case.sq_lens and len(alns) == len(case.recs)
    assert case.sq_names != [n for n in case.fa_names if n in set(case.sq_names)]          # the @SQ order is not the FASTA order
    prep = {c: (prepare_plain(case, c), prepare_numpy(case, c)) for c in (False, True)}
    for half, cleavage, max_category, alpha in SWEEP:
        gk, rk = _kw(half, cleavage, max_category, alpha)
        got, res = _scan(gpu_ctx, d, case, **gk)
        want, stats = restate_numpy(case, prep=prep[cleavage][1], **rk)
        assert got == want, (half, cleavage, max_category, alpha)
        assert (got, stats) == restate_plain(case, prep=prep[cleavage][0], **rk), (half, cleavage, max_category, alpha)
        assert {k: res[k] for k in STAT_KEYS} == stats
        assert (res["mirnas"], res["transcripts"], res["bases"]) == (len(case.mirnas), len(case.fa_names), case.P)
        if (half, cleavage, max_category, alpha) == (10, False, 4, 1.0):
            rows = _rows(got)
            assert len(rows) >= 50 and {r[6] for r in rows} == {b"0", b"1", b"2", b"3", b"4"}


def test_hits_are_lines_of_the_target_scan(gpu_ctx, sweep_input, tmp_path):
    d, case, paths = sweep_input
    gpu_ctx.ingest_sams(paths)
    for half, cleavage in ((10, False), (16, True)):
        got, _ = _scan(gpu_ctx, d, case, max_half_score=half, cleavage_site=cleavage)
        gpu_ctx.target_scan(str(d / "m.fa"), [str(d / "t.fa")], str(tmp_path / "targets.tsv"), max_half_score=half, cleavage_site=cleavage)
        lines = [ln.split(b"\t") for ln in (tmp_path / "targets.tsv").read_bytes().split(b"\n")[1:-1]]
        have = {tuple(f[:4] + f[5:]) for f in lines}            # without the strand column
        rows = _rows(got)
        assert len(rows) >= 50
        for r in rows:
            assert tuple(r[:2] + r[3:6] + r[11:]) in have, r
            assert int(r[9]) == sum(1 for f in lines if f[0] == r[0] and float(f[5]) <= float(r[5])), r
            assert int(r[2]) == int(r[4]) - 9


def test_forced_capacities_give_the_same_bytes(gpu_ctx, sweep_input, tmp_path):
    d, case, paths = sweep_input
    gpu_ctx.ingest_sams(paths)
    want, base = _scan(gpu_ctx, d, case, max_half_score=16)
    assert base["hits"] >= 50 and base["passes"] == 1
    try:
        # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change
        for cap, passes in ((2, 63), (40, 4)):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, d, case, out=tmp_path / "cap.tsv", max_half_score=16)
            assert got == want, cap
            assert res["passes"] == passes, (cap, res)
            assert res["passes"] > base["hits"] // max(cap, 1) // 2 and res["hits"] == base["hits"]
    finally:
        gpu_ctx.set_target_capacity(0)


def _load(ctx, recs, n_contigs):
    ctx.load_genome([("c%d" % i, np.full(1, 65, np.uint8)) for i in range(n_contigs)])
    ctx.load_alignments(recs)


def test_one_position_with_2m_records_past_2_32(gpu_ctx, tmp_path):
    rng = np.random.RandomState(11)
    mirs = random_mirnas(rng, 4, 20, 22, t_for_u=0)
    texts = [bytearray(ACGT[rng.randint(0, 4, 900)].tobytes()) for _ in range(3)]
    texts[1][400:400 + len(mirs[0])] = target_of_mirna(mirs[0])
    p = 400 + len(mirs[0]) - 9
    n = 2_000_000
    recs = np.zeros(n + 4, ALN_DTYPE)
    recs["tid"][:n], recs["pos"][:n], recs["len"][:n] = 1, p, 20
    recs["depth"][:n] = rng.randint(1 << 12, 1 << 13, n)
    recs["strand"][:n] = rng.rand(n) < 0.01
    for j, row in enumerate([(1, 50, 7, 20, 0, 0), (1, 700, 1, 20, 0, 0), (0, 33, 2, 20, 0, 0), (2, 800, 3, 20, 0, 0)]):
        recs[n + j] = row
    recs = recs[np.lexsort((recs["pos"], recs["tid"]))]
    names = ["a", "b", "c"]
    case = Case(parse_mirnas(b"".join(b">m%d\n%s\n" % (i, m) for i, m in enumerate(mirs))), names, [CODE[np.frombuffer(bytes(t), np.uint8)] for t in texts],
                names, [900] * 3, recs)
    _write_inputs(tmp_path, case, [bytes(t) for t in texts], mirs)
    _load(gpu_ctx, recs, 3)
    got, res = _scan(gpu_ctx, tmp_path, case, max_half_score=0)
    want, stats = restate_numpy(case, max_half=0)
    assert got == want and {k: res[k] for k in STAT_KEYS} == stats
    rows = _rows(got)
    assert len(rows) == 1 and int(rows[0][7]) > 1 << 32 and rows[0][6] == b"0" and rows[0][7] == rows[0][8]
    assert stats["minus"] > 10000 and stats["units"] == 5


def test_a_million_units_on_one_transcript_and_100k_transcripts(gpu_ctx, tmp_path):
    rng = np.random.RandomState(12)
    mirs = random_mirnas(rng, 2, 21, 21, t_for_u=0)
    big = bytearray(ACGT[rng.randint(0, 4, 1_300_000)].tobytes())
    n_small, small_len = 100_000, 40
    small = bytearray(ACGT[rng.randint(0, 4, n_small * small_len)].tobytes())
    upos = np.sort(rng.choice(np.arange(1, 1_300_001), size=1_000_000, replace=False))
    for j in range(40):                                   # planted sites under units of the big transcript
        p = int(upos[j * 20_000 + 5])
        o = p + 9 - 21
        if 0 <= o and o + 21 <= len(big):
            big[o:o + 21] = target_of_mirna(mirs[j % 2])
    spos = rng.randint(1, small_len + 1, n_small)
    for j in range(0, n_small, 2000):                     # and in some of the small ones: the whole site inside the transcript
        spos[j] = 21 - 9 + int(rng.randint(0, small_len - 21 + 1))
        o = j * small_len + int(spos[j]) + 9 - 21
        small[o:o + 21] = target_of_mirna(mirs[(j // 2000) % 2])
    texts = [bytes(small[i * small_len:(i + 1) * small_len]) for i in range(n_small // 2)] + [bytes(big)] + \
            [bytes(small[i * small_len:(i + 1) * small_len]) for i in range(n_small // 2, n_small)]
    names = ["s%d" % i for i in range(n_small // 2)] + ["big"] + ["s%d" % i for i in range(n_small // 2, n_small)]
    # the SAM header: the big transcript first, then the small ones from the last to the first
    sq_names = ["big"] + ["s%d" % i for i in range(n_small - 1, -1, -1)]
    sq_lens = [len(big)] + [small_len] * n_small
    recs = np.zeros(1_000_000 + n_small, ALN_DTYPE)
    recs["tid"][:1_000_000], recs["pos"][:1_000_000] = 0, upos
    recs["tid"][1_000_000:], recs["pos"][1_000_000:] = 1 + np.arange(n_small), spos[::-1]
    recs["depth"] = np.minimum(rng.geometric(0.3, len(recs)), 1000)
    recs["len"] = 20
    case = Case(parse_mirnas(b"".join(b">m%d\n%s\n" % (i, m) for i, m in enumerate(mirs))), names, [CODE[np.frombuffer(t, np.uint8)] for t in texts],
                sq_names, sq_lens, recs)
    _write_inputs(tmp_path, case, texts, mirs)
    _load(gpu_ctx, recs, len(sq_names))
    got, res = _scan(gpu_ctx, tmp_path, case, max_half_score=8)
    want, stats = restate_numpy(case, max_half=8)
    assert got == want and {k: res[k] for k in STAT_KEYS} == stats
    rows = _rows(got)
    assert stats["units"] == 1_000_000 + n_small and sum(r[1] == b"big" for r in rows) >= 30 and sum(r[1] != b"big" for r in rows) >= 40
    assert stats["c0"] + stats["c1"] + stats["c4"] >= n_small


def boundary_case():
    """Transcripts of 21..130 nt, among them every length next to a multiple of 32, each with a site at o = 0 and one at o + L = len where both fit,
    and a unit on every position of every transcript: also on the first and the last transcript of the packed text."""
    rng = np.random.RandomState(13)
    mirs = random_mirnas(rng, 6, 12, 24, t_for_u=0) + random_mirnas(rng, 2, 32, 32, t_for_u=0) + random_mirnas(rng, 2, 12, 12, t_for_u=0)
    lens = [33, 31, 32, 63, 64, 65, 95, 96, 97, 127, 128, 129, 21, 40, 50, 130, 32, 64]
    texts, rows = [], []
    for f, ln in enumerate(lens):
        t = bytearray(ACGT[rng.randint(0, 4, ln)].tobytes())
        a, b = mirs[f % len(mirs)], mirs[(f + 3) % len(mirs)]
        if len(a) + len(b) <= ln:
            t[ln - len(b):] = target_of_mirna(b)
        if len(a) <= ln:
            t[:len(a)] = target_of_mirna(a)
        if f == 7:
            t[40] = ord("N")
        texts.append(bytes(t))
        rows += [(f, p, int(rng.randint(1, 30)), 20, 0) for p in range(1, ln + 1)]
    names = ["w%d" % f for f in range(len(lens))]
    case = Case(parse_mirnas(b"".join(b">m%d\n%s\n" % (i, m) for i, m in enumerate(mirs))), names, [CODE[np.frombuffer(t, np.uint8)] for t in texts],
                names, lens, make_records(rows))
    return case, texts, mirs


def test_word_boundaries_and_the_ends_of_the_packed_text(gpu_ctx, tmp_path):
    case, texts, mirs = boundary_case()
    _write_inputs(tmp_path, case, texts, mirs)
    _load(gpu_ctx, case.recs, len(case.sq_names))
    # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change
    for (half, cleavage, cap), passes in zip(((0, False, 0), (16, False, 0), (16, True, 0), (16, False, 2), (16, False, 40)), (1, 1, 1, 28, 2)):
        try:
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, case, max_half_score=half, cleavage_site=cleavage)
        finally:
            gpu_ctx.set_target_capacity(0)
        want, stats = restate_numpy(case, max_half=half, cleavage=cleavage)
        assert got == want, (half, cleavage, cap)
        assert (got, stats) == restate_plain(case, max_half=half, cleavage=cleavage)
        assert {k: res[k] for k in STAT_KEYS} == stats
        assert res["passes"] == passes, (half, cleavage, cap, res)
        if cap == 2:                                  # some (miRNA, category, score) holds more hits than the capacity: split by position
            rows = _rows(got)
            bins = {}
            for r in rows:
                bins[r[0], r[6], r[5]] = bins.get((r[0], r[6], r[5]), 0) + 1
            assert max(bins.values()) > 2 and res["passes"] > len(rows) // 2
    ends = {(r[1], int(r[3]), int(r[4])) for r in _rows(restate_numpy(case, max_half=0)[0])}
    lens = dict(zip(case.fa_names, case.sq_lens))
    assert sum(1 for n in lens if (n.encode(), 1) in {e[:2] for e in ends}) >= 15
    assert sum(1 for n, ln in lens.items() if (n.encode(), ln) in {(e[0], e[2]) for e in ends}) >= 10
    assert (b"w0", 1) in {e[:2] for e in ends} and (b"w17", 64) in {(e[0], e[2]) for e in ends}


# ---------------------------------------------------------------------------------------------------- the command line
def _cli(module, args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli(sweep_input, tmp_path):
    d, case, paths = sweep_input
    r = _cli("mir_prefer_amd.degradome", [str(d / "m.fa"), str(d / "t.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want, stats = restate_numpy(case)
    out = paths[0] + ".degradome.tsv"
    assert open(out, "rb").read() == want and stats["hits"] >= 50
    assert r.stderr.decode().splitlines() == [degradome.summary(stats, out).rstrip("\n")]
    assert r.stderr.decode().startswith("degradome: %d records, %d sense records, %d units (categories 0..4: " % (stats["records"], stats["sense"], stats["units"]))
    os.unlink(out)
    r = _cli("mir_prefer_amd.degradome", ["-s", "5", "-c", "--max-category", "2", "-p", "0.05", "-o", str(tmp_path / "x.tsv"), str(d / "m.fa"), str(d / "t.fa"),
                                          paths[1], paths[0]], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    sub = case.recs[case.recs["sample"] != 2]
    want, stats = restate_numpy(Case(case.mirnas, case.fa_names, case.seqs, case.sq_names, case.sq_lens, sub), max_half=10, cleavage=True, max_category=2, alpha=0.05)
    assert (tmp_path / "x.tsv").read_bytes() == want and stats["hits"] > 5 and not os.path.exists(paths[1] + ".degradome.tsv")


def test_refusals_leave_no_output(sweep_input, tmp_path):
    d, case, paths = sweep_input
    sam = tmp_path / "a.sam"
    head = "@HD\tVN:1.0\n@SQ\tSN:c1\tLN:500\n@SQ\tSN:c2\tLN:300\n"
    sam.write_text(head + "".join("r%d_x3\t0\tc1\t%d\t255\t20M\t*\t0\t0\t%s\t*\n" % (j, 10 + 5 * j, "A" * 20) for j in range(10)))
    (tmp_path / "bad.sam").write_bytes(sam.read_bytes() + b"r_x1\t0\tnope\t5\t255\t20M\t*\t0\t0\t" + b"A" * 20 + b"\t*\n")
    write_fasta(tmp_path / "ok.fa", [("c2", b"ACGT" * 75), ("extra", b"ACGT" * 10), ("c1", b"ACGT" * 125)])
    write_fasta(tmp_path / "short.fa", [("c1", b"ACGT" * 125), ("c2", b"A" * 299)])
    write_fasta(tmp_path / "missing.fa", [("c1", b"ACGT" * 125)])
    (tmp_path / "m.fa").write_bytes(b">m\n" + b"AAAAACCCCC" * 2 + b"\n")       # no site on (ACGT)n at the default -s 4
    (tmp_path / "m11.fa").write_bytes(b">m\n" + b"ACGU" * 5 + b"\n>n\n" + b"A" * 11 + b"\n")
    cases = [(["m11.fa", "ok.fa", "a.sam"], "record 2: the sequence has 11 nt"),
             (["m.fa", "missing.fa", "a.sam"], "contig c2 of the SAM header is not in"),
             (["m.fa", "short.fa", "a.sam"], "contig c2 has 299 bases in"),
             (["m.fa", "ok.fa", "bad.sam"], "not in the @SQ header")]
    for args, why in cases:
        out = tmp_path / (args[2] + ".degradome.tsv")
        out.write_bytes(b"stale\n")
        r = _cli("mir_prefer_amd.degradome", [str(tmp_path / a) for a in args], tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr.decode())
        assert not out.exists(), args
    # an accepted run on the same files; no sense record and no hit are not errors
    r = _cli("mir_prefer_amd.degradome", [str(tmp_path / a) for a in ("m.fa", "ok.fa", "a.sam")], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "a.sam.degradome.tsv").read_bytes() == HEADER and ", 10 units " in r.stderr.decode()
    (tmp_path / "none.sam").write_text(head)
    r = _cli("mir_prefer_amd.degradome", [str(tmp_path / a) for a in ("m.fa", "ok.fa", "none.sam")], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "none.sam.degradome.tsv").read_bytes() == HEADER and "degradome: 0 records, 0 sense records, 0 units " in r.stderr.decode()


def test_chain_trim_collapse_align_degradome(tmp_path):
    """A degradome FASTQ with a 3' adapter through trim, reads collapse and align -r transcripts.fa, then degradome with a mature.fa-style miRNA
    file: each planted cleavage position is its transcript's single highest peak and comes out as a category-0 hit."""
    rng = np.random.RandomState(17)
    adapter = b"TGGAATTCTCGGGTGCCAAGG"
    mirs = random_mirnas(rng, 6, 20, 22, t_for_u=0)
    texts = [bytearray(ACGT[rng.randint(0, 4, 800)].tobytes()) for _ in range(12)]
    planted = []
    for i, m in enumerate(mirs):
        o = 100 + 37 * i
        texts[2 * i][o:o + len(m)] = target_of_mirna(m)
        planted.append((i, 2 * i, o + len(m) - 9))
    reads = []
    for _, f, p in planted:
        reads += [bytes(texts[f][p - 1:p - 1 + 20])] * 50
    for f in range(12):
        for _ in range(25):
            p = int(rng.randint(1, 770))
            reads += [bytes(texts[f][p - 1:p - 1 + 20])] * int(rng.randint(1, 4))
    order = rng.permutation(len(reads))
    with open(tmp_path / "deg.fastq", "wb") as fq:
        for k, j in enumerate(order):
            s = reads[j] + adapter[:int(rng.randint(10, len(adapter) + 1))]
            fq.write(b"@q%d\n%s\n+\n%s\n" % (k, s, b"I" * len(s)))
    write_fasta(tmp_path / "transcripts.fa", [("tx%d gene=%d" % (f, f), bytes(t)) for f, t in enumerate(texts)])
    (tmp_path / "mature.fa").write_bytes(b"".join(b">chr%d:%d-%d + miRNA_%d\n%s\n" % (i, 10, 10 + len(m) - 1, i, m) for i, m in enumerate(mirs)))
    (tmp_path / "names.txt").write_text("PARE\n")
    for module, args in (("mir_prefer_amd.trim", ["-a", adapter.decode(), "deg.fastq"]),
                         ("mir_prefer_amd.reads", ["collapse", "names.txt", "deg.fastq.trimmed.fa"]),
                         ("mir_prefer_amd.align", ["-f", "-r", "transcripts.fa", "deg.fastq.trimmed.fa.processed"]),
                         ("mir_prefer_amd.degradome", ["-s", "2", "mature.fa", "transcripts.fa", "deg.fastq.trimmed.fa.processed.sam"])):
        r = _cli(module, args, tmp_path)
        assert r.returncode == 0, (module, r.stderr.decode())
    rows = _rows((tmp_path / "deg.fastq.trimmed.fa.processed.sam.degradome.tsv").read_bytes())
    for i, f, p in planted:
        mine = [r for r in rows if r[0] == b"chr%d:%d-%d + miRNA_%d" % (i, 10, 10 + len(mirs[i]) - 1, i) and r[1] == b"tx%d" % f and int(r[2]) == p]
        assert len(mine) == 1 and mine[0][5] == b"0.0" and mine[0][6] == b"0" and int(mine[0][7]) >= 50 and mine[0][7] == mine[0][8], (i, mine)
