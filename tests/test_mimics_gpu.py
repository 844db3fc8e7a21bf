"""GPU tests of the target-mimic search (mirp_mimic_scan, mimic_kernels.hip): whole TSV files against the numpy restatement of
tests/mimic_restatement.py (pinned to the plain enumeration in test_mimics_cpu.py) over L = 12..32, -n, -l and -b, several target files, N runs,
IUPAC codes, lower case and unknown miRNA letters, with sites planted at every loop position on each strand; a 38-base interval across every
alignment of the packed words; contigs that are exactly one site; full, empty, first and last seed buckets; more than 65,536 miRNAs; forced
capacities; -k; the command line."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.mimic_restatement import (ACGT, HEADER, LOOPS, all_sites, columns, emit, loops_seen, mimic_line, mimic_text, plant_mimic, restate_files,
                                     seed_stats, sites_numpy)
from tests.test_targets_cpu import MCODE, ROOT, load_reference, parse_mirnas, random_mirnas, write_fasta

pytestmark = pytest.mark.gpu
BOTH = {(s, P) for s in (b"+", b"-") for P in LOOPS}


def _scan(ctx, tmp_path, mirna_path, target_paths, **kw):
    out = tmp_path / "out.tsv"
    res = ctx.mimic_scan(str(mirna_path), [str(p) for p in target_paths], str(out), **kw)
    return out.read_bytes(), res


def _rows(data):
    return [ln.split(b"\t") for ln in data.split(b"\n")[1:-1]]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Two target files, four contigs of which one is empty, N runs, IUPAC codes, lower case; one miRNA of every length 12..32 plus miRNAs with
    unknown letters, lower case and T for U; per miRNA and loop length 2, 3, 6 three mimic sites at a random strand and loop position with up to
    two substitutions."""
    d = tmp_path_factory.mktemp("mimics_small")
    rng = np.random.RandomState(27)
    mirs = [random_mirnas(np.random.RandomState(L), 1, L, L, t_for_u=0.3)[0] for L in range(12, 33)]
    mirs += random_mirnas(rng, 9, 12, 32, unknown=0.04, lower=0.3)
    texts = [bytearray(ACGT[rng.randint(0, 4, n)].tobytes()) for n in (9000, 4000, 6000)]
    for m in mirs:
        stand_in = bytes(c if c in b"ACGUTacgut" else ord("A") for c in m)         # an unknown letter is planted as a mismatch (or spoils the seed)
        for G in (2, 3, 6):
            for _ in range(3):
                plant_mimic(rng, texts[int(rng.randint(0, 3))], stand_in, int(rng.randint(0, 2)), LOOPS[int(rng.randint(0, 3))], G, subs=(0, 2))
    texts[0][1000:1040] = b"N" * 40
    texts[0][2500] = ord("R"); texts[0][5000] = ord("y"); texts[1][300] = ord("-")
    for t in texts:
        lo = int(rng.randint(0, len(t) - 500))
        t[lo:lo + 400] = t[lo:lo + 400].lower()
    write_fasta(d / "t1.fa", [("chrB desc", bytes(texts[0])), ("empty", b""), ("chrA", bytes(texts[1]))])
    write_fasta(d / "t2.fa", [("tx.1", bytes(texts[2]))], width=70)
    (d / "m.fa").write_bytes(b"header text\n" + b"".join(b">mir%d  some\tdesc \r\n%s\r\n%s\n" % (i, m[:7], m[7:]) for i, m in enumerate(mirs)))
    return d


def test_grid_matches_the_restatement(gpu_ctx, small, tmp_path):
    paths = [small / "t1.fa", small / "t2.fa"]
    mirnas = parse_mirnas((small / "m.fa").read_bytes())
    names, seqs = load_reference(paths)
    assert len(mirnas) == 30 and names == ["chrB", "chrA", "tx.1"]
    no_seed, seeds, entries = seed_stats(mirnas, seqs, True)
    assert no_seed >= 1 and any((mc > 3).any() and not (mc[1:8] > 3).any() for _, mc in mirnas)
    seen = 0
    for G in (2, 3, 6):
        sites = all_sites(mirnas, names, seqs, G)
        want3 = emit(sites, 3, True, 0)
        print("expected lines of -n 3 -l %d -b by (strand, loop):" % G, sorted(loops_seen(want3)), want3.count(b"\n") - 1)
        assert loops_seen(want3) == BOTH                                  # the comparison cannot pass on an empty class
        for n, both in itertools.product((0, 3, 6), (False, True)):
            got, res = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, max_imperfect=n, loop_len=G, both_strands=both)
            want = emit(sites, n, both, 0)
            assert got == want, (G, n, both)
            assert res["sites"] == want.count(b"\n") - 1 and res["mirnas"] == 30 and res["targets"] == 3 and res["bases"] == 19000
            assert res["no_seed"] == no_seed and res["passes"] == 1
            assert (res["seeds"], res["entries"]) == ((seeds, entries) if both else seed_stats(mirnas, seqs, False)[1:])
            seen += res["sites"]
    assert seen > 600


def test_38_base_interval_across_every_word_alignment(gpu_ctx, tmp_path):
    """A 32-nt miRNA with a loop of 6 spans 38 bases: planted at every start modulo 64 on both strands it crosses the 64-bit words of the packed
    target (32 bases per word) in every way, with the span of a lane starting up to 30 bases before the seed."""
    rng = np.random.RandomState(11)
    mir = random_mirnas(rng, 1, 32, 32, t_for_u=0.0)[0]
    recs, want_sites, total = [], [], 0
    for strand in (0, 1):
        for shift in range(64):
            P = LOOPS[shift % 3]
            pre = ACGT[rng.randint(0, 4, 3 + (shift - total - 3) % 64)].tobytes()         # the site starts at `shift` modulo 64, over all targets
            assert (total + len(pre)) % 64 == shift
            text = bytearray(pre + b"A" * 38 + ACGT[rng.randint(0, 4, 5 + shift % 3)].tobytes())
            plant_mimic(rng, text, mir, strand, P, 6, at=len(pre))
            recs.append(("c%d_%d" % (strand, shift), bytes(text)))
            total += len(text)
            want_sites.append((b"c%d_%d" % (strand, shift), len(pre) + 1, len(pre) + 38, b"-" if strand else b"+"))
    write_fasta(tmp_path / "t.fa", recs)
    write_fasta(tmp_path / "m.fa", [("m32", mir)])
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_imperfect=0, loop_len=6, both_strands=True)
    assert got == restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=0, G=6, both=True)
    have = {(f[1], int(f[2]), int(f[3]), f[4]) for f in _rows(got)}
    assert all(s in have for s in want_sites) and len(want_sites) == 128 and loops_seen(got) == BOTH


def test_sites_that_fill_a_contig(gpu_ctx, tmp_path):
    """Contigs that are exactly one mimic site, side by side so that a read past either end would meet real bases, and the same contigs one base
    short at either end; the first contig starts with a site at position 0 and the last ends with one at the last base."""
    rng = np.random.RandomState(12)
    mirs = random_mirnas(rng, 3, 12, 31, t_for_u=0.0) + random_mirnas(rng, 1, 32, 32, t_for_u=0.0)
    recs, whole = [], []
    for i, m in enumerate(mirs):
        for strand, P, G in itertools.product((0, 1), LOOPS, (2, 3, 6)):
            if G != 3 and P != 10:
                continue
            text = bytearray(len(m) + G)
            plant_mimic(rng, text, m, strand, P, G, at=0)
            name = "m%d_%d_%d_%d" % (i, strand, P, G)
            recs += [(name, bytes(text)), (name + "_a", bytes(text[1:])), (name + "_z", bytes(text[:-1]))]
            if G == 3:
                whole.append((b"m%d" % i, name.encode(), 1, len(text), b"-" if strand else b"+"))
    recs.append(("last", recs[-3][1]))                                    # recs[0] is a whole site at position 0; the last contig one at the last base
    write_fasta(tmp_path / "t.fa", recs)
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    for G in (2, 3, 6):
        got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_imperfect=6, loop_len=G, both_strands=True)
        assert got == restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, G=G, both=True), G
        have = {(f[0], f[1], int(f[2]), int(f[3]), f[4]) for f in _rows(got)}
        if G == 3:
            assert [s for s in whole if s not in have] == [] and len(whole) == 24
            assert any(f[1] == b"last" for f in have) and whole[0] in have
        assert all(f[3] <= len(dict(recs)[f[1].decode()]) for f in have) and len(have) >= 8


def test_seed_buckets(gpu_ctx, tmp_path):
    """300 miRNAs in one bucket (one seed, different lengths and 3' parts) beside an empty neighbour; the first bucket (a seed of A, key 0) and
    the last (a seed of U, key 16383); a miRNA with an unknown letter in the seed has no line and is counted."""
    rng = np.random.RandomState(13)
    head = b"GACGUAGC"                                                    # positions 1..8
    family = [head + bytes(b"ACGU"[c] for c in rng.randint(0, 4, int(rng.randint(4, 25)))) for _ in range(300)]
    lonely = [b"C" + b"A" * 7 + b"GCUAGCUAGGCAU", b"G" + b"U" * 7 + b"CAGUCGAUCGAUGC", b"GACGNAGC" + b"AUGCAUGCAUGCAU"]
    mirs = family + lonely
    text = bytearray(ACGT[rng.randint(0, 4, 8000)].tobytes())
    at = 20
    for i in list(range(0, 300, 7)) + [300, 301, 300, 301]:
        plant_mimic(rng, text, mirs[i], i % 2, LOOPS[i % 3], 3, subs=(0, 2), at=at)
        at += 60
    plant_mimic(rng, text, lonely[2].replace(b"N", b"U"), 0, 10, 3, at=at)
    write_fasta(tmp_path / "t.fa", [("a", bytes(text[:4000])), ("b", bytes(text[4000:]))])
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    mirnas = parse_mirnas((tmp_path / "m.fa").read_bytes())
    names, seqs = load_reference([tmp_path / "t.fa"])
    keys = {tuple(int(x) for x in mc[1:8]) for _, mc in mirnas}
    assert (0,) * 7 in keys and (3,) * 7 in keys and len(keys) == 4
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_imperfect=4, both_strands=True)
    assert got == emit(all_sites(mirnas, names, seqs, 3), 4, True, 0)
    by = {f[0] for f in _rows(got)}
    assert b"m300" in by and b"m301" in by and b"m302" not in by and len(by) > 100
    assert res["no_seed"] == 1 and (res["no_seed"], res["seeds"], res["entries"]) == seed_stats(mirnas, seqs, True)
    assert res["entries"] >= 300 * 40                                     # every planted family site makes its lane walk the whole bucket


def test_more_than_65536_mirnas(gpu_ctx, tmp_path):
    """70,000 miRNAs drawn from 300 sequences: the key holds the miRNA's index in the file, not one inside a group of 2^16."""
    rng = np.random.RandomState(5)
    base = random_mirnas(rng, 300, 18, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 18000)].tobytes())
    for i, m in enumerate(base):
        plant_mimic(rng, text, m, i % 2, LOOPS[i % 3], 3, subs=(0, 1), at=i * 60)
    write_fasta(tmp_path / "t.fa", [("t", bytes(text))])
    pick = rng.randint(0, 300, 70000)
    (tmp_path / "m.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, base[p]) for i, p in enumerate(pick)))
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_imperfect=3, both_strands=True)
    names, seqs = load_reference([tmp_path / "t.fa"])
    per = {}
    for p in set(pick.tolist()):
        mc = MCODE[np.frombuffer(base[p], dtype=np.uint8)]
        per[p] = [(s, columns(mc, seqs[0], s[1], s[2], s[3], 3)) for s in sorted(sites_numpy(mc, seqs[0], 3)) if s[0] <= 3]
    want = [HEADER]
    for i, p in enumerate(pick):
        mc = MCODE[np.frombuffer(base[p], dtype=np.uint8)]
        for (imperfect, o, strand, P), cols in per[p]:
            want.append(mimic_line(b"m%d" % i, "t", o, strand, imperfect, mc, P, cols))
    assert res["sites"] >= 60000 and res["mirnas"] == 70000 and res["no_seed"] == 0
    assert got == b"".join(want)
    assert got.count(b"\nm69999\t") >= 1 and loops_seen(got) == BOTH


def test_forced_capacities_give_the_same_bytes(gpu_ctx, tmp_path):
    """Capacities of 40 and 2 keys: passes by (miRNA, imperfect) and, for one (miRNA, imperfect) with 60 sites, by ranges of positions."""
    rng = np.random.RandomState(8)
    mirs = random_mirnas(rng, 5, 14, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 12000)].tobytes())
    for m in mirs[1:]:
        for j in range(12):
            plant_mimic(rng, text, m, j % 2, LOOPS[j % 3], 3, subs=(0, 3))
    for i in range(60):
        plant_mimic(rng, text, mirs[0], i % 2, LOOPS[i % 3], 3, at=150 * i)
    write_fasta(tmp_path / "t.fa", [("a", bytes(text[:7000])), ("b", bytes(text[7000:]))])
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    full = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, both=True)
    zero = [f for f in _rows(full) if f[0] == b"m0" and f[5] == b"0"]
    assert len(zero) >= 55
    try:
        for cap, (n, both, k) in itertools.product((40, 2, 0), ((6, True, 0), (3, False, 0), (6, True, 30), (2, True, 3))):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_imperfect=n, both_strands=both, max_sites=k)
            want = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=n, both=both, k=k)
            assert got == want, (cap, n, both, k)
            assert res["sites"] == want.count(b"\n") - 1 > 8
            assert (res["passes"] > 1) == (cap > 0), (cap, res)
            if cap and (n, both, k) == (6, True, 0):                      # the sites of (m0, 0) alone overflow a pass; the other miRNAs need one more
                assert res["passes"] >= -(-len(zero) // cap) + 1, (cap, res)
    finally:
        gpu_ctx.set_target_capacity(0)


def test_capacity_2_with_overlapping_sites_on_both_strands(gpu_ctx, tmp_path):
    """An A/U repeat miRNA on an (AT)n run has a site at every second start on each strand, the two strands interleaved: a bin over the capacity
    is split by interval start (the output order), not by the lane that found the site, which differs by up to 30 between the strands."""
    rng = np.random.RandomState(9)
    text = ACGT[rng.randint(0, 4, 300)].tobytes() + b"AT" * 90 + ACGT[rng.randint(0, 4, 300)].tobytes() + b"TA" * 40 + b"CCGG"
    write_fasta(tmp_path / "t.fa", [("t", text)])
    write_fasta(tmp_path / "m.fa", [("au21", b"UAUAUAUAUAUAUAUAUAUAU"), ("au12", b"AUAUAUAUAUAU"), ("other", b"GACGUAGCAUGCAUGCAUGCAU")])
    full = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=2, G=2, both=True)     # an even loop keeps the repeat in phase
    rows = _rows(full)
    starts = {s: sorted(int(f[2]) for f in rows if f[0] == b"au12" and f[5] == b"0" and f[4] == s) for s in (b"+", b"-")}
    assert len(starts[b"+"]) > 60 and len(starts[b"-"]) > 60 and starts[b"+"][0] < starts[b"-"][5] < starts[b"+"][-1]
    try:
        for cap, k, n in itertools.product((2, 7, 0), (0, 5, 40), (0, 2)):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_imperfect=n, loop_len=2, both_strands=True, max_sites=k)
            assert got == restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=n, G=2, both=True, k=k), (cap, k, n)
            assert (res["passes"] > 10) == (cap > 0), (cap, res)
    finally:
        gpu_ctx.set_target_capacity(0)


def test_max_sites_is_a_prefix_per_mirna(gpu_ctx, small, tmp_path):
    paths = [small / "t1.fa", small / "t2.fa"]
    full, _ = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, max_imperfect=6, both_strands=True)
    lines = full.split(b"\n")[1:-1]
    names = [n for n, _ in parse_mirnas((small / "m.fa").read_bytes())]
    for k in (1, 2, 3):
        got, res = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, max_imperfect=6, both_strands=True, max_sites=k)
        want = []
        for name in names:
            want += [ln for ln in lines if ln.startswith(name + b"\t")][:k]
        print("-k", k, len(want), "of", len(lines))
        assert got.split(b"\n")[1:-1] == want and res["sites"] == len(want) and 15 * k <= len(want) < len(lines)


def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.mimics"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli(small, tmp_path):
    shutil.copy(small / "m.fa", tmp_path / "m.fa")
    paths = [str(small / "t1.fa"), str(small / "t2.fa")]
    r = _cli(["-n", "4", "-l", "6", "-b", "-k", "6", str(tmp_path / "m.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_files(tmp_path / "m.fa", paths, n=4, G=6, both=True, k=6)
    assert (tmp_path / "m.fa.mimics.tsv").read_bytes() == want and want.count(b"\n") > 20
    no_seed = sum(1 for _, mc in parse_mirnas((tmp_path / "m.fa").read_bytes()) if (mc[1:8] > 3).any())
    assert r.stderr.decode().splitlines()[-1] == "mimics: 30 miRNAs (%d without a usable seed), 3 targets, %d bases scanned (both strands), %d sites written to %s" % (
        no_seed, 9000 + 4000 + 6000, want.count(b"\n") - 1, tmp_path / "m.fa.mimics.tsv")
    r = _cli(["-o", str(tmp_path / "x.tsv"), str(tmp_path / "m.fa"), paths[1]], tmp_path)
    assert r.returncode == 0 and (tmp_path / "x.tsv").read_bytes() == restate_files(tmp_path / "m.fa", [paths[1]])
    # a refused input: status 255, `Error: ...`, and no output file, not even the one the run before left
    for bad, where in ((b">ok\nACGUACGUACGUACGU\n> \t\nACGUACGUACGUACGU\n", "record 2"), (b">ok\nACGUACGUACGUACG\xc3\xa9\n", "record 1")):
        (tmp_path / "bad.fa").write_bytes(bad)
        shutil.copy(tmp_path / "x.tsv", tmp_path / "bad.fa.mimics.tsv")
        r = _cli([str(tmp_path / "bad.fa"), paths[1]], tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and where in r.stderr.decode()
        assert r.returncode == 255 and not (tmp_path / "bad.fa.mimics.tsv").exists()
