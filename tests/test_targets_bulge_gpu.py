"""GPU tests of the bulged target sites (mirp_target_scan with bulge = 1, tg_bulge_scan_kernel; DESIGN.md §14, "Bulged sites"): whole TSV files
against the numpy restatement of tests/test_targets_bulge_cpu.py (itself pinned there to the plain enumeration and to the alignment DP) over
L = 12..32, every option combination, several target files, N runs, IUPAC codes, lower case and unknown miRNA letters, with sites of each kind
planted on each strand; forced capacities of 2 and 40 keys; a 32-nt miRNA whose t site crosses a 64-bit word of the packed target at every
alignment; sites that fill a contig; more miRNAs than one group; the ungapped lines of a --bulge run against the run without it; the command line."""
import itertools
import shutil
import subprocess
import sys
import os

import numpy as np
import pytest

from tests.test_targets_bulge_cpu import (BHEADER, KIND_M, KIND_T, all_sites_numpy, bulge_line, bulge_site_plain, bulged_site, columns, emit,
                                          plant_bulged, sites_bulge_numpy)
from tests.test_targets_cpu import ACGT, CODE, MCODE, ROOT, load_reference, parse_mirnas, plant, random_mirnas, write_fasta

pytestmark = pytest.mark.gpu


def _scan(ctx, tmp_path, mirna_path, target_paths, **kw):
    out = tmp_path / "out.tsv"
    res = ctx.target_scan(str(mirna_path), [str(p) for p in target_paths], str(out), **kw)
    return out.read_bytes(), res


def _tags(data):
    """-> {(strand, first letter of the bulge column): lines}"""
    n = {}
    for ln in data.split(b"\n")[1:-1]:
        f = ln.split(b"\t")
        n[(f[4], f[11][:1])] = n.get((f[4], f[11][:1]), 0) + 1
    return n


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The `small` inputs of test_targets_gpu.py (two target files, four contigs of which one is empty, N runs, IUPAC codes, lower case; one miRNA
    of every length 12..32 plus miRNAs with unknown letters, lower case and T for U, planted ungapped), and per miRNA and target text three sites
    with one inserted or deleted base on a random strand."""
    d = tmp_path_factory.mktemp("targets_bulge_small")
    rng = np.random.RandomState(22)
    mirs = [random_mirnas(np.random.RandomState(L), 1, L, L, t_for_u=0.3)[0] for L in range(12, 33)]
    mirs += random_mirnas(rng, 9, 12, 32, unknown=0.06, lower=0.3)
    texts = [bytearray(ACGT[rng.randint(0, 4, n)].tobytes()) for n in (9000, 4000, 6000)]
    for m in mirs:
        for t in texts:
            plant(rng, t, m, 1, subs=(0, 3))
            plant_bulged(rng, t, m, 3, subs=(0, 1))
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
    sites = {c: all_sites_numpy(mirnas, names, seqs, c) for c in (False, True)}
    # the comparison cannot pass on an empty class: t and m lines on each strand in the expected file of -s 5 -b
    n = _tags(emit(sites[False], 10, True, 0))
    print("expected lines of -s 5 -b by (strand, kind):", sorted(n.items()))
    for strand in (b"+", b"-"):
        assert n.get((strand, b"t"), 0) >= 20 and n.get((strand, b"m"), 0) >= 20 and n.get((strand, b"."), 0) >= 20, n
    seen = 0
    for half, both, cleavage, k in itertools.product((0, 5, 6, 10, 16), (False, True), (False, True), (0, 1, 3)):
        got, res = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, max_half_score=half, both_strands=both, cleavage_site=cleavage, max_sites=k, bulge=True)
        want = emit(sites[cleavage], half, both, k)
        assert got == want, (half, both, cleavage, k)
        assert res["sites"] == want.count(b"\n") - 1 and res["mirnas"] == 30 and res["targets"] == 3
        assert res["evaluations"] == res["bases"] * 30 * (2 if both else 1)
        seen += res["sites"]
    assert seen > 2000


def test_ungapped_lines_are_the_run_without_bulge(gpu_ctx, small, tmp_path):
    paths = [small / "t1.fa", small / "t2.fa"]
    for half, both, cleavage in ((8, True, False), (11, True, True), (16, False, False)):
        kw = dict(max_half_score=half, both_strands=both, cleavage_site=cleavage)
        plain, res0 = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, **kw)
        bulged, res1 = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, bulge=True, **kw)
        lines = bulged.split(b"\n")
        assert lines[0] == plain.split(b"\n")[0] + b"\tbulge"
        dots = [ln[:-2] for ln in lines[1:-1] if ln.endswith(b"\t.")]
        assert dots == plain.split(b"\n")[1:-1] and len(dots) == res0["sites"] > 0
        assert res1["sites"] > res0["sites"] and res1["evaluations"] == res0["evaluations"]


def _restate_files(mirna_path, target_paths, max_half, both, cleavage=False, k=0):
    mirnas = parse_mirnas(open(mirna_path, "rb").read())
    names, seqs = load_reference(target_paths)
    return emit(all_sites_numpy(mirnas, names, seqs, cleavage, max_half), max_half, both, k)


def test_forced_capacities_give_the_same_bytes(gpu_ctx, tmp_path):
    """Capacities of 40 and 2 keys: passes by (miRNA, score) and, for one (miRNA, score) with 60 sites of one kind, by ranges of offsets."""
    rng = np.random.RandomState(8)
    mirs = random_mirnas(rng, 5, 14, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 12000)].tobytes())
    for i in range(60):
        site = bulged_site(mirs[0].replace(b"U", b"T"), i % 2, KIND_T if i % 3 else KIND_M, 6, b"A")
        text[150 * i:150 * i + len(site)] = site
    for m in mirs[1:]:
        plant(rng, text, m, 8, subs=(0, 2))
        plant_bulged(rng, text, m, 12, subs=(0, 1))
    write_fasta(tmp_path / "t.fa", [("a", bytes(text[:7000])), ("b", bytes(text[7000:]))])
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    try:
        # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change
        for cap, (half, both, cleavage, k), passes in ((40, (6, True, False, 0), 4), (40, (6, True, False, 30), 4), (2, (4, False, True, 0), 21),
                                                        (2, (5, True, False, 3), 33), (0, (6, True, False, 0), 1)):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=half, both_strands=both, cleavage_site=cleavage,
                             max_sites=k, bulge=True)
            want = _restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], half, both, cleavage, k)
            assert got == want, (cap, half, both, cleavage, k)
            assert (res["passes"] > 3) == (cap > 0), (cap, res)
            assert res["passes"] == passes, (cap, half, both, cleavage, k, res)
            assert k or {b"t", b"m", b"."} <= {tag for _, tag in _tags(want)}
    finally:
        gpu_ctx.set_target_capacity(0)


def test_capacity_2_with_three_sites_of_one_score_at_one_offset(gpu_ctx, tmp_path):
    """A 12-nt miRNA at -s 8 on random sequence has offsets that hold three bulged sites of one score (t and m on the two strands; up to four can
    meet).  A pass cannot split an offset, so with bulge it holds at least 4 keys; the set capacity of 2 must still end and give the same bytes."""
    t = np.random.RandomState(3).randint(0, 4, 60000)
    text = ACGT[np.concatenate([t[11043:13043], t[51040:53040]])].tobytes()
    write_fasta(tmp_path / "t.fa", [("t", text)])
    write_fasta(tmp_path / "m.fa", [("m", b"CUAAGUAUUGGU")])
    want = _restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], 16, True)
    per = {}
    for f in (ln.split(b"\t") for ln in want.split(b"\n")[1:-1]):
        per[(f[2], f[5])] = per.get((f[2], f[5]), 0) + 1
    assert max(per.values()) >= 3
    try:
        # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change (2 and 3 are both raised to 4)
        for cap, passes in ((2, 212), (3, 212), (40, 12), (0, 1)):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=16, both_strands=True, bulge=True)
            assert got == want, cap
            assert (res["passes"] > 3) == (cap > 0)
            assert res["passes"] == passes, (cap, res)
    finally:
        gpu_ctx.set_target_capacity(0)


def test_32_nt_t_site_across_every_word_alignment(gpu_ctx, tmp_path):
    """A 32-nt miRNA's t site spans 33 bases: at every start modulo 64 it crosses a 64-bit word of the packed target (32 bases per word)."""
    rng = np.random.RandomState(11)
    mir = random_mirnas(rng, 1, 32, 32, t_for_u=0.0)[0]
    dna = mir.replace(b"U", b"T")
    recs, want_sites, total = [], [], 0
    for shift in range(64):
        strand, P = shift % 2, 3 + shift % 27
        nb = (dna[P - 1:P], dna[P:P + 1])
        extra = next(bytes([c]) for c in b"ACGT" if bytes([c]) not in nb)
        site = bulged_site(dna, strand, KIND_T, P, extra)
        pre = ACGT[rng.randint(0, 4, 3 + (shift - total - 3) % 64)].tobytes()         # the site starts at `shift` modulo 64, over all targets
        assert (total + len(pre)) % 64 == shift
        recs.append(("c%d" % shift, pre + site + ACGT[rng.randint(0, 4, 5 + shift % 3)].tobytes()))
        total += len(recs[-1][1])
        want_sites.append((b"c%d" % shift, len(pre) + 1, len(pre) + 33, b"-" if strand else b"+", b"t%d" % P))
    write_fasta(tmp_path / "t.fa", recs)
    write_fasta(tmp_path / "m.fa", [("m32", mir)])
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=4, both_strands=True, bulge=True)
    assert got == _restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], 4, True)
    have = {(f[1], int(f[2]), int(f[3]), f[4], f[11]) for f in (ln.split(b"\t") for ln in got.split(b"\n")[1:-1])}
    assert all(s in have for s in want_sites)


def test_sites_that_fill_a_contig(gpu_ctx, tmp_path):
    """Contigs that are exactly one bulged site (its first and last base are the contig's), side by side so that a read past either end would meet
    real bases, and the same contigs one base short at either end."""
    rng = np.random.RandomState(12)
    mirs = random_mirnas(rng, 4, 19, 32, t_for_u=0.0) + random_mirnas(rng, 1, 32, 32, t_for_u=0.0)
    recs, want_sites, planted = [], [], 0
    for i, m in enumerate(mirs):
        dna = m.replace(b"U", b"T")
        mc = MCODE[np.frombuffer(m, dtype=np.uint8)]
        for strand, kind, P in itertools.product((0, 1), (KIND_T, KIND_M), (2, 7, len(m) - 2)):
            nb = (dna[P - 1:P], dna[P:P + 1])
            site = bulged_site(dna, strand, kind, P, next(bytes([c]) for c in b"ACGT" if bytes([c]) not in nb))
            name = "m%d_%d_%d_%d" % (i, strand, kind, P)
            recs += [(name, site), (name + "_a", site[1:]), (name + "_z", site[:-1])]
            planted += 1
            # the plain enumeration says which planted sites are written (one that an ungapped alignment matches is dominated) and at which P
            r = bulge_site_plain(mc, CODE[np.frombuffer(site, dtype=np.uint8)], 0, strand, kind, False)
            if r is not None and r[0] <= 6:
                want_sites.append((b"m%d" % i, name.encode(), 1, len(site), b"-" if strand else b"+", b"%s%d" % (b"t" if kind == KIND_T else b"m", r[1])))
    write_fasta(tmp_path / "t.fa", recs)
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=6, both_strands=True, bulge=True)
    assert got == _restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], 6, True)
    have = {(f[0], f[1], int(f[2]), int(f[3]), f[4], f[11]) for f in (ln.split(b"\t") for ln in got.split(b"\n")[1:-1]) if f[11] != b"."}
    assert [s for s in want_sites if s not in have] == []
    assert 2 * len(want_sites) > planted and {(s[4], s[5][:1]) for s in want_sites} == {(b"+", b"t"), (b"+", b"m"), (b"-", b"t"), (b"-", b"m")}
    # no bulged line on a contig that is the site less its first or last base reaches over the contig
    assert all(f[3] <= len(dict(recs)[f[1].decode()]) for f in have)


def test_more_mirnas_than_one_group(gpu_ctx, tmp_path):
    """70,000 miRNAs (65,536 per group) drawn from 300 sequences, each with one bulged site on the target."""
    rng = np.random.RandomState(5)
    base = random_mirnas(rng, 300, 18, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 30000)].tobytes())
    for i, m in enumerate(base):
        kind = KIND_T if i % 2 else KIND_M
        site = bulged_site(m.replace(b"U", b"T"), (i // 2) % 2, kind, 3 + i % 12, b"ACGT"[i % 4:][:1])
        text[i * 100:i * 100 + len(site)] = site
    write_fasta(tmp_path / "t.fa", [("t", bytes(text))])
    pick = rng.randint(0, 300, 70000)
    (tmp_path / "m.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, base[p]) for i, p in enumerate(pick)))
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=5, both_strands=True, bulge=True)
    names, seqs = load_reference([tmp_path / "t.fa"])
    per = {}
    for p in set(pick.tolist()):
        mc = MCODE[np.frombuffer(base[p], dtype=np.uint8)]
        per[p] = [(s, columns(mc, seqs[0], s[1], s[2], s[3], s[4])) for s in sorted(sites_bulge_numpy(mc, seqs[0], False, 5))]
    want = [BHEADER]
    for i, p in enumerate(pick):
        mc = MCODE[np.frombuffer(base[p], dtype=np.uint8)]
        for (half, o, strand, kind, P), cols in per[p]:
            want.append(bulge_line(b"m%d" % i, "t", o, len(mc), strand, half, mc, kind, P, cols))
    assert res["sites"] >= 50000 and res["mirnas"] == 70000
    assert got == b"".join(want)
    tags = _tags(got)
    assert all(tags.get((s, k), 0) > 1000 for s in (b"+", b"-") for k in (b"t", b"m")), tags


def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli(small, tmp_path):
    shutil.copy(small / "m.fa", tmp_path / "m.fa")
    paths = [str(small / "t1.fa"), str(small / "t2.fa")]
    r = _cli(["-g", "-s", "3.5", "-b", "-c", "-k", "6", str(tmp_path / "m.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = _restate_files(tmp_path / "m.fa", paths, 7, True, True, 6)
    assert (tmp_path / "m.fa.targets.tsv").read_bytes() == want
    assert {b"t", b"m", b"."} <= {tag for _, tag in _tags(want)}
    assert r.stderr.decode().splitlines()[-1] == "targets: 30 miRNAs, 3 targets, %d bases scanned (both strands), %d sites written to %s" % (
        9000 + 4000 + 6000, want.count(b"\n") - 1, tmp_path / "m.fa.targets.tsv")
    r = _cli(["--bulge", "-o", str(tmp_path / "x.tsv"), str(tmp_path / "m.fa"), paths[1]], tmp_path)
    assert r.returncode == 0 and (tmp_path / "x.tsv").read_bytes() == _restate_files(tmp_path / "m.fa", [paths[1]], 8, False)
