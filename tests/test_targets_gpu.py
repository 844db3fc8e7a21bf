"""GPU tests of the plant miRNA target-site search (mirp_target_scan, targets_kernels.hip): whole TSV files against the numpy
restatement of tests/test_targets_cpu.py over L = 12..32, every option combination, several target files, lower case and IUPAC codes; more
miRNAs than one group of the scan; a forced capacity overflow; target positions past 2^31; 2,000 miRNAs x 50 Mb; the refusals; the command line;
and the chain cli pipeline -> <prefix>_miRNA.mature.fa -> targets on a golden dataset."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_targets_cpu import (ACGT, HEADER, MCODE, ROOT, _line, load_reference, parse_mirnas, plant, random_mirnas, restate_files,
                                    restate_numpy, sites_numpy, target_of_mirna, write_fasta)

pytestmark = pytest.mark.gpu


def _scan(ctx, tmp_path, mirna_path, target_paths, **kw):
    out = tmp_path / "out.tsv"
    res = ctx.target_scan(str(mirna_path), [str(p) for p in target_paths], str(out), **kw)
    return out.read_bytes(), res


def _kw(max_half=8, both=False, cleavage=False, k=0):
    return dict(max_half_score=max_half, both_strands=both, cleavage_site=cleavage, max_sites=k), dict(max_half=max_half, both=both, cleavage=cleavage, k=k)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """Two target files (four contigs, one of them empty) with N runs, IUPAC codes and lower case, and one miRNA of every length 12..32 plus
    miRNAs with unknown letters, lower case and T for U, each planted a few times with up to 3 substitutions on either strand."""
    d = tmp_path_factory.mktemp("targets_small")
    rng = np.random.RandomState(21)
    mirs = [random_mirnas(np.random.RandomState(L), 1, L, L, t_for_u=0.3)[0] for L in range(12, 33)]
    mirs += random_mirnas(rng, 9, 12, 32, unknown=0.06, lower=0.3)
    texts = [bytearray(ACGT[rng.randint(0, 4, n)].tobytes()) for n in (9000, 4000, 6000)]
    for m in mirs:
        for t in texts:
            plant(rng, t, m, 2, subs=(0, 3))
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
    seen_sites = 0
    for half, both, cleavage, k in itertools.product((0, 3, 5, 8, 16), (False, True), (False, True), (0, 1, 3)):
        if half == 16 and k == 0 and both:
            continue                                 # the largest output is covered with -k
        gk, rk = _kw(half, both, cleavage, k)
        got, res = _scan(gpu_ctx, tmp_path, small / "m.fa", paths, **gk)
        want = restate_numpy(mirnas, names, seqs, **rk)
        assert got == want, (half, both, cleavage, k)
        assert res["sites"] == want.count(b"\n") - 1 and res["mirnas"] == 30 and res["targets"] == 3
        assert res["evaluations"] == res["bases"] * 30 * (2 if both else 1)
        seen_sites += res["sites"]
    assert seen_sites > 1000


def test_more_mirnas_than_one_group(gpu_ctx, tmp_path):
    """70,000 miRNAs (the scan takes 65,536 per group) drawn from 400 sequences, each planted on one target."""
    rng = np.random.RandomState(5)
    base = random_mirnas(rng, 400, 18, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 40000)].tobytes())
    for i, m in enumerate(base):
        site = target_of_mirna(m, i % 2)
        text[i * 100:i * 100 + len(site)] = site
    write_fasta(tmp_path / "t.fa", [("t", bytes(text))])
    pick = rng.randint(0, 400, 70000)
    (tmp_path / "m.fa").write_bytes(b"".join(b">m%d\n%s\n" % (i, base[p]) for i, p in enumerate(pick)))
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=3, both_strands=True)
    names, seqs = load_reference([tmp_path / "t.fa"])
    per = {}
    for p in set(pick.tolist()):
        mc = MCODE[np.frombuffer(base[p], dtype=np.uint8)]
        per[p] = sorted(sites_numpy(mc, seqs[0], 3, True, False), key=lambda s: (s[0], s[1], s[2]))
    want = [HEADER]
    for i, p in enumerate(pick):
        mc = MCODE[np.frombuffer(base[p], dtype=np.uint8)]
        for half, o, strand, C, Y in per[p]:
            want.append(_line(b"m%d" % i, "t", o, len(mc), strand, half, mc, C, Y))
    assert res["sites"] >= 70000
    assert got == b"".join(want)


def test_capacity_overflow(gpu_ctx, tmp_path):
    """A capacity of 40 keys: passes by (miRNA, score), and one (miRNA, score) with 150 sites split by offsets; with and without -k."""
    rng = np.random.RandomState(8)
    mirs = random_mirnas(rng, 6, 14, 24, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, 30000)].tobytes())
    for i in range(150):
        site = target_of_mirna(mirs[0], i % 2)
        text[150 * i:150 * i + len(site)] = site
    for m in mirs[1:]:
        plant(rng, text, m, 30, subs=(0, 2))
    write_fasta(tmp_path / "t.fa", [("a", bytes(text[:14000])), ("b", bytes(text[14000:]))])
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    try:
        # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change
        for cap, kw, passes in ((40, _kw(6, True), 12), (40, _kw(6, True, k=70), 12), (2, _kw(4, False, True), 120), (40, _kw(8, True, k=5), 10),
                                (0, _kw(6, True), 1)):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], **kw[0])
            assert got == restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], **kw[1]), (cap, kw)
            assert (res["passes"] > 3) == (cap > 0), (cap, res)
            assert res["passes"] == passes, (cap, kw, res)
    finally:
        gpu_ctx.set_target_capacity(0)


def test_positions_past_2_31(gpu_ctx, tmp_path):
    rng = np.random.RandomState(9)
    pad = 2 ** 31 + 777
    mirs = random_mirnas(rng, 20, 18, 24, t_for_u=0.0)
    tail = bytearray(ACGT[rng.randint(0, 4, 200000)].tobytes())
    other = bytearray(ACGT[rng.randint(0, 4, 20000)].tobytes())
    for m in mirs:
        plant(rng, tail, m, 4, subs=(0, 2))
        plant(rng, other, m, 2, subs=(0, 2))
    p = tmp_path / "big.fa"
    line = b"N" * 4095 + b"\n"
    with open(p, "wb") as f:
        f.write(b">big\n")
        left = pad
        while left >= 4095 * 16384:
            f.write(line * 16384)
            left -= 4095 * 16384
        f.write(b"N" * left + b"\n" + bytes(tail) + b"\n>other\n" + bytes(other) + b"\n")
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [p], max_half_score=8, both_strands=True, cleavage_site=True)
    os.unlink(p)
    assert res["bases"] == pad + len(tail) + len(other) > 2 ** 31
    write_fasta(tmp_path / "small.fa", [("big", bytes(tail)), ("other", bytes(other))])
    want = restate_files(tmp_path / "m.fa", [tmp_path / "small.fa"], max_half=8, both=True, cleavage=True).split(b"\n")
    for i in range(1, len(want) - 1):                # positions on `big` move by the N prefix
        f = want[i].split(b"\t")
        if f[1] == b"big":
            f[2], f[3] = b"%d" % (int(f[2]) + pad), b"%d" % (int(f[3]) + pad)
            want[i] = b"\t".join(f)
    assert got == b"\n".join(want)
    assert any(int(ln.split(b"\t")[2]) > 2 ** 31 for ln in got.split(b"\n")[1:-1])


def _chunked_sites(mc, t, max_half, both, chunk=1 << 19):
    L = len(mc)
    out = []
    for c0 in range(0, max(len(t) - L + 1, 0), chunk):
        for half, o, strand, C, Y in sites_numpy(mc, t[c0:c0 + chunk + L - 1], max_half, both, False):
            out.append((half, o + c0, strand, C, Y))
    return out


def test_2000_mirnas_on_50_mb(gpu_ctx, tmp_path):
    rng = np.random.RandomState(13)
    n = 50_000_000
    mirs = random_mirnas(rng, 2000, 20, 22, t_for_u=0.0)
    text = bytearray(ACGT[rng.randint(0, 4, n)].tobytes())
    slots = rng.choice(n // 64 - 1, size=3 * len(mirs), replace=False) * 64      # non-overlapping sites
    planted = []
    for i, m in enumerate(mirs):
        for j in range(3):
            o, strand = int(slots[3 * i + j]), j % 2
            site = bytearray(target_of_mirna(m, strand))
            if j == 2:
                site[int(rng.randint(0, len(site)))] = b"ACGT"[rng.randint(0, 4)]
            text[o:o + len(site)] = site
            planted.append((i, o, strand))
    write_fasta(tmp_path / "t.fa", [("chr1", bytes(text[:30_000_000])), ("chr2", bytes(text[30_000_000:]))], width=80)
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "t.fa"], max_half_score=6, both_strands=True)
    lines = got.split(b"\n")
    assert lines[0] + b"\n" == HEADER and lines[-1] == b""
    have = set()
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        off = int(f[2]) - 1 + (30_000_000 if f[1] == b"chr2" else 0)
        have.add((int(f[0][1:]), off, 1 if f[4] == b"-" else 0))
    assert all(p in have for p in planted)
    names, seqs = load_reference([tmp_path / "t.fa"])
    for i in (0, 999, 1999):
        mc = MCODE[np.frombuffer(mirs[i], dtype=np.uint8)]
        sites = []
        for tid, t in enumerate(seqs):
            sites += [(half, tid, o, strand, _line(b"m%d" % i, names[tid], o, len(mc), strand, half, mc, C, Y))
                      for half, o, strand, C, Y in _chunked_sites(mc, t, 6, True)]
        want = [s[4].rstrip(b"\n") for s in sorted(sites, key=lambda s: s[:4])]
        assert [ln for ln in lines[1:-1] if ln.startswith(b"m%d\t" % i)] == want


def test_refusals_write_nothing(gpu_ctx, tmp_path):
    from mir_prefer_amd import capi
    good_t = tmp_path / "t.fa"
    good_t.write_bytes(b">t\n" + b"ACGT" * 100 + b"\n")
    m12 = b"ACGUACGUACGU"
    cases = [(b">a\n" + m12 + b"\n>b\n" + b"A" * 11 + b"\n", None, "record 2: the sequence has 11 nt"),
             (b">a\n" + m12 + b"\n>b\n" + b"A" * 33 + b"\n", None, "record 2: the sequence has 33 nt"),
             (b">a\n" + m12 + b"\n>  \t\n" + m12 + b"\n", None, "record 2: a header without a name"),
             (b">a\n" + m12 + b"\n>b\n" + m12 + "é\n".encode(), None, "record 2: a byte >= 0x80"),
             (">é\n".encode() + m12 + b"\n", None, "record 1: a byte >= 0x80"),
             (b">a\n" + m12 + b"\n", b">t\nACGT\n>t\nACGT\n", "duplicate contig name t"),
             (b">a\n" + m12 + b"\n", b">\nACGT\n", "a header without a contig name")]
    for mdata, tdata, msg in cases:
        (tmp_path / "m.fa").write_bytes(mdata)
        t = tmp_path / "bad_t.fa"
        t.write_bytes(tdata or good_t.read_bytes())
        out = tmp_path / "out.tsv"
        out.write_bytes(b"stale\n")
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.target_scan(str(tmp_path / "m.fa"), [str(t)], str(out))
        assert msg in str(e.value), (msg, str(e.value))
        assert not out.exists()
    # more than 2^24 miRNAs: the record after the limit is named
    with open(tmp_path / "many.fa", "wb") as f:
        rec = b">a\n" + m12 + b"\n"
        f.write(rec * (1 << 20) * 16 + rec)
    out = tmp_path / "out.tsv"
    out.write_bytes(b"stale\n")
    with pytest.raises(capi.MirpError) as e:
        gpu_ctx.target_scan(str(tmp_path / "many.fa"), [str(good_t)], str(out))
    assert "record 16777217: more than 16,777,216 miRNAs" in str(e.value) and not out.exists()
    os.unlink(tmp_path / "many.fa")
    # empty inputs are not refused: a header line only
    (tmp_path / "m.fa").write_bytes(b"")
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [good_t])
    assert got == HEADER and res["mirnas"] == 0
    (tmp_path / "m.fa").write_bytes(b">a\n" + m12 + b"\n")
    (tmp_path / "e.fa").write_bytes(b">e\n\n")
    got, res = _scan(gpu_ctx, tmp_path, tmp_path / "m.fa", [tmp_path / "e.fa"])
    assert got == HEADER and res["targets"] == 0


def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli(small, tmp_path):
    shutil.copy(small / "m.fa", tmp_path / "m.fa")
    paths = [str(small / "t1.fa"), str(small / "t2.fa")]
    r = _cli(["-s", "2.5", "-b", "-c", "-k", "4", str(tmp_path / "m.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_files(tmp_path / "m.fa", paths, max_half=5, both=True, cleavage=True, k=4)
    assert (tmp_path / "m.fa.targets.tsv").read_bytes() == want
    n = want.count(b"\n") - 1
    assert r.stderr.decode().splitlines() == ["Warning: contig empty in %s has length 0 and is dropped." % paths[0],
                                              "targets: 30 miRNAs, 3 targets, %d bases scanned (both strands), %d sites written to %s" % (
                                                  9000 + 4000 + 6000, n, tmp_path / "m.fa.targets.tsv")]
    r = _cli(["-o", str(tmp_path / "x.tsv"), str(tmp_path / "m.fa"), paths[1]], tmp_path)
    assert r.returncode == 0 and (tmp_path / "x.tsv").read_bytes() == restate_files(tmp_path / "m.fa", [paths[1]], max_half=8)
    # a refused run: status 255, no output (also not the old one)
    (tmp_path / "bad.fa").write_bytes(b">a\nACGU\n")
    (tmp_path / "bad.fa.targets.tsv").write_bytes(b"stale\n")
    r = _cli([str(tmp_path / "bad.fa")] + paths, tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and "record 1: the sequence has 4 nt" in r.stderr.decode()
    assert not (tmp_path / "bad.fa.targets.tsv").exists()


def test_chain_pipeline_mature_to_own_locus(tmp_path):
    """cli pipeline on the golden `mini` dataset, then targets -b -s 0 of its mature.fa against the genome: every mature whose text is all ACGU
    reports its own locus as a score-0 site, on the strand opposite the locus' strand."""
    from tests.test_cli_gpu import _setup
    exp, cfg, out = _setup("mini", tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.cli", "pipeline", cfg], cwd=str(tmp_path), capture_output=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr.decode()
    prefix = exp["config"]["NAME_PREFIX"]
    mature = out / (prefix + "_miRNA.mature.fa")
    r = _cli(["-b", "-s", "0", str(mature), str(tmp_path / "genome.fa")], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    rows = {}
    for ln in open(str(mature) + ".targets.tsv", "rb").read().split(b"\n")[1:-1]:
        f = ln.split(b"\t")
        rows.setdefault(f[0], set()).add((f[1], int(f[2]), int(f[3]), f[4], f[5]))
    text = mature.read_bytes().split(b"\n")
    checked = 0
    for h, s in zip(text[0::2], text[1::2]):
        if not h.startswith(b">"):
            continue
        name = h[1:].strip()
        loc, strand = name.split(b" ")[:2]
        chrom, span = loc.rsplit(b":", 1)
        a, b = (int(x) for x in span.split(b"-"))
        if set(s) - set(b"ACGU"):
            continue
        assert (chrom, a, b, b"-" if strand == b"+" else b"+", b"0.0") in rows.get(name, set()), name
        checked += 1
    assert checked >= 40
