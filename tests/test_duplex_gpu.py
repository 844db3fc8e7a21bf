"""GPU tests of the two-strand fold (mirp_duplex_batch, duplex_kernels.hip) and of `targets -e`: the device's energies, record
fields and structure bytes against the plain-Python restatement of tests/test_duplex_cpu.py (pinned there to §21's values, to the CPU oracle and
to the enumeration of every chain) over the largest and smallest shapes, 500 seeded pairs, the loop-limit cases, unknown letters, unbound pairs,
batch sizes and forced pass capacities, with the refusals; and whole `targets -e` files against the existing restatements' lines plus the four
columns, over the option combinations, forced capacities and the command line.  The restatement's folds run in worker processes that are started
fresh (spawn), never forked from a process that holds a device context."""
import multiprocessing
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import test_duplex_cpu as R
from tests.test_duplex_cpu import MIR156, duplex, loop_limit_case, near_complement, random_strand, revcomp_rna, seeded_pairs
from tests.test_targets_bulge_cpu import all_sites_numpy, emit, plant_bulged
from tests.test_targets_cpu import ACGT, ROOT, load_reference, parse_mirnas, plant, random_mirnas, restate_numpy, target_of_mirna, write_fasta

pytestmark = pytest.mark.gpu
FIELDS = ("mfe", "pairs", "a_first", "a_last", "b_first", "b_last")


@pytest.fixture(scope="module")
def fold_many():
    with multiprocessing.get_context("spawn").Pool(12) as pool:
        yield lambda pairs: pool.starmap(duplex, pairs, chunksize=8)


def _check(ctx, pairs, want, **kw):
    recs, ss = ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs], **kw)
    assert len(recs) == len(ss) == len(pairs)
    for q, (w, (a, b)) in enumerate(zip(want, pairs)):
        assert tuple(int(recs[q][f]) for f in FIELDS) == tuple(w[f] for f in FIELDS), (q, a, b, recs[q], w)
        assert ss[q] == w["structure"], (q, a, b, ss[q], w["structure"])
    return recs, ss


# ---------------------------------------------------------------------------------------------------- duplex_batch
def test_pins_on_the_device(gpu_ctx):
    rc = revcomp_rna(MIR156)
    pairs = [("GGGG", "CCCC"), ("A", "U"), ("AAAA", "AAAA"), (MIR156, rc), (MIR156, "A" + rc + "A"), (MIR156, "CGUGCUCUCUCUCUUCUGUCAU")]
    recs, ss = gpu_ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs])
    assert recs["mfe"].tolist() == [-580, 0, 0, -3720, -3840, -3340]
    assert ss[0] == b"((((&))))" and ss[1] == b".&." and ss[2] == b"....&...." and ss[3] == b"(" * 20 + b"&" + b")" * 20
    assert [tuple(int(recs[1][f]) for f in FIELDS), tuple(int(recs[3][f]) for f in FIELDS)] == [(0, 0, 0, 0, 0, 0), (-3720, 20, 1, 20, 1, 20)]
    assert gpu_ctx.duplex_last_stats()["pairs"] == 6 and gpu_ctx.duplex_last_stats()["passes"] == 1


def test_extreme_shapes(gpu_ctx, fold_many):
    rng = np.random.RandomState(41)
    pairs = []
    for la, lb in ((1, 1), (1, 64), (64, 1), (64, 64), (32, 35)):
        for rep in range(3):
            a = random_strand(rng, la)
            if rep == 0:
                b = random_strand(rng, lb)
            else:                                            # a near-complement cut or padded to the shape
                b = near_complement(rng, a, edits=4)
                b = (b + random_strand(rng, lb))[:lb]
            pairs.append((a, b))
    pairs += [("G" * 64, "C" * 64), ("G", "C" * 64), ("GU" * 32, "AC" * 32), ("G" * 32 + "A" * 30 + "GG", "CC" + "C" * 32)]
    want = fold_many(pairs)
    assert min(w["mfe"] for w in want) < -8000 and sum(w["pairs"] == 0 for w in want) >= 2
    _check(gpu_ctx, pairs, want)


def test_500_seeded_pairs(gpu_ctx, fold_many):
    pairs = seeded_pairs(11, 500)
    want = fold_many(pairs)
    loops = sum(1 for w in want if b".(" in w["structure"] or b")." in w["structure"].rstrip(b"."))
    print("bound %d of %d, with an interior loop or bulge %d, evaluations %d" % (sum(w["mfe"] < 0 for w in want), len(want), loops, sum(w["evals"] for w in want)))
    assert sum(w["mfe"] < 0 for w in want) > 300 and loops > 100
    _check(gpu_ctx, pairs, want)
    assert gpu_ctx.duplex_last_stats()["evaluations"] == sum(w["evals"] for w in want)


def test_loop_limit_letters_and_unbound(gpu_ctx, fold_many):
    pairs = [loop_limit_case(30), loop_limit_case(31), ("CCCCCCCCCC", loop_limit_case(30)[0]), ("CCCCCCCCCC", loop_limit_case(31)[0]),
             ("GGNGG", "CCNCC"), ("ggggtt", "aacccc"), ("GGGGTT", "AACCCC"), ("GGGGUUxRY-", "..AACCCC"), ("NNNN", "NNNN"), ("acgu", "ACGT"),
             ("A", "U"), ("G", "C"), ("AAAA", "AAAA"), ("AU", "AU"), ("GGG", "CCCCCC"), ("GGGGGG", "ACCCA"), ("GGG", "CCCCC")]
    want = fold_many(pairs)
    assert want[0]["pairs"] == 10 and want[1]["pairs"] == 5 and want[2]["pairs"] == 10 and want[3]["pairs"] == 5
    assert want[5] == want[6] and want[8]["mfe"] == 0 and want[10]["mfe"] == 0
    _check(gpu_ctx, pairs, want)


def test_batch_sizes_and_capacities(gpu_ctx, fold_many):
    pairs = seeded_pairs(12, 257, la=(1, 40), lb=(1, 40))
    want = fold_many(pairs)
    for n in (1, 3, 257):
        _check(gpu_ctx, pairs[:n], want[:n])
    base, ss0 = gpu_ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs])
    for cap, n in ((1, 23), (4, 257), (256, 257)):
        recs, ss = _check(gpu_ctx, pairs[:n], want[:n], capacity=cap)
        assert recs.tobytes() == base[:n].tobytes() and ss == ss0[:n]
        assert gpu_ctx.duplex_last_stats()["passes"] == (n + cap - 1) // cap
    recs, ss = gpu_ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs], structures=False)
    assert ss is None and recs.tobytes() == base.tobytes()
    recs, ss = gpu_ctx.duplex_batch([], [])
    assert len(recs) == 0 and ss == []


def test_the_fold_model_does_not_change_it(gpu_ctx):
    pairs = seeded_pairs(13, 40)
    base, ss0 = gpu_ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs])
    gpu_ctx.set_fold_model("vienna-1.8.5")
    try:
        recs, ss = gpu_ctx.duplex_batch([a for a, _ in pairs], [b for _, b in pairs])
    finally:
        gpu_ctx.set_fold_model("vienna-2.1.2")
    assert recs.tobytes() == base.tobytes() and ss == ss0


def test_refusals(gpu_ctx):
    from mir_prefer_amd import capi
    for a_list, b_list, what in ((["ACGU", ""], ["ACGU", "A"], "pair 2: strand a has 0 nt"), (["A", "C", "G"], ["U", "G", "C" * 65], "pair 3: strand b has 65 nt"),
                                 (["A" * 65], ["U"], "pair 1: strand a has 65 nt"), (["A"], [""], "pair 1: strand b has 0 nt")):
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.duplex_batch(a_list, b_list)
        assert what in str(e.value) and "(-10)" in str(e.value), str(e.value)
    recs, _ = gpu_ctx.duplex_batch(["A" * 64], ["U" * 64])
    assert recs["pairs"][0] > 0


# ---------------------------------------------------------------------------------------------------- targets -e
def _scan(ctx, tmp_path, mirna_path, target_paths, **kw):
    out = tmp_path / "out.tsv"
    res = ctx.target_scan(str(mirna_path), [str(p) for p in target_paths], str(out), **kw)
    return out.read_bytes(), res


@pytest.fixture(scope="module")
def energy_input(tmp_path_factory):
    """40 miRNAs (lengths 12..32, T for U, lower case, one with an unknown letter) over 20 kb in four contigs of two files, with ungapped and bulged
    sites planted on both strands and, by hand: a site at a contig's first base and one at a contig's last base, right before the next contig's
    first base, which starts another site; sites whose flank is N on either side; and a site of the miRNA with the unknown letter."""
    d = tmp_path_factory.mktemp("targets_energy")
    rng = np.random.RandomState(31)
    mirs = [random_mirnas(np.random.RandomState(100 + L), 1, L, L, t_for_u=0.3)[0] for L in (12, 15, 18, 19, 20, 21, 21, 22, 23, 24, 27, 32)]
    mirs += random_mirnas(rng, 27, 19, 24, lower=0.2)
    clean = random_mirnas(rng, 1, 21, 21, t_for_u=0.0)[0]
    mirs.append(clean[:17] + b"N" + clean[18:])
    texts = [bytearray(ACGT[rng.randint(0, 4, n)].tobytes()) for n in (6000, 5000, 3000, 6000)]
    for i, m in enumerate(mirs[:-1]):
        plant(rng, texts[i % 4], m, 1, subs=(0, 2))
        plant_bulged(rng, texts[(i + 1) % 4], m, 1, subs=(0, 1))
    texts[3][2000:2030] = b"N" * 30
    texts[1][700] = ord("R")
    edge = {}

    def put(t, o, m, strand, tag):
        site = target_of_mirna(m, strand)
        o = o if o >= 0 else len(texts[t]) + o - len(site) + 1
        texts[t][o:o + len(site)] = site
        edge[tag] = (t, o + 1, o + len(site))
    put(0, 0, mirs[5], 0, "first")
    put(0, -1, mirs[6], 1, "last")
    put(1, 0, mirs[7], 0, "after_boundary")
    put(2, 500, mirs[8], 0, "n_before")
    texts[2][499] = ord("N")
    put(2, 900, mirs[9], 1, "n_after")
    texts[2][900 + len(mirs[9])] = ord("n")
    put(3, 1000, clean, 0, "unknown")
    texts[3][3000:3400] = texts[3][3000:3400].lower()
    write_fasta(d / "t1.fa", [("chrB desc", bytes(texts[0])), ("chrA", bytes(texts[1]))])
    write_fasta(d / "t2.fa", [("tx.1", bytes(texts[2])), ("tx.2", bytes(texts[3]))], width=70)
    (d / "m.fa").write_bytes(b"".join(b">mir%d d\n%s\n" % (i, m) for i, m in enumerate(mirs)))
    return d, edge


OPTIONS = (dict(), dict(both_strands=True), dict(bulge=True), dict(bulge=True, both_strands=True, cleavage_site=True, max_sites=3))


def _plain(mirnas, names, seqs, kw):
    half, both, cleavage, k = kw.get("max_half_score", 8), kw.get("both_strands", False), kw.get("cleavage_site", False), kw.get("max_sites", 0)
    if kw.get("bulge"):
        return emit(all_sites_numpy(mirnas, names, seqs, cleavage, half), half, both, k)
    return restate_numpy(mirnas, names, seqs, max_half=half, both=both, cleavage=cleavage, k=k)


@pytest.fixture(scope="module")
def energy_want(energy_input, fold_many):
    """the expected file of every option combination: the existing restatement's lines plus the four columns"""
    d, _ = energy_input
    mirnas = parse_mirnas((d / "m.fa").read_bytes())
    names, seqs = load_reference([d / "t1.fa", d / "t2.fa"])
    assert len(mirnas) == 40 and names == ["chrB", "chrA", "tx.1", "tx.2"] and sum(len(s) for s in seqs) == 20000
    plain = [_plain(mirnas, names, seqs, kw) for kw in OPTIONS]
    need = set()
    for data in plain:                                       # every fold any of the files needs, once, in the pool
        R.add_energy(data, names, seqs, fold=lambda a, b: need.add((bytes(a), bytes(b))) or {"mfe": 0, "structure": b""})
    need = sorted(need)
    for key, r in zip(need, fold_many(need)):
        R._CACHE[key] = r
    return [R.add_energy(data, names, seqs) for data in plain]


def test_targets_energy_files(gpu_ctx, energy_input, energy_want, tmp_path):
    d, edge = energy_input
    paths = [d / "t1.fa", d / "t2.fa"]
    for kw, want in zip(OPTIONS, energy_want):
        got, res = _scan(gpu_ctx, tmp_path, d / "m.fa", paths, energy=True, **kw)
        assert got == want, kw
        assert res["sites"] == want.count(b"\n") - 1 > 30 and len(res["seconds"]) == 5
        # without -e: the same lines less the four columns
        plain, res0 = _scan(gpu_ctx, tmp_path, d / "m.fa", paths, **kw)
        assert plain == b"".join(b"\t".join(ln.split(b"\t")[:-4]) + b"\n" for ln in want.split(b"\n")[:-1])
        assert res0["sites"] == res["sites"] and res0["passes"] == res["passes"]
    # the planted edge cases are lines of the -b file, with the flanks the contig allows
    rows = {(f[1], int(f[2]), int(f[3])): f for f in (ln.split(b"\t") for ln in energy_want[1].split(b"\n")[1:-1])}
    names = [b"chrB", b"chrA", b"tx.1", b"tx.2"]
    flank = {"first": 1, "last": 1, "after_boundary": 1, "n_before": 2, "n_after": 2, "unknown": 2}
    for tag, (t, start, end) in edge.items():
        f = rows[(names[t], start, end)]
        L = end - start + 1
        assert len(f) == 15 and len(f[14]) == L + 1 + L + flank[tag], (tag, f)
        assert float(f[11]) < -10.0 and f[13] != b"NA", (tag, f)
    assert rows[(b"tx.2",) + edge["unknown"][1:]][8][17:18] == b"N"
    assert any(f[13].startswith(b"1.") for f in rows.values()) and any(f[13].startswith(b"0.") for f in rows.values())


def test_targets_energy_capacities(gpu_ctx, energy_input, energy_want, tmp_path):
    d, _ = energy_input
    paths = [d / "t1.fa", d / "t2.fa"]
    split = set()
    # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change, per capacity in the order of OPTIONS
    recorded = {4: (10, 19, 15, 27), 40: (1, 2, 2, 3)}
    try:
        for cap in (4, 40):
            gpu_ctx.set_target_capacity(cap)
            for kw, want, passes in zip(OPTIONS, energy_want, recorded[cap]):
                got, res = _scan(gpu_ctx, tmp_path, d / "m.fa", paths, energy=True, **kw)
                assert got == want, (cap, kw)
                # the keys of a run are at least its lines (-k cuts keys, not passes): more than one pass whenever they exceed the capacity
                lines = want.count(b"\n") - 1
                assert lines > 4
                assert res["passes"] == passes, (cap, kw, res)
                if lines > cap:
                    assert res["passes"] > 1, (cap, kw, res)
                    split.add(cap)
                elif not kw.get("max_sites"):
                    assert res["passes"] == 1, (cap, kw, res)
    finally:
        gpu_ctx.set_target_capacity(0)
    assert split == {4, 40}                                  # either capacity split at least one of the runs


def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_targets_energy_cli(energy_input, energy_want, tmp_path):
    d, _ = energy_input
    shutil.copy(d / "m.fa", tmp_path / "m.fa")
    paths = [str(d / "t1.fa"), str(d / "t2.fa")]
    r = _cli(["-e", "-g", "-b", "-c", "-k", "3", str(tmp_path / "m.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "m.fa.targets.tsv").read_bytes() == energy_want[3]
    assert r.stderr.decode().splitlines()[-1] == "targets: 40 miRNAs, 4 targets, 20000 bases scanned (both strands), %d sites written to %s" % (
        energy_want[3].count(b"\n") - 1, tmp_path / "m.fa.targets.tsv")
    r = _cli(["--energy", "-o", str(tmp_path / "x.tsv"), str(tmp_path / "m.fa")] + paths, tmp_path)
    assert r.returncode == 0 and (tmp_path / "x.tsv").read_bytes() == energy_want[0]
