"""GPU tests of the known-miRNA annotation (mirp_annotate_scan, annotate_kernels.hip): both output files byte for byte against the
restatements of tests/test_annotate_cpu.py over a grid of -m / -e / -k on a mixed input; more queries than one key group and more known sequences
than queries (lanes on either side); forced key capacities; 200,000 queries against 50,000 known sequences with planted relatives; refusals and
degenerate inputs; the command line; and the chains cli pipeline -> mature.fa -> annotate and reads collapse -> annotate."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_annotate_cpu import (CLASSES, HEADER, ROOT, KnownMatrix, blocks_numpy, fasta_bytes, make_mixed, parse_known, random_seq, restate_files,
                                     summary_name)
from tests.test_targets_cpu import parse_mirnas

pytestmark = pytest.mark.gpu


def _scan(ctx, tmp_path, query_path, known_paths, E=2, M=2, k=0, species=()):
    out = tmp_path / "got.annot.tsv"
    summ = tmp_path / "got.annot.summary.tsv"
    res = ctx.annotate_scan(str(query_path), [str(p) for p in known_paths], str(out), str(summ), max_offset=E, max_mismatches=M, max_lines=k,
                            species=species)
    return out.read_bytes(), summ.read_bytes(), res


def _check_stats(res, counts):
    assert (res["queries"], res["known"], res["skipped"], res["hits"], res["lines"]) == (counts["queries"], counts["known"], counts["skipped"],
                                                                                          counts["hits"], counts["lines"]), (res, counts)
    assert [res[c.decode()] for c in CLASSES] == counts["classes"], (res, counts)
    assert res["pairs"] == counts["queries"] * counts["known"]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("annotate_small")
    qd, kds = make_mixed(11, 300, 260)
    (d / "q.fa").write_bytes(qd)
    (d / "k1.fa").write_bytes(kds[0])
    (d / "k2.fa").write_bytes(kds[1])
    return d


def test_grid_matches_the_restatement(gpu_ctx, small, tmp_path):
    paths = [small / "k1.fa", small / "k2.fa"]
    total = 0
    for M, E, k in itertools.product((0, 1, 2, 4, 6), (0, 1, 2, 4), (0, 1, 3)):
        hits, summ, res = _scan(gpu_ctx, tmp_path, small / "q.fa", paths, E=E, M=M, k=k)
        w_hits, w_summ, counts = restate_files(small / "q.fa", paths, E=E, M=M, k=k)
        assert hits == w_hits, (M, E, k)
        assert summ == w_summ, (M, E, k)
        _check_stats(res, counts)
        assert counts["skipped"] == 4 and res["evaluations"] <= res["pairs"] * (2 * E + 1)
        if k == 0:
            total += counts["hits"]
        if (M, E) in ((2, 2), (6, 4), (0, 0)) and k in (0, 3):
            assert (hits, summ) == restate_files(small / "q.fa", paths, numpy=False, E=E, M=M, k=k)[:2], (M, E, k)
    print("hits over the grid (k = 0):", total)
    assert total > 1000
    # --species, and one file only
    for species in (["ath"], ["cel", "osa", "nope"]):
        hits, summ, res = _scan(gpu_ctx, tmp_path, small / "q.fa", paths, E=4, M=6, species=species)
        w = restate_files(small / "q.fa", paths, species=[s.encode() for s in species], E=4, M=6)
        assert (hits, summ) == w[:2]
        _check_stats(res, w[2])
        assert 0 < res["known"] < 261
    hits, summ, res = _scan(gpu_ctx, tmp_path, small / "q.fa", paths[1:], E=3, M=3, k=2)
    assert (hits, summ) == restate_files(small / "q.fa", paths[1:], E=3, M=3, k=2)[:2]


def test_evaluations_count_the_admissible_shifts(gpu_ctx, tmp_path):
    (tmp_path / "q.fa").write_bytes(b">a\n" + b"A" * 20 + b"\n>b\n" + b"C" * 23 + b"\n")
    (tmp_path / "k.fa").write_bytes(b">x\n" + b"A" * 20 + b"\n>y\n" + b"A" * 22 + b"\n>z\n" + b"A" * 30 + b"\n")
    _, _, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"], E=2)
    assert res["pairs"] == 6 and res["evaluations"] == (5 + 3 + 0) + (2 + 4 + 0)


def test_families_on_the_device_path(gpu_ctx, tmp_path):
    ids = [b"ath-miR156a-5p", b"osa-MIR2118b", b"cel-let-7-5p", b"novel_17", b"miR156a", b"MIR166", b"let-7", b"lin-4", b"cel-lin-4-3p", b"hsa-mir-21",
           b"hsa-Let-7a", b"miR156a-5p", b"bantam", b"dme-bantam-3p", b"ath-miR", b"mir-", b"a-b-miR1", b"x_1-miR5", b"ath-miRf10", b"LIN28", b"mir-let-7"]
    seq = b"UGACAGAAGAGAGUGAGCAC"
    (tmp_path / "q.fa").write_bytes(b">q\n" + seq + b"\n")
    (tmp_path / "k.fa").write_bytes(b"".join(b">" + i + b" description\n" + seq + b"\n" for i in ids))
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"])
    assert (hits, summ) == restate_files(tmp_path / "q.fa", [tmp_path / "k.fa"])[:2]
    assert res["hits"] == len(ids) and res["identical"] == 1


def test_more_queries_than_one_group_and_more_known_than_queries(gpu_ctx, tmp_path):
    rng = np.random.RandomState(3)
    known = [(b"ath-miR%d" % i, random_seq(rng, int(rng.randint(18, 25)))) for i in range(700)]
    nq = (1 << 16) * 2 + 1234                       # three key groups
    picks = rng.randint(0, len(known), nq)
    queries = []
    for i in range(nq):
        s = known[picks[i]][1] if i % 3 == 0 else random_seq(rng, int(rng.randint(18, 25)))
        if i % 6 == 0:
            s = s[1:] + b"A"
        queries.append((b"q%d" % i, s))
    (tmp_path / "q.fa").write_bytes(fasta_bytes(rng, queries))
    (tmp_path / "k.fa").write_bytes(fasta_bytes(rng, known))
    w_hits, w_summ, counts = restate_files(tmp_path / "q.fa", [tmp_path / "k.fa"])
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"])
    assert hits == w_hits and summ == w_summ
    _check_stats(res, counts)
    assert res["hits"] >= nq // 3 and res["passes"] == 3
    first, last = [], None                          # -k 1: the first line of every query (the names are unique here)
    for ln in w_hits.split(b"\n")[1:-1]:
        name = ln.split(b"\t", 1)[0]
        if name != last:
            first.append(ln + b"\n")
        last = name
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"], k=1)
    assert hits == HEADER + b"".join(first) and summ == w_summ
    _check_stats(res, dict(counts, lines=len(first)))
    # the other orientation: the known sequences on the lanes
    (tmp_path / "q2.fa").write_bytes(fasta_bytes(rng, queries[:150]))
    big = known + [(b"osa-miR%d" % i, random_seq(rng, int(rng.randint(18, 25)))) for i in range(70000)]
    (tmp_path / "k2.fa").write_bytes(fasta_bytes(rng, big))
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q2.fa", [tmp_path / "k2.fa"], E=3, M=3)
    w_hits, w_summ, counts = restate_files(tmp_path / "q2.fa", [tmp_path / "k2.fa"], E=3, M=3)
    assert hits == w_hits and summ == w_summ
    _check_stats(res, counts)


def test_forced_capacities_give_identical_files(gpu_ctx, small, tmp_path):
    paths = [small / "k1.fa", small / "k2.fa"]
    # one query with many hits in one (distance, mismatches) bin, next to the mixed input's queries
    seq = b"UGACAGAAGAGAGUGAGCAC"
    (tmp_path / "k3.fa").write_bytes(b"".join(b">ath-miR%d\n%s\n" % (i, seq if i % 3 else seq[:-1] + b"G") for i in range(130)))
    (tmp_path / "q.fa").write_bytes((small / "q.fa").read_bytes() + b">many\n" + seq + b"\n>tail\n" + seq[1:] + b"\n")
    paths.append(tmp_path / "k3.fa")
    # the pass counts are those of the hand-written pass loops that pass_plan.h replaced, recorded on an MI355X before the change: (E, M, k) -> capacity 0, 2, 40
    recorded = {(2, 2, 0): (1, 205, 21), (4, 6, 0): (1, 4616, 180), (4, 6, 3): (1, 361, 101), (2, 2, 1): (1, 71, 7), (2, 2, 50): (1, 119, 9),
                (2, 2, 100): (1, 175, 19)}
    try:
        for E, M, k in ((2, 2, 0), (4, 6, 0), (4, 6, 3), (2, 2, 1), (2, 2, 50), (2, 2, 100)):
            gpu_ctx.set_target_capacity(0)
            ref = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", paths, E=E, M=M, k=k)
            assert ref[:2] == restate_files(tmp_path / "q.fa", paths, E=E, M=M, k=k)[:2]
            assert ref[2]["passes"] <= 2 and ref[2]["passes"] == recorded[E, M, k][0]
            for cap, passes in zip((2, 40), recorded[E, M, k][1:]):
                gpu_ctx.set_target_capacity(cap)
                got = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", paths, E=E, M=M, k=k)
                assert got[0] == ref[0] and got[1] == ref[1], (E, M, k, cap)
                assert got[2]["passes"] > ref[2]["passes"] and got[2]["passes"] == passes, (E, M, k, cap, got[2])
                assert {x: got[2][x] for x in got[2] if x not in ("passes", "seconds")} == {x: ref[2][x] for x in ref[2] if x not in ("passes", "seconds")}
    finally:
        gpu_ctx.set_target_capacity(0)


def test_200000_queries_against_50000_known(gpu_ctx, tmp_path):
    rng = np.random.RandomState(2024)
    nk, nq, planted = 50000, 200000, 4000
    known = [(b"%s-miR%d" % (b"ath" if i % 2 else b"osa", i), random_seq(rng, int(rng.randint(18, 25)))) for i in range(nk)]
    assert len({s for _, s in known}) == nk
    queries, plan = [], {}
    where = set(rng.choice(nq, planted, replace=False).tolist())
    for i in range(nq):
        if i not in where:
            queries.append((b"read_%d_x%d" % (i, 1 + i % 7), random_seq(rng, int(rng.randint(18, 25)))))
            continue
        ki = int(rng.randint(0, nk))
        s = known[ki][1]
        kind = len(plan) % 4
        if kind == 0:                                   # a copy
            want = (b"identical", 0, 0, 0, 0)
        elif kind == 1:                                 # one nucleotide later at both ends
            s = s[1:] + b"ACGU"[rng.randint(0, 4):][:1]
            want = (b"isomir", 2, 0, 1, 1)
        elif kind == 2:                                 # two nucleotides shorter at the 3' end
            s = s[:-2]
            want = (b"isomir", 2, 0, 0, -2)
        else:                                           # one or two substitutions
            n = 1 + len(plan) // 4 % 2
            t = bytearray(s)
            for p in rng.choice(np.arange(3, len(s) - 3), n, replace=False):
                t[p] = b"ACGU"[(b"ACGU".index(t[p]) + 1 + int(rng.randint(0, 3))) % 4]
            s = bytes(t)
            want = (b"homolog", n, n, 0, 0)
        plan[i] = (ki, want)
        queries.append((b"planted_%d" % i, s))
    (tmp_path / "q.fa").write_bytes(fasta_bytes(rng, queries))
    (tmp_path / "k.fa").write_bytes(fasta_bytes(rng, known))
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"])
    print("scale:", {x: res[x] for x in res if x != "seconds"}, ["%.3f" % s for s in res["seconds"]])
    srows = summ.split(b"\n")
    assert srows[-1] == b"" and len(srows) == nq + 1 and res["queries"] == nq and res["known"] == nk and res["pairs"] == nq * nk
    assert hits.startswith(HEADER)
    for i, (ki, (cls, dist, mm, o5, o3)) in plan.items():
        f = srows[i].split(b"\t")
        assert f[0] == b"planted_%d" % i and f[2] == cls and f[3] == known[ki][0] and f[4] == b"miR%d" % ki, (i, f)
        assert [int(x) for x in f[5:9]] == [dist, mm, o5, o3], (i, f)
    assert res["identical"] >= planted // 4 and res["novel"] <= nq - planted and res["novel"] + res["identical"] + res["isomir"] + res["homolog"] == nq
    # the line blocks of 200 sample queries (planted ones among them) against the numpy restatement
    parsed_q = parse_mirnas((tmp_path / "q.fa").read_bytes())
    parsed_k, _ = parse_known([(tmp_path / "k.fa").read_bytes()])
    sample = sorted(set(rng.choice(nq, 160, replace=False).tolist()) | set(sorted(where)[:40]))
    blocks = {}
    for ln in hits[len(HEADER):].split(b"\n")[:-1]:
        blocks.setdefault(ln.split(b"\t", 1)[0], []).append(ln + b"\n")
    K = KnownMatrix(parsed_k)
    for qi, (lines, sline, n, cls) in zip(sample, blocks_numpy(parsed_q, parsed_k, only=sample, K=K)):
        assert b"".join(blocks.get(parsed_q[qi][0], [])) == lines, qi
        assert srows[qi] + b"\n" == sline, qi
    assert sum(len(v) for v in blocks.values()) == res["lines"] == res["hits"]


def test_refusals_write_nothing(gpu_ctx, tmp_path):
    from mir_prefer_amd import capi
    s12 = b"ACGUACGUACGU"
    good_q = b">a\n" + s12 + b"\n"
    good_k = b">ath-miR1\n" + s12 + b"\n"
    cases = [(b">a\n" + s12 + b"\n>b\n" + b"A" * 11 + b"\n", good_k, "q.fa: record 2: the sequence has 11 nt"),
             (b">a\n" + s12 + b"\n>b\n" + s12 + "é\n".encode(), good_k, "q.fa: record 2: a byte >= 0x80"),
             (good_q, good_k + b">b\n" + b"A" * 40 + b"\n>c\n" + s12 + b"\xff\n", "k.fa: record 3: a byte >= 0x80"),
             (good_q, good_k + ">é x\n".encode() + s12 + b"\n", "k.fa: record 2: a byte >= 0x80"),
             (b">a\n" + s12 + b"\n>  \t\n" + s12 + b"\n", good_k, "q.fa: record 2: a header without a name"),
             (good_q, good_k + b">\n" + s12 + b"\n", "k.fa: record 2: a header without a name")]
    for qdata, kdata, msg in cases:
        (tmp_path / "q.fa").write_bytes(qdata)
        (tmp_path / "k.fa").write_bytes(kdata)
        out, summ = tmp_path / "out.tsv", tmp_path / "out.summary.tsv"
        out.write_bytes(b"stale\n")
        summ.write_bytes(b"stale\n")
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.annotate_scan(str(tmp_path / "q.fa"), [str(tmp_path / "k.fa")], str(out), str(summ))
        assert msg in str(e.value), (msg, str(e.value))
        assert not out.exists() and not summ.exists()
    with pytest.raises(capi.MirpError):
        gpu_ctx.annotate_scan(str(tmp_path / "q.fa"), [str(tmp_path / "k.fa")], str(tmp_path / "o"), str(tmp_path / "s"), max_offset=5)
    with pytest.raises(capi.MirpError):
        gpu_ctx.annotate_scan(str(tmp_path / "q.fa"), [str(tmp_path / "k.fa")], str(tmp_path / "o"), str(tmp_path / "s"), max_mismatches=7)


def test_degenerate_inputs_are_not_refusals(gpu_ctx, tmp_path):
    s = b"UGACAGAAGAGAGUGAGCAC"
    (tmp_path / "q.fa").write_bytes(b">a x\n" + s + b"\n>b\n" + s[:15] + b"\n")
    novel = b"a x\t20\tnovel\t.\t.\t.\t.\t.\t.\t0\nb\t15\tnovel\t.\t.\t.\t.\t.\t.\t0\n"
    for kdata, skipped in ((b"", 0), (b">x\n" + b"A" * 11 + b"\n>y\n" + b"A" * 33 + b"\n>z\n", 3), (b"no header\n", 0)):
        (tmp_path / "k.fa").write_bytes(kdata)
        hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"])
        assert hits == HEADER and summ == novel
        assert (res["queries"], res["known"], res["skipped"], res["hits"], res["novel"], res["pairs"]) == (2, 0, skipped, 0, 2, 0)
    # a species that no id has, no query, and no hit at all
    (tmp_path / "k.fa").write_bytes(b">ath-miR1\n" + s + b"\n")
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"], species=["osa"])
    assert hits == HEADER and summ == novel and res["known"] == 0
    (tmp_path / "e.fa").write_bytes(b"")
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "e.fa", [tmp_path / "k.fa"])
    assert hits == HEADER and summ == b"" and res["queries"] == 0 and res["known"] == 1
    (tmp_path / "k.fa").write_bytes(b">ath-miR1\n" + b"C" * 20 + b"\n")
    hits, summ, res = _scan(gpu_ctx, tmp_path, tmp_path / "q.fa", [tmp_path / "k.fa"])
    assert hits == HEADER and summ == novel and res["passes"] == 0


def _cli(module, args, cwd, timeout=900):
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), capture_output=True, timeout=timeout, env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli(small, tmp_path):
    (tmp_path / "q.fa").write_bytes((small / "q.fa").read_bytes())
    paths = [str(small / "k1.fa"), str(small / "k2.fa")]
    r = _cli("mir_prefer_amd.annotate", ["-e", "3", "-m", "4", "-k", "2", "--species", "ath,cel", str(tmp_path / "q.fa")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    w_hits, w_summ, c = restate_files(tmp_path / "q.fa", paths, species=[b"ath", b"cel"], E=3, M=4, k=2)
    assert (tmp_path / "q.fa.annot.tsv").read_bytes() == w_hits and (tmp_path / "q.fa.annot.summary.tsv").read_bytes() == w_summ
    assert r.stderr.decode().splitlines() == [
        "annotate: %d queries, %d known sequences kept (4 skipped), %d pairs, %d hits; %d identical, %d isomir, %d homolog, %d novel; written to %s and %s"
        % (c["queries"], c["known"], c["queries"] * c["known"], c["hits"], c["classes"][0], c["classes"][1], c["classes"][2], c["classes"][3],
           tmp_path / "q.fa.annot.tsv", tmp_path / "q.fa.annot.summary.tsv")]
    r = _cli("mir_prefer_amd.annotate", ["-o", str(tmp_path / "x.out"), str(tmp_path / "q.fa"), paths[1]], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    w = restate_files(tmp_path / "q.fa", [paths[1]])
    assert (tmp_path / "x.out").read_bytes() == w[0] and (tmp_path / "x.out.summary.tsv").read_bytes() == w[1]
    assert summary_name(str(tmp_path / "x.out")) == str(tmp_path / "x.out.summary.tsv")
    # a refused run: status 255, neither output (also not the old ones)
    (tmp_path / "bad.fa").write_bytes(b">a\nACGU\n")
    (tmp_path / "bad.fa.annot.tsv").write_bytes(b"stale\n")
    (tmp_path / "bad.fa.annot.summary.tsv").write_bytes(b"stale\n")
    r = _cli("mir_prefer_amd.annotate", [str(tmp_path / "bad.fa")] + paths, tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and "record 1: the sequence has 4 nt" in r.stderr.decode()
    assert not (tmp_path / "bad.fa.annot.tsv").exists() and not (tmp_path / "bad.fa.annot.summary.tsv").exists()


def test_chain_pipeline_mature_to_known(tmp_path):
    """cli pipeline on the golden `mini` dataset, then annotate of its mature.fa against a known file built from those sequences: copies, copies
    extended at the 3' end, copies with one substitution, and unrelated sequences.  The classes come out as constructed."""
    from tests.test_cli_gpu import _setup
    exp, cfg, out = _setup("mini", tmp_path)
    r = _cli("mir_prefer_amd.cli", ["pipeline", cfg], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    mature = out / (exp["config"]["NAME_PREFIX"] + "_miRNA.mature.fa")
    queries = parse_mirnas(mature.read_bytes())
    assert len(queries) >= 40
    rng = np.random.RandomState(5)
    letters = [bytes(b"ACGUN"[c] for c in cd) for _, cd in queries]
    seen, want, known = {}, {}, []
    for i, s in enumerate(letters):
        if s in seen or b"N" in s or len(s) > 30:
            continue
        seen[s] = i
        kind = len(seen) % 4
        if kind == 0:
            continue                                      # left out of the known file
        if kind == 1:
            known.append((b"ath-miR%da" % (100 + i), s))
            want[s] = (b"identical", b"ath-miR%da" % (100 + i), b"miR%d" % (100 + i))
        elif kind == 2:
            known.append((b"osa-MIR%db" % (100 + i), s + b"AG"))
            want[s] = (b"isomir", b"osa-MIR%db" % (100 + i), b"miR%d" % (100 + i))
        else:
            p = len(s) // 2
            t = s[:p] + b"ACGU"[(b"ACGU".index(s[p:p + 1]) + 1) % 4:][:1] + s[p + 1:]
            known.append((b"zma-miR%dc-3p" % (100 + i), t))
            want[s] = (b"homolog", b"zma-miR%dc-3p" % (100 + i), b"miR%d" % (100 + i))
    for i in range(50):
        known.append((b"unrelated-%d" % i, b"CCCCGGGG" + random_seq(rng, 14)))
    (tmp_path / "known.fa").write_bytes(fasta_bytes(rng, known))
    r = _cli("mir_prefer_amd.annotate", [str(mature), str(tmp_path / "known.fa")], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    w = restate_files(mature, [tmp_path / "known.fa"])
    assert open(str(mature) + ".annot.tsv", "rb").read() == w[0]
    summ = open(str(mature) + ".annot.summary.tsv", "rb").read()
    assert summ == w[1]
    checked = 0
    for (name, _), s, ln in zip(queries, letters, summ.split(b"\n")):
        f = ln.split(b"\t")
        assert f[0] == name
        if s in want:
            assert (f[2], f[3], f[4]) == want[s], ln
            checked += 1
        elif seen.get(s) is not None and b"N" not in s:
            assert f[2] == b"novel", ln
    assert checked >= 30


def test_chain_collapsed_reads_as_queries(tmp_path):
    """reads collapse output as the query file, -k 1: the known-miRNA profile of a library."""
    rng = np.random.RandomState(9)
    known = [(b"ath-miR%d" % i, random_seq(rng, 21)) for i in range(40)]
    reads = []
    for i in range(3000):
        s = known[int(rng.randint(0, 40))][1] if i % 2 else random_seq(rng, int(rng.randint(18, 25)))
        if i % 10 == 1:
            s = s[:-1]
        reads.append((b"r%d" % i, s.replace(b"U", b"T")))
    (tmp_path / "lib.fa").write_bytes(fasta_bytes(rng, reads))
    (tmp_path / "known.fa").write_bytes(fasta_bytes(rng, known))
    (tmp_path / "names.txt").write_text("LIB\n")
    r = _cli("mir_prefer_amd.reads", ["collapse", "names.txt", "lib.fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    r = _cli("mir_prefer_amd.annotate", ["-k", "1", "lib.fa.processed", "known.fa"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    w = restate_files(tmp_path / "lib.fa.processed", [tmp_path / "known.fa"], k=1)
    assert (tmp_path / "lib.fa.processed.annot.tsv").read_bytes() == w[0]
    assert (tmp_path / "lib.fa.processed.annot.summary.tsv").read_bytes() == w[1]
    assert w[2]["classes"][0] >= 40 and w[2]["classes"][1] >= 40 and w[2]["classes"][3] > 1000
    assert w[0].count(b"\n") - 1 == w[2]["queries"] - w[2]["classes"][3]
