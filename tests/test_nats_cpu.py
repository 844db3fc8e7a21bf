"""The definition of the NAT search without a GPU: the two statements of tests/nats_restatement.py against each other and against
plain recursions, the pinned cases, the writers of mir_prefer_amd.nats, its option errors, the header's declarations and the kernels' resources."""
import functools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import nats_cases as C
from tests import nats_restatement as R
from tests.test_targets_cpu import ROOT


def brief(recs):
    return [(r["a"], r["b"], r["score"], r["a_start"], r["a_end"], r["b_start"], r["b_end"], r["cigar"]) for r in recs]


@pytest.mark.parametrize("first", [0, 10, 20])
def test_the_two_statements_agree(first):
    found = 0
    for seed in range(first, first + 10):
        seqs, o = C.seeded_inputs(seed)
        assert len(seqs) <= 40 and max(len(s) for s in seqs) <= 400
        plain = R.find(seqs, **o)
        assert plain == R.find_numpy(seqs, **o)
        found += len(plain[0])
    assert found >= 5


def test_the_band_cut_is_the_band():
    for seed in (0, 5, 20):
        seqs, o = C.seeded_inputs(seed)
        assert R.find(seqs, cells=R.band_cells, **o) == R.find(seqs, **o)


def test_h_is_a_plain_recursion():
    """Sequences of 2..8 nt: bin 0 of W = 16 holds the whole matrix, so H is the unbanded recursion."""
    rng = random.Random(1)
    for _ in range(60):
        A, Bp = C.rand_seq(rng, rng.randint(2, 8), "ACGTN"), C.rand_seq(rng, rng.randint(2, 8), "ACGTN")
        match, mismatch, gap = rng.randint(1, 4), rng.randint(1, 4), rng.randint(1, 4)

        @functools.lru_cache(maxsize=None)
        def h(i, j):
            if i < 1 or j < 1:
                return 0
            s = match if A[i - 1] == Bp[j - 1] != "N" else -mismatch
            return max(0, h(i - 1, j - 1) + s, h(i - 1, j) - gap, h(i, j - 1) - gap)

        want = {(i, j): h(i, j) for i in range(1, len(A) + 1) for j in range(1, len(Bp) + 1)}
        assert R.band_cells(A, Bp, 0, 16, match, mismatch, gap) == want == R.band_cells_quick(A, Bp, 0, 16, match, mismatch, gap)
        ca, cb = R.np_codes(A), R.np_codes(Bp)
        Hs, delta, cells = R.np_band(ca, cb, 0, 16, match, mismatch, gap)
        assert cells == len(want)
        for (i, j), v in want.items():
            assert Hs[i + j, i - j - delta[0] + 1] == v
        # a band that does not hold the matrix: the cells beyond it count as 0
        narrow = R.band_cells(A + A + A, Bp + Bp + Bp + Bp, 1, 16, match, mismatch, gap)
        m = 4 * len(Bp)
        assert all(0 <= i - j + m - 1 <= 47 for i, j in narrow) and len(narrow) == sum(1 for i in range(1, 3 * len(A) + 1) for j in range(1, m + 1)
                                                                                         if 0 <= i - j + m - 1 <= 47)


def rescore(A, B, r, match, mismatch, gap):
    """The score of a record's cigar on the two transcripts, checking the letters it claims."""
    Bp = R.revcomp(R.letters(B))
    A = R.letters(A)
    i, j, score = r["a_start"], r["b_len"] + 1 - r["b_end"], 0
    for n, op in re.findall(r"(\d+)([=XID])", r["cigar"]):
        for _ in range(int(n)):
            if op in "=X":
                assert (A[i - 1] == Bp[j - 1] != "N") == (op == "=")
                score += match if op == "=" else -mismatch
                i, j = i + 1, j + 1
            elif op == "I":
                score -= gap
                i += 1
            else:
                score -= gap
                j += 1
    assert (i - 1, j - 1) == (r["a_end"], r["b_len"] + 1 - r["b_start"])
    return score


def test_cigars_rescore_and_end_in_pairs():
    n = 0
    for seed in range(30):
        seqs, o = C.seeded_inputs(seed)
        for r in R.find(seqs, **o)[0]:
            assert rescore(seqs[r["a"]], seqs[r["b"]], r, o["match"], o["mismatch"], o["gap"]) == r["score"]
            assert re.fullmatch(r"\d+=(\d+[=XID])*", r["cigar"]) and r["cigar"].endswith("=")
            assert r["a"] < r["b"] and r["score"] >= o["min_score"] and r["matches"] + r["mismatches"] + r["gaps"] >= o["min_length"]
            n += 1
    assert n >= 20


def test_pins():
    seqs, where = C.perfect_region()
    got, stats = R.find(seqs)
    assert brief(got) == [(0, 1, 360) + where + ("120=",)] and got[0]["seeds"] == 105 and got[0]["bin"] == (71 - (280 + 1 - 215) + 280 - 1) // 64
    # a seed that touches an unknown letter is none
    seqs, o, where = C.n_in_seed()
    got, stats = R.find(seqs, **o)
    assert stats["seed_hits"] == 9 and brief(got) == [(0, 1, 113) + where + ("20=1X19=",)]
    # f(v) = M is kept, f(v) = M + 1 is ignored, in either sense
    seqs, o = C.occurrence_edge()
    got, stats = R.find(seqs, max_occ=3, **o)
    assert [(r["a"], r["b"], r["cigar"]) for r in got] == [(0, 1, "16="), (1, 2, "16="), (1, 3, "16=")] and stats["kmers_ignored"] == 0
    got, stats = R.find(seqs, max_occ=2, **o)
    assert got == [] and stats["kmers_ignored"] == 2 and stats["seed_hits"] == 0
    # --min-seeds
    seqs, o, where = C.two_seeds()
    for min_seeds, n in ((1, 1), (2, 1), (3, 0)):
        got, stats = R.find(seqs, min_seeds=min_seeds, **o)
        assert len(got) == n and stats["seed_hits"] == 2 and stats["candidates"] == 1 and stats["kept_candidates"] == n
    # the end cell: the smallest i, then the smallest j
    (first, second), o = C.end_cell_ties()
    assert brief(R.find(first, **o)[0]) == [(0, 1, 90, 21, 50, 31, 60, "30=")]
    assert brief(R.find(second, **o)[0]) == [(0, 1, 90, 21, 50, 69, 98, "30=")]
    # the traceback: the diagonal, then (i - 1, j), then (i, j - 1)
    (first, second), o = C.traceback_ties()
    assert [r["cigar"] for r in R.find(first, **o)[0]] == ["20=1I21="]
    assert [r["cigar"] for r in R.find(second, **o)[0]] == ["20=1D1I20="]
    # one region of A against two copies in B: two records; the same region from two bins: one
    seqs, o = C.two_copies_in_b()
    assert brief(R.find(seqs, **o)[0]) == [(0, 1, 150, 61, 110, 41, 90, "50="), (0, 1, 150, 61, 110, 241, 290, "50=")]
    seqs, o = C.two_bins()
    got, stats = R.find(seqs, **o)
    assert brief(got) == [(0, 1, 228, 11, 91, 39, 118, "39=1I41=")] and stats["above"] == 2 and stats["candidates"] == 2 and got[0]["bin"] == 1


def test_mirror():
    """Tie-free planted inputs: with the two files swapped the hits keep their diagonals e and the regions their scores; the columns of a and b swap."""
    for seed in range(6):
        rng = random.Random(100 + seed)
        A, B = C.rand_seq(rng, rng.randint(150, 250)), C.rand_seq(rng, rng.randint(150, 250))
        A, B = C.plant(rng, A, rng.randint(5, 60), B, rng.randint(5, 60), C.rand_seq(rng, rng.randint(30, 80)))
        o = dict(seed=12, band=rng.choice([16, 32, 64]), min_score=60, min_length=20)
        one, two = R.find([A, B], **o)[0], R.find([B, A], **o)[0]
        assert len(one) == 1 and len(two) == 1
        r, s = one[0], two[0]
        assert (r["score"], r["seeds"], r["bin"], r["matches"]) == (s["score"], s["seeds"], s["bin"], s["matches"])
        assert (r["a_start"], r["a_end"], r["a_len"], r["b_start"], r["b_end"], r["b_len"]) == (s["b_start"], s["b_end"], s["b_len"], s["a_start"], s["a_end"],
                                                                                              s["a_len"])


def as_array(recs):
    from mir_prefer_amd import capi
    return np.array([tuple(r[f] for f in R.FIELDS) for r in recs], dtype=capi.NATS_DTYPE)


def test_writers_and_the_bed_parser(tmp_path):
    from mir_prefer_amd import loci, nats
    seqs = C.two_copies_in_b()[0] + C.perfect_region()[0]
    seqs[2], seqs[1] = C.plant(random.Random(9), seqs[2], 200, seqs[1], 120, "ACGGTCATTGCAGTCAGGCTTAACGTGCAACGTGGCATGCAAGTCCGTAA")
    names = ["tx1", "tx|2", "tx3", "tx4"]
    recs = R.find(seqs, seed=12, band=16, min_score=100, min_length=40)[0]
    assert [(r["a"], r["b"]) for r in recs] == [(0, 1), (0, 1), (1, 2), (2, 3)]
    arr, cigars = as_array(recs), [r["cigar"] for r in recs]
    assert nats.tsv_table(names, arr, cigars) == R.tsv_text(names, recs)
    assert nats.pairs_table(names, arr) == R.pairs_text(names, recs)
    assert nats.bed_table(names, arr) == R.bed_text(names, recs)
    assert nats.tsv_table(names, arr[:0], []) == nats.TSV_HEADER == R.TSV_HEADER and nats.pairs_table(names, arr[:0]) == nats.PAIRS_HEADER == R.PAIRS_HEADER
    assert nats.bed_table(names, arr[:0]) == ""
    lines = R.tsv_text(names, recs).splitlines()
    assert lines[1] == "NAT_1\ttx1\ttx|2\t150\t61\t110\t200\t41\t90\t400\t50\t0\t0\t100.00\t39\t50="
    assert [l.split("\t")[0] for l in lines[1:]] == ["NAT_1", "NAT_2", "NAT_3", "NAT_4"]
    # the two copies in tx|2 are one region of tx1: 50 covered positions of 200, 100 of 400
    assert R.pairs_text(names, recs).splitlines()[1] == "tx1\ttx|2\t2\t100\t50\t25.00\t100\t25.00"
    bed = tmp_path / "x.bed"
    bed.write_text(nats.bed_table(names, arr))
    got = loci.read_bed(str(bed))
    want = []
    for k, r in enumerate(recs):
        want.append(("NAT_%d_a" % (k + 1), ".", names[r["a"]], r["a_start"], r["a_end"], "+"))
        want.append(("NAT_%d_b" % (k + 1), ".", names[r["b"]], r["b_start"], r["b_end"], "+"))
    assert [g[:5] for g in got] == [w[:5] for w in want] and len({g[5] for g in got}) == 1
    assert nats.output_names("b") == ("b.tsv", "b.pairs.tsv", "b.bed")


def test_option_errors_need_no_binding(tmp_path, capsys):
    from mir_prefer_amd import nats
    f = str(tmp_path / "t.fa")
    o, files, base = nats.parse_args([f, f + "2"])
    assert (o.seed, o.band, o.max_occ, o.min_seeds, o.match, o.mismatch, o.gap, o.min_score, o.min_length, o.device) == (16, 64, 200, 1, 3, 4, 12, 200, 100, 0)
    assert files == [f, f + "2"] and base == f + ".nats"
    assert nats.parse_args(["-k", "12", "--band", "256", "--max-occ", "10000", "-s", "1", "-l", "1", "--gap", "50", "-o", "out", f])[2] == "out"
    bad = [[], ["-k", "11", f], ["-k", "25", f], ["--band", "48", f], ["--band", "512", f], ["--max-occ", "0", f], ["--max-occ", "10001", f],
           ["--min-seeds", "0", f], ["-s", "0", f], ["-l", "0", f], ["--match", "0", f], ["--match", "11", f], ["--mismatch", "0", f], ["--mismatch", "11", f],
           ["--gap", "0", f], ["--gap", "51", f], ["--device", "-1", f], ["-o", "", f], ["-x", f], ["-k", "x", f]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            nats.parse_args(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    probe = "import sys\nfrom mir_prefer_amd import nats\ntry:\n    nats.main(['-k', '5', %r])\nfinally:\n    print('capi' in ' '.join(sys.modules))\n" % f
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and b"Error: " not in r.stderr and r.stdout.strip() == b"False", (r.stdout, r.stderr)
    # a missing file is reported before a device is opened; the outputs of an earlier run are gone all the same
    stale = [f + ".nats" + ext for ext in (".tsv", ".pairs.tsv", ".bed")]
    for path in stale:
        open(path, "w").write("old\n")
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.nats", f], cwd=str(tmp_path), capture_output=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 255 and r.stderr.startswith(b"Error: file ") and not any(os.path.exists(path) for path in stale)


def test_abi_entries_are_declared():
    import ctypes
    from mir_prefer_amd import capi
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_nats_scan(", "mirp_set_nats_capacity(", "mirp_nats_last_stats(", "MirpNatsOpts", "MirpNatsRec"):
        assert name in header
    assert capi.ABI_VERSION == 17          # entries are only added
    m = re.search(r"typedef struct \{([^}]*)\} MirpNatsRec;", header)
    fields = [f.strip() for part in m.group(1).split(";") for f in part.replace("int32_t", "").split(",") if f.strip()]
    assert fields == list(capi.NATS_DTYPE.names) == list(R.FIELDS) and capi.NATS_DTYPE.itemsize == 56
    m = re.search(r"typedef struct \{([^}]*)\} MirpNatsOpts;", header)
    fields = [f.strip() for f in m.group(1).replace("int32_t", "").replace(";", "").split(",")]
    assert fields == [f for f, _ in capi.NatsOpts._fields_] and ctypes.sizeof(capi.NatsOpts) == 40
    assert int(re.search(r"#define MIRP_NATS_MAX_LEN\s+(\d+)", header).group(1)) == capi.NATS_MAX_LEN == R.MAX_LEN == 65535
    assert len(capi.NATS_STATS) == 15 and capi.NATS_STATS[:12] == R.STAT_NAMES and capi.NATS_FAMILY == 8
    assert hasattr(capi.Context, "nats_scan") and hasattr(capi.Context, "nats_last_stats")


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_kernels_use_no_scratch(tmp_path):
    import shutil
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "mir-prefer_amd", "csrc", "nats_kernels.hip"), "-o", str(tmp_path / "nats_kernels.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    report, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    for kernel, copies in (("nt_keys_kernel", 1), ("nt_head_kernel", 1), ("nt_start_kernel", 1), ("nt_join_kernel", 2), ("nt_cand_kernel", 1), ("nt_scan_kernel", 5),
                           ("nt_trace_kernel", 1)):
        mine = [v for k, v in report.items() if kernel in k]
        assert len(mine) == copies and all(v["ScratchSize"] == 0 for v in mine), (kernel, mine)
