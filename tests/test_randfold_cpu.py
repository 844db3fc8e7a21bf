"""Host tests of the shuffle test of precursor MFEs (mir_prefer_amd.randfold): the tests' pure-Python restatement of the whole
definition -- the stateless random numbers, the mononucleotide and the dinucleotide (Altschul-Erikson, tree by cycle popping) shuffle, the integer
record of a sequence with MFEs from the CPU oracle, and the table -- pinned to the values DESIGN.md §20 states; the properties of the shuffles
(composition, dinucleotide counts and ends kept; uniform over the sequences that keep them); the table's formats; the command line's option
errors, FASTA rules, exit statuses and output removal, checked with the binding replaced by a stand-in; and the new kernels' resource report (no
scratch).  The GPU tests (test_randfold_gpu.py) compare the device output with this restatement."""
import collections
import itertools
import math
import os
import random
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mir-prefer_amd", "csrc")
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
HEADER = "name\tlength\tgc\tmfe\tamfe\tmfei\tshuffles\tle\tp\tmean\tsd\tz\n"
PIN_SEQ = "UGACAGAAGAGAGUGAGCACACAAAGGCAAUUUGCAUAUCAUUGCACUUGCUUCUCUUGCGUGCUCACUGCUCUUUCUGUCAGA"
LONG_WALK = "A" * 100 + "C" + "A" * 100 + "G"          # 400 draws under di at (seed 0, q 0, k 0)


# ---------------------------------------------------------------------------------------------------- restatement: random numbers and shuffles
def mix64(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


class Draws:
    """the draws of one (seed, q, k), consumed in order"""
    def __init__(self, seed, q, k):
        self.x0 = mix64((mix64(seed ^ (G * (q + 1) & M64)) + k) & M64)
        self.t = 0

    def below(self, m):
        self.t += 1
        return ((mix64((self.x0 + self.t * G) & M64) >> 32) * m) >> 32


def codes(seq):
    """A C G U in either case and T -> 0..3, every other letter 4"""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    return [{65: 0, 67: 1, 71: 2, 85: 3, 84: 3}.get(ch & 0xDF if 97 <= ch <= 122 else ch, 4) for ch in seq]


def letters(x):
    return bytes(b"ACGUN"[c] for c in x)


def fy(lst, d):
    for i in range(len(lst) - 1, 0, -1):
        j = d.below(i + 1)
        lst[i], lst[j] = lst[j], lst[i]


def mono(x, d):
    y = list(x)
    fy(y, d)
    return y


def di(x, d):
    n = len(x)
    if n < 3:
        return list(x)
    E = [[] for _ in range(5)]
    for i in range(n - 1):
        E[x[i]].append(x[i + 1])
    f = x[n - 1]
    intree = [a == f for a in range(5)]
    last = [None] * 5
    for a in range(5):
        if a == f or not E[a]:
            continue
        u = a
        while not intree[u]:
            last[u] = d.below(len(E[u]))
            u = E[u][last[u]]
        u = a
        while not intree[u]:
            intree[u] = True
            u = E[u][last[u]]
    for a in range(5):
        if not E[a]:
            continue
        if a != f:
            kept = E[a].pop(last[a])
            fy(E[a], d)
            E[a].append(kept)
        else:
            fy(E[a], d)
    y, used = [x[0]], [0] * 5
    for _ in range(1, n):
        a = y[-1]
        y.append(E[a][used[a]])
        used[a] += 1
    return y


def shuffled(seq, dinucleotide, seed, q, k, count_draws=False):
    """shuffle k of sequence q of a call as ACGUN bytes"""
    d = Draws(seed, q, k)
    y = letters((di if dinucleotide else mono)(codes(seq), d))
    return (y, d.t) if count_draws else y


# ---------------------------------------------------------------------------------------------------- restatement: records and table
def oracle_mfe(job):
    """(sequence bytes, model) -> the global MFE in 0.01 kcal/mol; a module-level function so that worker processes can run it"""
    from tests import oracle_binding
    s, model = job
    return oracle_binding.load().lfold(s, max(300, len(s)), model=model)["mfe"]


def restate_records(seqs, n, dinucleotide, seed, model="vienna-2.1.2", fold_many=None):
    """-> one dict per sequence with the fields of MirpRandfoldRec.  fold_many: maps a list of (bytes, model) jobs to MFEs (a worker pool's map)."""
    fold_many = fold_many or (lambda jobs: [oracle_mfe(j) for j in jobs])
    jobs = []
    for q, s in enumerate(seqs):
        jobs.append((letters(codes(s)), model))
        jobs.extend((shuffled(s, dinucleotide, seed, q, k), model) for k in range(n))
    mfes = fold_many(jobs)
    out = []
    for q, s in enumerate(seqs):
        native, sh = mfes[q * (n + 1)], mfes[q * (n + 1) + 1:(q + 1) * (n + 1)]
        c = codes(s)
        out.append({"len": len(c), "gc": sum(v in (1, 2) for v in c), "mfe": native, "le": sum(m <= native for m in sh), "min_mfe": min(sh),
                    "sum": sum(sh), "sum_sq": sum(m * m for m in sh)})
    return out


def restate_line(name, r, n):
    L, gc, mfe, le, S, Q = r["len"], r["gc"], r["mfe"], r["le"], r["sum"], r["sum_sq"]
    var = n * Q - S * S                                   # exact
    f = [name, str(L), "%.2f" % (100 * gc / L), "%.2f" % (mfe / 100), "%.2f" % ((0 - mfe) / L)]
    f.append("NA" if gc == 0 else "%.4f" % ((0 - mfe) / (100 * gc)))
    f += [str(n), str(le), "%.6f" % ((le + 1) / (n + 1)), "%.2f" % (S / n / 100)]
    if n == 1:
        f += ["NA", "NA"]
    else:
        sd = math.sqrt(var / (n * (n - 1)))
        f += ["%.2f" % (sd / 100), "NA" if var == 0 else "%.3f" % ((mfe - S / n) / sd)]
    return "\t".join(f) + "\n"


def restate_table(names, recs, n):
    return HEADER + "".join(restate_line(nm, r, n) for nm, r in zip(names, recs))


def records_as_dicts(arr):
    return [{k: int(r[k]) for k in ("len", "gc", "mfe", "le", "min_mfe", "sum", "sum_sq")} for r in arr]


# ---------------------------------------------------------------------------------------------------- seeded inputs
def random_seq(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGU", "UGCA"))


def planted_hairpin(rng):
    """stem 24..34 with three substituted bases on the 3' arm, loop 5..12, flanks 3..10"""
    stem = random_seq(rng, rng.randint(24, 34))
    arm = list(revcomp(stem))
    for p in rng.sample(range(len(arm)), 3):
        arm[p] = rng.choice([c for c in "ACGU" if c != arm[p]])
    return random_seq(rng, rng.randint(3, 10)) + stem + random_seq(rng, rng.randint(5, 12)) + "".join(arm) + random_seq(rng, rng.randint(3, 10))


# ---------------------------------------------------------------------------------------------------- the pins of §20
def test_random_number_pins():
    d = Draws(0, 0, 0)
    assert d.x0 == 0x48218226ff3cd4bf and [d.below(10) for _ in range(8)] == [3, 2, 2, 4, 5, 4, 0, 2]
    d = Draws(1, 2, 3)
    assert d.x0 == 0x843766e8929f9d9c and [d.below(1000) for _ in range(4)] == [72, 26, 979, 578]


def test_shuffle_pins():
    table = [(0, 0, 0, 0, "CAUCUUCUUACACAGCUGAAGCGGGAUAUUUUCCUCUUGUUGUUUGGGACCCAAGAAUUCUCCGACGAAGUCCGAGAACUUGAA", 83),
             (0, 12345, 7, 998, "CUAUCUCAGUACUCAGGCCAAGUGUUGUAUAGUAUGGGCAUAUUAUUCCCGACUGGCAUACGACUUCGCUCCAAUUUACAAGGG", 83),
             (1, 0, 0, 0, "UGAUGCACUGGAGCGAAGCUGCACUCUCAUUCACAUAUCAACAAGAGAGUUUGCAGCACUUUGCUUGAGCUUCUCUGUUGUCAA", 79),
             (1, 0, 0, 1, "UUGUCACAGGCAAAUUGCUUUUCUCAGCAAUCUGCUUGAUAAGAUUUGAGCUGCGCUCUCACACUCUGAGUGCAGUGACACAGA", 79),
             (1, M64, (1 << 24) - 1, 99999, "UGGCAGCACUGUUUUGACAAUUGCAGAUUGCUUGCGACAGAGAGUGAGCUCACUCUGUCUCAGCUGCACAUUCUCUUAAUCAAA", 83)]
    for method, seed, q, k, want, draws in table:
        assert shuffled(PIN_SEQ, method, seed, q, k, count_draws=True) == (want.encode(), draws), (method, seed, q, k)
    assert shuffled(LONG_WALK, 1, 0, 0, 0, count_draws=True)[1] == 400


# ---------------------------------------------------------------------------------------------------- properties of the shuffles
def _dicounts(x):
    return collections.Counter(zip(x, x[1:]))


def test_shuffles_keep_what_they_must():
    rng = random.Random(5)
    changed = 0
    for trial in range(400):
        n = rng.randint(1, 60)
        s = random_seq(rng, n, rng.choice(["ACGU", "AC", "ACGUN", "A", "AAAAAAAC"]))
        x = codes(s)
        y = di(x, Draws(3, trial, 0))
        assert len(y) == n and _dicounts(y) == _dicounts(x) and y[0] == x[0] and y[-1] == x[-1], s
        z = mono(x, Draws(3, trial, 0))
        assert sorted(z) == sorted(x), s
        changed += (y != x) + (z != x)
        if n < 3:
            assert y == x
    assert changed > 400


def test_dinucleotide_shuffle_is_uniform():
    """All 60 sequences with the dinucleotide counts and the ends of ACGAUCAGGACU, 12,000 shuffles of (seed 9, q 0, k = 0 .. 11999): every one is
    seen, none outside, and chi-square against the uniform distribution stays below 98.3, the 0.999 quantile at 59 degrees of freedom (the
    seed is fixed, so the value is: 63.19)."""
    x = codes("ACGAUCAGGACU")
    want = _dicounts(x)
    every = {(x[0],) + p + (x[-1],) for p in set(itertools.permutations(x[1:-1])) if _dicounts((x[0],) + p + (x[-1],)) == want}
    assert len(every) == 60
    seen = collections.Counter(tuple(di(x, Draws(9, 0, k))) for k in range(200 * len(every)))
    assert set(seen) == every
    expected = 200.0
    chi2 = sum((seen[p] - expected) ** 2 / expected for p in every)
    print("chi-square %.2f on 59 degrees of freedom" % chi2)
    assert abs(chi2 - 63.19) < 0.005 and chi2 < 98.3


def test_letters_case_t_and_others():
    assert codes("ACGUacgutTNnXKI-.*") == [0, 1, 2, 3, 0, 1, 2, 3, 3, 3] + [4] * 8
    assert letters(codes("acgtTuNxRY")) == b"ACGUUUNNNN"
    a = "UGACAGAAGAGAGUGAGCACXKI"
    b = "tgacagaagagagtgagcacnnn"
    for method in (0, 1):
        assert shuffled(a, method, 7, 3, 5) == shuffled(b, method, 7, 3, 5)
        assert set(shuffled(a, method, 7, 3, 5)) <= set(b"ACGUN") and shuffled(a, method, 7, 3, 5).count(b"N") == 3
    # the draws depend on the sequence's index and on the shuffle's, not on what else is in the call
    assert shuffled(a, 1, 7, 3, 5) != shuffled(a, 1, 7, 3, 6) and shuffled(a, 1, 7, 3, 5) != shuffled(a, 1, 7, 4, 5) != shuffled(a, 1, 8, 4, 5)


# ---------------------------------------------------------------------------------------------------- records with the CPU oracle
def test_records_with_oracle_folds(oracle):
    rng = random.Random(11)
    seqs = [planted_hairpin(rng), random_seq(rng, 40), "A" * 30, random_seq(rng, 25, "ACGUN")]
    for model in ("vienna-2.1.2", "vienna-1.8.5"):
        recs = restate_records(seqs, 12, 1, 4, model=model)
        assert [r["len"] for r in recs] == [len(s) for s in seqs] and recs[2]["gc"] == 0 and recs[2]["mfe"] == 0
        assert recs[0]["mfe"] < -1500 and recs[0]["le"] == 0 and recs[0]["min_mfe"] > recs[0]["mfe"]
        assert recs[2]["le"] == 12 and recs[2]["sum"] == 0 and recs[2]["sum_sq"] == 0 and recs[2]["min_mfe"] == 0
        for q, r in enumerate(recs):
            sh = [oracle.lfold(shuffled(seqs[q], 1, 4, q, k), 300, model=model)["mfe"] for k in range(12)]
            assert (r["sum"], r["sum_sq"], r["min_mfe"]) == (sum(sh), sum(m * m for m in sh), min(sh))
            # the global MFE does not depend on the span once the span covers the sequence
            assert oracle.lfold(seqs[q], len(seqs[q]), model=model)["mfe"] == r["mfe"] == oracle.lfold(seqs[q], 301, model=model)["mfe"]
    text = restate_table(["a", "b", "c", "d"], recs, 12)
    assert text.startswith(HEADER) and text.count("\n") == 5
    from mir_prefer_amd import randfold
    assert randfold.table(["a", "b", "c", "d"], recs, 12) == text


# ---------------------------------------------------------------------------------------------------- the table
def _rec(**kw):
    r = {"len": 80, "gc": 40, "mfe": -3050, "le": 0, "min_mfe": -2000, "sum": -999 * 1500, "sum_sq": 999 * 1500 * 1500 + 998 * 90000}
    r.update(kw)
    return r


def test_table_formats():
    from mir_prefer_amd import randfold
    assert randfold.HEADER == HEADER
    r = _rec()
    # mean -15.00; var = N Q - S^2 = N * 998 * 90000, sd = sqrt(90000) = 300 -> 3.00; z = (-3050 + 1500) / 300
    assert restate_line("pre1", r, 999) == "pre1\t80\t50.00\t-30.50\t38.12\t0.7625\t999\t0\t0.001000\t-15.00\t3.00\t-5.167\n"
    cases = [(r, 999), (_rec(mfe=0, le=999), 999), (_rec(gc=0), 999), (_rec(sum=-1500, sum_sq=1500 * 1500, le=1), 1),
             (_rec(sum=-999 * 1500, sum_sq=999 * 1500 * 1500), 999), (_rec(len=3000, gc=1, mfe=-123456, sum=-7, sum_sq=49), 2),
             (_rec(mfe=0, sum=0, sum_sq=0, le=5), 5), (_rec(len=1, gc=1, mfe=0, sum=0, sum_sq=0, le=100000), 100000)]
    for rec, n in cases:
        assert randfold.table_line("x", rec, n) == restate_line("x", rec, n), (rec, n)
    f = restate_line("x", _rec(mfe=0, le=999), 999).split("\t")
    assert f[3] == "0.00" and f[4] == "0.00" and f[5] == "0.0000" and f[8] == "1.000000"          # not -0.00
    assert restate_line("x", _rec(gc=0), 999).split("\t")[5] == "NA"
    one = restate_line("x", _rec(sum=-1500, sum_sq=1500 * 1500, le=1), 1).rstrip("\n").split("\t")
    assert one[6:] == ["1", "1", "1.000000", "-15.00", "NA", "NA"]
    flat = restate_line("x", _rec(sum=-999 * 1500, sum_sq=999 * 1500 * 1500), 999).rstrip("\n").split("\t")
    assert flat[9:] == ["-15.00", "0.00", "NA"]                                                    # no spread: no z
    # the variance is exact where a double would not be: S^2 and N Q beyond 2^53
    big = _rec(mfe=-150000, sum=-100000 * 140000, sum_sq=100000 * 140000 * 140000 + 99999 * 100)
    assert restate_line("x", big, 100000).rstrip("\n").split("\t")[10:] == ["0.10", "-1000.000"]
    assert randfold.table_line("x", big, 100000) == restate_line("x", big, 100000)
    assert randfold.table(["a", "b"], [r, _rec(gc=0)], 999) == restate_table(["a", "b"], [r, _rec(gc=0)], 999)
    assert randfold.table([], [], 999) == HEADER


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.randfold"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    fa = tmp_path / "p.fa"
    fa.write_bytes(b">p\n" + PIN_SEQ.encode() + b"\n")
    bad = [[], [str(fa), str(fa)], ["-n", "0", str(fa)], ["-n", "100001", str(fa)], ["-n", "x", str(fa)], ["-m", "tri", str(fa)], ["-m", "", str(fa)],
           ["--seed", "-1", str(fa)], ["--seed", str(1 << 64), str(fa)], ["--seed", "1.5", str(fa)], ["--seed", "", str(fa)],
           ["--fold-model", "vienna-3", str(fa)], ["--device", "-1", str(fa)], ["-o", "", str(fa)], ["-x", str(fa)]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_option_errors_do_not_import_the_binding():
    code = ("import sys\nfrom mir_prefer_amd import randfold\n"
            "for a in (['-n', '0', 'p'], ['-m', 'tri', 'p'], ['--seed', '-1', 'p'], ['--fold-model', 'x', 'p'], []):\n"
            "    try:\n        randfold.main(a)\n    except SystemExit as e:\n        assert e.code == 2, (a, e.code)\n    else:\n        raise AssertionError(a)\n"
            "assert 'mir_prefer_amd.capi' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr.decode()


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "nope.fa.randfold.tsv").write_bytes(b"stale\n")
    r = run_cli([str(tmp_path / "nope.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.fa" in r.stderr.decode()


def test_helpers_of_the_command_line(capsys):
    from mir_prefer_amd import randfold
    o, path, seed, out = randfold.parse_args(["p.fa"])
    assert (o.shuffles, o.method, seed, o.fold_model, o.device, path, out) == (999, "di", 0, "vienna-2.1.2", 0, "p.fa", "p.fa.randfold.tsv")
    o, path, seed, out = randfold.parse_args(["-n", "50", "-m", "mono", "--seed", str(M64), "--fold-model", "vienna-1.8.5", "-o", "x.tsv", "--device", "2", "d/p.fa"])
    assert (o.shuffles, o.method, seed, o.fold_model, o.device, path, out) == (50, "mono", M64, "vienna-1.8.5", 2, "d/p.fa", "x.tsv")
    assert randfold.parse_seed("0x10") == 16 and randfold.parse_seed("12 ") == 12 and randfold.parse_seed("x") is None and randfold.parse_seed(str(1 << 64)) is None
    assert randfold.output_name("out/prefix_miRNA.precursor.fa") == "out/prefix_miRNA.precursor.fa.randfold.tsv"
    with pytest.raises(SystemExit) as e:
        randfold.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--shuffles", "--method", "--seed", "--fold-model", "--output", "--device"):
        assert opt in text


def test_fasta_rules():
    from mir_prefer_amd import randfold
    data = (b"junk before\n>chr1:100-183 + miRNA-precursor_0  extra\tfields\nUGACAG\r\nAAGAGA\rgugagc ac\n\n>second\n>third x\nAC GU\t\nNNXX\n"
            b">p4|a=b\nacgt")
    assert randfold.parse_fasta(data) == [(b"chr1:100-183", b"UGACAGAAGAGAgugagcac"), (b"second", b""), (b"third", b"ACGUNNXX"), (b"p4|a=b", b"acgt")]
    assert randfold.parse_fasta(b"") == [] and randfold.parse_fasta(b"no header\nACGU\n") == []
    for bad in (b">a\nACGU\n>\nACGU\n", b">a\nACGU\n>  \t \nACGU\n"):
        with pytest.raises(ValueError) as e:
            randfold.parse_fasta(bad)
        assert "record 2: a header without a name" in str(e.value)


class _StandIn(types.ModuleType):
    """mir_prefer_amd.capi for the host logic: a context whose randfold answers from the restatement's integers, or refuses"""
    class MirpError(RuntimeError):
        pass

    def __init__(self, usable=True, refuse=None):
        super().__init__("mir_prefer_amd.capi")
        self.calls = []
        mod = self

        class Context:
            def __init__(self, device=0):
                if not usable:
                    raise mod.MirpError("mirp_create(device=%d) failed with code -3 (no usable GPU?)" % device)
                mod.calls.append(("create", device))

            def set_fold_model(self, model):
                mod.calls.append(("model", model))

            def randfold(self, seqs, n_shuffles=999, dinucleotide=True, seed=0, capacity=0):
                mod.calls.append(("randfold", list(seqs), n_shuffles, dinucleotide, seed))
                if refuse:
                    raise mod.MirpError(refuse)
                recs = [{"len": len(s), "gc": sum(v in (1, 2) for v in codes(s)), "mfe": -100 * q, "le": q, "min_mfe": -5, "sum": -3 * n_shuffles,
                         "sum_sq": 9 * n_shuffles + q, "reserved": 0} for q, s in enumerate(seqs)]
                return recs, {"sequences": len(seqs), "folds": len(seqs) * (n_shuffles + 1), "passes": 1, "fallbacks": 0, "seconds": [0.0] * 5}

            def close(self):
                mod.calls.append(("close",))
        self.Context = Context


def _main_with(monkeypatch, stand_in, argv):
    import mir_prefer_amd
    from mir_prefer_amd import randfold
    monkeypatch.setitem(sys.modules, "mir_prefer_amd.capi", stand_in)
    monkeypatch.setattr(mir_prefer_amd, "capi", stand_in, raising=False)
    return randfold.main(argv)


def test_main_writes_the_table_and_removes_it_on_refusal(tmp_path, monkeypatch, capsys):
    fa = tmp_path / "prefix_miRNA.precursor.fa"
    fa.write_bytes(b">chr1:5-88 + miRNA-precursor_0\n" + PIN_SEQ[:60].encode() + b"\n" + PIN_SEQ[60:].encode() + b"\n>p2 x\nacgtn\n")
    out = tmp_path / "prefix_miRNA.precursor.fa.randfold.tsv"
    ok = _StandIn()
    assert _main_with(monkeypatch, ok, ["-n", "7", "-m", "mono", "--seed", "0xff", "--fold-model", "vienna-1.8.5", "--device", "1", str(fa)]) == 0
    assert ok.calls == [("create", 1), ("model", "vienna-1.8.5"), ("randfold", [PIN_SEQ.encode(), b"acgtn"], 7, False, 255), ("close",)]
    recs = [{"len": 84, "gc": sum(v in (1, 2) for v in codes(PIN_SEQ)), "mfe": 0, "le": 0, "sum": -21, "sum_sq": 63},
            {"len": 5, "gc": 2, "mfe": -100, "le": 1, "sum": -21, "sum_sq": 64}]
    assert out.read_text() == restate_table(["chr1:5-88", "p2"], recs, 7)
    err = capsys.readouterr().err
    assert err.startswith("randfold: 2 precursors, 16 folds, 1 passes, ") and err.endswith("written to %s\n" % out)
    # -o, and an empty FASTA file is a table without lines
    (tmp_path / "empty.fa").write_bytes(b"")
    assert _main_with(monkeypatch, _StandIn(), ["-o", str(tmp_path / "e.tsv"), str(tmp_path / "empty.fa")]) == 0
    assert (tmp_path / "e.tsv").read_text() == HEADER
    capsys.readouterr()
    # a refused input, no device, a header without a name, an output that cannot be written: status 255, `Error: `, and no file, not even the old one
    for stand_in, data, msg in ((_StandIn(refuse="mirp_randfold failed (-10): mirp_randfold: record 2: an empty sequence"), None, "record 2: an empty sequence"),
                                (_StandIn(usable=False), None, "there is no CPU path"),
                                (_StandIn(), b">a\nACGU\n> \nACGU\n", "record 2: a header without a name")):
        assert out.exists() or out.write_text("stale\n")
        if data is not None:
            fa.write_bytes(data)
        assert _main_with(monkeypatch, stand_in, [str(fa)]) == 255
        err = capsys.readouterr().err
        assert err.startswith("Error: ") and msg in err, err
        assert not out.exists()
        if data is not None:
            assert stand_in.calls == []                  # refused before a device was opened
    fa.write_bytes(b">a\nACGU\n")
    assert _main_with(monkeypatch, _StandIn(), ["-o", str(tmp_path / "no" / "dir.tsv"), str(fa)]) == 255
    assert capsys.readouterr().err.startswith("Error: ") and not (tmp_path / "no").exists()


# ---------------------------------------------------------------------------------------------------- the new kernels' resources
def test_randfold_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "randfold_kernels.hip"), "-o", str(tmp_path / "randfold_kernels.o")]
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
    assert sum("rf_shuffle_kernel" in k for k in report) == 2 and sum("rf_stats_kernel" in k for k in report) == 1, sorted(report)
    for k, r in sorted(report.items()):
        print(k, "VGPRs", r["VGPRs"], "SGPRs", r.get("TotalSGPRs"), "occupancy", r["Occupancy"], "scratch", r["ScratchSize"], "LDS", r.get("LDS Size"))
        assert r["ScratchSize"] == 0 and r.get("LDS Size", 0) == 0, (k, r)
