"""Host tests of the recorded long-sequence reference of the partition function (tests/golden/ensemble_long.json.gz): six sequences of
700..1,400 nt restated once by tests/test_ensemble_cpu.py's inside / outside program in extended precision (tests/golden/tools/gen_ensemble_long.py;
minutes of Python, so not run inside a GPU test), which tests/test_ensemble_long_gpu.py compares the slab kernels with.  This module holds the
recipes' interpreter (the generator and the tests build the letters with it) and pins the file: the letters to the recipes, mfe to the CPU oracle,
the centroid to the stored pairs, the row sums to the identities, and ln Z of the 700-nt entry to a fresh run of inside()."""
import random

import numpy as np
import pytest

from tests.golden_util import load_json
from tests.test_ensemble_cpu import KT, SumProduct, inside, pair_table, planted_hairpin, random_seq, revcomp
from tests.test_randfold_cpu import oracle_mfe

FIXTURE = "ensemble_long.json.gz"
STORED_FROM = 5e-4          # every pair with a restated p of at least this is in the file
SLAB_THREADS = 1024         # the block size of en_*_kernel<false>: position i >= 1024 is a thread's second cell of a diagonal

# The recipes: parts are drawn in order from one random.Random(seed).
#   ["random", n]             n letters of ACGU
#   ["hairpin", n]            planted_hairpin(rng, n): a stem with three edits around a loop of 4..9, random flanks
#   ["gc_hairpin", arm, loop] a perfect G/C stem of `arm` pairs around `loop` (letters)
#   ["n_loop", arm, u]        a perfect G/C stem of `arm` pairs around u letters N: a hairpin loop of u unpaired bases
#   ["text", letters]
# and then the edits: "lower" / "t" = [from, to) ranges written in lower case / with T for U, "n" = positions overwritten with N.
RECIPES = [
    dict(seed=2331, parts=[["random", 120], ["hairpin", 110], ["random", 150], ["hairpin", 80], ["random", 140], ["hairpin", 100]]),
    dict(seed=2332, parts=[["random", 200], ["hairpin", 120], ["random", 300], ["hairpin", 90], ["random", 217], ["hairpin", 100]]),
    dict(seed=2333, parts=[["random", 310], ["hairpin", 140], ["random", 250], ["hairpin", 70], ["random", 178], ["hairpin", 80]]),
    dict(seed=2334, parts=[["random", 250], ["hairpin", 100], ["random", 330], ["hairpin", 120], ["random", 224], ["text", "GAAAC"]]),
    dict(seed=2335, parts=[["random", 280], ["hairpin", 130], ["random", 300], ["hairpin", 100], ["random", 214], ["random", 20],
                           ["gc_hairpin", 14, "GAAA"], ["random", 4], ["gc_hairpin", 8, "UUCG"]],
         lower=[[0, 60], [500, 620]], t=[[30, 90], [700, 1000]], n=[17, 333, 650, 871, 1010]),
    dict(seed=2336, parts=[["random", 400], ["hairpin", 150], ["random", 300], ["hairpin", 120], ["random", 60], ["n_loop", 14, 210], ["random", 40],
                           ["hairpin", 60], ["gc_hairpin", 14, "GCAA"]]),
]
LENGTHS = [700, 1027, 1028, 1029, 1100, 1400]


def build(recipe):
    """the letters of a recipe"""
    rng = random.Random(recipe["seed"])
    out = []
    for part in recipe["parts"]:
        kind = part[0]
        if kind == "random":
            out.append(random_seq(rng, part[1]))
        elif kind == "hairpin":
            out.append(planted_hairpin(rng, part[1]))
        elif kind == "gc_hairpin":
            arm = random_seq(rng, part[1], "GC")
            out.append(arm + part[2] + revcomp(arm))
        elif kind == "n_loop":
            arm = random_seq(rng, part[1], "GC")
            out.append(arm + "N" * part[2] + revcomp(arm))
        elif kind == "text":
            out.append(part[1])
        else:
            raise ValueError(kind)
    s = list("".join(out))
    for a, b in recipe.get("t", ()):
        s[a:b] = [{"U": "T"}.get(ch, ch) for ch in s[a:b]]
    for a, b in recipe.get("lower", ()):
        s[a:b] = [ch.lower() for ch in s[a:b]]
    for x in recipe.get("n", ()):
        s[x] = "N"
    return "".join(s)


def normalised(s):
    """upper case, U for T, N for anything else: the letters as §23 reads them"""
    return "".join(ch if ch in "ACGU" else "N" for ch in s.upper().replace("T", "U"))


def load():
    """the fixture with its pair lists as arrays: per entry i, j (1-based, int64) and p, ordered by (i, j), and row (n doubles)"""
    fx = load_json(FIXTURE)
    for e in fx["sequences"]:
        e["i"], e["j"] = np.array(e["pairs_i"], dtype=np.int64), np.array(e["pairs_j"], dtype=np.int64)
        e["p"], e["row"] = np.array(e["pairs_p"], dtype=np.float64), np.array(e["row"], dtype=np.float64)
    return fx


@pytest.fixture(scope="module")
def entries():
    return load()["sequences"]


def test_letters_regenerate_from_the_recipes(entries):
    assert [e["n"] for e in entries] == LENGTHS and [e["recipe"] for e in entries] == RECIPES
    for e in entries:
        assert build(e["recipe"]) == e["seq"] and len(e["seq"]) == e["n"] == e["record"]["len"]
        assert sum(normalised(e["seq"]).count(ch) for ch in "ACGU") >= e["n"] - 215
    # what the lengths and recipes are for
    e = entries[3]
    assert e["seq"][SLAB_THREADS:] == "GAAAC"
    k = np.nonzero((e["i"] == 1025) & (e["j"] == 1029))[0]
    assert e["p_spilled_cell"] >= 1e-6 and (len(k) == 0 or abs(e["p"][k[0]] - e["p_spilled_cell"]) <= 1e-13)
    for e in entries[4:]:
        assert ((e["p"] > 0.5) & (e["i"] > SLAB_THREADS)).any()
    s = entries[4]["seq"]
    assert any(ch.islower() for ch in s) and "T" in s and "t" in s and 3 <= s.count("N") <= 10
    assert "N" * 200 in entries[5]["seq"]
    u = entries[5]["seq"].index("N" * 200)
    loop = np.nonzero((entries[5]["i"] == u) & (entries[5]["j"] == u + 211))[0]          # the pair that closes the N run, 1-based
    assert len(loop) == 1 and entries[5]["p"][loop[0]] > 0.5 and u >= SLAB_THREADS


def test_records_and_identities(entries):
    for e in entries:
        rec, n = e["record"], e["n"]
        assert rec["mfe"] == oracle_mfe((normalised(e["seq"]).encode(), "vienna-2.1.2")), n
        assert rec["efe"] <= rec["mfe"] / 100 and 0 < rec["mfe_freq"] <= 1
        assert abs(rec["efe"] + KT * e["lnz"]) <= 1e-12 * abs(rec["efe"])
        assert e["min_gap"] >= 1e-6
        i, j, p, row = e["i"], e["j"], e["p"], e["row"]
        assert len(i) == len(j) == len(p) and len(row) == n
        assert p.min() >= STORED_FROM and p.max() <= 1 and (i >= 1).all() and (j - i >= 4).all() and (j <= n).all()
        assert (np.diff(i * 4096 + j) > 0).all(), "ordered by (i, j)"
        # the centroid: the stored pairs with p > 0.5, balanced
        text = ["."] * n
        for a, b in zip(i[p > 0.5], j[p > 0.5]):
            text[a - 1], text[b - 1] = "(", ")"
        assert "".join(text) == e["centroid"]
        assert sorted(pair_table(e["centroid"]).items()) == [(int(a) - 1, int(b) - 1) for a, b in zip(i[p > 0.5], j[p > 0.5])]
        assert rec["centroid_pairs"] == int((p > 0.5).sum()) > 20
        # the row sums of the whole matrix: at most 1, at least what the stored pairs hold
        stored = np.zeros(n + 1)
        np.add.at(stored, i, p)
        np.add.at(stored, j, p)
        assert row.max() <= 1 + 1e-12 and row.min() >= 0 and (row >= stored[1:] - 1e-12).all()
        # diversity and centroid_dist are bounded below by their stored terms and above by the rows
        assert rec["diversity"] >= 2 * float((p * (1 - p)).sum()) - 1e-9 and rec["diversity"] <= float(row.sum()) + 1e-9
        assert rec["centroid_dist"] >= float(np.where(p > 0.5, 1 - p, p).sum()) - 1e-9


def test_the_file_is_the_restatement_at_700_nt(entries):
    e = entries[0]
    I = inside(e["seq"], SumProduct)
    lnz = float(np.log(I["Q5"][I["n"]]))
    assert abs(lnz - e["lnz"]) <= 1e-12 * abs(e["lnz"]), (lnz, e["lnz"])
