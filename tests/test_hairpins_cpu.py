"""Host tests of the known-hairpin comparison (mir_prefer_amd.hairpins): the tests' restatement of the whole definition, which the
GPU tests (test_hairpins_gpu.py) import: the recurrences cell by cell in plain Python (fill_plain), the same matrices row by row in numpy (fill:
E as a prefix maximum along the row), a numpy scorer of one query against many known sequences (score_many: one Python step per query row, a
matrix over known sequences x columns), the traceback in plain Python, and both file writers.  The restatement is pinned to an enumeration of all
local alignments, to its own re-scored cigars, to the best ungapped segment as a lower bound, to hand-made values and to the tie rules.

The enumeration walks every alignment (every start cell, every string of = X I D).  It covers more than 1,000 random pairs of 1..9 nt: of
1,300 seeded pairs those whose lengths multiply to at most 49 (up to 7 x 7 and 9 x 5), and six more of 8 x 8, 8 x 9, 9 x 8 and 9 x 9, which take
seconds each.  Every pair is also checked against a memoised recursion over (row, column, last op), as a second, cheaper witness."""
import functools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_annotate_cpu import family as annotate_family
from tests.test_targets_cpu import ROOT

NEG = -10 ** 6
DEFAULT = (2, 3, 5, 2)          # match, mismatch, gap_open, gap_extend
HEADER = "query\tknown\tfamily\tscore\tidentity\tq_start\tq_end\tq_len\tk_start\tk_end\tk_len\tmatches\tmismatches\tgap_opens\tgap_bases\tcigar\n"
_CODE = np.full((2, 256), 255, dtype=np.uint8)
for _ch, _v in zip(b"AaCcGgUuTt", (0, 0, 1, 1, 2, 2, 3, 3, 3, 3)):
    _CODE[:, _ch] = _v
_CODE[0][_CODE[0] == 255] = 4          # an unknown letter of a query
_CODE[1][_CODE[1] == 255] = 5          # an unknown letter of a known sequence: equal to nothing, another unknown letter included


def as_bytes(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def codes(seq, known):
    return _CODE[1 if known else 0][np.frombuffer(as_bytes(seq), dtype=np.uint8)]


# ---------------------------------------------------------------------------------------------------- the recurrences
def fill_plain(q, k, par):
    """H, E, F as lists of rows, (len q + 1) x (len k + 1), by the recurrences of §25, cell by cell."""
    a, b, o, e = par
    cq, ck = codes(q, False).tolist(), codes(k, True).tolist()
    n, m = len(cq), len(ck)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(H[i][j - 1] - o - e, E[i][j - 1] - e)
            F[i][j] = max(H[i - 1][j] - o - e, F[i - 1][j] - e)
            s = a if cq[i - 1] == ck[j - 1] else -b
            H[i][j] = max(0, H[i - 1][j - 1] + s, E[i][j], F[i][j])
    return H, E, F


def fill(q, k, par):
    """The same three matrices as int32 arrays, one numpy step per row: F and the diagonal need the row above only, and E(i, j) = max over j' < j
    of max(0, diagonal, F)(i, j') - o - (j - j') e, a running maximum along the row.  Column 0 of E and row 0 of F hold NEG as in fill_plain; a
    gap that starts at the border is the term j' = 0, with H(i, 0) = 0."""
    a, b, o, e = par
    cq, ck = codes(q, False), codes(k, True)
    n, m = len(cq), len(ck)
    H = np.zeros((n + 1, m + 1), dtype=np.int32)
    E = np.full((n + 1, m + 1), NEG, dtype=np.int32)
    F = np.full((n + 1, m + 1), NEG, dtype=np.int32)
    je = np.arange(m + 1, dtype=np.int32) * e
    for i in range(1, n + 1):
        s = np.where(ck == cq[i - 1], a, -b)
        D = H[i - 1, :-1] + s
        F[i, 1:] = np.maximum(H[i - 1, 1:] - o - e, F[i - 1, 1:] - e)
        Ht = np.maximum(np.maximum(D, F[i, 1:]), 0)
        P = np.maximum.accumulate(np.concatenate(([0], Ht + je[1:])))
        E[i, 1:] = P[:-1] - o - je[1:]
        H[i, 1:] = np.maximum(Ht, E[i, 1:])
    return H, E, F


def end_cell(H):
    """(score, i, j): the maximal cell with the smallest i, then the smallest j"""
    H = np.asarray(H)
    at = int(np.argmax(H))          # the first maximum in row-major order
    i, j = divmod(at, H.shape[1])
    return int(H[i, j]), i, j


def traceback(q, k, H, E, F, par, i, j):
    """The ops from the end cell (i, j) back, in forward order, and the cell before the first op."""
    a, b, o, e = par
    cq, ck = codes(q, False), codes(k, True)
    ops, state = [], "H"
    while True:
        if state == "H":
            if H[i][j] == 0:
                break
            s = a if cq[i - 1] == ck[j - 1] else -b
            if H[i][j] == H[i - 1][j - 1] + s:
                ops.append("=" if s > 0 else "X")
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                state = "E"
            else:
                assert H[i][j] == F[i][j]
                state = "F"
        elif state == "E":
            ops.append("D")
            if E[i][j] == H[i][j - 1] - o - e:
                state = "H"
            j -= 1
        else:
            ops.append("I")
            if F[i][j] == H[i - 1][j] - o - e:
                state = "H"
            i -= 1
    return "".join(reversed(ops)), i, j


def rle(ops):
    return "".join("%d%s" % (len(m.group(0)), m.group(0)[0]) for m in re.finditer(r"=+|X+|I+|D+", ops))


def hit_of(ops, score, i0, j0, i1, j1):
    return dict(score=score, q_start=i0 + 1, q_end=i1, k_start=j0 + 1, k_end=j1, matches=ops.count("="), mismatches=ops.count("X"),
                gap_opens=len(re.findall(r"I+|D+", ops)), gap_bases=ops.count("I") + ops.count("D"), cigar=rle(ops), ops=ops)


def align_pair(q, k, par=DEFAULT, plain=False, end=None):
    """The hit record of the pair (a dict with the cigar and the ops), or None when the score is 0.  end: the (score, i, j) already known; then
    only q[1 .. i] x k[1 .. j] is filled, whose matrices are those of the whole pair up to there and whose end cell is the same."""
    q, k = as_bytes(q), as_bytes(k)
    if end is not None:
        q, k = q[:end[1]], k[:end[2]]
    H, E, F = (fill_plain if plain else fill)(q, k, par)
    score, i1, j1 = end_cell(H)
    assert end is None or (score, i1, j1) == tuple(end)
    if score == 0:
        return None
    ops, i0, j0 = traceback(q, k, H, E, F, par, i1, j1)
    return hit_of(ops, score, i0, j0, i1, j1)


def score_many(q, known, par):
    """(score, end i, end j) int arrays of the query against every known sequence: the known sequences in groups of similar length as one matrix,
    padded with a letter that equals nothing (a padded cell stays strictly below a real one, as every step into it costs at least 1).  One numpy
    step per query row as in fill; all rows of H are kept, and the end cell is the first maximum of each known sequence's matrix in row-major
    order.  16-bit integers where every intermediate value fits them."""
    a, b, o, e = par
    cq = codes(q, False)
    n, nk = len(cq), len(known)
    score, ei, ej = np.zeros(nk, dtype=np.int64), np.zeros(nk, dtype=np.int64), np.zeros(nk, dtype=np.int64)
    order = sorted(range(nk), key=lambda x: len(known[x]))
    for g0 in range(0, nk, 128):
        idx = order[g0:g0 + 128]
        m = max(len(known[x]) for x in idx)
        small = a * min(n, m) + e * (m + 1) + o + e + b < 30000
        dt, neg = (np.int16, -30000) if small else (np.int32, NEG)
        K = np.full((len(idx), m), 7, dtype=np.uint8)
        for r, x in enumerate(idx):
            K[r, :len(known[x])] = codes(known[x], True)
        S = [np.where(K == c, dt(a), dt(-b)) for c in range(5)]          # (an unknown letter of the query, 4, equals no known letter)
        H = np.zeros((len(idx), n + 1, m + 1), dtype=dt)
        F = np.full((len(idx), m), neg, dtype=dt)
        je = (np.arange(m + 1, dtype=dt) * dt(e))[None, :]
        oje = je[:, 1:] + dt(o)
        P = np.zeros((len(idx), m + 1), dtype=dt)
        for i in range(1, n + 1):
            Hp = H[:, i - 1, :]
            F -= dt(e)
            np.maximum(Hp[:, 1:] - dt(o + e), F, out=F)
            Ht = np.maximum(Hp[:, :-1] + S[cq[i - 1]], F)
            np.maximum(Ht, 0, out=Ht)
            np.add(Ht, je[:, 1:], out=P[:, 1:])
            acc = np.maximum.accumulate(P, axis=1)
            np.maximum(Ht, acc[:, :-1] - oje, out=H[:, i, 1:])
        at = np.argmax(H.reshape(len(idx), -1), axis=1)
        score[idx], ei[idx], ej[idx] = H.reshape(len(idx), -1)[np.arange(len(idx)), at], at // (m + 1), at % (m + 1)
    return score, ei, ej


# ---------------------------------------------------------------------------------------------------- the whole comparison and both files
def family(name):
    return annotate_family(as_bytes(name)).decode("latin-1")


def restate(queries, known, par=DEFAULT, min_score=60, max_lines=0):
    """-> (hit dicts in output order, each with query, known and the fields of hit_of; hits per query before the cut)"""
    hits, per_query = [], []
    for qi, q in enumerate(queries):
        if not known:
            per_query.append(0)
            continue
        score, ei, ej = score_many(q, known, par)
        found = sorted((-int(score[x]), x) for x in np.nonzero(score >= min_score)[0].tolist())
        per_query.append(len(found))
        for neg, x in found[:max_lines] if max_lines > 0 else found:
            h = align_pair(q, known[x], par, end=(-neg, int(ei[x]), int(ej[x])))
            h.update(query=qi, known=x)
            hits.append(h)
    return hits, per_query


def hits_text(q_names, queries, k_names, known, hits):
    lines = [HEADER]
    for h in hits:
        n_ops = h["matches"] + h["mismatches"] + h["gap_bases"]
        fields = [q_names[h["query"]], k_names[h["known"]], family(k_names[h["known"]]), "%d" % h["score"], "%.2f" % (100 * h["matches"] / n_ops),
                  "%d" % h["q_start"], "%d" % h["q_end"], "%d" % len(queries[h["query"]]), "%d" % h["k_start"], "%d" % h["k_end"],
                  "%d" % len(known[h["known"]]), "%d" % h["matches"], "%d" % h["mismatches"], "%d" % h["gap_opens"], "%d" % h["gap_bases"], h["cigar"]]
        lines.append("\t".join(fields) + "\n")
    return "".join(lines)


def summary_text(q_names, queries, k_names, known, hits, per_query):
    lines = []
    for qi, name in enumerate(q_names):
        mine = [h for h in hits if h["query"] == qi]
        if not mine:
            lines.append("%s\t%d\tnovel\t.\t.\t.\t.\t.\t.\t0\t.\n" % (name, len(queries[qi])))
            continue
        h = mine[0]
        lq, lk = len(queries[qi]), len(known[h["known"]])
        cls = "identical" if h["cigar"] == "%d=" % lq and lq == lk else "homolog"
        fams = []
        for x in mine:
            if family(k_names[x["known"]]) not in fams:
                fams.append(family(k_names[x["known"]]))
        n_ops = h["matches"] + h["mismatches"] + h["gap_bases"]
        lines.append("\t".join([name, "%d" % lq, cls, k_names[h["known"]], family(k_names[h["known"]]), "%d" % h["score"],
                                "%.2f" % (100 * h["matches"] / n_ops), "%.2f" % (100 * (h["q_end"] - h["q_start"] + 1) / lq),
                                "%.2f" % (100 * (h["k_end"] - h["k_start"] + 1) / lk), "%d" % per_query[qi], ",".join(fams)]) + "\n")
    return "".join(lines)


def as_records(hits):
    """The hit dicts as tuples in the order of capi.HAIRPIN_DTYPE's fields (reserved = 0) and their cigars."""
    return ([(h["query"], h["known"], h["score"], h["q_start"], h["q_end"], h["k_start"], h["k_end"], h["matches"], h["mismatches"], h["gap_opens"],
              h["gap_bases"], 0) for h in hits], [h["cigar"] for h in hits])


# ---------------------------------------------------------------------------------------------------- independent checks of the restatement
def enumerated(q, k, par):
    """The largest score of any local alignment, by walking all of them; 0 for the empty one."""
    a, b, o, e = par
    cq, ck = codes(q, False).tolist(), codes(k, True).tolist()
    n, m = len(cq), len(ck)
    best = 0

    def go(i, j, score, last):
        nonlocal best
        if score > best:
            best = score
        if i < n and j < m:
            go(i + 1, j + 1, score + (a if cq[i] == ck[j] else -b), 0)
        if i < n:
            go(i + 1, j, score - (e if last == 1 else o + e), 1)
        if j < m:
            go(i, j + 1, score - (e if last == 2 else o + e), 2)
    for i0 in range(n):
        for j0 in range(m):
            go(i0, j0, 0, 0)
    return best


def memoised(q, k, par):
    """The same maximum by recursion over (row, column, last op): the best continuation from a state does not depend on how it was reached."""
    a, b, o, e = par
    cq, ck = codes(q, False).tolist(), codes(k, True).tolist()
    n, m = len(cq), len(ck)

    @functools.lru_cache(maxsize=None)
    def rest(i, j, last):
        best = 0
        if i < n and j < m:
            best = max(best, (a if cq[i] == ck[j] else -b) + rest(i + 1, j + 1, 0))
        if i < n:
            best = max(best, rest(i + 1, j, 1) - (e if last == 1 else o + e))
        if j < m:
            best = max(best, rest(i, j + 1, 2) - (e if last == 2 else o + e))
        return best
    return max(rest(i, j, 0) for i in range(n) for j in range(m))


def rescore(q, k, h, par):
    """The score of the hit's ops laid on the two sequences from its start, and the cell they end in."""
    a, b, o, e = par
    cq, ck = codes(q, False).tolist(), codes(k, True).tolist()
    i, j, score, prev = h["q_start"] - 1, h["k_start"] - 1, 0, ""
    for op in h["ops"]:
        if op in "=X":
            assert (cq[i] == ck[j]) == (op == "=")
            score += a if op == "=" else -b
            i, j = i + 1, j + 1
        else:
            score -= e if op == prev else o + e
            i, j = (i + 1, j) if op == "I" else (i, j + 1)
        prev = op
    return score, i, j


def random_par(rng):
    return (rng.randint(1, 10), rng.randint(1, 10), rng.choice((0, 0, 1, 2, 5, 11, 20)), rng.randint(1, 10))


def random_seq(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def kadane(q, k, par):
    """The best ungapped segment over all diagonals: a lower bound of the score."""
    a, b, _, _ = par
    cq, ck = codes(q, False), codes(k, True)
    best = 0
    for d in range(-(len(cq) - 1), len(ck)):
        i0, j0 = max(0, -d), max(0, d)
        L = min(len(cq) - i0, len(ck) - j0)
        run = 0
        for s in np.where(cq[i0:i0 + L] == ck[j0:j0 + L], a, -b).tolist():
            run = max(0, run + s)
            best = max(best, run)
    return best


def pinned_to_the_walk(q, k, par, walk):
    """the checks of one short pair; -> whether all its alignments were walked"""
    H, E, F = fill_plain(q, k, par)
    score, i1, j1 = end_cell(H)
    if walk:
        assert score == enumerated(q, k, par), (q, k, par)
    assert score == memoised(q, k, par), (q, k, par)
    h = align_pair(q, k, par, plain=True)
    assert (h is None) == (score == 0)
    H2, E2, F2 = fill(q, k, par)
    assert H2.tolist() == H and F2.tolist() == F
    assert E2[1:, 1:].tolist() == [row[1:] for row in E[1:]]
    assert align_pair(q, k, par) == h
    s_many = score_many(q, [k, k + "A", "G" + k], par)
    assert (int(s_many[0][0]), int(s_many[1][0]), int(s_many[2][0])) == (score, i1 if score else 0, j1 if score else 0)
    if h:
        assert rescore(q, k, h, par) == (score, i1, j1) == (h["score"], h["q_end"], h["k_end"])
        assert h["ops"][0] == "=" and h["ops"][-1] == "="
    return walk


def test_enumeration_and_rescoring():
    rng = random.Random(25)
    walked = 0
    for t in range(1300):
        alphabet = "ACGUN" if t % 2 == 0 else "AC"
        q, k = random_seq(rng, rng.randint(1, 9), alphabet), random_seq(rng, rng.randint(1, 9), alphabet)
        walked += pinned_to_the_walk(q, k, random_par(rng), len(q) * len(k) <= 49)
    for t, (n, m) in enumerate(((8, 8), (8, 8), (8, 9), (9, 8), (9, 9), (9, 9))):          # the largest pairs: seconds each
        alphabet = "ACGUN" if t % 2 == 0 else "AC"
        par = random_par(rng) if t != 4 else (2, 3, 0, 1)
        walked += pinned_to_the_walk(random_seq(rng, n, alphabet), random_seq(rng, m, alphabet), par, True)
    assert walked >= 1000


def test_lower_bound_and_scorers_agree_at_realistic_lengths():
    rng = random.Random(7)
    for t in range(12):
        q, k = random_seq(rng, rng.randint(50, 300), "ACGUN" if t % 3 == 0 else "ACGU"), random_seq(rng, rng.randint(50, 300))
        if t % 2:
            k = k[:20] + q[10:60] + k[20:]          # a shared segment, so that gaps pay
        par = DEFAULT if t < 6 else random_par(rng)
        H, E, F = fill(q, k, par)
        score, i1, j1 = end_cell(H)
        assert score >= kadane(q, k, par) > 0
        if t < 3:
            assert H.tolist() == fill_plain(q, k, par)[0]
        s, ei, ej = score_many(q, [k, "ACGU", k[:40]], par)
        assert (int(s[0]), int(ei[0]), int(ej[0])) == (score, i1, j1)
        h = align_pair(q, k, par, end=(score, i1, j1))
        assert h == align_pair(q, k, par) and rescore(q, k, h, par) == (score, i1, j1)


def test_pins():
    h = align_pair("ACGUACGUACGU", "ACGU")
    assert (h["score"], h["q_start"], h["q_end"], h["k_start"], h["k_end"], h["cigar"]) == (8, 1, 4, 1, 4, "4=")
    h = align_pair("GGGAAACCC", "GGGCCC", (2, 3, 0, 1))
    assert (h["score"], h["cigar"], h["gap_opens"], h["gap_bases"], h["matches"]) == (9, "3=3I3=", 1, 3, 6)
    assert align_pair("acgt", "ACGU")["cigar"] == "4=" and align_pair("NNNN", "NNNN") is None and align_pair("ACNGU", "ACNGU")["cigar"] == "2=1X2="


def test_tie_rules():
    # the end cell: the smallest i, then the smallest j
    h = align_pair("ACGU", "ACGUACGUACGU")
    assert (h["q_end"], h["k_start"], h["k_end"]) == (4, 1, 4)
    h = align_pair("A" * 50, "A" * 20)
    assert (h["score"], h["q_start"], h["q_end"], h["k_end"], h["cigar"]) == (40, 1, 20, 20, "20=")
    h = align_pair("AC" * 30, "AC" * 10)
    assert (h["q_start"], h["q_end"], h["cigar"]) == (1, 20, "20=")
    # the diagonal before E before F: with a = b + ... chosen so that a mismatch column and a gap pair tie
    par = (4, 2, 0, 1)          # X costs 2; one I and one D cost 1 + 1 = 2
    h = align_pair("AAAACGGGG", "AAAAUGGGG", par)
    assert h["cigar"] == "4=1X4=" and h["score"] == 30
    # E before F: the same score through a deletion first or an insertion first
    H, E, F = fill_plain("AAAACGGGG", "AAAAUGGGG", (4, 5, 0, 1))
    h = align_pair("AAAACGGGG", "AAAAUGGGG", (4, 5, 0, 1), plain=True)
    assert h["score"] == 30 and h["cigar"] == "4=1I1D4=" and h["gap_opens"] == 2     # walking back, D is met first: it stands last
    # opening before extending: GGG AAA CCC against GGG CCC with o = 0 may open anywhere in the run; the walk takes the opening at once
    h = align_pair("GGGAAACCC", "GGGCCC", (2, 3, 0, 1))
    assert h["cigar"] == "3=3I3="
    h = align_pair("GGGCCC", "GGGAAACCC", (2, 3, 0, 1))
    assert h["cigar"] == "3=3D3=" and (h["k_start"], h["k_end"]) == (1, 9)


def test_family_rule_is_annotates():
    from mir_prefer_amd import hairpins
    ids = ["ath-MIR166a", "osa-miR166b-5p", "cel-let-7", "cel-lin-4", "hsa-mir-21", "MIR12", "mir-1", "let7", "lin-14x", "xyz", "ath-miRf10", "a-b-mir-3",
           "ath-MIR", "bna-MiR-0042c", "x1-LET-7a", "-mir-5", "ath-mirx-5", ""]
    for w in ids:
        assert hairpins.family(w) == annotate_family(w.encode()).decode(), w
    assert hairpins.family("ath-MIR166a") == "miR166" and hairpins.family("cel-let-7") == "let-7" and hairpins.family("xyz") == "xyz"


def test_names_and_option_errors_exit_2_before_the_binding(tmp_path, capsys):
    from mir_prefer_amd import hairpins
    assert hairpins.output_name("x.fa") == "x.fa.hairpins.tsv"
    assert hairpins.summary_name("x.fa.hairpins.tsv") == "x.fa.hairpins.summary.tsv" and hairpins.summary_name("out") == "out.summary.tsv"
    fa = tmp_path / "p.fa"
    fa.write_bytes(b">p\nGGGAAACCC\n")
    f = str(fa)
    got = hairpins.parse_args(["-o", "t/x.tsv", f, f, f])
    assert got[1:3] == (f, [f, f]) and got[4:] == ("t/x.tsv", "t/x.summary.tsv")
    o = hairpins.parse_args([f, f])[0]
    assert (o.match, o.mismatch, o.gap_open, o.gap_extend, o.min_score, o.max_hits) == (2, 3, 5, 2, 60, 0)
    assert hairpins.parse_args(["--gap-open", "0", "--species", "ath,osa", f, f])[3] == ["ath", "osa"]
    bad = [[], [f], ["--match", "0", f, f], ["--match", "11", f, f], ["--mismatch", "0", f, f], ["--mismatch", "11", f, f], ["--gap-open", "-1", f, f],
           ["--gap-open", "21", f, f], ["--gap-extend", "0", f, f], ["--gap-extend", "11", f, f], ["-s", "0", f, f], ["-k", "-1", f, f], ["--species", "", f, f],
           ["--species", "ath,,osa", f, f], ["--device", "-1", f, f], ["-o", "", f, f], ["-x", f, f], ["--match", "x", f, f]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            hairpins.parse_args(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    probe = "import sys\nfrom mir_prefer_amd import hairpins\ntry:\n    hairpins.main(['-s', '0', %r, %r])\nfinally:\n    print('capi' in ' '.join(sys.modules))\n" % (f, f)
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and b"Error: " not in r.stderr and r.stdout.strip() == b"False", (r.stdout, r.stderr)
    assert not list(tmp_path.glob("*.tsv"))


def test_readers_skip_filter_and_refuse():
    from mir_prefer_amd import hairpins
    assert hairpins.read_queries(b"junk\n>a some text\nACGU\nac\n>b\nGG\n") == [(b"a", b"ACGUac"), (b"b", b"GG")]
    for data, record in ((b">a\nACGU\n>b\n\n", 2), (b">a\n" + b"A" * 3001 + b"\n", 1), (b">a\nACGU\n>b\nAC\xe9U\n", 2), (b">a\nACGU\n>b caf\xe9\nACGU\n", 2),
                         (b">a\xff\nACGU\n", 1)):
        with pytest.raises(ValueError) as e:
            hairpins.read_queries(data)
        assert str(e.value).startswith("record %d: " % record), (data, str(e.value))
    assert hairpins.read_queries(b"caf\xe9\n>a\nACGU\n") == [(b"a", b"ACGU")]          # text before the first header is ignored
    known = b">ath-MIR1 x\nACGU\n>osa-MIR2\nGG\n>ath-MIR3 empty\n\n>ath-MIR4 long\n" + b"A" * 3001 + b"\n>athx-MIR5\nCC\n"
    assert hairpins.read_known([known, b">zma-MIR6\nUU\n"], []) == ([(b"ath-MIR1", b"ACGU"), (b"osa-MIR2", b"GG"), (b"athx-MIR5", b"CC"), (b"zma-MIR6", b"UU")], 2)
    assert hairpins.read_known([known, b">zma-MIR6\nUU\n"], ["ath", "zma"]) == ([(b"ath-MIR1", b"ACGU"), (b"zma-MIR6", b"UU")], 2)
    # a byte >= 0x80 is refused wherever it stands in a record: in a record that --species would drop, in one that the length would skip, in the
    # rest of a header line
    for data in (b">ath-MIR1\nACGU\n>osa-MIR2\nG\x80G\n", b">ath-MIR1\nACGU\n>ath-MIR3 \xb5\n\n", b">ath-MIR1\nACGU\n>ath-MIR7 caf\xe9\nACGU\n"):
        with pytest.raises(ValueError) as e:
            hairpins.read_known([b">ath-MIR0\nAC\n", data], ["ath"])
        assert e.value.args == (1, "record 2: a byte >= 0x80")


def test_writers():
    from mir_prefer_amd import capi, hairpins
    queries = ["GGGAAACCC", "ACGUACGU", "UUUU"]
    known = ["GGGCCC", "GGGAAACCC", "ACGUACGU"]
    q_names, k_names = ["pre1", "pre2", "pre3"], ["ath-MIR166a", "osa-MIR166b", "cel-let-7"]
    hits, per_query = restate(queries, known, (2, 3, 0, 1), min_score=9)
    assert [(h["query"], h["known"], h["score"], h["cigar"]) for h in hits] == [(0, 1, 18, "9="), (0, 0, 9, "3=3I3="), (1, 2, 16, "8=")] and per_query == [2, 1, 0]
    text = hits_text(q_names, queries, k_names, known, hits)
    assert text == (HEADER + "pre1\tosa-MIR166b\tmiR166\t18\t100.00\t1\t9\t9\t1\t9\t9\t9\t0\t0\t0\t9=\n"
                    "pre1\tath-MIR166a\tmiR166\t9\t66.67\t1\t9\t9\t1\t6\t6\t6\t0\t1\t3\t3=3I3=\n"
                    "pre2\tcel-let-7\tlet-7\t16\t100.00\t1\t8\t8\t1\t8\t8\t8\t0\t0\t0\t8=\n")
    summ = summary_text(q_names, queries, k_names, known, hits, per_query)
    assert summ == ("pre1\t9\tidentical\tosa-MIR166b\tmiR166\t18\t100.00\t100.00\t100.00\t2\tmiR166\n"
                    "pre2\t8\tidentical\tcel-let-7\tlet-7\t16\t100.00\t100.00\t100.00\t1\tlet-7\n"
                    "pre3\t4\tnovel\t.\t.\t.\t.\t.\t.\t0\t.\n")
    # the product's writers on the same records
    recs, cigars = as_records(hits)
    arr = np.array(recs, dtype=capi.HAIRPIN_DTYPE)
    lens = [len(s) for s in queries], [len(s) for s in known]
    assert hairpins.HEADER == HEADER and hairpins.hits_table(q_names, lens[0], k_names, lens[1], arr, cigars) == text
    got, classes = hairpins.summary_table(q_names, lens[0], k_names, lens[1], arr, per_query)
    assert got == summ and classes == {"identical": 2, "homolog": 0, "novel": 1}
    # -k 1: the families are those of the written lines, the hit count is the one before the cut; a homolog
    hits1, per1 = restate(queries[:1], known[:1] + ["CCCC"] + known[1:], (2, 3, 0, 1), min_score=9, max_lines=1)
    assert [h["known"] for h in hits1] == [2] and per1 == [2]
    hits2, per2 = restate(queries[:1], known[:1], (2, 3, 0, 1), min_score=9)
    assert summary_text(q_names[:1], queries[:1], k_names[:1], known[:1], hits2, per2) == "pre1\t9\thomolog\tath-MIR166a\tmiR166\t9\t66.67\t100.00\t100.00\t1\tmiR166\n"
    assert capi.cigar_of(b"===III===") == "3=3I3=" and capi.cigar_of(b"=") == "1=" and capi.cigar_of(b"") == ""


def capi_abi():
    from mir_prefer_amd import capi
    return capi.ABI_VERSION


def test_abi_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_hairpin_align(", "mirp_set_hairpin_capacity(", "mirp_hairpin_last_stats(", "MirpHairpinOpts", "MirpHairpinHit", "MIRP_HAIRPIN_STRIP"):
        assert name in header
    assert capi_abi() == 17
    from mir_prefer_amd import capi
    m = re.search(r"typedef struct \{([^}]*)\} MirpHairpinHit;", header)
    fields = [f.strip() for f in m.group(1).replace("int32_t", "").replace(";", "").split(",")]
    assert fields == list(capi.HAIRPIN_DTYPE.names) and capi.HAIRPIN_DTYPE.itemsize == 4 * len(fields) == 48
    assert int(re.search(r"#define MIRP_HAIRPIN_STRIP\s+(\d+)", header).group(1)) == capi.HAIRPIN_STRIP


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_kernels_use_no_scratch(tmp_path):
    import shutil
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "mir-prefer_amd", "csrc", "hairpin_kernels.hip"), "-o", str(tmp_path / "hairpin_kernels.o")]
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
    for kernel in ("hp_score_kernel", "hp_filter_kernel", "hp_cut_kernel", "hp_hit_kernel", "hp_trace_kernel"):
        mine = [v for k, v in report.items() if kernel in k]
        assert len(mine) == 1 and mine[0]["ScratchSize"] == 0, (kernel, mine)
