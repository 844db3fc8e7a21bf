"""Host tests of the degradome (PARE) cleavage scan (mir_prefer_amd.degradome): the tests' two restatements of the whole definition,
both producing the TSV bytes -- a plain one (dicts; every miRNA scored at every unit with score_site, the site counts from a plain loop over every
offset) and a numpy one that goes the other way round (every site of every miRNA from sites_numpy, each looked up among the units) -- on top of
the helpers of tests/test_targets_cpu.py; hand-made cases for the categories, the offset identity and the edges; the p-value formula against exact
rational arithmetic; and the option errors of the command line, checked without opening a device.  The GPU tests (test_degradome_gpu.py) compare
the device output with these restatements."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd.synth import ALN_DTYPE
from tests.test_align_cpu import CODE
from tests.test_targets_cpu import ACGT, CLS, MIR, PAIR, RNA, ROOT, parse_mirnas, plant, random_mirnas, score_site, sites_numpy, target_of_mirna

HEADER = b"miRNA\ttarget\tcleavage\tstart\tend\tscore\tcategory\treads\ttranscript_max\tsites\tpvalue\tmismatches\tgu\tmirna_5to3\tpairs\ttarget_3to5\n"
STAT_KEYS = ("records", "sense", "minus", "units", "c0", "c1", "c2", "c3", "c4", "evaluations", "hits")


def pvalue(n, c, P):
    """§18: the chance that at least one of n sites falls on one of c positions out of P, in IEEE double."""
    return 1.0 if c >= P else -math.expm1(n * math.log1p(-(c / P)))


def hit_line(mname, tname, p, half, cat, a, amax, n, pv, mc, cls, ys):
    L = len(mc)
    o = p + 9 - L
    cls = np.asarray(cls)
    return b"%s\t%s\t%d\t%d\t%d\t%d.%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%s\t%s\t%s\n" % (
        mname, tname.encode(), p, o + 1, o + L, half // 2, 5 * (half & 1), cat, a, amax, n, b"%.3e" % pv, int((cls == 2).sum()), int((cls == 1).sum()),
        bytes(RNA[c] for c in mc), bytes(PAIR[c] for c in cls), bytes(RNA[y] for y in ys))


def _emit(hits):
    """hits: (m, category, half, transcript, p, line) -> the TSV bytes in §18's order"""
    hits.sort(key=lambda h: h[:5])
    return HEADER + b"".join(h[5] for h in hits)


def make_records(rows):
    """rows of (tid, pos, depth, len, strand[, sample]) -> ALN_DTYPE array sorted stably by (tid, pos)."""
    a = np.zeros(len(rows), ALN_DTYPE)
    if rows:
        r = np.array([tuple(x) + (0,) * (6 - len(x)) for x in rows], dtype=np.int64)
        a["tid"], a["pos"], a["depth"], a["len"], a["strand"], a["sample"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5]
    return a[np.lexsort((a["pos"], a["tid"]))]


class Case:
    """One input: mirnas [(name, codes)], the FASTA's names and code arrays, the @SQ names and lengths (any order, a subset of the FASTA) and the
    records (tid = @SQ index)."""

    def __init__(self, mirnas, fa_names, seqs, sq_names, sq_lens, recs):
        self.mirnas, self.fa_names, self.seqs, self.sq_names, self.sq_lens, self.recs = mirnas, fa_names, seqs, list(sq_names), list(sq_lens), recs
        index = {n: i for i, n in enumerate(fa_names)}
        self.fa_of_sq = [index[n] for n in sq_names]
        assert all(len(seqs[f]) == ln for f, ln in zip(self.fa_of_sq, sq_lens))
        self.P = sum(len(s) for s in seqs)


# ---------------------------------------------------------------------------------------------------- the plain restatement
def units_plain(case):
    """-> ({(FASTA index, p): abundance}, sense records, minus-strand records)"""
    units, sense, minus = {}, 0, 0
    for tid, pos, depth, _, strand, _ in case.recs.tolist():
        if strand:
            minus += 1
            continue
        if not (0 <= tid < len(case.sq_lens) and 1 <= pos <= case.sq_lens[tid]):
            continue
        sense += 1
        key = (case.fa_of_sq[tid], pos)
        units[key] = units.get(key, 0) + depth
    return units, sense, minus


def categories_plain(units):
    """-> ({unit: category}, {transcript: amax}, [C_0 .. C_4])"""
    by_t = {}
    for (t, p), a in units.items():
        by_t.setdefault(t, []).append(a)
    cat, amax, C = {}, {}, [0] * 5
    for (t, p), a in units.items():
        v = by_t[t]
        mx, tot, npos = max(v), sum(v), len(v)
        amax[t] = mx
        k = 4 if a == 1 else 0 if a == mx and v.count(mx) == 1 else 1 if a == mx else 2 if a * npos > tot else 3
        cat[t, p] = k
        C[k] += 1
    return cat, amax, C


_CLS = CLS.tolist()


def count_sites_plain(mc, t, cleavage, limit=16):
    """hist[h] = plus-strand sites of the miRNA on t with half-score h <= limit (a plain loop over every offset, leaving a site once it is over)"""
    mcl, tl, L = [int(x) for x in mc], t.tolist(), len(mc)
    w = [2 if 2 <= i <= 13 else 1 for i in range(1, L + 1)]
    hist = [0] * (limit + 1)
    for o in range(len(tl) - L + 1):
        half = 0
        for i in range(L):
            x = tl[o + L - 1 - i]
            if x > 3:
                half = limit + 1
                break
            k = _CLS[mcl[i]][x]
            if k:
                if cleavage and k == 2 and (i == 9 or i == 10):
                    half = limit + 1
                    break
                half += w[i] * k
                if half > limit:
                    break
        if half <= limit:
            hist[half] += 1
    return hist


def prepare_plain(case, cleavage):
    """hist[m][h] over all transcripts (the costly part; reused over -s, --max-category and -p)"""
    out = []
    for _, mc in case.mirnas:
        tot = [0] * 17
        for t in case.seqs:
            tot = [x + y for x, y in zip(tot, count_sites_plain(mc, t, cleavage))]
        out.append(tot)
    return out


def restate_plain(case, max_half=8, cleavage=False, max_category=4, alpha=1.0, prep=None):
    hist = prep if prep is not None else prepare_plain(case, cleavage)
    units, sense, minus = units_plain(case)
    cat, amax, C = categories_plain(units)
    hits, kept = [], 0
    for (t, p), a in units.items():
        k = cat[t, p]
        if k > max_category:
            continue
        kept += 1
        for m, (mname, mc) in enumerate(case.mirnas):
            r = score_site(mc, case.seqs[t], p + 9 - len(mc), 0, cleavage)
            if r is None or r[0] > max_half:
                continue
            n = sum(hist[m][:r[0] + 1])
            pv = pvalue(n, sum(C[:k + 1]), case.P)
            if pv <= alpha:
                hits.append((m, k, r[0], t, p, hit_line(mname, case.fa_names[t], p, r[0], k, a, amax[t], n, pv, mc, r[1], r[2])))
    stats = dict(zip(STAT_KEYS, [len(case.recs), sense, minus, len(units)] + C + [kept * len(case.mirnas), len(hits)]))
    return _emit(hits), stats


# ---------------------------------------------------------------------------------------------------- the numpy restatement
def units_numpy(case):
    """-> (FASTA index, p, abundance) arrays of the units in (tid, p) order, sense records, minus-strand records"""
    r = case.recs
    lens = np.asarray(case.sq_lens, dtype=np.int64)
    tid, pos = r["tid"].astype(np.int64), r["pos"].astype(np.int64)
    inside = (tid >= 0) & (tid < len(lens))
    ok = (r["strand"] == 0) & inside
    ok[ok] &= (pos[ok] >= 1) & (pos[ok] <= lens[tid[ok]])
    key = (tid[ok] << 32) | pos[ok]
    order = np.argsort(key, kind="stable")
    key, dep = key[order], r["depth"][ok][order].astype(np.int64)
    if len(key) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, 0, int((r["strand"] != 0).sum())
    first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    a = np.add.reduceat(dep, first)
    uk = key[first]
    return np.asarray(case.fa_of_sq, dtype=np.int64)[uk >> 32], uk & 0xffffffff, a, int(ok.sum()), int((r["strand"] != 0).sum())


def categories_numpy(t, a):
    """units in transcript-contiguous order -> (category per unit, amax per unit, [C_0 .. C_4])"""
    if len(t) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), [0] * 5
    first = np.flatnonzero(np.concatenate(([True], t[1:] != t[:-1])))
    seg = np.repeat(np.arange(len(first)), np.diff(np.concatenate((first, [len(t)]))))
    mx = np.maximum.reduceat(a, first)[seg]
    npos = np.diff(np.concatenate((first, [len(t)])))[seg]
    tot = np.add.reduceat(a, first)[seg]
    nmax = np.add.reduceat((a == mx).astype(np.int64), first)[seg]
    above = a.astype(object) * npos.astype(object) > tot.astype(object)
    cat = np.where(a == 1, 4, np.where((a == mx) & (nmax == 1), 0, np.where(a == mx, 1, np.where(above.astype(bool), 2, 3))))
    return cat, mx, [int((cat == k).sum()) for k in range(5)]


def prepare_numpy(case, cleavage):
    """sites[m] = every plus-strand site (half <= 16) of miRNA m: (half, FASTA index, o, classes, target bases)"""
    out = []
    for _, mc in case.mirnas:
        s = []
        for f, t in enumerate(case.seqs):
            s += [(half, f, o, C, Y) for half, o, _, C, Y in sites_numpy(mc, t, 16, False, cleavage)]
        out.append(s)
    return out


def restate_numpy(case, max_half=8, cleavage=False, max_category=4, alpha=1.0, prep=None):
    sites = prep if prep is not None else prepare_numpy(case, cleavage)
    t, p, a, sense, minus = units_numpy(case)
    cat, mx, C = categories_numpy(t, a)
    ccum = np.cumsum(C).tolist()
    look = {k: i for i, k in enumerate(zip(t.tolist(), p.tolist()))}
    cat_l, a_l, mx_l = cat.tolist(), a.tolist(), mx.tolist()
    hits = []
    for m, (mname, mc) in enumerate(case.mirnas):
        L = len(mc)
        ncum = np.cumsum(np.bincount([s[0] for s in sites[m]], minlength=17)).tolist()
        for half, f, o, Cc, Y in sites[m]:
            i = look.get((f, o + L - 9))
            if half > max_half or i is None or cat_l[i] > max_category:
                continue
            pv = pvalue(ncum[half], ccum[cat_l[i]], case.P)
            if pv <= alpha:
                hits.append((m, cat_l[i], half, f, o + L - 9, hit_line(mname, case.fa_names[f], o + L - 9, half, cat_l[i], a_l[i], mx_l[i], ncum[half], pv,
                                                                      mc, Cc, Y)))
    kept = int((cat <= max_category).sum())
    stats = dict(zip(STAT_KEYS, [len(case.recs), sense, minus, len(t)] + C + [kept * len(case.mirnas), len(hits)]))
    return _emit(hits), stats


# ---------------------------------------------------------------------------------------------------- the seeded input (also used on the GPU)
PLANT_DEPTHS = (1, 2, 3, 8, 40, 200)


def seeded_case(seed, n_tx=120, lo=300, hi=2500, n_mir=30, background=40, minus=0.15):
    """Transcripts of lo..hi nt, miRNAs of 19..24 nt each planted four times with 0..3 substitutions, up to `background` units per transcript with
    geometric depths, planted cleavage units with depths cycling through PLANT_DEPTHS, minus-strand records at planted and random positions, records
    outside 1..LN; a unit's depth is split over up to three records (the three SAM files of the GPU test).  The @SQ order is a shuffle of the FASTA
    order without its last transcript.  -> (Case, texts, miRNA letters)."""
    rng = np.random.RandomState(seed)
    texts = [bytearray(ACGT[rng.randint(0, 4, int(rng.randint(lo, hi + 1)))].tobytes()) for _ in range(n_tx)]
    mirs = random_mirnas(rng, n_mir, 19, 24, t_for_u=0.3)
    sq = list(rng.permutation(n_tx - 1))
    sq_of_fa = {int(f): s for s, f in enumerate(sq)}
    rows, k = [], 0
    for m in mirs:
        for _ in range(4):
            f = int(rng.randint(0, n_tx - 1))
            (o, _), = plant(rng, texts[f], m, 1, subs=(0, 3), both=False)
            rows.append((sq_of_fa[f], o + len(m) - 9, PLANT_DEPTHS[k % len(PLANT_DEPTHS)]))
            k += 1
    texts[3][40:44] = b"NNRY"
    texts[5][100:160] = bytes(texts[5][100:160]).lower()
    for f in range(n_tx - 1):
        for _ in range(int(rng.randint(0, background + 1))):
            rows.append((sq_of_fa[f], int(rng.randint(1, len(texts[f]) + 1)), int(rng.geometric(0.4))))
    recs = []
    for tid, p, a in rows:
        if p < 1:
            continue
        parts = [a] if a < 3 else [a - a // 2 - a // 3, a // 2, a // 3]
        for j, d in enumerate(parts):
            if d:
                recs.append((tid, p, d, int(rng.randint(18, 25)), 0, j))
        if rng.rand() < minus:
            recs.append((tid, p, int(rng.randint(1, 300)), 20, 1, int(rng.randint(0, 3))))
    for _ in range(30):
        tid = int(rng.randint(0, n_tx - 1))
        recs.append((tid, int(rng.choice([0, len(texts[sq[tid]]) + 1])), 5, 20, 0, int(rng.randint(0, 3))))
    names = ["tx%d" % i for i in range(n_tx)]
    mirnas = parse_mirnas(b"".join(b">mir%d\n%s\n" % (i, m) for i, m in enumerate(mirs)))
    seqs = [CODE[np.frombuffer(bytes(t), dtype=np.uint8)] for t in texts]
    case = Case(mirnas, names, seqs, [names[f] for f in sq], [len(texts[f]) for f in sq], make_records(recs))
    return case, [bytes(t) for t in texts], mirs


def _rows(data):
    assert data.startswith(HEADER)
    return [ln.split(b"\t") for ln in data[len(HEADER):].split(b"\n")[:-1]]


# ---------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("seed", [1, 2])
def test_restatements_agree_on_seeded_inputs(seed):
    case, _, _ = seeded_case(seed, n_tx=12, lo=200, hi=500, n_mir=6, background=25)
    seen = 0
    for cleavage in (False, True):
        pp, pn = prepare_plain(case, cleavage), prepare_numpy(case, cleavage)
        assert [sum(h) for h in pp] == [len(s) for s in pn]
        for max_half, max_category, alpha in ((8, 4, 1.0), (16, 4, 1.0), (10, 2, 1.0), (16, 4, 0.05), (0, 0, 1.0), (12, 3, 1e-3)):
            a = restate_plain(case, max_half, cleavage, max_category, alpha, pp)
            b = restate_numpy(case, max_half, cleavage, max_category, alpha, pn)
            assert a == b, (seed, cleavage, max_half, max_category, alpha)
            seen += a[1]["hits"]
    assert seen > 40


def test_seeded_shape_of_the_gpu_sweep():
    """The input of the GPU settings sweep: at least 50 hits at -s 5 with all five categories among them (numpy restatement)."""
    case, _, _ = seeded_case(7)
    data, stats = restate_numpy(case, max_half=10)
    rows = _rows(data)
    print("hits %d, by category %s, units %d, C %s" % (len(rows), [sum(r[6] == b"%d" % k for r in rows) for k in range(5)], stats["units"],
                                                      [stats["c%d" % k] for k in range(5)]))
    assert len(rows) >= 50 and {r[6] for r in rows} == {b"0", b"1", b"2", b"3", b"4"}
    assert stats["minus"] > 50 and stats["sense"] < stats["records"] - stats["minus"]


def _one_tx(units, mirna=MIR, text=None, **kw):
    """units {p: [depths]} on one transcript -> the rows of both restatements"""
    text = text if text is not None else b"ACGT" * 30
    case = Case(parse_mirnas(b">m\n" + mirna + b"\n"), ["t"], [CODE[np.frombuffer(text, dtype=np.uint8)]], ["t"], [len(text)],
                make_records([(0, p, d, 20, 0) for p, ds in units.items() for d in ds]))
    a, b = restate_plain(case, **kw), restate_numpy(case, **kw)
    assert a == b
    return case, _rows(a[0]), a[1]


def test_categories_by_hand():
    def cats(abund):
        case = Case([], ["t"], [np.zeros(100, np.uint8)], ["t"], [100], make_records([(0, 10 * (i + 1), a, 20, 0) for i, a in enumerate(abund)]))
        units, _, _ = units_plain(case)
        cat, amax, C = categories_plain(units)
        t, p, a, _, _ = units_numpy(case)
        cn, mx, Cn = categories_numpy(t, a)
        assert [cat[0, int(q)] for q in p] == cn.tolist() and C == Cn and set(mx.tolist()) == {max(abund)}
        return cn.tolist()
    assert cats([5, 5, 2, 1]) == [1, 1, 3, 4]
    assert cats([9, 5, 2, 1]) == [0, 2, 3, 4]        # tot 17, npos 4: 5 * 4 > 17, 2 * 4 <= 17
    assert cats([1]) == [4] and cats([2]) == [0]
    assert cats([1, 1]) == [4, 4] and cats([3, 3]) == [1, 1]
    assert cats([2 ** 31, 2 ** 31 - 1, 7]) == [0, 2, 3]


@pytest.mark.parametrize("L", [12, 21, 32])
def test_offset_identity(L):
    """A planted perfect site at offset o is hit only by the unit at o + L - 9 (1-based), whatever L is."""
    mir = random_mirnas(np.random.RandomState(L), 1, L, L, t_for_u=0)[0]
    o = 37
    text = bytearray(b"C" * 120)
    text[o:o + L] = target_of_mirna(mir)
    p = o + L - 9
    for q in (p - 1, p, p + 1):
        _, rows, stats = _one_tx({q: [3]}, mir, bytes(text), max_half=0)
        assert stats["units"] == 1 and stats["evaluations"] == 1
        if q != p:
            assert rows == []
            continue
        assert len(rows) == 1
        r = rows[0]
        assert r[:10] == [b"m", b"t", b"%d" % p, b"%d" % (o + 1), b"%d" % (o + L), b"0.0", b"0", b"3", b"3", b"1"]
        assert r[10] == b"%.3e" % (1 / 120) and r[13] == mir and r[14] == b"|" * L


def test_sites_off_the_transcript_or_on_an_n_give_no_hit():
    L = len(MIR)
    site = target_of_mirna(MIR)
    # the site would start before the transcript (o = p + 9 - L < 0) or end after it (p + 9 > len)
    text = site[5:] + b"C" * 40 + site[:L - 4]
    n = len(text)
    _, rows, stats = _one_tx({L - 9 - 5: [4], n - 9 + 4: [4], 1: [2], n: [2]}, MIR, text, max_half=16)
    assert rows == [] and stats["units"] == 4 and stats["evaluations"] == 4
    # whole sites at o = 0 and at o + L = len are hits
    text = site + b"C" * 40 + site
    _, rows, _ = _one_tx({L - 9: [4], len(text) - 9: [4]}, MIR, text, max_half=0)
    assert [(r[3], r[4]) for r in rows] == [(b"1", b"%d" % L), (b"%d" % (len(text) - L + 1), b"%d" % len(text))]
    # an N inside the site
    text = bytearray(b"C" * 30 + site + b"C" * 30)
    text[30 + 4] = ord("N")
    _, rows, _ = _one_tx({30 + L - 9: [4]}, MIR, bytes(text), max_half=16)
    assert rows == []
    text[30 + 4] = site[4]
    text[29] = ord("N")                                # next to the site: no matter
    _, rows, _ = _one_tx({30 + L - 9: [4]}, MIR, bytes(text), max_half=0)
    assert len(rows) == 1


def test_minus_strand_and_outside_records_change_only_the_summary():
    site = target_of_mirna(MIR)
    text = b"C" * 30 + site + b"C" * 30
    p = 30 + len(MIR) - 9
    base = [(0, p, 5, 20, 0), (0, 12, 2, 20, 0), (0, 12, 1, 20, 0)]
    extra = [(0, p, 100, 20, 1), (0, 3, 9, 20, 1), (0, 0, 9, 20, 0), (0, len(text) + 1, 9, 20, 0), (1, 5, 9, 20, 0)]
    out = []
    for rows in (base, base + extra):
        case = Case(parse_mirnas(b">m\n" + MIR + b"\n"), ["t"], [CODE[np.frombuffer(text, dtype=np.uint8)]], ["t"], [len(text)], make_records(rows))
        a, b = restate_plain(case, max_half=0), restate_numpy(case, max_half=0)
        assert a == b
        out.append(a)
    assert out[0][0] == out[1][0] and len(_rows(out[0][0])) == 1 and _rows(out[0][0])[0][6:9] == [b"0", b"5", b"5"]
    assert out[0][1] == dict(out[1][1], records=3, minus=0) and out[1][1]["records"] == 8 and out[1][1]["minus"] == 2 and out[1][1]["sense"] == 3


def test_cleavage_rule_and_pvalue_filter():
    L = len(MIR)
    site = bytearray(target_of_mirna(MIR))
    site[L - 10] = ord("C") if site[L - 10] != ord("C") else ord("A")      # a mismatch at miRNA position 10
    text = b"G" * 30 + bytes(site) + b"G" * 30
    p = 30 + L - 9
    _, rows, _ = _one_tx({p: [6]}, MIR, text, max_half=8)
    assert len(rows) == 1 and rows[0][5] == b"2.0" and rows[0][14][9:10] == b"x"
    assert _one_tx({p: [6]}, MIR, text, max_half=8, cleavage=True)[1] == []
    pv = float(rows[0][10])
    assert _one_tx({p: [6]}, MIR, text, max_half=8, alpha=pv * 1.01)[1] == rows
    assert _one_tx({p: [6]}, MIR, text, max_half=8, alpha=pv * 0.9)[1] == []
    assert _one_tx({p: [6]}, MIR, text, max_half=8, max_category=0)[1] == rows
    assert _one_tx({p: [1]}, MIR, text, max_half=8, max_category=3)[1] == []


def _exact(n, c, P):
    return 1 - Fraction(P - c, P) ** n


def test_pvalue_formula_against_exact_arithmetic():
    assert "%.3e" % pvalue(5, 7, 7) == "1.000e+00" and "%.3e" % pvalue(5, 9, 7) == "1.000e+00"
    triples = set()
    for seed in (1, 2):
        case, _, _ = seeded_case(seed, n_tx=12, lo=200, hi=500, n_mir=6, background=25)
        t, _, a, _, _ = units_numpy(case)
        _, _, C = categories_numpy(t, a)
        for s in prepare_numpy(case, False):
            ncum = np.cumsum(np.bincount([x[0] for x in s], minlength=17)).tolist()
            triples |= {(n, c, case.P) for n in ncum if n for c in np.cumsum(C).tolist() if c}
    rng = np.random.RandomState(1)
    for _ in range(10000):
        P = int(rng.randint(1000, 10 ** 7 + 1))
        triples.add((int(rng.randint(1, 3001)), int(rng.randint(1, min(P, 10 ** 6) + 1)), P))
    bad = [(n, c, P) for n, c, P in triples if "%.3e" % pvalue(n, c, P) != "%.3e" % float(_exact(n, c, P))]
    assert not bad, bad[:5]


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.degradome"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    m, t, s = tmp_path / "m.fa", tmp_path / "t.fa", tmp_path / "d.sam"
    m.write_bytes(b">m\n" + MIR + b"\n")
    t.write_bytes(b">t\nACGT\n")
    s.write_bytes(b"@SQ\tSN:t\tLN:4\n")
    ok = [str(m), str(t), str(s)]
    bad = [[], [str(m)], [str(m), str(t)], ["-s", "8.5"] + ok, ["-s", "-1"] + ok, ["-s", "0.25"] + ok, ["-s", "x"] + ok, ["--max-category", "5"] + ok,
           ["--max-category", "-1"] + ok, ["--max-category", "x"] + ok, ["-p", "0"] + ok, ["-p", "1.5"] + ok, ["-p", "-0.1"] + ok, ["-p", "x"] + ok,
           ["-p", ""] + ok, ["-p", "nan"] + ok, ["-p", "0e5"] + ok, ["--device", "-1"] + ok, ["-o", ""] + ok, ["-x"] + ok]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "m.fa").write_bytes(b">m\n" + MIR + b"\n")
    (tmp_path / "d.sam").write_bytes(b"@SQ\tSN:t\tLN:4\n")
    for args in (["nope.fa", "m.fa", "d.sam"], ["m.fa", "nope.fa", "d.sam"], ["m.fa", "m.fa", "nope.sam"], ["m.fa", "m.fa", "d.sam", "nope2.sam"]):
        r = run_cli([str(tmp_path / a) for a in args], tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope" in r.stderr.decode(), args


def test_helpers_of_the_command_line(capsys):
    from mir_prefer_amd import degradome
    assert [degradome.parse_alpha(x) for x in ("1", "0.05", "1e-3", ".5", "1.0", "5E-2", "0", "1.5", "-1", "", "nan", "inf", "1e", "0.0")] == \
        [1.0, 0.05, 1e-3, 0.5, 1.0, 0.05, None, None, None, None, None, None, None, None]
    assert degradome.output_name("d/x.sam") == "d/x.sam.degradome.tsv"
    o, m, t, sams, half, alpha, out = degradome.parse_args(["-s", "5", "-c", "--max-category", "2", "-p", "0.05", "m.fa", "t.fa", "a.sam", "b.sam"])
    assert (m, t, sams, half, alpha, out, o.cleavage_site, o.max_category) == ("m.fa", "t.fa", ["a.sam", "b.sam"], 10, 0.05, "a.sam.degradome.tsv", True, 2)
    o, _, _, _, half, alpha, out = degradome.parse_args(["-o", "x.tsv", "m.fa", "t.fa", "a.sam"])
    assert (half, alpha, out, o.max_category, o.cleavage_site) == (8, 1.0, "x.tsv", 4, None)
    with pytest.raises(SystemExit) as e:
        degradome.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--max-score", "--cleavage-site", "--max-category", "--max-pvalue", "--output", "--device"):
        assert opt in text
