"""Host tests of the partition function (mirp_ensemble, `ensemble`): a plain-Python / numpy restatement of the model -- the tables
parsed from csrc/energy_params_t2004.h (test_duplex_cpu's), an evaluator E(S) of a dot-bracket text, an enumerator of the structures of a short
sequence, and the inside / outside program of §23 written over a semiring, so that the same code runs as (sum, x) in extended precision and as
(min, +) on integers -- which the GPU tests (test_ensemble_gpu.py) compare the device with.  Here the restatement is pinned: Z and every p(i,j) to
the enumeration, the enumeration's minimum and the (min, +) run to the project's CPU oracle, and to the identities of §23; the table formatter and
the command line's option errors (exit 2 without a device) are tested as well."""
import math
import os
import random
import re

import numpy as np
import pytest

from tests.test_duplex_cpu import D3, D5, HAIRPIN, MM_H, MM_I, MM_1N, MM_23, PAIR, RTYPE, STACK, BULGE, ILOOP, T, TERM_AU, NINIO, MAX_NINIO, codes, e_ext, e_int
from tests.test_randfold_cpu import oracle_mfe
from tests.test_targets_cpu import ROOT

KT = 1.98717 * 310.15 / 1000
MAXLOOP = 30
ML_CLOSING, ML_INTERN, ML_BASE, LXC = T["ML_closing"], T["ML_intern"], T["ML_BASE"], T["LXC"]
MM_M = T["mismatchM"]
SPECIAL = {}
_text = open(os.path.join(ROOT, "mir-prefer_amd", "csrc", "energy_params_t2004.h")).read()
for _key, _n in (("Triloop", 5), ("Tetraloop", 6), ("Hexaloop", 8)):
    _names = re.findall(r'"([ACGU]+)"', re.search(r"T04_%ss\[\d+\]\[\d+\] = \{([^}]*)\}" % _key, _text).group(1))
    for _name, _e in zip(_names, T[_key + "_E"]):
        assert len(_name) == _n
        SPECIAL[_name] = _e
assert len(SPECIAL) == 22 and ML_BASE == 0


# ---------------------------------------------------------------------------------------------------- the loop terms of oracle/lfold.c (0-based)
def e_ml(t, a, b):
    e = ML_INTERN + (TERM_AU if t > 2 else 0)
    if a >= 0 and b >= 0:
        e += min(0, MM_M[t][a][b])
    elif a >= 0:
        e += min(0, D5[t][a])
    elif b >= 0:
        e += min(0, D3[t][b])
    return e


def e_hairpin(S, i, j, t):
    u = j - i - 1
    e = HAIRPIN[u] if u <= 30 else HAIRPIN[30] + int(LXC * math.log(u / 30.0))
    if u in (3, 4, 6):
        motif = "".join("NACGU"[c] for c in S[i:j + 1])
        if motif in SPECIAL:
            return SPECIAL[motif]
        if u == 3:
            return e + (TERM_AU if t > 2 else 0)
    return e + MM_H[t][S[i + 1]][S[j - 1]]


def pair_table(ss):
    stack, pt = [], {}
    for x, ch in enumerate(ss):
        if ch == "(":
            stack.append(x)
        elif ch == ")":
            pt[stack.pop()] = x
    assert not stack
    return pt


def energy_of(S, pairs):
    """E(S) of §23 for a set of pairs {i: j}; None when the structure is not in Omega (a pair that cannot form, a hairpin under 3, a loop over 30)"""
    n = len(S)
    total = 0

    def children(a, b):
        out, x = [], a
        while x <= b:
            if x in pairs:
                out.append((x, pairs[x]))
                x = pairs[x] + 1
            else:
                x += 1
        return out
    for p, q in children(0, n - 1):
        t = PAIR[S[p]][S[q]]
        if t:
            total += e_ext(t, S[p - 1] if p > 0 else -1, S[q + 1] if q < n - 1 else -1)
    for i, j in pairs.items():
        t = PAIR[S[i]][S[j]]
        if not t or j - i < 4:
            return None
        kids = children(i + 1, j - 1)
        if not kids:
            total += e_hairpin(S, i, j, t)
        elif len(kids) == 1:
            p, q = kids[0]
            if p - i - 1 + j - q - 1 > MAXLOOP:
                return None
            total += e_int(p - i - 1, j - q - 1, t, RTYPE[PAIR[S[p]][S[q]]], S[i + 1], S[j - 1], S[p - 1], S[q + 1])
        else:
            total += ML_CLOSING + e_ml(RTYPE[t], S[j - 1], S[i + 1]) + ML_BASE * (j - i - 1 - sum(q - p + 1 for p, q in kids))
            total += sum(e_ml(PAIR[S[p]][S[q]], S[p - 1], S[q + 1]) for p, q in kids)
    return total


def enumerate_structures(S):
    """every non-crossing set of pairs that can form with hairpins of at least 3, as dicts {i: j} (the loop limit is checked by energy_of)"""
    n = len(S)
    memo = {}

    def rec(a, b):            # structures on [a, b]
        if b - a < 4:
            return [()]
        if (a, b) in memo:
            return memo[(a, b)]
        out = list(rec(a + 1, b))
        for k in range(a + 4, b + 1):
            if PAIR[S[a]][S[k]]:
                for inner in rec(a + 1, k - 1):
                    for rest in rec(k + 1, b):
                        out.append(((a, k),) + inner + rest)
        memo[(a, b)] = out
        return out
    return [dict(s) for s in rec(0, n - 1)]


def enumerated(s):
    """-> (Z, {(i, j): p}, minimum energy, the dot-bracket texts' pair dicts) by enumeration, in extended precision"""
    S = codes(s)
    Z, w_pair, best, structs = np.longdouble(0), {}, None, []
    for pairs in enumerate_structures(S):
        e = energy_of(S, pairs)
        if e is None:
            continue
        structs.append(pairs)
        w = np.exp(np.longdouble(-e) / np.longdouble(100 * KT))
        Z += w
        best = e if best is None or e < best else best
        for ij in pairs.items():
            w_pair[ij] = w_pair.get(ij, np.longdouble(0)) + w
    return Z, {ij: w / Z for ij, w in w_pair.items()}, best, structs


# ---------------------------------------------------------------------------------------------------- the two semirings
class SumProduct:
    """(sum, x) on Boltzmann weights in extended precision (x87: 64-bit mantissa, exponents to 2^16383 -- e^8000 fits)"""
    dtype = np.longdouble
    zero, one = np.longdouble(0), np.longdouble(1)

    @staticmethod
    def weight(e):
        return np.exp(np.asarray(e, dtype=np.longdouble) * np.longdouble(-1.0) / np.longdouble(100 * KT))

    @staticmethod
    def times(a, b):
        return a * b

    @staticmethod
    def plus(a, b):
        return a + b

    @staticmethod
    def total(v):
        return v.sum() if len(v) else np.longdouble(0)


class MinPlus:
    """(min, +) on energies in 0.01 kcal/mol"""
    dtype = np.int64
    zero, one = np.int64(1 << 40), np.int64(0)

    @staticmethod
    def weight(e):
        return np.asarray(e, dtype=np.int64)

    @staticmethod
    def times(a, b):
        return np.minimum(a + b, np.int64(1 << 40))

    @staticmethod
    def plus(a, b):
        return np.minimum(a, b)

    @staticmethod
    def total(v):
        return v.min() if len(v) else np.int64(1 << 40)


# the interior loops of a cell as arrays over the shapes (n1, n2), ordered by size: all but 1x1, 1x2, 2x1, 2x2 (scalar e_int) are
# base[k] + stack? + TerminalAU (both pairs)? + mismatch table m[k] of either pair
_SPECIAL_SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2))
_SHAPES = sorted(((a, b) for a in range(31) for b in range(31 - a) if (a, b) not in _SPECIAL_SHAPES), key=lambda ab: (ab[0] + ab[1], ab[0]))
_N1 = np.array([a for a, _ in _SHAPES])
_N2 = np.array([b for _, b in _SHAPES])
_SIZE = _N1 + _N2
_COUNT_UP_TO = [int((_SIZE <= u).sum()) for u in range(31)]
_BASE, _STK, _TAU, _MMK = [], [], [], []
for _a, _b in _SHAPES:
    _nl, _ns = max(_a, _b), min(_a, _b)
    if _nl == 0:
        _row = (0, 1, 0, 0)
    elif _ns == 0:
        _row = (BULGE[1], 1, 0, 0) if _nl == 1 else (BULGE[_nl], 0, 1, 0)
    elif _ns == 1:
        _row = (ILOOP[_nl + 1] + min(MAX_NINIO, (_nl - 1) * NINIO), 0, 0, 2)
    elif _ns == 2 and _nl == 3:
        _row = (ILOOP[5] + NINIO, 0, 0, 3)
    else:
        _row = (ILOOP[_nl + _ns] + min(MAX_NINIO, (_nl - _ns) * NINIO), 0, 0, 1)
    for _lst, _v in zip((_BASE, _STK, _TAU, _MMK), _row):
        _lst.append(_v)
_BASE, _STK, _TAU, _MMK = (np.array(x, dtype=np.int64) for x in (_BASE, _STK, _TAU, _MMK))
_MMALL = np.array([np.zeros((8, 5, 5), dtype=np.int64).tolist(), MM_I, MM_1N, MM_23], dtype=np.int64)
_STACKA = np.array(STACK, dtype=np.int64)
_TAUV = np.array([0, 0, 0, TERM_AU, TERM_AU, TERM_AU, TERM_AU, 0], dtype=np.int64)
_PAIRA = np.array(PAIR, dtype=np.int64)
_RTYPEA = np.array(RTYPE, dtype=np.int64)


def _loops(S, Sa, o_i, o_j, t, n_shapes):
    """the interior loops closed by the pair (o_i, o_j) of type t: arrays (p, q, energy) over the inner pairs that can form, the first n_shapes
    vector shapes and the four special ones"""
    p, q = o_i + 1 + _N1[:n_shapes], o_j - 1 - _N2[:n_shapes]
    t2 = _PAIRA[Sa[p], Sa[q]]
    ok = np.nonzero(t2)[0]
    p, q, t2 = p[ok], q[ok], _RTYPEA[t2[ok]]
    mk = _MMK[ok]
    e = (_BASE[ok] + _STK[ok] * _STACKA[t, t2] + _TAU[ok] * (_TAUV[t] + _TAUV[t2]) + _MMALL[mk, t, Sa[o_i + 1], Sa[o_j - 1]]
         + _MMALL[mk, t2, Sa[q + 1], Sa[p - 1]])
    ps, qs, es = list(p), list(q), list(e)
    for n1, n2 in _SPECIAL_SHAPES:
        pp, qq = o_i + 1 + n1, o_j - 1 - n2
        if qq - pp >= 4 and PAIR[S[pp]][S[qq]]:
            ps.append(pp)
            qs.append(qq)
            es.append(e_int(n1, n2, t, RTYPE[PAIR[S[pp]][S[qq]]], S[o_i + 1], S[o_j - 1], S[pp - 1], S[qq + 1]))
    return np.array(ps, dtype=np.int64), np.array(qs, dtype=np.int64), np.array(es, dtype=np.int64)


def _loops_around(S, Sa, i_i, i_j, rt, n):
    """the interior loops whose inner pair is (i_i, i_j) (rt = its rtype'd type, 0 < i_i, i_j < n - 1): arrays (p, q, energy) over the outer pairs"""
    p, q = i_i - 1 - _N1, i_j + 1 + _N2
    ok = np.nonzero((p >= 0) & (q <= n - 1))[0]
    p, q = p[ok], q[ok]
    t = _PAIRA[Sa[p], Sa[q]]
    sub = np.nonzero(t)[0]
    ok, p, q, t = ok[sub], p[sub], q[sub], t[sub]
    mk = _MMK[ok]
    e = (_BASE[ok] + _STK[ok] * _STACKA[t, rt] + _TAU[ok] * (_TAUV[t] + _TAUV[rt]) + _MMALL[mk, t, Sa[p + 1], Sa[q - 1]]
         + _MMALL[mk, rt, Sa[i_j + 1], Sa[i_i - 1]])
    ps, qs, es = list(p), list(q), list(e)
    for n1, n2 in _SPECIAL_SHAPES:
        pp, qq = i_i - 1 - n1, i_j + 1 + n2
        if pp >= 0 and qq <= n - 1 and PAIR[S[pp]][S[qq]]:
            ps.append(pp)
            qs.append(qq)
            es.append(e_int(n1, n2, PAIR[S[pp]][S[qq]], rt, S[pp + 1], S[qq - 1], S[i_i - 1], S[i_j + 1]))
    return np.array(ps, dtype=np.int64), np.array(qs, dtype=np.int64), np.array(es, dtype=np.int64)


def inside(s, R):
    """the inside recursions of §23 over the semiring R -> dict of the tables ([i][j], 0-based) and Q5 (Q5[j + 1] = the prefix [0, j])"""
    S = codes(s)
    Sa = np.array(S + [0], dtype=np.int64)
    n = len(S)
    Qb, Qm1, U, Qm, Qmm = (np.full((n + 1, n + 1), R.zero, dtype=R.dtype) for _ in range(5))
    for d in range(4, n):
        n_shapes = _COUNT_UP_TO[min(MAXLOOP, d - 6)] if d >= 6 else 0
        for i in range(n - d):
            j = i + d
            t = PAIR[S[i]][S[j]]
            if t:
                v = R.weight(e_hairpin(S, i, j, t))
                if d >= 6:
                    p, q, e = _loops(S, Sa, i, j, t, n_shapes)
                    keep = q - p >= 4
                    v = R.plus(v, R.total(R.times(R.weight(e[keep]), Qb[p[keep], q[keep]])))
                v = R.plus(v, R.times(R.weight(ML_CLOSING + e_ml(RTYPE[t], S[j - 1], S[i + 1])), Qmm[i + 1, j - 1]))
                Qb[i, j] = v
                Qm1[i, j] = R.plus(Qm1[i, j - 1], R.times(v, R.weight(e_ml(t, S[i - 1] if i > 0 else -1, S[j + 1] if j < n - 1 else -1))))
            else:
                Qm1[i, j] = Qm1[i, j - 1]
            if ML_BASE:
                raise NotImplementedError
            U[i, j] = R.plus(U[i + 1, j], Qm1[i, j])
            Qmm[i, j] = R.total(R.times(Qm[i, i + 4:j - 4], Qm1[i + 5:j - 3, j]))
            Qm[i, j] = R.plus(U[i, j], Qmm[i, j])
    Q5 = np.full(n + 1, R.one, dtype=R.dtype)
    ext = {}
    for j in range(n):
        v = Q5[j]
        for k in range(0, j - 3):
            t = PAIR[S[k]][S[j]]
            if t:
                ext[(k, j)] = R.weight(e_ext(t, S[k - 1] if k > 0 else -1, S[j + 1] if j < n - 1 else -1))
                v = R.plus(v, R.times(R.times(Q5[k], Qb[k, j]), ext[(k, j)]))
        Q5[j + 1] = v
    return dict(S=S, Sa=Sa, n=n, Qb=Qb, Qm1=Qm1, U=U, Qm=Qm, Qmm=Qmm, Q5=Q5, ext=ext)


def outside(I, R=SumProduct):
    """the reverse-mode derivative of inside(): Pb[i][j] = dZ / dQb(i,j)"""
    S, Sa, n, Qb, Qm1, Qm, Q5, ext = I["S"], I["Sa"], I["n"], I["Qb"], I["Qm1"], I["Qm"], I["Q5"], I["ext"]
    P5 = np.full(n + 1, R.zero, dtype=R.dtype)          # P5[j + 1] = dZ / dQ5(prefix [0, j])
    P5[n] = R.one
    for jp in range(n - 1, -1, -1):                      # the prefix that ends at jp - 1
        v = P5[jp + 1]
        for j in range(jp + 4, n):
            if (jp, j) in ext:
                v = R.plus(v, R.times(R.times(P5[j + 1], Qb[jp, j]), ext[(jp, j)]))
        P5[jp] = v
    Pb, A1, AU, Amm = (np.full((n + 2, n + 2), R.zero, dtype=R.dtype) for _ in range(4))
    for d in range(n - 1, 3, -1):
        for i in range(n - d):
            j = i + d
            am = R.total(R.times(Amm[i, j + 5:n], Qm1[j + 1, j + 5:n]))
            amm = am
            if i >= 1 and j + 1 < n:
                t = PAIR[S[i - 1]][S[j + 1]]
                if t:
                    amm = R.plus(amm, R.times(Pb[i - 1, j + 1], R.weight(ML_CLOSING + e_ml(RTYPE[t], S[j], S[i]))))
            au = R.plus(AU[i - 1, j] if i >= 1 else R.zero, am)
            a1 = R.plus(R.plus(A1[i, j + 1], au), R.total(R.times(Amm[0:max(i - 4, 0), j], Qm[0:max(i - 4, 0), i - 1])))
            t = PAIR[S[i]][S[j]]
            if t:
                v = R.times(R.times(Q5[i], P5[j + 1]), ext[(i, j)])
                v = R.plus(v, R.times(a1, R.weight(e_ml(t, S[i - 1] if i > 0 else -1, S[j + 1] if j < n - 1 else -1))))
                # the pairs (p, q) around (i, j): the loops of _loops seen from inside
                if 0 < i and j < n - 1:
                    p, q, e = _loops_around(S, Sa, i, j, RTYPE[t], n)
                    v = R.plus(v, R.total(R.times(R.weight(e), Pb[p, q])))
                Pb[i, j] = v
            A1[i, j], AU[i, j], Amm[i, j] = a1, au, amm
    return Pb


def restate(s, want_p=True):
    """-> dict(n, lnz, efe, p = {(i, j) 0-based: p > 0 as float}, diversity, centroid (text), centroid_dist, min_gap = the smallest |p - 0.5|)"""
    I = inside(s, SumProduct)
    n, Z = I["n"], I["Q5"][I["n"]]
    lnz = float(np.log(Z))
    out = dict(n=n, lnz=lnz, efe=0.0 - KT * lnz)
    if not want_p:
        return out
    Pb = outside(I)
    p = {}
    for i in range(n):
        for j in range(i + 4, n):
            if I["Qb"][i, j] != 0:
                v = float(I["Qb"][i, j] * Pb[i, j] / Z)
                if v > 0:
                    p[(i, j)] = v
    text = ["."] * n
    for (i, j), v in p.items():
        if v > 0.5:
            text[i], text[j] = "(", ")"
    out.update(p=p, diversity=2 * math.fsum(v * (1 - v) for v in p.values()), centroid="".join(text),
               centroid_dist=math.fsum(1 - v if v > 0.5 else v for v in p.values()), min_gap=min([abs(v - 0.5) for v in p.values()] + [0.5]))
    return out


def record_of(r, mfe):
    """the fields of MirpEnsembleRec from restate()'s result and the MFE"""
    return dict(len=r["n"], mfe=mfe, efe=r["efe"], mfe_freq=math.exp((r["efe"] - mfe / 100) / KT), diversity=r["diversity"], centroid_dist=r["centroid_dist"],
                centroid_pairs=r["centroid"].count("("))


def mfe_min_plus(s):
    I = inside(s, MinPlus)
    return int(I["Q5"][I["n"]])


# ---------------------------------------------------------------------------------------------------- sequences
def random_seq(rng, n, alphabet="ACGU"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def revcomp(s):
    return "".join({"A": "U", "C": "G", "G": "C", "U": "A"}.get(ch, "N") for ch in reversed(s))


def planted_hairpin(rng, n, alphabet="ACGU", loop=None, edits=3):
    """a stem with a few mismatches around a loop, with random flanks, n nt in all"""
    loop = rng.randint(4, 9) if loop is None else loop
    arm = max(4, min((n - loop) // 2 - rng.randint(0, 3), (n - loop) // 2))
    a = random_seq(rng, arm, alphabet)
    b = list(revcomp(a))
    for _ in range(edits):
        b[rng.randrange(len(b))] = rng.choice("ACGU")
    core = a + random_seq(rng, loop, alphabet) + "".join(b)
    flank = n - len(core)
    left = rng.randint(0, flank) if flank > 0 else 0
    return (random_seq(rng, left, alphabet) + core + random_seq(rng, flank - left, alphabet))[:n]


def seeded(seed, count, lo, hi):
    """`count` sequences of lo..hi nt, alternately random and a planted hairpin"""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = rng.randint(lo, hi)
        out.append(random_seq(rng, n) if k % 2 == 0 else planted_hairpin(rng, n))
    return out


MULTI = "GGAAACGAAACC"
SHORT = seeded(2301, 44, 8, 18) + [MULTI]


def realistic():
    rng = random.Random(2304)
    out = seeded(2305, 24, 40, 160)
    out += [planted_hairpin(rng, n) for n in (200, 250, 300)]
    out += [random_seq(rng, n, "GU") for n in (40, 77)] + [planted_hairpin(rng, n, "GGUUAC") for n in (60, 120, 181)]        # GU-rich
    for n in (45, 90, 150):                                                                                                       # N-containing
        s = list(planted_hairpin(rng, n))
        for _ in range(n // 12):
            s[rng.randrange(n)] = rng.choice("NRYX")
        out.append("".join(s))
    arm = random_seq(rng, 14, "GC")
    out.append("AU" + arm + random_seq(rng, 41, "A") + revcomp(arm) + "UA")                                                       # a hairpin loop over 30
    out += [planted_hairpin(rng, n, loop=34) for n in (80, 110)]
    out += seeded(2306, 6, 40, 100)
    return out


REALISTIC = realistic()


@pytest.fixture(scope="module")
def short_cases():
    return [(s, enumerated(s), inside(s, SumProduct)) for s in SHORT]


# ---------------------------------------------------------------------------------------------------- the pins
def test_enumeration_z(short_cases):
    assert len(SHORT) >= 41
    for s, (Z, _, _, structs), I in short_cases:
        got = I["Q5"][I["n"]]
        assert abs(got - Z) <= np.longdouble(1e-12) * Z, s
    multi = dict(pair_table("((...)(...))"))
    assert any(st == multi for st in short_cases[-1][1][3]), "the multiloop ((...)(...)) is a structure of " + MULTI
    assert sum(len(c[1][3]) for c in short_cases) > 2000


def test_enumeration_p(short_cases):
    seen = 0
    for s, (Z, p_enum, _, _), I in short_cases:
        Pb = outside(I)
        n = I["n"]
        for i in range(n):
            for j in range(i + 1, n):
                got = float(I["Qb"][i, j] * Pb[i, j] / Z)
                want = float(p_enum.get((i, j), 0))
                assert abs(got - want) <= 1e-12, (s, i, j, got, want)
                seen += want > 0
    assert seen > 500


def test_enumerated_minimum_is_the_oracle_mfe(short_cases):
    for s, (_, _, best, _), _ in short_cases:
        assert best == oracle_mfe((s.encode(), "vienna-2.1.2")), s
        assert mfe_min_plus(s) == best, s


def test_min_plus_is_the_oracle_mfe_at_realistic_lengths():
    assert len(REALISTIC) >= 40 and min(map(len, REALISTIC)) >= 40 and max(map(len, REALISTIC)) == 300
    assert any("N" in s for s in REALISTIC) and any(set(s) <= set("GU") for s in REALISTIC)
    folded = 0
    for s in REALISTIC:
        want = oracle_mfe((s.encode(), "vienna-2.1.2"))
        assert mfe_min_plus(s) == want, s
        folded += want < 0
    assert folded >= 30
    big = REALISTIC[-9]          # its MFE structure closes a hairpin loop over 30
    assert "A" * 41 in big and oracle_mfe((big.encode(), "vienna-2.1.2")) < -1000


def test_identities():
    r = restate("AAAA")
    assert r["lnz"] == 0.0 and r["efe"] == 0.0 and r["centroid"] == "...." and r["p"] == {} and r["diversity"] == 0
    for s in SHORT[:12] + REALISTIC[:4]:
        r = restate(s)
        n = r["n"]
        rows = [0.0] * n
        for (i, j), v in r["p"].items():
            rows[i] += v
            rows[j] += v
        assert max(rows) <= 1 + 1e-12, s
        mfe = oracle_mfe((s.encode(), "vienna-2.1.2"))
        assert 0 < record_of(r, mfe)["mfe_freq"] <= 1 + 1e-12, s
        assert r["efe"] <= mfe / 100 + 1e-12
    H = "GGGCGCAGCGAAAGCGCAGCGCCC"            # no U: a leading run of A pairs with nothing and is the same dangle for every length
    efes = [restate("A" * k + H, want_p=False)["efe"] for k in (1, 2, 5, 30)]
    assert max(efes) - min(efes) <= 1e-12 and efes[0] < -5
    assert abs(restate(H, want_p=False)["efe"] - efes[0]) > 1e-3


# ---------------------------------------------------------------------------------------------------- the table and the command line
def test_table_formatter():
    from mir_prefer_amd import ensemble
    recs = [dict(len=12, mfe=-130, efe=-1.4567, mfe_freq=0.5898123, diversity=1.234, centroid_dist=0.905, centroid_pairs=3),
            dict(len=4, mfe=0, efe=0.0, mfe_freq=1.0, diversity=0.0, centroid_dist=-0.0, centroid_pairs=0)]
    text = ensemble.table(["a", "b c"], recs, [b"(((......)))", "...."])
    assert text == ("name\tlength\tmfe\tefe\tmfe_freq\tdiversity\tcentroid_dist\tcentroid\n"
                    "a\t12\t-1.30\t-1.46\t0.589812\t1.23\t0.91\t(((......)))\n"
                    "b c\t4\t0.00\t0.00\t1\t0.00\t0.00\t....\n")
    bpp = np.array([(0, 1, 12, 0, 0.98765432), (1, 2, 9, 0, 0.001)], dtype=[("seq", "<i4"), ("i", "<i4"), ("j", "<i4"), ("reserved", "<i4"), ("p", "<f8")])
    assert ensemble.bpp_table(["a", "b"], bpp) == "a\t1\t12\t0.987654\nb\t2\t9\t0.001000\n"
    assert ensemble.output_name("x.fa") == "x.fa.ensemble.tsv"
    assert ensemble.bpp_name("x.fa.ensemble.tsv") == "x.fa.ensemble.bpp.tsv" and ensemble.bpp_name("out") == "out.bpp.tsv"


def test_option_errors_exit_2_before_a_device(tmp_path, capsys):
    import subprocess
    import sys
    from mir_prefer_amd import ensemble
    fa = tmp_path / "p.fa"
    fa.write_bytes(b">p\nGGGAAACCC\n")
    bad = [[], [str(fa), str(fa)], ["-c", "0", str(fa)], ["-c", "1.5", str(fa)], ["-c", "-0.1", str(fa)], ["-c", "nan", str(fa)], ["-c", "x", str(fa)],
           ["--device", "-1", str(fa)], ["-o", "", str(fa)], ["-x", str(fa)]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            ensemble.parse_args(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    assert ensemble.parse_args(["-p", "-c", "1", str(fa)])[0].cutoff == 1 and ensemble.parse_args([str(fa)])[0].cutoff == 0.001
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.ensemble", "-c", "2", str(fa)], cwd=str(tmp_path), capture_output=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2 and b"Error: " not in r.stderr, r.stderr.decode()
    assert not list(tmp_path.glob("*.tsv"))


def test_abi_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_ensemble(", "mirp_set_ensemble_capacity(", "mirp_ensemble_last_stats(", "MirpEnsembleOpts", "MirpEnsembleRec", "MirpBpp"):
        assert name in header
    from mir_prefer_amd import capi
    assert capi.ENSEMBLE_DTYPE.itemsize == 48 and capi.BPP_DTYPE.itemsize == 24


def restate_job(s):
    """sequence -> (restate(s), record_of with the oracle's MFE); a module-level function so that worker processes can run it"""
    s = s.decode() if isinstance(s, bytes) else s
    r = restate(s)
    return r, record_of(r, oracle_mfe((s.encode(), "vienna-2.1.2")))


def qualifies(r, cutoffs=()):
    """no p of restate()'s result within 1e-6 of 0.5 or of a cutoff of the pair list: the comparisons that depend on a threshold are decided"""
    return r["min_gap"] >= 1e-6 and all(abs(v - c) >= 1e-6 for v in r["p"].values() for c in cutoffs)


def range_hairpin():
    """300 nt over A C G (no U, so a leading run of A pairs with nothing): a G/C stem of 140 pairs with a few A mismatches"""
    rng = random.Random(2307)
    a = random_seq(rng, 140, "GC")
    b = list(revcomp(a))
    for x in rng.sample(range(8, 132), 6):
        b[x] = "A"
    h = "AC" + a + "GAAAAAAC" + "".join(b) + "CAACAAGAAC"
    assert len(h) == 300 and "U" not in h
    return h
