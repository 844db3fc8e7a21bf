"""Host tests of the bulged target sites (python -m mir_prefer_amd.targets --bulge; DESIGN.md §14, "Bulged sites").  Three restatements of the
definition, each producing the TSV bytes: a plain-Python enumeration over offset, kind and placement P (the reference); an alignment DP over the
target-strand text of an interval that allows at most one single-base gap, followed by the same tie, -c and domination rules; and a numpy
enumeration over all offsets at once, which the GPU tests (test_targets_bulge_gpu.py) compare whole files with.  The three agree on seeded random
inputs; hand-made cases pin the placements, the gap cost, the tie, -c, the blocks, the contig edges and the domination rule; the command line's
option errors exit 2 without a device."""
import numpy as np
import pytest

from tests.test_targets_cpu import (ACGT, CLS, CODE, HEADER, MCODE, MIR, PAIR, RNA, parse_mirnas, plant, random_mirnas, restate_numpy, run_cli,
                                    score_site, target_of_mirna)

BHEADER = HEADER[:-1] + b"\tbulge\n"
KIND_M, KIND_U, KIND_T = 0, 1, 2             # in the order of their ends at one start: o + L - 1, o + L, o + L + 1
COST = (0, 1, 2)


def weight(i):
    return 2 if 2 <= i <= 13 else 1


def gap_cost(kind, P):
    if kind == KIND_T:
        return 4 if 2 <= P <= 12 else 2
    return 4 if P <= 13 else 2


def span(kind, L):
    return L + kind - 1


def partner(L, o, strand, kind, P, i):
    """Index on the forward target of the base paired with miRNA position i in the site (kind, P) whose interval starts at o; None for the
    unpaired position of an m site."""
    if kind == KIND_T:
        u = (o + 1 if i <= P else o) if strand == 0 else (o if i <= P else o + 1)
    elif kind == KIND_M:
        if i == P:
            return None
        u = (o - 1 if i < P else o) if strand == 0 else (o if i < P else o - 1)
    else:
        u = o
    return u + i - 1 if strand else u + L - i


# ---------------------------------------------------------------------------------------------------- 1: the plain enumeration
def columns(mc, t, o, strand, kind, P):
    """The aligned columns of a site: [(miRNA position or 0, target-strand base or -1)], 5'->3' on the miRNA."""
    L = len(mc)
    cols = []
    for i in range(1, L + 1):
        q = partner(L, o, strand, kind, P, i)
        x = None if q is None else int(t[q])
        cols.append((i, -1 if x is None else (3 - x if strand else x)))
        if kind == KIND_T and i == P:
            x = int(t[o + P] if strand else t[o + L - P])
            cols.append((0, 3 - x if strand else x))
    return cols


def score_columns(mc, cols, kind, P):
    half, mm = 0, set()
    for i, y in cols:
        if i and y >= 0:
            k = int(CLS[mc[i - 1], y])
            half += weight(i) * COST[k]
            if k == 2:
                mm.add(i)
    return half + (gap_cost(kind, P) if kind != KIND_U else 0), mm


def bulge_site_plain(mc, t, o, strand, kind, cleavage):
    """The bulged site of one kind whose interval starts at o -> (half, P, columns) or None: outside the target, an ambiguous base in the interval,
    rejected by -c, or dominated by one of its two ungapped alignments."""
    L = len(mc)
    n = span(kind, L)
    if o < 0 or o + n > len(t) or any(int(x) > 3 for x in t[o:o + n]):
        return None
    best = None
    for P in range(1 if kind == KIND_T else 2, L):
        cols = columns(mc, t, o, strand, kind, P)
        half, mm = score_columns(mc, cols, kind, P)
        if best is None or half < best[0]:
            best = (half, P, cols, mm)
    half, P, cols, mm = best
    if cleavage and (10 in mm or 11 in mm or P == 10 or (kind == KIND_M and P == 11)):
        return None
    first, second = (o + 1, o) if kind == KIND_T else (o - 1, o)          # plus: A, B; minus: B, A (the rule treats A and B alike)
    for u in (first, second):
        r = score_site(mc, t, u, strand, cleavage)
        if r is not None and r[0] <= half:
            return None
    return half, P, cols


# ---------------------------------------------------------------------------------------------------- 2: the alignment DP
def bulge_site_dp(mc, t, o, strand, kind, cleavage):
    """The same site from an alignment of the miRNA (5'->3') with the interval's target-strand text y (3'->5'), at most one single-base gap:
    D0[i] = cost of positions 1..i without a gap, G[i] = (cost, P) of positions 1..i with the gap used."""
    L = len(mc)
    n = span(kind, L)
    if o < 0 or o + n > len(t):
        return None
    fwd = [int(x) for x in t[o:o + n]]
    if max(fwd) > 3:
        return None
    y = [0] + ([3 - x for x in fwd] if strand else fwd[::-1])            # y[c], c = 1 .. n

    def c(i, col):
        return weight(i) * COST[int(CLS[mc[i - 1], y[col]])]
    D0 = [0] * (L + 1)
    for i in range(1, min(L, n) + 1):
        D0[i] = D0[i - 1] + c(i, i)
    G = [None] * (L + 1)
    for i in range(1, L + 1):
        cand = []
        if kind == KIND_T:
            if G[i - 1] is not None:
                cand.append((G[i - 1][0] + c(i, i + 1), G[i - 1][1]))
            if i <= L - 1:
                cand.append((D0[i] + gap_cost(kind, i), i))              # y[i + 1] stays unpaired
        else:
            if G[i - 1] is not None:
                cand.append((G[i - 1][0] + c(i, i - 1), G[i - 1][1]))
            if 2 <= i <= L - 1:
                cand.append((D0[i - 1] + gap_cost(kind, i), i))          # position i stays unpaired
        G[i] = min(cand) if cand else None
    half, P = G[L]
    if kind == KIND_T:
        cols = [(i, y[i]) for i in range(1, P + 1)] + [(0, y[P + 1])] + [(i, y[i + 1]) for i in range(P + 1, L + 1)]
    else:
        cols = [(i, y[i]) for i in range(1, P)] + [(P, -1)] + [(i, y[i - 1]) for i in range(P + 1, L + 1)]
    if cleavage:
        if P == 10 or (kind == KIND_M and P == 11):
            return None
        for i, b in cols:
            if i in (10, 11) and b >= 0 and CLS[mc[i - 1], b] == 2:
                return None
    for u in ((o, o + 1) if kind == KIND_T else (o, o - 1)):
        r = score_site(mc, t, u, strand, cleavage)
        if r is not None and r[0] <= half:
            return None
    return half, P, cols


# ---------------------------------------------------------------------------------------------------- the lines
def bulge_line(mname, tname, o, L, strand, half, mc, kind, P, cols):
    cls = [int(CLS[mc[i - 1], y]) if i and y >= 0 else 3 for i, y in cols]
    return b"%s\t%s\t%d\t%d\t%s\t%d.%d\t%d\t%d\t%s\t%s\t%s\t%s\n" % (
        mname, tname.encode(), o + 1, o + span(kind, L), b"-" if strand else b"+", half // 2, 5 * (half & 1), cls.count(2), cls.count(1),
        bytes(RNA[mc[i - 1]] if i else ord("-") for i, _ in cols), bytes((PAIR + b"-")[k] for k in cls),
        bytes(RNA[y] if y >= 0 else ord("-") for _, y in cols), b"." if kind == KIND_U else b"%s%d" % (b"t" if kind == KIND_T else b"m", P))


def emit(sites, max_half, both, k):
    """sites: (m, half, tid, o, strand, kind, line) -> the TSV bytes: miRNA, score, target, start, + before -, end; -k over the lines of all kinds"""
    out, per = [BHEADER], {}
    for s in sorted(x for x in sites if x[1] <= max_half and (both or x[4] == 0)):
        per[s[0]] = per.get(s[0], 0) + 1
        if k == 0 or per[s[0]] <= k:
            out.append(s[6])
    return b"".join(out)


def restate_bulge(mirnas, names, seqs, max_half=8, both=False, cleavage=False, k=0, site=bulge_site_plain):
    sites = []
    for m, (mname, mc) in enumerate(mirnas):
        L = len(mc)
        for tid, t in enumerate(seqs):
            for o in range(len(t)):
                for strand in ((0, 1) if both else (0,)):
                    r = score_site(mc, t, o, strand, cleavage)
                    if r is not None and r[0] <= max_half:
                        cols = [(i + 1, y) for i, y in enumerate(r[2])]
                        sites.append((m, r[0], tid, o, strand, KIND_U, bulge_line(mname, names[tid], o, L, strand, r[0], mc, KIND_U, 0, cols)))
                    for kind in (KIND_M, KIND_T):
                        r = site(mc, t, o, strand, kind, cleavage)
                        if r is not None and r[0] <= max_half:
                            sites.append((m, r[0], tid, o, strand, kind, bulge_line(mname, names[tid], o, L, strand, r[0], mc, kind, r[1], r[2])))
    return emit(sites, max_half, both, k)


# ---------------------------------------------------------------------------------------------------- 3: numpy, all offsets at once
def sites_bulge_numpy(mc, t, cleavage, max_half=16):
    """Every site (ungapped and bulged, both strands) of one miRNA on one target with half <= max_half -> [(half, o, strand, kind, P)].
    Row r of the padded windows is the ungapped alignment U(r - 1); S[r, i] = the weighted cost of its positions 1..i."""
    L, n = len(mc), len(t)
    if n < L - 1:
        return []
    tp = np.concatenate([[4], t, [4, 4]]).astype(np.int64)
    W = np.lib.stride_tricks.sliding_window_view(tp, L)
    amb = np.concatenate([[0], np.cumsum(t > 3)])
    wts = np.array([weight(i) for i in range(1, L + 1)])
    out = []
    for strand in (0, 1):
        Y = (3 - np.minimum(W, 3)) if strand else np.minimum(W, 3)[:, ::-1]
        C = CLS[mc[None, :], Y]
        S = np.concatenate([np.zeros((len(W), 1), np.int64), np.cumsum(np.array(COST)[C] * wts, axis=1)], axis=1)
        MM = C == 2
        own = ~(W > 3).any(axis=1)                                        # U(r - 1) is a site of its own ...
        if cleavage:
            own &= ~(MM[:, 9] | MM[:, 10])                                # ... that passes -c
        for r in np.flatnonzero(own & (S[:, L] <= max_half)):
            out.append((int(S[r, L]), int(r) - 1, strand, KIND_U, 0))
        for kind in (KIND_M, KIND_T):
            ln = span(kind, L)
            o = np.arange(0, n - ln + 1)
            if len(o) == 0:
                continue
            ok = amb[o + ln] == amb[o]
            rA, rB = ((o + 2, o + 1) if kind == KIND_T else (o, o + 1))[::-1 if strand else 1]
            Ps = np.arange(1 if kind == KIND_T else 2, L)
            gaps = np.array([gap_cost(kind, P) for P in Ps])
            five = S[rA][:, Ps] if kind == KIND_T else S[rA][:, Ps - 1]
            tot = five + S[rB][:, L:L + 1] - S[rB][:, Ps] + gaps
            best = tot.min(axis=1)
            P = Ps[tot.argmin(axis=1)]                                    # the first minimum: the smallest P
            if cleavage:
                for i in (10, 11):
                    ok &= ~np.where(P > i if kind == KIND_M else P >= i, MM[rA, i - 1], MM[rB, i - 1]) | ((kind == KIND_M) & (P == i))
                ok &= (P != 10) & ((kind == KIND_T) | (P != 11))
            for rows in (rA, rB):
                ok &= ~(own[rows] & (S[rows, L] <= best))
            for j in np.flatnonzero(ok & (best <= max_half)):
                out.append((int(best[j]), int(o[j]), strand, kind, int(P[j])))
    return out


def all_sites_numpy(mirnas, names, seqs, cleavage, max_half=16, only=None):
    """-> the tuples `emit` takes, for every site with half <= max_half on both strands"""
    sites = []
    for m, (mname, mc) in enumerate(mirnas):
        if only is not None and m not in only:
            continue
        for tid, t in enumerate(seqs):
            for half, o, strand, kind, P in sites_bulge_numpy(mc, t, cleavage, max_half):
                cols = columns(mc, t, o, strand, kind, P)
                sites.append((m, half, tid, o, strand, kind, bulge_line(mname, names[tid], o, len(mc), strand, half, mc, kind, P, cols)))
    return sites


def restate_bulge_numpy(mirnas, names, seqs, max_half=8, both=False, cleavage=False, k=0):
    return emit(all_sites_numpy(mirnas, names, seqs, cleavage, max_half), max_half, both, k)


# ---------------------------------------------------------------------------------------------------- generators (also used on the GPU)
def bulged_site(mirna, strand, kind, P, extra=b"A"):
    """The forward target text of the miRNA's perfect site with one base inserted after the partner of position P (t) or the partner of position P
    deleted (m)."""
    perfect = target_of_mirna(mirna, 1)                                   # minus-strand text: column i is the partner of position i
    s = perfect[:P] + extra + perfect[P:] if kind == KIND_T else perfect[:P - 1] + perfect[P:]
    if strand:
        return s
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    return s.translate(comp)[::-1]


def plant_bulged(rng, text, mirna, n, subs=(0, 1), both=True):
    """Writes n bulged sites of the miRNA (kind, P and strand random, up to subs[1] substitutions) into the bytearray text -> [(offset, strand, kind, P)]"""
    clean = bytes(c for c in mirna if c in b"ACGUTacgut").upper()
    out = []
    if len(clean) != len(mirna):
        return out
    for _ in range(n):
        strand = int(rng.randint(0, 2)) if both else 0
        kind = KIND_T if rng.randint(0, 2) else KIND_M
        P = int(rng.randint(1 if kind == KIND_T else 2, len(clean)))
        site = bytearray(bulged_site(clean, strand, kind, P, b"ACGT"[rng.randint(0, 4):][:1]))
        for _ in range(int(rng.randint(subs[0], subs[1] + 1))):
            site[int(rng.randint(0, len(site)))] = b"ACGT"[rng.randint(0, 4)]
        o = int(rng.randint(0, len(text) - len(site)))
        text[o:o + len(site)] = site
        out.append((o, strand, kind, P))
    return out


# ---------------------------------------------------------------------------------------------------- hand-made cases
def _rows(mirna, target, **kw):
    """one miRNA against one target text under all three restatements -> the rows split at tabs"""
    mirnas = parse_mirnas(b">m\n" + mirna + b"\n")
    codes = CODE[np.frombuffer(target, dtype=np.uint8)]
    got = restate_bulge(mirnas, ["t"], [codes], **kw)
    assert got == restate_bulge(mirnas, ["t"], [codes], site=bulge_site_dp, **kw)
    assert got == restate_bulge_numpy(mirnas, ["t"], [codes], **kw)
    assert got.startswith(BHEADER)
    return [ln.split(b"\t") for ln in got.split(b"\n")[1:-1]]


def _other(base, avoid):
    return next(bytes([c]) for c in b"ACGT" if bytes([c]) not in avoid)


MIX = b"UCGAUGCAGUCAUGCUAGCAU"                   # 21 nt, no two equal neighbours: every placement of a bulge is distinct


def test_mix_has_no_equal_neighbours():
    assert len(MIX) == 21 and all(a != b for a, b in zip(MIX, MIX[1:]))


@pytest.mark.parametrize("strand", [0, 1])
def test_inserted_target_base_at_every_p(strand):
    L = len(MIX)
    perfect = target_of_mirna(MIX, 1)
    want3 = bytes(b"ACGU"[3 - b"ACGU".index(c)] for c in MIX)
    for P in range(1, L):
        extra = _other(None, (perfect[P - 1:P], perfect[P:P + 1]))       # differs from both neighbours: the placement is unique
        site = bulged_site(MIX, strand, KIND_T, P, extra)
        rows = _rows(MIX, b"CC" + site + b"CC", max_half=4, both=True)
        if P in (1, L - 1):
            # a gap next to a terminal position costs 1.0, and the ungapped alignment that pairs that position instead costs at most 1.0
            assert [r[11] for r in rows] == [b"."] and float(rows[0][5]) <= 1.0
            continue
        gap = b"2.0" if 2 <= P <= 12 else b"1.0"
        rows = [r for r in rows if r[11].startswith(b"t")]
        assert [r[:8] + [r[11]] for r in rows] == [[b"m", b"t", b"3", b"%d" % (2 + L + 1), b"-" if strand else b"+", gap, b"0", b"0", b"t%d" % P]]
        r = rows[0]
        assert r[8] == MIX[:P] + b"-" + MIX[P:] and r[9] == b"|" * P + b"-" + b"|" * (L - P)
        unpaired = bytes([b"UGCA"[b"ACGT".index(extra)]])                 # on the target strand, on either strand of the text
        assert r[10] == want3[:P] + unpaired + want3[P:]


@pytest.mark.parametrize("strand", [0, 1])
def test_deleted_target_base_at_every_p(strand):
    L = len(MIX)
    for P in range(2, L):
        site = bulged_site(MIX, strand, KIND_M, P)
        rows = [r for r in _rows(MIX, b"CC" + site + b"CC", max_half=4, both=True) if r[11].startswith(b"m")]
        gap = b"2.0" if P <= 13 else b"1.0"
        assert [r[:8] + [r[11]] for r in rows] == [[b"m", b"t", b"3", b"%d" % (2 + L - 1), b"-" if strand else b"+", gap, b"0", b"0", b"m%d" % P]]
        want3 = bytes(b"ACGU"[3 - b"ACGU".index(c)] for c in MIX)
        r = rows[0]
        assert r[8] == MIX and r[9] == b"|" * (P - 1) + b"-" + b"|" * (L - P) and r[10] == want3[:P - 1] + b"-" + want3[P:]


def test_gap_cost_doubles_inside_2_to_13():
    assert [gap_cost(KIND_T, P) for P in (1, 2, 12, 13, 14)] == [2, 4, 4, 2, 2]
    assert [gap_cost(KIND_M, P) for P in (2, 12, 13, 14)] == [4, 4, 4, 2]
    perfect = target_of_mirna(MIX, 1)
    # t1 costs 1.0 and is never written: the ungapped alignment that pairs position 1 with the unpaired base costs at most 1.0 (see above)
    for P, t_score, m_score in ((2, b"2.0", b"2.0"), (12, b"2.0", b"2.0"), (13, b"1.0", b"2.0"), (14, b"1.0", b"1.0")):
        extra = _other(None, (perfect[P - 1:P], perfect[P:P + 1]))
        rows = _rows(MIX, b"GG" + bulged_site(MIX, 1, KIND_T, P, extra) + b"GG", max_half=4, both=True)
        assert [(r[5], r[11]) for r in rows if r[11].startswith(b"t")] == [(t_score, b"t%d" % P)]
        rows = _rows(MIX, b"GG" + bulged_site(MIX, 1, KIND_M, P) + b"GG", max_half=4, both=True)
        assert [(r[5], r[11]) for r in rows if r[11].startswith(b"m")] == [(m_score, b"m%d" % P)]
    # the gap of t1 from the score of a site that no ungapped alignment reaches: L = 12 would be dominated too, so through the scorer
    mc = MCODE[np.frombuffer(MIX, dtype=np.uint8)]
    t = CODE[np.frombuffer(bulged_site(MIX, 1, KIND_T, 1, b"A"), dtype=np.uint8)]
    assert score_columns(mc, columns(mc, t, 0, 1, KIND_T, 1), KIND_T, 1)[0] == 2 and score_columns(mc, columns(mc, t, 0, 1, KIND_T, 2), KIND_T, 2)[0] > 4


def test_tie_takes_the_smallest_p():
    mir = b"UCGAUGCAGUCAUGCAAAAGU"               # positions 16..19 are A: deleting any one of their partners is the same text
    assert mir[15:19] == b"AAAA" and mir[14:15] != b"A" and mir[19:20] != b"A"
    rows = _rows(mir, b"CC" + bulged_site(mir, 1, KIND_M, 18) + b"CC", max_half=2, both=True)
    assert [(r[5], r[11]) for r in rows if r[11] != b"."] == [(b"1.0", b"m16")]
    # an inserted T next to the partners of 16..19: after 15, 16, 17, 18 or 19
    rows = _rows(mir, b"CC" + bulged_site(mir, 1, KIND_T, 17, b"A") + b"CC", max_half=2, both=True)
    assert [(r[5], r[11]) for r in rows if r[11] != b"."] == [(b"1.0", b"t15")]


def test_cleavage_rejects_t10_m10_m11_and_a_mismatch_at_10_or_11():
    perfect = target_of_mirna(MIX, 1)
    for kind, P in ((KIND_T, 10), (KIND_M, 10), (KIND_M, 11)):
        extra = _other(None, (perfect[P - 1:P], perfect[P:P + 1]))
        text = b"GG" + bulged_site(MIX, 1, kind, P, extra) + b"GG"
        tag = b"%s%d" % (b"t" if kind == KIND_T else b"m", P)
        assert tag in [r[11] for r in _rows(MIX, text, max_half=4, both=True)]
        assert all(r[11] == b"." for r in _rows(MIX, text, max_half=4, both=True, cleavage=True))
    for kind, P in ((KIND_T, 9), (KIND_T, 11), (KIND_M, 9), (KIND_M, 12)):
        extra = _other(None, (perfect[P - 1:P], perfect[P:P + 1]))
        text = b"GG" + bulged_site(MIX, 1, kind, P, extra) + b"GG"
        assert b"%s%d" % (b"t" if kind == KIND_T else b"m", P) in [r[11] for r in _rows(MIX, text, max_half=4, both=True, cleavage=True)]
    # a t3 site with a mismatch at position 11 (miRNA C at 11: target C instead of G): kept without -c, rejected with it; a G:U there stays
    assert MIX[10:11] == b"C" and MIX[9:10] == b"U"
    site = bytearray(bulged_site(MIX, 1, KIND_T, 3, b"C"))
    site[11] = ord("A")                           # minus strand: column 12 of the text is the partner of position 11 (one inserted base before)
    rows = _rows(MIX, b"GG" + bytes(site) + b"GG", max_half=8, both=True)
    assert (b"4.0", b"1", b"t3") in [(r[5], r[6], r[11]) for r in rows]
    assert all(r[11] == b"." for r in _rows(MIX, b"GG" + bytes(site) + b"GG", max_half=8, both=True, cleavage=True))
    site = bytearray(bulged_site(MIX, 1, KIND_T, 3, b"C"))
    site[10] = ord("C")                           # position 10 is U, target strand G: a G:U
    rows = _rows(MIX, b"GG" + bytes(site) + b"GG", max_half=8, both=True, cleavage=True)
    assert (b"3.0", b"1", b"t3") in [(r[5], r[7], r[11]) for r in rows]


def test_an_unpaired_n_blocks_the_site():
    perfect = target_of_mirna(MIX, 1)
    P = 5
    extra = _other(None, (perfect[P - 1:P], perfect[P:P + 1]))
    for strand in (0, 1):
        site = bytearray(bulged_site(MIX, strand, KIND_T, P, extra))
        assert [r[11] for r in _rows(MIX, b"GG" + bytes(site) + b"GG", max_half=4, both=True)] == [b"t5"]
        at = P if strand else len(site) - 1 - P                        # the unpaired base
        site[at] = ord("N")
        rows = _rows(MIX, b"GG" + bytes(site) + b"GG", max_half=16, both=True)
        assert all(not int(r[2]) <= 3 + at <= int(r[3]) for r in rows)
        assert [r for r in rows if float(r[5]) <= 2.0] == []


def test_contig_edges():
    perfect = target_of_mirna(MIX, 1)
    for kind, P in ((KIND_T, 6), (KIND_M, 6), (KIND_T, 2), (KIND_M, 20), (KIND_T, 19), (KIND_M, 2)):
        extra = _other(None, (perfect[P - 1:P], perfect[P:P + 1]))
        for strand in (0, 1):
            site = bulged_site(MIX, strand, kind, P, extra)
            tag = b"%s%d" % (b"t" if kind == KIND_T else b"m", P)
            rows = [r for r in _rows(MIX, site, max_half=4, both=True) if r[5] in (b"1.0", b"2.0") and r[11] == tag]
            assert [(r[2], r[3], r[4]) for r in rows] == [(b"1", b"%d" % len(site), b"-" if strand else b"+")], (kind, P, strand)
            # one base short at either end: the interval leaves the contig
            for cut in (site[1:], site[:-1]):
                assert [r for r in _rows(MIX, cut, max_half=4, both=True) if r[11] == tag and r[5] in (b"1.0", b"2.0")] == []


def test_two_contigs_do_not_share_a_site():
    site = bulged_site(MIX, 1, KIND_T, 7, b"C")
    mirnas = parse_mirnas(b">m\n" + MIX + b"\n")
    seqs = [CODE[np.frombuffer(site[:9], dtype=np.uint8)], CODE[np.frombuffer(site[9:], dtype=np.uint8)], CODE[np.frombuffer(site, dtype=np.uint8)]]
    for f in (restate_bulge, restate_bulge_numpy):
        got = f(mirnas, ["a", "b", "c"], seqs, max_half=4, both=True)
        assert [ln.split(b"\t")[1] for ln in got.split(b"\n")[1:-1]] == [b"c"]


def test_domination_equal_is_dropped_better_by_half_is_kept():
    # an ungapped site with a mismatch at position 21 (1.0) against m20 (gap 1.0): equal, so only the ungapped site is written
    perfect = target_of_mirna(MIX, 1)
    rows = _rows(MIX, b"GG" + perfect[:20] + b"GG", max_half=2, both=True)
    assert [(r[5], r[11]) for r in rows] == [(b"1.0", b".")]
    # t14 (1.0) on the minus strand at start 3.  A = U(start 3) pairs 1..14 as the site does, position 15 with the inserted base (a mismatch,
    # 1.0) and 16..21 one base early.  With C at 15..21 those all pair: A = 1.0 = t14, dropped.
    equal = b"UCGAUGCAGUCAUGCCCCCCC"
    text = target_of_mirna(equal, 1)
    rows = _rows(equal, b"AA" + text[:14] + b"A" + text[14:] + b"AA", max_half=4, both=True)
    assert [(r[5], r[11]) for r in rows if r[4] == b"-" and r[2] == b"3"] == [(b"1.0", b".")]
    # with U at 21 position 21 of A meets the partner of position 20 (C, a G:U, 0.5): A = 1.5, t14 = 1.0 is better by 0.5 and kept
    better = b"UCGAUGCAGUCAUGCCCCCCU"
    text = target_of_mirna(better, 1)
    rows = _rows(better, b"AA" + text[:14] + b"A" + text[14:] + b"AA", max_half=4, both=True)
    assert [(r[3], r[5], r[11]) for r in rows if r[4] == b"-" and r[2] == b"3"] == [(b"24", b"1.0", b"t14"), (b"23", b"1.5", b".")]


@pytest.mark.parametrize("seed", [1, 2])
def test_the_three_restatements_agree(seed):
    rng = np.random.RandomState(seed)
    mirs = random_mirnas(rng, 4, lower=0.2) + random_mirnas(rng, 1, unknown=0.1)
    text = bytearray(ACGT[rng.randint(0, 4, 700)].tobytes())
    for m in mirs:
        plant(rng, text, m, 2)
        plant_bulged(rng, text, m, 4)
    text[100:104] = b"NNNN"
    text[333] = ord("R")
    seqs = [CODE[np.frombuffer(bytes(text[:400]), dtype=np.uint8)], CODE[np.frombuffer(bytes(text[400:]), dtype=np.uint8)]]
    mirnas = parse_mirnas(b"".join(b">m%d x\n%s\n" % (i, m) for i, m in enumerate(mirs)))
    seen = set()
    for kw in (dict(max_half=8, both=True), dict(max_half=11, both=True, cleavage=True), dict(max_half=16, k=3)):
        want = restate_bulge(mirnas, ["a", "b"], seqs, **kw)
        assert restate_bulge(mirnas, ["a", "b"], seqs, site=bulge_site_dp, **kw) == want
        assert restate_bulge_numpy(mirnas, ["a", "b"], seqs, **kw) == want
        seen |= {ln.split(b"\t")[11][:1] for ln in want.split(b"\n")[1:-1]}
        # the ungapped lines, minus the last column, are the file without --bulge
        if kw.get("k", 0) == 0:
            dots = [ln[:-2] for ln in want.split(b"\n")[1:-1] if ln.endswith(b"\t.")]
            assert dots == restate_numpy(mirnas, ["a", "b"], seqs, **kw).split(b"\n")[1:-1]
    assert seen == {b".", b"t", b"m"}


def test_option_errors_exit_2_before_a_device(tmp_path):
    m, t = tmp_path / "m.fa", tmp_path / "t.fa"
    m.write_bytes(b">m\n" + MIR + b"\n")
    t.write_bytes(b">t\nACGT\n")
    for args in (["-g"], ["-g", str(m)], ["--bulge=1", str(m), str(t)], ["-g", "-s", "9", str(m), str(t)], ["--bulge", "-k", "-1", str(m), str(t)],
                 ["-g", "--device", "-1", str(m), str(t)], ["--bulges", str(m), str(t)], ["-g", "-o", "", str(m), str(t)]):
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_parse_args_and_help(capsys):
    from mir_prefer_amd import targets
    assert targets.parse_args(["-g", "m.fa", "a.fa"])[0].bulge is True
    assert targets.parse_args(["--bulge", "-b", "m.fa", "a.fa"])[0].bulge is True
    assert not targets.parse_args(["m.fa", "a.fa"])[0].bulge
    with pytest.raises(SystemExit):
        targets.parse_args(["-h"])
    assert "--bulge" in capsys.readouterr().out
