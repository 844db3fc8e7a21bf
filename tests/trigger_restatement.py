"""The tests' two restatements of the miRNA triggers of PHAS loci (mir_prefer_amd.triggers).  Both produce the bytes of
<base>.triggers.tsv and <base>.triggers.summary.tsv from (records, contigs, miRNAs, loci, options):

  restate_plain   the definition word by word: a dict of units, the per-site scorer of tests/test_targets_cpu.py at every offset of every locus
                  interval, every window coordinate looked up one by one, p-values as Fractions of math.comb sums.
  restate_numpy   brute-force scoring of every offset of an interval at once (sites_numpy), the windows of all sites by searchsorted over the
                  sorted unit keys with cumulative sums, the test through phasing.Hypergeom's kmin table.

Inputs: alns = ALN_DTYPE records; names[tid], seqs[tid] = the contigs (bytes; the genome's contigs are the SAM's, in tid order); mirnas =
test_targets_cpu.parse_mirnas's [(name, codes)]; rows = [(contig name, start, end, best_start)], the loci of the phas.tsv in file order."""
import math
from fractions import Fraction

import numpy as np

from mir_prefer_amd import phasing
from tests.test_align_cpu import CODE
from tests.test_targets_cpu import PAIR, RNA, score_site, sites_numpy

HEADER = (b"locus\tmiRNA\tcontig\tstart\tend\tstrand\tscore\tmismatches\tgu\tmirna_len\tcut\tside\toffset\tn\tk\tpvalue\tphased_reads\twindow_reads\t"
          b"locus_register\tmirna_5to3\tpairs\ttarget_3to5\n")
SUMMARY_HEADER = b"locus\tsites\ttrigger_lines\tbest_miRNA\tbest_side\tbest_offset\tbest_pvalue\n"
SIDES = (b"down", b"up")


def codes_of(seq):
    return CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


def interval(row, ln, flank):
    """The locus interval I_q, 1-based and closed."""
    return max(1, row[1] - flank), min(ln, row[2] + flank)


def cut_and_register(o, L, strand, Lp):
    """cut and the register r of the first siRNA 3' of it, for the site at the 0-based offset o."""
    if strand == 0:
        cut = o + L - 9
        return cut, cut
    cut = o + 10
    return cut, cut - Lp + 3


def window_start(r, strand, side, delta, m, Lp):
    if strand == 0:
        return r + delta if side == 0 else r - m * Lp + delta
    return r - (m - 1) * Lp + delta if side == 0 else r + Lp + delta


def p_direct(n, k, m, Lp):
    S, G = 2 * m * Lp, 2 * m
    return Fraction(sum(math.comb(G, j) * math.comb(S - G, n - j) for j in range(max(k, 0), min(n, G) + 1)), math.comb(S, n))


def _emit(rows, mirnas, site_counts, trig, Lp):
    """trig: (q, m, half, o, strand, side, delta, n, k, p, phased, reads, classes, target-strand bases), in any order."""
    trig = sorted(trig, key=lambda t: t[:7])
    out, lines, best = [HEADER], [0] * len(rows), [None] * len(rows)
    for q, m, half, o, strand, side, delta, n, k, p, ph, rd, cls, ys in trig:
        name, start, end, best_start = rows[q]
        mname, mc = mirnas[m]
        L = len(mc)
        cut, r = cut_and_register(o, L, strand, Lp)
        cls = np.asarray(cls)
        f = [b"%s:%d-%d" % (name.encode(), start, end), mname, name.encode(), b"%d" % (o + 1), b"%d" % (o + L), b"-" if strand else b"+",
             b"%d.%d" % (half // 2, 5 * (half & 1)), b"%d" % int((cls == 2).sum()), b"%d" % int((cls == 1).sum()), b"%d" % L, b"%d" % cut, SIDES[side],
             b"%d" % delta, b"%d" % n, b"%d" % k, b"%.3e" % float(p), b"%d" % ph, b"%d" % rd, b"1" if (r + delta - best_start) % Lp == 0 else b"0",
             bytes(RNA[c] for c in mc), bytes(PAIR[c] for c in cls), bytes(RNA[y] for y in ys)]
        out.append(b"\t".join(f) + b"\n")
        lines[q] += 1
        if best[q] is None or (p, half) < best[q][:2]:
            best[q] = (p, half, mname, side, delta)
    summ = [SUMMARY_HEADER]
    for q, (name, start, end, _) in enumerate(rows):
        b = best[q]
        tail = b".\t.\t.\t." if b is None else b"%s\t%s\t%d\t%.3e" % (b[2], SIDES[b[3]], b[4], float(b[0]))
        summ.append(b"%s:%d-%d\t%d\t%d\t%s\n" % (name.encode(), start, end, site_counts[q], lines[q], tail))
    return b"".join(out), b"".join(summ)


def restate_plain(alns, names, seqs, mirnas, rows, Lp=21, m=10, alpha=Fraction(1, 1000), K=3, D=1, max_half=8, flank=100, drift=0):
    units = {}
    for r in alns.tolist():
        tid, pos, depth, ln, strand = r[0], r[1], r[2], r[3], r[4]
        if ln == Lp:
            u = (tid, strand, pos + 2 if strand else pos)
            units[u] = units.get(u, 0) + depth
    units = {u: a for u, a in units.items() if a >= D}
    codes = [codes_of(s) for s in seqs]
    trig, site_counts = [], []
    for q, row in enumerate(rows):
        tid = names.index(row[0])
        a, b = interval(row, len(seqs[tid]), flank)
        t = codes[tid]
        nsites = 0
        for mi, (_, mc) in enumerate(mirnas):
            L = len(mc)
            for o in range(a - 1, b - L + 1):                       # [o + 1, o + L] inside [a, b]
                for strand in (0, 1):
                    sc = score_site(mc, t, o, strand, True)
                    if sc is None or sc[0] > max_half:
                        continue
                    nsites += 1
                    _, r = cut_and_register(o, L, strand, Lp)
                    for side in (0, 1):
                        for delta in range(-drift, drift + 1):
                            x = window_start(r, strand, side, delta, m, Lp)
                            n = k = ph = rd = 0
                            for s in (0, 1):
                                for c in range(x, x + m * Lp):
                                    ab = units.get((tid, s, c))
                                    if ab is not None:
                                        n += 1
                                        rd += ab
                                        if (c - x) % Lp == 0:
                                            k += 1
                                            ph += ab
                            p = p_direct(n, k, m, Lp)
                            if k >= K and p <= alpha:
                                trig.append((q, mi, sc[0], o, strand, side, delta, n, k, p, ph, rd, sc[1], sc[2]))
        site_counts.append(nsites)
    return _emit(rows, mirnas, site_counts, trig, Lp)


def _streams(alns, Lp, D):
    """Per strand: the sorted unit keys tid << 32 | c, their abundances and the abundances' cumulative sums."""
    a = alns[(alns["len"] == Lp) & (alns["pos"] >= 0)]
    out = []
    for s in (0, 1):
        r = a[a["strand"] == s]
        key = (r["tid"].astype(np.int64) << 32) + r["pos"].astype(np.int64) + 2 * s
        ukey, inv = np.unique(key, return_inverse=True)
        ab = np.zeros(len(ukey), np.int64)
        np.add.at(ab, inv, r["depth"].astype(np.int64))
        keep = ab >= D
        ukey, ab = ukey[keep], ab[keep]
        out.append((ukey, ab, np.concatenate([[0], np.cumsum(ab)]).astype(np.int64)))
    return out


def restate_numpy(alns, names, seqs, mirnas, rows, Lp=21, m=10, alpha=Fraction(1, 1000), K=3, D=1, max_half=8, flank=100, drift=0):
    hg = phasing.Hypergeom(m, Lp)
    kmin = np.asarray(hg.kmin(alpha), np.int64)
    codes = [codes_of(s) for s in seqs]
    sites, site_counts = [], []                                    # (q, m, half, o, strand, tid, r, classes, bases)
    for q, row in enumerate(rows):
        tid = names.index(row[0])
        a, b = interval(row, len(seqs[tid]), flank)
        before = len(sites)
        for mi, (_, mc) in enumerate(mirnas):
            for half, o, strand, C, Y in sites_numpy(mc, codes[tid][a - 1:b], max_half, True, True):
                o += a - 1
                sites.append((q, mi, half, o, strand, tid, cut_and_register(o, len(mc), strand, Lp)[1], C, Y))
        site_counts.append(len(sites) - before)
    if not sites:
        return _emit(rows, mirnas, site_counts, [], Lp)
    # every (site, side, delta) as one row of the arrays
    idx, sd, dl, xs = [], [], [], []
    for i, s in enumerate(sites):
        for side in (0, 1):
            for delta in range(-drift, drift + 1):
                idx.append(i)
                sd.append(side)
                dl.append(delta)
                xs.append(window_start(s[6], s[4], side, delta, m, Lp))
    x = np.asarray(xs, np.int64)
    tb = np.asarray([sites[i][5] for i in idx], np.int64) << 32
    n = np.zeros(len(x), np.int64)
    k = np.zeros(len(x), np.int64)
    ph = np.zeros(len(x), np.int64)
    rd = np.zeros(len(x), np.int64)
    for ukey, ab, P in _streams(alns, Lp, D):
        lo = np.searchsorted(ukey, tb + np.maximum(x, 0))         # a register below 0 holds no unit and must not reach into the contig before
        hi = np.searchsorted(ukey, tb + np.maximum(x + m * Lp, 0))
        n += hi - lo
        rd += P[hi] - P[lo]
        if len(ukey):
            for j in range(m):
                c = x + j * Lp
                i = np.searchsorted(ukey, tb + np.maximum(c, 0))
                ic = np.minimum(i, len(ukey) - 1)
                hit = (c >= 0) & (i < len(ukey)) & (ukey[ic] == tb + c)
                k += hit
                ph += np.where(hit, ab[ic], 0)
    ok = k >= np.maximum(kmin[n], K)
    trig = []
    for w in np.flatnonzero(ok).tolist():
        s = sites[idx[w]]
        trig.append((s[0], s[1], s[2], s[3], s[4], sd[w], dl[w], int(n[w]), int(k[w]), hg.p(int(n[w]), int(k[w])), int(ph[w]), int(rd[w]), s[7], s[8]))
    return _emit(rows, mirnas, site_counts, trig, Lp)
