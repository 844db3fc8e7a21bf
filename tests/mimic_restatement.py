"""CPU restatements of the target-mimic search (python -m mir_prefer_amd.mimics).  TEST INFRASTRUCTURE ONLY: the yardstick of
tests/test_mimics_cpu.py and tests/test_mimics_gpu.py.  Two independent restatements of the definition, each producing the TSV bytes: a plain-Python
enumeration over (miRNA, o, strand, P) straight from the rules, and a numpy version over all offsets of a contig at once, which the GPU tests
compare whole files with.  Also the generators: the perfect mimic text of a miRNA for (strand, P, G, loop bases) and planting with substitutions."""
import numpy as np

from tests.test_targets_cpu import ACGT, CLS, CODE, MCODE, PAIR, RNA, load_reference, parse_mirnas, target_of_mirna

HEADER = b"miRNA\ttarget\tstart\tend\tstrand\timperfect\tmismatches\tgu\tmirna_5to3\tpairs\ttarget_3to5\tloop\n"
LOOPS = (9, 10, 11)


def partner(L, G, o, strand, P, i):
    """Index on the forward target of the base paired with miRNA position i in the site (o, strand, P) with loop length G: the table of §27."""
    if strand == 0:
        return o + G + L - i if i <= P else o + L - i
    return o + i - 1 if i <= P else o + G + i - 1


def unpaired(L, G, o, strand, P):
    """Indices of the loop bases, in the order of the alignment's columns (5'->3' on the miRNA)."""
    if strand == 0:
        return [o + L - P + G - 1 - g for g in range(G)]
    return [o + P + g for g in range(G)]


def columns(mc, t, o, strand, P, G):
    """The aligned columns of a site: [(miRNA position or 0, target-strand base)], 5'->3' on the miRNA."""
    L = len(mc)

    def y(q):
        return 3 - int(t[q]) if strand else int(t[q])
    cols = [(i, y(partner(L, G, o, strand, P, i))) for i in range(1, P + 1)]
    cols += [(0, y(q)) for q in unpaired(L, G, o, strand, P)]
    cols += [(i, y(partner(L, G, o, strand, P, i))) for i in range(P + 1, L + 1)]
    return cols


def mimic_line(mname, tname, o, strand, imperfect, mc, P, cols):
    cls = [int(CLS[mc[i - 1], y]) if i else 3 for i, y in cols]
    return b"%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\n" % (
        mname, tname.encode(), o + 1, o + len(cols), b"-" if strand else b"+", imperfect, cls.count(2), cls.count(1),
        bytes(RNA[mc[i - 1]] if i else ord("-") for i, _ in cols), bytes((PAIR + b"-")[k] for k in cls), bytes(RNA[y] for _, y in cols), P)


# ---------------------------------------------------------------------------------------------------- 1: the plain enumeration
def site_plain(mc, t, o, strand, G):
    """The mimic site of one (miRNA, interval start, strand) before rule 4 -> (imperfect, P) or None."""
    L = len(mc)
    if o < 0 or o + L + G > len(t) or any(int(x) > 3 for x in t[o:o + L + G]):
        return None
    best = None
    for P in LOOPS:
        if P >= L:                                                        # rule 1
            continue
        cls = [None]
        for i in range(1, L + 1):
            x = int(t[partner(L, G, o, strand, P, i)])
            cls.append(int(CLS[mc[i - 1], 3 - x if strand else x]))
        if any(cls[i] != 0 for i in range(2, 9)):                          # rule 2
            continue
        if cls[P] == 2 or cls[P + 1] == 2:                                 # rule 3
            continue
        imperfect = sum(1 for k in cls[1:] if k != 0)
        if best is None or imperfect < best[0]:                            # rule 5: the smallest P on a tie
            best = (imperfect, P)
    return best


def sites_plain(mc, t, G):
    """-> [(imperfect, o, strand, P)] of one miRNA on one contig, both strands, every imperfect"""
    out = []
    for o in range(len(t)):
        for strand in (0, 1):
            r = site_plain(mc, t, o, strand, G)
            if r is not None:
                out.append((r[0], o, strand, r[1]))
    return out


# ---------------------------------------------------------------------------------------------------- 2: numpy, all offsets at once
def sites_numpy(mc, t, G):
    """The same list from the windows of L + G bases of the contig, every offset at once.  Column c (1-based) of a window read on the target
    strand 3'->5' is paired with position c (c <= P) or c - G (c > P + G)."""
    L = len(mc)
    n = L + G
    if len(t) < n:
        return []
    W = np.lib.stride_tricks.sliding_window_view(np.asarray(t), n)
    ok = ~(W > 3).any(axis=1)
    Wc = np.minimum(W, 3).astype(np.int64)
    out = []
    for strand in (0, 1):
        Y = (3 - Wc) if strand else Wc[:, ::-1]
        imp = np.full((len(W), len(LOOPS)), 99, dtype=np.int64)
        for a, P in enumerate(LOOPS):
            if P >= L:
                continue
            idx = list(range(P)) + list(range(P + G, n))
            C = CLS[np.asarray(mc)[None, :], Y[:, idx]]
            good = ok & (C[:, 1:8] == 0).all(axis=1) & (C[:, P - 1] != 2) & (C[:, P] != 2)
            imp[good, a] = (C[good] != 0).sum(axis=1)
        a = imp.argmin(axis=1)                                             # the first minimum: the smallest P
        best = imp[np.arange(len(W)), a]
        for o in np.flatnonzero(best < 99):
            out.append((int(best[o]), int(o), strand, LOOPS[int(a[o])]))
    return out


# ---------------------------------------------------------------------------------------------------- the file
def all_sites(mirnas, names, seqs, G, sites=sites_numpy, only=None):
    """-> (m, imperfect, tid, o, strand, line) for every site on both strands"""
    out = []
    for m, (mname, mc) in enumerate(mirnas):
        if only is not None and m not in only:
            continue
        for tid, t in enumerate(seqs):
            for imperfect, o, strand, P in sites(mc, t, G):
                out.append((m, imperfect, tid, o, strand, mimic_line(mname, names[tid], o, strand, imperfect, mc, P, columns(mc, t, o, strand, P, G))))
    return out


def emit(sites, n=3, both=False, k=0):
    """The TSV bytes: rule 4, the strands scanned, the order miRNA, imperfect, target, start, + before -, and -k."""
    out, per = [HEADER], {}
    for s in sorted((x for x in sites if x[1] <= n and (both or x[4] == 0)), key=lambda x: x[:5]):
        per[s[0]] = per.get(s[0], 0) + 1
        if k == 0 or per[s[0]] <= k:
            out.append(s[5])
    return b"".join(out)


def restate(mirnas, names, seqs, n=3, G=3, both=False, k=0, plain=False):
    return emit(all_sites(mirnas, names, seqs, G, sites_plain if plain else sites_numpy), n, both, k)


def restate_files(mirna_path, target_paths, **kw):
    mirnas = parse_mirnas(open(mirna_path, "rb").read())
    names, seqs = load_reference(target_paths)
    return restate(mirnas, names, seqs, **kw)


def seed_stats(mirnas, seqs, both):
    """-> (miRNAs without a usable seed, seeds looked up, bucket entries evaluated) as §27 counts them"""
    keys = {}
    no_seed = 0
    for _, mc in mirnas:
        if (np.asarray(mc[1:8]) > 3).any():
            no_seed += 1
        else:
            key = tuple(int(x) for x in mc[1:8])
            keys[key] = keys.get(key, 0) + 1
    seeds = entries = 0
    for t in seqs:
        for q in range(len(t) - 6):
            w = t[q:q + 7]
            if (w > 3).any():
                continue
            seeds += 2 if both else 1
            entries += keys.get(tuple(int(3 - x) for x in w[::-1]), 0)     # plus: the reverse complement pairs with positions 2..8
            if both:
                entries += keys.get(tuple(int(x) for x in w), 0)
    return no_seed, seeds, entries


# ---------------------------------------------------------------------------------------------------- generators
def clean_mirna(mirna):
    """The miRNA's letters as upper-case A C G U, or None with any other letter."""
    s = mirna.upper().replace(b"T", b"U")
    return s if all(c in b"ACGU" for c in s) else None


def mimic_text(mirna, strand, P, loop):
    """The forward target text of the miRNA's perfect mimic site: its perfect site with the forward bases `loop` between the partners of
    positions P and P + 1."""
    L = len(mirna)
    site = target_of_mirna(mirna, strand)
    at = P if strand else L - P
    return site[:at] + loop + site[at:]


def plant_mimic(rng, text, mirna, strand, P, G, subs=(0, 0), at=None):
    """Writes one mimic site of the miRNA into the bytearray text (random loop bases, up to subs[1] substitutions outside the seed's partners)
    -> its offset, or None for a miRNA with an unknown letter."""
    clean = clean_mirna(mirna)
    if clean is None:
        return None
    L = len(clean)
    site = bytearray(mimic_text(clean, strand, P, ACGT[rng.randint(0, 4, G)].tobytes()))
    seed = {partner(L, G, 0, strand, P, i) for i in range(2, 9)}
    for _ in range(int(rng.randint(subs[0], subs[1] + 1))):
        j = int(rng.randint(0, len(site)))
        if j not in seed:
            site[j] = b"ACGT"[rng.randint(0, 4)]
    o = int(rng.randint(0, len(text) - len(site))) if at is None else at
    text[o:o + len(site)] = site
    return o


def loops_seen(data):
    """-> {(strand, P)} over the lines of a TSV"""
    return {(f[4], int(f[11])) for f in (ln.split(b"\t") for ln in data.split(b"\n")[1:-1])}


__all__ = ["ACGT", "CODE", "MCODE", "HEADER", "LOOPS", "all_sites", "clean_mirna", "columns", "emit", "loops_seen", "mimic_line", "mimic_text", "partner",
           "plant_mimic", "restate", "restate_files", "seed_stats", "site_plain", "sites_numpy", "sites_plain", "unpaired"]
