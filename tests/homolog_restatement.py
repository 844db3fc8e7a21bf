"""CPU restatement of the homolog search. TEST INFRASTRUCTURE ONLY: the yardstick of tests/test_homologs_gpu.py, built from code
that is already pinned on the real reference -- a brute-force numpy Hamming scan over both strands, then tests.oracle_binding: lfold(window, span)
-> structures_from_lines -> maturestar per structure, then the selection and merge rules of §26."""
import functools
import random

import numpy as np

from mir_prefer_amd import homologs

COMP = str.maketrans("ACGTN", "TGCAN")
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def revcomp(s):
    return s.translate(COMP)[::-1]


def clean(seq):
    """A contig as the windows show it: upper case, every letter other than A C G T as N."""
    return "".join(ch if ch in "ACGT" else "N" for ch in seq.upper())


def placements(queries, contigs, v, max_placements):
    """[(query, contig, 0-based offset, strand, mismatches)] in (query, contig, offset, + before -) order, and the number of queries dropped for
    more than max_placements placements.  queries: [sequence of A C G T]; contigs: [(name, letters)]."""
    coded = [_CODE[np.frombuffer(s.encode("latin-1"), dtype=np.uint8)] for _, s in contigs]
    out, dropped = [], 0
    for q, seq in enumerate(queries):
        L = len(seq)
        fwd = _CODE[np.frombuffer(seq.encode(), dtype=np.uint8)]
        rev = (3 - fwd)[::-1]
        mine = []
        for ci, g in enumerate(coded):
            n = len(g) - L + 1
            if n <= 0:
                continue
            amb = np.concatenate(([0], np.cumsum(g > 3)))
            ok = (amb[L:] - amb[:-L]) == 0
            for strand, pat in ((0, fwd), (1, rev)):
                mm = np.zeros(n, dtype=np.int32)
                for j in range(L):
                    mm += g[j:j + n] != pat[j]
                for o in np.nonzero(ok & (mm <= v))[0]:
                    mine.append((q, ci, int(o), strand, int(mm[o])))
        if len(mine) > max_placements:
            dropped += 1
            continue
        out += sorted(mine)
    return out, dropped


def window_of(contig, o, L, P, strand):
    """(ws, we, letters): the window [o - F, o + L + F) clipped to the contig as 1-based coordinates with an exclusive end, on the strand."""
    F = (P - L) // 2
    lo, hi = max(0, o - F), min(len(contig), o + L + F)
    letters = clean(contig[lo:hi])
    return lo + 1, hi + 1, (revcomp(letters) if strand else letters)


@functools.lru_cache(maxsize=None)
def _structures(letters, span, model):
    """[(norm_energy, fold_start, ss, sstype, line energy, line length)] of a window: a8's list, each entry with its line's figures."""
    from tests import oracle_binding
    o = oracle_binding.load()
    lines = o.lfold(letters, span, model=model)["lines"]
    whole = o.structures_from_lines(lines, 55)
    per_line = []
    for ss, e, st in lines:
        per_line += [x + (e, len(ss)) for x in o.structures_from_lines([(ss, e, st)], 55)]
    assert [x[:4] for x in per_line] == whole
    return per_line


def evaluate(letters, span, m0, m1, ws, we, strand, model="vienna-2.1.2"):
    """-> (the passing structure of lowest normalised energy (first of equals) with its maturestar record, or None; the code of the structure of
    lowest normalised energy, or -1 for an empty list)."""
    from tests import oracle_binding
    o = oracle_binding.load()
    structs = _structures(letters, span, model)
    best, lowest = None, None
    for st in structs:
        ms = o.maturestar(st[2], m0, m1, st[1], ws, we, strand)
        if lowest is None or st[0] < lowest[0]:
            lowest = (st[0], ms.code)
        if ms.code == 0 and (best is None or st[0] < best[0][0]):
            best = (st, ms)
    return best, (-1 if lowest is None else lowest[1])


def run(queries, contigs, v=1, P=300, max_placements=100, model="vienna-2.1.2"):
    """queries: [(sequence, [names])] as homologs.read_known returns them; contigs: [(name, letters)] as the index defines them.  -> (the loci as
    homologs.loci_of returns them, the counts of homolog_last_stats that §26 defines)."""
    pl, dropped = placements([q for q, _ in queries], contigs, v, max_placements)
    stats = {"queries": len(queries), "repeat_like": dropped, "placements": len(pl), "passing": 0, "loci": 0, "fail_codes": [0] * 13, "no_structure": 0}
    sites = {}
    for q, ci, o, strand, mm in pl:
        L = len(queries[q][0])
        ws, we, letters = window_of(contigs[ci][1], o, L, P, strand)
        best, code = evaluate(letters, P, o + 1, o + L + 1, ws, we, strand, model)
        if best is None:
            if code < 0:
                stats["no_structure"] += 1
            else:
                stats["fail_codes"][code] += 1
            continue
        stats["passing"] += 1
        sites.setdefault((ci, strand, o + 1, o + L + 1), []).append((mm, q, ws, we, letters, best))
    loci = []
    for (ci, strand, m0, m1), group in sites.items():
        group.sort(key=lambda x: (x[0], x[1]))
        mm, q, ws, we, letters, (st, ms) = group[0]
        cut = lambda a, b: homologs.interval(letters, ws, we, strand, a, b)
        loci.append((ci, {"names": list(queries[q][1]), "contig": contigs[ci][0], "strand": "+-"[strand], "mat_s": m0, "mat_e": m1, "mature": cut(m0, m1),
                          "mismatches": mm, "arm": "5p" if ms.prime5 else "3p", "star_s": ms.star_s, "star_e": ms.star_e,
                          "star": cut(ms.star_s, ms.star_e), "fold_s": ms.fold_s, "fold_e": ms.fold_e, "precursor": cut(ms.fold_s, ms.fold_e),
                          "energy": st[4], "line_len": st[5], "total_bps": ms.total_bps, "total_dots": ms.total_dots, "ss": st[2],
                          "also": [(list(queries[k][1]), m) for k, m in sorted((x[1], x[0]) for x in group[1:])]}))
    loci.sort(key=lambda x: (x[0], x[1]["fold_s"], x[1]["strand"] == "-", x[1]["mat_s"], x[1]["mat_e"]))
    stats["loci"] = len(loci)
    return [x for _, x in loci], stats


# ---- generators shared by the CPU and the GPU tests
def random_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def planted_hairpin(rng, v):
    """(hairpin letters, known sequence, offset of the known sequence's site in the hairpin): a random arm, a loop of 8..40 nt and the arm's reverse
    complement with at most two substitutions and one 1-nt bulge; the known sequence is a 21-nt stretch of the arm mutated at <= v positions."""
    arm = random_seq(rng, rng.randint(38, 46))
    loop = random_seq(rng, rng.randint(8, 40))
    other = list(revcomp(arm))
    for _ in range(rng.randint(0, 2)):
        p = rng.randrange(len(other))
        other[p] = rng.choice([c for c in "ACGT" if c != other[p]])
    if rng.random() < 0.5:
        other.insert(rng.randrange(5, len(other) - 5), rng.choice("ACGT"))
    at = rng.randint(6, len(arm) - 21 - 6)
    known = list(arm[at:at + 21])
    for p in rng.sample(range(21), rng.randint(0, v)):
        known[p] = rng.choice([c for c in "ACGT" if c != known[p]])
    return arm + loop + "".join(other), "".join(known), at


def planted_genome(seed, contig_lens, n_planted, v, n_decoys=0):
    """(contigs [(name, letters)], queries [(sequence, [names])], planted [(contig, 0-based offset, strand)]): hairpins planted on either strand of
    random contigs, at least 400 nt apart, with their known sequences first and n_decoys decoy sequences of 21 nt behind them."""
    rng = random.Random(seed)
    contigs = [list(random_seq(rng, n)) for n in contig_lens]
    slots = [(ci, at) for ci, n in enumerate(contig_lens) for at in range(200, n - 400, 400)]
    queries, planted = [], []
    for k, (ci, at) in enumerate(rng.sample(slots, n_planted)):
        hp, known, off = planted_hairpin(rng, v)
        strand = rng.randrange(2)
        contigs[ci][at:at + len(hp)] = revcomp(hp) if strand else hp
        planted.append((ci, at + (len(hp) - off - 21 if strand else off), strand))
        queries.append((known, ["pln-miR%d" % (k + 1)]))
    for k in range(n_decoys):          # decoys: random 21-nt sequences, every other one copied from a random place of the genome (either strand)
        seq = random_seq(rng, 21)
        if k % 2:
            ci = rng.randrange(len(contigs))
            at = rng.randrange(len(contigs[ci]) - 21)
            seq = "".join(contigs[ci][at:at + 21])
            seq = revcomp(seq) if rng.randrange(2) else seq
        queries.append((seq, ["dcy-miR%d" % (k + 1)]))
    assert len({q for q, _ in queries}) == len(queries)
    return [("chr%d" % (i + 1), "".join(c)) for i, c in enumerate(contigs)], queries, planted


def found(loci, contigs, planted):
    """How many of the planted sites are loci."""
    names = [n for n, _ in contigs]
    have = {(names.index(x["contig"]), x["mat_s"] - 1, "+-".index(x["strand"])) for x in loci}
    return sum(1 for p in planted if p in have)


MIXTURE = dict(seed=11, contig_lens=(50000, 40000, 30000, 20000, 10000), n_planted=40, v=2, n_decoys=200)


@functools.lru_cache(maxsize=None)
def mixture():
    """The mixture of the GPU test (40 planted loci and 200 decoys in 150 kb of 5 contigs, v = 2) with its restatement, computed once."""
    contigs, queries, planted = planted_genome(**MIXTURE)
    loci, stats = run(queries, contigs, v=2)
    return contigs, queries, planted, loci, stats


def write_fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
            if not seq:
                f.write("\n")
