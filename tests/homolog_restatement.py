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
def _lines(letters, span, model):
    """[(ss, energy, start)]: the structure lines of a window's fold."""
    from tests import oracle_binding
    return oracle_binding.load().lfold(letters, span, model=model)["lines"]


@functools.lru_cache(maxsize=None)
def _structures(letters, span, model):
    """[(norm_energy, fold_start, ss, sstype, line energy, line length)] of a window: a8's list, each entry with its line's figures."""
    from tests import oracle_binding
    o = oracle_binding.load()
    lines = _lines(letters, span, model)
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


# ---- inputs of tests/test_homologs_large_gpu.py: windows of 600 .. 2,500 nt.  Every builder returns its input with the figures its test conditions
# read, computed from the restatement alone; tests/test_homologs_cpu.py asserts those conditions without a GPU.
FOLD_LINES, STAGED_LINES, MIN_LINE = 96, 48, 55          # mirp_homolog_scan's defaults: lines the fold keeps at first, lines staged at first, a8's minlen
ORACLE_MAX_LINES, ORACLE_MAX_STRUCTS = 384, 512           # what tests/oracle_binding.py holds per window
BOUNDARIES = (32, 64, 96, 128, 160, 192)
_SWAP = {"A": "C", "C": "A", "G": "T", "T": "G"}


def ssw_words(n_chars):
    return (n_chars + 31) >> 5


def eval_lds(max_lines, stride, caps, text_in_lds=True):
    """hm_eval_lds of homolog_kernels.hip: the dynamic LDS bytes of homolog_eval_kernel at caps = (pieces, structures, staged lines)."""
    p_cap, s_cap, l_cap = caps
    b = ((l_cap * ssw_words(stride) * 8 + 15) & ~15) if text_in_lds else 0
    b += 8 * (s_cap + 64 * p_cap) + 4 * 64 + 2 * (max_lines + l_cap)
    return (b + 15) & ~15


def window_shapes(queries, contigs, v, P, max_placements=100, model="vienna-2.1.2"):
    """[{letters, lines, usable (lines of at least 55 characters), structures}] of every placement's window, in placement order."""
    pl, _ = placements([q for q, _ in queries], contigs, v, max_placements)
    out = []
    for q, ci, o, strand, mm in pl:
        _, _, letters = window_of(contigs[ci][1], o, len(queries[q][0]), P, strand)
        lines = _lines(letters, P, model)
        out.append({"letters": len(letters), "lines": len(lines), "usable": sum(1 for ss, _, _ in lines if len(ss) >= MIN_LINE),
                    "structures": len(_structures(letters, P, model))})
    return out


def natural_launch(shapes):
    """(max_lines, stride, caps of the last evaluation round, its LDS bytes with the text in LDS) of mirp_device_homolog_eval on one chunk of these
    windows with nothing lowered: the fold is repeated with room for the longest line list, and the windows with more than 48 usable lines are run
    again with capacities for the largest of them."""
    max_lines = max([FOLD_LINES] + [w["lines"] for w in shapes])
    stride = (max(w["letters"] for w in shapes) + 3 + 7) // 8 * 8
    caps = (max(6, stride // 56 + 1), max(2 * max_lines, 192, *[w["structures"] for w in shapes]),
            max([min(max_lines, STAGED_LINES)] + [min(w["usable"], max_lines) for w in shapes]))
    return max_lines, stride, caps, eval_lds(max_lines, stride, caps)


def within_oracle_limits(shapes):
    return all(w["lines"] <= ORACLE_MAX_LINES and w["structures"] <= ORACLE_MAX_STRUCTS for w in shapes)


def long_hairpin(rng, arm_len, loop_len, f5, f3, bulge_at=None, mismatch_at=None, gc=0):
    """(5' flank, arm, loop, other arm, 3' flank): a perfect hairpin whose arm begins with `gc` letters of G and C (the whole stem is then the
    structure of lowest normalised energy, not an inner part of it); bulge_at / mismatch_at: a 2-nt bulge and a substitution in the other arm."""
    arm = "".join(rng.choice("GC") for _ in range(gc)) + random_seq(rng, arm_len - gc)
    other = list(revcomp(arm))
    if mismatch_at is not None:
        other[mismatch_at] = _SWAP[other[mismatch_at]]
    if bulge_at is not None:
        other[bulge_at:bulge_at] = list("AA")
    return random_seq(rng, f5), arm, random_seq(rng, loop_len), "".join(other), random_seq(rng, f3)


# (arm, loop, 5' flank, 3' flank, bulge, mismatch, G/C letters): stems of 96 .. 124 nt so that either arm lies over every boundary of BOUNDARIES in some
# structure, three of them with a bulge and a mismatch
SWEEP = dict(seed=2, P=600, specs=((124, 8, 12, 12, None, None, 24), (120, 10, 12, 16, 40, 80), (122, 10, 12, 12, None, None, 30), (108, 9, 14, 18, 70, 30),
                                   (96, 8, 14, 18), (96, 8, 12, 16, 30, 60)))


def boundary_coverage(records):
    """{(prime5, boundary, "mat" | "star", "in" | "l0" | "l1"): placements, (prime5, "far"): placements} of MatureStar records: the interval
    straddles the boundary, starts at it, ends at it; mature and star four or more words apart."""
    t = {}
    for ms in records:
        for b in BOUNDARIES:
            for name, l0, l1 in (("mat", ms.mat_l0, ms.mat_l1), ("star", ms.star_l0, ms.star_l1)):
                for rel, hit in (("in", l0 < b < l1), ("l0", l0 == b), ("l1", l1 == b)):
                    if hit:
                        t[(ms.prime5, b, name, rel)] = t.get((ms.prime5, b, name, rel), 0) + 1
        if abs((ms.mat_l0 >> 5) - (ms.star_l0 >> 5)) >= 4:
            t[(ms.prime5, "far")] = t.get((ms.prime5, "far"), 0) + 1
    return t


def coverage_gaps(t):
    """What boundary_coverage's table lacks.  A window here is a whole contig of at most 287 nt, so a stem's 5' arm ends before character 128 of any
    structure and its 3' arm begins after character 96: a mature in the 5' arm (prime5 = 1) meets the boundaries 32, 64, 96 and its star 128, 160,
    192, and the other way round with the mature in the 3' arm.  Asked: at every boundary the three positions for the mature and the three for the
    star; on either arm, at every boundary, the three positions for the interval of that arm's placements that can lie there; on either arm a
    placement whose mature and star lie four or more words apart."""
    gaps = []
    for b in BOUNDARIES:
        for name in ("mat", "star"):
            gaps += [(b, name, rel) for rel in ("in", "l0", "l1") if not t.get((0, b, name, rel), 0) + t.get((1, b, name, rel), 0)]
        for p in (1, 0):
            name = "mat" if (b <= 96) == (p == 1) else "star"
            gaps += [(p, b, name, rel) for rel in ("in", "l0", "l1") if not t.get((p, b, name, rel), 0)]
    return gaps + [(p, "far") for p in (1, 0) if not t.get((p, "far"), 0)]


@functools.lru_cache(maxsize=None)
def boundary_sweep():
    """(contigs, queries, MatureStar of the chosen structure of every passing placement, placements): six long hairpins, each a contig short
    enough that every placement's window at P = 600 is the whole contig (two folds per contig serve the restatement), and as queries the 21-nt
    stretch at every offset of both arms (every 16th offset also 18 and 26 nt), none equal to another or to another's reverse complement."""
    rng = random.Random(SWEEP["seed"])
    P = SWEEP["P"]
    contigs, queries, seen = [], [], set()
    for k, spec in enumerate(SWEEP["specs"]):
        f5, arm, loop, other, f3 = long_hairpin(rng, *spec)
        c = f5 + arm + loop + other + f3
        assert len(c) <= (P - 26) // 2
        contigs.append(("hp%d" % (k + 1), c))
        arms = ((len(f5), len(arm)), (len(f5) + len(arm) + len(loop), len(other)))
        for off in range(len(other) - 18 + 1):
            for start, n in (arms if off % 2 == 0 else arms[::-1]):          # the arms of a perfect stem are each other's reverse complement: take turns
                for L in ((21,) if off % 16 else (21, 18, 26)):
                    s = c[start + off:start + off + L]
                    if off + L > n or s in seen or revcomp(s) in seen:
                        continue
                    seen.add(s)
                    queries.append((s, ["swp-%d-%d-%d" % (k + 1, start + off, L)]))
    pl, _ = placements([q for q, _ in queries], contigs, 0, 100)
    records = []
    for q, ci, o, strand, mm in pl:
        L = len(queries[q][0])
        ws, we, letters = window_of(contigs[ci][1], o, L, P, strand)
        assert (ws, we) == (1, len(contigs[ci][1]) + 1)
        best, _ = evaluate(letters, P, o + 1, o + L + 1, ws, we, strand)
        if best is not None:
            records.append(best[1])
    return contigs, queries, records, len(pl)


def spaced_genome(seed, n_planted, v, gap, repeat=None):
    """(contigs, queries): one contig of random sequence with n_planted hairpins (planted_hairpin) on either strand, `gap` nt from each other and
    from the contig's ends; repeat = (hairpin, unit, copies, distance): a run of `copies` x `unit` that far behind that hairpin's end."""
    rng = random.Random(seed)
    g = list(random_seq(rng, gap * (n_planted + 1) + 200))
    queries = []
    for k in range(n_planted):
        hp, known, _ = planted_hairpin(rng, v)
        at = gap * (k + 1)
        g[at:at + len(hp)] = revcomp(hp) if rng.randrange(2) else hp
        if repeat and repeat[0] == k:
            run = repeat[1] * repeat[2]
            g[at + len(hp) + repeat[3]:at + len(hp) + repeat[3] + len(run)] = run
        queries.append((known, ["far-miR%d" % (k + 1)]))
    assert len({q for q, _ in queries}) == len(queries)
    return [("chrL", "".join(g))], queries


THOUSAND = dict(seed=21, n_planted=4, v=1, gap=1300, repeat=(1, "GTGG", 80, 60))


@functools.lru_cache(maxsize=None)
def thousand():
    """(contigs, queries, window_shapes): four planted hairpins 1,300 nt apart for windows of P = 1000 (five placements), the second with 320 nt of
    (GTGG)n in its flank."""
    contigs, queries = spaced_genome(**THOUSAND)
    return contigs, queries, window_shapes(queries, contigs, THOUSAND["v"], 1000)


def global_text_caps(shapes):
    """(fold_lines, eval_caps) that put the staged text of these windows in global memory: the fewest lines, in steps of 64, whose words alone exceed
    the 160 KB of LDS a workgroup can have."""
    _, stride, _, _ = natural_launch(shapes)
    lines = 64
    while lines * ssw_words(stride) * 8 <= 160 * 1024:
        lines += 64
    return lines, (20, 2 * lines, lines)


FIFTEEN_HUNDRED = dict(seed=41, n_planted=1, v=1, gap=800)


@functools.lru_cache(maxsize=None)
def fifteen_hundred():
    """(contigs, queries, window_shapes): one planted hairpin in 1,800 nt, placed on both strands, for windows of P = 1500."""
    contigs, queries = spaced_genome(**FIFTEEN_HUNDRED)
    return contigs, queries, window_shapes(queries, contigs, FIFTEEN_HUNDRED["v"], 1500)


WIDEST_P = 2600
WIDEST = dict(seed=62, n_planted=1, v=1, gap=WIDEST_P // 2 + 60)


@functools.lru_cache(maxsize=None)
def widest():
    """(contigs, queries, window_shapes): one planted hairpin placed once, for a window of P = 2600."""
    contigs, queries = spaced_genome(**WIDEST)
    return contigs, queries, window_shapes(queries, contigs, WIDEST["v"], WIDEST_P)


def write_fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
            if not seq:
                f.write("\n")
