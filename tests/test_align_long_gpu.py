"""GPU tests of the read alignment where -v 1..3 meets reads past 30 nt, contig joins and more than one batch (align_kernels.hip, mirp_align.cpp;
DESIGN.md §12).  With a half longer than 16 bases the seed is a prefix of the half: a substitution variant beyond it shares the exact half's SA
range and only al_check tells the two apart, and the canonical-finder rule has to count every hit once.  Every comparison is the whole .sam
against the brute-force restatement of tests/test_align_cpu.py; the guards on the inputs are asserted from the brute-force hits."""
import numpy as np
import pytest

from tests.test_align_cpu import brute_hits, load_reads, load_reference, normalise_pg, revcomp, sam_bytes
from tests.test_align_gpu import _letters, _write_fasta

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N = 4                                   # the code of a base outside ACGT


def _rc_letters(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def _write_reads(path, reads, rng=None, sample="S"):
    """reads: code arrays -> FASTA with QNAMEs <sample>_r<k>_x1; with rng some lower case and, for every fourth longer read, two or more lines."""
    with open(path, "wb") as f:
        for k, r in enumerate(reads):
            s = _letters(r, rng, lower=0.1 if rng is not None else 0.0)
            f.write(b">%s_r%d_x1\n" % (sample.encode(), k))
            if rng is not None and len(s) > 15 and k % 4 == 0:
                f.write(s[:9] + b"\n" + b"".join(s[i:i + 70] + b"\n" for i in range(9, len(s), 70)))
            else:
                f.write(s + b"\n")


def _first_diff(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i in range(max(len(g), len(w))):
        a, b = (g[i] if i < len(g) else None), (w[i] if i < len(w) else None)
        if a != b:
            return "line %d of %d / %d: device %r, restatement %r" % (i, len(g), len(w), a and a[:300], b and b[:300])
    return "equal"


def _assert_no_record_twice(got, what):
    seen = set()
    for ln in got.split(b"\n"):
        if ln and not ln.startswith(b"@"):
            key = tuple(ln.split(b"\t", 4)[:4])
            assert key not in seen, "a hit printed twice (QNAME, FLAG, RNAME, POS) = %r at %r" % (key, what)
            seen.add(key)


def _compare(ctx, ref, reads_path, reads, hits, out, v, k, m=0, f=False):
    """One device call against the restatement: no record twice, whole-file byte equality, the stats identities."""
    names, seqs = ref
    res = ctx.align_reads(reads_path, out, "x", v=v, k=k, m=m, filter_unmapped=f)
    got = normalise_pg(open(out, "rb").read())
    _assert_no_record_twice(got, (v, k, m, f))
    want = sam_bytes(names, seqs, reads, hits, v, k, m, f)
    assert got == want, ((v, k, m, f), _first_diff(got, want))
    assert res["reads"] == len(reads) == res["aligned"] + res["unaligned"] + res["suppressed"]
    assert res["records"] == want.count(b"\n") - 2 - len(names)
    return res


def _best(hs, v):
    """(best stratum, its hits) of a read at -v v."""
    hs = [h for h in hs if h[3] <= v]
    b = min((h[3] for h in hs), default=None)
    return b, [h for h in hs if h[3] == b]


# ---------------------------------------------------------------------------------------------------- 1. long reads, every mismatch split
LENGTHS = (30, 31, 32, 33, 34, 35, 47, 48, 49, 63, 64, 65, 100, 151, 255, 256, 257, 1023, 1024)
SPLITS = [(a, b) for a in range(4) for b in range(4 - a)]                  # (nA, nB), nA + nB <= 3: 10 splits


def _long_genome(rng):
    """Three contigs over two files (about 13 kb): random sequence, an N run, 40 copies of a 23-mer, a 60-nt reverse-complement palindrome, lower
    case, IUPAC codes.  -> (files, the clean regions (contig, lo, hi) that the constructed reads are cut from)."""
    def rnd(n):
        return ACGT[rng.randint(0, 4, n)].copy()
    z = rnd(7000)
    z[1200:1260] = ord("N")
    z[5000:5000 + 23 * 40] = np.tile(rnd(23), 40)
    x = rnd(30)
    z[6000:6060] = np.frombuffer(x.tobytes() + _rc_letters(x.tobytes()), dtype=np.uint8)
    z[100:400] += 32
    ten = rnd(3500)
    ten[0:5] = ord("N")
    ten[-3:] = ord("n")
    a = rnd(2600)
    a[1000:1005] = ord("K")
    a[1700:1900] += 32
    files = [[("chrZ", z.tobytes()), ("chr10", ten.tobytes())], [("chrEmpty", b""), ("chrA", a.tobytes())]]
    return files, [(0, 0, 1200), (0, 1260, 4990), (1, 5, 3497), (2, 1005, 2600), (2, 0, 1000)]


def _half_positions(hlen, n, mode):
    """n positions inside a half of hlen bases: `inside` its 16-base seed, `beyond` it (what does not fit there goes inside), or with the half's
    `first` / `last` base."""
    m = min(hlen, 16)
    if mode == "inside":
        return [[], [m - 1], [2, m - 1], [1, 8, m - 1]][n]
    if mode == "beyond":
        far = sorted({p for p in [[], [16], [16, hlen - 1], [16, (16 + hlen) // 2, hlen - 1]][n] if 16 <= p < hlen})
        return far + [1, 8, 13][:n - len(far)]
    if mode == "first":
        return [[], [0], [0, hlen - 1], [0, 1, hlen - 1]][n]
    return [[], [hlen - 1], [hlen - 2, hlen - 1], [0, hlen - 2, hlen - 1]][n]


class _LongSet:
    """The constructed reads of test 1 and what was planted in each: meta[i] = dict(L, tid, off, strand, split, subs, ns, kind)."""

    def __init__(self, seqs, regions, rng):
        self.seqs, self.regions, self.rng = seqs, regions, rng
        self.reads, self.meta = [], []
        self.n_sub = 0

    def window(self, L, site=None):
        if site is None:
            fit = [r for r in self.regions if r[2] - r[1] >= L]
            t, lo, hi = fit[len(self.reads) % len(fit)]
            site = (t, int(self.rng.randint(lo, hi - L + 1)))
        w = self.seqs[site[0]][site[1]:site[1] + L]
        assert len(w) == L and (w < 4).all()
        return site, w.copy()

    def add(self, L, strand, subs=(), ns=(), kind="planted", site=None):
        """A read whose oriented sequence is the window with substitutions at `subs` and a read N at `ns` (oriented positions)."""
        site, o = self.window(L, site)
        assert len(set(subs) | set(ns)) == len(subs) + len(ns) and all(0 <= p < L for p in list(subs) + list(ns))
        for p in subs:
            o[p] = (o[p] + 1 + self.n_sub % 3) % 4
            self.n_sub += 1
        for p in ns:
            o[p] = N
        a = (L + 1) // 2
        split = (sum(p < a for p in list(subs) + list(ns)), sum(p >= a for p in list(subs) + list(ns)))
        self.reads.append(revcomp(o) if strand else o)
        self.meta.append(dict(L=L, tid=site[0], off=site[1], strand=strand, split=split, subs=tuple(subs), ns=tuple(ns), kind=kind))

    def planted(self, L, strand, nA, nB, mode, site=None):
        a = (L + 1) // 2
        self.add(L, strand, [p for p in _half_positions(a, nA, mode)] + [a + p for p in _half_positions(L - a, nB, mode)], site=site)


def _placement(mt):
    """Where the planted substitutions of a read lie with respect to the 16-base seeds of their halves: inside, beyond, or mixed."""
    a = (mt["L"] + 1) // 2
    rel = [p if p < a else p - a for p in mt["subs"]]
    return "inside" if all(p < 16 for p in rel) else "beyond" if all(p >= 16 for p in rel) else "mixed"


@pytest.fixture(scope="module")
def long_reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_long")
    rng = np.random.RandomState(1201)
    files, regions = _long_genome(rng)
    refs = []
    for i, recs in enumerate(files):
        _write_fasta(d / ("ref%d.fa" % i), recs)
        refs.append(str(d / ("ref%d.fa" % i)))
    names, seqs = load_reference(refs)
    assert names == ["chrZ", "chr10", "chrA"] and 12000 < sum(len(s) for s in seqs) <= 15000
    S = _LongSet(seqs, regions, rng)
    for L in LENGTHS:
        a = (L + 1) // 2
        if L < 255:
            for strand in (0, 1):
                # the exact read: once at a contig's first base, once at a contig's last
                S.planted(L, strand, 0, 0, "inside", site=(2, 0) if strand == 0 else (0, len(seqs[0]) - L))
                for nA, nB in SPLITS[1:]:
                    for mode in ("inside", "beyond", "first", "last"):
                        if mode != "beyond" or L >= 34:
                            S.planted(L, strand, nA, nB, mode)
                # a read N in place of a substitution, inside the seed and beyond it, and halves with two N (no seed from that half)
                far = L >= 34
                S.add(L, strand, ns=[3], kind="n")
                S.add(L, strand, ns=[3], subs=[a + (16 if far else 5)], kind="n")
                S.add(L, strand, ns=[16 if far else 9], kind="n")
                S.add(L, strand, ns=[a + 2], kind="n")
                S.add(L, strand, ns=[a + (16 if far else 7)], subs=[16 if far else 4], kind="n")
                S.add(L, strand, ns=[2, 9], kind="n")
                S.add(L, strand, ns=[a + 1, L - 1], subs=[a - 1], kind="n")
        else:
            S.planted(L, 0, 0, 0, "inside")
            S.planted(L, 1, 1, 1, "beyond")
            S.planted(L, 0, 2, 1, "beyond")
            S.planted(L, 1, 0, 3, "last")
            S.planted(L, 0, 1, 2, "first")
            S.add(L, 1, ns=[a // 2], subs=[a + 40], kind="n")
    for k in range(30):                                   # inside the 23-mer array: many hits in the best stratum
        L = 40 + (k * 37) % 161
        off = 5000 + int(rng.randint(0, 920 - L + 1))
        S.add(L, k % 2, subs=[int(p) for p in rng.choice(L, k % 3, replace=False)], kind="array", site=(0, off))
    S.add(60, 0, kind="palindrome", site=(0, 6000))       # its own reverse complement: one offset, both strands
    S.add(60, 0, subs=[41], kind="palindrome", site=(0, 6000))
    path = d / "reads.fa"
    _write_reads(path, S.reads, rng)
    reads = load_reads(str(path))
    assert all(np.array_equal(r, s) for (_, r), s in zip(reads, S.reads))
    assert sum(len(r) for r in S.reads) < 150000
    return {"dir": d, "refs": refs, "ref": (names, seqs), "path": str(path), "reads": reads, "meta": S.meta, "hits": brute_hits(seqs, reads, vmax=3)}


def test_long_reads_every_mismatch_split(gpu_ctx, long_reads):
    D = long_reads
    names, seqs = D["ref"]
    meta, hits = D["meta"], D["hits"]
    # ---- guards on the input, from the brute-force hits
    covered = set()
    for mt, (_, r), hs in zip(meta, D["reads"], hits):
        if mt["kind"] != "planted":
            continue
        o = revcomp(r) if mt["strand"] else r
        d = o != seqs[mt["tid"]][mt["off"]:mt["off"] + mt["L"]]
        a = (mt["L"] + 1) // 2
        assert (int(d[:a].sum()), int(d[a:].sum())) == mt["split"] and int(d.sum()) == len(mt["subs"])
        mm = sum(mt["split"])
        for v in range(mm, 4):                            # its best-stratum hit at the planted offset has exactly the planted split
            b, sel = _best(hs, v)
            if b == mm and (mt["tid"], mt["off"], mt["strand"], mm) in sel:
                covered.add((v, mt["split"], mt["strand"], _placement(mt)))
                for p in mt["subs"]:
                    covered.add((v, mt["strand"], "pos", "0" if p == 0 else "a-1" if p == a - 1 else "a" if p == a else "L-1" if p == mt["L"] - 1 else ""))
    for v in range(4):
        for split in SPLITS:
            if sum(split) <= v:
                for strand in (0, 1):
                    for place in (("inside", "beyond") if sum(split) else ("inside",)):
                        assert (v, split, strand, place) in covered, (v, split, strand, place)
    for v in range(1, 4):
        for strand in (0, 1):
            for pos in ("0", "a-1", "a", "L-1"):
                assert (v, strand, "pos", pos) in covered, (v, strand, pos)
    for strand in (0, 1):                                 # read N: inside and beyond the seed of either half, and two in one half
        for want_ns in ("A in", "A far", "B in", "B far", "A two", "B two"):
            def is_kind(mt):
                a = (mt["L"] + 1) // 2
                rel = [(p < a, p if p < a else p - a) for p in mt["ns"]]
                half = "A" if rel[0][0] else "B"
                return half + (" two" if len(rel) == 2 else " in" if rel[0][1] < 16 else " far") == want_ns
            found = [i for i, mt in enumerate(meta) if mt["kind"] == "n" and mt["strand"] == strand and is_kind(mt) and
                     (mt["tid"], mt["off"], strand, sum(mt["split"])) in _best(hits[i], 3)[1]]
            assert found, (strand, want_ns)
    assert sum(len(_best(hs, 3)[1]) > 20 for hs in hits) >= 5
    for L in LENGTHS:
        assert any(mt["L"] == L and _best(hs, 3)[0] is not None for mt, hs in zip(meta, hits)), L
    pal = [hs for mt, hs in zip(meta, hits) if mt["kind"] == "palindrome"]
    assert (0, 6000, 0, 0) in pal[0] and (0, 6000, 1, 0) in pal[0] and (0, 6000, 0, 1) in pal[1] and (0, 6000, 1, 1) in pal[1]
    # ---- the device
    idx = gpu_ctx.align_index(D["refs"])
    assert idx["n_contigs"] == 3 and idx["total"] == sum(len(s) for s in seqs)
    out = str(D["dir"] / "out.sam")
    suppressed = 0
    for v in range(4):
        for k in (1, 10 ** 6):
            for m in (0, 3):
                suppressed += _compare(gpu_ctx, D["ref"], D["path"], D["reads"], hits, out, v, k, m)["suppressed"]
                assert gpu_ctx.align_last_batches() == 1
        _compare(gpu_ctx, D["ref"], D["path"], D["reads"], hits, out, v, 20, 3, f=True)
    assert suppressed > 0


# ---------------------------------------------------------------------------------------------------- 2. contig joins, ambiguous bases, padding
def _join_genome(rng):
    def rnd(n):
        return ACGT[rng.randint(0, 4, n)].copy()
    c1 = rnd(1500)
    c1[-21], c1[-20:] = ord("C"), ord("A")
    c2 = rnd(1200)
    c2[:30], c2[30] = ord("A"), ord("G")
    c3 = rnd(3000)
    c3[981], c3[982:1000], c3[1000:1040] = ord("T"), ord("A"), ord("N")
    c3[400], c3[1800], c3[2500] = ord("R"), ord("-"), ord("n")
    c4 = rnd(1300)
    c4[-26], c4[-25:] = ord("G"), ord("A")
    return [[("c1", c1.tobytes()), ("c2", c2.tobytes()), ("cEmpty", b""), ("c3", c3.tobytes())], [("c4", c4.tobytes())]]


def test_contig_joins_ambiguous_bases_and_padding(gpu_ctx, tmp_path):
    rng = np.random.RandomState(1202)
    refs = []
    for i, recs in enumerate(_join_genome(rng)):
        _write_fasta(tmp_path / ("ref%d.fa" % i), recs)
        refs.append(str(tmp_path / ("ref%d.fa" % i)))
    names, seqs = load_reference(refs)
    assert names == ["c1", "c2", "c3", "c4"]                # the empty contig is dropped: c2 and c3 are neighbours in the concatenation
    cat = np.concatenate(seqs)
    cstart = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    reads, meta = [], []              # meta: (kind, tid, offset of the construction site in that contig (may run past its end), substitutions, strand)

    def add(r, kind, tid, off, nsub=0):
        for strand in (0, 1):
            reads.append(revcomp(r) if strand else r.copy())
            meta.append((kind, tid, off, nsub, strand))

    def with_sub(r, p):
        r = r.copy()
        r[p] = (r[p] + 1 + p % 3) % 4
        return r
    for t in range(3):                # straddlers: the last x bases of contig t and the first L - x of contig t + 1
        for L in (20, 40, 100):
            h = (L + 1) // 2
            for x in (1, h - 1, h, h + 1, L - 1):
                r = np.concatenate([seqs[t][len(seqs[t]) - x:], seqs[t + 1][:L - x]])
                assert len(r) == L and np.array_equal(r, cat[cstart[t + 1] - x:cstart[t + 1] - x + L])
                add(r, "straddler", t, len(seqs[t]) - x)
                add(with_sub(r, (7 * x + 3) % L), "straddler", t, len(seqs[t]) - x, 1)
            for r, off in ((seqs[t][len(seqs[t]) - L:], len(seqs[t]) - L), (seqs[t + 1][:L], 0)):       # controls: wholly inside one contig
                tt = t if off else t + 1
                add(r, "control", tt, off)
                add(with_sub(r, L // 2 + t), "control", tt, off, 1)
    amb = [int(p) for p in np.nonzero(seqs[2] == N)[0] if not (1000 <= p < 1040)]
    assert amb == [400, 1800, 2500]
    for p in amb:                     # reads over one ambiguous reference base, that base set to each of A, C, G, T
        for lo, hi in ((p - 20, p + 30), (p - 150, p + 50)):
            for b in range(4):
                r = seqs[2][lo:hi].copy()
                assert (r == N).sum() == 1 and r[p - lo] == N
                r[p - lo] = b
                add(r, "ambiguous", 2, lo)
        add(seqs[2][p + 1:p + 51], "control", 2, p + 1)
        add(seqs[2][p - 200:p], "control", 2, p - 200)
    polya = {}
    for k in (18, 25, 40):            # poly-A reads next to the padded keys
        polya[k] = len(reads)
        add(np.zeros(k, np.uint8), "polyA", -1, -1)
    for t, run, pre, ks in ((0, 20, len(seqs[0]) - 28, (18, 20, 21, 22, 30, 45)),           # 8 bases, then A running past the contig's end,
                            (3, 25, len(seqs[3]) - 33, (24, 25, 26, 27, 33, 41)),           # past the genome's end
                            (2, 18, 974, (17, 18, 19, 20, 26, 34))):                        # and into the N run
        assert (seqs[t][pre + 8:pre + 8 + run] == 0).all() and seqs[t][pre + 7] != 0
        for k in ks:
            add(np.concatenate([seqs[t][pre:pre + 8], np.zeros(k, np.uint8)]), "control" if k <= run else "padding", t, pre)
    assert np.array_equal(cat[cstart[1] - 20:cstart[1] + 30], np.zeros(50, np.uint8))     # c1 | c2 is 50 A in the concatenation
    path = tmp_path / "reads.fa"
    _write_reads(path, reads, rng)
    rd = load_reads(str(path))
    assert all(np.array_equal(a, b) for (_, a), b in zip(rd, reads)) and sum(len(r) for r in reads) < 150000
    hits = brute_hits(seqs, rd, vmax=3)
    # ---- guards, from the brute-force hits
    probes = [i for i, mt in enumerate(meta) if mt[0] in ("straddler", "ambiguous")]
    for i, (kind, t, off, nsub, strand) in enumerate(meta):
        at_site = [h for h in hits[i] if h[0] == t and h[1] == off and h[2] == strand]
        if kind in ("straddler", "ambiguous", "padding"):
            assert not at_site, (i, meta[i])
        elif kind == "control":
            assert at_site and at_site[0][3] == nsub == _best(hits[i], 3)[0], (i, meta[i])
    assert len(probes) == 2 * (3 * 3 * 5 * 2 + 3 * 2 * 4)
    assert sum(not hits[i] for i in probes) >= 0.8 * len(probes)
    ends18 = {(0, 1480 + j, 0, 0) for j in range(3)} | {(1, j, 0, 0) for j in range(13)} | {(2, 982, 0, 0)} | {(3, 1275 + j, 0, 0) for j in range(8)}
    assert {h for h in hits[polya[18]] if h[3] == 0} == ends18
    assert {h for h in hits[polya[25]] if h[3] == 0} == {(1, j, 0, 0) for j in range(6)} | {(3, 1275, 0, 0)}
    assert not hits[polya[40]]                            # 40 A exist only across the c1 | c2 join
    # ---- the device: the bytes show the straddlers, the reads over an ambiguous base and the over-long A tails unaligned
    idx = gpu_ctx.align_index(refs)
    assert idx["n_contigs"] == 4 and idx["total"] == len(cat)
    for v in range(4):
        res = _compare(gpu_ctx, (names, seqs), str(path), rd, hits, str(tmp_path / "out.sam"), v, 10 ** 6)
        assert res["unaligned"] >= sum(not hits[i] for i in range(len(rd)))


# ---------------------------------------------------------------------------------------------------- 3. a file that takes two batches
def _batches_of(ctx, tmp_path, lengths, n):
    """Batches that a file of the first n of these read lengths takes at -v 2.  The reads are all N: the host cuts batches by the lengths alone, and a
    read of N has no seed, so the probe costs the device next to nothing."""
    p = tmp_path / "probe.fa"
    with open(p, "wb") as f:
        f.write(b"".join(b">P_r%d_x1\n%s\n" % (k, b"N" * L) for k, L in enumerate(lengths[:n])))
    ctx.align_reads(str(p), str(tmp_path / "probe.sam"), "x", v=2, k=1)
    return ctx.align_last_batches()


def _first_batch(ctx, tmp_path, lengths, near=None):
    """Reads in the first batch of a file of these lengths, found by bisection over prefixes of the file (the last prefix that runs in one batch)."""
    lo, hi = 1, len(lengths)
    if near is not None and near - 3 >= 1 and near + 3 <= len(lengths) and _batches_of(ctx, tmp_path, lengths, near - 3) == 1 \
            and _batches_of(ctx, tmp_path, lengths, near + 3) > 1:
        lo, hi = near - 3, near + 3
    else:
        assert _batches_of(ctx, tmp_path, lengths, lo) == 1 and _batches_of(ctx, tmp_path, lengths, hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _batches_of(ctx, tmp_path, lengths, mid) == 1:
            lo = mid
        else:
            hi = mid
    return lo


def test_a_file_that_takes_two_batches(gpu_ctx, tmp_path):
    rng = np.random.RandomState(1203)
    g1, g2 = rng.randint(0, 4, 40000).astype(np.uint8), rng.randint(0, 4, 20000).astype(np.uint8)
    seg = rng.randint(0, 4, 1500).astype(np.uint8)
    g1[5000:6500] = g1[25000:26500] = g2[8000:9500] = seg               # three copies: -m 2 suppresses the reads cut from them
    _write_fasta(tmp_path / "g.fa", [("c1", _letters(g1)), ("c2", _letters(g2))], width=80)
    names, seqs = load_reference([str(tmp_path / "g.fa")])
    free = [(0, 6600, 24900), (0, 26600, 40000), (1, 0, 7900), (1, 9600, 20000)]        # away from the copies
    T, kind = [], []

    def cut(i, nsub=0, ns=()):
        t, lo, hi = free[i % 4]
        off = int(rng.randint(lo, hi - 1024 + 1))
        o = seqs[t][off:off + 1024].copy()
        for p in rng.choice(1024, nsub, replace=False):
            o[p] = (o[p] + 1 + p % 3) % 4
        for p in ns:
            o[p] = N
        return revcomp(o) if i % 2 else o
    for i in range(30):
        T.append(cut(i, nsub=i % 3)); kind.append("minus" if i % 2 else "plus")
    for i in range(4):
        T.append(rng.randint(0, 4, 1024).astype(np.uint8)); kind.append("random")
    for i in range(4):
        o = seg[100 * i:100 * i + 1024].copy()
        T.append(revcomp(o) if i % 2 else o); kind.append("copies")
    T.append(cut(0, ns=[5])); kind.append("n")
    T.append(cut(1, ns=[700])); kind.append("n")
    T.append(np.zeros(0, np.uint8)); kind.append("empty")
    T.append(np.array([0, 1], np.uint8)); kind.append("two")
    templates = [("T%d" % j, r) for j, r in enumerate(T)]
    hits = brute_hits(seqs, templates, vmax=3)
    for j, hs in enumerate(hits):                         # the templates are what they are meant to be
        b, sel = _best(hs, 2)
        assert {"plus": b == j % 3 and len(sel) == 1 and sel[0][2] == 0, "minus": b == j % 3 and len(sel) == 1 and sel[0][2] == 1, "random": not hs,
                "copies": b == 0 and len(sel) == 3, "n": b == 1 and len(sel) == 1, "empty": not hs, "two": len(hs) > 20}[kind[j]], (j, kind[j])
    text = [_letters(r) for r in T]
    gpu_ctx.align_index([str(tmp_path / "g.fa")])

    # ---- the order of the records: the templates in turn, and around the split an unaligned read, the empty read | a suppressed read, a read on -.
    # The split is read off the device: probes of the same read lengths say which prefixes of the file still run in one batch.
    count = 8400
    while _batches_of(gpu_ctx, tmp_path, [len(T[k % len(T)]) for k in range(count)], count) < 2:
        count += 2000
        assert count <= 40000
    around = [kind.index("random"), kind.index("empty"), kind.index("copies"), kind.index("minus")]

    def order_for(s):
        order = [k % len(T) for k in range(count)]
        if s is not None:
            order[s - 2:s + 2] = around
        return order
    s, order = None, order_for(None)
    for _ in range(5):
        s2 = _first_batch(gpu_ctx, tmp_path, [len(T[j]) for j in order], near=s)
        if s2 == s:
            break
        s, order = s2, order_for(s2)
    else:
        raise AssertionError("the split did not settle")
    assert 2 <= s <= count - 2 and [order[s + i] for i in (-2, -1, 0, 1)] == around
    qn = [b"S_r%d_x1" % k for k in range(count)]

    def write(path, lo, hi):
        with open(path, "wb") as f:
            f.write(b"".join(b">%s\n%s\n" % (qn[k], text[order[k]]) for k in range(lo, hi)))
    write(tmp_path / "all.fa", 0, count)
    assert 8.0e6 < (tmp_path / "all.fa").stat().st_size

    def expected(v, k, m):
        """header, per-record bytes and per-record class: every template formatted once by the restatement, the QNAME substituted."""
        want = sam_bytes(names, seqs, templates, hits, v, k, m).split(b"\n")[:-1]
        head, per = want[:4], [[] for _ in T]
        for ln in want[4:]:
            q, rest = ln.split(b"\t", 1)
            per[int(q[1:])].append(b"\t" + rest + b"\n")
        assert all(per)
        cls = ["aligned" if not p[0].startswith(b"\t4\t") else "suppressed" if p[0].endswith(b"XM:i:%d\n" % (m + 1)) and m else "unaligned" for p in per]
        return b"".join(h + b"\n" for h in head), [b"".join(qn[k] + ln for ln in per[order[k]]) for k in range(count)], [cls[j] for j in order], per

    def check_stats(res, cls, per, lo, hi):
        assert res["reads"] == hi - lo
        for c in ("aligned", "unaligned", "suppressed"):
            assert res[c] == sum(x == c for x in cls[lo:hi]), c
        assert res["records"] == sum(len(per[order[k]]) for k in range(lo, hi))

    def run(path, v, k, m):
        res = gpu_ctx.align_reads(str(path), str(path) + ".sam", "x", v=v, k=k, m=m)
        return res, normalise_pg(open(str(path) + ".sam", "rb").read())
    for v, k, m in ((2, 20, 2), (3, 1, 0)):
        head, recs, cls, per = expected(v, k, m)
        res, got = run(tmp_path / "all.fa", v, k, m)
        assert gpu_ctx.align_last_batches() >= 2
        want = head + b"".join(recs)
        assert got == want, ((v, k, m), _first_diff(got, want))
        check_stats(res, cls, per, 0, count)
        if m:
            assert [cls[s + i] for i in (-2, -1, 0, 1)] == ["unaligned", "unaligned", "suppressed", "aligned"] and b"\t16\t" in recs[s + 1][:40]
            assert res["suppressed"] >= count // len(T) * 4
    # ---- the same reads as two files cut somewhere else: the same records
    head, recs, cls, per = expected(2, 20, 2)
    cutat = count // 3
    assert abs(cutat - s) > 100
    parts = []
    for name, lo, hi in (("a.fa", 0, cutat), ("b.fa", cutat, count)):
        write(tmp_path / name, lo, hi)
        res, got = run(tmp_path / name, 2, 20, 2)
        assert got.startswith(head)
        check_stats(res, cls, per, lo, hi)
        parts.append(got[len(head):])
    assert b"".join(parts) == b"".join(recs)
    # ---- -v 0 has two seeds a read: one batch
    head, recs, cls, per = expected(0, 20, 0)
    res, got = run(tmp_path / "all.fa", 0, 20, 0)
    assert gpu_ctx.align_last_batches() == 1
    want = head + b"".join(recs)
    assert got == want, ((0, 20, 0), _first_diff(got, want))
    check_stats(res, cls, per, 0, count)
