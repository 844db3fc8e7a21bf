"""GPU tests of the placement of multi-mapped reads (mirp_align_reads_placed, `align --place`; DESIGN.md §12 "Placement"): whole .sam files byte for
byte against the brute-force restatement of tests/place_restatement.py.  Every test first asserts, from the restatement alone, that its input holds
the cases it is about."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.place_restatement import draw, hits_of, load_reads, load_reference, place
from tests.test_align_cpu import ROOT, normalise_pg, revcomp, sam_bytes

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _letters(codes):
    s = ACGT[np.minimum(codes, 3)].copy()
    s[codes > 3] = ord("N")
    return s.tobytes()


def _write_fasta(path, records, width=70):
    with open(path, "wb") as f:
        for name, codes in records:
            s = _letters(codes)
            f.write(b">" + name.encode() + b"\n" + b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)))


def _write_reads(path, reads, sample="S"):
    """reads: [(codes, depth)], distinct sequences; ids <sample>_r<k>_x<depth>."""
    assert len({r.tobytes() for r, _ in reads}) == len(reads)
    with open(path, "wb") as f:
        f.write(b"".join(b">%s_r%d_x%d\n%s\n" % (sample.encode(), k, d, _letters(r)) for k, (r, d) in enumerate(reads)))


def _snp(seq, at):
    s = seq.copy()
    for p in at:
        s[p] = (s[p] + 1) % 4
    return s


class Case:
    """A reference and a read file on disk with the restatement's view of them."""

    def __init__(self, d, contigs, reads, vmax):
        self.dir = d
        self.ref = str(d / "g.fa")
        self.reads_path = str(d / "r.fa")
        _write_fasta(self.ref, contigs)
        _write_reads(self.reads_path, reads)
        self.names, self.seqs = load_reference([self.ref])
        self.reads = load_reads(self.reads_path)
        self.hits = hits_of(self.seqs, self.reads, vmax)

    def want(self, v, M, W, seed, mode, f=False):
        return place(self.names, self.seqs, self.reads, self.hits, v, M, W, seed, mode, f)


def _run(ctx, case, v, M, W, seed, mode, f=False, out=None):
    out = out or str(case.dir / "out.sam")
    res = ctx.align_reads(case.reads_path, out, "x", v=v, k=20, m=M, filter_unmapped=f, place=mode, window=W, seed=seed)
    return res, normalise_pg(open(out, "rb").read())


def _check(ctx, case, v, M, W, seed, mode, f=False):
    want, info = case.want(v, M, W, seed, mode, f)
    res, got = _run(ctx, case, v, M, W, seed, mode, f)
    assert got == want, (v, M, W, seed, mode, f)
    cls = [i["cls"] for i in info]
    assert (res["unique"], res["by_density"], res["at_random"]) == (cls.count("N"), cls.count("U"), cls.count("R"))
    assert res["reads"] == len(info) and res["aligned"] == len(info) - cls.count(None) and res["suppressed"] == sum(i.get("suppressed", False) for i in info)
    assert res["records"] == want.count(b"\n") - (2 + len(case.names))
    return info


# ---------------------------------------------------------------------------------------------------- 1. mixture
def _mixture(d):
    """Three contigs.  A 200-nt segment in three copies (A and B on c1, C reverse-complemented on c3), each with private substitutions, so that a
    read over a copy's own substitution is unique and every other read of the segment has 2 or 3 hits.  A 60-nt segment in two copies on c2 with
    no unique read anywhere near: its reads are placed at random under mode u as well."""
    rng = np.random.RandomState(2024)
    c1, c2, c3 = (rng.randint(0, 4, n).astype(np.uint8) for n in (3000, 2500, 3500))
    seg = rng.randint(0, 4, 200).astype(np.uint8)
    cA, cB, cC = _snp(seg, [30, 130]), _snp(seg, [70, 170]), _snp(seg, [100])
    c1[500:700], c1[2000:2200], c3[1000:1200] = cA, cB, revcomp(cC)
    seg2 = rng.randint(0, 4, 60).astype(np.uint8)
    c2[300:360] = c2[1500:1560] = seg2
    reads, seen = [], set()

    def add(r, depth=None):
        if r.tobytes() not in seen:
            seen.add(r.tobytes())
            reads.append((r.copy(), int(rng.randint(1, 501)) if depth is None else depth))
    for o in range(0, 176, 3):                              # reads of the base segment: two or three hits, none over a substitution that is theirs alone
        L = int(rng.randint(18, 27))
        if o + L <= 200:
            add(seg[o:o + L] if o % 2 else revcomp(seg[o:o + L]))
    for copy, sites, depths in ((cA, (30, 130), (400, 500)), (cB, (170,), (3,)), (cC, (100,), (60,))):   # unique reads over the private substitutions
        for site, dp in zip(sites, depths):                 # (none over B's at 70: B weighs 0 for reads around there)
            for j in range(4):
                L = 18 + 2 * j
                o = site - 3 - 4 * j
                r = copy[o:o + L]
                add(revcomp(r) if j % 2 else r, dp + j)
    for lo, hi, dp in ((440, 482, 300), (700, 740, 200), (1950, 1982, 1), (2200, 2230, 2)):            # unique reads beside A (dense) and B (sparse)
        for o in range(lo, hi, 7):
            add(c1[o:o + 20] if o % 2 else revcomp(c1[o:o + 20]), dp)
    for o in range(950, 982, 6):                            # and beside C, on the minus strand
        add(revcomp(c3[o:o + 21]), 40)
    for o in range(0, 40, 4):                               # reads of the second family
        add(seg2[o:o + 20] if o % 8 else revcomp(seg2[o:o + 20]))
    near = ([(350, 850), (1850, 2350)], [(150, 510), (1350, 1710)], [(850, 1350)])
    while len(reads) < 290:                                 # unique reads elsewhere, none within 150 bases of a copy
        k = len(reads) % 3
        t = (c1, c2, c3)[k]
        L = int(rng.randint(18, 27))
        o = int(rng.randint(0, len(t) - L))
        if not any(lo <= o < hi for lo, hi in near[k]):
            add(t[o:o + L] if o % 2 else revcomp(t[o:o + L]))
    for _ in range(8):                                      # reads that align nowhere, one with an N, one with a substitution
        add(rng.randint(0, 4, 22).astype(np.uint8))
    n = c2[900:922].copy()
    n[7] = 4
    add(n)
    add(_snp(c2[1000:1024], [11]))
    order = rng.permutation(len(reads))
    return Case(d, [("c1", c1), ("c2", c2), ("c3", c3)], [reads[i] for i in order], vmax=1)


@pytest.fixture(scope="module")
def mixture(tmp_path_factory):
    return _mixture(tmp_path_factory.mktemp("place_mixture"))


def _mixture_guards(case):
    for v in (0, 1):
        for W in (0, 50):
            info = case.want(v, 50, W, 0, "u")[1]
            cls = [i["cls"] for i in info]
            assert min(cls.count("N"), cls.count("U"), cls.count("R")) >= 5, (v, W, cls.count("N"), cls.count("U"), cls.count("R"))
            assert cls.count(None) >= 5
    info = case.want(0, 50, 50, 0, "u")[1]
    assert any(i["cls"] == "U" and i["n"] == 3 and i["w"][0] > 0 and i["w"][1] == 0 and i["w"][2] > 0 for i in info)      # a zero between two weights
    assert len({i["idx"] for i in info if i["cls"] == "U"}) > 1 and len({i["idx"] for i in info if i["cls"] == "R"}) > 1
    assert {i["n"] for i in info if i["cls"] in ("U", "R")} >= {2, 3}
    # a unique read on the minus strand inside a window: taking the minus-strand unique reads away changes some weight
    exact = [[h for h in hs if h[3] == 0] for hs in case.hits]
    without_minus = [[] if len(e) == 1 and e[0][2] == 1 else hs for e, hs in zip(exact, case.hits)]
    info_plus = place(case.names, case.seqs, case.reads, without_minus, 0, 50, 50, 0, "u")[1]
    assert any(a["cls"] == "U" and a["w"] != b["w"] for a, b in zip(info, info_plus))
    assert case.want(0, 50, 50, 0, "u")[0] != case.want(0, 50, 50, 7, "u")[0] != case.want(0, 50, 0, 7, "u")[0]


def test_mixture_over_modes_mismatches_windows_and_seeds(gpu_ctx, mixture):
    _mixture_guards(mixture)
    gpu_ctx.align_index([mixture.ref])
    for mode in ("u", "r"):
        for v in (0, 1):
            for W in (0, 50):
                for seed in (0, 7):
                    for f in (False, True):
                        _check(gpu_ctx, mixture, v, 50, W, seed, mode, f)


# ---------------------------------------------------------------------------------------------------- 2. contig edges
def _edges(d):
    """Family E: c1's last 30 bases and c3[100:130].  Family F: c2's first 30 bases and c3[300:330].  Dense unique reads sit just before E's copy
    on c1 (across the join from F's copy at c2 POS 1) and just after F's copy on c2 (across the join from E's copy at the end of c1)."""
    rng = np.random.RandomState(77)
    c1, c2, c3 = (rng.randint(0, 4, n).astype(np.uint8) for n in (400, 500, 450))
    E, F = rng.randint(0, 4, 30).astype(np.uint8), rng.randint(0, 4, 30).astype(np.uint8)
    c1[370:400] = c3[100:130] = E
    c2[0:30] = c3[300:330] = F
    reads = [(E[0:20].copy(), 3), (E[8:30].copy(), 2), (revcomp(E[4:25]), 5), (F[0:20].copy(), 4), (F[10:30].copy(), 1), (revcomp(F[3:24]), 6)]
    for o in range(340, 366, 3):
        reads.append((c1[o:o + 19].copy(), 50))              # before E on c1; some reach into the copy and are still unique
    for o in range(30, 56, 3):
        reads.append((c2[o:o + 19].copy(), 70))              # after F on c2
    for o in (60, 140, 280, 340):
        reads.append((revcomp(c3[o:o + 20]), 9))             # on c3 beside its two copies
    return Case(d, [("c1", c1), ("c2", c2), ("c3", c3)], reads, vmax=0)


def _naive_weight(case, hit, L, W, upos):
    """the weight over the concatenation, ignoring contig ends: what the definition forbids"""
    start = [0]
    for s in case.seqs:
        start.append(start[-1] + len(s))
    g = start[hit[0]] + hit[1]
    return sum(dp for (t, p), dp in upos.items() if g - W <= start[t] + p - 1 <= g + L - 1 + W)


def test_windows_stop_at_contig_ends(gpu_ctx, tmp_path):
    case = _edges(tmp_path)
    sel = [[h for h in hs if h[3] == 0] for hs in case.hits]
    upos = {}
    for (q, r), s in zip(case.reads, sel):
        if len(s) == 1:
            upos[(s[0][0], s[0][1] + 1)] = upos.get((s[0][0], s[0][1] + 1), 0) + int(q.rsplit("_x", 1)[1])
    for W in (40, 10000):
        info = case.want(0, 50, W, 0, "u")[1]
        seen = set()
        for (q, r), s, i in zip(case.reads, sel, info):
            if len(s) > 1:
                assert i["cls"] == "U"
                for h, w in zip(sorted(s), i["w"]):
                    if _naive_weight(case, h, len(r), W, upos) > w:
                        seen.add("end of c1" if h[0] == 0 else "start of c2" if h[0] == 1 and h[1] < 30 else "other")
        assert {"end of c1", "start of c2"} <= seen, (W, seen)       # unique reads within W across both joins, and they weigh nothing
    assert any(h == (1, 0, 0, 0) for s in sel for h in s) and any(h[0] == 0 and h[1] + len(r) == 400 for (q, r), s in zip(case.reads, sel) for h in s)
    assert all(i["cls"] == "R" for i in case.want(0, 50, 0, 0, "u")[1] if i["n"] > 1)
    gpu_ctx.align_index([case.ref])
    for W in (0, 40, 10000):
        for seed in (0, 1, 2):
            _check(gpu_ctx, case, 0, 50, W, seed, "u")


# ---------------------------------------------------------------------------------------------------- 3. running-sum boundaries
def test_running_sum_boundaries(gpu_ctx, tmp_path):
    rng = np.random.RandomState(5)
    g = rng.randint(0, 4, 1500).astype(np.uint8)
    seg = rng.randint(0, 4, 24).astype(np.uint8)
    g[200:224] = g[700:724] = g[1200:1224] = seg
    reads = [(seg.copy(), 1), (g[180:200].copy(), 2), (g[690:712].copy(), 3), (g[1226:1246].copy(), 2)]
    case = Case(tmp_path, [("c", g)], reads, vmax=0)
    i0 = case.want(0, 50, 50, 0, "u")[1][0]
    assert i0["w"] == [2, 3, 2] and i0["wt"] == 7
    found = {}
    for seed in range(4096):
        found.setdefault(draw(case.reads[0][1], seed) % 7, seed)
    assert {1, 2, 4, 5} <= set(found)              # r = c_0 - 1, c_0, c_1 - 1, c_1 with c = (2, 5, 7)
    gpu_ctx.align_index([case.ref])
    for r, idx in ((1, 0), (2, 1), (4, 1), (5, 2), (0, 0), (6, 2)):
        info = _check(gpu_ctx, case, 0, 50, 50, found[r], "u")
        assert info[0]["r"] == r and info[0]["idx"] == idx


# ---------------------------------------------------------------------------------------------------- 4. 64 bits
def test_weights_past_2_32(gpu_ctx, tmp_path):
    rng = np.random.RandomState(64)
    g = rng.randint(0, 4, 7000).astype(np.uint8)
    seg = rng.randint(0, 4, 24).astype(np.uint8)
    g[4030:4054] = g[6000:6024] = seg
    reads = [(g[o:o + 20].copy(), 1) for o in range(0, 3600, 10)]                      # 360 unique reads of depth 1 before the two deep ones
    reads += [(g[4000:4020].copy(), 4000000000), (g[4000:4023].copy(), 4000000000)]     # two deep unique reads at one position
    reads += [(g[5980:6000].copy(), 3000000000), (seg.copy(), 9)]
    case = Case(tmp_path, [("c", g)], reads, vmax=0)
    info = case.want(0, 50, 50, 0, "u")[1]
    assert info[-1]["w"] == [8000000000, 3000000000] and info[-1]["wt"] > 2 ** 33 and [i["cls"] for i in info].count("N") == 363
    picks = {case.want(0, 50, 50, s, "u")[1][-1]["idx"] for s in range(8)}
    assert picks == {0, 1}
    gpu_ctx.align_index([case.ref])
    for seed in range(8):
        _check(gpu_ctx, case, 0, 50, 50, seed, "u")
    got = open(case.dir / "out.sam", "rb").read()
    assert b"\tXW:Z:8000000000/11000000000\n" in got or b"\tXW:Z:3000000000/11000000000\n" in got


def test_depth_rule_of_the_host_parser(gpu_ctx, tmp_path):
    """QNAMEs that do and do not carry a depth: the weights in XW show what the library's parser made of each."""
    rng = np.random.RandomState(33)
    g = rng.randint(0, 4, 2000).astype(np.uint8)
    seg = rng.randint(0, 4, 22).astype(np.uint8)
    g[300:322] = g[1300:1322] = seg
    _write_fasta(tmp_path / "g.fa", [("c", g)])
    named = [("m_r0_x3", seg), ("a_r1_x7", g[270:290]), ("a_r1_x", g[275:295]), ("a_x3_r1", g[330:350]), ("x_r1_x4294967296", g[335:356]),
             ("x_r1_x4294967295", g[1280:1300]), ("b_x3_x0012", g[1325:1345]), ("_x5", g[1330:1351]), ("x40", g[1335:1357]), ("c_r2_x0", g[1340:1360]),
             ("d_r3_x00000000000000000009", g[1345:1366]), ("e_r4_x99999999999999999999", g[1350:1372])]
    with open(tmp_path / "r.fa", "wb") as f:
        f.write(b"".join(b">%s\n%s\n" % (q.encode(), _letters(r)) for q, r in named))
    case = Case.__new__(Case)
    case.dir, case.ref, case.reads_path = tmp_path, str(tmp_path / "g.fa"), str(tmp_path / "r.fa")
    case.names, case.seqs = load_reference([case.ref])
    case.reads = load_reads(case.reads_path)
    case.hits = hits_of(case.seqs, case.reads, 0)
    info = case.want(0, 50, 50, 0, "u")[1]
    assert info[0]["w"] == [7 + 1 + 1 + 1, 4294967295 + 12 + 5 + 1 + 0 + 9 + 1] and all(i["cls"] == "N" for i in info[1:])
    gpu_ctx.align_index([case.ref])
    for seed in (0, 1):
        _check(gpu_ctx, case, 0, 50, 50, seed, "u")


# ---------------------------------------------------------------------------------------------------- 5. the -m boundary
def _cli(args, cwd):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.align"] + args, cwd=cwd, capture_output=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))


def test_m_boundary_on_a_tandem_array(gpu_ctx, tmp_path):
    rng = np.random.RandomState(40)
    g = rng.randint(0, 4, 3000).astype(np.uint8)
    unit = rng.randint(0, 4, 23).astype(np.uint8)
    g[1000:1000 + 23 * 40] = np.tile(unit, 40)
    reads = [(unit.copy(), 5), (g[985:1005].copy(), 30), (g[1000 + 23 * 40 - 6:1000 + 23 * 40 + 14].copy(), 11), (g[100:120].copy(), 2)]
    case = Case(tmp_path, [("c", g)], reads, vmax=0)
    info40, info39 = case.want(0, 40, 50, 0, "u")[1], case.want(0, 39, 50, 0, "u")[1]
    assert info40[0]["n"] == 40 and info40[0]["cls"] == "U" and info39[0]["cls"] is None and info39[0]["suppressed"]
    assert sum(w > 0 for w in info40[0]["w"]) >= 4 and info40[0]["w"][10] == 0
    gpu_ctx.align_index([case.ref])
    for seed in (0, 3):
        _check(gpu_ctx, case, 0, 40, 50, seed, "u")
        _check(gpu_ctx, case, 0, 39, 50, seed, "u")
        _check(gpu_ctx, case, 0, 39, 50, seed, "r", f=True)
    res, got40 = _run(gpu_ctx, case, 0, 40, 50, 0, "u")
    assert b"\tNH:i:40\tXY:Z:U\t" in got40 and res["suppressed"] == 0
    res, got39 = _run(gpu_ctx, case, 0, 39, 50, 0, "u")
    assert b"\tXM:i:40\n" in got39 and res["suppressed"] == 1
    # the command line without -m: M = 50
    r = _cli(["--place", "u", "-r", case.ref, case.reads_path], tmp_path)
    assert r.returncode == 0, r.stderr
    assert normalise_pg(open(case.reads_path + ".sam", "rb").read()) == case.want(0, 50, 50, 0, "u")[0] == got40
    assert "Placed: 3 unique, 1 by density, 0 at random, 0 suppressed\n" in r.stdout.decode()


# ---------------------------------------------------------------------------------------------------- 6. two batches, both routes of pass 2
def test_two_batches_resident_and_realigned(gpu_ctx, tmp_path):
    rng = np.random.RandomState(6)
    g = rng.randint(0, 4, 4000).astype(np.uint8)
    seg = rng.randint(0, 4, 25).astype(np.uint8)
    g[500:525] = g[2500:2525] = seg
    _write_fasta(tmp_path / "g.fa", [("c", g)])
    names, seqs = load_reference([str(tmp_path / "g.fa")])
    first = [(seg.copy(), 4), (g[100:121].copy(), 6), (revcomp(seg[2:24]), 1)]                       # batch 1: multi-mapped reads and a far unique read
    last = [(g[2530:2550].copy(), 17), (revcomp(g[2470:2492]), 2), (g[3000:3020].copy(), 1)]          # batch 2: the unique reads beside the second copy
    filler = b"N" * 1024
    gpu_ctx.align_index([str(tmp_path / "g.fa")])

    def write(path, lo_first, n_fill, with_last):
        with open(path, "wb") as f:
            k = 0
            for r, dp in (first if lo_first else []):
                f.write(b">S_r%d_x%d\n%s\n" % (k, dp, _letters(r)))
                k += 1
            f.write(b"".join(b">S_f%d_x1\n%s\n" % (j, filler) for j in range(n_fill)))
            for r, dp in (last if with_last else []):
                f.write(b">S_t%d_x%d\n%s\n" % (k, dp, _letters(r)))
                k += 1

    def run(path, cap):
        gpu_ctx.set_align_place_capacity(cap)
        try:
            res = gpu_ctx.align_reads(str(path), str(path) + ".sam", "x", v=2, k=20, m=50, filter_unmapped=True, place="u", window=50, seed=0)
        finally:
            gpu_ctx.set_align_place_capacity(0)
        return res, normalise_pg(open(str(path) + ".sam", "rb").read()), gpu_ctx.align_last_batches(), gpu_ctx.align_place_last_realigned()
    n_fill = 8400
    while True:
        write(tmp_path / "all.fa", True, n_fill, True)
        res, got, batches, realigned = run(tmp_path / "all.fa", 0)
        if batches >= 2:
            break
        n_fill += 2000
        assert n_fill <= 40000
    assert realigned == 0
    reads = load_reads(str(tmp_path / "all.fa"))
    hits = hits_of(seqs, reads, 2)
    want, info = place(names, seqs, reads, hits, 2, 50, 50, 0, "u", True)
    assert info[0]["cls"] == "U" and info[0]["w"] == [0, 19] and info[2]["cls"] == "U" and [i["cls"] for i in info[-3:]] == ["N", "N", "N"]
    assert got == want
    assert (res["unique"], res["by_density"], res["at_random"], res["unaligned"]) == (4, 2, 0, n_fill)
    res1, got1, batches1, realigned1 = run(tmp_path / "all.fa", 1)
    assert batches1 == batches and realigned1 >= 1 and got1 == want
    assert {k: v for k, v in res1.items() if k != "seconds"} == {k: v for k, v in res.items() if k != "seconds"}
    # the same reads as two files: each file stands alone, so the multi-mapped reads of the first see no unique read near either copy
    write(tmp_path / "a.fa", True, n_fill // 2, False)
    ra = load_reads(str(tmp_path / "a.fa"))
    want_a, info_a = place(names, seqs, ra, hits_of(seqs, ra, 2), 2, 50, 50, 0, "u", True)
    assert info_a[0]["cls"] == "R" and want_a.split(b"\n")[3] != want.split(b"\n")[3]
    res_a, got_a, _, _ = run(tmp_path / "a.fa", 0)
    assert got_a == want_a and res_a["at_random"] == 2


# ---------------------------------------------------------------------------------------------------- 7. mode 0
def test_mode_0_is_align_reads(gpu_ctx, mixture):
    import ctypes as C
    from mir_prefer_amd import capi
    gpu_ctx.align_index([mixture.ref])
    a, b = str(mixture.dir / "plain.sam"), str(mixture.dir / "mode0.sam")
    for k in (1, 20):
        for opts in (capi.AlignPlaceOpts(0, 50, 7), None):
            res = gpu_ctx.align_reads(mixture.reads_path, a, "x", v=1, k=k, m=0)
            st, sec = (C.c_int64 * 8)(), (C.c_double * 8)()
            rc = gpu_ctx.lib.mirp_align_reads_placed(gpu_ctx.h, os.fsencode(mixture.reads_path), os.fsencode(b), b"x", 1, k, 0, 0,
                                                     C.byref(opts) if opts is not None else None, st, sec)
            assert rc == 0
            assert open(a, "rb").read() == open(b, "rb").read()
            assert list(st) == [res["reads"], res["aligned"], res["unaligned"], res["suppressed"], res["records"], 0, 0, 0]
            assert open(a, "rb").read() == sam_bytes(mixture.names, mixture.seqs, mixture.reads, mixture.hits, 1, k, 0, False,
                                                     pg=b"@PG\tID:mir_prefer_amd.align\tCL:\"x\"\n")
    with pytest.raises(capi.MirpError):
        gpu_ctx.align_reads(mixture.reads_path, b, "x", v=0, k=20, m=0, place="u")            # a placed call needs m in 1..10000


# ---------------------------------------------------------------------------------------------------- 8. downstream
def test_placed_file_feeds_ingest_and_clusters(gpu_ctx, mixture, tmp_path):
    import shutil
    rp = str(tmp_path / "root.fa")
    shutil.copy(mixture.reads_path, rp)
    r = _cli(["--place", "u", "-v", "0", "-f", "-r", mixture.ref, rp], tmp_path)
    assert r.returncode == 0, r.stderr
    want, info = mixture.want(0, 50, 50, 0, "u", True)
    got = open(rp + ".sam", "rb").read()
    assert normalise_pg(got) == want
    tags = [ln.split(b"\tXY:Z:")[1][:1] for ln in got.splitlines() if b"\tXY:Z:" in ln]
    line = "Placed: %d unique, %d by density, %d at random, 0 suppressed\n" % (tags.count(b"N"), tags.count(b"U"), tags.count(b"R"))
    out = r.stdout.decode()
    assert line in out and out.index("Mapping file " + rp) < out.index(line) and min(tags.count(b"N"), tags.count(b"U"), tags.count(b"R")) >= 5
    aligned = sum(i["cls"] is not None for i in info)
    total_depth = sum(int(q.rsplit("_x", 1)[1]) for q, _ in mixture.reads)
    sums = []
    for path, records in ((rp + ".sam", aligned), (None, None)):
        if path is None:                                   # the same input with -k 20: a multi-mapped read counts at each of its places
            r = _cli(["-k", "20", "-v", "0", "-f", "-r", mixture.ref, rp], tmp_path)
            assert r.returncode == 0 and "Placed:" not in r.stdout.decode()
            path = rp + ".sam"
            records = open(path, "rb").read().count(b"\n") - 5
            assert records > aligned
        names, lens, samples, alns, segs, sec = gpu_ctx.ingest_sams([path])
        assert names == mixture.names and len(alns) == records
        clusters, counts, stats = gpu_ctx.cluster_scan(1, 75, lens, len(samples))
        assert len(clusters) > 3
        sums.append(int(clusters["reads"].sum()))
    assert sums[0] <= total_depth < sums[1]
