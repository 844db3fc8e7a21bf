"""GPU tests of `align --tail` (align_tail_kernels.hip, mirp_align_reads_tailed; DESIGN.md §12 "Tails"): whole .sam and .tails.tsv files against the
brute-force restatement of tests/tail_restatement.py, byte for byte.  The genome is a few kb; every test first asserts from the restatement alone
that its input holds the cases it names."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.place_restatement import depth_of
from tests.tail_restatement import tail_align
from tests.test_align_cpu import brute_hits, load_reads, load_reference, normalise_pg, revcomp
from tests.test_align_gpu import _letters, _write_fasta
from tests.test_align_long_gpu import _assert_no_record_twice, _first_batch, _first_diff

pytestmark = pytest.mark.gpu
STATS = ("reads", "aligned", "unaligned", "suppressed", "records", "tailed", "tail_suppressed")


def _other(code, step=1):
    """A base that differs from `code` (a code 0..3)."""
    return (int(code) + step) % 4


class World:
    """The genome of tests 1 to 5, 7 and 8 (three contigs over two files, about 5 kb), the labelled reads cut from it and their brute-force hits."""

    def __init__(self, d):
        rng = np.random.RandomState(4177)

        def rnd(n):
            return rng.randint(0, 4, n).astype(np.uint8)
        cA, cB, cC = rnd(2600), rnd(1500), rnd(1200)
        cA[600:640] = 4                                         # an N run
        cA[1200] = 4                                            # one ambiguous base
        unit = rnd(25)
        cA[1500:2250] = np.tile(unit, 30)                       # a 30-copy tandem array
        cA[1499], cA[2250] = _other(unit[24]), _other(unit[0])  # exactly 30 copies
        X = rnd(20)                                             # one templated part at three loci, followed by G / TG / TTC
        cA[2300:2321] = np.concatenate([X, [2]])
        cB[300:322] = np.concatenate([X, [3, 2]])
        cB[700:723] = np.concatenate([X, [3, 3, 1]])
        cB[-1] = 2                                              # the contig before the A's ends in G
        cC[:10] = 0                                             # the join cB | cC: the keys of cB's last positions are padded with A, and cC begins AAAAAAAAAA
        cC[10] = 1
        pal = rnd(12)
        P = np.concatenate([pal, revcomp(pal)])                 # its own reverse complement: + and - hit at the same offset
        cC[400:424] = P
        cC[399], cC[424] = 1, 2                                 # not A before, not T after: both strands are maximal for the tail T
        self.seq_letters = [_letters(cA), _letters(cB), _letters(cC)]
        la = bytearray(self.seq_letters[0])
        la[1200:1201] = b"R"
        la[100:160] = bytes(la[100:160]).lower()
        self.files = [str(d / "g1.fa"), str(d / "g2.fa")]
        _write_fasta(d / "g1.fa", [("cA", bytes(la)), ("cB", self.seq_letters[1])])
        _write_fasta(d / "g2.fa", [("cC", self.seq_letters[2])], width=71)
        self.names, self.seqs = load_reference(self.files)
        assert self.names == ["cA", "cB", "cC"] and [len(s) for s in self.seqs] == [2600, 1500, 1200]
        assert (self.seqs[0] == cA).all() and (self.seqs[1] == cB).all() and (self.seqs[2] == cC).all()
        R, label = [], []

        def add(name, codes):
            R.append(np.asarray(codes, dtype=np.uint8))
            label.append(name)

        def plus(g, p, n, tail):
            return np.concatenate([g[p:p + n], np.asarray(tail, dtype=np.uint8)])

        def minus(g, p, n, tail):                               # templated part g[p : p + n] on -, tail as sequenced
            return np.concatenate([revcomp(g[p:p + n]), np.asarray(tail, dtype=np.uint8)])
        # ---- 1. every length 12..40 with every tail length 1..8, alternating strands and U / A tails; cut from cB and cC away from the planted parts
        k = 0
        for L in range(12, 41):
            for t in range(1, 9):
                if L - t < 4:
                    continue
                g = (cB, cC)[k % 2]
                p = int(rng.randint(730, len(g) - 60))
                letter = 3 if k % 3 else 0                      # U or A; the other one where this one would continue the match
                if (L + t) % 2:
                    add("mix", minus(g, p, L - t, [letter if 3 - letter != g[p - 1] else 3 - letter] * t))
                else:
                    add("mix", plus(g, p, L - t, [letter if letter != g[p + L - t] else 3 - letter] * t))
                k += 1
        add("tie", plus(cC, 400, 24, [3]))
        # ---- 2. maximal extension
        p = 900
        add("shrink1", plus(cB, p, 20, [cB[p + 20], _other(cB[p + 21])]))                                # the tail's first letter is templated
        add("shrink2", plus(cB, p + 40, 20, [cB[p + 60], cB[p + 61], _other(cB[p + 62])]))               # its first two letters
        add("shrink1-", minus(cB, p + 80, 20, [3 - cB[p + 79], 3 - _other(cB[p + 78])]))
        add("exact", cB[p + 120:p + 144].copy())                                                        # a tail that extends to L: an end-to-end hit
        add("exact-", revcomp(cB[p + 160:p + 184]))
        add("contig_end+", plus(cB, 1480, 20, [1, 1]))
        add("contig_start-", minus(cB, 0, 20, [2, 2]))
        add("genome_first-", minus(cA, 0, 20, [3, 3, 3]))
        add("genome_last+", plus(cC, 1180, 20, [0, 0, 0]))
        add("amb+", plus(cA, 1180, 20, [3, 3]))                                                          # the next genome base is R
        add("amb-", minus(cA, 1201, 20, [0, 0]))
        add("nrun+", plus(cA, 580, 20, [0, 3]))
        add("nrun-", minus(cA, 640, 20, [3, 0]))
        add("join+", np.concatenate([cB[-18:], cC[:3]]))                                                 # spans cB | cC: 18 templated, AAA clipped
        add("join-", revcomp(np.concatenate([cB[-3:], cC[:18]])))                                        # 18 templated in cC, revcomp(cB's end) clipped
        add("join_polyA", plus(cB, 1480, 20, [0, 0, 0, 0]))                                              # a poly-A tail where A's follow behind the join
        add("join_padded", np.concatenate([cB[-10:], [0] * 6, [1, 1]]))                                  # its seed equals a padded key: no hit
        add("n_in_tail", plus(cB, p + 200, 20, [_other(cB[p + 220]), 4]))
        add("n_in_tail2", plus(cB, p + 230, 20, [4, 3, 4]))
        add("n_in_tail-", minus(cB, p + 260, 20, [4, 0]))
        bad = plus(cB, p + 290, 20, [3, 3])
        bad[5] = 4
        add("n_in_templated", bad)
        # ---- 3. strata and multiplicity
        add("three_loci", np.concatenate([X, [3, 3, 3, 3]]))
        two = np.concatenate([unit, unit])
        add("tandem", np.concatenate([two[3:25], [_other(two[25], 2), _other(two[26], 2)]]))
        add("tandem-", np.concatenate([revcomp(two[5:27]), [3 - _other(two[4]), 3 - _other(two[3], 2)]]))
        # ---- 4. one substitution: within T = 4 of the 3' end, and far from it
        for name, pos in (("sub_near", 22), ("sub_far", 9)):
            for strand in (0, 1):
                o = cB[p + 330 + 40 * strand:p + 354 + 40 * strand].copy()
                o = revcomp(o) if strand else o
                o[pos] = _other(o[pos])
                add(name + "+-"[strand], o)
        add("random", rnd(30))
        self.label = label
        self.idx = {n: i for i, n in enumerate(label) if n != "mix"}
        self.path = str(d / "S1.fa")
        depths = [1 + (j * 7) % 13 for j in range(len(R))]
        with open(self.path, "wb") as f:
            for j, r in enumerate(R):
                q = b"S1_r%d_x%d" % (j, depths[j])
                s = _letters(r, rng, lower=0.1)
                f.write(b">" + q + b"\n" + (s[:7] + b"\n" + s[7:] if j % 5 == 0 else s) + b"\n")
        self.reads = load_reads(self.path)
        assert len(self.reads) == len(R) and all((a[1] == b).all() for a, b in zip(self.reads, R))
        self.hits = brute_hits(self.seqs, self.reads, vmax=3)
        self.indexed = None

    def expected(self, v=0, k=20, m=0, f=False, T=4, M=16, trim=False):
        return tail_align(self.names, self.seqs, self.reads, self.hits, v, k, m, f, T, M, trim)

    def index(self, ctx):
        ctx.align_index(self.files)

    def check(self, ctx, tmp_path, v=0, k=20, m=0, f=False, T=4, M=16, trim=False, want=None):
        """One device call against the restatement: both files byte for byte, no record twice, every statistic."""
        out = str(tmp_path / "out.sam")
        res = ctx.align_reads(self.path, out, "x", v=v, k=k, m=m, filter_unmapped=f, tail=T, tail_min=M, tail_trim=trim)
        got = normalise_pg(open(out, "rb").read())
        got_tsv = open(out + ".tails.tsv", "rb").read()
        what = dict(v=v, k=k, m=m, f=f, T=T, M=M, trim=trim)
        _assert_no_record_twice(got, what)
        sam, tsv, st, info = want or self.expected(v, k, m, f, T, M, trim)
        assert got == sam, (what, _first_diff(got, sam))
        assert got_tsv == tsv, (what, _first_diff(got_tsv, tsv))
        assert {s: res[s] for s in STATS} == st, what
        assert len(res["seconds"]) == 7
        return res, got, got_tsv, info


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("tail_world"))


def _rec(sam, q):
    return [ln.split("\t") for ln in sam.decode().splitlines() if ln.startswith(q + "\t")]


# ---------------------------------------------------------------------------------------------------- 1. every tail length on both strands
@pytest.mark.parametrize("T", [1, 4, 8])
@pytest.mark.parametrize("M", [12, 13, 16, 17, 20])
def test_every_tail_length_on_both_strands(gpu_ctx, world, tmp_path, M, T):
    want = world.expected(T=T, M=M)
    info = want[3]
    tailed = [(i["t"], i["hits"][0][2]) for i in info if i and not i["suppressed"]]
    assert {(t, s) for t in range(1, T + 1) for s in (0, 1)} <= set(tailed)                      # every t in 1..T on + and on -
    lens = {len(r) for (_, r), i in zip(world.reads, info) if i}
    assert M + 1 in lens and max(lens) == 40 and M not in lens                                    # L = M + 1 is searched, L = M is not
    assert any(len(r) == M for _, r in world.reads)
    if T > 1:                                                                                     # L - M < T: a tail of at most L - M letters
        assert any(i and len(r) - M < T and i["t"] == len(r) - M for (_, r), i in zip(world.reads, info))
    assert all(i["t"] <= min(T, len(r) - M) for (_, r), i in zip(world.reads, info) if i)
    tie = info[world.idx["tie"]]
    assert tie and [h[1:3] for h in tie["hits"]] == [(400, 0), (400, 1)] and tie["t"] == 1        # + and - tie at one offset
    assert len(world.reads[world.idx["tie"]][1]) - 1 >= M
    world.index(gpu_ctx)
    world.check(gpu_ctx, tmp_path, T=T, M=M, want=want)


# ---------------------------------------------------------------------------------------------------- 2. maximal extension
def test_maximal_extension(gpu_ctx, world, tmp_path):
    want = world.expected(T=4, M=16)
    sam, tsv, st, info = want
    I = lambda n: info[world.idx[n]]                                                              # noqa: E731
    q = lambda n: world.reads[world.idx[n]][0]                                                    # noqa: E731
    assert I("shrink1")["t"] == 1 and I("shrink2")["t"] == 1 and I("shrink1-")["t"] == 1          # the stratum moved, the tail shrank
    assert I("shrink1-")["hits"][0][2] == 1
    for n, flag in (("exact", "0"), ("exact-", "16")):                                            # the end-to-end pass reports them
        assert I(n) is None and _rec(sam, q(n))[0][1] == flag and _rec(sam, q(n))[0][5] == "24M"
    assert I("contig_end+")["hits"] == [(1, 1480, 0, 20)] and I("contig_start-")["hits"] == [(1, 0, 1, 20)]
    assert I("genome_first-")["hits"] == [(0, 0, 1, 20)] and I("genome_last+")["hits"] == [(2, 1180, 0, 20)]
    assert I("amb+")["hits"] == [(0, 1180, 0, 20)] and I("amb-")["hits"] == [(0, 1201, 1, 20)]
    assert I("nrun+")["hits"] == [(0, 580, 0, 20)] and I("nrun-")["hits"] == [(0, 640, 1, 20)]
    assert I("join+")["hits"] == [(1, 1482, 0, 18)] and _rec(sam, q("join+"))[0][-1] == "XT:Z:AAA"
    assert I("join-")["hits"] == [(2, 0, 1, 18)] and _rec(sam, q("join-"))[0][5] == "3S18M"
    assert I("join_polyA")["hits"] == [(1, 1480, 0, 20)] and _rec(sam, q("join_polyA"))[0][-1] == "XT:Z:AAAA"
    assert I("join_padded") is None and _rec(sam, q("join_padded"))[0][1] == "4"
    assert _rec(sam, q("n_in_tail"))[0][-1] == "XT:Z:%sN" % "ACGT"[_other(world.seqs[1][1120])] and _rec(sam, q("n_in_tail2"))[0][-1] == "XT:Z:NTN"
    assert _rec(sam, q("n_in_tail-"))[0][-1] == "XT:Z:NA" and _rec(sam, q("n_in_tail-"))[0][9].startswith("TN")
    assert I("n_in_templated") is None and _rec(sam, q("n_in_templated"))[0][-1] == "XM:i:0"
    assert b"N\t" in tsv
    world.index(gpu_ctx)
    world.check(gpu_ctx, tmp_path, T=4, M=16, want=want)
    _, _, _, i2 = world.check(gpu_ctx, tmp_path, T=2, M=16)                                       # a smaller T: the same strata where they are in reach
    assert i2[world.idx["shrink2"]]["t"] == 1 and i2[world.idx["join+"]] is None and i2[world.idx["join_polyA"]] is None


# ---------------------------------------------------------------------------------------------------- 3. strata and multiplicity
def test_strata_and_multiplicity(gpu_ctx, world, tmp_path):
    base = world.expected(T=4, M=16, k=10 ** 6)
    info = base[3]
    three = info[world.idx["three_loci"]]
    assert three["t"] == 2 and three["hits"] == [(1, 700, 0, 22)]                                 # loci with m = 20, 21, 22: only the longest
    from tests.tail_restatement import tailed_hits
    assert sorted(h[3] for h in tailed_hits(world.seqs, world.reads[world.idx["three_loci"]][1], 4, 16)) == [20, 21, 22]
    for n, strand in (("tandem", 0), ("tandem-", 1)):
        t = info[world.idx[n]]
        assert t["t"] == 2 and len(t["hits"]) in (29, 30) and all(h[2] == strand for h in t["hits"])
    world.index(gpu_ctx)
    for k in (1, 5, 10 ** 6):
        res, got, _, _ = world.check(gpu_ctx, tmp_path, T=4, M=16, k=k)
        q = world.reads[world.idx["tandem"]][0]
        assert len(_rec(got, q)) == min(k, len(info[world.idx["tandem"]]["hits"]))
    for f in (False, True):
        want = world.expected(T=4, M=16, m=3, f=f)
        assert want[3][world.idx["tandem"]]["suppressed"] and want[3][world.idx["tandem-"]]["suppressed"]
        assert want[2]["tail_suppressed"] >= 2 and want[2]["suppressed"] >= want[2]["tail_suppressed"]
        res, got, tsv, _ = world.check(gpu_ctx, tmp_path, T=4, M=16, m=3, f=f, want=want)
        q = world.reads[world.idx["tandem"]][0]
        assert (_rec(got, q) == []) if f else (_rec(got, q)[0][-1] == "XM:i:4" and _rec(got, q)[0][1] == "4")
        assert res["tail_suppressed"] == want[2]["tail_suppressed"] and res["suppressed"] == want[2]["suppressed"]


# ---------------------------------------------------------------------------------------------------- 4. interaction with -v
def test_interaction_with_v(gpu_ctx, world, tmp_path):
    world.index(gpu_ctx)
    for v in (0, 1, 2, 3):
        want = world.expected(v=v, T=4, M=16)
        sam, _, st, info = want
        for s, flag in (("+", "0"), ("-", "16")):
            near, far = world.idx["sub_near" + s], world.idx["sub_far" + s]
            rn, rf = _rec(sam, world.reads[near][0]), _rec(sam, world.reads[far][0])
            if v == 0:                                          # tailed only where the substitution sits within T of the 3' end
                assert info[near] and info[near]["t"] == 2 and rn[0][1] == flag and info[far] is None and rf[0][1] == "4"
            else:                                               # a plain mismatch hit, never re-interpreted
                assert info[near] is None and info[far] is None and rn[0][11] == rf[0][11] == "XA:i:1" and "XT:Z:" not in "\t".join(rn[0])
        res, _, _, _ = world.check(gpu_ctx, tmp_path, v=v, T=4, M=16, want=want)
        plain = res["aligned"] - res["tailed"]                  # `aligned` includes the tailed reads
        assert plain + res["tailed"] + res["unaligned"] == res["reads"] and res["suppressed"] == 0
        assert res["tailed"] == st["tailed"] > 0 and plain == st["aligned"] - st["tailed"] > 0 and res["unaligned"] == st["unaligned"] > 0


# ---------------------------------------------------------------------------------------------------- 5. --tail-trim
def test_tail_trim(gpu_ctx, world, tmp_path):
    world.index(gpu_ctx)
    _, clip, clip_tsv, info = world.check(gpu_ctx, tmp_path, T=4, M=16)
    _, trim, trim_tsv, _ = world.check(gpu_ctx, tmp_path, T=4, M=16, trim=True)
    assert trim_tsv == clip_tsv
    a, b = clip.decode().splitlines(), trim.decode().splitlines()
    assert len(a) == len(b)
    differ = 0
    for x, y in zip(a, b):
        fx, fy = x.split("\t"), y.split("\t")
        assert [f for i, f in enumerate(fx) if i not in (5, 9, 10)] == [f for i, f in enumerate(fy) if i not in (5, 9, 10)]
        if x != y:
            differ += 1
            m = int(fy[5][:-1])
            assert fx[-1].startswith("XT:Z:") and fy[5] == "%dM" % m and len(fy[9]) == len(fy[10]) == m
            assert fy[9] == (fx[9][:m] if fx[1] == "0" else fx[9][-m:])
    assert differ == sum(len(i["hits"][:20]) for i in info if i and not i["suppressed"]) > 100


# ---------------------------------------------------------------------------------------------------- 6. batches and pieces
def test_two_batches_and_text_pieces(gpu_ctx, tmp_path):
    rng = np.random.RandomState(977)
    g1, g2 = rng.randint(0, 4, 6000).astype(np.uint8), rng.randint(0, 4, 4000).astype(np.uint8)
    seg = rng.randint(0, 4, 1200).astype(np.uint8)
    g1[500:1700] = g1[3000:4200] = g2[1000:2200] = seg                   # three copies
    _write_fasta(tmp_path / "g.fa", [("c1", _letters(g1)), ("c2", _letters(g2))], width=80)
    names, seqs = load_reference([str(tmp_path / "g.fa")])

    def miss(g, lo, hi):                                                 # letters that all differ from g[lo : hi]
        return np.array([_other(x, 1 + i % 3) for i, x in enumerate(g[lo:hi])], dtype=np.uint8)
    T = {
        "tail+": np.concatenate([g1[1800:2820], miss(g1, 2820, 2824)]),
        "tail-": np.concatenate([revcomp(g2[2400:3420]), revcomp(miss(g2, 2396, 2400))]),
        "tail_supp": np.concatenate([seg[100:1120], miss(seg, 1120, 1124)]),
        "tail_supp-": np.concatenate([revcomp(seg[50:1070]), revcomp(miss(seg, 46, 50))]),
        "plain+": g1[4300:5324].copy(),
        "plain-": revcomp(g2[2900:3924]),
        "plain_supp": seg[20:1044].copy(),
        "random": rng.randint(0, 4, 1024).astype(np.uint8),
    }
    kinds = list(T)
    templates = [("T%d" % j, T[n]) for j, n in enumerate(kinds)]
    assert all(len(r) == 1024 for _, r in templates)
    hits = brute_hits(seqs, templates, vmax=3)
    v, k, m, TT, M = 2, 20, 2, 4, 16
    sam_t, _, _, info = tail_align(names, seqs, templates, hits, v, k, m, False, TT, M)
    ti = dict(zip(kinds, info))
    assert ti["tail+"]["t"] == 4 and ti["tail+"]["hits"] == [(0, 1800, 0, 1020)] and ti["tail-"]["hits"] == [(1, 2400, 1, 1020)]
    assert ti["tail_supp"]["suppressed"] and len(ti["tail_supp"]["hits"]) == 3 and ti["tail_supp-"]["suppressed"] and ti["tail_supp-"]["hits"][0][2] == 1
    assert ti["plain+"] is None and ti["plain-"] is None and ti["plain_supp"] is None and ti["random"] is None
    per = [[] for _ in kinds]
    for ln in sam_t.split(b"\n")[4:-1]:
        qn_, rest = ln.split(b"\t", 1)
        per[int(qn_[1:])].append(b"\t" + rest + b"\n")
    assert all(per) and per[kinds.index("plain_supp")][0].endswith(b"XM:i:3\n") and per[kinds.index("random")][0].endswith(b"XM:i:0\n")
    head = b"".join(ln + b"\n" for ln in sam_t.split(b"\n")[:4])
    gpu_ctx.align_index([str(tmp_path / "g.fa")])
    count = 8400
    s = _first_batch(gpu_ctx, tmp_path, [1024] * count)                  # every read has 1,024 nt: the split does not depend on their order
    assert 3 <= s <= count - 3
    order = [j % len(kinds) for j in range(count)]
    around = [kinds.index(n) for n in ("tail+", "tail_supp", "tail-")]
    order[s - 3:s + 3] = around + around                                 # a tailed read, a suppressed one and one on - on each side of the split
    qn = [b"S_r%d_x%d" % (j, 1 + j % 7) for j in range(count)]
    qn[s - 3] = b"S_r%d_x99999999999" % (s - 3)                          # a tailed read with an oversized depth: it counts 1
    text = [_letters(r) for _, r in templates]

    def write(path, lo, hi):
        with open(path, "wb") as f:
            f.write(b"".join(b">%s\n%s\n" % (qn[j], text[order[j]]) for j in range(lo, hi)))

    def want_for(lo, hi):
        recs = b"".join(qn[j] + ln for j in range(lo, hi) for ln in per[order[j]])
        table = {}
        for j in range(lo, hi):
            i = info[order[j]]
            if i and not i["suppressed"]:
                tail = _letters(templates[order[j]][1][-i["t"]:]).decode()
                row = table.setdefault(tail, [0, 0])
                row[0] += 1
                row[1] += depth_of(qn[j].decode())
        return head + recs, table

    def parse_tsv(data):
        lines = data.decode().splitlines()
        assert lines[0] == "tail\tlength\treads\tdepth"
        rows = [ln.split("\t") for ln in lines[1:]]
        assert all(len(r[0]) == int(r[1]) for r in rows)
        return {r[0]: [int(r[2]), int(r[3])] for r in rows}

    def run(path):
        res = gpu_ctx.align_reads(str(path), str(path) + ".sam", "x", v=v, k=k, m=m, tail=TT, tail_min=M)
        return res, normalise_pg(open(str(path) + ".sam", "rb").read()), open(str(path) + ".sam.tails.tsv", "rb").read()
    write(tmp_path / "all.fa", 0, count)
    res, got, got_tsv = run(tmp_path / "all.fa")
    assert gpu_ctx.align_last_batches() == 2
    want, table = want_for(0, count)
    assert got == want, _first_diff(got, want)
    assert parse_tsv(got_tsv) == table and len(table) == 2
    n_of = lambda name: sum(kinds[j] == name for j in order)             # noqa: E731
    assert res["tailed"] == n_of("tail+") + n_of("tail-") and res["tail_suppressed"] == n_of("tail_supp") + n_of("tail_supp-")
    assert res["suppressed"] == res["tail_suppressed"] + n_of("plain_supp") and res["unaligned"] == n_of("random")
    assert res["aligned"] == res["tailed"] + n_of("plain+") + n_of("plain-") and res["reads"] == count
    # ---- the same reads cut into two files elsewhere: the same records, and the two summaries add up to the file's
    cutat = count // 3
    assert abs(cutat - s) > 100
    parts, total = [], {}
    for name, lo, hi in (("a.fa", 0, cutat), ("b.fa", cutat, count)):
        write(tmp_path / name, lo, hi)
        _, g, t = run(tmp_path / name)
        assert gpu_ctx.align_last_batches() == 1 and g.startswith(head)
        parts.append(g[len(head):])
        for tl, (n, d) in parse_tsv(t).items():
            row = total.setdefault(tl, [0, 0])
            row[0] += n
            row[1] += d
    assert head + b"".join(parts) == want and total == table
    # ---- small text pieces: the same bytes
    gpu_ctx.set_text_piece(4096)
    try:
        _, got2, tsv2 = run(tmp_path / "a.fa")
        pieces = gpu_ctx.text_pieces_last()
    finally:
        gpu_ctx.set_text_piece(0)
    assert got2 == head + parts[0] and tsv2 == open(str(tmp_path / "a.fa") + ".sam.tails.tsv", "rb").read() and pieces > 1


# ---------------------------------------------------------------------------------------------------- 7. off means off
def test_off_means_off(gpu_ctx, world, tmp_path, capsys):
    from mir_prefer_amd import align, capi
    world.index(gpu_ctx)
    plain = str(tmp_path / "plain.sam")
    res0 = gpu_ctx.align_reads(world.path, plain, "x", v=1, k=5, m=7)                              # mirp_align_reads
    ref = open(plain, "rb").read()
    sam, none, st, _ = world.expected(v=1, k=5, m=7, T=0)
    assert none is None and normalise_pg(ref) == sam
    out = str(tmp_path / "off.sam")
    res = gpu_ctx.align_reads(world.path, out, "x", v=1, k=5, m=7, tail=0, tail_min=16, tail_trim=True, tails_path=str(tmp_path / "never.tsv"))
    assert open(out, "rb").read() == ref and {s: res[s] for s in STATS[:5]} == {s: res0[s] for s in STATS[:5]}
    # the entry point itself with max_tail = 0 and with no options
    for opts in (C.byref(capi.AlignTailOpts(0, 5, 9, 0)), None):
        os.remove(out)
        stats, sec = (C.c_int64 * 7)(), (C.c_double * 7)()
        rc = gpu_ctx.lib.mirp_align_reads_tailed(gpu_ctx.h, os.fsencode(world.path), os.fsencode(out), os.fsencode(str(tmp_path / "never.tsv")), b"x",
                                                 1, 5, 7, 0, opts, stats, sec)
        assert rc == 0 and open(out, "rb").read() == ref and list(stats)[:5] == [res0[s] for s in STATS[:5]] and list(stats)[5:] == [0, 0]
    assert not (tmp_path / "never.tsv").exists() and not os.path.exists(out + ".tails.tsv") and not os.path.exists(plain + ".tails.tsv")
    # options out of range are refused before anything is opened
    for bad in ((9, 16, 0), (-1, 16, 0), (4, 11, 0), (4, 1025, 0), (4, 16, 2)):
        stats, sec = (C.c_int64 * 7)(), (C.c_double * 7)()
        rc = gpu_ctx.lib.mirp_align_reads_tailed(gpu_ctx.h, os.fsencode(world.path), os.fsencode(str(tmp_path / "bad.sam")),
                                                 os.fsencode(str(tmp_path / "bad.tsv")), b"x", 0, 20, 0, 0, C.byref(capi.AlignTailOpts(*bad, 0)), stats, sec)
        assert rc == -1 and not (tmp_path / "bad.sam").exists() and not (tmp_path / "bad.tsv").exists()
    # the command: without --tail the same bytes and no summary; with it the summary next to the .sam and the Tailed: line
    reads = str(tmp_path / "S1.fa")
    open(reads, "wb").write(open(world.path, "rb").read())
    argv = ["-v", "1", "-k", "5", "-m", "7"] + [a for f in world.files for a in ("-r", f)] + [reads]
    assert align.main(argv) == 0
    assert normalise_pg(open(reads + ".sam", "rb").read()) == normalise_pg(ref) and not os.path.exists(reads + ".sam.tails.tsv")
    assert "Tailed:" not in capsys.readouterr().out
    sam, tsv, st, _ = world.expected(v=0, k=5, m=7, T=4, M=16)
    assert align.main(["--tail", "4", "-k", "5", "-m", "7"] + argv[6:]) == 0
    assert normalise_pg(open(reads + ".sam", "rb").read()) == sam and open(reads + ".sam.tails.tsv", "rb").read() == tsv
    assert "Tailed: %d reads, %d suppressed\n" % (st["tailed"], st["tail_suppressed"]) in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- 8. downstream
def test_trimmed_sam_through_the_ingest(gpu_ctx, world, tmp_path):
    world.index(gpu_ctx)
    sam, tsv, st, info = world.expected(T=4, M=16, trim=True, f=True)
    out = str(tmp_path / "S1.sam")
    gpu_ctx.align_reads(world.path, out, "x", filter_unmapped=True, tail=4, tail_min=16, tail_trim=True)
    assert normalise_pg(open(out, "rb").read()) == sam
    names, lens, samples, alns, segs, _ = gpu_ctx.ingest_sams([out])
    assert names == world.names and list(lens) == [len(s) for s in world.seqs] and samples == ["S1"] and len(segs) == 0
    want = []
    for (q, r), hs, i in zip(world.reads, world.hits, info):
        if i is None:
            want += [(h[0], h[1] + 1, len(r), h[2], depth_of(q)) for h in hs if h[3] == 0][:20]
        elif not i["suppressed"]:
            want += [(h[0], h[1] + 1, h[3], h[2], depth_of(q)) for h in i["hits"][:20]]
    assert st["tailed"] > 100 and len(want) == st["records"] == len(alns)                        # one plain record per SAM record
    got = [(int(a["tid"]), int(a["pos"]), int(a["len"]), int(a["strand"]), int(a["depth"])) for a in alns]
    assert sorted(got) == sorted(want)
