"""CPU tests of the phased siRNA (PHAS) loci: a plain-Python dict restatement and a numpy restatement of the whole TSV agree on
seeded inputs; the exact p-value against brute-force enumeration and the hand values of §15; the kmin table against a direct scan; hand-made
loci; and the option errors of the command line, which exit 2 without opening a device."""
import itertools
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd import phasing
from mir_prefer_amd.synth import ALN_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"contig\tstart\tend\twindows\tbest_start\tn\tk\tpvalue\tphased_reads\twindow_reads\n"


# ---------------------------------------------------------------------------------------------------- restatements
def p_direct(n, k, m, L):
    S, G = 2 * m * L, 2 * m
    return Fraction(sum(math.comb(G, j) * math.comb(S - G, n - j) for j in range(k, min(n, G) + 1)), math.comb(S, n))


def restate_plain(alns, names, lens, L=21, m=10, alpha=Fraction(1, 1000), K=3, D=1):
    """The definition of §15 word by word with dicts: units, anchors, windows, the exact test, the merge and the TSV."""
    units = {}
    for r in alns.tolist():
        tid, pos, depth, ln, strand = r[0], r[1], r[2], r[3], r[4]
        if ln == L:
            u = (tid, strand, pos + 2 if strand else pos)
            units[u] = units.get(u, 0) + depth
    units = {u: a for u, a in units.items() if a >= D}
    passing = []
    for tid, x in sorted({(u[0], u[2]) for u in units}):
        n = k = ph = rd = 0
        for s in (0, 1):
            for c in range(x, x + m * L):
                a = units.get((tid, s, c))
                if a is not None:
                    n += 1
                    rd += a
                    if (c - x) % L == 0:
                        k += 1
                        ph += a
        p = p_direct(n, k, m, L)
        if k >= K and p <= alpha:
            passing.append((tid, x, n, k, ph, rd, p))
    loci = []
    for w in passing:
        end = min(w[1] + m * L - 1, int(lens[w[0]]))
        if loci and loci[-1]["tid"] == w[0] and w[1] <= loci[-1]["end"]:
            lc = loci[-1]
            lc["end"] = max(lc["end"], end)
            lc["wins"].append(w)
        else:
            loci.append({"tid": w[0], "start": w[1], "end": end, "wins": [w]})
    out = [HEADER]
    for lc in loci:
        b = min(lc["wins"], key=lambda w: (w[6], w[1]))
        out.append(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\n" % (names[lc["tid"]].encode(), lc["start"], lc["end"], len(lc["wins"]), b[1], b[2], b[3],
                                                                 (b"%.3e" % float(b[6])), b[4], b[5]))
    return b"".join(out)


def windows_numpy(alns, L=21, m=10, alpha=Fraction(1, 1000), K=3, D=1, kmin=None):
    """Passing windows (tid, start, n, k, phased_reads, window_reads) from sorted record arrays, vectorised: unit keys tid << 32 | c per strand,
    searchsorted ranges and prefix sums for n, searchsorted membership for k."""
    a = alns[(alns["len"] == L) & (alns["pos"] >= 0)]
    streams = []
    for s in (0, 1):
        r = a[a["strand"] == s]
        key = (r["tid"].astype(np.int64) << 32) + r["pos"].astype(np.int64) + 2 * s
        order = np.argsort(key, kind="stable")
        key, dep = key[order], r["depth"].astype(np.int64)[order]
        if len(key):
            head = np.concatenate([[True], key[1:] != key[:-1]])
            starts = np.flatnonzero(head)
            ukey, ab = key[starts], np.add.reduceat(dep, starts)
        else:
            ukey, ab = key, dep
        keep = ab >= D
        ukey, ab = ukey[keep], ab[keep]
        streams.append((ukey, ab, np.concatenate([[0], np.cumsum(ab)])))
    anchors = np.union1d(streams[0][0], streams[1][0])
    n = np.zeros(len(anchors), np.int64)
    k = np.zeros(len(anchors), np.int64)
    ph = np.zeros(len(anchors), np.int64)
    rd = np.zeros(len(anchors), np.int64)
    for ukey, ab, P in streams:
        lo, hi = np.searchsorted(ukey, anchors), np.searchsorted(ukey, anchors + m * L)
        n += hi - lo
        rd += P[hi] - P[lo]
        for j in range(m):
            t = anchors + j * L
            i = np.searchsorted(ukey, t)
            ic = np.minimum(i, max(len(ukey) - 1, 0))
            hit = (i < len(ukey)) & (ukey[ic] == t) if len(ukey) else np.zeros(len(t), bool)
            k += hit
            ph += np.where(hit, ab[ic] if len(ukey) else 0, 0)
    if kmin is None:
        kmin = phasing.Hypergeom(m, L).kmin(alpha)
    ok = k >= np.maximum(np.asarray(kmin, np.int64)[n], K)
    return list(zip((anchors[ok] >> 32).tolist(), (anchors[ok] & 0xffffffff).tolist(), n[ok].tolist(), k[ok].tolist(), ph[ok].tolist(),
                    rd[ok].tolist()))


def restate_numpy(alns, names, lens, L=21, m=10, alpha=Fraction(1, 1000), K=3, D=1):
    """The numpy windows through phasing.py's merge and writer."""
    hg = phasing.Hypergeom(m, L)
    wins = windows_numpy(alns, L, m, alpha, K, D, kmin=hg.kmin(alpha))
    return phasing.format_tsv(names, phasing.merge_loci(wins, lens, m, L, hg))


# ---------------------------------------------------------------------------------------------------- inputs
def make_records(rows):
    """rows of (tid, pos, depth, len, strand) -> ALN_DTYPE array sorted stably by (tid, pos)."""
    a = np.zeros(len(rows), ALN_DTYPE)
    if rows:
        r = np.array(rows, dtype=np.int64)
        a["tid"], a["pos"], a["depth"], a["len"], a["strand"] = r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4]
    return a[np.lexsort((a["pos"], a["tid"]))]


def plant_locus(rows, rng, tid, x0, L, cycles, strands=(0, 1), shift=0, depth=(1, 30), lengths=None):
    """Phased reads from register x0: plus reads at x0 + jL, minus reads at x0 + jL - 2 + shift (shift != 0: off register)."""
    for j in range(cycles):
        for s in strands:
            c = x0 + j * L
            pos = c if s == 0 else c - 2 + shift
            for ln in (lengths or (L,)):
                rows.append((tid, pos, int(rng.randint(depth[0], depth[1] + 1)), ln, s))


def random_records(rng, lens, L, n_noise, n_loci, mixed=(18, 20, 21, 22, 23, 24, 26)):
    rows = []
    for _ in range(n_loci):
        tid = int(rng.randint(0, len(lens)))
        span = 10 * L + 30
        if lens[tid] <= span + 10:
            continue
        x0 = int(rng.randint(3, lens[tid] - span))
        strands = [(0,), (1,), (0, 1)][rng.randint(0, 3)]
        plant_locus(rows, rng, tid, x0, L, int(rng.randint(3, 11)), strands)
    for _ in range(n_noise):
        tid = int(rng.randint(0, len(lens)))
        ln = int(mixed[rng.randint(0, len(mixed))])
        pos = int(rng.randint(1, max(2, lens[tid] - ln + 2)))
        rows.append((tid, pos, int(rng.randint(1, 20)), ln, int(rng.randint(0, 2))))
    for i in rng.randint(0, len(rows), size=len(rows) // 10):      # multi-mapped reads: the same read once more somewhere else
        tid = int(rng.randint(0, len(lens)))
        rows.append((tid, int(rng.randint(1, max(2, lens[tid] - 30))), rows[i][2], rows[i][3], int(rng.randint(0, 2))))
    return make_records(rows)


# ---------------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("seed", range(6))
def test_numpy_restatement_agrees_with_the_plain_one(seed):
    rng = np.random.RandomState(seed)
    L = (21, 22, 24)[seed % 3]
    lens = [3000, 700, 150, 5000]
    alns = random_records(rng, lens, L, 1500, 8)
    names = ["chr%d" % i for i in range(len(lens))]
    for m, alpha, K, D in ((10, Fraction(1, 1000), 3, 1), (4, Fraction(1, 100), 2, 3), (6, Fraction(1), 1, 1), (20, Fraction(1, 10 ** 5), 5, 2)):
        want = restate_plain(alns, names, lens, L, m, alpha, K, D)
        assert restate_numpy(alns, names, lens, L, m, alpha, K, D) == want, (seed, m, alpha, K, D)
        if m == 10:
            assert want.count(b"\n") > 2


# ---------------------------------------------------------------------------------------------------- the exact test
@pytest.mark.parametrize("m,L", [(1, 3), (2, 2), (2, 3), (3, 2)])
def test_p_value_equals_enumeration(m, L):
    hg = phasing.Hypergeom(m, L)
    S, G = hg.S, hg.G
    for n in range(S + 1):
        subsets = list(itertools.combinations(range(S), n))
        for k in range(0, G + 2):
            hits = sum(1 for sub in subsets if sum(1 for s in sub if s < G) >= k)
            assert hg.p(n, k) == Fraction(hits, len(subsets)), (n, k)


def test_hand_values():
    alpha = Fraction(1, 1000)
    table = {(4, 21): (["7.214e-05", "4.074e-04", "7.525e-14", "1.000e+00"], [3, 4, 5, 7, 9]),
             (10, 21): (["9.299e-05", "6.597e-04", "1.320e-34", "1.000e+00"], [3, 4, 6, 8, 12]),
             (10, 24): (["6.224e-05", "3.954e-04", "8.622e-36", "1.000e+00"], [3, 4, 5, 7, 11])}
    for (m, L), (ps, ks) in table.items():
        hg = phasing.Hypergeom(m, L)
        G, S = hg.G, hg.S
        assert [phasing.pvalue_text(hg.p(n, k)) for n, k in ((3, 3), (10, 4), (G, G), (S, G))] == ps
        km = hg.kmin(alpha)
        assert [km[n] for n in (3, 10, 20, 40, 100)] == ks
    assert phasing.Hypergeom(4, 21).kmin(alpha)[100] == 9        # G + 1: never


@pytest.mark.parametrize("m,L", [(4, 18), (10, 21), (7, 24), (20, 30)])
def test_kmin_against_a_direct_scan(m, L):
    hg = phasing.Hypergeom(m, L)
    ns = range(hg.S + 1) if m < 20 else list(range(0, hg.S + 1, 37)) + [hg.S]
    for alpha in (Fraction(1), Fraction(1, 2), Fraction(1, 1000), Fraction(1, 10 ** 9), Fraction(37, 100000)):
        km = hg.kmin(alpha)
        assert len(km) == hg.S + 1
        for n in ns:
            want = next((k for k in range(hg.G + 2) if p_direct(n, k, m, L) <= alpha), hg.G + 1)
            assert km[n] == want, (alpha, n)


# ---------------------------------------------------------------------------------------------------- hand-made loci
def _both(alns, lens, **kw):
    names = ["chr%d" % i for i in range(len(lens))]
    a = restate_plain(alns, names, lens, **kw)
    assert restate_numpy(alns, names, lens, **kw) == a
    return [ln.split(b"\t") for ln in a.split(b"\n")[1:-1]]


def test_perfect_locus_on_both_strands():
    rows = []
    for j in range(10):
        rows += [(0, 1000 + 21 * j, 5, 21, 0), (0, 998 + 21 * j, 5, 21, 1)]
    got = _both(make_records(rows), [5000])
    p = phasing.pvalue_text(p_direct(20, 20, 10, 21))
    assert got == [[b"chr0", b"1000", b"1377", b"9", b"1000", b"20", b"20", p.encode(), b"100", b"100"]]


def test_minus_reads_off_register_do_not_count():
    rows = []
    for j in range(10):
        rows += [(0, 1000 + 21 * j, 5, 21, 0), (0, 999 + 21 * j, 5, 21, 1)]       # c = 1001 + 21 j: one off
    got = _both(make_records(rows), [5000])
    assert len(got) == 1 and got[0][6] == b"10" and got[0][4:6] in ([b"1000", b"20"], [b"1001", b"19"])
    rows = [r for r in rows if r[4] == 0]
    assert _both(make_records(rows), [5000])[0][4:7] == [b"1000", b"10", b"10"]


def test_abutting_windows_do_not_merge_overlapping_ones_do():
    kw = dict(alpha=Fraction(1), K=1)
    got = _both(make_records([(0, 100, 1, 21, 0), (0, 310, 1, 21, 0)]), [2000], **kw)
    assert [g[:4] for g in got] == [[b"chr0", b"100", b"309", b"1"], [b"chr0", b"310", b"519", b"1"]]
    got = _both(make_records([(0, 100, 1, 21, 0), (0, 309, 1, 21, 0)]), [2000], **kw)
    assert [g[:4] for g in got] == [[b"chr0", b"100", b"518", b"2"]]


def test_window_clipped_at_contig_end():
    got = _both(make_records([(0, 200, 1, 21, 0), (1, 50, 1, 21, 1)]), [300, 80], alpha=Fraction(1), K=1)
    assert [g[:3] for g in got] == [[b"chr0", b"200", b"300"], [b"chr1", b"52", b"80"]]


def test_min_depth_removes_an_anchor():
    rows = []
    for j in range(6):
        rows += [(0, 1000 + 21 * j, 4, 21, 0), (0, 998 + 21 * j, 4, 21, 1)]
    rows.append((0, 1005, 1, 21, 0))
    got1 = _both(make_records(rows), [5000])
    got2 = _both(make_records(rows), [5000], D=2)
    assert got1[0][3:7] == [b"5", b"1000", b"13", b"12"] and got1[0][9] == b"49"
    assert got2[0][3:7] == [b"5", b"1000", b"12", b"12"] and got2[0][9] == b"48"
    rows.append((0, 3000, 1, 21, 1))                                  # an isolated unit: its own locus at alpha = 1, gone under -d 2
    assert [g[1] for g in _both(make_records(rows), [5000], alpha=Fraction(1), K=1)][-1] == b"3002"
    assert b"3002" not in [g[1] for g in _both(make_records(rows), [5000], alpha=Fraction(1), K=1, D=2)]


def test_alpha_one_passes_every_window_with_k_phased():
    rows = [(0, 100, 1, 21, 0), (0, 101, 1, 21, 0), (0, 2000, 3, 21, 1), (0, 5000, 2, 22, 0)]
    got = _both(make_records(rows), [9000], alpha=Fraction(1), K=1)
    assert [g[:7] for g in got] == [[b"chr0", b"100", b"310", b"2", b"101", b"1", b"1"], [b"chr0", b"2002", b"2211", b"1", b"2002", b"1", b"1"]]
    assert [g[7] for g in got] == [phasing.pvalue_text(Fraction(20, 420)).encode()] * 2
    assert _both(make_records(rows), [9000], alpha=Fraction(1), K=2) == []


def test_fasta_of_the_loci():
    loci = [(1, 3, 7, 1, (1, 3, 1, 1, 1, 1), Fraction(1)), (0, 1, 2, 1, (0, 1, 1, 1, 1, 1), Fraction(1))]
    assert phasing.format_fasta(["a", "b"], loci, [b"ACGT", b"acgtNNa"]) == b">b:3-7\ngtNNa\n>a:1-2\nAC\n"
    assert phasing.fasta_name("x/out.phas.tsv") == "x/out.phas.fa" and phasing.fasta_name("out.txt") == "out.txt.fa"


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.phasing"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    sam = tmp_path / "a.sam"
    sam.write_bytes(b"@SQ\tSN:c\tLN:100\n")
    s = str(sam)
    bad = [[], ["-l", "17", s], ["-l", "31", s], ["-l", "x", s], ["-c", "3", s], ["-c", "21", s], ["-p", "0", s], ["-p", "1.5", s],
           ["-p", "-0.1", s], ["-p", "x", s], ["-p", "", s], ["-p", "1/1000", s], ["-p", "nan", s], ["-k", "0", s], ["-c", "4", "-k", "9", s],
           ["-k", "21", s], ["-d", "0", s], ["-d", "2147483648", s], ["--device", "-1", s], ["-o", "", s], ["-g", "", s], ["-x", s]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "a.sam").write_bytes(b"@SQ\tSN:c\tLN:100\n")
    (tmp_path / "a.sam.phas.tsv").write_bytes(b"stale\n")
    r = run_cli([str(tmp_path / "a.sam"), str(tmp_path / "nope.sam")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.sam" in r.stderr.decode()
    r = run_cli(["-g", str(tmp_path / "nope.fa"), str(tmp_path / "a.sam")], tmp_path)
    assert r.returncode == 255 and "nope.fa" in r.stderr.decode()


def test_helpers_of_the_command_line(capsys):
    assert [phasing.parse_alpha(x) for x in ("0.001", "1", "1.0", ".5", "1e-5", "2.5E-3", "0", "1.01", "x", "", "1/2", "-1e-3", "1e1")] == \
        [Fraction(1, 1000), 1, 1, Fraction(1, 2), Fraction(1, 100000), Fraction(1, 400), None, None, None, None, None, None, None]
    o, sams, alpha, out = phasing.parse_args(["-l", "24", "-c", "8", "-p", "1e-4", "-k", "4", "-d", "2", "a.sam", "b.sam"])
    assert (o.length, o.cycles, alpha, o.min_phased, o.min_depth, sams, out) == (24, 8, Fraction(1, 10000), 4, 2, ["a.sam", "b.sam"], "a.sam.phas.tsv")
    assert phasing.parse_args(["-o", "x.tsv", "a.sam"])[3] == "x.tsv"
    with pytest.raises(SystemExit) as e:
        phasing.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--length", "--cycles", "--pvalue", "--min-phased", "--min-depth", "--output", "--genome", "--device"):
        assert opt in text
