"""Host tests of the plant miRNA target-site search (mir_prefer_amd.targets): the tests' two restatements of the whole definition,
a plain-Python per-site scorer and a numpy brute force, both producing the TSV bytes; hand-made cases that pin the score, the strands, the blocks,
the order and -k; and every option error of the command line with its exit status, checked without opening a device.  The GPU tests
(test_targets_gpu.py) compare the device output with these restatements."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_align_cpu import CODE, load_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"miRNA\ttarget\tstart\tend\tstrand\tscore\tmismatches\tgu\tmirna_5to3\tpairs\ttarget_3to5\n"
WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"
RNA = b"ACGUN"
MCODE = np.full(256, 4, dtype=np.uint8)          # miRNA letters: A C G U/T in either case 0..3, anything else unknown
for _i, _ch in enumerate(b"ACGU"):
    MCODE[_ch] = MCODE[_ch + 32] = _i
MCODE[ord("T")] = MCODE[ord("t")] = 3
# pair class of (miRNA code 0..4, target-strand base 0..3 = A C G U): 0 Watson-Crick, 1 G:U, 2 mismatch
CLS = np.full((5, 4), 2, dtype=np.int64)
for _m in range(4):
    CLS[_m, 3 - _m] = 0
CLS[2, 3] = CLS[3, 2] = 1
PAIR = b"|ox"


class Refused(Exception):
    def __init__(self, record, reason):
        super().__init__(record, reason)
        self.record, self.reason = record, reason


def _strip(b):
    return b.strip(WS)


def parse_mirnas(data):
    """§14's miRNA FASTA -> [(name bytes, code array)], or Refused(record, reason) with reason in {"name", "byte", "length", "count"}."""
    out = []
    cur = None
    lines = re.split(rb"\r\n|\r|\n", data)

    def finish():
        if cur is not None:
            L = len(cur[1])
            if not 12 <= L <= 32:
                raise Refused(len(out) + 1, "length")
            out.append((cur[0], MCODE[np.frombuffer(bytes(cur[1]), dtype=np.uint8)]))
    for line in lines:
        if line.startswith(b">"):
            finish()
            cur = None
            if len(out) + 1 > 1 << 24:
                raise Refused(len(out) + 1, "count")
            name = _strip(line[1:])
            if not name:
                raise Refused(len(out) + 1, "name")
            if any(c >= 0x80 for c in name):
                raise Refused(len(out) + 1, "byte")
            cur = (name.replace(b"\t", b" "), bytearray())
        elif cur is not None:
            s = _strip(line)
            if any(c >= 0x80 for c in s):
                raise Refused(len(out) + 1, "byte")
            cur[1].extend(s)
    finish()
    return out


def _line(mname, tname, o, L, strand, half, mc, cls, ys):
    return b"%s\t%s\t%d\t%d\t%s\t%d.%d\t%d\t%d\t%s\t%s\t%s\n" % (
        mname, tname.encode(), o + 1, o + L, b"-" if strand else b"+", half // 2, 5 * (half & 1), int((cls == 2).sum()), int((cls == 1).sum()),
        bytes(RNA[c] for c in mc), bytes(PAIR[c] for c in cls), bytes(RNA[y] for y in ys))


def score_site(mc, t, o, strand, cleavage):
    """The plain per-site scorer: miRNA codes mc against target codes t at offset o -> (half-score, classes, target-strand bases) or None when the
    window leaves the target, holds an ambiguous base, or fails -c."""
    L = len(mc)
    if o < 0 or o + L > len(t):
        return None
    half, cls, ys = 0, [], []
    for i in range(1, L + 1):
        x = int(t[o + i - 1] if strand else t[o + L - i])
        if x > 3:
            return None
        y = 3 - x if strand else x
        k = int(CLS[mc[i - 1], y])
        w = 2 if 2 <= i <= 13 else 1
        half += w * (0, 1, 2)[k]
        cls.append(k)
        ys.append(y)
    cls = np.array(cls)
    if cleavage and (cls[9] == 2 or cls[10] == 2):
        return None
    return half, cls, ys


def _emit(mirnas, names, sites, k):
    """sites: (m, half, tid, o, strand, line) -> the TSV bytes in §14's order, -k applied."""
    sites.sort(key=lambda s: s[:5])
    out, per = [HEADER], {}
    for s in sites:
        per[s[0]] = per.get(s[0], 0) + 1
        if k == 0 or per[s[0]] <= k:
            out.append(s[5])
    return b"".join(out)


def restate_plain(mirnas, names, seqs, max_half=8, both=False, cleavage=False, k=0):
    sites = []
    for m, (mname, mc) in enumerate(mirnas):
        L = len(mc)
        for tid, t in enumerate(seqs):
            for o in range(len(t) - L + 1):
                for strand in ((0, 1) if both else (0,)):
                    r = score_site(mc, t, o, strand, cleavage)
                    if r is not None and r[0] <= max_half:
                        sites.append((m, r[0], tid, o, strand, _line(mname, names[tid], o, L, strand, r[0], mc, r[1], r[2])))
    return _emit(mirnas, names, sites, k)


WEIGHT = {L: np.array([2 if 2 <= i <= 13 else 1 for i in range(1, L + 1)]) for L in range(12, 33)}


def sites_numpy(mc, t, max_half, both, cleavage):
    """Every site of one miRNA on one target, vectorised: -> list of (half, o, strand, classes, target-strand bases)."""
    L = len(mc)
    if len(t) < L:
        return []
    W = np.lib.stride_tricks.sliding_window_view(t, L)
    ok = ~(W > 3).any(axis=1)
    out = []
    for strand in ((0, 1) if both else (0,)):
        Y = (3 - np.minimum(W, 3)) if strand else np.minimum(W, 3)[:, ::-1]
        C = CLS[mc[None, :], Y]
        half = (np.array([0, 1, 2])[C] * WEIGHT[L]).sum(axis=1)
        keep = ok & (half <= max_half)
        if cleavage:
            keep &= (C[:, 9] != 2) & (C[:, 10] != 2)
        for o in np.flatnonzero(keep):
            out.append((int(half[o]), int(o), strand, C[o], Y[o]))
    return out


def restate_numpy(mirnas, names, seqs, max_half=8, both=False, cleavage=False, k=0, only=None):
    """The numpy brute force of the whole output; only = miRNA indices to restate (the others contribute no lines)."""
    sites = []
    for m, (mname, mc) in enumerate(mirnas):
        if only is not None and m not in only:
            continue
        for tid, t in enumerate(seqs):
            for half, o, strand, C, Y in sites_numpy(mc, t, max_half, both, cleavage):
                sites.append((m, half, tid, o, strand, _line(mname, names[tid], o, len(mc), strand, half, mc, C, Y)))
    return _emit(mirnas, names, sites, k)


def restate_files(mirna_path, target_paths, numpy=True, **kw):
    mirnas = parse_mirnas(open(mirna_path, "rb").read())
    names, seqs = load_reference(target_paths)
    return (restate_numpy if numpy else restate_plain)(mirnas, names, seqs, **kw)


# ---------------------------------------------------------------------------------------------------- shared generators (also used on the GPU)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def target_of_mirna(mirna_letters, strand=0):
    """The forward target text that pairs perfectly with the miRNA (letters A C G U/T): plus = reverse complement, minus = the miRNA as DNA."""
    m = MCODE[np.frombuffer(mirna_letters, dtype=np.uint8)]
    assert (m < 4).all()
    x = m if strand else (3 - m)[::-1]
    return ACGT[x].tobytes()


def random_mirnas(rng, n, lo=12, hi=32, unknown=0.0, lower=0.0, t_for_u=0.5):
    out = []
    for k in range(n):
        L = int(rng.randint(lo, hi + 1))
        s = bytearray(b"ACGU"[c] for c in rng.randint(0, 4, L))
        for i in range(L):
            if s[i] == ord("U") and rng.rand() < t_for_u:
                s[i] = ord("T")
            if unknown and rng.rand() < unknown:
                s[i] = b"NRYX-."[rng.randint(0, 6)]
            if lower and rng.rand() < lower:
                s[i] = ord(chr(s[i]).lower())
        out.append(bytes(s))
    return out


def plant(rng, text, mirna, n, subs=(0, 3), both=True):
    """Writes n copies of the miRNA's perfect site into the bytearray text at random offsets (strand random when both), with up to subs[1] random
    substitutions each.  -> list of (offset, strand)."""
    sites = []
    clean = bytes(c for c in mirna if c in b"ACGUTacgut").upper()
    if len(clean) != len(mirna):
        return sites
    for _ in range(n):
        strand = int(rng.randint(0, 2)) if both else 0
        site = bytearray(target_of_mirna(clean, strand))
        for _ in range(int(rng.randint(subs[0], subs[1] + 1))):
            site[int(rng.randint(0, len(site)))] = b"ACGT"[rng.randint(0, 4)]
        o = int(rng.randint(0, len(text) - len(site)))
        text[o:o + len(site)] = site
        sites.append((o, strand))
    return sites


def write_fasta(path, records, width=60):
    with open(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + (name.encode() if isinstance(name, str) else name) + b"\n")
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + b"\n")


# ---------------------------------------------------------------------------------------------------- hand-made cases
def _one(mirna, target, **kw):
    """one miRNA against one target text, both restatements -> the rows split at tabs"""
    mirnas = parse_mirnas(b">m\n" + mirna + b"\n")
    codes = CODE[np.frombuffer(target, dtype=np.uint8)]
    got = restate_plain(mirnas, ["t"], [codes], **kw)
    assert got == restate_numpy(mirnas, ["t"], [codes], **kw)
    return [ln.split(b"\t") for ln in got.split(b"\n")[1:-1]]


MIR = b"UUCCACAGCUUUCUUGAACUG"            # 21 nt


def test_perfect_site_scores_zero():
    site = target_of_mirna(MIR)
    rows = _one(MIR, b"GG" + site + b"GG", max_half=0)
    assert len(rows) == 1
    r = rows[0]
    assert r[:8] == [b"m", b"t", b"3", b"23", b"+", b"0.0", b"0", b"0"]
    assert r[8] == MIR and r[9] == b"|" * 21
    # target_3to5: column i pairs with miRNA position i
    assert r[10] == bytes(b"ACGU"[3 - b"ACGU".index(c)] for c in MIR)


def _mutate(site, L, i, base):
    """the plus-strand site with the base paired to miRNA position i replaced"""
    s = bytearray(site)
    s[L - i] = ord(base)
    return bytes(s)


def test_gu_weights_by_position():
    L = len(MIR)
    site = target_of_mirna(MIR)
    # position 5: miRNA C -> would pair G; G:U needs miRNA G or U: use position 2 (U) with target G instead of A
    assert MIR[1:2] == b"U" and MIR[4:5] == b"A"
    rows = _one(MIR, _mutate(site, L, 2, "G"))
    assert rows[0][5] == b"1.0" and rows[0][7] == b"1" and rows[0][9][1:2] == b"o"
    mir5 = MIR[:4] + b"G" + MIR[5:]                       # position 5 = G, target U (forward T on +)
    rows = _one(mir5, _mutate(target_of_mirna(mir5), L, 5, "T"))
    assert rows[0][5] == b"1.0" and rows[0][9] == b"||||o" + b"|" * 16
    assert MIR[0:1] == b"U"
    rows = _one(MIR, _mutate(site, L, 1, "G"))         # position 1: weight 1
    assert rows[0][5] == b"0.5" and rows[0][9][0:1] == b"o"
    rows = _one(MIR, _mutate(site, L, 21, "A"), max_half=8)   # mismatch at 21: 1.0; at 13: 2.0
    assert rows[0][5] == b"1.0" and rows[0][6] == b"1"
    rows = _one(MIR, _mutate(site, L, 13, "C" if site[L - 13:L - 12] != b"C" else "G"), max_half=8)
    assert rows[0][5] == b"2.0"


def test_cleavage_rule():
    L = len(MIR)
    site = target_of_mirna(MIR)
    bad = _mutate(site, L, 10, "C" if site[L - 10:L - 9] != b"C" else "A")
    assert _one(MIR, bad, cleavage=True) == []
    rows = _one(MIR, bad)
    assert rows[0][5] == b"2.0" and rows[0][9][9:10] == b"x"
    # a G:U at 10 is not a mismatch: MIR[9] = 'U' pairs A; G:U = target G
    assert MIR[9:10] == b"U"
    rows = _one(MIR, _mutate(site, L, 10, "G"), cleavage=True)
    assert rows[0][5] == b"1.0"


def test_letters_case_and_t():
    site = target_of_mirna(MIR)
    want = _one(MIR, site)
    assert _one(MIR.replace(b"U", b"T"), site) == want
    assert _one(MIR.lower(), site) == want
    assert _one(MIR, site.lower()) == want


def test_unknown_mirna_letter_is_a_mismatch():
    L = len(MIR)
    mir = MIR[:L - 1] + b"N"
    rows = _one(mir, target_of_mirna(MIR))
    assert rows[0][5] == b"1.0" and rows[0][6] == b"1" and rows[0][8].endswith(b"N") and rows[0][9].endswith(b"x")
    rows = _one(MIR[:3] + b"R" + MIR[4:], target_of_mirna(MIR))
    assert rows[0][5] == b"2.0" and rows[0][8][3:4] == b"N"


def test_n_in_target_blocks_the_site():
    site = bytearray(target_of_mirna(MIR))
    site[5] = ord("N")
    assert _one(MIR, bytes(site), max_half=16) == []
    site[5] = ord("R")
    assert _one(MIR, bytes(site), max_half=16) == []


def test_contig_boundary(tmp_path):
    site = target_of_mirna(MIR)
    write_fasta(tmp_path / "t.fa", [("a", b"CC" + site[:10]), ("b", site[10:] + b"CC"), ("c", site)])
    write_fasta(tmp_path / "m.fa", [("m", MIR)])
    got = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], max_half=0)
    assert [ln.split(b"\t")[:6] for ln in got.split(b"\n")[1:-1]] == [[b"m", b"c", b"1", b"21", b"+", b"0.0"]]
    assert restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], numpy=False, max_half=0) == got


def test_minus_strand_coordinates_and_target_text():
    site = target_of_mirna(MIR, strand=1)
    assert site == MIR.replace(b"U", b"T")
    rows = _one(MIR, b"AAAA" + site + b"A", both=True, max_half=0)
    assert len(rows) == 1 and rows[0][:6] == [b"m", b"t", b"5", b"25", b"-", b"0.0"]
    # target_3to5 column i = complement of the forward base at start + i - 1
    assert rows[0][10] == bytes(b"ACGU"[3 - b"ACGU".index(c)] for c in MIR)
    assert _one(MIR, b"AAAA" + site + b"A", both=False, max_half=0) == []


def test_order_of_ties(tmp_path):
    """score, then target in file order (not by name), then start, then + before - at the same offset (a palindrome)"""
    mir = b"ACGUACGUACGUACGU"                               # its own reverse complement: + and - at the same offset
    assert target_of_mirna(mir, 0) == target_of_mirna(mir, 1)
    site = target_of_mirna(mir)
    write_fasta(tmp_path / "t.fa", [("z", b"T" + site + b"TT" + site), ("a", site)])
    write_fasta(tmp_path / "m.fa", [("second", mir), ("first", MIR)])
    got = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], both=True, max_half=4)
    rows = [ln.split(b"\t")[:6] for ln in got.split(b"\n")[1:-1]]
    zero = [r for r in rows if r[5] == b"0.0"]
    assert zero == [[b"second", b"z", b"2", b"17", b"+", b"0.0"], [b"second", b"z", b"2", b"17", b"-", b"0.0"],
                    [b"second", b"z", b"20", b"35", b"+", b"0.0"], [b"second", b"z", b"20", b"35", b"-", b"0.0"],
                    [b"second", b"a", b"1", b"16", b"+", b"0.0"], [b"second", b"a", b"1", b"16", b"-", b"0.0"]]
    assert rows[:6] == zero
    halves = [float(r[5]) for r in rows if r[0] == b"second"]
    assert halves == sorted(halves)
    assert restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], numpy=False, both=True, max_half=4) == got


def test_max_sites_cuts_per_mirna_in_output_order(tmp_path):
    rng = np.random.RandomState(3)
    text = bytearray(ACGT[rng.randint(0, 4, 3000)].tobytes())
    mirs = random_mirnas(rng, 3, 18, 22, t_for_u=0)
    for m in mirs:
        plant(rng, text, m, 6, subs=(0, 2))
    write_fasta(tmp_path / "t.fa", [("t", bytes(text))])
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    full = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], both=True).split(b"\n")[1:-1]
    for k in (1, 2, 5):
        got = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], both=True, k=k).split(b"\n")[1:-1]
        want = []
        for i in range(3):
            want += [ln for ln in full if ln.startswith(b"m%d\t" % i)][:k]
        assert got == want and len(got) > 0


@pytest.mark.parametrize("seed", [1, 2])
def test_numpy_restatement_agrees_with_the_plain_one(seed):
    rng = np.random.RandomState(seed)
    mirs = random_mirnas(rng, 6, unknown=0.05, lower=0.2)
    text = bytearray(ACGT[rng.randint(0, 4, 1500)].tobytes())
    for m in mirs:
        plant(rng, text, m, 3)
    text[100:110] = b"N" * 10
    seqs = [CODE[np.frombuffer(bytes(text[:800]), dtype=np.uint8)], CODE[np.frombuffer(bytes(text[800:]), dtype=np.uint8)]]
    mirnas = parse_mirnas(b"".join(b">m%d x\n%s\n" % (i, m) for i, m in enumerate(mirs)))
    for kw in (dict(max_half=8), dict(max_half=6, both=True, cleavage=True), dict(max_half=16, both=True, k=3)):
        assert restate_plain(mirnas, ["a", "b"], seqs, **kw) == restate_numpy(mirnas, ["a", "b"], seqs, **kw)


def test_mirna_fasta_rules_and_refusals():
    got = parse_mirnas(b"junk\n>  a\tb c  \nACGU\r\nacgu\rTTTT\n\n>x\n" + b"A" * 12 + b"\n>x\n" + b"G" * 32)
    assert [n for n, _ in got] == [b"a b c", b"x", b"x"]
    assert list(got[0][1]) == [0, 1, 2, 3] * 2 + [3] * 4
    for data, rec, why in ((b">a\n" + b"A" * 11 + b"\n", 1, "length"), (b">a\n" + b"A" * 12 + b"\n>b\n" + b"A" * 33, 2, "length"),
                           (b">a\n" + b"A" * 12 + b"\n> \t\n" + b"A" * 12, 2, "name"), (b">a\n" + b"A" * 12 + b"\n>b\n" + b"A" * 11 + b"\xc3\xa9", 2, "byte"),
                           (">é\n".encode() + b"A" * 12, 1, "byte"), (b">a\n>b\n" + b"A" * 12, 1, "length")):
        with pytest.raises(Refused) as e:
            parse_mirnas(data)
        assert (e.value.record, e.value.reason) == (rec, why), data


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    m, t = tmp_path / "m.fa", tmp_path / "t.fa"
    m.write_bytes(b">m\n" + MIR + b"\n")
    t.write_bytes(b">t\nACGT\n")
    bad = [[], [str(m)], ["-s", "8.5", str(m), str(t)], ["-s", "-1", str(m), str(t)], ["-s", "0.25", str(m), str(t)], ["-s", "x", str(m), str(t)],
           ["-s", "1e0", str(m), str(t)], ["-s", "", str(m), str(t)], ["-k", "-1", str(m), str(t)], ["-k", "x", str(m), str(t)],
           ["--device", "-1", str(m), str(t)], ["-o", "", str(m), str(t)], ["-x", str(m), str(t)]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "m.fa").write_bytes(b">m\n" + MIR + b"\n")
    (tmp_path / "m.fa.targets.tsv").write_bytes(b"stale\n")
    r = run_cli([str(tmp_path / "m.fa"), str(tmp_path / "nope.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.fa" in r.stderr.decode()
    r = run_cli([str(tmp_path / "nope.fa"), str(tmp_path / "m.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ")


def test_helpers_of_the_command_line(capsys):
    from mir_prefer_amd import targets
    assert [targets.parse_half_score(x) for x in ("0", "4", "4.0", "2.5", ".5", "8", "8.00", "3.", "8.5", "0.25", "-1", "", "nan", "1e0")] == \
        [0, 8, 8, 5, 1, 16, 16, 6, None, None, None, None, None, None]
    assert targets.output_name("d/x_miRNA.mature.fa") == "d/x_miRNA.mature.fa.targets.tsv"
    o, m, t, half, out = targets.parse_args(["-s", "3.5", "-b", "-c", "-k", "7", "m.fa", "a.fa", "b.fa"])
    assert (m, t, half, out, o.both_strands, o.cleavage_site, o.max_sites) == ("m.fa", ["a.fa", "b.fa"], 7, "m.fa.targets.tsv", True, True, 7)
    assert targets.parse_args(["-o", "x.tsv", "m.fa", "a.fa"])[4] == "x.tsv"
    with pytest.raises(SystemExit) as e:
        targets.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--max-score", "--both-strands", "--cleavage-site", "--max-sites", "--output", "--device"):
        assert opt in text
