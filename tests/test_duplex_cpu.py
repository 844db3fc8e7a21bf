"""Host tests of the two-strand fold (mirp_duplex_batch, targets --energy): a plain-Python restatement of the model -- the tables
parsed from csrc/energy_params_t2004.h, the dynamic program, the trace-back with its tie rules, an evaluator of a structure text, the column
formatter of `targets -e` and the extraction of the target strand -- which the GPU tests (test_duplex_gpu.py) compare the device with.  Here the
restatement is pinned: to §21's values, to the project's CPU oracle through the hairpin identity, to the enumeration of every chain on short
strands, to its own symmetry, to the evaluator, the tie rule and the loop limit; and the command line's option errors exit 2 without a device."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_targets_cpu import MIR, ROOT, run_cli

CSRC = os.path.join(ROOT, "mir-prefer_amd", "csrc")
INF = 10000000
MAXLOOP = 30
DUPLEX_INIT = 410
RNA = "NACGU"
PAIR = [[0, 0, 0, 0, 0], [0, 0, 0, 0, 5], [0, 0, 0, 1, 0], [0, 0, 2, 0, 3], [0, 6, 0, 4, 0]]       # [N A C G U][N A C G U]
RTYPE = [0, 2, 1, 4, 3, 6, 5, 7]
MIR156 = "UGACAGAAGAGAGUGAGCAC"


def _tables():
    text = open(os.path.join(CSRC, "energy_params_t2004.h")).read()
    t = {}
    for name, dims, body in re.findall(r"static const int T04_(\w+)((?:\[\d+\])+) = \{([^}]*)\}", text):
        shape = [int(x) for x in re.findall(r"\d+", dims)]
        t[name] = np.array([int(x) for x in body.split(",")], dtype=np.int64).reshape(shape).tolist()
    for name, value in re.findall(r"#define T04_(\w+) \((-?[0-9.]+)\)", text):
        t[name] = float(value) if "." in value else int(value)
    return t


T = _tables()
STACK, BULGE, ILOOP, HAIRPIN = T["stack"], T["bulge"], T["internal_loop"], T["hairpin"]
MM_I, MM_H, MM_1N, MM_23 = T["mismatchI"], T["mismatchH"], T["mismatch1nI"], T["mismatch23I"]
MM_EXT, D5, D3 = T["mismatchExt"], T["dangle5"], T["dangle3"]
INT11, INT21, INT22 = T["int11"], T["int21"], T["int22"]
TERM_AU, NINIO, MAX_NINIO = T["TerminalAU"], T["ninio"], T["MAX_NINIO"]


def codes(s):
    """letters -> 0..4 (N A C G U); T = U, either case, anything else N"""
    s = s.decode() if isinstance(s, (bytes, bytearray)) else s
    return ["NACGU".find(ch) if ch in "ACGU" else 0 for ch in s.upper().replace("T", "U")]


def e_ext(t, a, b):
    """the oracle's E_extloop: a = the 5' neighbour's code or -1, b = the 3' neighbour's"""
    e = TERM_AU if t > 2 else 0
    if a >= 0 and b >= 0:
        e += min(0, MM_EXT[t][a][b])
    elif a >= 0:
        e += min(0, D5[t][a])
    elif b >= 0:
        e += min(0, D3[t][b])
    return e


def e_int(n1, n2, t, t2, si1, sj1, sp1, sq1):
    """the oracle's E_intloop for n1 + n2 <= 30; t2 is already rtype'd"""
    if n1 > n2:
        nl, ns = n1, n2
    else:
        nl, ns = n2, n1
    if nl == 0:
        return STACK[t][t2]
    if ns == 0:
        if nl == 1:
            return BULGE[1] + STACK[t][t2]
        return BULGE[nl] + (TERM_AU if t > 2 else 0) + (TERM_AU if t2 > 2 else 0)
    if ns == 1:
        if nl == 1:
            return INT11[t][t2][si1][sj1]
        if nl == 2:
            return INT21[t][t2][si1][sq1][sj1] if n1 == 1 else INT21[t2][t][sq1][si1][sp1]
        return ILOOP[nl + 1] + min(MAX_NINIO, (nl - 1) * NINIO) + MM_1N[t][si1][sj1] + MM_1N[t2][sq1][sp1]
    if ns == 2:
        if nl == 2:
            return INT22[t][t2][si1][sp1][sq1][sj1]
        if nl == 3:
            return ILOOP[5] + NINIO + MM_23[t][si1][sj1] + MM_23[t2][sq1][sp1]
    return ILOOP[nl + ns] + min(MAX_NINIO, (nl - ns) * NINIO) + MM_I[t][si1][sj1] + MM_I[t2][sq1][sp1]


def _loop(A, B, k, l, i, j):
    """the loop between the pairs (k, l) and (i, j), k < i, l > j (0-based)"""
    return e_int(i - k - 1, l - j - 1, PAIR[A[k]][B[l]], RTYPE[PAIR[A[i]][B[j]]], A[k + 1], B[l - 1], A[i - 1], B[j + 1])


def fill(A, B, init=DUPLEX_INIT):
    """c[i][j] of §21 (0-based) and the number of loop evaluations"""
    n, m = len(A), len(B)
    c = [[INF] * m for _ in range(n)]
    rows, evals = [], 0
    for i in range(n):
        si = A[i - 1] if i else -1
        for j in range(m):
            t = PAIR[A[i]][B[j]]
            if not t:
                continue
            sj = B[j + 1] if j + 1 < m else -1
            best = init + e_ext(t, si, sj)
            t2 = RTYPE[t]
            for k in range(i - 1, max(-1, i - MAXLOOP - 2), -1):
                n1 = i - k - 1
                for l, ckl, tk, sk1, sl1 in rows[k]:
                    if l <= j:
                        continue
                    n2 = l - j - 1
                    if n1 + n2 > MAXLOOP:
                        break
                    evals += 1
                    e = ckl + e_int(n1, n2, tk, t2, sk1, sl1, si, sj)
                    if e < best:
                        best = e
            c[i][j] = best
        rows.append([(l, c[i][l], PAIR[A[i]][B[l]], A[i + 1] if i + 1 < n else -1, B[l - 1] if l else -1) for l in range(m) if c[i][l] < INF])
    return c, evals


def inner_end(A, B, i, j):
    return e_ext(RTYPE[PAIR[A[i]][B[j]]], B[j - 1] if j else -1, A[i + 1] if i + 1 < len(A) else -1)


def duplex(a, b):
    """§21 for one pair of strands -> {mfe, pairs, a_first, a_last, b_first, b_last, structure, evals}"""
    A, B = codes(a), codes(b)
    n, m = len(A), len(B)
    c, evals = fill(A, B)
    best, at = 0, None
    for i in range(n):                                       # ties: the smallest i, then the largest j
        for j in range(m - 1, -1, -1):
            if c[i][j] < INF:
                f = c[i][j] + inner_end(A, B, i, j)
                if f < best:
                    best, at = f, (i, j)
    pa, pb = [], []
    while at is not None:
        i, j = at
        pa.append(i)
        pb.append(j)
        at = None
        for k in range(i - 1, -1, -1):
            for l in range(j + 1, m):
                if (i - k - 1) + (l - j - 1) > MAXLOOP:
                    break
                if c[k][l] < INF and c[i][j] == c[k][l] + _loop(A, B, k, l, i, j):
                    at = (k, l)
                    break
            if at is not None:
                break
    ss = "".join("(" if i in pa else "." for i in range(n)) + "&" + "".join(")" if j in pb else "." for j in range(m))
    rec = dict(mfe=best, pairs=len(pa), a_first=0, a_last=0, b_first=0, b_last=0, structure=ss.encode(), evals=evals)
    if pa:
        rec.update(a_first=min(pa) + 1, a_last=max(pa) + 1, b_first=min(pb) + 1, b_last=max(pb) + 1)
    return rec


_CACHE = {}


def duplex_cached(a, b):
    key = (bytes(a), bytes(b))
    if key not in _CACHE:
        _CACHE[key] = duplex(*key)
    return _CACHE[key]


def chain_of(ss, n):
    """the pairs of a structure text, outermost first, or None when it is not one"""
    ss = ss.decode() if isinstance(ss, (bytes, bytearray)) else ss
    if len(ss) < n + 1 or ss[n] != "&" or set(ss[:n]) - set("(.") or set(ss[n + 1:]) - set(")."):
        return None
    ia = [i for i, ch in enumerate(ss[:n]) if ch == "("]
    jb = [j for j, ch in enumerate(ss[n + 1:]) if ch == ")"]
    return list(zip(ia, jb[::-1])) if len(ia) == len(jb) else None


def evaluate(a, b, chain):
    """the energy §21 gives a chain of pairs (i ascending, j descending), None when it is not allowed; the empty chain is 0"""
    A, B = codes(a), codes(b)
    if not chain:
        return 0
    for (k, l), (i, j) in zip(chain, chain[1:]):
        if not (k < i and l > j) or (i - k - 1) + (l - j - 1) > MAXLOOP:
            return None
    if any(not PAIR[A[i]][B[j]] for i, j in chain):
        return None
    i, j = chain[0]
    e = DUPLEX_INIT + e_ext(PAIR[A[i]][B[j]], A[i - 1] if i else -1, B[j + 1] if j + 1 < len(B) else -1)
    for (k, l), (i, j) in zip(chain, chain[1:]):
        e += _loop(A, B, k, l, i, j)
    i, j = chain[-1]
    return e + inner_end(A, B, i, j)


def brute_force(a, b):
    A, B = codes(a), codes(b)
    best = 0
    for r in range(1, min(len(A), len(B)) + 1):
        for ia in itertools.combinations(range(len(A)), r):
            for jb in itertools.combinations(range(len(B)), r):
                e = evaluate(a, b, list(zip(ia, jb[::-1])))
                if e is not None and e < best:
                    best = e
    return best


def revcomp_rna(a):
    return "".join("NUGCA"[x] for x in codes(a))[::-1]


# ---------------------------------------------------------------------------------------------------- the columns of targets -e
def fmt_mfe(e):
    return b"%s%d.%02d" % (b"-" if e < 0 else b"", abs(e) // 100, abs(e) % 100)


def fmt_ratio(mfe, perfect):
    """mfe / perfect rounded half up to three decimals, in integers; NA when the perfect duplex is unbound"""
    if perfect == 0:
        return b"NA"
    q = (2000 * -mfe + -perfect) // (2 * -perfect)
    return b"%d.%03d" % (q // 1000, q % 1000)


def target_strand(t, o, end, strand):
    """strand b of a site whose interval is t[o:end] on the forward target (codes 0..3 = A C G T, above = ambiguous): one more base on each side where
    the contig has one, an ambiguous one as N; the reverse complement on the minus strand"""
    lo, hi = max(0, o - 1), min(len(t), end + 1)
    x = [int(v) for v in t[lo:hi]]
    if strand:
        x = [3 - v if v < 4 else 4 for v in x][::-1]
    return "".join("ACGUN"[min(v, 4)] for v in x)


def add_energy(data, names, seqs, fold=duplex_cached):
    """The TSV of a run without -e (with or without the bulge column) -> the TSV with -e: four more columns on every line."""
    lines = data.split(b"\n")
    out = [lines[0] + b"\tmfe\tmfe_perfect\tmfe_ratio\tduplex"]
    tid = {nm.encode(): k for k, nm in enumerate(names)}
    assert len(tid) == len(names)
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        a = f[8].replace(b"-", b"")
        b = target_strand(seqs[tid[f[1]]], int(f[2]) - 1, int(f[3]), f[4] == b"-").encode()
        r, p = fold(a, b), fold(a, revcomp_rna(a).encode())
        out.append(ln + b"\t" + fmt_mfe(r["mfe"]) + b"\t" + fmt_mfe(p["mfe"]) + b"\t" + fmt_ratio(r["mfe"], p["mfe"]) + b"\t" + r["structure"])
    return b"\n".join(out) + b"\n"


# ---------------------------------------------------------------------------------------------------- generators (also used on the GPU)
def random_strand(rng, n, alphabet="ACGU"):
    return "".join(alphabet[int(x)] for x in rng.randint(0, len(alphabet), n))


def near_complement(rng, a, edits=3, alphabet="ACGU", flank=2):
    """the reverse complement of a with a few substituted, inserted and deleted bases, and up to `flank` bases on each side"""
    b = list("".join({"A": "U", "C": "G", "G": "C", "U": "A"}.get(ch, "N") for ch in a.upper().replace("T", "U"))[::-1])
    for _ in range(int(rng.randint(0, edits + 1))):
        at, kind = int(rng.randint(0, len(b))), int(rng.randint(0, 4))
        if kind == 0:
            b[at] = alphabet[int(rng.randint(0, len(alphabet)))]
        elif kind == 1:
            b[at:at] = list(random_strand(rng, int(rng.randint(1, 4)), alphabet))
        elif kind == 2 and len(b) > 4:
            del b[at]
        else:                                                 # an interior loop: a few bases in a row replaced
            w = int(rng.randint(1, 4))
            b[at:at + w] = list(random_strand(rng, len(b[at:at + w]), alphabet))
    b = list(random_strand(rng, int(rng.randint(0, flank + 1)), alphabet)) + b + list(random_strand(rng, int(rng.randint(0, flank + 1)), alphabet))
    return "".join(b)


def seeded_pairs(seed, n, la=(12, 32), lb=(12, 35)):
    """n strand pairs, every other one a near-complement"""
    rng = np.random.RandomState(seed)
    out = []
    for q in range(n):
        a = random_strand(rng, int(rng.randint(la[0], la[1] + 1)))
        if q % 2:
            b = near_complement(rng, a)[:lb[1]]
            b += random_strand(rng, max(0, lb[0] - len(b)))
        else:
            b = random_strand(rng, int(rng.randint(lb[0], lb[1] + 1)))
        out.append((a, b))
    return out


def loop_limit_case(k):
    return "GGGGG" + "A" * k + "GGGGG", "CCCCCCCCCC"


# ---------------------------------------------------------------------------------------------------- pins
def test_pins():
    assert duplex("GGGG", "CCCC")["mfe"] == -580 == 3 * -330 + 410
    A, B = codes("A"), codes("U")
    c, _ = fill(A, B)
    assert c[0][0] + inner_end(A, B, 0, 0) == 510
    r = duplex("A", "U")
    assert (r["mfe"], r["pairs"], r["structure"], r["a_first"], r["b_last"]) == (0, 0, b".&.", 0, 0)
    r = duplex("AAAA", "AAAA")
    assert (r["mfe"], r["pairs"], r["structure"]) == (0, 0, b"....&....")
    rc = revcomp_rna(MIR156)
    assert rc == "GUGCUCACUCUCUUCUGUCA"
    assert duplex(MIR156, rc)["mfe"] == -3720
    assert duplex(MIR156, "A" + rc + "A")["mfe"] == -3840
    assert duplex(MIR156, "C" + "GUGCUCUCUCUCUUCUGUCA" + "U")["mfe"] == -3340
    assert fmt_ratio(-3340, -3720) == b"0.898"
    r = duplex(MIR156, rc)
    assert r["structure"] == b"(" * 20 + b"&" + b")" * 20 and (r["pairs"], r["a_first"], r["a_last"], r["b_first"], r["b_last"]) == (20, 1, 20, 1, 20)


def test_letters():
    assert codes("acgutTNxR-") == [1, 2, 3, 4, 4, 4, 0, 0, 0, 0] and codes(b"Ag") == [1, 3]
    assert duplex("ggggtt", "aacccc") == duplex("GGGGUU", "AACCCC")
    assert duplex("GGNGG", "CCNCC")["structure"] == b"((.((&)).))"
    assert duplex("NNNN", "NNNN")["mfe"] == 0


# ---------------------------------------------------------------------------------------------------- the hairpin identity
def hairpin_identity_mfe(a, b, linker=5):
    """The DP without the initiation and with the oracle's hairpin term at the inner end: the MFE of a + N x linker + b when neither strand can pair
    with itself."""
    A, B = codes(a), codes(b)
    c, _ = fill(A, B, init=0)
    best = 0
    for i in range(len(A)):
        for j in range(len(B)):
            if c[i][j] < INF:
                u = (len(A) - 1 - i) + linker + j
                h = HAIRPIN[u] if u <= 30 else HAIRPIN[30] + int(T["LXC"] * np.log(u / 30.))
                s5 = A[i + 1] if i + 1 < len(A) else 0
                s3 = B[j - 1] if j else 0
                best = min(best, c[i][j] + h + MM_H[PAIR[A[i]][B[j]]][s5][s3])
    return best


def test_hairpin_identity_against_the_oracle():
    from tests import oracle_binding
    o = oracle_binding.load()
    rng = np.random.RandomState(21)
    bound = 0
    for q in range(240):
        a = random_strand(rng, int(rng.randint(3, 33)), "AG")
        if q % 3 == 0:
            b = near_complement(rng, a, edits=1, alphabet="CU", flank=1)[:35]
            if len(b) < 3:
                b += "CUC"
        else:
            b = random_strand(rng, int(rng.randint(3, 36)), "CU")
        seq = a + "NNNNN" + b
        want = min(0, o.lfold(seq, max(300, len(seq)))["mfe"])
        assert hairpin_identity_mfe(a, b) == want, (a, b)
        bound += want < 0
    assert bound > 120


# ---------------------------------------------------------------------------------------------------- enumeration, symmetry, structures
def test_brute_force_on_short_strands():
    rng = np.random.RandomState(4)
    bound = 0
    for q in range(400):
        a = random_strand(rng, int(rng.randint(1, 8)), "ACGUN" if q % 4 == 0 else "GCGU")
        b = random_strand(rng, int(rng.randint(1, 8)), "ACGUN" if q % 4 == 0 else "GCCU")
        r = duplex(a, b)
        assert r["mfe"] == brute_force(a, b), (a, b)
        bound += r["mfe"] < 0
    assert bound > 50


def test_symmetry():
    rng = np.random.RandomState(6)
    cases = seeded_pairs(5, 60) + [(random_strand(rng, int(rng.randint(1, 8)), "ACGUN"), random_strand(rng, int(rng.randint(1, 8)), "ACGUN")) for _ in range(100)]
    for a, b in cases:
        assert duplex(a, b)["mfe"] == duplex(b, a)["mfe"], (a, b)


def test_structures_are_chains_with_the_mfe():
    bound = 0
    for a, b in seeded_pairs(7, 80) + [loop_limit_case(30), loop_limit_case(31), ("GGNGG", "CCNCC")]:
        r = duplex(a, b)
        chain = chain_of(r["structure"], len(a))
        assert chain is not None and len(r["structure"]) == len(a) + 1 + len(b) and len(chain) == r["pairs"]
        assert evaluate(a, b, chain) == r["mfe"], (a, b)
        if chain:
            assert (r["a_first"], r["a_last"], r["b_first"], r["b_last"]) == (chain[0][0] + 1, chain[-1][0] + 1, chain[-1][1] + 1, chain[0][1] + 1)
            bound += 1
    assert bound > 40


def test_tie_rule():
    def ends_of(a, b):
        A, B = codes(a), codes(b)
        c, _ = fill(A, B)
        f = {(i, j): c[i][j] + inner_end(A, B, i, j) for i in range(len(A)) for j in range(len(B)) if c[i][j] < INF}
        return sorted(k for k, v in f.items() if v == min(f.values())), min(f.values())
    # GGG x CCCCC has one placement of the helix with a base of b beyond both ends, so one minimal end cell; with six C there are two such
    # placements of one energy: the end cell is the one with the larger j
    assert ends_of("GGG", "CCCCC")[0] == [(2, 1)] and duplex("GGG", "CCCCC")["structure"] == b"(((&.)))."
    ends, low = ends_of("GGG", "CCCCCC")
    assert ends == [(2, 1), (2, 2)]
    r = duplex("GGG", "CCCCCC")
    assert r["mfe"] == low and r["structure"] == b"(((&..)))." and (r["b_first"], r["b_last"]) == (3, 5)
    # two placements on a: the smaller i
    ends, low = ends_of("GGGGGG", "ACCCA")
    assert ends == [(3, 1), (4, 1)]
    r = duplex("GGGGGG", "ACCCA")
    assert r["mfe"] == low and r["structure"] == b".(((..&.)))." and (r["a_first"], r["a_last"]) == (2, 4)


def test_loop_limit():
    r30, r31 = duplex(*loop_limit_case(30)), duplex(*loop_limit_case(31))
    assert r30["pairs"] == 10 and r30["structure"] == b"(((((" + b"." * 30 + b"(((((&))))))))))"
    assert r31["pairs"] == 5 and r31["mfe"] > r30["mfe"]
    one = duplex("GGGGG", "CCCCCCCCCC")
    assert r31["mfe"] <= one["mfe"] + 100 and r30["mfe"] < one["mfe"]


def test_ratio_rounding_and_na():
    assert fmt_ratio(0, 0) == b"NA" and fmt_ratio(-100, 0) == b"NA"
    assert fmt_ratio(0, -3720) == b"0.000" and fmt_ratio(-3720, -3720) == b"1.000" and fmt_ratio(-3840, -3720) == b"1.032"
    assert fmt_ratio(-1, -2000) == b"0.001" and fmt_ratio(-1, -2001) == b"0.000"          # 0.0005 rounds up, 0.00049975 down
    assert fmt_ratio(-3, -2000) == b"0.002" and fmt_ratio(-2999, -2000) == b"1.500"
    assert [fmt_mfe(e) for e in (0, -5, -100, -3340, -12345)] == [b"0.00", b"-0.05", b"-1.00", b"-33.40", b"-123.45"]


def test_target_strand_and_columns():
    t = np.array([0, 1, 2, 3, 4, 0, 0, 1], dtype=np.uint8)                       # A C G T N A A C
    assert target_strand(t, 1, 3, 0) == "ACGU" and target_strand(t, 1, 3, 1) == "ACGU"[::-1].translate(str.maketrans("ACGU", "UGCA"))
    assert target_strand(t, 0, 3, 0) == "ACGU" and target_strand(t, 5, 8, 0) == "NAAC" and target_strand(t, 5, 8, 1) == "GUUN"
    assert target_strand(t, 0, 8, 0) == "ACGUNAAC"
    from tests.test_targets_cpu import CODE, parse_mirnas, restate_numpy, target_of_mirna
    mir = MIR156.encode()
    text = b"A" + target_of_mirna(mir) + b"A"
    seqs = [CODE[np.frombuffer(text, dtype=np.uint8)]]
    plain = restate_numpy(parse_mirnas(b">m\n" + mir + b"\n"), ["t"], seqs, max_half=0)
    got = add_energy(plain, ["t"], seqs)
    assert got.split(b"\n")[0].endswith(b"\ttarget_3to5\tmfe\tmfe_perfect\tmfe_ratio\tduplex")
    assert got.split(b"\n")[1].split(b"\t")[11:] == [b"-38.40", b"-37.20", b"1.032", b"(" * 20 + b"&." + b")" * 20 + b"."]


# ---------------------------------------------------------------------------------------------------- the command line
def test_option_errors_exit_2_before_a_device(tmp_path):
    m, t = tmp_path / "m.fa", tmp_path / "t.fa"
    m.write_bytes(b">m\n" + MIR + b"\n")
    t.write_bytes(b">t\nACGT\n")
    for args in (["-e"], ["-e", str(m)], ["--energy=1", str(m), str(t)], ["-e", "-s", "9", str(m), str(t)], ["--energy", "-k", "-1", str(m), str(t)],
                 ["-e", "--device", "-1", str(m), str(t)], ["--energies", str(m), str(t)], ["-e", "-g", "-o", "", str(m), str(t)]):
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_parse_args_and_help(capsys):
    from mir_prefer_amd import targets
    assert targets.parse_args(["-e", "m.fa", "a.fa"])[0].energy is True
    assert targets.parse_args(["--energy", "-g", "m.fa", "a.fa"])[0].energy is True
    assert not targets.parse_args(["m.fa", "a.fa"])[0].energy
    assert len(targets.parse_args(["-e", "m.fa", "a.fa"])) == 5
    with pytest.raises(SystemExit):
        targets.parse_args(["-h"])
    out = capsys.readouterr().out
    assert "--energy" in out and "mfe_ratio" in out


def test_abi_version_is_17_on_both_sides():
    from mir_prefer_amd import capi
    assert capi.ABI_VERSION == 17
    assert re.search(r"#define MIRP_ABI_VERSION 17\b", open(os.path.join(CSRC, "mirp_api.cpp")).read())


# ---------------------------------------------------------------------------------------------------- the new kernel's resources
def test_duplex_kernel_uses_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "duplex_kernels.hip"), "-o", str(tmp_path / "duplex_kernels.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    report, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    assert sum("duplex_kernel" in k for k in report) >= 1, sorted(report)
    for k, r in sorted(report.items()):
        print(k, "VGPRs", r["VGPRs"], "SGPRs", r.get("TotalSGPRs"), "occupancy", r["Occupancy"], "scratch", r["ScratchSize"], "LDS", r.get("LDS Size"))
        assert r["ScratchSize"] == 0, (k, r)
        assert r.get("LDS Size", 0) == 0, (k, r)             # the slab is dynamic: sized per launch by the longest strands
