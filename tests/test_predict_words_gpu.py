"""GPU tests of the filter kernel's structure rules on words (mir-prefer_amd/csrc/ss_words.h in predict_kernel): lines injected through
mirp_predict_batch_reasons, as tests/test_predict_gpu.py does, at the lengths, view offsets and pair counts where a word rule can go wrong.  The truth is
the CPU oracle: structures_from_lines for the structure list, maturestar for every (mature, structure) pair's code and coordinates, check_loci for the
miRNA list."""
import random

import numpy as np
import pytest

from mir_prefer_amd import records, synth

pytestmark = pytest.mark.gpu

LINE_DTYPE = [("start", "<i4"), ("len", "<i4"), ("energy", "<i4"), ("printed", "<i4")]
ALL_LENGTHS = (1, 1, 100, 0, 1, 55)          # n_samples, min / max mature length, allow_3nt, allow_no_star, minlen: every mature length counts
MIRNA_LENGTHS = (1, 18, 23, 0, 1, 55)


def hairpin(rng, n_pairs, loop, p_bulge, t5, t3):
    """5' tail, an arm of n_pairs '(' with bulges, a loop, the mirrored arm with its own bulges, 3' tail"""
    s = "." * t5
    for _ in range(n_pairs):
        s += "("
        if rng.randrange(100) < p_bulge:
            s += "." * rng.randint(1, 3)
    s += "." * loop
    for _ in range(n_pairs):
        s += ")"
        if rng.randrange(100) < p_bulge:
            s += "." * rng.randint(1, 3)
    return s + "." * t3


def batch(windows, stride, max_lines):
    """windows: [{"ws", "we", "lines": [(ss, energy_dcal, start)], "matures": [(m0, m1, strand, depth)]}] -> W, M, raw"""
    n = len(windows)
    W = np.zeros(n, dtype=records.WINDOW_DTYPE)
    M = np.zeros(sum(len(w["matures"]) for w in windows), dtype=records.MATURE_DTYPE)
    lines = np.zeros((n, max_lines), dtype=LINE_DTYPE)
    ss = np.zeros((n, max_lines, stride), dtype=np.uint8)
    nl = np.zeros(n, dtype=np.int32)
    off = 0
    for k, w in enumerate(windows):
        W[k] = (0, w["ws"], w["we"], 0, w["ws"], w["we"], 0, 0, 0, len(w["matures"]), 0, off, 0, w["we"] - w["ws"], 0)
        for j, m in enumerate(w["matures"]):
            M[off + j] = m
        off += len(w["matures"])
        assert len(w["lines"]) <= max_lines
        nl[k] = len(w["lines"])
        for j, (s, e, st) in enumerate(w["lines"]):
            assert len(s) <= stride - 3
            lines[k, j] = (st, len(s), e, 1)
            ss[k, j, :len(s)] = np.frombuffer(s.encode(), dtype=np.uint8)
    return W, M, {"lines": lines, "ss": ss, "n_lines": nl, "stride": stride, "max_lines": max_lines}


def reads_of(windows):
    """one record per candidate mature, exactly on it and as deep as the mature says: what lets a pair with a good duplex pass the expression rules
    (the windows of a test do not overlap, so a window sees its own reads only)"""
    recs = {}
    for w in windows:
        for m in w["matures"]:
            recs[(m[0], m[1] - m[0], m[2])] = m[3]
    a = np.zeros(max(1, len(recs)), dtype=synth.ALN_DTYPE)
    a["pos"] = 1; a["len"] = 20; a["depth"] = 1
    for k, (pos, ln, st) in enumerate(sorted(recs)):
        a[k] = (0, pos, recs[(pos, ln, st)], ln, st, 0)
    return a


def run_and_check(gpu_ctx, oracle, windows, stride, max_lines, params, alns=None):
    """-> per window: (codes of its pairs, number of miRNAs the oracle finds, the GPU's miRNA rows)"""
    W, M, raw = batch(windows, stride, max_lines)
    alns = reads_of(windows) if alns is None else alns
    mir, nm, st, rec = gpu_ctx.predict_batch_reasons(W, M, alns, raw, params)
    assert (st == 0).all()
    pairs, perw = {}, {}
    for r in rec:
        if r[1] < 0:
            assert int(r[0]) not in perw
            perw[int(r[0])] = r
        else:
            key = (int(r[0]), int(r[1]), int(r[2]))
            assert key not in pairs
            pairs[key] = r
    out = []
    for k, w in enumerate(windows):
        structs = oracle.structures_from_lines(w["lines"], params[5])
        # the structure list: line order, piece order
        assert int(perw[k][2]) == len(structs), (k, [l[0] for l in w["lines"]], structs)
        in_range = [j for j, m in enumerate(w["matures"]) if params[1] <= m[1] - m[0] <= params[2]]
        assert sorted(key for key in pairs if key[0] == k) == [(k, j, s) for j in in_range for s in range(len(structs))] or not structs
        codes = []
        for j in in_range:
            m0, m1, strand, _ = w["matures"][j]
            for s, (ne, fold_start, text, sstype) in enumerate(structs):
                r = pairs[(k, j, s)]
                line = w["lines"][int(r[3])]
                assert (line[2] + int(r[4]), line[0][int(r[4]):int(r[4]) + int(r[5])]) == (fold_start, text), (k, s)
                want = oracle.maturestar(text, m0, m1, fold_start, w["ws"], w["we"], strand)
                assert int(r[6]) == want.code, (k, j, s, text, (m0, m1, strand), int(r[6]), want.code)
                if want.code != 1:
                    assert (int(r[8]), int(r[9])) == (want.fold_s, want.fold_e)
                if want.code == 0:
                    assert (int(r[10]), int(r[11])) == (want.star_s, want.star_e)
                codes.append(want.code)
        # the miRNA list
        loci = oracle.check_loci(structs, M[W[k]["mature_off"]:W[k]["mature_off"] + W[k]["n_matures"]], W[k], alns, params)
        assert int(nm[k]) == min(len(loci), records.MAX_MIRNA_PER_WINDOW), (k, int(nm[k]), len(loci))
        for g, o in zip(mir[k, :nm[k]], loci):
            text = w["lines"][int(g["line"])][0][int(g["ss_off"]):int(g["ss_off"]) + int(g["ss_len"])]
            assert [int(g[f]) for f in ("fold_s", "fold_e", "mat_s", "mat_e", "star_s", "star_e", "strand", "has_star")] + [text] == \
                [o.fold_s, o.fold_e, o.mat_s, o.mat_e, o.star_s, o.star_e, o.strand, o.has_star, o.ss.decode()], k
            assert (int(g["total_depth_mature"]), int(g["total_depth_star"])) == (o.total_depth_mature, o.total_depth_star)
        out.append((codes, len(loci), mir[k, :nm[k]].copy()))
    return out


def matures_on(rng, s, start, ws, we, n):
    """n candidate matures of 18 .. 24 nt on the line s whose first character stands at line position start (1-based), on either strand"""
    out = []
    for _ in range(n):
        ml, strand = rng.randint(18, 24), rng.randrange(2)
        l0 = rng.randint(-2, max(0, len(s) - ml + 2))
        if strand == 0:
            m0 = l0 + ws + start - 1
        else:
            m0 = we - start + 1 - l0 - ml
        out.append((m0, m0 + ml, strand, rng.randint(1, 500)))
    return out


# word boundaries of the staged text lie at multiples of 32 characters of the LINE; the old staging had them at multiples of 16
BOUNDARY = (15, 16, 17, 31, 32, 33, 63, 64, 65)


def boundary_windows(seed, max_len):
    """windows of one to three lines whose lengths, stem starts, loop positions and partner distances straddle the word boundaries"""
    rng = random.Random(seed)
    lens = [n for n in (63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 255, 256, 257, 299, 300) if n <= max_len]
    windows = []
    for n in lens:
        for t5 in BOUNDARY + (0, 1, 30, 47, 48, 49):
            for kind in range(3):
                body = n - t5
                if body < 40:
                    continue
                if kind == 0:          # a plain hairpin whose loop ends the line: arms as long as fit
                    loop = rng.randint(3, 9)
                    s = hairpin(rng, (body - loop) // 2, loop + (body - loop) % 2, 0, t5, 0)
                elif kind == 1:        # bulged arms, a 3' tail
                    s = hairpin(rng, max(14, body // 3), rng.randint(3, 12), rng.randint(3, 20), t5, 0)
                    s = (s + "." * n)[:n] if len(s) <= n else None
                else:                  # two stems side by side inside an outer helix (a bifurcation), or unbalanced when cut
                    a = hairpin(rng, max(8, body // 6), rng.randint(3, 8), 5, 0, rng.randint(0, 4))
                    b = hairpin(rng, max(8, body // 6), rng.randint(3, 8), 5, 0, 0)
                    s = "." * t5 + "((" + a + b + "))"
                    s = (s + "." * n)[:n]
                if s is None or s.count("(") == 0:
                    continue
                assert len(s) == n
                start = rng.randint(1, 40)
                ws = 1000 * (len(windows) + 1) + rng.randint(0, 500); we = ws + start + n + rng.randint(0, 30)
                lines = [(s, -rng.randint(1500, 6000), start)]
                for _ in range(rng.randrange(3)):          # up to two more lines: other lengths, their own starts
                    m = rng.choice(lens)
                    st2 = rng.randint(1, 40)
                    if st2 + m > we - ws:
                        continue
                    lines.append((hairpin(rng, (m - 7) // 2, 7 + (m - 7) % 2, 0, 0, 0) if rng.randrange(2) else
                                  (hairpin(rng, m // 3, 5, 12, rng.randint(0, 20), 0) + "." * m)[:m], -rng.randint(1500, 6000), st2))
                matures = matures_on(rng, s, start, ws, we, 3)
                # one mature laid on the 5' arm from its first pair and one on the 3' arm up to its last: the duplex rules run
                first = s.index("("); last = s.rindex(")")
                for strand in (0, 1):          # deep enough to carry the expression rules against the window's other reads
                    for l0, depth in ((first, 20000 - 5000 * strand), (max(0, last - 21), 300 - 100 * strand)):
                        m0 = l0 + ws + start - 1 if strand == 0 else we - start + 1 - l0 - 22
                        matures.append((m0, m0 + 22, strand, depth))
                windows.append({"ws": ws, "we": we, "lines": lines, "matures": matures})
    return windows


@pytest.mark.parametrize("precursor_len,stride", [(300, 352), (300, 360), (120, 184)])
def test_boundary_length_lines(precursor_len, stride, gpu_ctx, oracle):
    """Lines of 63 .. 300 characters (.. 120 at the short stride) with stems, loops and partners across the word boundaries, at a stride that is a multiple
    of the word's 32 characters and at two that are not.  Structure list, every pair's code and coordinates, the miRNA list; the passing code and at
    least five failure codes occur."""
    windows = boundary_windows(11, precursor_len)
    assert len(windows) > 60
    res = run_and_check(gpu_ctx, oracle, windows, stride, 4, ALL_LENGTHS)
    codes = {}
    for c, _, _ in res:
        for x in c:
            codes[x] = codes.get(x, 0) + 1
    print(sorted(codes.items()), sum(n for _, n, _ in res))
    assert codes.get(0, 0) > 0 and sum(1 for c in codes if c != 0) >= 5, codes
    assert sum(n for _, n, _ in res) > 0          # and some pairs pass the expression rules too: the miRNA list is not empty


def test_bifurcated_lines_with_pieces_at_odd_offsets(gpu_ctx, oracle):
    """Lines of several top-level stems: filter_ss cuts them into pieces that start at offsets which are no multiple of 16, 32 or 64, stem-loops and
    good bifurcations among them, and a piece that has the normalised energy of a whole line of the same window (a tie the selection rule must break
    towards the later structure)."""
    rng = random.Random(5)
    windows, offs = [], set()
    for rep in range(40):
        parts, s = [], "." * rng.choice((0, 1, 3, 17, 33))
        for _ in range(rng.randint(2, 4)):
            if rng.randrange(3) == 0:          # a bifurcated stem: two hairpins inside a helix
                p = "(((" + hairpin(rng, rng.randint(10, 14), 4, 0, rng.randint(2, 9), 2) + hairpin(rng, rng.randint(10, 14), 5, 0, 1, rng.randint(2, 9)) + ")))"
            else:
                p = hairpin(rng, rng.randint(24, 34), rng.randint(3, 9), rng.choice((0, 0, 8)), 0, 0)
            parts.append(len(s))
            s += p + "." * rng.choice((1, 2, 5, 13, 21))
        if len(s) > 345:
            continue
        start = rng.randint(1, 30)
        ws = 2000 * (len(windows) + 1); we = ws + start + len(s) + 5
        e = -rng.randint(3000, 9000)
        lines = [(s, e, start)]
        # a whole line with the same energy / length ratio as the bifurcated line its pieces inherit from: same text length, a single hairpin
        lines.append((hairpin(rng, (len(s) - 5) // 2, 5 + (len(s) - 5) % 2, 0, 0, 0), e, start))
        matures = []
        for o in parts:
            for strand in (0, 1):
                l0 = o + 1
                m0 = l0 + ws + start - 1 if strand == 0 else we - start + 1 - l0 - 21
                matures.append((m0, m0 + 21, strand, 10 ** (4 - len(matures) // 2) if len(matures) < 8 else 1))
        windows.append({"ws": ws, "we": we, "lines": lines, "matures": matures})
        for _, fs, text, _ in oracle.structures_from_lines(lines[:1], 55):
            offs.add(fs - start)
    assert any(o % 16 and o % 32 and o % 64 for o in offs) and len({o % 32 for o in offs}) >= 8, sorted(offs)
    res = run_and_check(gpu_ctx, oracle, windows, 352, 2, ALL_LENGTHS)
    assert sum(n for _, n, _ in res) > 10 and sum(c.count(0) for c, _, _ in res) > 20


def pair_window(rng, ws, n_structs, mature_lens, depths, n_good=None):
    """a window of n_structs one-hairpin lines (each its own structure) and matures laid on the 5' arm of them all; the lines differ in their tails"""
    arm = 30
    lines = []
    for k in range(n_structs):
        t5 = 2 + (k % 7)
        s = hairpin(rng, arm, 6, 0, t5, 3 + (k % 5))
        if n_good is not None and k >= n_good:
            s = s.replace("(" * arm, "(" * 10 + "...." + "(" * (arm - 10), 1).replace(")" * arm, ")" * (arm - 10) + "." + ")" * 10, 1)      # a bulge of 4: fails
        lines.append((s, -3000 - 13 * k, 10 - t5))          # the first pair of every line stands at the same window position
    we = ws + 10 + len(lines[0][0]) + 20
    first = ws + 10 - 1
    matures = [(first + (j % 4), first + (j % 4) + ml, 0, d) for j, (ml, d) in enumerate(zip(mature_lens, depths))]
    return {"ws": ws, "we": we, "lines": lines, "matures": matures}


def test_pair_passes(gpu_ctx, oracle):
    """Windows by their number of (in-range mature, structure) pairs: 100 (5 x 20: two passes of 64), 64 exactly, one; in-range matures at ranks 1 and 3
    of four; more loci than MIRP_MAX_MIRNA_PER_WINDOW.  Each equals the oracle, and equals its matures run as one-mature windows."""
    rng = random.Random(9)
    windows = [
        pair_window(rng, 3000, 20, [21, 22, 20, 23, 21], [50, 400, 400, 7, 90]),
        pair_window(rng, 6000, 16, [21, 22, 20, 23], [5, 5, 300, 2]),
        pair_window(rng, 9000, 1, [21], [10]),
        pair_window(rng, 12000, 6, [24, 21, 24, 22], [900, 500, 100, 20]),          # depth order = list order: the in-range ones are ranks 1 and 3
        pair_window(rng, 15000, 3, [20, 21, 22, 23] * 4, [100 - j for j in range(16)]),
        pair_window(rng, 18000, 12, [21, 23, 22], [10, 30, 20], n_good=5),
    ]
    alns = reads_of(windows)
    res = run_and_check(gpu_ctx, oracle, windows, 352, 24, MIRNA_LENGTHS, alns)
    n_pairs = [len(c) for c, _, _ in res]
    assert n_pairs[:4] == [100, 64, 1, 12] and res[4][1] > records.MAX_MIRNA_PER_WINDOW and len(res[4][2]) == records.MAX_MIRNA_PER_WINDOW, (n_pairs, [r[1] for r in res])
    assert all(n > 0 for _, n, _ in res)
    # the same matures as windows of one mature each: window k's j-th locus is the locus of its j-th passing mature in depth order
    for k, w in enumerate(windows):
        order = sorted(range(len(w["matures"])), key=lambda j: (-w["matures"][j][3], j))
        singles = [dict(w, matures=[w["matures"][j]]) for j in order]
        got = [r[2][0] for r in run_and_check(gpu_ctx, oracle, singles, 352, 24, MIRNA_LENGTHS, alns) if len(r[2])]
        got = got[:records.MAX_MIRNA_PER_WINDOW]
        assert len(got) == len(res[k][2])
        fields = [f for f in records.MIRNA_DTYPE.names if f != "window"]
        for a, b in zip(got, res[k][2]):
            assert [int(a[f]) for f in fields] == [int(b[f]) for f in fields], k


def test_long_line_in_global_memory(gpu_ctx, oracle):
    """A window whose staged text does not fit in LDS (384 lines of up to 3,197 characters: the text goes to the kernel's global scratch area): one line
    of 2,900 characters with eleven top-level stems, pieces at odd offsets far into the line, and two ordinary lines."""
    rng = random.Random(21)
    s = "." * 7
    parts = []
    while len(s) < 2600:
        parts.append(len(s))
        if len(parts) % 3 == 0:
            s += "((" + hairpin(rng, 40, 6, 4, 3, 2) + hairpin(rng, 38, 5, 4, 2, 5) + "))" + "." * rng.randint(1, 30)
        else:
            s += hairpin(rng, rng.randint(60, 120), rng.randint(3, 11), rng.choice((0, 3, 6)), 0, 0) + "." * rng.randint(1, 30)
    assert 1024 < len(s) < 3190 and len(parts) >= 8
    ws, start = 5000, 12
    we = ws + start + len(s) + 40
    lines = [(s, -90000, start), (hairpin(rng, 100, 7, 2, 33, 4), -9000, 40), (hairpin(rng, 30, 4, 0, 1, 0), -2500, 2000)]
    matures = []
    for o in parts:
        for strand in (0, 1):
            l0 = o + 2
            m0 = l0 + ws + start - 1 if strand == 0 else we - start + 1 - l0 - 21
            matures.append((m0, m0 + 21, strand, rng.randint(1, 500)))
    w = {"ws": ws, "we": we, "lines": lines, "matures": matures}
    from mir_prefer_amd import capi  # noqa: F401
    res = run_and_check(gpu_ctx, oracle, [w], 3200, 384, ALL_LENGTHS)
    assert len(res[0][0]) >= len(matures) * 8 and res[0][0].count(0) >= 4 and res[0][1] > 0
