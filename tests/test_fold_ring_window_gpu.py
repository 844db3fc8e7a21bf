"""GPU parity of the fill kernel's wrap-free ring window.  The candidate-pool pass of the default model mirrors the first A1_CHUNK rows of the c ring
behind row 31 and reads the ring rows of a chunk of bulge / 1xn candidates at compile-time offsets from one lane base (a1_win_row, fold_lds_common.h).
A stale or missing mirror row shows as a wrong energy of a bulge or 1xn loop whose chunk crosses the seam between row 31 and the mirror rows, so the
windows here plant exactly those loops, at every loop size and at every ring phase (d - 2) & 31 of the loop's closing pair.  Every comparison is
pool path == dense path (set_fold_split_path(1): the checked code on the row table) == CPU oracle, exact on lines (structure text, energy, start
column), MFE and status.

On the MI355X (both tests): no window leaves the pool path (last_fold_dense() == 0, last_fold_fallbacks() == 0).  A build without the mirror rows'
store (make VARIANT=nomirror VFLAGS=-DMIRP_NO_RING_MIRROR) fails test 1 at both spans."""
import random

import pytest

from tests.test_fold_two_per_cu_gpu import _both_paths
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu

_COMP = {"G": "C", "C": "G"}


def _helix(r, k):
    a = "".join(r.choice("GC") for _ in range(k))
    return a, "".join(_COMP[c] for c in reversed(a))


def _construct(r, n5, n3, h, hl):
    """outer helix of 8 bp | n5 unpaired A | inner helix of h bp | GAAA / GAAAA | inner helix | n3 unpaired A | outer helix.
    Returns the sequence and, 0-based inside it, the loop's closing pair (i, j) and inner pair (p, q)."""
    o5, o3 = _helix(r, 8)
    i5, i3 = _helix(r, h)
    s = o5 + "A" * n5 + i5 + "G" + "A" * (hl - 1) + i3 + "A" * n3 + o3
    i = 7
    p = i + n5 + 1
    q = p + 2 * h + hl - 1
    j = q + n3 + 1
    assert j == len(s) - 8 and s[i] == _COMP[s[j]] and s[p] == _COMP[s[q]]
    return s, (i, j, p, q)


def _loops():
    """(n5, n3): bulges of 2 .. 30 on either side, 1 x n loops with n = 3 .. 29 on either side"""
    out = []
    for u in range(2, 31):
        out += [(u, 0), (0, u)]
    for k in range(3, 30):
        out += [(1, k), (k, 1)]
    return out


def _phase_windows():
    """Every loop of _loops() at every ring phase: d = j - i = n5 + n3 + 2 h + hl + 1 of the closing pair, and 2 h + hl runs over 32 consecutive values
    (h = 6 .. 21, hl = 4, 5), so (d - 2) & 31 -- the ring row of the stacked pair, from which a job counts its rows down -- takes every value for every loop size:
    every position of every chunk across the seam.  The A padding in front (0 .. 31) moves the columns."""
    r = random.Random(1307)
    seqs, marks = [], []
    for n5, n3 in _loops():
        phases = set()
        for h in range(6, 22):
            for hl in (4, 5):
                pad = (len(seqs) * 7 + n5) % 32
                s, (i, j, p, q) = _construct(r, n5, n3, h, hl)
                phases.add((j - i - 2) & 31)
                seqs.append("A" * pad + s + "AAAA")
                marks.append((pad + i, pad + j, pad + p, pad + q))
        assert len(phases) == 32
    return seqs, marks


def _pairs(ss, start):
    """{0-based position: partner} of one structure line (start: 1-based column of its first character)"""
    st, pt = [], {}
    for x, c in enumerate(ss):
        if c == "(":
            st.append(x)
        elif c == ")":
            y = st.pop()
            pt[start - 1 + y] = start - 1 + x
            pt[start - 1 + x] = start - 1 + y
    return pt


def _realised(lines, mark):
    i, j, p, q = mark
    for ss, _, start in lines:
        pt = _pairs(ss, start)
        if pt.get(i) == j and pt.get(p) == q and not any(x in pt for x in range(i + 1, p)) and not any(x in pt for x in range(q + 1, j)):
            return True
    return False


def _check(seqs, span, a, b, want):
    assert len(a) == len(seqs) and len(b) == len(seqs) and len(want) == len(seqs)
    for k, s in enumerate(seqs):
        assert a[k]["status"] == 0 and b[k]["status"] == 0, (span, s, a[k]["status"], b[k]["status"])
        assert (a[k]["lines"], a[k]["mfe"]) == (b[k]["lines"], b[k]["mfe"]), (span, s)
        assert (a[k]["lines"], a[k]["mfe"]) == (want[k][0], want[k][1]), (span, s)


@pytest.mark.parametrize("span", [300, 40])
def test_every_loop_size_at_every_ring_phase(gpu_ctx, span):
    """3,584 windows of 38 .. 123 nt in one batch.  At span 300 the oracle must choose the planted loop in at least 95 % of them (3,583 of 3,584 on the
    CPU oracle), so that the test cannot pass on windows that never take the loop; at span 40 most closing pairs lie beyond the span: the same
    sequences on the first diagonals' code and its hand-over to the steady state, where the mirror rows are read as INF rows."""
    seqs, marks = _phase_windows()
    assert len(seqs) == 3584 and 34 <= min(map(len, seqs)) and max(map(len, seqs)) <= 130
    want = oracle_fold_all(seqs, span)
    if span == 300:
        hit = sum(_realised(w[0], m) for w, m in zip(want, marks))
        print("planted loop in the oracle's structure: %d of %d windows" % (hit, len(seqs)))
        assert hit >= 0.95 * len(seqs), (hit, len(seqs))
    a, n_dense, n_generic, b = _both_paths(gpu_ctx, seqs, span)
    print("span %d: %d windows left the pool path for the dense pass, %d for the generic kernel" % (span, n_dense, n_generic))
    assert n_generic == 0
    _check(seqs, span, a, b, want)


def _long_windows():
    """256 windows of 300 .. 350 nt, in (nearly) equal parts the three families of the fold micro-benchmark, each with one planted loop construct of
    _loops() spliced in at a random position; then 64 windows of 5 .. 60 nt, where the ramp-up reads INF rows and their mirrors."""
    import bench
    r = random.Random(2614)
    loops = _loops()
    fams = bench.micro_families(86, n=350, seed=77)
    seqs = []
    for k in range(256):
        mat = fams[k % 3][1]
        n = 300 + (k * 13) % 51
        s = mat[k // 3, :n].tobytes().decode()
        n5, n3 = loops[(k * 29) % len(loops)]
        c, _ = _construct(r, n5, n3, r.randint(6, 21), r.choice((4, 5)))
        o = r.randint(0, n - len(c))
        seqs.append(s[:o] + c + s[o + len(c):])
        assert len(seqs[-1]) == n
    lens = sorted(set(map(len, seqs)))
    assert lens[0] == 300 and lens[-1] == 350 and sum(len(s) >= 328 for s in seqs) >= 64
    acgu = "ACGU"
    for k in range(64):
        n = 5 + (k * 7) % 56
        seqs.append("".join(r.choice(acgu if k % 2 else "GGCCAU") for _ in range(n)))
    return seqs


def test_long_windows_and_ramp_up(gpu_ctx):
    """n = 300 .. 350: the diagonals take two blocks, lanes go ahead (one ring row later: the last mirror row), n >= 328 reaches the row ends; n = 5 .. 60: ramp-up only."""
    seqs = _long_windows()
    want = oracle_fold_all(seqs, 300)
    a, n_dense, n_generic, b = _both_paths(gpu_ctx, seqs, 300)
    print("%d of %d windows left the pool path for the dense pass, %d for the generic kernel" % (n_dense, len(seqs), n_generic))
    assert n_generic == 0
    _check(seqs, 300, a, b, want)
