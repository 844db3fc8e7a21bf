"""GPU parity of the fill kernel's first interior-loop diagonals (6 .. 35: not every loop size admissible yet), which the candidate-pool pass of the
default model runs on the unchecked steady-state code: a candidate whose inner pair would lie on a diagonal < 4 reads an INF ring row instead of being
skipped.  What that rests on is checked here against the CPU oracle and against the dense kernel (set_fold_split_path(1), which keeps the checked
code): the per-window INF initialisation of the ring, the ring's row stride (reads behind a row's last column), the special-hairpin energies in a
region of their own, and the padded pair-code arrays.  Equality is exact: every line (structure text, energy, start column), the MFE and the status."""
import os
import random
import re

import pytest

from tests import seqgen
from tests.test_fold_two_per_cu_gpu import _both_paths, _every_length
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu

MODELS = ["vienna-2.1.2", "vienna-1.8.5"]


def _check(seqs, span, a, b, model="vienna-2.1.2"):
    assert len(a) == len(seqs) and len(b) == len(seqs)
    want = oracle_fold_all(seqs, span, model)
    for k, s in enumerate(seqs):
        assert a[k]["status"] == 0 and b[k]["status"] == 0, (span, s, a[k]["status"], b[k]["status"])
        assert (a[k]["lines"], a[k]["mfe"]) == (b[k]["lines"], b[k]["mfe"]), (model, span, s)
        assert (a[k]["lines"], a[k]["mfe"]) == (want[k][0], want[k][1]), (model, span, s)


def _exact(r, n):
    w = seqgen.window(r, n, n)
    return w[:n] if len(w) >= n else w + "A" * (n - len(w))


@pytest.mark.parametrize("span", [7, 8, 12, 20, 35, 36, 37])
def test_folds_that_are_all_ramp_up(gpu_ctx, span):
    """One window of every length 5 .. 60.  With span <= 36 the largest pair distance is 35: no diagonal reaches um == MAXLOOP, the whole fold runs on
    the first diagonals' code; 36 and 37 are the hand-over to the steady state."""
    r = random.Random(4100 + span)
    seqs = [_exact(r, n) for n in range(5, 61)]
    a, _, n_generic, b = _both_paths(gpu_ctx, seqs, span)
    assert n_generic == 0
    _check(seqs, span, a, b)


def test_every_length_at_span_40(gpu_ctx):
    """Every length 5 .. 350 at span 40: thirty ramp-up diagonals and four steady-state ones at every window length, i.e. at every distance of the last
    columns from the end of a ring row."""
    seqs = _every_length(4140)
    a, _, n_generic, b = _both_paths(gpu_ctx, seqs, 40)
    assert n_generic == 0
    _check(seqs, 40, a, b)


def _row_end_window(r, n):
    """5' end: GAAAC / CUUUG units over the first 30 nt, so that diagonal 4 has finite cells in columns 1 .. 23 (ring row 4 follows the row that stands for
    "diagonal 3").  3' end: the last 45 nt are G...(4-20 nt)...C stems, so that paired cells with i >= 323 exist on the diagonals 6 .. 26, whose lanes
    read up to 32 columns behind i."""
    head = "".join(r.choice(["GAAAC", "CUUUG"]) for _ in range(6))
    tail = ""
    while len(tail) < 45:
        k, loop = r.randint(1, 3), r.randint(4, 20)
        piece = "G" * k + "".join(r.choice("AU") for _ in range(loop)) + "C" * k
        tail += piece if len(tail) + len(piece) <= 45 else "A" * (45 - len(tail))
    mid = _exact(r, n - 75)
    s = head + mid + tail
    assert len(s) == n
    return s


@pytest.mark.parametrize("span", [300, 30])
def test_row_end_reads_on_the_first_diagonals(gpu_ctx, span):
    """Lengths 323 .. 350, three windows each: on the first diagonals a lane of the last columns reads behind column n, at the ring's former stride
    (354 shorts) into the head of the next row for n >= 328."""
    r = random.Random(4200 + span)
    seqs = [_row_end_window(r, n) for n in range(323, 351) for _ in range(3)]
    a, _, _, b = _both_paths(gpu_ctx, seqs, span)
    _check(seqs, span, a, b)


def _special_loops():
    """The tri-, tetra- and hexaloop strings (closing pair included) of the Turner-2004 parameter header."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mir-prefer_amd", "csrc", "energy_params_t2004.h")
    with open(path) as f:
        text = f.read()
    loops = sorted(set(m for m in re.findall(r'"([ACGU]{5,8})[ "\\]', text) if len(m) in (5, 6, 8)))
    assert {len(m) for m in loops} == {5, 6, 8}, loops
    return loops


def _special_windows():
    r = random.Random(4300)
    loops = _special_loops()
    seqs = []
    for n in [r.randint(20, 120) for _ in range(200)] + [r.randint(300, 350) for _ in range(50)]:
        s = list(_exact(r, n))
        starts = [1, 2] + list(range(n - 7, n - 3)) + [r.randint(3, n - 8) for _ in range(max(2, n // 25))]
        r.shuffle(starts)
        for p in starts[:r.randint(2, len(starts))]:      # 1-based start; a loop that does not fit is cut at the window's end
            m = r.choice(loops)
            for t, ch in enumerate(m):
                if p + t <= n:
                    s[p - 1 + t] = ch
        seqs.append("".join(s))
    return seqs


@pytest.mark.parametrize("model", MODELS)
def test_special_hairpins(gpu_ctx, model):
    """200 windows of 20 .. 120 nt and 50 of 300 .. 350 nt seeded with special hairpin loops at positions 1, 2, n-7 .. n-4 and at random interior
    positions: their energies by start position no longer live in ring rows 29 - 31 where the first diagonals now read INF."""
    seqs = _special_windows()
    try:
        gpu_ctx.set_fold_model(model)
        a, _, _, b = _both_paths(gpu_ctx, seqs, 300)
    finally:
        gpu_ctx.set_fold_model("vienna-2.1.2")
    _check(seqs, 300, a, b, model)


def test_back_to_back_windows_in_one_workgroup(gpu_ctx):
    """2,048 windows of mixed length 5 .. 350 in random order: every workgroup folds several, a long one followed by a short one must find no ring row of
    its predecessor (the INF initialisation is per window)."""
    seqs = seqgen.windows(4400, 2048, 5, 350)
    a, _, _, b = _both_paths(gpu_ctx, seqs, 300)
    _check(seqs, 300, a, b)
