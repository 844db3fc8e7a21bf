"""GPU parity of the default model's candidate-pool pass after round 12: a wave's two interior-loop jobs run in one pass over the blocks of 64 paired
cells (one list read, one decode of the loop parameters and one LDS atomic per block), and a wave that owns no cell of a diagonal branches round
phase B.  Every case compares the candidate-pool path with the dense path (set_fold_split_path(1)) and with the CPU oracle, exactly: every printed
line (structure, energy, start), the MFE and the status.

What the cases aim at:
  * 0, 1, 2 and 3 blocks per interval inside one window (half of the cells pair in a G/U-only or G/C-only window: up to 173 paired cells on a
    diagonal at n = 350), no paired cell at all (poly-A) and a pair at the two ends only;
  * intervals whose whole list went ahead in the previous one (rem == 0, done > 0: only the stacked-pair fix-up runs), and a fill that stops while
    cells still go ahead (spans 40 and 120: `mix` switches off at d + 1 > D);
  * diagonals on which the cell count n - d crosses a multiple of 64, where the last phase-B wave loses its last cell and takes the new branch;
  * several windows of very different shape folded by one workgroup one after the other (what a workgroup carries from diagonal to diagonal must
    be set up again by every window)."""
import random

import pytest

from tests.test_fold_two_per_cu_gpu import _both_paths
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu

LENGTHS = (64, 65, 129, 130, 257, 258, 350)


def _two_letter(seed, ab, n):
    r = random.Random(seed)
    return "".join(r.choice(ab) for _ in range(n))


def _ends_only(n):
    """a window whose only possible pair joins its two ends"""
    return "G" + "A" * (n - 2) + "C"


def _family(n):
    """(name, window) of length n: three G/U-only and three G/C-only random windows, poly-A, a pair at the two ends only"""
    out = [("GU-%d" % k, _two_letter(1200 + 7 * n + k, "GU", n)) for k in range(3)]
    out += [("GC-%d" % k, _two_letter(2200 + 7 * n + k, "GC", n)) for k in range(3)]
    return out + [("polyA", "A" * n), ("ends", _ends_only(n))]


def _same_as_dense_and_oracle(seqs, span, a, b, want):
    assert len(a) == len(seqs) and len(b) == len(seqs) and len(want) == len(seqs)
    for k, s in enumerate(seqs):
        assert a[k]["status"] == 0 and b[k]["status"] == 0, (span, s, a[k]["status"], b[k]["status"])
        assert (a[k]["lines"], a[k]["mfe"]) == (b[k]["lines"], b[k]["mfe"]), (span, s)
        assert (a[k]["lines"], a[k]["mfe"]) == (want[k][0], want[k][1]), (span, s)


@pytest.fixture(scope="module")
def families():
    return {n: _family(n) for n in LENGTHS}


@pytest.fixture(scope="module")
def family_oracle(families):
    """span -> length -> [(lines, mfe)]: one oracle run per span over all lengths"""
    flat = [s for n in LENGTHS for _, s in families[n]]
    out = {}
    for span in (300, 120, 40):
        want = oracle_fold_all(flat, span)
        out[span], at = {}, 0
        for n in LENGTHS:
            out[span][n] = want[at:at + len(families[n])]
            at += len(families[n])
    return out


@pytest.mark.parametrize("span", [300, 120, 40])
def test_block_counts_zero_to_three(gpu_ctx, families, family_oracle, span):
    """Every length on its own, so that the windows the pool pass kept are counted per length: a length all of whose windows went to the dense or
    the generic kernel would prove nothing about the pool pass."""
    for n in LENGTHS:
        seqs = [s for _, s in families[n]]
        a, n_dense, n_generic, b = _both_paths(gpu_ctx, seqs, span)
        print("span %d, n = %d: %d of %d windows handed to the dense kernel, %d to the generic kernel" % (span, n, n_dense, len(seqs), n_generic))
        # poly-A and the ends-only window have no split candidate and tiny energies: the two-letter windows must not all leave either
        assert n_dense + n_generic <= len(seqs) - 3, (span, n, n_dense, n_generic)
        _same_as_dense_and_oracle(seqs, span, a, b, family_oracle[span][n])


def test_cell_count_crosses_a_multiple_of_64(gpu_ctx, oracle):
    """n = 197 .. 200: n - d crosses 192 on the diagonals 5 .. 8 (every span 6 .. 40 ends the fill on or just behind them), 128 on 69 .. 72 (span 120)
    and 64 on 133 .. 136 (span 300)."""
    r = random.Random(1964)
    seqs = []
    for n in (197, 198, 199, 200):
        seqs += [_two_letter(r.randrange(1 << 30), "GU", n), _two_letter(r.randrange(1 << 30), "ACGU", n), _two_letter(r.randrange(1 << 30), "GC", n)]
    kept = 0
    for span in list(range(6, 41)) + [120, 300]:
        a, n_dense, n_generic, b = _both_paths(gpu_ctx, seqs, span)
        kept += len(seqs) - n_dense - n_generic
        want = []
        for s in seqs:
            w = oracle.lfold(s, span)
            want.append((w["lines"], w["mfe"]))
        _same_as_dense_and_oracle(seqs, span, a, b, want)
    print("%d of %d folds stayed on the pool path" % (kept, 37 * len(seqs)))
    assert kept >= 37 * len(seqs) // 2


@pytest.fixture(scope="module")
def quadruples():
    """16 x (long GC-rich, poly-A, 5 nt, long mixed) and the oracle's folds of these 64 windows"""
    r = random.Random(412)
    seqs = []
    for k in range(16):
        n1, n2 = r.randint(300, 350), r.randint(280, 350)
        gc_rich = "".join(r.choice("GC") if r.random() < 0.8 else r.choice("AU") for _ in range(n1))
        seqs += [gc_rich, "A" * r.randint(150, 350), _two_letter(r.randrange(1 << 30), "ACGU", 5), _two_letter(r.randrange(1 << 30), "ACGU", n2)]
    return seqs, oracle_fold_all(seqs, 300)


def test_windows_of_different_shape_back_to_back(gpu_ctx, quadruples):
    """2,560 windows in the order long GC-rich, poly-A, 5 nt, long, ...: several times as many as the chip holds workgroups of the pool pass, which
    draw them in order from one counter, so every workgroup folds windows of unlike shape one after the other.  (A batch of four windows capped by
    set_fold_capacity(4) is folded too, as a second grid geometry: its launch has four workgroups, one per window -- the capacity bounds the
    windows of a launch, not its grid.)"""
    base, want = quadruples
    seqs = base * 40
    a, n_dense, n_generic, b = _both_paths(gpu_ctx, seqs, 300)
    print("%d of %d windows handed to the dense kernel, %d to the generic kernel" % (n_dense, len(seqs), n_generic))
    assert n_dense + n_generic <= len(seqs) // 2
    _same_as_dense_and_oracle(seqs, 300, a, b, want * 40)
    try:
        gpu_ctx.set_fold_overlap(0)
        gpu_ctx.set_fold_capacity(4)
        for k in range(0, 16, 4):
            a4, _, _, b4 = _both_paths(gpu_ctx, base[k:k + 4], 300)
            _same_as_dense_and_oracle(base[k:k + 4], 300, a4, b4, want[k:k + 4])
    finally:
        gpu_ctx.set_fold_capacity(0)
        gpu_ctx.set_fold_overlap(-1)
