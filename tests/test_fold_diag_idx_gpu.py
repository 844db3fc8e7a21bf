"""GPU parity of the default model's candidate-pool pass on what its diagonal loop does once per barrier interval (round 16): the buffers it turns with
d % 3, d % 6 and d & 31, the intervals whose list of paired cells is empty, and the lane fill from the first interior-loop diagonal on (lanes of
diagonal d + 1 ride in the last block of diagonal d although loop sizes up to 30 do not all exist yet: they read ring rows that are still INF).
Every case requires candidate-pool path == dense path (set_fold_split_path(1)) == CPU oracle exactly -- every printed line, the MFE, the status --
and that no window leaves the pool path (last_fold_dense() == last_fold_fallbacks() == 0).  The families and the properties that make them cases are
in tests/test_fold_diag_idx_cpu.py, which checks those properties without a GPU.

Which case a build switch of the fill kernel changes the code path of: MIRP_RAMP_MIX (lane fill on the first diagonals, the only switch this round
left in the tree) -- every window with paired cells on two consecutive diagonals in 6 .. 35, i.e. all cases but the poly-A / ends-only one; the whole
fold of the 30 .. 36 nt windows of test_whole_fold_on_the_first_diagonals."""
import pytest

from tests import test_fold_diag_idx_cpu as fam
from tests.test_fold_two_per_cu_gpu import _both_paths
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu


def _exact(gpu_ctx, seqs, span, want):
    a, n_dense, n_generic, b = _both_paths(gpu_ctx, seqs, span)
    assert (n_dense, n_generic) == (0, 0), (span, n_dense, n_generic)
    assert len(a) == len(seqs) and len(b) == len(seqs) and len(want) == len(seqs)
    for k, s in enumerate(seqs):
        assert a[k]["status"] == 0 and b[k]["status"] == 0, (span, s, a[k]["status"], b[k]["status"])
        assert (a[k]["lines"], a[k]["mfe"]) == (b[k]["lines"], b[k]["mfe"]), (span, s)
        assert (a[k]["lines"], a[k]["mfe"]) == (want[k][0], want[k][1]), (span, s)
    return a


@pytest.fixture(scope="module")
def short_oracle():
    seqs = fam.short_windows()
    return seqs, {span: oracle_fold_all(seqs, span) for span in fam.SHORT_SPANS}


@pytest.mark.parametrize("span", fam.SHORT_SPANS)
def test_short_windows_end_on_every_early_diagonal(gpu_ctx, short_oracle, span):
    """n = 5 .. 80: the fill ends on every diagonal 4 .. 79 (spans 6 .. 12: on 5 .. 11, span 40: on 39), i.e. before, on and past the first wrap of
    every buffer cycle, with and without a mirror row, and with the lane fill switched off by d + 1 > D on every one of them."""
    seqs, want = short_oracle
    _exact(gpu_ctx, seqs, span, want[span])


@pytest.fixture(scope="module")
def long_oracle():
    seqs = fam.long_windows()
    return seqs, {span: oracle_fold_all(seqs, span) for span in (120, 300)}


@pytest.mark.parametrize("span", [120, 300])
def test_long_windows(gpu_ctx, long_oracle, span):
    """n = 197 .. 200 and 320 .. 350, uniform and G/U-only: the cell count crosses multiples of 64 on the first diagonals, three blocks on them at 350 nt"""
    seqs, want = long_oracle
    _exact(gpu_ctx, seqs, span, want[span])


def test_unlike_windows_back_to_back(gpu_ctx):
    """2,560 windows in the order long GC-rich, poly-A, 5 nt, long uniform: several windows per workgroup, each of which sets up again what the
    diagonal loop carries (cells that went ahead, list lengths, the split pool's snapshot)."""
    base = fam.quadruples()
    want = oracle_fold_all(base, 300)
    _exact(gpu_ctx, base * 40, 300, want * 40)


def test_windows_without_a_paired_cell(gpu_ctx):
    """poly-A and ends-only windows of 64 .. 350 nt: every interval is empty"""
    seqs = fam.unpaired_windows()
    _exact(gpu_ctx, seqs, 300, oracle_fold_all(seqs, 300))


@pytest.fixture(scope="module")
def gu_oracle():
    seqs = fam.gu_windows()
    return seqs, oracle_fold_all(seqs, 300)


def test_gu_only_windows(gpu_ctx, gu_oracle):
    """G/U-only windows of 64 .. 350 nt: up to three blocks per interval, lanes going ahead on every one of the first diagonals"""
    seqs, want = gu_oracle
    _exact(gpu_ctx, seqs, 300, want)


def test_whole_fold_on_the_first_diagonals(gpu_ctx):
    """uniform windows of 30 .. 45 nt at spans 300 and 40"""
    seqs = fam.rampup_windows()
    for span in (300, 40):
        _exact(gpu_ctx, seqs, span, oracle_fold_all(seqs, span))


def test_two_folds_back_to_back_on_one_context(gpu_ctx, gu_oracle):
    """the second fold of a context starts from what the first one left in the archive, the control block and the lists"""
    seqs, want = gu_oracle
    first = gpu_ctx.fold_batch(seqs[-64:], 300)
    other = gpu_ctx.fold_batch(fam.unpaired_windows()[-64:], 300)
    second = gpu_ctx.fold_batch(seqs[-64:], 300)
    assert gpu_ctx.last_fold_dense() == 0 and gpu_ctx.last_fold_fallbacks() == 0
    assert len(other) == 64
    for k in range(64):
        assert first[k]["status"] == 0 and second[k]["status"] == 0
        assert (first[k]["lines"], first[k]["mfe"]) == (second[k]["lines"], second[k]["mfe"]) == (want[-64 + k][0], want[-64 + k][1]), seqs[-64 + k]
