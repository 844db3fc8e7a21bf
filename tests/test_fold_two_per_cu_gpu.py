"""GPU parity of the default model's candidate-pool pass in its two-windows-per-CU form (512-thread workgroups, fML triangle in the archive slab,
multiloop-split operands gathered from there): against the CPU oracle and against the dense kernel (set_fold_split_path(1)), which keeps the
triangle in LDS.  Equality is exact: every line (structure text, energy, start column), the MFE and the status."""
import random

import pytest

from tests import seqgen
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu


def _both_paths(gpu_ctx, seqs, span, max_lines=352):
    """(candidate-pool pass, windows it handed to the dense kernel, windows handed to the generic kernel, dense kernel alone)"""
    a = gpu_ctx.fold_batch(seqs, span, max_lines=max_lines)
    n_dense, n_generic = gpu_ctx.last_fold_dense(), gpu_ctx.last_fold_fallbacks()
    try:
        gpu_ctx.set_fold_split_path(1)
        b = gpu_ctx.fold_batch(seqs, span, max_lines=max_lines)
    finally:
        gpu_ctx.set_fold_split_path(0)
    return a, n_dense, n_generic, b


def _check(seqs, span, a, b):
    assert len(a) == len(seqs) and len(b) == len(seqs)
    want = oracle_fold_all(seqs, span)
    for k, s in enumerate(seqs):
        assert a[k]["status"] == 0 and b[k]["status"] == 0, (span, s, a[k]["status"], b[k]["status"])
        assert (a[k]["lines"], a[k]["mfe"]) == (b[k]["lines"], b[k]["mfe"]), (span, s)
        assert (a[k]["lines"], a[k]["mfe"]) == (want[k][0], want[k][1]), (span, s)


def _every_length(seed):
    r = random.Random(seed)
    seqs = []
    for n in range(5, 351):
        w = seqgen.window(r, n, n)
        seqs.append(w[:n] if len(w) >= n else w + "A" * (n - len(w)))
    assert [len(s) for s in seqs] == list(range(5, 351))
    return seqs


@pytest.mark.parametrize("span", [300, 120])
def test_every_window_length(gpu_ctx, span):
    """One window of every length 5..350: every length of the two-diagonal fML ring, every row-block and tile edge of the archive the fill kernel now
    writes fML to cell by cell, and (span 120) a fill that stops long before the window's last diagonal."""
    seqs = _every_length(777 + span)
    a, _, n_generic, b = _both_paths(gpu_ctx, seqs, span)
    assert n_generic == 0
    _check(seqs, span, a, b)


def test_stress_families_and_the_dense_hand_off(gpu_ctx):
    """The five sequence families of the differential stress plus full-length tandem repeats: a pool that overflows must still hand its window to the dense
    kernel (counted by last_fold_dense()), never drop candidates."""
    r = random.Random(512)
    seqs = [seqgen.stress_family(r, i % 5) for i in range(600)]
    seqs += [(u * 350)[:n] for u in ("AU", "GU", "AAUU", "ACGU", "GGGUUC", "AGU") for n in (350, 349, 301, 256)]
    a, n_dense, _, b = _both_paths(gpu_ctx, seqs, 300)
    assert n_dense > 0
    _check(seqs, 300, a, b)


def test_gc_windows_leave_the_16_bit_range(gpu_ctx):
    """GC-only windows whose energies leave the 16-bit tables are flagged by the fill kernel and folded by the generic kernel; their neighbours in the batch are not."""
    seqs = ["G" * 150 + "C" * 150, "G" * 170 + "AAAA" + "C" * 170, "GC" * 150] + seqgen.windows(91, 13, 200, 350) + ["G" * 160 + "UUCG" + "C" * 160]
    a, _, n_generic, b = _both_paths(gpu_ctx, seqs, 300)
    assert 1 <= n_generic < len(seqs)
    _check(seqs, 300, a, b)


def test_large_mixed_batch_keeps_both_workgroups_of_a_cu_on_different_lengths(gpu_ctx):
    """4 x 256 x 2 windows of mixed length 5..350 in random order: more than twice as many as the chip holds workgroups, so that the two resident
    workgroups of every CU fold windows of different lengths side by side and pick up new ones at different times."""
    seqs = seqgen.windows(20488, 4 * 256 * 2, 5, 350)
    a, _, _, b = _both_paths(gpu_ctx, seqs, 300)
    _check(seqs, 300, a, b)
