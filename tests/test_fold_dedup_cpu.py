"""The inputs of the fold-dedup tests, checked without a GPU: the CPU oracle's candidate stage writes the duplicates and near misses each case of
tests/fold_dedup_cases.py is there for, and the switch, the counter and the map are in the header, the binding and the integration notes."""
import os

import numpy as np
import pytest

from tests import fold_dedup_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(fc.CASES))
def test_case_has_the_duplicates_it_is_there_for(oracle, name):
    case = fc.CASES[name]()
    seqs = fc.window_seqs(fc.oracle_windows(oracle, case))
    assert fc.first_index_map(seqs).tolist() == fc.EXPECT[name][1]
    assert all(60 <= len(s) <= 130 for s in seqs) or case["L"] == 350


def test_the_generators_own_pattern(oracle):
    """a short locus with a peak on either strand: (+,L) (-,L) (+,L) (+,R) (-,L) (-,R)"""
    win = fc.oracle_windows(oracle, fc.short_both_strands())
    assert [(int(w["strand"]), int(w["tag"])) for w in win["windows"]] == [(0, 1), (1, 1), (0, 1), (0, 2), (1, 1), (1, 2)]


def test_near_misses_are_near(oracle):
    seqs = fc.window_seqs(fc.oracle_windows(oracle, fc.planted_segment()))
    assert seqs[5] != seqs[1] and seqs[5][:-1] == seqs[1][:-1]                        # the last base differs
    assert len(seqs[11]) < len(seqs[1]) and seqs[1].startswith(seqs[11])              # clipped at the contig end: a prefix
    assert seqs[6] != seqs[0] and seqs[6].upper() == seqs[0] and seqs[7].upper() == seqs[1]      # soft-masked
    assert len({len(c[1]) for c in fc.planted_segment()["contigs"]}) == 2


def test_line_capacity_case_overflows(oracle):
    case = fc.tandem_over_line_capacity()
    seqs = fc.window_seqs(fc.oracle_windows(oracle, case))
    for model in ("vienna-2.1.2", "vienna-1.8.5"):
        assert all(len(oracle.lfold(s, case["span"], model=model)["lines"]) > case["max_lines"] for s in seqs[:4])


def test_entry_points_are_declared_everywhere():
    from mir_prefer_amd import capi
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mirp_set_fold_dedup", "mirp_last_fold_duplicates", "mirp_get_fold_duplicates", "mirp_set_fold_dedup_hash_bits"):
        assert name + "(" in header and name in notes, name
    for method in ("set_fold_dedup", "last_fold_duplicates", "get_fold_duplicates", "set_fold_dedup_hash_bits"):
        assert callable(getattr(capi.Context, method))
    assert capi.ABI_VERSION == 17      # entries are added only
    assert np.array_equal(fc.first_index_map([b"AC", b"AC", b"ac", b"A", b"AC"]), [-1, 0, -1, -1, 0])
