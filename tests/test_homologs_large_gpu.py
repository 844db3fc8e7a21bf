"""The evaluation kernel of the homolog search (homolog_eval_kernel) past the 300 / 400-nt windows of tests/test_homologs_gpu.py: mature
and star intervals on every word boundary of a long stem, windows of 1,000 to 2,600 nt whose line lists take several rounds of 64, the natural re-fold
and capacity re-run, the opt-in LDS size and the staged text in global memory.  The truth is the restatement (tests/homolog_restatement.run) by exact
equality, through check() of tests/test_homologs_gpu.py; the inputs come from tests/homolog_restatement.py, and tests/test_homologs_cpu.py asserts on
the CPU that each of them reaches its path.  The cost of these tests is the CPU oracle's fold of the windows, not the device's."""
import pytest

from mir_prefer_amd import homologs
from tests import homolog_restatement as hr
from tests.test_homologs_gpu import check, device_run

pytestmark = pytest.mark.gpu


def test_word_boundary_sweep_on_long_stems(gpu_ctx, tmp_path):
    """1,339 placements of 810 queries on six stems of 96 .. 124 nt, P = 600: the mature and the star of the chosen structure lie across, begin at and
    end at the characters 32, 64, 96, 128, 160 and 192 of its line, with the mature in either arm (prime5 0 and 1) and up to seven words from its star."""
    contigs, queries, records, n_placements = hr.boundary_sweep()
    assert hr.coverage_gaps(hr.boundary_coverage(records)) == []          # before the device is called
    loci, stats = check(gpu_ctx, tmp_path, queries, contigs, v=0, P=hr.SWEEP["P"])
    assert stats["placements"] == n_placements and stats["passing"] == len(records)
    assert {x["arm"] for x in loci} == {"5p", "3p"} and any(x["total_dots"] for x in loci)


@pytest.fixture(scope="module")
def thousand(gpu_ctx, tmp_path_factory):
    """The 1,000-nt input on default capacities: (loci, table text), checked against the restatement."""
    contigs, queries, shapes = hr.thousand()
    assert max(w["lines"] for w in shapes) > hr.FOLD_LINES and max(w["usable"] for w in shapes) > 64 and hr.within_oracle_limits(shapes)
    loci, stats = check(gpu_ctx, tmp_path_factory.mktemp("thousand"), queries, contigs, v=hr.THOUSAND["v"], P=1000)
    assert stats["folds"] > 1 and stats["eval_reruns"] >= 1 and stats["eval_global_text"] == 0, stats
    assert len(loci) >= 4
    return loci, homologs.table(loci)


def test_windows_of_1000_nt_on_default_capacities(thousand):
    """Five windows of 999 nt with 92 .. 185 structure lines, up to 167 of them staged (three rounds of 64) and up to 89 structures (two rounds): the
    chunk is folded again for the lines past 96, and the windows with more than 48 usable lines are run again with grown capacities."""
    assert thousand[0]


@pytest.mark.parametrize("chunk", [0, 2])
def test_windows_of_1000_nt_with_the_text_in_global_memory(gpu_ctx, tmp_path, thousand, chunk):
    """The same call with room for so many staged lines that their words alone exceed 160 KB: every workgroup stages into its own slice of a global
    scratch area; with chunks of two placements, over three launches.  The output is the default run's byte for byte."""
    contigs, queries, shapes = hr.thousand()
    lines, caps = hr.global_text_caps(shapes)
    want_loci, want_stats = hr.run(queries, contigs, v=hr.THOUSAND["v"], P=1000)          # cached folds
    loci, counts, stats = device_run(gpu_ctx, tmp_path, queries, contigs, v=hr.THOUSAND["v"], P=1000, fold_lines=lines, eval_caps=caps, chunk=chunk)
    assert counts == want_stats
    assert loci == want_loci == thousand[0] and homologs.table(loci) == thousand[1]
    assert stats["eval_global_text"] >= (3 if chunk else 1) and stats["chunks"] == (3 if chunk else 1), stats


def test_windows_of_1500_nt_take_the_opt_in_lds_size(gpu_ctx, tmp_path):
    """Two windows of 1,499 nt (211 and 223 lines, 144 and 165 of them staged) on natural capacities: the last evaluation round asks for 80,480 bytes
    of dynamic LDS, above the 64 KB a kernel has without asking and below the 160 KB where the text moves to global memory."""
    contigs, queries, shapes = hr.fifteen_hundred()
    lds = hr.natural_launch(shapes)[3]
    assert lds == 80480 and 64 * 1024 < lds <= 160 * 1024
    _, stats = check(gpu_ctx, tmp_path, queries, contigs, v=hr.FIFTEEN_HUNDRED["v"], P=1500)
    assert stats["folds"] > 1 and stats["eval_reruns"] >= 1 and stats["eval_global_text"] == 0, stats


def test_widest_window_the_oracle_can_judge(gpu_ctx, tmp_path):
    """One window of 2,599 nt with 383 structure lines, P = 2600: the widest found whose line list stays within the 384 lines the oracle binding holds
    (at P = 2600 another seed gave 406 lines, at P = 2700 two seeds gave 407 and 411).  285 lines are staged, 218,752 bytes with the text in LDS, so
    the text lies in global memory on natural capacities.  The one slow case: the CPU oracle's fold of this window takes about 30 s."""
    contigs, queries, shapes = hr.widest()
    assert len(shapes) == 1 and hr.within_oracle_limits(shapes)
    _, stats = check(gpu_ctx, tmp_path, queries, contigs, v=hr.WIDEST["v"], P=hr.WIDEST_P)
    assert stats["placements"] == 1 and stats["eval_global_text"] >= 1, stats
