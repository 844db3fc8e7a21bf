"""GPU tests of the pieces in which text leaves the device: site_finish_pass (site_lines.h; targets, mimics) launches site_emit_kernel once per piece
of whole lines with the first index of the piece, and mirp_download_text (mirp_ctx.h; align, trim) copies a batch's text piece by piece.  The piece
is 1 GiB, so a plain run never has a second one; mirp_set_text_piece lowers it here, and mirp_text_pieces_last tells how many pieces a call handed
to its output.

Every search runs on one small input of the existing tests: first at the default piece, where the bytes must be those of that test's restatement,
then at piece sizes 1, 7, L - 1, L, L + 1 (L = the length of the first line, of the header and of the first site or record), 3 L and 4,096,
where they must not change by a byte.  The site searches run again with -k 1 and -k 3 (cut keys are zero-length lines, which then sit on piece
boundaries) and in at least three passes with a piece of 7 bytes.  The number of pieces is checked as well: for the site searches against the
greedy walk of tests/test_text_pieces_cpu.py over the line lengths (every line at 1 and 7, at least two pieces at L), for align and trim
ceil(bytes / piece).  targets -e and -u are the ones whose line functor reads per-key arrays by the global index of the key."""
import multiprocessing

import numpy as np
import pytest

from tests.mimic_restatement import restate_files as mimic_restate_files
from tests.test_align_cpu import normalise_pg, sam_bytes
from tests.test_align_place_gpu import mixture                                                        # noqa: F401  (fixture)
from tests.test_duplex_gpu import OPTIONS as ENERGY_OPTIONS, energy_input, energy_want, fold_many     # noqa: F401  (fixtures)
from tests.test_mimics_gpu import small as mimics_small                                               # noqa: F401  (fixture)
from tests.test_targets_bulge_gpu import _restate_files as bulge_restate_files, small as bulge_small  # noqa: F401  (fixture)
from tests.test_targets_cpu import restate_files
from tests.test_targets_gpu import small as targets_small                                             # noqa: F401  (fixture)
from tests.test_targets_upe_gpu import upe_input, windows_of                                          # noqa: F401  (fixture)
from tests.test_text_pieces_cpu import restate as pieces_of
from tests.test_trim_cpu import ILLUMINA, restate_trim, to_fastq
from tests.test_trim_gpu import _edge_reads
from tests.test_unpaired_cpu import format_upe, upe_job

pytestmark = pytest.mark.gpu


def line_sizes(data):
    """the lengths of the lines after the header, newline included"""
    return [len(ln) + 1 for ln in data.split(b"\n")[1:-1]]


def n_pieces(piece, sizes):
    return sum(1 for _, _, ln in pieces_of(piece, sizes) if ln > 0)


def check_site_search(ctx, scan, want, want_k=None, cap=40):
    """scan(**kw) -> (bytes, result) of one search, kw = max_sites; want = the restatement's bytes of the run without -k, want_k(k) of a run with -k."""
    try:
        got, res = scan()
        assert got == want
        sizes = line_sizes(want)
        n, head, L = len(sizes), len(want.split(b"\n")[0]) + 1, sizes[0]
        assert res["sites"] == n >= 8 and res["passes"] == 1 and ctx.text_pieces_last() == 1 and 7 < min(sizes)
        count = {}
        for piece in sorted({1, 7, head - 1, head, head + 1, L - 1, L, L + 1, 3 * L, 4096}):
            ctx.set_text_piece(piece)
            got, res = scan()
            assert got == want, piece
            count[piece] = ctx.text_pieces_last()
            assert count[piece] == n_pieces(piece, sizes), (piece, count)
        assert count[1] == count[7] == n and count[L] >= 2 and count[head] >= 2 and 1 < count[3 * L] < n, count
        # -k: the keys it cuts are zero-length lines between, before and after the pieces
        cut = {}
        for k in (1, 3):
            ctx.set_text_piece(0)
            cut[k], res0 = scan(max_sites=k)
            assert want_k is None or cut[k] == want_k(k)
            ksizes = line_sizes(cut[k])
            assert res0["sites"] == len(ksizes) <= n and (k > 1 or len(ksizes) < n) and set(cut[k].split(b"\n")) <= set(want.split(b"\n")) and ctx.text_pieces_last() == 1
            for piece in (1, 7, L, 3 * L, 4096):
                ctx.set_text_piece(piece)
                got, res = scan(max_sites=k)
                assert got == cut[k], (k, piece)
                assert ctx.text_pieces_last() == n_pieces(piece, ksizes) and (piece > 7 or ctx.text_pieces_last() == res["sites"]), (k, piece)
        # several passes: the `emitted` counters of -k and the piece loop across passes
        ctx.set_target_capacity(cap)
        ctx.set_text_piece(7)
        got, res = scan()
        assert got == want and res["passes"] >= 3 and ctx.text_pieces_last() == n, res
        for k in (1, 3):
            got, res = scan(max_sites=k)
            assert got == cut[k] and ctx.text_pieces_last() == res["sites"] == len(line_sizes(cut[k])), (k, res)
    finally:
        ctx.set_text_piece(0)
        ctx.set_target_capacity(0)


def _targets(ctx, tmp_path, mirna, targets, **fixed):
    def scan(**kw):
        out = tmp_path / "out.tsv"
        res = ctx.target_scan(str(mirna), [str(p) for p in targets], str(out), **fixed, **kw)
        return out.read_bytes(), res
    return scan


def test_targets_plain(gpu_ctx, targets_small, tmp_path):
    d = targets_small
    paths = [d / "t1.fa", d / "t2.fa"]
    check_site_search(gpu_ctx, _targets(gpu_ctx, tmp_path, d / "m.fa", paths, max_half_score=8, both_strands=True),
                      restate_files(d / "m.fa", paths, max_half=8, both=True), lambda k: restate_files(d / "m.fa", paths, max_half=8, both=True, k=k))


def test_targets_bulge(gpu_ctx, bulge_small, tmp_path):
    d = bulge_small
    paths = [d / "t1.fa", d / "t2.fa"]
    check_site_search(gpu_ctx, _targets(gpu_ctx, tmp_path, d / "m.fa", paths, max_half_score=10, both_strands=True, bulge=True),
                      bulge_restate_files(d / "m.fa", paths, 10, True), lambda k: bulge_restate_files(d / "m.fa", paths, 10, True, False, k))


def test_targets_energy(gpu_ctx, energy_input, energy_want, tmp_path):
    """-e: TgLine reads the fold of key i of the pass (tg_emfe, tg_ema, tg_emb) by the index site_emit_kernel hands it"""
    d, _ = energy_input
    assert ENERGY_OPTIONS[0] == {}
    check_site_search(gpu_ctx, _targets(gpu_ctx, tmp_path, d / "m.fa", [d / "t1.fa", d / "t2.fa"], energy=True), energy_want[0], cap=4)


@pytest.fixture(scope="module")
def upe_want(upe_input):
    """the expected file of targets -b -u on upe_input: the lines of the plain restatement, each with the restated accessibility of its window"""
    d, contigs = upe_input
    plain = restate_files(d / "m.fa", [d / "t.fa"], max_half=8, both=True)
    jobs = windows_of(plain, contigs)
    with multiprocessing.get_context("spawn").Pool(14) as pool:
        upe = pool.map(upe_job, sorted(set(jobs)), chunksize=1)
    column = {j: format_upe(r["upe"]).encode() for j, r in zip(sorted(set(jobs)), upe)}
    lines = plain.split(b"\n")[:-1]
    return b"".join([lines[0] + b"\tupe\n"] + [ln + b"\t" + column[j] + b"\n" for ln, j in zip(lines[1:], jobs)])


def test_targets_accessibility(gpu_ctx, upe_input, upe_want, tmp_path):
    """-u: TgLine reads the accessibility of key i of the pass (tg_upe) by the index site_emit_kernel hands it"""
    d, _ = upe_input
    values = [ln.split(b"\t")[-1] for ln in upe_want.split(b"\n")[1:-1]]
    assert len(set(values)) >= 6                                                              # a line with another key's value would show
    check_site_search(gpu_ctx, _targets(gpu_ctx, tmp_path, d / "m.fa", [d / "t.fa"], both_strands=True, accessibility=True), upe_want, cap=2)


def test_mimics(gpu_ctx, mimics_small, tmp_path):
    d = mimics_small
    paths = [d / "t1.fa", d / "t2.fa"]

    def scan(**kw):
        out = tmp_path / "out.tsv"
        res = gpu_ctx.mimic_scan(str(d / "m.fa"), [str(p) for p in paths], str(out), max_imperfect=3, loop_len=3, both_strands=True, **kw)
        return out.read_bytes(), res
    check_site_search(gpu_ctx, scan, mimic_restate_files(d / "m.fa", paths, n=3, G=3, both=True),
                      lambda k: mimic_restate_files(d / "m.fa", paths, n=3, G=3, both=True, k=k), cap=8)


# ---------------------------------------------------------------------------------------------------- align, trim: pieces cut at any byte
def check_stream(ctx, run, want, body_of):
    """run() -> the bytes of the file; want: the restatement's; body_of(bytes) = the bytes that went through mirp_download_text"""
    try:
        assert run() == want and ctx.text_pieces_last() == 1
        body = body_of(want)
        lines = want.split(b"\n")
        first = len(lines[0]) + 1
        L = len(next(ln for ln in lines if not ln.startswith(b"@"))) + 1
        assert body > 2 * 4096
        for piece in sorted({1, 7, first - 1, first, first + 1, L - 1, L, L + 1, 4096} - {0}):
            ctx.set_text_piece(piece)
            assert run() == want, piece
            assert ctx.text_pieces_last() == (body + piece - 1) // piece, piece
    finally:
        ctx.set_text_piece(0)


def _sam_body(data):
    return len(data) - sum(len(ln) + 1 for ln in data.split(b"\n") if ln.startswith(b"@"))


def test_align_plain(gpu_ctx, mixture):
    gpu_ctx.align_index([mixture.ref])
    out = str(mixture.dir / "pieces.sam")

    def run():
        gpu_ctx.align_reads(mixture.reads_path, out, "x", v=1, k=20, m=0)
        assert gpu_ctx.align_last_batches() == 1
        return normalise_pg(open(out, "rb").read())
    check_stream(gpu_ctx, run, sam_bytes(mixture.names, mixture.seqs, mixture.reads, mixture.hits, 1, 20, 0, False), _sam_body)


def test_align_placed(gpu_ctx, mixture):
    gpu_ctx.align_index([mixture.ref])
    out = str(mixture.dir / "pieces_placed.sam")

    def run():
        gpu_ctx.align_reads(mixture.reads_path, out, "x", v=1, k=20, m=50, place="u", window=50, seed=7)
        assert gpu_ctx.align_last_batches() == 1
        return normalise_pg(open(out, "rb").read())
    check_stream(gpu_ctx, run, mixture.want(1, 50, 50, 7, "u")[0], _sam_body)


def test_trim(gpu_ctx, tmp_path):
    data = to_fastq(_edge_reads(np.random.RandomState(1)))
    out = tmp_path / "in.fastq.trimmed.fa"

    def run():
        gpu_ctx.trim_reads(data, "in.fastq", str(out), adapter=ILLUMINA)
        return out.read_bytes()
    check_stream(gpu_ctx, run, restate_trim(data, adapter=ILLUMINA)[0], len)


def test_the_piece_knob(gpu_ctx):
    from mir_prefer_amd.capi import MirpError
    with pytest.raises(MirpError, match=r"mirp_set_text_piece failed \(-1\)"):
        gpu_ctx.set_text_piece(-1)
    gpu_ctx.set_text_piece(5)
    gpu_ctx.set_text_piece(0)
