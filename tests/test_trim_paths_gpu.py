"""GPU tests of the trim kernel's two read paths and of its second adapter word (trim_reads_kernel, trim_kernels.hip; DESIGN.md §13, "Tests").
A workgroup whose 128 reads span more than 32 KiB reads them from device memory instead of an LDS slab, and an adapter past 32 nt is compared in
two 64-bit words; tests/test_trim_gpu.py reaches neither.  Here whole output files and all seven counts are compared by equality with the plain
restatement of tests/test_trim_cpu.py on the inputs of tests/test_trim_paths_cpu.py, which also states why they can tell; after every call
mirp_trim_last_paths must report the workgroups per path that block_spans predicts, so no test passes on the path it was not written for."""
import pytest

from tests.test_trim_cpu import ILLUMINA, STATS, Refused, restate_trim
from tests.test_trim_gpu import OPTION_GRID, QUALITY_GRID, _gpu
from tests.test_trim_paths_cpu import (FASTA_LAYOUTS, LIMIT_OPTIONS, LIMIT_SPANS, SLAB, WORD_LAYOUTS, block_spans, limit_file, paths_fasta, paths_fastq,
                                       predicted_paths, reference, word_adapters, word_file, word_options)

pytestmark = pytest.mark.gpu


def _check(ctx, tmp_path, data, want, paths, name="in.fastq", **kw):
    """The output file and the counts equal `want`, and the call took the paths `paths`."""
    got = _gpu(ctx, tmp_path, data, name, **kw)
    assert got[1] == want[1], kw
    assert got[0] == want[0], kw
    s = got[1]
    assert s["reads"] == s["untrimmed"] + s["too_short"] + s["too_long"] + s["written"]
    assert ctx.trim_last_paths() == paths, kw
    return s


def test_fastq_groups_on_both_paths(gpu_ctx, tmp_path):
    data = paths_fastq()
    paths = predicted_paths(data)
    assert paths == (4, 3)
    seen = dict.fromkeys(STATS, 0)
    for kw in OPTION_GRID + QUALITY_GRID:
        s = _check(gpu_ctx, tmp_path, data, reference(data, **kw), paths, **kw)
        for k in STATS:
            seen[k] += s[k]
    assert all(seen[k] > 0 for k in STATS), seen


@pytest.mark.parametrize("span", LIMIT_SPANS)
def test_slab_limit(gpu_ctx, tmp_path, span):
    """The first group's span is 16 under, at, 1 over and 16 over the slab's 32,768 bytes: slab, slab, device memory, device memory."""
    data = limit_file(span)
    assert block_spans(data)[0] == span
    paths = (2, 0) if span <= SLAB else (1, 1)
    for kw in LIMIT_OPTIONS:
        _check(gpu_ctx, tmp_path, data, reference(data, **kw), paths, **kw)


@pytest.mark.parametrize("width,eol", FASTA_LAYOUTS)
def test_fasta_groups_on_both_paths(gpu_ctx, tmp_path, width, eol):
    """The four layouts hold the same names and reads (test_trim_paths_cpu checks that they parse alike), so the restatement of one serves all."""
    data, plain = paths_fasta(width, eol), paths_fasta(0, b"\n")
    assert predicted_paths(data) == (2, 2)
    for kw in OPTION_GRID:
        _check(gpu_ctx, tmp_path, data, reference(plain, **kw), (2, 2), name="in.fa", **kw)


@pytest.mark.parametrize("layout", WORD_LAYOUTS)
@pytest.mark.parametrize("i", range(5))
def test_adapter_words(gpu_ctx, tmp_path, i, layout):
    adapter = word_adapters()[i]
    data = word_file(adapter, layout)
    paths = predicted_paths(data)
    assert (paths[1] == 0 and paths[0] >= 13) if layout == "slab" else (paths[1] >= 4 and paths[0] <= 1)
    found = 0
    for kw in word_options(adapter):
        found += _check(gpu_ctx, tmp_path, data, reference(data, **kw), paths, **kw)["adapter"]
    assert found > 0


def test_paths_of_empty_and_refused_calls(gpu_ctx, tmp_path):
    from mir_prefer_amd import capi
    data = paths_fastq()
    _check(gpu_ctx, tmp_path, data, reference(data, adapter=ILLUMINA), (4, 3), adapter=ILLUMINA)
    bad = data + b"@b\nAC\n+\nI\x7f\n"                                  # refused by the trim kernel itself, after it has counted its paths
    with pytest.raises(Refused):
        restate_trim(bad, adapter=ILLUMINA)
    with pytest.raises(capi.MirpError):
        gpu_ctx.trim_reads(bad, "bad.fastq", str(tmp_path / "bad.trimmed.fa"), adapter=ILLUMINA)
    assert gpu_ctx.trim_last_paths() == (0, 0)
    _check(gpu_ctx, tmp_path, data, reference(data, adapter=ILLUMINA), (4, 3), adapter=ILLUMINA)
    _check(gpu_ctx, tmp_path, b"", reference(b"", min_len=0), (0, 0), min_len=0)
    with pytest.raises(capi.MirpError):                               # a whole-file refusal, before the trim kernel
        gpu_ctx.trim_reads(b"ACGT\n", "bad.fastq", str(tmp_path / "bad.trimmed.fa"))
    assert gpu_ctx.trim_last_paths() == (0, 0)
