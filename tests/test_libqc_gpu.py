"""GPU tests of the library profile (mirp_libqc_reads, libqc_kernels.hip).  Every call is compared by equality with the restatements
of tests/libqc_restatement.py: the whole table of 4^12 counters (mirp_libqc_last_table), the found adapter with the walk's record, the four
counters and the three tables; the verb's three files byte for byte.  The inputs are the smallest at which the kernels can go wrong: reads around
the wave and the workgroup, lengths around K and the 64-base window, N and lower case on the edges of a 12-mer, the first and the last code, a
wave that merges into one atomic and a wave that merges nothing, samples that end inside a workgroup, every input layout, and reads that leave the
trim kernel's LDS slab."""
import numpy as np
import pytest

from tests import libqc_restatement as lr
from tests.test_libqc_cpu import CONSTRUCT, LIBRARIES, head, is_truth, library, planted
from tests.test_trim_cpu import ILLUMINA, Refused, make_reads, restate_trim, to_fasta, to_fastq
from tests.test_trim_paths_cpu import paths_fasta, paths_fastq, predicted_paths

pytestmark = pytest.mark.gpu

FOUND_KEYS = ("adapter", "status", "seed", "seed_count", "min_count", "left_steps", "left_stop")
COUNT_KEYS = ("reads", "sampled", "with_adapter", "dimers")
TABLE_KEYS = ("raw_len", "cycles", "insert")


def _check(ctx, data, name="in.fastq", restate=lr.restate_libqc_numpy, **kw):
    """One call against the restatement, entry by entry; -> the restatement's result."""
    want = restate(data, **kw)
    got = ctx.libqc_reads(data, name, adapter=kw.get("adapter", ""), error_permille=kw.get("e_pm", 100), overlap=kw.get("overlap"),
                          sample=kw.get("sample", lr.SAMPLE))
    table = ctx.libqc_last_table()
    assert table is not None and table.dtype == np.uint32 and np.array_equal(table, want["table"]), kw
    assert {k: got[k] for k in FOUND_KEYS} == {k: want[k] for k in FOUND_KEYS}, kw
    assert {k: got[k] for k in COUNT_KEYS} == {k: want[k] for k in COUNT_KEYS}, kw
    for k in TABLE_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, kw)
    assert len(got["seconds"]) == 6 and all(s >= 0 for s in got["seconds"])
    return want


def _bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.randint(0, len(alphabet), size=n)].tobytes()


def _fastq(reads):
    return to_fastq([(b"r%d" % i, s, bytes(33 + (7 * i + j) % 42 for j in range(len(s)))) for i, s in enumerate(reads)])


def _constructs(rng, n, lo=15, hi=30):
    """n reads of an insert and the Illumina construct, 51 nt, a tenth with N or lower case."""
    out = []
    for i in range(n):
        s = (_bases(rng, int(rng.randint(lo, hi + 1))) + CONSTRUCT.encode())[:51]
        out.append(s.lower() if i % 10 == 3 else s[:7] + b"N" + s[8:] if i % 10 == 7 else s)
    return out


@pytest.mark.parametrize("n_reads", [0, 1, 63, 64, 65, 129])
def test_reads_around_the_wave(gpu_ctx, n_reads):
    data = _fastq(_constructs(np.random.RandomState(n_reads), n_reads))
    want = _check(gpu_ctx, data, restate=lr.restate_libqc)
    assert want["reads"] == n_reads and (want["status"] == "none") == (n_reads < 16)
    if n_reads >= 63:                                        # at 63 reads the four predecessors of the adapter's head may all lie under min_count: unsure
        assert is_truth(want["adapter"], CONSTRUCT) and want["with_adapter"] >= n_reads - 2
    _check(gpu_ctx, data, adapter=ILLUMINA, overlap=5, e_pm=0)


def test_read_lengths_around_k_and_the_window(gpu_ctx):
    rng = np.random.RandomState(2)
    reads = []
    for n in (0, 11, 12, 13, 63, 64, 65, 1024):
        s = _bases(rng, n)
        reads += [s] * 17 + [_bases(rng, n, b"ACGTacgtN")] * 3
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    want = _check(gpu_ctx, _fastq(reads))
    t = want["table"]
    assert int((t >= 17).sum()) == 1 + 2 + 52 + 53 + 53 + 53 and want["status"] != "none"    # nothing behind base 64 is counted: 65 and 1,024 add 53 each
    assert [int(want["raw_len"][n]) for n in (0, 11, 12, 13, 63, 64, 65, 1024)] == [20] * 8 and want["cycles"][1023][:5].sum() == 20
    _check(gpu_ctx, to_fasta([(b"r%d" % i, s, None) for i, s in enumerate(reads)], width=70), name="in.fa", adapter="ACGTTGCA", overlap=8)


def test_n_and_lower_case_on_the_edges_of_a_kmer(gpu_ctx):
    core = b"ACGTTGCAAGCT"                                      # one 12-mer; the cases put N / n / lower case before, inside, at both ends and behind it
    cases = [core, core.lower(), b"N" + core, core + b"N", b"n" + core + b"n", core[:11] + b"N", b"N" + core[1:], core[:6] + b"n" + core[7:],
             core[:1].lower() + core[1:], core[:11] + core[11:].lower(), core + core, core + b"N" + core, core[:11] + b"N" + core, b"NNNNNNNNNNNN",
             core + b"-" + core, core + b"U" * 12]
    reads = [s for s in cases for _ in range(16)]
    want = _check(gpu_ctx, _fastq(reads), restate=lr.restate_libqc)
    assert int(want["table"][lr.code_of(core.decode())]) == 16 * (1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 2 + 1 + 2 + 1)
    assert want["cycles"][:, 4].sum() == 16 * (1 + 1 + 2 + 1 + 1 + 1 + 1 + 1 + 12 + 1 + 12)
    _check(gpu_ctx, to_fasta([(b"x", s, None) for s in reads]), name="in.fa", restate=lr.restate_libqc)


def test_first_and_last_code(gpu_ctx):
    reads = [b"A" * 12] * 20 + [b"T" * 12] * 21 + [b"a" * 30] * 5 + [b"T" * 64] * 3 + [b"AAAAAACCCCCC"] * 18 + [b"G" * 1024]
    want = _check(gpu_ctx, _fastq(reads), restate=lr.restate_libqc)
    t = want["table"]
    assert int(t[0]) == 20 + 5 * 19 and int(t[lr.CODES - 1]) == 21 + 3 * 53 and int(t[lr.code_of("G" * 12)]) == 53
    assert want["seed"] == "AAAAAACCCCCC" and want["seed_count"] == 18 and want["status"] == "unsure"        # the homopolymers are no seed


def test_a_wave_of_one_read_and_a_wave_of_strangers(gpu_ctx):
    rng = np.random.RandomState(4)
    same = [_bases(rng, 50)] * 64
    strangers = [_bases(rng, 50) for _ in range(64)]
    want = _check(gpu_ctx, _fastq(same + strangers + same[:7]))
    t = want["table"]
    assert int((t == 71).sum()) == 39 and int((t == 1).sum()) == 64 * 39 and int(t.sum()) == 135 * 39       # no 12-mer is shared by two strangers
    want = _check(gpu_ctx, _fastq(strangers))
    assert want["status"] == "none" and int(want["table"].max()) == 1


@pytest.mark.parametrize("sample", [1, 63, 100, 256, 300, 599, 600, 601, 1 << 26])
def test_sample_below_at_and_above_the_reads(gpu_ctx, sample):
    rng = np.random.RandomState(6)
    data = _fastq(_constructs(rng, 300) + [_bases(rng, 40) for _ in range(300)])
    want = _check(gpu_ctx, data, sample=sample)
    assert want["reads"] == 600 and want["sampled"] == min(sample, 600) and want["raw_len"].sum() == 600
    assert (want["status"] == "none") == (sample == 1)
    if sample >= 256:
        assert want["status"] == "ok" and is_truth(want["adapter"], CONSTRUCT)
    if sample >= 300:
        assert want["seed_count"] == _check(gpu_ctx, data, sample=300)["seed_count"]          # the random reads behind add nothing to the seed


@pytest.mark.parametrize("layout", ["fastq", "fastq_crlf", "fastq_cr_open", "fasta", "fasta_crlf", "fasta_wrapped", "fasta_wrapped_crlf"])
def test_every_input_layout(gpu_ctx, layout):
    rng = np.random.RandomState(8)
    reads = make_reads(rng, 400, adapter=CONSTRUCT[:40], lo=16, hi=30, err=0.02)
    reads[5] = (b"e", b"", b"")
    data = {"fastq": lambda: to_fastq(reads), "fastq_crlf": lambda: to_fastq(reads, b"\r\n"), "fastq_cr_open": lambda: to_fastq(reads, b"\r", final_eol=False),
            "fasta": lambda: to_fasta(reads), "fasta_crlf": lambda: to_fasta(reads, b"\r\n"), "fasta_wrapped": lambda: to_fasta(reads, width=17),
            "fasta_wrapped_crlf": lambda: to_fasta(reads, b"\r\n", width=23)}[layout]()
    want = _check(gpu_ctx, data, name="in." + layout[:5])
    assert want["status"] == "ok" and is_truth(want["adapter"], CONSTRUCT[:40]) and want["dimers"] > 0
    assert (want["cycles"][:, 5].sum() > 0) == layout.startswith("fastq")
    first = lr.restate_libqc_numpy(to_fastq(reads))
    assert np.array_equal(want["table"], first["table"]) and np.array_equal(want["insert"], first["insert"])        # the layout changes nothing but the qualities


@pytest.mark.parametrize("which", ["fastq", "fasta", "fasta_wrapped"])
def test_reads_on_the_trim_kernels_global_memory_path(gpu_ctx, which):
    data = paths_fastq() if which == "fastq" else paths_fasta(60 if which == "fasta_wrapped" else 0, b"\n")
    paths = predicted_paths(data)
    assert paths == ((4, 3) if which == "fastq" else (2, 2))
    want = _check(gpu_ctx, data, name="in." + which[:5], adapter=ILLUMINA)
    assert gpu_ctx.trim_last_paths() == paths
    assert want["with_adapter"] > 100 and want["raw_len"][1024] >= 1 and want["dimers"] > 0
    want = _check(gpu_ctx, data, name="in." + which[:5])
    assert gpu_ctx.trim_last_paths() == paths and want["status"] != "none" and want["insert"][:, 5].sum() == want["reads"]


def test_adapter_given_and_found(gpu_ctx):
    data = head(library("51nt_top60"), 3000)
    found = _check(gpu_ctx, data)
    assert found["status"] == "ok" and len(found["adapter"]) > len(ILLUMINA) and found["adapter"].startswith(ILLUMINA)
    given = _check(gpu_ctx, data, adapter=ILLUMINA.lower(), e_pm=0, overlap=21)
    assert {k: given[k] for k in FOUND_KEYS} == {k: found[k] for k in FOUND_KEYS}                   # the search runs and is reported either way
    assert given["with_adapter"] < found["with_adapter"] and not np.array_equal(given["insert"], found["insert"])
    short = _check(gpu_ctx, data, adapter="TGGA", overlap=64)                                     # an overlap beyond the adapter counts as its length
    assert 0 < short["with_adapter"] != found["with_adapter"]
    none = _check(gpu_ctx, head(data, 10))
    assert none["status"] == "none" and none["insert"].sum() == 0 and none["with_adapter"] == 0 and none["raw_len"].sum() == 10


def test_a_refused_input_leaves_no_table(gpu_ctx):
    from mir_prefer_amd import capi
    good = head(library("36nt"), 200)
    _check(gpu_ctx, good)
    assert gpu_ctx.libqc_last_table() is not None
    cases = [(good + b"@b\nAC\n+\nI\x7f\n", "(-10)", "record 201: a quality byte is outside 33..126"),          # seen by the trim kernel, behind the k-mers
             (good + b"@b\nAC\n+\nI\n", "(-10)", "record 201: the sequence and quality lengths differ"),
             (good + b"@b\nAC\n+\n", "(-10)", "record 201: the file ends inside the record"),
             (good + b"@b\n" + b"A" * 1025 + b"\n+\n" + b"I" * 1025 + b"\n", "(-10)", "record 201: the read is longer than 1,024 nt"),
             (good + b"\xc3\xa9", "(-9)", "is not ASCII"), (b"ACGT\n", "(-10)", "neither '@' (FASTQ) nor '>' (FASTA)"),
             (b">a\n" + b"A" * 1025 + b"\n", "(-10)", "record 1: the read is longer than 1,024 nt")]
    for data, code, text in cases:
        with pytest.raises(Refused):
            lr.restate_libqc(data)
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.libqc_reads(data, "bad.fastq")
        assert code in str(e.value) and "bad.fastq: " in str(e.value) and text in str(e.value), data[-40:]
        assert gpu_ctx.libqc_last_table() is None and gpu_ctx.trim_last_paths() == (0, 0)
    for kw in (dict(sample=0), dict(sample=(1 << 26) + 1), dict(adapter="ACGU"), dict(overlap=65), dict(error_permille=1000)):
        with pytest.raises(capi.MirpError):
            gpu_ctx.libqc_reads(good, "in.fastq", **kw)
        assert gpu_ctx.libqc_last_table() is None
    _check(gpu_ctx, good)                                                        # and the context goes on


@pytest.mark.parametrize("name", ["36nt", "dimers50", "adapter17_random"])
def test_library_through_libqc_then_trim_a_auto(tmp_path, capsys, name):
    from mir_prefer_amd import libqc, trim
    data = library(name)
    path = tmp_path / "lib.fastq"
    path.write_bytes(data)
    assert libqc.main([str(path)]) == 0
    want = lr.restate_libqc_numpy(data)
    assert want["status"] == LIBRARIES[name][1] == "ok" and is_truth(want["adapter"], planted(name))
    for out, text in zip(libqc.output_names(str(path)), lr.render(want)):
        assert open(out, "rb").read() == text, out
    out = capsys.readouterr().out
    assert "adapter %s (ok): python -m mir_prefer_amd.trim -a %s %s\n" % (want["adapter"], want["adapter"], path) in out
    assert trim.main(["-a", "auto", str(path)]) == 0
    assert "found the adapter " + want["adapter"] + "\n" in capsys.readouterr().err
    trimmed, st = restate_trim(data, adapter=want["adapter"])
    assert open(trim.output_name(str(path)), "rb").read() == trimmed and st["adapter"] == want["with_adapter"]


def test_verb_on_gz_fasta_with_options_and_a_refusal(tmp_path, capsys):
    import gzip
    from mir_prefer_amd import libqc, trim
    reads = make_reads(np.random.RandomState(9), 300, adapter=CONSTRUCT[:30], lo=18, hi=26)
    data = to_fasta(reads, width=30)
    path = tmp_path / "lib.fa.gz"
    path.write_bytes(gzip.compress(data))
    assert libqc.main(["-a", "tggaattc", "-e", "0.125", "-O", "8", "--sample", "200", str(path)]) == 0
    want = lr.restate_libqc_numpy(data, adapter="tggaattc", e_pm=125, overlap=8, sample=200)
    assert libqc.output_names(str(path))[0] == str(tmp_path / "lib.fa.libqc.tsv")
    for out, text in zip(libqc.output_names(str(path)), lr.render(want)):
        assert open(out, "rb").read() == text, out
    # an already trimmed library: libqc says unsure, and trim -a auto refuses with the candidate and writes nothing
    inserts = tmp_path / "trimmed.fastq"
    inserts.write_bytes(head(library("trimmed"), 4000))
    capsys.readouterr()
    assert libqc.main([str(inserts)]) == 0
    res = lr.restate_libqc_numpy(inserts.read_bytes())
    assert res["status"] == "unsure" and "adapter %s (unsure" % res["adapter"] in capsys.readouterr().out
    assert trim.main(["-a", "auto", str(inserts)]) == 255
    err = capsys.readouterr().err
    assert "status unsure" in err and res["adapter"] in err and not (tmp_path / "trimmed.fastq.trimmed.fa").exists()
    # a refused file leaves no table behind, not even one of an earlier run
    bad = tmp_path / "bad.fastq"
    bad.write_bytes(b"@a\nACGT\n+\nIII\n")
    for p in libqc.output_names(str(bad)):
        open(p, "wb").write(b"stale")
    assert libqc.main([str(bad)]) == 255 and "record 1: the sequence and quality lengths differ" in capsys.readouterr().err
    assert not any((tmp_path / ("bad.fastq" + s)).exists() for s in libqc.SUFFIXES)
