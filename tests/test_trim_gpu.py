"""GPU tests of the read trimming (mirp_trim_reads, trim_kernels.hip): whole output files and counts against the restatements of
tests/test_trim_cpu.py over FASTQ and FASTA (multi-line), three line ends, adapter lengths 1 / 3 / 21 / 64, E, O, -q, -m / -M and
--discard-untrimmed; the refusals and their messages; 2 M reads against the numpy restatement; a file past 2^31 bytes; multi-member gzip; the
command line on three files; and the chain trim -> reads collapse -> align -> pipeline through the command lines."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_trim_cpu import (ILLUMINA, REASONS, ROOT, STATS, Refused, fastq_record, make_reads, restate_trim, restate_trim_numpy, to_fasta,
                                 to_fastq)

pytestmark = pytest.mark.gpu


def _gpu(ctx, tmp_path, data, name="in.fastq", **kw):
    out = tmp_path / (name + ".trimmed.fa")
    if out.exists():
        out.unlink()
    opts = dict(adapter=kw.get("adapter", ""), error_permille=kw.get("e_pm", 100), overlap=kw.get("overlap", 3), quality=kw.get("q", 0),
                min_length=kw.get("min_len", 18), max_length=kw.get("max_len", 0), discard_untrimmed=kw.get("discard", False))
    res = ctx.trim_reads(data, name, str(out), **opts)
    return out.read_bytes(), {k: res[k] for k in STATS}


def _edge_reads(rng):
    """Empty reads, reads shorter than O, dimers, N and lower case, adapter prefixes with errors at the 3' end, a read at the length limit."""
    ad = ILLUMINA.encode()
    reads = [(b"empty", b"", b""), (b"one", b"T", b"I"), (b"two", b"TG", b"II"), (b"dimer", ad + b"ACGT", b"I" * 25),
             (b"dimer_lc", ad.lower(), b"5" * 21), (b"nn", b"ACGTNNNNACGT" + ad[:10], b"I" * 22), (b"lc", b"acgtacgtacgtacgtacgtac" + ad[:5].lower(), b"I" * 27),
             (b"err", b"ACGTTTGCAGCATCGATCGA" + ad[:4] + b"T" + ad[5:15], b"I" * 35), (b"limit", (b"ACGT" * 256)[:1024 - 21] + ad, b"I" * 1024),
             (b"limit2", rng.choice(list(b"ACGTN"), 1024).astype(np.uint8).tobytes(), b"#" * 512 + b"I" * 512), (b"tab\tname", b"CCCCCCCCCCCCCCCCCCCCCTGGAA", b"I" * 26)]
    return reads + make_reads(rng, 1500) + make_reads(rng, 300, adapter=b"A" * 64, lo=0, hi=80)


def _check(ctx, tmp_path, data, name="in.fastq", **kw):
    got = _gpu(ctx, tmp_path, data, name, **kw)
    want = restate_trim(data, **kw)
    assert got[1] == want[1], kw
    assert got[0] == want[0], kw
    s = got[1]
    assert s["reads"] == s["untrimmed"] + s["too_short"] + s["too_long"] + s["written"]
    return s


OPTION_GRID = [dict(adapter=ILLUMINA), dict(adapter=ILLUMINA, e_pm=0, overlap=1, min_len=0), dict(adapter=ILLUMINA, e_pm=250, overlap=21, discard=True),
               dict(adapter="T", e_pm=0, overlap=1, min_len=0), dict(adapter="TGG", e_pm=250, overlap=3, min_len=5, max_len=22),
               dict(adapter="tggaat", e_pm=100, overlap=3, discard=True, min_len=0), dict(adapter="A" * 64, e_pm=100, overlap=64, min_len=0),
               dict(adapter="A" * 64, e_pm=250, overlap=1, min_len=10, max_len=40), dict(min_len=0), dict(min_len=18, max_len=26)]
QUALITY_GRID = [dict(q=20), dict(q=10, adapter=ILLUMINA, min_len=0), dict(q=30, adapter="TGG", e_pm=0, overlap=1, discard=True, min_len=0),
                dict(q=93, min_len=0), dict(q=1, adapter="A" * 64, overlap=3, max_len=30)]


@pytest.mark.parametrize("eol", [b"\n", b"\r\n", b"\r"])
def test_fastq_grid_matches_the_restatement(gpu_ctx, tmp_path, eol):
    rng = np.random.RandomState(len(eol) + (3 if eol == b"\r" else 0))
    reads = _edge_reads(rng)
    rng.shuffle(reads)
    data = to_fastq(reads, eol, final_eol=eol != b"\r") + (eol + b"  " + eol if eol == b"\n" else b"")
    seen = dict.fromkeys(STATS, 0)
    for kw in OPTION_GRID + QUALITY_GRID:
        s = _check(gpu_ctx, tmp_path, data, **kw)
        for k in STATS:
            seen[k] += s[k]
    assert all(seen[k] > 0 for k in STATS), seen


@pytest.mark.parametrize("eol,width", [(b"\n", 0), (b"\r\n", 7), (b"\r", 60)])
def test_fasta_grid_matches_the_restatement(gpu_ctx, tmp_path, eol, width):
    rng = np.random.RandomState(20 + width)
    reads = _edge_reads(rng)
    data = to_fasta(reads, eol, width) + b">last no newline\n" + b"ACGTACGTACGTACGTACGT" + ILLUMINA.encode()[:9]
    for kw in OPTION_GRID:
        _check(gpu_ctx, tmp_path, data, name="in.fa", **kw)


def test_empty_and_tiny_inputs(gpu_ctx, tmp_path):
    for data in (b"", b"@a\nACGT\n+\nIIII", b">a", b">", b"@\n\n+\n\n@x\nA\n+\nI\n", b">a\n\n\n>b\nAC GT\n"):
        _check(gpu_ctx, tmp_path, data, min_len=0, adapter="ACG", overlap=1)


def _refused(ctx, tmp_path, data, **kw):
    from mir_prefer_amd import capi
    with pytest.raises(Refused) as want:
        restate_trim(data, **kw)
    out = tmp_path / "bad.fastq.trimmed.fa"
    out.write_bytes(b">stale\nACGT\n")              # an output of an earlier run goes too: a refused input has no output
    with pytest.raises(capi.MirpError) as got:
        ctx.trim_reads(data, "bad.fastq", str(out), adapter=kw.get("adapter", ""), quality=kw.get("q", 0))
    assert not out.exists()
    return want.value, str(got.value)


def test_refusals_name_the_record_and_write_nothing(gpu_ctx, tmp_path):
    rng = np.random.RandomState(5)
    good = to_fastq(make_reads(rng, 700))
    bad_records = [b"@b\nAC\n+\n", b"Xb\nAC\n+\nII\n", b"@b\nAC\n-\nII\n", b"@b\n" + b"A" * 1025 + b"\n+\n" + b"I" * 1025 + b"\n", b"@b\nAC\n+\nI\n",
                   b"@b\nAC\n+\nI \n", b"@b\nAC\n+\nI\x7f\n", b"@b\nAC\n+\nI\x1f\n", b"@" + b"n" * (1 << 20 | 1) + b"\nAC\n+\nII\n"]
    for rec in bad_records:
        for data in (good + rec, good + rec + good):
            if rec == b"@b\nAC\n+\n" and data != good + rec:
                continue
            want, msg = _refused(gpu_ctx, tmp_path, data, adapter=ILLUMINA)
            assert want.kind == "record" and ("bad.fastq: record %d: %s" % (want.record, REASONS[want.reason])) in msg, (msg, want.reason)
    # a refusal in the middle beats a later one; within a record the first reason in §13's order
    data = good + b"@b\nAC\n-\nI\n" + good + b"@c\nAC\n+\nI\n"
    want, msg = _refused(gpu_ctx, tmp_path, data)
    assert want.record == 701 and want.reason == 1 and "record 701: line 3" in msg
    want, msg = _refused(gpu_ctx, tmp_path, b">a\nACGT\n>b\n" + b"ACGT\n" * 256 + b"A\n")
    assert "record 2: " + REASONS[2] in msg
    for data in (good + "é".encode() + good, b"\x80"):
        want, msg = _refused(gpu_ctx, tmp_path, data)
        assert "offset %d is not ASCII" % want.offset in msg
    want, msg = _refused(gpu_ctx, tmp_path, b"ACGT\n")
    assert want.kind == "format" and "neither '@' (FASTQ) nor '>' (FASTA)" in msg
    want, msg = _refused(gpu_ctx, tmp_path, b">a\nACGT\n", q=20)
    assert want.kind == "quality" and "needs FASTQ input" in msg


def test_two_million_reads_against_numpy(gpu_ctx, tmp_path):
    rng = np.random.RandomState(9)
    base = make_reads(rng, 40000, err=0.01, lo=18, hi=26, tail=(4, 10))
    idx = rng.randint(0, len(base), size=2_100_000)
    data = b"".join(fastq_record(b"q%d" % i, base[k][1], base[k][2]) for i, k in enumerate(idx))
    for kw in (dict(adapter=ILLUMINA, q=20), dict(adapter=ILLUMINA[:10], e_pm=0, overlap=1, min_len=0, max_len=30, discard=True)):
        got = _gpu(gpu_ctx, tmp_path, data, **kw)
        want = restate_trim_numpy(data, **kw)
        assert got[1] == want[1] and got[0] == want[0], kw


def test_file_past_2gib(gpu_ctx, tmp_path):
    """A block of FASTQ records repeated past 2^31 bytes: the output is the block's output repeated."""
    rng = np.random.RandomState(17)
    block = to_fastq(make_reads(rng, 4000, lo=10, hi=200, tail=(0, 300)))
    want, st = restate_trim(block, adapter=ILLUMINA, q=15)
    m = (2 ** 31) // len(block) + 2
    data = block * m
    assert len(data) > 2 ** 31
    got, gs = _gpu(gpu_ctx, tmp_path, data, adapter=ILLUMINA, q=15)
    del data
    assert gs == {k: v * m for k, v in st.items()}
    assert len(got) == len(want) * m and got == want * m


def test_gzip_multi_member_equals_plain(tmp_path):
    rng = np.random.RandomState(4)
    data = to_fastq(make_reads(rng, 3000))
    (tmp_path / "p.fastq").write_bytes(data)
    (tmp_path / "z.fastq.gz").write_bytes(b"".join(gzip.compress(data[i:i + 7777]) for i in range(0, len(data), 7777)))
    r = _cli(["-a", ILLUMINA, "-q", "20", str(tmp_path / "p.fastq"), str(tmp_path / "z.fastq.gz")], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    got = (tmp_path / "z.fastq.trimmed.fa").read_bytes()
    assert got == (tmp_path / "p.fastq.trimmed.fa").read_bytes() == restate_trim(data, adapter=ILLUMINA, q=20)[0]
    (tmp_path / "c.fastq.gz").write_bytes(gzip.compress(data)[:-9] + b"\0" * 9)
    (tmp_path / "c.fastq.trimmed.fa").write_bytes(b">stale\nACGT\n")
    r = _cli([str(tmp_path / "c.fastq.gz")], tmp_path)
    assert r.returncode == 255 and b"corrupt gzip" in r.stderr and not (tmp_path / "c.fastq.trimmed.fa").exists()


def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.trim"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_cli_on_three_files(tmp_path):
    rng = np.random.RandomState(8)
    files = []
    for k, (fmt, eol) in enumerate(((to_fastq, b"\n"), (to_fasta, b"\r\n"), (to_fastq, b"\r"))):
        p = tmp_path / ("s%d.%s" % (k, "fa" if fmt is to_fasta else "fastq"))
        p.write_bytes(fmt(make_reads(rng, 500 + k), eol))
        files.append(str(p))
    r = _cli(["-a", ILLUMINA, "-e", "0.15", "-O", "5", "-m", "16", "-M", "30", "--discard-untrimmed"] + files, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want_out = []
    for p in files:
        out, st = restate_trim(open(p, "rb").read(), adapter=ILLUMINA, e_pm=150, overlap=5, min_len=16, max_len=30, discard=True)
        assert open(p + ".trimmed.fa", "rb").read() == out
        want_out += ["Start processing file " + p, "Finish file " + p,
                     "File %s: %d reads, %d quality-trimmed, %d with adapter, %d untrimmed discarded, %d too short, %d too long, %d written"
                     % ((p,) + tuple(st[k] for k in STATS))]
    assert r.stdout.decode().splitlines() == want_out + ["DONE", ""]
    # a refused file in the middle: the one before keeps its output, the ones after are not processed
    for p in files:
        os.unlink(p + ".trimmed.fa")
    bad = tmp_path / "bad.fastq"
    bad.write_bytes(b"@a\nACGT\n+\nIII\n")
    bad.with_name("bad.fastq.trimmed.fa").write_bytes(b">stale\nACGT\n")
    r = _cli([files[0], str(bad), files[2]], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and "record 1: " + REASONS[3] in r.stderr.decode()
    assert os.path.exists(files[0] + ".trimmed.fa") and not bad.with_name("bad.fastq.trimmed.fa").exists() and not os.path.exists(files[2] + ".trimmed.fa")


def test_chain_trim_collapse_align_pipeline(tmp_path):
    from mir_prefer_amd import synth
    from tests.test_align_gpu import _synth_read
    ds = synth.make_dataset([50000, 30000], 30, n_samples=2, seed=6, contig_names=["chr2", "chr1"])
    ds.write_fasta(str(tmp_path / "genome.fa"))
    rng = np.random.RandomState(12)
    ad = ILLUMINA.encode()
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(mod, args, cwd):
        r = subprocess.run([sys.executable, "-m", mod] + args, cwd=str(cwd), capture_output=True, timeout=900, env=env)
        assert r.returncode == 0, (mod, r.stderr.decode())
    results = []
    for exact in (True, False):
        d = tmp_path / ("exact" if exact else "noisy")
        (d / "want").mkdir(parents=True)
        raw, inserts = [], []
        for si, sname in enumerate(ds.sample_names):
            recs = []
            for k, a in enumerate(ds.alns[ds.alns["sample"] == si]):
                s = _synth_read(ds, a).tobytes()
                for j in range(int(a["depth"])):
                    a2 = bytearray(ad)
                    if not exact:
                        for i in np.flatnonzero(rng.rand(len(a2)) < 0.02):
                            a2[i] = b"ACGT"[rng.randint(0, 4)]
                    tail = rng.choice(list(b"ACGT"), rng.randint(0, 12)).astype(np.uint8).tobytes()
                    seq = (s + bytes(a2) + tail)[:51]
                    recs.append((b"x%d_%d" % (k, j), seq, bytes(np.clip(40 - np.arange(len(seq)) // 4, 2, 40).astype(np.uint8) + 33)))
                    inserts.append(s)
            p = d / (sname + ".fastq")
            p.write_bytes(to_fastq(recs))
            raw.append(p)
        args = ["-a", ILLUMINA, "-m", "1"] + ([] if not exact else ["-e", "0"])
        run("mir_prefer_amd.trim", args + [str(p) for p in raw], d)
        trimmed = [str(p) + ".trimmed.fa" for p in raw]
        if exact:
            got = [ln for p in trimmed for ln in open(p, "rb").read().split(b"\n")[1::2]]
            assert got == inserts
        for p in raw:
            (d / "want" / (p.name + ".trimmed.fa")).write_bytes(restate_trim(p.read_bytes(), adapter=ILLUMINA, e_pm=0 if exact else 100, min_len=1)[0])
        (d / "names.txt").write_text("".join(s + "\n" for s in ds.sample_names))
        loci = []
        for tag, files in (("got", trimmed), ("want", [str(d / "want" / (p.name + ".trimmed.fa")) for p in raw])):
            run("mir_prefer_amd.reads", ["collapse", str(d / "names.txt")] + files, d)
            run("mir_prefer_amd.align", ["-f", "-r", str(tmp_path / "genome.fa")] + [f + ".processed" for f in files], d)
            cfg = d / ("config_" + tag)
            cfg.write_text("FASTA_FILE = %s\nALIGNMENT_FILE = %s\nPRECURSOR_LEN = 300\nREADS_DEPTH_CUTOFF = 20\nMAX_GAP = 100\nMIN_MATURE_LEN = 18\n"
                           "MAX_MATURE_LEN = 24\nALLOW_NO_STAR_EXPRESSION = Y\nALLOW_3NT_OVERHANG = N\nOUTFOLDER = %s\nNAME_PREFIX = chain\n"
                           % (tmp_path / "genome.fa", ", ".join(f + ".processed.sam" for f in files), d / ("out_" + tag)))
            run("mir_prefer_amd.cli", ["pipeline", str(cfg)], d)
            out = d / ("out_" + tag)
            loci.append([open(out / fn, "rb").read() for fn in ("chain_miRNA.gff3", "chain_miRNA.mature.fa", "chain_miRNA.precursor.fa")])
        assert loci[0] == loci[1]
        results.append(loci[0])
    assert results[0][0].count(b"\n") > 1
