"""CPU tests of the library profile (mir_prefer_amd.libqc, mirp_libqc_reads): the walk's rules on hand-built tables, the two
restatements of tests/libqc_restatement.py against each other, the adapter they find on seeded synthetic libraries, the verb's and `trim -a auto`'s
argument paths with the device call stubbed, and the declaration of the C-ABI entries.  The generators are shared with tests/test_libqc_gpu.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import libqc_restatement as lr
from tests.test_trim_cpu import ROOT, Refused, to_fasta, to_fastq

CONSTRUCT = "TGGAATTCTCGGGTGCCAAGGAACTCCAGTCACATCACGATCTCGTATGCCGTCTTCTGCTTG"      # Illumina small-RNA 3' adapter, index read primer site, index, P7
N_READS = 30000


# ---- seeded synthetic libraries

def make_library(seed, n=N_READS, read_len=51, top=0.3, dimers=0.0, flank=0, construct=CONSTRUCT, random_after=False, trimmed=False, pool=2000):
    """[(name, read, qual)]: an insert of 19..35 nt from a pool (the first insert with probability `top`, the others Zipf(1.5) by rank), `flank`
    random bases on both of its sides, the construct, then G up to read_len (random bases with random_after); substitutions at 1 % on the first
    cycle rising to 3 % on the last; `dimers` of the reads have no insert; trimmed: the insert alone."""
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    inserts = [acgt[rng.randint(0, 4, size=rng.randint(19, 36))] for _ in range(pool)]
    cons = np.frombuffer(construct.encode(), np.uint8)
    rate = 0.01 * (1 + 2 * np.arange(max(read_len, 64)) / max(read_len - 1, 1))
    out = []
    for i in range(n):
        k = 0 if rng.rand() < top else 1 + min(int(rng.zipf(1.5)) - 1, pool - 2)
        ins = inserts[k] if rng.rand() >= dimers else acgt[:0]
        if trimmed:
            seq = ins.copy()
        else:
            parts = [acgt[rng.randint(0, 4, size=flank)], ins, acgt[rng.randint(0, 4, size=flank)], cons]
            used = sum(len(p) for p in parts)
            fill = max(read_len - used, 0)
            parts.append(acgt[rng.randint(0, 4, size=fill)] if random_after else np.full(fill, ord("G"), np.uint8))
            seq = np.concatenate(parts)[:read_len]
        err = rng.rand(len(seq)) < rate[:len(seq)]
        seq = np.where(err, acgt[(np.searchsorted(acgt, seq) + rng.randint(1, 4, size=len(seq))) % 4], seq).astype(np.uint8)
        qual = (np.clip(38 - (np.arange(len(seq)) * 20) // max(read_len, 1) + rng.randint(-3, 4, size=len(seq)), 2, 40) + 33).astype(np.uint8)
        out.append((b"r%d" % i, seq.tobytes(), qual.tobytes()))
    return out


LIBRARIES = {
    "51nt_top30": (dict(seed=1, read_len=51, top=0.3), "ok"),
    "51nt_top60": (dict(seed=2, read_len=51, top=0.6), "ok"),
    "36nt": (dict(seed=3, read_len=36), "ok"),
    "100nt_polyG": (dict(seed=4, read_len=100), "ok"),
    "150nt_polyG": (dict(seed=5, read_len=150), "ok"),
    "dimers50": (dict(seed=6, read_len=51, dimers=0.5), "ok"),
    "flank4N": (dict(seed=7, read_len=51, flank=4), "ok"),
    "adapter17_random": (dict(seed=8, read_len=51, construct=CONSTRUCT[:17], random_after=True), "ok"),
    # at 75 % the purity before the adapter is 75 % + the inserts that end in the same base, a quarter of the rest on average: about 81 % against
    # the bound of 80 %, so the outcome hangs on the pool; this seed's pool has them (seeds 9, 10, 11 and 14 do not and give `ok`)
    "top75": (dict(seed=12, read_len=51, top=0.75), "unsure"),
    "trimmed": (dict(seed=10, trimmed=True), "unsure"),
}


@functools.lru_cache(maxsize=None)
def library(name):
    """The FASTQ text of one of LIBRARIES; cached, not to be modified."""
    return to_fastq(make_library(**LIBRARIES[name][0]))


def head(data, n):
    """The first n records of a FASTQ text."""
    return b"".join(data.splitlines(True)[:4 * n])


def planted(name):
    return LIBRARIES[name][0].get("construct", CONSTRUCT)


def is_truth(adapter, construct):
    return len(adapter) >= lr.K and (construct.startswith(adapter) or adapter.startswith(construct))


# ---- the walk's rules on hand-built tables

def _table(counts):
    t = np.zeros(lr.CODES, np.uint32)
    for kmer, c in counts.items():
        t[lr.code_of(kmer)] = c
    return t


def _chain(seq, count):
    """Every 12-mer of seq at `count`."""
    return {seq[i:i + lr.K]: count for i in range(len(seq) - lr.K + 1)}


SEQ = "ACGTTGCAAGCTTAGGCATCGATTACGGATCCATGCAAGTC"


def test_codes_and_eligibility():
    assert lr.code_of("A" * 12) == 0 and lr.code_of("T" * 12) == lr.CODES - 1 and lr.code_of("A" * 11 + "C") == 1 and lr.code_of("C" + "A" * 11) == 4 ** 11
    for code in (0, 1, 12345678, lr.CODES - 1):
        assert lr.code_of(lr.kmer_of(code)) == code
    assert lr.eligible("AAAAAACCCCCC") and not lr.eligible("AAAAAAACCCCC") and not lr.eligible("G" * 12) and lr.eligible("ACGTACGTACGT")
    mask = lr.eligible_mask()
    for code in (0, 0x555, 0x556, 12345678, lr.CODES - 1, lr.code_of("AAAAAAACCCCC")):
        assert bool(mask[code]) == lr.eligible(lr.kmer_of(code))


def test_none_below_16_and_without_reads():
    f = lr.find_adapter(_table({SEQ[:12]: 15}), 100)
    assert f["status"] == "none" and f["adapter"] == "" and f["seed"] == SEQ[:12] and f["seed_count"] == 15 and f["min_count"] == 0
    assert lr.find_adapter(_table({SEQ[:12]: 16}), 100)["status"] != "none"
    assert lr.find_adapter(_table({SEQ[:12]: 16}), 0)["status"] == "none"
    f = lr.find_adapter(_table({}), 0)
    assert f["status"] == "none" and f["seed"] == "AAAAAACCCCCC" and f["seed_count"] == 0       # the smallest eligible code


def test_seed_tie_goes_to_the_smallest_code():
    a, b = "CATGCATGCATT", "CATGCATGCATG"
    assert lr.code_of(b) < lr.code_of(a)
    f = lr.find_adapter(_table({a: 100, b: 100}), 1000)
    assert f["seed"] == b and f["seed_count"] == 100
    assert lr.find_adapter(_table({a: 101, b: 100}), 1000)["seed"] == a


def test_an_ineligible_top_kmer_is_no_seed():
    t = _chain(SEQ[:20], 500)
    t["GGGGGGGAGGGG"] = 100000
    t["AAAAAAACCCCC"] = 100000
    f = lr.find_adapter(_table(t), 1000)
    assert f["seed"] == min(_chain(SEQ[:20], 1), key=lr.code_of) and f["seed_count"] == 500 and f["min_count"] == 16
    assert f["adapter"] == SEQ[:20] and f["status"] == "unsure" and f["left_stop"] == "support"


def test_purity_bound_is_inclusive():
    seed = SEQ[4:16]
    pred = {"A" + seed[:11]: 80, "C" + seed[:11]: 20}                          # 5 * 80 == 4 * 100: accepted
    f = lr.find_adapter(_table({seed: 1000, **pred}), 5000)
    assert f["adapter"] == "A" + seed and f["left_steps"] == 1 and f["left_stop"] == "support"
    pred["C" + seed[:11]] = 21                                                 # 400 < 404: stops, and that is the adapter's start
    f = lr.find_adapter(_table({seed: 1000, **pred}), 5000)
    assert f["adapter"] == seed and f["left_steps"] == 0 and f["left_stop"] == "purity" and f["status"] == "ok"
    # the right walk under the same bound
    f = lr.find_adapter(_table({seed: 1000, seed[1:] + "G": 80, seed[1:] + "T": 20}), 5000)
    assert f["adapter"] == seed + "G"
    assert lr.find_adapter(_table({seed: 1000, seed[1:] + "G": 80, seed[1:] + "T": 21}), 5000)["adapter"] == seed


def test_support_bound_is_inclusive_and_comes_first():
    seed = SEQ[4:16]
    t = {seed: 64 * 40}                                                        # minc = 40
    f = lr.find_adapter(_table({**t, "G" + seed[:11]: 40}), 5000)
    assert f["min_count"] == 40 and f["adapter"] == "G" + seed and f["left_steps"] == 1
    f = lr.find_adapter(_table({**t, "G" + seed[:11]: 39}), 5000)
    assert f["adapter"] == seed and f["left_stop"] == "support" and f["status"] == "unsure"
    # m < minc is tested before purity: 39 of 39 + 39 is impure as well, and the stop is still support
    f = lr.find_adapter(_table({**t, "G" + seed[:11]: 39, "T" + seed[:11]: 39}), 5000)
    assert f["left_stop"] == "support"
    assert lr.find_adapter(_table({seed: 64 * 16 + 63}), 10)["min_count"] == 16 and lr.find_adapter(_table({seed: 64 * 17}), 10)["min_count"] == 17
    # a tie between predecessors goes to the first of A, C, G, T -- here both at 50 %: impure
    f = lr.find_adapter(_table({**t, "C" + seed[:11]: 50, "G" + seed[:11]: 50}), 5000)
    assert f["left_stop"] == "purity"


def test_a_long_left_walk_is_cut_to_64():
    rng = np.random.RandomState(5)
    while True:
        seq = "".join("ACGT"[x] for x in rng.randint(0, 4, size=200))
        kmers = [seq[i:i + 12] for i in range(189)]
        if len(set(kmers)) == 189 and all(lr.eligible(k) for k in kmers):
            break
    t = _chain(seq, 100)
    t[seq[-12:]] = 101                                                         # the seed is the last 12-mer: everything else lies to its left
    f = lr.find_adapter(_table(t), 1000)
    assert f["seed"] == seq[-12:] and f["left_steps"] == 188 and f["left_stop"] == "support" and f["status"] == "unsure"
    assert f["adapter"] == seq[:64] and len(f["adapter"]) == lr.ADAPTER_MAX
    # a cycle never ends by itself: the cap does it
    loop = "ACGTTGCAAGCTTAGG"
    f = lr.find_adapter(_table(_chain(loop * 3, 100)), 1000)
    assert f["left_stop"] == "cap" and f["left_steps"] == lr.LEFT_CAP - 12 and f["status"] == "unsure" and len(f["adapter"]) == 64


# ---- the two restatements

SMALL = [b"", b">a\nACGTACGTACGTA\n", b"@a\nACGTACGTACGT\n+\nIIIIIIIIIIII\n", b"@a\nacgtnACGTACGTACGTAn\n+\n" + b"5" * 19 + b"\n",
         b">a\n\n>b\nACGTACGTAC\nGTACGT\n>c x\r\nTTTTTTTTTTTTTTTT\r\n"]


@pytest.mark.parametrize("i", range(len(SMALL)))
def test_restatements_agree_on_small_inputs(i):
    for kw in (dict(), dict(adapter="ACGT", overlap=2), dict(adapter="gtac", e_pm=250, sample=1)):
        assert lr.same(lr.restate_libqc(SMALL[i], **kw), lr.restate_libqc_numpy(SMALL[i], **kw)), kw


def test_restatement_by_hand():
    res = lr.restate_libqc(b"@a\nACGTACGTACGTN\n+\n" + b"+5?I" * 3 + b"!\n@c\n\n+\n\n" + b"@b\nacgtacgtacgta\n+\n" + b"I" * 13 + b"\n", adapter="TACG", overlap=4, e_pm=0)
    assert res["reads"] == 3 and res["sampled"] == 3 and res["status"] == "none" and res["with_adapter"] == 2 and res["dimers"] == 0
    t = res["table"]
    assert t[lr.code_of("ACGTACGTACGT")] == 2 and t[lr.code_of("CGTACGTACGTA")] == 1 and t.sum() == 3          # ...GTN holds no further 12-mer
    assert res["raw_len"][13] == 2 and res["raw_len"][0] == 1 and res["raw_len"].sum() == 3
    assert list(res["cycles"][0]) == [2, 0, 0, 0, 0, 10 + 40] and list(res["cycles"][12]) == [1, 0, 0, 0, 1, 0 + 40] and res["cycles"][13].sum() == 0
    assert list(res["insert"][3]) == [2, 0, 0, 0, 0, 2] and list(res["insert"][0]) == [0, 0, 0, 0, 1, 1] and res["insert"].sum() == 6
    res = lr.restate_libqc(b">d\nTACGAAAA\n>e\nNTACG\n", adapter="TACG", overlap=4, e_pm=0)
    assert res["dimers"] == 1 and list(res["insert"][0]) == [0, 0, 0, 0, 1, 1] and list(res["insert"][1]) == [0, 0, 0, 0, 1, 1]
    with pytest.raises(Refused):
        lr.restate_libqc(b"@a\nAC\n+\nI\n")
    summary, lengths, cycles = lr.render(lr.restate_libqc(b"@a\nACG\n+\n+5?\n@b\nAC\n+\n+,\n", adapter="CG", overlap=2))
    assert summary == (b"reads\t2\nsampled\t2\nadapter\t\nstatus\tnone\nseed\tAAAAAACCCCCC\nseed_count\t0\nleft_steps\t0\nleft_stop\tpurity\n"
                       b"with_adapter\t1\ndimers\t0\ninsert_mode\t1\n")
    assert lengths == b"length\traw\tinserts\tA\tC\tG\tT\tother\n0\t0\t0\t0\t0\t0\t0\t0\n1\t0\t1\t1\t0\t0\t0\t0\n2\t1\t1\t1\t0\t0\t0\t0\n3\t1\t0\t0\t0\t0\t0\t0\n"
    assert cycles == b"cycle\tA\tC\tG\tT\tother\tmean_quality\n1\t2\t0\t0\t0\t0\t10.000\n2\t0\t2\t0\t0\t0\t15.500\n3\t0\t0\t1\t0\t0\t30.000\n"


@pytest.mark.parametrize("name", sorted(LIBRARIES))
def test_synthetic_libraries(name):
    data, want = library(name), LIBRARIES[name][1]
    res = lr.restate_libqc_numpy(data)
    assert res["reads"] == N_READS and res["status"] == want, (res["status"], res["adapter"], res["left_stop"], res["left_steps"])
    if want == "ok":
        assert is_truth(res["adapter"], planted(name)), res["adapter"]
        assert res["left_stop"] == "purity"
    else:
        assert res["left_stop"] == "support"
    # the plain restatement: the table and the walk on the whole library, every table on its first 2,000 reads, also under a sample below that
    table = lr.table_plain([r for _, r, _ in make_library(**LIBRARIES[name][0])])
    assert np.array_equal(table, res["table"])
    part = head(data, 2000)
    for kw in (dict(), dict(sample=1000)):
        assert lr.same(lr.restate_libqc(part, **kw), lr.restate_libqc_numpy(part, **kw)), kw


# ---- the verb's and trim's argument paths

def run_cli(module, args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd." + module] + args, cwd=cwd, capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_libqc_option_errors_exit_2_before_a_device(tmp_path):
    fq = tmp_path / "a.fastq"
    fq.write_bytes(b"@a\nACGT\n+\nIIII\n")
    bad = [[], ["-a", "ACGU", str(fq)], ["-a", "auto", str(fq)], ["-a", "A" * 65, str(fq)], ["-e", "1", str(fq)], ["-O", "0", str(fq)], ["-O", "65", str(fq)],
           ["-a", "ACG", "-O", "4", str(fq)], ["--sample", "0", str(fq)], ["--sample", str(2 ** 26 + 1), str(fq)], ["--device", "-1", str(fq)], ["-q", "20", str(fq)]]
    for args in bad:
        r = run_cli("libqc", args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
    r = run_cli("libqc", [str(tmp_path / "nope.fastq")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ")
    assert not list(tmp_path.glob("*.libqc*"))


def test_libqc_helpers():
    from mir_prefer_amd import libqc
    assert libqc.output_names("d/lib.fastq.gz") == ("d/lib.fastq.libqc.tsv", "d/lib.fastq.libqc.lengths.tsv", "d/lib.fastq.libqc.cycles.tsv")
    assert libqc.parse_args(["x.fq"])[0].sample == 2 ** 20 == lr.SAMPLE
    for data in SMALL + [head(library("dimers50"), 300)]:
        res = lr.restate_libqc_numpy(data)
        assert libqc.render(res) == lr.render(res)
    res = lr.restate_libqc_numpy(head(library("36nt"), 500))
    assert libqc.insert_mode(res["insert"]) == lr.insert_mode(res["insert"]) > 0
    tie = np.zeros((1025, 6), np.int64)
    tie[[21, 24], 5] = 7
    assert libqc.insert_mode(tie) == lr.insert_mode(tie) == 21 and libqc.insert_mode(tie * 0) == lr.insert_mode(tie * 0) == 0
    assert "trim -a ACGTACGTACGT lib.fq" in libqc.advice("lib.fq", dict(status="ok", adapter="ACGTACGTACGT"))
    assert "unsure" in libqc.advice("lib.fq", dict(status="unsure", adapter="ACGTACGTACGT", left_stop="support"))
    assert "no adapter" in libqc.advice("lib.fq", dict(status="none", adapter=""))


class _StubContext:
    """Stands in for capi.Context: libqc_reads answers from the class attribute, trim_reads records its arguments."""
    answer = None
    calls = []

    def __init__(self, device):
        type(self).calls = [("open", device)]

    def libqc_reads(self, data, name, **kw):
        self.calls.append(("libqc", bytes(data), name, kw))
        return dict(type(self).answer)

    def trim_reads(self, data, name, out_path, **kw):
        self.calls.append(("trim", bytes(data), name, out_path, kw))
        return dict(reads=1, quality_trimmed=0, adapter=1, untrimmed=0, too_short=0, too_long=0, written=1, seconds=[0] * 6)

    def close(self):
        self.calls.append(("close",))


def test_trim_a_auto_passes_the_found_adapter_on(tmp_path, monkeypatch, capsys):
    from mir_prefer_amd import capi, trim
    monkeypatch.setattr(capi, "Context", _StubContext)
    fq = tmp_path / "a.fastq"
    fq.write_bytes(b"@a\nACGT\n+\nIIII\n")
    _StubContext.answer = dict(status="ok", adapter="TGGAATTCTCGGGTGCCAAGGAACTCC", left_stop="purity")
    assert trim.main(["-a", "auto", "-q", "20", "--device", "1", str(fq)]) == 0
    calls = _StubContext.calls
    assert [c[0] for c in calls] == ["open", "libqc", "trim", "close"] and calls[0][1] == 1
    assert calls[1][1] == fq.read_bytes() and calls[1][2] == str(fq) and calls[1][3] == {}            # the detection's defaults, on the file's bytes
    kw = calls[2][4]
    assert kw["adapter"] == "TGGAATTCTCGGGTGCCAAGGAACTCC" and kw["overlap"] == 3 and kw["quality"] == 20 and kw["error_permille"] == 100
    err = capsys.readouterr().err
    assert "TGGAATTCTCGGGTGCCAAGGAACTCC" in err and str(fq) in err
    # -O is checked against the found adapter
    assert trim.main(["-a", "auto", "-O", "27", str(fq)]) == 0 and _StubContext.calls[2][4]["overlap"] == 27
    assert trim.main(["-a", "auto", "-O", "28", str(fq)]) == 255 and [c[0] for c in _StubContext.calls] == ["open", "libqc", "close"]
    # a given adapter never runs the detection
    assert trim.main(["-a", "ACGTAC", str(fq)]) == 0 and [c[0] for c in _StubContext.calls] == ["open", "trim", "close"]


@pytest.mark.parametrize("status,adapter", [("unsure", "ACGTTGCAAGCTTAGG"), ("none", "")])
def test_trim_a_auto_refuses_without_a_sure_adapter(tmp_path, monkeypatch, capsys, status, adapter):
    from mir_prefer_amd import capi, trim
    monkeypatch.setattr(capi, "Context", _StubContext)
    fq = tmp_path / "a.fastq"
    fq.write_bytes(b"@a\nACGT\n+\nIIII\n")
    (tmp_path / "a.fastq.trimmed.fa").write_bytes(b"stale")
    _StubContext.answer = dict(status=status, adapter=adapter, left_stop="support")
    assert trim.main(["-a", "auto", str(fq), str(fq)]) == 255
    assert [c[0] for c in _StubContext.calls] == ["open", "libqc", "close"]                           # nothing is trimmed, the second file is not reached
    err = capsys.readouterr().err
    assert err.startswith("Error: ") and "status " + status in err and (adapter or "candidate -") in err and "mir_prefer_amd.libqc" in err
    assert not (tmp_path / "a.fastq.trimmed.fa").exists()


def test_auto_is_still_no_adapter_elsewhere(tmp_path):
    fq = tmp_path / "a.fastq"
    fq.write_bytes(b"@a\nACGT\n+\nIIII\n")
    for args in (["-a", "Auto", str(fq)], ["-a", "auto", "-O", "65", str(fq)], ["-a", "auto", "-e", "2", str(fq)]):
        assert run_cli("trim", args, tmp_path).returncode == 2, args


# ---- the C-ABI

def test_entries_are_declared_defined_and_bound(tmp_path):
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    csrc = os.path.join(ROOT, "mir-prefer_amd", "csrc")
    assert "int mirp_libqc_reads(mirp_ctx* ctx, const char* data, int64_t n, const char* name, const MirpLibqcOpts* opts, MirpLibqcFound* found," in header
    assert "int mirp_libqc_last_table(mirp_ctx* ctx, uint32_t out[1 << 24]);" in header
    host = open(os.path.join(csrc, "mirp_libqc.cpp")).read()
    assert 'extern "C" int mirp_libqc_reads(' in host and 'extern "C" int mirp_libqc_last_table(' in host
    assert "mirp_libqc.cpp" in open(os.path.join(csrc, "Makefile")).read()
    kernels = open(os.path.join(csrc, "libqc_kernels.hip")).read()
    for const in ("LQ_K %d " % lr.K, "LQ_W %d " % lr.W, "LQ_MIN_COUNT %d" % lr.MIN_COUNT, "LQ_LEFT_CAP %d " % lr.LEFT_CAP):
        assert "#define " + const in kernels, const
    from mir_prefer_amd import capi
    assert callable(capi.Context.libqc_reads) and callable(capi.Context.libqc_last_table)
    assert capi.LIBQC_STATUS == (lr.NONE, lr.OK, lr.UNSURE) and capi.LIBQC_STOPS == lr.STOPS and capi.LIBQC_SAMPLE == lr.SAMPLE
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirprefer.h"\nint main(void) {\n'
                   ' printf("%zu %zu %zu %zu %zu %d %d %d", sizeof(MirpLibqcOpts), offsetof(MirpLibqcOpts, sample), sizeof(MirpLibqcFound),\n'
                   '        offsetof(MirpLibqcFound, status), offsetof(MirpLibqcFound, seed_count), MIRP_LIBQC_NONE, MIRP_LIBQC_OK, MIRP_LIBQC_UNSURE);\n return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().split()
    want = [C.sizeof(capi.LibqcOpts), capi.LibqcOpts.sample.offset, C.sizeof(capi.LibqcFound), capi.LibqcFound.status.offset, capi.LibqcFound.seed_count.offset, 0, 1, 2]
    assert [int(x) for x in got] == want and want[:3] == [88, 80, 104]
