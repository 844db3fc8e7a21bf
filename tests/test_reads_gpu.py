"""GPU tests of the read collapse (mirp_collapse_reads, reads_kernels.hip): byte for byte against the reference's process-reads-fasta.py on the
fixtures, against a plain dict restatement on seeded random files, under forced hash collisions, past 2^31 bytes, the refusal of non-ASCII
input, the command line on three samples, and the collapsed ids read back by the SAM ingest as depths."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as gu
from tests.test_reads_cpu import ROOT, restate_collapse

pytestmark = pytest.mark.gpu
GOLD = gu.load_json("reads.json.gz")


def _collapse(ctx, tmp_path, data, prefix="S1", hash_bits=64, name="in.fa"):
    p = tmp_path / name
    p.write_bytes(data)
    res = ctx.collapse_reads(str(p), prefix, str(p) + ".processed", hash_bits=hash_bits)
    return open(str(p) + ".processed", "rb").read(), res


def _check(ctx, tmp_path, data, hash_bits=64):
    got, res = _collapse(ctx, tmp_path, data, hash_bits=hash_bits)
    want, n = restate_collapse(data, "S1")
    assert res["n_unique"] == n
    assert got == want
    return res


def _pool(rng, n, lo, hi, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return [a[rng.randint(0, len(a), size=rng.randint(lo, hi + 1))].tobytes() for _ in range(n)]


def _join(rng, lines, eols=(b"\n",)):
    if len(eols) == 1:
        return eols[0].join(lines) + eols[0]
    pick = rng.randint(0, len(eols), size=len(lines))
    return b"".join(x + eols[k] for x, k in zip(lines, pick))


def test_collapse_matches_reference_fixtures(gpu_ctx, tmp_path):
    for c in GOLD["collapse"]:
        got, res = _collapse(gpu_ctx, tmp_path, c["input"].encode("latin-1"), prefix=c["prefix"], name=c["name"] + ".fa")
        assert got == c["output"].encode("latin-1"), c["name"]
        assert res["n_unique"] == c["unique"], c["name"]


def test_collapse_zipf_duplicated(gpu_ctx, tmp_path):
    rng = np.random.RandomState(11)
    pool = _pool(rng, 200000, 18, 26)
    idx = np.minimum(rng.zipf(1.3, size=1600000) - 1, len(pool) - 1)
    reads = [pool[k] for k in idx] + _pool(rng, 400000, 18, 26)
    rng.shuffle(reads)
    lines = []
    for k, r in enumerate(reads):
        lines.append(b">q%d" % k)
        lines.append(r)
    res = _check(gpu_ctx, tmp_path, _join(rng, lines))
    assert res["n_reads"] == 2000000 and res["collisions"] == 0


def test_collapse_all_unique_and_all_identical(gpu_ctx, tmp_path):
    rng = np.random.RandomState(12)
    reads = sorted(set(_pool(rng, 300000, 30, 40)))
    rng.shuffle(reads)
    res = _check(gpu_ctx, tmp_path, _join(rng, reads))
    assert res["n_unique"] == len(reads)
    res = _check(gpu_ctx, tmp_path, b"TGAGGTAGTAGGTTGTATAGTT\n" * 500000)
    assert res["n_unique"] == 1


def test_collapse_lengths_0_to_300_and_a_100kb_line(gpu_ctx, tmp_path):
    rng = np.random.RandomState(13)
    pool = [r[:k] for r in _pool(rng, 3000, 300, 300, b"ACGTNacgt") for k in (rng.randint(0, 301),)]
    lines = [pool[k] for k in rng.randint(0, len(pool), size=60000)]
    big = _pool(rng, 1, 100000, 100000)[0]
    lines[20000:20000] = [big, b"  " + big + b"\t", big[:-1]]
    _check(gpu_ctx, tmp_path, _join(rng, lines))


def test_collapse_crlf_and_lone_cr(gpu_ctx, tmp_path):
    rng = np.random.RandomState(14)
    pool = _pool(rng, 5000, 0, 40) + [b" ", b"\t", b">h", b" >h", b"\x0b", b"A\x1c"]
    lines = [pool[k] for k in rng.randint(0, len(pool), size=300000)]
    _check(gpu_ctx, tmp_path, _join(rng, lines, (b"\n", b"\r\n", b"\r")))
    _check(gpu_ctx, tmp_path, _join(rng, lines, (b"\r",))[:-1])


def test_collapse_forced_hash_collisions_stay_exact(gpu_ctx, tmp_path):
    """4-bit hashes: 16 hash runs for thousands of distinct reads, every run fails verification and is resolved exactly."""
    rng = np.random.RandomState(15)
    pool = _pool(rng, 20000, 15, 30)
    lines = [pool[k] for k in np.minimum(rng.zipf(1.2, size=200000) - 1, len(pool) - 1)]
    res = _check(gpu_ctx, tmp_path, _join(rng, lines, (b"\n", b"\r\n")), hash_bits=4)
    assert res["collisions"] > res["n_reads"] // 2
    res = _check(gpu_ctx, tmp_path, b"ACGT\nACGT\n", hash_bits=4)
    assert res["collisions"] == 0


def test_collapse_file_past_2gib(gpu_ctx, tmp_path):
    """K distinct reads repeated M times, more than 2^31 bytes: the answer is K records `_x<M>` in block order."""
    rng = np.random.RandomState(16)
    reads = sorted(set(_pool(rng, 4096, 100, 300)))
    rng.shuffle(reads)
    block = b"".join(b">h\n" + r + b"\n" for r in reads)
    m = (2 ** 31) // len(block) + 2
    p = tmp_path / "big.fa"
    with open(p, "wb") as f:
        for _ in range(m):
            f.write(block)
    assert os.path.getsize(p) > 2 ** 31
    res = gpu_ctx.collapse_reads(str(p), "B", str(p) + ".processed")
    os.unlink(p)
    want = b"".join(b">B_r%d_x%d\n%s\n" % (k, m, r) for k, r in enumerate(reads))
    assert res["n_reads"] == len(reads) * m and res["n_unique"] == len(reads)
    assert open(str(p) + ".processed", "rb").read() == want


def test_collapse_refuses_non_ascii_with_offset(gpu_ctx, tmp_path):
    from mir_prefer_amd import capi
    p = tmp_path / "u.fa"
    p.write_bytes(b"ACGT\n" * 1000 + b"AC\xc3\xa9GT\n" + b"TT\n")
    with pytest.raises(capi.MirpError) as e:
        gpu_ctx.collapse_reads(str(p), "S1", str(p) + ".processed")
    assert str(p) in str(e.value) and "offset 5002" in str(e.value)
    assert not os.path.exists(str(p) + ".processed")


def test_cli_collapses_three_samples(tmp_path):
    rng = np.random.RandomState(17)
    pool = _pool(rng, 2000, 18, 24)
    paths, datas = [], []
    for s in range(3):
        lines = []
        for k in np.minimum(rng.zipf(1.5, size=30000) - 1, len(pool) - 1):
            lines += [b">x%d" % len(lines), pool[k]]
        datas.append(_join(rng, lines))
        p = tmp_path / ("s%d.fa" % s)
        p.write_bytes(datas[-1])
        paths.append(str(p))
    (tmp_path / "names.txt").write_text("root\nleaf\n\nflower\n")
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.reads", "collapse", "--device", "0", str(tmp_path / "names.txt")] + paths, cwd=str(tmp_path),
                       capture_output=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
    out = r.stdout.decode()
    for p, d, name in zip(paths, datas, ["root", "leaf", "flower"]):
        want, n = restate_collapse(d, name)
        assert open(p + ".processed", "rb").read() == want
        assert "Start processing file %s\nFinish file %s\n" % (p, p) in out and "File %s has %d unique reads\n" % (p, n) in out
    assert out.endswith("DONE\n\n")


def test_collapsed_ids_give_the_ingest_its_depths(gpu_ctx, tmp_path):
    """The collapse's ids are what the pipeline parses (`_xN`, miR_PREFeR.py:242-253): through a SAM and mirp_ingest_sams_gpu they come back as
    MirpAln.depth equal to the counts."""
    rng = np.random.RandomState(18)
    pool = _pool(rng, 500, 18, 24)
    lines = []
    for k in np.minimum(rng.zipf(1.4, size=20000) - 1, len(pool) - 1):
        lines += [b">x", pool[k]]
    got, res = _collapse(gpu_ctx, tmp_path, _join(rng, lines), prefix="leaf")
    recs = got.decode().split("\n")[:-1]
    ids, seqs = recs[0::2], recs[1::2]
    counts = {}
    for ln in lines[1::2]:
        counts[ln.decode()] = counts.get(ln.decode(), 0) + 1
    sam = tmp_path / "leaf.sam"
    with open(sam, "w") as f:
        f.write("@SQ\tSN:chr1\tLN:100000\n")
        for k, (q, s) in enumerate(zip(ids, seqs)):
            f.write("%s\t0\tchr1\t%d\t255\t%dM\t*\t0\t0\t%s\t*\n" % (q[1:], 1 + 50 * k, len(s), s))
    cn, cl, sn, alns, segs, sec = gpu_ctx.ingest_sams([str(sam)])
    assert len(alns) == len(ids) == res["n_unique"]
    assert list(alns["pos"]) == [1 + 50 * k for k in range(len(ids))]
    assert list(alns["depth"]) == [counts[s] for s in seqs]
    assert sum(counts.values()) == res["n_reads"]
