"""GPU tests of the read alignment (mirp_align_index / mirp_align_reads, align_kernels.hip): the whole .sam bytes against the brute-force
restatement of tests/test_align_cpu.py over -v 0..3, -k, -m and -f on small genomes with the hard cases; -v 0 at scale against the searchsorted
restatement; positions past 2^31; several read files in one invocation; the round trip through both SAM ingest paths and the candidate stage; the
chain of the three command lines; and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_align_cpu import (CODE, ROOT, brute_hits, load_reads, load_reference, normalise_pg, revcomp, sam_bytes, searchsorted_hits_v0)

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _letters(codes, rng=None, lower=0.0):
    s = ACGT[np.minimum(codes, 3)].copy()
    s[codes > 3] = ord("N")
    if rng is not None and lower:
        low = rng.rand(len(s)) < lower
        s[low] += 32
    return s.tobytes()


def _write_fasta(path, records, width=60):
    with open(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + name.encode() + b" some description\n")
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + b"\n")


def _genome(rng):
    """Three contigs over two files, not in lexicographic order, with lower case, N runs, IUPAC codes, tandem repeats and a palindrome."""
    def rnd(n):
        return ACGT[rng.randint(0, 4, n)].copy()
    z = rnd(7000)
    z[1200:1260] = ord("N")
    z[3000] = ord("R"); z[3001] = ord("y"); z[4500] = ord("-")
    z[2000:2400] = np.tile(rnd(8), 50)                      # short tandem repeat: reads hit many offsets
    unit = rnd(23)
    z[5000:5000 + 23 * 40] = np.tile(unit, 40)              # 40 copies of a 23-mer
    x = rnd(10)
    pal = np.concatenate([x, ACGT[3 - CODE[x]][::-1]])      # reverse-complement palindrome: one offset, both strands
    z[6000:6020] = pal
    z[100:400] = z[100:400] + 32                            # lower case
    ten = rnd(3500)
    ten[0:5] = ord("N")
    ten[-3:] = ord("n")
    a = rnd(2600)
    a[1000:1005] = ord("K")
    return [[("chrZ", z.tobytes()), ("chr10", ten.tobytes())], [("chrA", a.tobytes()), ("chrEmpty", b"")]]


def _reads(rng, names, seqs, n=700):
    out = []
    for k in range(n):
        kind = k % 10
        L = int(rng.randint(12, 31))
        if kind == 9:
            r = rng.randint(0, 4, L).astype(np.uint8)                       # random
        else:
            t = int(rng.randint(0, len(seqs)))
            s = seqs[t]
            if kind == 0:
                o = 0                                                      # contig start
            elif kind == 1:
                o = len(s) - L                                             # contig end
            elif kind == 2 and t == 0:
                o = int(rng.choice([2000 + int(rng.randint(0, 300)), 5000 + int(rng.randint(0, 800)), 6000]))
                L = 20 if o == 6000 else L
            else:
                o = int(rng.randint(0, len(s) - L))
            r = s[o:o + L].copy()
            r[r > 3] = rng.randint(0, 4, int((r > 3).sum()))
            if rng.rand() < 0.5:
                r = revcomp(r)
            for _ in range(int(rng.randint(0, 4))):                          # 0..3 substitutions
                i = int(rng.randint(0, L))
                r[i] = (r[i] + 1 + rng.randint(0, 3)) % 4
            if kind == 8:
                r[int(rng.randint(0, L))] = 4                                # a read N
        out.append(r)
    for L in (0, 1, 2, 3):                                                   # L <= v for some v
        out.append(rng.randint(0, 4, L).astype(np.uint8))
    out.append(np.full(25, 4, np.uint8))
    out.append(seqs[0][6000:6020].copy())                                    # the palindrome itself
    return out


def _write_reads(path, reads, rng, sample="S1"):
    with open(path, "wb") as f:
        for k, r in enumerate(reads):
            s = _letters(r, rng, lower=0.1)
            f.write(b">%s_r%d_x%d\n" % (sample.encode(), k, 1 + k % 7))
            if len(s) > 15 and k % 4 == 0:
                f.write(s[:9] + b"\n" + s[9:] + b"\n")                         # multi-line sequence
            else:
                f.write(s + b"\n")


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_small")
    rng = np.random.RandomState(31)
    files = []
    for i, recs in enumerate(_genome(rng)):
        p = d / ("ref%d.fa" % i)
        _write_fasta(p, recs)
        files.append(str(p))
    names, seqs = load_reference(files)
    assert names == ["chrZ", "chr10", "chrA"]
    reads_p = d / "reads.fa"
    _write_reads(reads_p, _reads(rng, names, seqs), rng)
    reads = load_reads(str(reads_p))
    hits = brute_hits(seqs, reads, vmax=3)
    return {"dir": d, "refs": files, "names": names, "seqs": seqs, "reads_path": str(reads_p), "reads": reads, "hits": hits}


def test_brute_force_parity_over_options(gpu_ctx, small):
    idx = gpu_ctx.align_index(small["refs"])
    assert idx["n_contigs"] == 3 and idx["total"] == sum(len(s) for s in small["seqs"])
    out = str(small["dir"] / "out.sam")
    seen_m = 0
    for v in range(4):
        for k in (1, 20, 10 ** 6):
            for m in (0, 3):
                for f in (False, True):
                    res = gpu_ctx.align_reads(small["reads_path"], out, "x", v=v, k=k, m=m, filter_unmapped=f)
                    want = sam_bytes(small["names"], small["seqs"], small["reads"], small["hits"], v, k, m, f)
                    got = open(out, "rb").read()
                    assert normalise_pg(got) == want, (v, k, m, f)
                    assert res["reads"] == len(small["reads"]) == res["aligned"] + res["unaligned"] + res["suppressed"]
                    assert res["records"] == want.count(b"\n") - 5
                    seen_m += res["suppressed"]
    assert seen_m > 0                           # -m suppressed reads somewhere in the grid
    # the hard cases are present: both strands at one offset, reads at contig ends, more than 20 hits
    pal = [hs for (q, r), hs in zip(small["reads"], small["hits"]) if len(r) == 20 and any(h[1] == 6000 and h[2] == 1 for h in hs)]
    assert pal and any((0, 6000, 0, 0) in hs and (0, 6000, 1, 0) in hs for hs in pal)
    assert any(len([h for h in hs if h[3] == 0]) > 20 for hs in small["hits"])


def test_v0_at_scale_against_searchsorted(gpu_ctx, tmp_path):
    rng = np.random.RandomState(5)
    g = [rng.randint(0, 4, 5_000_000).astype(np.uint8), rng.randint(0, 4, 3_000_000).astype(np.uint8)]
    g[0][1_000_000:1_000_500] = 4
    g[1][200_000:200_000 + 30 * 400] = np.tile(g[1][200_000:200_030], 400)
    _write_fasta(tmp_path / "g.fa", [("c1", _letters(g[0])), ("c2", _letters(g[1]))], width=80)
    seen, reads = set(), []
    while len(reads) < 200_000:
        L = int(rng.randint(18, 27))
        kind = int(rng.randint(0, 4))            # 0 forward, 1 reverse strand, 2 one substitution, 3 random
        if kind == 3:
            r = rng.randint(0, 4, L).astype(np.uint8)
        else:
            t = int(rng.randint(0, 2))
            if rng.rand() < 0.05:                # inside the tandem repeat of c2: many hits
                t, o = 1, 200_000 + int(rng.randint(0, 400 * 30 - L))
            else:
                o = int(rng.randint(0, len(g[t]) - L))
            r = g[t][o:o + L].copy()
            if (r > 3).any():
                continue
            if kind == 1:
                r = revcomp(r)
            if kind == 2:
                r[int(rng.randint(0, L))] ^= 1
        b = r.tobytes()
        if b in seen:
            continue
        seen.add(b)
        reads.append(r)
    with open(tmp_path / "r.fa", "wb") as f:
        for k, r in enumerate(reads):
            f.write(b">S_r%d_x1\n%s\n" % (k, _letters(r)))
    gpu_ctx.align_index([str(tmp_path / "g.fa")])
    res = gpu_ctx.align_reads(str(tmp_path / "r.fa"), str(tmp_path / "r.sam"), "x", v=0, k=20)
    rd = load_reads(str(tmp_path / "r.fa"))
    hits = searchsorted_hits_v0(g, rd)
    want = sam_bytes(["c1", "c2"], g, rd, hits, 0, 20)
    assert normalise_pg(open(tmp_path / "r.sam", "rb").read()) == want
    assert res["aligned"] > 90_000 and any(len(h) > 20 for h in hits)


def test_positions_past_2_31(gpu_ctx, tmp_path):
    rng = np.random.RandomState(9)
    pad = 2 ** 31 + 1234
    tail = rng.randint(0, 4, 1 << 20).astype(np.uint8)
    other = rng.randint(0, 4, 20000).astype(np.uint8)
    p = tmp_path / "big.fa"
    line = b"N" * 4095 + b"\n"
    chunk = line * 16384
    with open(p, "wb") as f:
        f.write(b">big\n")
        left = pad
        while left >= len(line) * 16384:
            f.write(chunk)
            left -= 4095 * 16384
        f.write(b"N" * left + b"\n")
        f.write(_letters(tail) + b"\n>other\n" + _letters(other) + b"\n")
    reads = []
    for k in range(400):
        L = int(rng.randint(18, 27))
        src = tail if k % 4 else other
        o = len(src) - L if k % 50 == 1 else int(rng.randint(0, len(src) - L))
        r = src[o:o + L].copy()
        if k % 3 == 0:
            r = revcomp(r)
        if k % 5 == 0:
            r[int(rng.randint(0, L))] ^= 2
        reads.append(("S_r%d_x1" % k, r))
    with open(tmp_path / "r.fa", "wb") as f:
        for q, r in reads:
            f.write(b">%s\n%s\n" % (q.encode(), _letters(r)))
    idx = gpu_ctx.align_index([str(p)])
    os.unlink(p)
    assert idx["total"] == pad + len(tail) + len(other) > 2 ** 31
    res = gpu_ctx.align_reads(str(tmp_path / "r.fa"), str(tmp_path / "r.sam"), "x", v=1, k=20)
    got = open(tmp_path / "r.sam", "rb").read().decode().splitlines()
    # the restatement on the non-N part, positions on `big` moved by the N prefix
    hits = brute_hits([tail, other], reads, vmax=1)
    want = sam_bytes(["big", "other"], [tail, other], reads, hits, 1, 20).decode().splitlines()
    want[1] = "@SQ\tSN:big\tLN:%d" % (pad + len(tail))
    for i in range(4, len(want)):
        f = want[i].split("\t")
        if f[2] == "big":
            f[3] = str(int(f[3]) + pad)
            want[i] = "\t".join(f)
    assert got[:3] == want[:3] and got[4:] == want[4:]          # @HD, the two @SQ lines, the records (the @PG lines differ)
    assert res["aligned"] > 380 and any(int(ln.split("\t")[3]) > 2 ** 31 for ln in got[3:] if ln.split("\t")[2] == "big")


def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.align"] + args, cwd=cwd, capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_several_read_files_in_one_invocation(gpu_ctx, small, tmp_path):
    rng = np.random.RandomState(77)
    paths = []
    for i, sample in enumerate(["root", "leaf", "flower"]):
        rd = _reads(rng, small["names"], small["seqs"], n=150 + 40 * i)
        p = tmp_path / (sample + ".fa")
        _write_reads(p, rd, rng, sample)
        paths.append(str(p))
    refs = ["-r", small["refs"][0], "-r", small["refs"][1]]
    r = _cli(["-v", "2", "-k", "5", "-t", str(tmp_path / "idx")] + refs + paths, tmp_path)
    assert r.returncode == 0, r.stderr
    out = r.stdout.decode()
    assert out.count("Indexing reference genomes") == 1 and out.endswith("DONE\nOutput SAM files can be found at:\n" + "".join(p + ".sam\n" for p in paths))
    assert "chrEmpty" in r.stderr.decode() and os.path.isdir(tmp_path / "idx") and not os.listdir(tmp_path / "idx")
    together = [open(p + ".sam", "rb").read() for p in paths]
    assert all(b"\n@PG\tID:mir_prefer_amd.align\tCL:\"python -m mir_prefer_amd.align -v 2 -k 5 " in t for t in together)
    for p, t in zip(paths, together):
        os.unlink(p + ".sam")
        r = _cli(["-v", "2", "-k", "5"] + refs + [p], tmp_path)
        assert r.returncode == 0, r.stderr
        assert normalise_pg(open(p + ".sam", "rb").read()) == normalise_pg(t)
    # one context, one index: repeated calls on it give the same bytes as the first
    gpu_ctx.align_index(small["refs"])
    for p, t in zip(paths, together):
        res = gpu_ctx.align_reads(p, p + ".again", "x", v=2, k=5)
        assert normalise_pg(open(p + ".again", "rb").read()) == normalise_pg(t)
        assert res["reads"] == open(p, "rb").read().count(b">")


COMP = np.full(256, ord("N"), np.uint8)
COMP[list(b"ACGTacgt")] = list(b"TGCATGCA")


def _synth_read(ds, a):
    """The read of a synthetic record: the genome under it, reverse-complemented on -."""
    s = ds.contigs[a["tid"]][1][a["pos"] - 1:a["pos"] - 1 + a["len"]]
    return COMP[s[::-1]] if a["strand"] else s


def _synth_reads(ds, path):
    """The dataset's records as one collapsed FASTA: -> (qname, tid, pos, strand) of the records whose footprint has no N (an alignment never
    covers one)."""
    recs = []
    with open(path, "wb") as f:
        for k, a in enumerate(ds.alns):
            s = _synth_read(ds, a)
            q = "%s_r%d_x%d" % (ds.sample_names[a["sample"]], k, a["depth"])
            f.write(b">%s\n%s\n" % (q.encode(), s.tobytes()))
            if not (CODE[s] > 3).any():
                recs.append((q, int(a["tid"]), int(a["pos"]), int(a["strand"])))
    return recs


def test_round_trip_through_both_ingests_and_the_candidate_stage(gpu_ctx, tmp_path):
    from mir_prefer_amd import capi, ingest, synth
    ds = synth.make_dataset([60000, 40000], 40, n_samples=1, seed=4, contig_names=["chrB", "chrA"], edge_cases=True)
    ds.write_fasta(str(tmp_path / "genome.fa"))
    recs = _synth_reads(ds, tmp_path / "S1.fa")
    gpu_ctx.align_index([str(tmp_path / "genome.fa")])
    gpu_ctx.align_reads(str(tmp_path / "S1.fa"), str(tmp_path / "S1.sam"), "x", v=0, k=1000, filter_unmapped=True)
    got = open(tmp_path / "S1.sam", "rb").read()
    names, seqs = load_reference([str(tmp_path / "genome.fa")])
    rd = load_reads(str(tmp_path / "S1.fa"))
    want = sam_bytes(names, seqs, rd, searchsorted_hits_v0(seqs, rd), 0, 1000, 0, True)
    assert normalise_pg(got) == want
    (tmp_path / "want").mkdir()
    (tmp_path / "want" / "S1.sam").write_bytes(want)
    # every synthetic record is among the alignments; every other alignment matches the genome exactly
    lines = [ln.split("\t") for ln in got.decode().splitlines() if not ln.startswith("@")]
    have = {(f[0], names.index(f[2]), int(f[3]), int(f[1]) >> 4 & 1) for f in lines}
    assert len(recs) > len(ds.alns) - 5 and set(recs) <= have
    for f in lines:
        g = seqs[names.index(f[2])][int(f[3]) - 1:int(f[3]) - 1 + len(f[9])]
        assert f[9] == ACGT[g].tobytes().decode()          # SEQ is on the forward strand (reverse-complemented for flag 16)
    # both SAM ingest paths accept it and agree
    a_nat = capi.ingest_sams([str(tmp_path / "S1.sam")])
    a_py = ingest.read_sams([str(tmp_path / "S1.sam")], native=False)
    assert a_nat[0] == a_py[0] == names and np.array_equal(a_nat[3], a_py[3]) and len(a_nat[3]) == len(lines)
    # the candidate stage gives the same loci on the aligned SAM and on the restatement's
    loci = []
    for p in (tmp_path / "S1.sam", tmp_path / "want" / "S1.sam"):
        cn, cl, sn, alns, segs, sec = gpu_ctx.ingest_sams([str(p)])
        gpu_ctx.load_genome(ds.contigs)
        gpu_ctx.load_alignments(alns)
        order = np.argsort(np.array(cn, dtype=object), kind="stable").astype(np.int32)
        gpu_ctx.candidate(10, 100, 300, order)
        loci.append(gpu_ctx.get_loci()[0])
    assert len(loci[0]) > 0 and loci[0].tobytes() == loci[1].tobytes()


def test_chain_of_the_three_command_lines(tmp_path):
    from mir_prefer_amd import synth
    ds = synth.make_dataset([50000, 30000], 30, n_samples=2, seed=6, contig_names=["chr2", "chr1"])
    ds.write_fasta(str(tmp_path / "genome.fa"))
    raw = []
    for si, sname in enumerate(ds.sample_names):
        p = tmp_path / (sname + ".fa")
        with open(p, "wb") as f:
            for k, a in enumerate(ds.alns[ds.alns["sample"] == si]):
                s = _synth_read(ds, a)
                for j in range(int(a["depth"])):
                    f.write(b">x%d_%d\n%s\n" % (k, j, s.tobytes()))
        raw.append(str(p))
    (tmp_path / "names.txt").write_text("".join(s + "\n" for s in ds.sample_names))
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(mod, args):
        r = subprocess.run([sys.executable, "-m", mod] + args, cwd=tmp_path, capture_output=True, timeout=900, env=env)
        assert r.returncode == 0, (mod, r.stderr.decode())
    run("mir_prefer_amd.reads", ["collapse", str(tmp_path / "names.txt")] + raw)
    run("mir_prefer_amd.align", ["-f", "-r", str(tmp_path / "genome.fa")] + [p + ".processed" for p in raw])
    names, seqs = load_reference([str(tmp_path / "genome.fa")])
    (tmp_path / "want").mkdir()
    for p in raw:
        rd = load_reads(p + ".processed")
        (tmp_path / "want" / (os.path.basename(p) + ".processed.sam")).write_bytes(sam_bytes(names, seqs, rd, searchsorted_hits_v0(seqs, rd), 0, 20, 0, True))
        assert normalise_pg(open(p + ".processed.sam", "rb").read()) == (tmp_path / "want" / (os.path.basename(p) + ".processed.sam")).read_bytes()
    results = []
    for tag, sams in (("got", [p + ".processed.sam" for p in raw]), ("want", [str(tmp_path / "want" / (os.path.basename(p) + ".processed.sam")) for p in raw])):
        cfg = tmp_path / ("config_" + tag)
        cfg.write_text("FASTA_FILE = %s\nALIGNMENT_FILE = %s\nPRECURSOR_LEN = 300\nREADS_DEPTH_CUTOFF = 20\nMAX_GAP = 100\nMIN_MATURE_LEN = 18\n"
                       "MAX_MATURE_LEN = 24\nALLOW_NO_STAR_EXPRESSION = Y\nALLOW_3NT_OVERHANG = N\nOUTFOLDER = %s\nNAME_PREFIX = chain\n"
                       % (tmp_path / "genome.fa", ", ".join(sams), tmp_path / ("out_" + tag)))
        run("mir_prefer_amd.cli", ["pipeline", str(cfg)])
        out = tmp_path / ("out_" + tag)
        results.append([open(out / fn, "rb").read() for fn in ("chain_miRNA.gff3", "chain_miRNA.mature.fa", "chain_miRNA.precursor.fa")])
    assert results[0] == results[1] and results[0][0].count(b"\n") > 1


def test_refusals_write_nothing(gpu_ctx, tmp_path):
    from mir_prefer_amd import capi
    (tmp_path / "dup.fa").write_bytes(b">c1\nACGTACGTACGT\n>c2 x\nACGT\n>c1\nGGGG\n")
    with pytest.raises(capi.MirpError, match="duplicate contig name c1"):
        gpu_ctx.align_index([str(tmp_path / "dup.fa")])
    (tmp_path / "g.fa").write_bytes(b">c1\n" + b"ACGTTGCA" * 500 + b"\n")
    (tmp_path / "long.fa").write_bytes(b">S_r0_x1\nACGTACGTAC\n>S_r1_x2\n" + b"ACGT" * 200 + b"\n" + b"ACGT" * 57 + b"\n")
    gpu_ctx.align_index([str(tmp_path / "g.fa")])
    with pytest.raises(capi.MirpError, match="long.fa: read S_r1_x2 is longer than 1,024 nt"):
        gpu_ctx.align_reads(str(tmp_path / "long.fa"), str(tmp_path / "long.fa.sam"), "x")
    assert not (tmp_path / "long.fa.sam").exists()
    # through the command line: a message and status 255, no output
    r = _cli(["-r", str(tmp_path / "dup.fa"), str(tmp_path / "long.fa")], tmp_path)
    assert r.returncode == 255 and b"duplicate contig name c1" in r.stderr and not (tmp_path / "long.fa.sam").exists()
    r = _cli(["-r", str(tmp_path / "g.fa"), str(tmp_path / "long.fa")], tmp_path)
    assert r.returncode == 255 and b"longer than 1,024 nt" in r.stderr and not (tmp_path / "long.fa.sam").exists()
    # 1,024 nt itself is fine
    (tmp_path / "ok.fa").write_bytes(b">S_r0_x1\n" + b"ACGTTGCA" * 128 + b"\n")
    res = gpu_ctx.align_reads(str(tmp_path / "ok.fa"), str(tmp_path / "ok.fa.sam"), "x")
    assert res["aligned"] == 1 and res["records"] >= 1
