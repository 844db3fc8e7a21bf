"""Host tests of the read alignment command (mir_prefer_amd.align): the argument errors of bowtie-align-reads.py, each with its message and exit status
and without opening a device, and self-checks of the tests' CPU restatement of the alignment semantics: a brute-force numpy aligner
and, for -v 0 at larger scale, a packed-L-mer searchsorted aligner.  The GPU tests (test_align_gpu.py) compare the device output with both."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG = b"@PG\tID:mir_prefer_amd.align\tCL:\"-\"\n"

# ---------------------------------------------------------------------------------------------------- restatement
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    CODE[_ch] = CODE[_ch + 32] = _i
LETTER = np.frombuffer(b"ACGTN", dtype=np.uint8)
_WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"


def _lines(data):
    return data.replace(b"\r\n", b"\n").replace(b"\r", b"\n").split(b"\n")


def parse_fasta(data):
    """-> [(name, sequence bytes)]: name = first word of the header, sequence lines stripped and concatenated, text before the first header ignored."""
    out = []
    for line in _lines(data):
        if line.startswith(b">"):
            out.append([line[1:].split()[0].decode(), []])
        elif out:
            out[-1][1].append(line.strip(_WS))
    return [(n, b"".join(s)) for n, s in out]


def load_reference(paths):
    """-> (names, [uint8 code arrays]) in reference order, contigs of length 0 dropped."""
    names, seqs = [], []
    for p in paths:
        for n, s in parse_fasta(open(p, "rb").read()):
            if s:
                names.append(n)
                seqs.append(CODE[np.frombuffer(s, dtype=np.uint8)])
    return names, seqs


def load_reads(path):
    return [(n, CODE[np.frombuffer(s, dtype=np.uint8)]) for n, s in parse_fasta(open(path, "rb").read())]


def revcomp(codes):
    r = codes[::-1].copy()
    acgt = r < 4
    r[acgt] = 3 - r[acgt]
    return r


def brute_hits(seqs, reads, vmax=3):
    """Every hit with at most vmax mismatches: per read a list of (tid, offset, strand, mm).  No window holds an ambiguous reference base; a read
    base outside ACGT mismatches everything."""
    amb_cs = [np.concatenate([[0], np.cumsum(s == 4)]) for s in seqs]
    out = []
    for _, r in reads:
        L = len(r)
        hits = []
        if L > 0:
            for strand, o in ((0, r), (1, revcomp(r))):
                for t, s in enumerate(seqs):
                    n = len(s)
                    if L > n:
                        continue
                    w = n - L + 1
                    mm = np.zeros(w, dtype=np.int32)
                    for i in range(L):
                        mm += s[i:i + w] != o[i]
                    ok = (mm <= vmax) & (amb_cs[t][L:] - amb_cs[t][:w] == 0)
                    hits += [(t, int(x), strand, int(mm[x])) for x in np.nonzero(ok)[0]]
        out.append(hits)
    return out


def _pack(arr_rows):
    v = np.zeros(arr_rows[0].shape, dtype=np.uint64)
    for a in arr_rows:
        v = v * np.uint64(4) + a.astype(np.uint64)
    return v


def searchsorted_hits_v0(seqs, reads):
    """Exact hits (-v 0) by sorted packed L-mers of the genome, one table per read length (L <= 32): per read a list of (tid, offset, strand, 0)."""
    out = [[] for _ in reads]
    by_len = {}
    for k, (_, r) in enumerate(reads):
        if 0 < len(r) <= 32 and (r < 4).all():
            by_len.setdefault(len(r), []).append(k)
    for L, ks in by_len.items():
        vals, tids, offs = [], [], []
        for t, s in enumerate(seqs):
            w = len(s) - L + 1
            if w <= 0:
                continue
            cs = np.concatenate([[0], np.cumsum(s == 4)])
            ok = cs[L:] - cs[:w] == 0
            v = _pack([s[i:i + w] for i in range(L)])
            idx = np.nonzero(ok)[0]
            vals.append(v[idx]); tids.append(np.full(len(idx), t, dtype=np.int64)); offs.append(idx)
        if not vals:
            continue
        vals, tids, offs = np.concatenate(vals), np.concatenate(tids), np.concatenate(offs)
        order = np.argsort(vals, kind="stable")
        vals, tids, offs = vals[order], tids[order], offs[order]
        for strand in (0, 1):
            q = np.stack([reads[k][1] if strand == 0 else revcomp(reads[k][1]) for k in ks])
            qv = _pack([q[:, i] for i in range(L)])
            lo, hi = np.searchsorted(vals, qv, "left"), np.searchsorted(vals, qv, "right")
            for k, a, b in zip(ks, lo, hi):
                out[k] += [(int(tids[j]), int(offs[j]), strand, 0) for j in range(a, b)]
    return out


def _md(o, g):
    md, run = [], 0
    for a, b in zip(o, g):
        if a == b:
            run += 1
        else:
            md.append("%d%s" % (run, "ACGT"[b]))
            run = 0
    return "".join(md) + str(run)


def sam_bytes(names, seqs, reads, hits, v, k, m=0, f=False, pg=PG):
    """The SAM text of DESIGN.md §12 from the hits of every read (any superset of the hits with <= v mismatches)."""
    out = [b"@HD\tVN:1.0\tSO:unsorted\n"] + [b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), len(s)) for n, s in zip(names, seqs)] + [pg]
    for (q, r), hs in zip(reads, hits):
        L = len(r)
        hs = [h for h in hs if h[3] <= v] if L > v else []
        best = min((h[3] for h in hs), default=None)
        sel = sorted((h for h in hs if h[3] == best), key=lambda h: (h[0], h[1], h[2]))
        xm = 0
        if m and len(sel) > m:
            sel, xm = [], m + 1
        if not sel:
            if not f:
                seq = LETTER[r].tobytes().decode() if L else "*"
                out.append(("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXM:i:%d\n" % (q, seq, "I" * L if L else "*", xm)).encode())
            continue
        for t, off, strand, mm in sel[:k]:
            o = r if strand == 0 else revcomp(r)
            g = seqs[t][off:off + L]
            out.append(("%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s\tXA:i:%d\tMD:Z:%s\tNM:i:%d\n"
                        % (q, 16 * strand, names[t], off + 1, L, LETTER[o].tobytes().decode(), "I" * L, mm, _md(o, g), mm)).encode())
    return b"".join(out)


def normalise_pg(data):
    return b"".join(PG if ln.startswith(b"@PG\t") else ln for ln in data.splitlines(keepends=True))


# ---------------------------------------------------------------------------------------------------- restatement self-checks
def test_brute_force_finds_planted_reads_and_respects_its_rules():
    rng = np.random.RandomState(1)
    g = CODE[np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, 3000)]]
    g[1000:1010] = 4
    r0 = g[200:220].copy()
    r1 = revcomp(g[500:522])
    r1[3] = (r1[3] + 1) % 4
    r2 = g[995:1015].copy()          # overlaps the N run: never a hit
    r3 = g[2980:3000].copy()         # the contig's end
    r4 = r0.copy()
    r4[5] = 4                        # a read N mismatches every base
    hits = brute_hits([g], [("a", r0), ("b", r1), ("c", r2), ("d", r3), ("e", r4)], vmax=1)
    assert (0, 200, 0, 0) in hits[0]
    assert (0, 500, 1, 1) in hits[1]
    assert not any(h[1] + 20 > 1000 and h[1] < 1010 for h in hits[2])
    assert (0, 2980, 0, 0) in hits[3]
    assert (0, 200, 0, 1) in hits[4] and not any(h[3] == 0 for h in hits[4])


def test_searchsorted_restatement_equals_brute_force_at_v0():
    rng = np.random.RandomState(2)
    seqs = [rng.randint(0, 4, n).astype(np.uint8) for n in (4000, 2500)]
    seqs[0][100:140] = np.tile(seqs[0][100:104], 10)        # tandem repeat
    seqs[1][50:60] = 4
    reads = []
    for k in range(300):
        L = int(rng.randint(4, 26))
        t = int(rng.randint(0, 2))
        o = int(rng.randint(0, len(seqs[t]) - L))
        r = seqs[t][o:o + L].copy()
        if k % 3 == 0:
            r = revcomp(r)
        if k % 7 == 0:
            r = rng.randint(0, 4, L).astype(np.uint8)
        reads.append(("q%d" % k, r))
    brute = [[h for h in hs if h[3] == 0] for hs in brute_hits(seqs, reads, vmax=0)]
    ss = searchsorted_hits_v0(seqs, reads)
    assert [sorted(a) for a in brute] == [sorted(b) for b in ss]
    assert sum(len(h) for h in ss) > 300


def test_sam_text_of_the_restatement():
    g = CODE[np.frombuffer(b"ACGTACGTTTGCA", dtype=np.uint8)]
    r = CODE[np.frombuffer(b"CGTACcTT", dtype=np.uint8)]
    reads = [("s_r0_x3", r), ("s_r1_x1", CODE[np.frombuffer(b"A", dtype=np.uint8)])]
    hits = brute_hits([g], reads, vmax=1)
    got = sam_bytes(["chr1"], [g], reads, hits, v=1, k=5).decode().splitlines()
    assert got[:2] == ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:chr1\tLN:13"]
    assert got[3] == "s_r0_x3\t0\tchr1\t2\t255\t8M\t*\t0\t0\tCGTACCTT\tIIIIIIII\tXA:i:1\tMD:Z:5G2\tNM:i:1"
    assert got[4] == "s_r1_x1\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\tXM:i:0"      # L <= v: unaligned
    assert sam_bytes(["chr1"], [g], reads, hits, v=1, k=5, f=True).decode().splitlines()[3:] == got[3:4]
    assert sam_bytes(["chr1"], [g], reads, hits, v=0, k=5, m=1).decode().splitlines()[3] == "s_r0_x3\t4\t*\t0\t0\t*\t*\t0\t0\tCGTACCTT\tIIIIIIII\tXM:i:0"


# ---------------------------------------------------------------------------------------------------- argument errors
@pytest.fixture
def no_device(monkeypatch):
    from mir_prefer_amd import capi

    def refuse(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(capi, "Context", refuse)


@pytest.fixture
def files(tmp_path):
    (tmp_path / "g.fa").write_text(">chr1\nACGTACGTAC\n")
    (tmp_path / "s.fa").write_text(">s_r0_x3\nACGTA\n")
    return tmp_path


def _main(argv, capsys):
    from mir_prefer_amd import align
    try:
        rc = align.main(argv)
    except SystemExit as e:
        rc = e.code
    return rc, capsys.readouterr().err


@pytest.mark.parametrize("argv,msg", [
    ([], "incorrect number of arguments"),
    (["-r", "{d}/g.fa", "-i", "{d}/idx", "{d}/s.fa"], "Options -r and -i are mutually exclusive"),
    (["{d}/s.fa"], "Either option -r or -i should be provided."),
    (["-r", "{d}/missing.fa", "{d}/s.fa"], "File {d}/missing.fa in option -r does not exist!!"),
    (["-r", "{d}/g.fa", "{d}/missing.fa"], "File {d}/missing.fa does not exist!!"),
    (["-i", "{d}/idx", "{d}/s.fa"], "Index file {d}/idx.1.ebwt does not exist!! Please use the -r option instead."),
    (["-i", "{d}/idx", "-t", "{d}/tmp", "{d}/s.fa"], "Option -t is not needed for option '-r'"),
    (["-v", "4", "-r", "{d}/g.fa", "{d}/s.fa"], "Option -v must be between 0 and 3."),
    (["-k", "0", "-r", "{d}/g.fa", "{d}/s.fa"], "Option -k must be at least 1."),
    (["-m", "0", "-r", "{d}/g.fa", "{d}/s.fa"], "Option -m must be at least 1."),
])
def test_option_errors(files, no_device, capsys, argv, msg):
    rc, err = _main([a.format(d=files) for a in argv], capsys)
    assert rc == 2
    assert "mir_prefer_amd.align: error: " + msg.format(d=files) in err
    assert not (files / "s.fa.sam").exists()


def test_index_option_is_refused_after_the_scripts_checks(files, no_device, capsys):
    for s in ["1.ebwt", "2.ebwt", "3.ebwt", "4.ebwt", "rev.1.ebwt", "rev.2.ebwt"]:
        (files / ("idx." + s)).write_text("")
    rc, err = _main(["-i", str(files / "idx"), str(files / "s.fa")], capsys)
    assert rc == 255
    assert "option -i cannot be used" in err and "with -r" in err
    assert not (files / "s.fa.sam").exists()


def test_read_ids_are_checked(files, no_device, capsys):
    (files / "bad.fa").write_text(">s_r0_x3\nACGT\n>plain_read\nACGT\n")
    rc, err = _main(["-r", str(files / "g.fa"), str(files / "s.fa"), str(files / "bad.fa")], capsys)
    assert rc == 255
    assert "ERROR: The format of the read IDs in file %s is not right." % (files / "bad.fa") in err
    assert "ERROR: The format of the read IDs in file %s is not right." % (files / "s.fa") not in err
    assert "SampleName_rA_xN" in err
    assert not (files / "s.fa.sam").exists() and not (files / "bad.fa.sam").exists()


def test_read_id_check_stops_before_the_2000th_header(files):
    from mir_prefer_amd import align
    p = files / "many.fa"
    p.write_text("".join(">s_r%d_x1\nACGT\n" % k for k in range(1999)) + ">not_an_id\nACGT\n")
    assert align.check_readid(str(p))
    p.write_text("".join(">s_r%d_x1\nACGT\n" % k for k in range(1998)) + ">not_an_id\nACGT\n")
    assert not align.check_readid(str(p))


def test_help_names_the_options(capsys):
    from mir_prefer_amd import align
    text = align.make_parser().format_help()
    for opt in ("-r", "-i", "-t", "-v", "-k", "-m", "-p", "-f", "--device"):
        assert opt in text
