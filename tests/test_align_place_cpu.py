"""Host tests of the placement of multi-mapped reads (`align --place`, DESIGN.md §12 "Placement"): the known answers of the draw, the worked example
of the definition to the byte and the depth rule, all on the tests' restatement (tests/place_restatement.py); the option errors, each with exit
status 2 and without opening a device; --help; and the three new entries of the C header."""
import os
import re

import numpy as np
import pytest

from tests.place_restatement import depth_of, draw, hits_of, place
from tests.test_align_cpu import CODE, LETTER, ROOT, revcomp


def test_known_answers_of_the_draw():
    assert draw(b"", 0) == 0xf52a15e9a9b5e89b
    assert draw(bytes([0, 1, 2, 3]), 0) == 0xc0bd9d7f5fa9fca0
    assert draw(bytes([0, 1, 2, 3]), 1) == 0x830d248c7fc6bf9b
    assert draw(bytes([4] * 21), 0) == 0xd0ca14f88741e669
    assert draw(CODE[np.frombuffer(b"acgt", dtype=np.uint8)], 0) == draw(bytes([0, 1, 2, 3]), 0)       # either case, as numpy codes


def test_depth_rule():
    assert depth_of("a_r1_x7") == 7
    assert depth_of("a_r1_x") == 1
    assert depth_of("a_x3_r1") == 1
    assert depth_of("x_r1_x4294967296") == 1
    assert depth_of("x_r1_x4294967295") == 4294967295
    assert depth_of("a_x3_x0012") == 12 and depth_of("_x5") == 5 and depth_of("x5") == 1 and depth_of("a_x0") == 0


def test_worked_example_to_the_byte():
    rng = np.random.RandomState(12)
    c1 = rng.randint(0, 4, 100).astype(np.uint8)
    c2 = rng.randint(0, 4, 60).astype(np.uint8)
    c2[0:20] = c1[30:50]                                     # the 20-nt read: c1 POS 31 and c2 POS 1
    names, seqs = ["c1", "c2"], [c1, c2]
    reads = [("s_r0_x5", c1[9:27].copy()), ("s_r1_x2", revcomp(c1[39:59])), ("s_r2_x7", c1[94:100].copy()), ("s_r3_x1", c1[30:50].copy())]
    hits = hits_of(seqs, reads, 0)
    assert [sorted(h) for h in hits] == [[(0, 9, 0, 0)], [(0, 39, 1, 0)], [(0, 94, 0, 0)], [(0, 30, 0, 0), (1, 0, 0, 0)]]
    got, info = place(names, seqs, reads, hits, 0, 50, 10, 0, "u")
    assert info[3]["w"] == [2, 0] and info[3]["wt"] == 2 and info[3]["idx"] == 0 and info[3]["cls"] == "U"

    def letters(x):
        return LETTER[x].tobytes().decode()

    def rec(q, flag, contig, pos, seq, tags):
        return "%s\t%d\t%s\t%d\t255\t%dM\t*\t0\t0\t%s\t%s\tXA:i:0\tMD:Z:%d\tNM:i:0\t%s\n" % (q, flag, contig, pos, len(seq), seq, "I" * len(seq), len(seq), tags)
    want = ("@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:c1\tLN:100\n@SQ\tSN:c2\tLN:60\n@PG\tID:mir_prefer_amd.align\tCL:\"-\"\n"
            + rec("s_r0_x5", 0, "c1", 10, letters(c1[9:27]), "NH:i:1\tXY:Z:N\tXW:Z:0/0")
            + rec("s_r1_x2", 16, "c1", 40, letters(c1[39:59]), "NH:i:1\tXY:Z:N\tXW:Z:0/0")
            + rec("s_r2_x7", 0, "c1", 95, letters(c1[94:100]), "NH:i:1\tXY:Z:N\tXW:Z:0/0")
            + rec("s_r3_x1", 0, "c1", 31, letters(c1[30:50]), "NH:i:2\tXY:Z:U\tXW:Z:2/2"))
    assert got == want.encode()
    for seed in range(8):                                    # either value of r
        assert place(names, seqs, reads, hits, 0, 50, 10, seed, "u")[0] == got
    # mode r: no weights; -m 1 suppresses the read; W = 60 reaches POS 95 from c1 POS 31, and from c2 POS 1 only across the join: still 0
    r_lines = place(names, seqs, reads, hits, 0, 50, 10, 0, "r")[0].decode().splitlines()
    assert r_lines[-1].endswith("\tNH:i:2\tXY:Z:R\tXW:Z:0/0") and r_lines[-2].endswith("\tNH:i:1\tXY:Z:N\tXW:Z:0/0")
    assert place(names, seqs, reads, hits, 0, 1, 10, 0, "u")[0].decode().splitlines()[-1].endswith("\tXM:i:2")
    assert place(names, seqs, reads, hits, 0, 50, 60, 0, "u")[1][3]["w"] == [14, 0]


# ---------------------------------------------------------------------------------------------------- the command line
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


@pytest.mark.parametrize("argv,msg", [
    (["--place", "x"], "option --place: invalid choice: 'x'"),
    (["--place", "u", "-m", "0"], "Option -m must be at least 1."),
    (["--place", "u", "-m", "10001"], "Option -m must be between 1 and 10000 with --place."),
    (["--place", "r", "-m", "-3"], "Option -m must be at least 1."),
    (["--window", "50"], "Option --window needs --place."),
    (["--seed", "1"], "Option --seed needs --place."),
    (["--place", "u", "--window", "-1"], "Option --window must be between 0 and 10000."),
    (["--place", "u", "--window", "10001"], "Option --window must be between 0 and 10000."),
    (["--place", "r", "--seed", "-1"], "Option --seed must be between 0 and 2^64-1."),
    (["--place", "u", "--seed", str(2 ** 64)], "Option --seed must be between 0 and 2^64-1."),
    (["--place", "u", "--seed", "abc"], "option --seed: invalid integer value: 'abc'"),
])
def test_option_errors(files, no_device, capsys, argv, msg):
    from mir_prefer_amd import align
    with pytest.raises(SystemExit) as e:
        align.main(argv + ["-r", str(files / "g.fa"), str(files / "s.fa")])
    assert e.value.code == 2
    assert "mir_prefer_amd.align: error: " + msg in capsys.readouterr().err
    assert not (files / "s.fa.sam").exists()


def test_accepted_options_and_their_defaults(files):
    from mir_prefer_amd import align
    tail = ["-r", str(files / "g.fa"), str(files / "s.fa")]
    o, _ = align.parse_args(["--place", "u"] + tail)
    assert (o.place, o.window, o.seed, o.maxmultialignment) == ("u", 50, 0, 50)
    o, _ = align.parse_args(["--place", "r", "--window", "0", "--seed", str(2 ** 64 - 1), "-m", "10000"] + tail)
    assert (o.place, o.window, o.seed, o.maxmultialignment) == ("r", 0, 2 ** 64 - 1, 10000)
    o, _ = align.parse_args(tail)
    assert (o.place, o.window, o.seed, o.maxmultialignment) == (None, None, None, None)


def test_help_names_the_options():
    from mir_prefer_amd import align
    text = align.make_parser().format_help()
    for opt in ("--place", "--window", "--seed"):
        assert opt in text


def test_header_declares_the_entries_and_keeps_the_abi_number():
    from mir_prefer_amd import capi
    h = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    api = open(os.path.join(ROOT, "mir-prefer_amd", "csrc", "mirp_api.cpp")).read()
    assert re.search(r"#define MIRP_ABI_VERSION 17\b", api) and capi.ABI_VERSION == 17           # entries are only added
    assert re.search(r"typedef struct \{\s*int32_t mode;[^}]*int32_t window;[^}]*uint64_t seed;[^}]*\} MirpAlignPlaceOpts;", h)
    assert re.search(r"\bint mirp_align_reads_placed\(mirp_ctx\* ctx, const char\* reads_path, const char\* out_path, const char\* pg_cl, int32_t v, int32_t k, "
                     r"int32_t m,\s*int32_t filter_unmapped, const MirpAlignPlaceOpts\* place, int64_t stats\[8\], double seconds\[8\]\);", h)
    assert re.search(r"\bint mirp_set_align_place_capacity\(mirp_ctx\* ctx, int64_t items\);", h)
    assert re.search(r"\bint64_t mirp_align_place_last_realigned\(const mirp_ctx\* ctx\);", h)
    assert [f[0] for f in capi.AlignPlaceOpts._fields_] == ["mode", "window", "seed"]
