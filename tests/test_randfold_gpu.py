"""GPU tests of the shuffle test of precursor MFEs (mirp_randfold, mirp_shuffle_batch, randfold_kernels.hip): the device's shuffles
byte for byte against the restatement of tests/test_randfold_cpu.py; records and table against the restatement with CPU-oracle folds, both
methods and both fold models, on sequences either side of 300 nt; the natives' MFE against fold_batch_summary; forced pass capacities; 1,000
planted hairpins and 1,000 random sequences at 999 shuffles; refusals; the command line; and the chain cli pipeline -> precursor.fa -> randfold.
Oracle folds run in worker processes that are started fresh (spawn), never forked from a process that holds a device context."""
import ctypes as C
import multiprocessing
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.test_randfold_cpu import (HEADER, LONG_WALK, M64, PIN_SEQ, ROOT, codes, letters, oracle_mfe, planted_hairpin, random_seq, records_as_dicts,
                                     restate_records, restate_table, shuffled)

pytestmark = pytest.mark.gpu
MODELS = ("vienna-2.1.2", "vienna-1.8.5")


@pytest.fixture(scope="module")
def fold_many():
    with multiprocessing.get_context("spawn").Pool(12) as pool:
        yield lambda jobs: pool.map(oracle_mfe, jobs, chunksize=16)


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_fold_model(MODELS[0])
    yield gpu_ctx
    gpu_ctx.set_fold_model(MODELS[0])


def _cli(args, cwd, module="mir_prefer_amd.randfold", limit=900):
    """a child process of its own under its own time limit"""
    return subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", module] + args, cwd=str(cwd), capture_output=True,
                          env=dict(os.environ, PYTHONPATH=ROOT))


# ---------------------------------------------------------------------------------------------------- shuffle bytes
def _check_shuffles(ctx, seqs, k0, n_k, seed, capacity=0):
    for method in (0, 1):
        got = ctx.shuffle_batch(seqs, k0, n_k, dinucleotide=method, seed=seed, capacity=capacity)
        assert len(got) == len(seqs)
        for q, s in enumerate(seqs):
            assert got[q] == [shuffled(s, method, seed, q, k) for k in range(k0, k0 + n_k)], (method, seed, q, len(s))


def test_shuffle_pins_on_the_device(ctx):
    assert ctx.shuffle_batch([PIN_SEQ], 0, 2, dinucleotide=True, seed=0)[0] == [
        b"UGAUGCACUGGAGCGAAGCUGCACUCUCAUUCACAUAUCAACAAGAGAGUUUGCAGCACUUUGCUUGAGCUUCUCUGUUGUCAA",
        b"UUGUCACAGGCAAAUUGCUUUUCUCAGCAAUCUGCUUGAUAAGAUUUGAGCUGCGCUCUCACACUCUGAGUGCAGUGACACAGA"]
    assert ctx.shuffle_batch([PIN_SEQ], 0, 1, dinucleotide=False, seed=0)[0] == [
        b"CAUCUUCUUACACAGCUGAAGCGGGAUAUUUUCCUCUUGUUGUUUGGGACCCAAGAAUUCUCCGACGAAGUCCGAGAACUUGAA"]
    seqs = ["A"] * 7 + [PIN_SEQ]                          # q = 7
    assert ctx.shuffle_batch(seqs, 998, 1, dinucleotide=False, seed=12345)[7] == [
        b"CUAUCUCAGUACUCAGGCCAAGUGUUGUAUAGUAUGGGCAUAUUAUUCCCGACUGGCAUACGACUUCGCUCCAAUUUACAAGGG"]


def test_shuffle_bytes_match_the_restatement(ctx):
    rng = random.Random(21)
    grid = [random_seq(rng, n) for n in list(range(1, 41)) + list(range(43, 351, 7))]
    _check_shuffles(ctx, grid, 0, 5, 0)
    _check_shuffles(ctx, grid[::3], 3, 4, M64)
    _check_shuffles(ctx, grid[1::5], 99990, 10, 1 << 63)
    special = ["A", "AC", "ACG", "AAA", "U" * 50, "g" * 301, LONG_WALK, "AC" * 100 + "AG", "ACGUN" * 20, "N" * 30, "ANNNNNNNNNNNNNNNNNNNNC" * 3,
               "acgtTTxkiRY-" * 12, random_seq(rng, 120, "AAAAAAAC"), random_seq(rng, 200, "AC"), random_seq(rng, 333, "ACGUN")]
    for seed in (0, 1, 12345, M64):
        _check_shuffles(ctx, special, 0, 6, seed)
    _check_shuffles(ctx, special, 17, 3, 5)
    longs = [random_seq(rng, 1000), random_seq(rng, 2999, "ACGUN"), random_seq(rng, 3000), "A" * 1500 + "C" + "A" * 1400 + "G"]
    _check_shuffles(ctx, longs, 1, 2, 77)
    # passes: the same rows whatever the capacity
    _check_shuffles(ctx, special, 0, 6, 9, capacity=4)
    _check_shuffles(ctx, grid[:30], 2, 3, 9, capacity=1)


def test_the_sequence_with_the_long_walk_on_the_device(ctx):
    got = ctx.shuffle_batch([LONG_WALK], 0, 64, dinucleotide=True, seed=0)[0]
    assert got == [shuffled(LONG_WALK, 1, 0, 0, k) for k in range(64)]
    assert all(g[0:1] == b"A" and g[-1:] == b"G" and g.count(b"C") == 1 and len(g) == 202 for g in got)


# ---------------------------------------------------------------------------------------------------- records and table against the oracle
def _mixed_sequences():
    rng = random.Random(31)
    lens = [60, 75, 84, 99, 110, 128, 150, 163, 181, 200, 222, 240, 263, 280, 299, 300, 301, 305, 312, 320, 90, 140, 70, 310]
    seqs = [random_seq(rng, n) for n in lens]
    seqs[2] = planted_hairpin(rng)
    seqs[5] = random_seq(rng, 128, "ACGUN").lower().replace("u", "t")
    seqs[20] = "A" * 90                                   # gc = 0, every MFE 0
    seqs[17] = (planted_hairpin(rng) * 6)[:305]           # a long one that folds well
    assert len(seqs) == 24 and sum(len(s) > 300 for s in seqs) >= 5 and min(map(len, seqs)) >= 60 and max(map(len, seqs)) <= 320
    return seqs


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("method", [0, 1])
def test_records_and_table_match_the_oracle(fold_many, ctx, tmp_path, model, method):
    seqs = _mixed_sequences()
    want = restate_records(seqs, 100, method, 2024, model=model, fold_many=fold_many)
    ctx.set_fold_model(model)
    recs, res = ctx.randfold(seqs, 100, dinucleotide=method, seed=2024)
    assert records_as_dicts(recs) == want
    assert (res["sequences"], res["folds"], res["passes"]) == (24, 24 * 101, 2)          # one pass for the sequences up to 300 nt, one for the longer
    assert want[20]["gc"] == 0 and want[20]["le"] == 100 and want[2]["le"] == 0
    names = ["p%d" % q for q in range(24)]
    from mir_prefer_amd import randfold
    assert randfold.table(names, recs, 100) == restate_table(names, want, 100)
    if method == 1:
        # the command line: the same bytes in the file
        (tmp_path / "p.fa").write_text("".join(">%s some text\n%s\n%s\n" % (nm, s[:50], s[50:]) for nm, s in zip(names, seqs)))
        r = _cli(["-n", "100", "--seed", "2024", "--fold-model", model, str(tmp_path / "p.fa")], tmp_path)
        assert r.returncode == 0, r.stderr.decode()
        assert (tmp_path / "p.fa.randfold.tsv").read_text() == restate_table(names, want, 100)
        assert r.stderr.decode().startswith("randfold: 24 precursors, 2424 folds, 2 passes, ")


def test_native_mfe_is_the_batch_folds(ctx):
    seqs = _mixed_sequences()
    blob = b"".join(letters(codes(s)) for s in seqs)
    offs = np.cumsum([0] + [len(s) for s in seqs])
    for model in MODELS:
        ctx.set_fold_model(model)
        recs, _ = ctx.randfold(seqs, 3, seed=1)
        _, mfe, status = ctx.fold_batch_summary(blob, offs, 320)
        assert (status >= 0).all() and list(recs["mfe"]) == list(mfe), model          # (status 1, more lines than the capacity, leaves the MFE whole)
        short = [q for q, s in enumerate(seqs) if len(s) <= 300]
        _, mfe300, _ = ctx.fold_batch_summary(b"".join(letters(codes(seqs[q])) for q in short), np.cumsum([0] + [len(seqs[q]) for q in short]), 300)
        assert [int(recs["mfe"][q]) for q in short] == list(mfe300), model


def test_capacity_does_not_change_the_records(ctx):
    seqs = _mixed_sequences()[12:] + ["ACGUACGUAC", "G"]
    for method in (0, 1):
        ref, res = ctx.randfold(seqs, 20, dinucleotide=method, seed=5)
        assert res["passes"] == 2 and res["folds"] == len(seqs) * 21
        for cap in (1, 7, 20, 21, 50, 10 ** 6):
            got, r2 = ctx.randfold(seqs, 20, dinucleotide=method, seed=5, capacity=cap)
            assert got.tobytes() == ref.tobytes(), (method, cap)
            assert r2["passes"] >= res["passes"] and (cap > 50 or r2["passes"] > res["passes"])
    assert ctx.randfold(seqs, 20, dinucleotide=1, seed=6)[0].tobytes() != ref.tobytes()


# ---------------------------------------------------------------------------------------------------- scale and sense
def test_hairpins_stand_out_and_random_sequences_do_not(ctx):
    rng = random.Random(2026)
    hairpins = [planted_hairpin(rng) for _ in range(1000)]
    randoms = [random_seq(rng, rng.randint(70, 100)) for _ in range(1000)]
    recs, res = ctx.randfold(hairpins + randoms, 999, dinucleotide=True, seed=3)
    print("scale:", {k: v for k, v in res.items() if k != "seconds"}, ["%.3f" % s for s in res["seconds"]])
    assert res["folds"] == 2000 * 1000
    clear = int((recs["le"][:1000] == 0).sum())
    low_p = float((((recs["le"][1000:] + 1) / 1000.0) <= 0.05).mean())
    print("hairpins with le = 0: %d of 1000; random sequences with p <= 0.05: %.3f" % (clear, low_p))
    assert clear >= 900
    assert 0.01 <= low_p <= 0.15
    again, _ = ctx.randfold(hairpins + randoms, 999, dinucleotide=True, seed=3)
    assert again.tobytes() == recs.tobytes()
    assert (recs["min_mfe"] <= recs["sum"] // 999).all() and (recs["sum_sq"] >= 0).all()


# ---------------------------------------------------------------------------------------------------- refusals
def _raw_randfold(ctx, blob, offs, n_shuffles):
    from mir_prefer_amd import capi
    o = capi.RandfoldOpts()
    o.seed, o.n_shuffles, o.dinucleotide, o.capacity = 0, n_shuffles, 1, 0
    ptr = C.c_void_p()
    rc = ctx.lib.mirp_randfold(ctx.h, blob.ctypes.data_as(C.c_char_p), offs.ctypes.data_as(C.POINTER(C.c_int64)), len(offs) - 1, C.byref(o), C.byref(ptr), None, None)
    return rc, ctx.lib.mirp_last_error(ctx.h).decode()


def test_refusals(ctx, tmp_path):
    from mir_prefer_amd import capi
    good = "UGACAGAAGAGAGUGAGCAC"
    cases = [([good, "", good], "record 2: an empty sequence"), ([good, good, "A" * 3001], "record 3: a sequence longer than 3,000 nt"),
             ([good.encode() + "é".encode()], "record 1: a byte >= 0x80"), ([good, b"ACG\xffU"], "record 2: a byte >= 0x80")]
    for seqs, msg in cases:
        for call in (lambda: ctx.randfold(seqs, 5), lambda: ctx.shuffle_batch(seqs, 0, 2)):
            with pytest.raises(capi.MirpError) as e:
                call()
            assert "(-10)" in str(e.value) and msg in str(e.value), (msg, str(e.value))
    assert ctx.shuffle_batch(["AC" * 1500], 4, 1)[0] == [shuffled("AC" * 1500, 1, 0, 0, 4)]          # the limit itself is served
    for bad in (dict(n_shuffles=0), dict(n_shuffles=100001), dict(n_shuffles=5, capacity=-1)):
        with pytest.raises(capi.MirpError):
            ctx.randfold([good], **bad)
    for k0, n_k in ((-1, 1), (0, 0), (99999, 2)):
        with pytest.raises(capi.MirpError):
            ctx.shuffle_batch([good], k0, n_k)
    # more than 2^40 folds: refused from the counts alone
    n = (1 << 40) // 100001 + 1
    rc, err = _raw_randfold(ctx, np.full(n, ord("A"), dtype=np.uint8), np.arange(n + 1, dtype=np.int64), 100000)
    assert rc == -10 and "more than 2^40 folds" in err, (rc, err)
    # the command line: every refusal leaves no file, not even an old one
    for data, msg in ((">a\n%s\n>b\n>c\n%s\n" % (good, good), "record 2: an empty sequence"), (">a\n%s\n" % ("ACGU" * 751), "record 1: a sequence longer than 3,000 nt"),
                      (">a\n%s\n>b\nAC\xe9GU\n" % good, "record 2: a byte >= 0x80"), (">a\n%s\n>\n%s\n" % (good, good), "record 2: a header without a name")):
        (tmp_path / "p.fa").write_bytes(data.encode("latin-1"))
        (tmp_path / "p.fa.randfold.tsv").write_text("stale\n")
        r = _cli(["-n", "3", str(tmp_path / "p.fa")], tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and msg in r.stderr.decode(), (msg, r.stderr.decode())
        assert not (tmp_path / "p.fa.randfold.tsv").exists()
    # a device that does not exist, with an input that is fine
    (tmp_path / "p.fa").write_text(">a\n%s\n" % good)
    (tmp_path / "p.fa.randfold.tsv").write_text("stale\n")
    r = _cli(["--device", "4096", str(tmp_path / "p.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and "there is no CPU path" in r.stderr.decode(), r.stderr.decode()
    assert not (tmp_path / "p.fa.randfold.tsv").exists()


def test_degenerate_inputs_are_not_refusals(ctx):
    recs, res = ctx.randfold([], 9)
    assert len(recs) == 0 and (res["sequences"], res["folds"], res["passes"]) == (0, 0, 0)
    assert ctx.shuffle_batch([], 0, 3) == []
    recs, res = ctx.randfold(["A", "ac", "NNNNNNNNNN"], 1, dinucleotide=True)
    assert [(int(r["len"]), int(r["gc"]), int(r["mfe"]), int(r["le"]), int(r["min_mfe"]), int(r["sum"]), int(r["sum_sq"])) for r in recs] == [
        (1, 0, 0, 1, 0, 0, 0), (2, 1, 0, 1, 0, 0, 0), (10, 0, 0, 1, 0, 0, 0)]


# ---------------------------------------------------------------------------------------------------- chain
def test_chain_pipeline_precursors_to_randfold(fold_many, tmp_path):
    """cli pipeline on the golden `mini` dataset, then randfold of its precursor.fa: the table against the restatement with oracle folds."""
    from mir_prefer_amd import randfold
    from tests.test_cli_gpu import _setup
    exp, cfg, out = _setup("mini", tmp_path)
    r = _cli(["pipeline", cfg], tmp_path, module="mir_prefer_amd.cli")
    assert r.returncode == 0, r.stderr.decode()
    pre = out / (exp["config"]["NAME_PREFIX"] + "_miRNA.precursor.fa")
    records = randfold.parse_fasta(pre.read_bytes())
    assert len(records) >= 40 and all(s for _, s in records)
    r = _cli(["-n", "20", "-m", "di", "--seed", "8", str(pre)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_records([s for _, s in records], 20, 1, 8, fold_many=fold_many)
    text = open(str(pre) + ".randfold.tsv").read()
    assert text == restate_table([n.decode() for n, _ in records], want, 20)
    assert text.startswith(HEADER) and text.count("\n") == len(records) + 1
