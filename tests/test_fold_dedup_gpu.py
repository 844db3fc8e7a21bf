"""GPU tests of the fold dedup (set_fold_dedup, the default): fold() folds each distinct window sequence once and copies the result to the windows
that repeat it.  Every case of tests/fold_dedup_cases.py goes load_genome / load_alignments -> candidate -> fold -> predict_raw and is compared
three ways: dedup on against dedup off (every output array, the three hand-off counters), dedup off against the CPU oracle (every structure line,
every MFE, the loci list), and the map of duplicates against its restatement (the first index of each distinct byte string).  Both fold models;
everything again with the hash cut to 4 bits, where different windows collide everywhere: a collision may leave a duplicate unmerged, so the map
is then the restatement's or -1 per window, and the outputs stay what they were."""
import numpy as np
import pytest

from mir_prefer_amd import capi, records
from tests import fold_dedup_cases as fc
from tests.test_oracle_golden import mirna_record, run_predict

pytestmark = pytest.mark.gpu

MODELS = ["vienna-2.1.2", "vienna-1.8.5"]


def _run(ctx, case, dedup, bits=0, model="vienna-2.1.2", overlap=-1, tailfree=-1, capacity=0, folds=1):
    """one pass of the pipeline over the case with the switches as given; every switch is put back"""
    try:
        ctx.set_fold_model(model)
        ctx.set_fold_dedup(dedup)
        ctx.set_fold_dedup_hash_bits(bits)
        ctx.set_fold_overlap(overlap)
        ctx.set_fold_overlap_tailfree(tailfree)
        ctx.set_fold_capacity(capacity)
        ctx.load_genome(case["contigs"])
        ctx.load_alignments(case["alns"])
        _, _, nwin = ctx.candidate(case["cut"], case["gap"], case["L"], case["order"])
        maps = []
        for _ in range(folds):
            ctx.fold(case["span"], case["max_lines"])
            maps.append(ctx.get_fold_duplicates())
        return {"nwin": nwin, "fold": ctx.get_fold(), "pred": ctx.predict_raw(1, 18, 23, False, True), "win": ctx.get_windows(),
                "counters": (ctx.last_fold_fallbacks(), ctx.last_fold_dense(), ctx.last_fold_overflow()), "chunks": ctx.last_fold_overlap_chunks(),
                "duplicates": ctx.last_fold_duplicates(), "map": maps[-1], "maps": maps}
    finally:
        ctx.set_fold_capacity(0)
        ctx.set_fold_overlap_tailfree(-1)
        ctx.set_fold_overlap(-1)
        ctx.set_fold_dedup_hash_bits(0)
        ctx.set_fold_dedup(True)
        ctx.set_fold_model("vienna-2.1.2")


def _window_lines(raw, k):
    wl, wss = capi.fold_window_lines(raw, k)
    return [(wss[j, :wl[j]["len"]].tobytes().decode(), int(wl[j]["energy"]), int(wl[j]["start"])) for j in range(raw["n_lines"][k]) if wl[j]["printed"]]


def _same_outputs(a, b):
    """every output of the fold and the filter, and the counters"""
    assert a["nwin"] == b["nwin"]
    fa, fb = a["fold"], b["fold"]
    for f in ("n_lines", "mfe", "status"):
        assert np.array_equal(fa[f], fb[f]), f
    assert sorted(fa["overflow"]) == sorted(fb["overflow"])
    for k in range(a["nwin"]):
        la, sa = capi.fold_window_lines(fa, k)
        lb, sb = capi.fold_window_lines(fb, k)
        nl = int(fa["n_lines"][k]) if k in fa["overflow"] else min(int(fa["n_lines"][k]), fa["max_lines"])
        assert la[:nl].tobytes() == lb[:nl].tobytes(), k
        for j in range(nl):
            ln = int(la[j]["len"])
            assert sa[j, :ln].tobytes() == sb[j, :ln].tobytes(), (k, j)
    for f in ("result", "text", "n_passed", "status"):
        assert a["pred"][f].shape == b["pred"][f].shape and a["pred"][f].tobytes() == b["pred"][f].tobytes(), f
    assert a["counters"] == b["counters"]


def _device_seqs(run):
    W = run["win"]["windows"]
    return [run["win"]["seq"][W[k]["seq_off"]:W[k]["seq_off"] + W[k]["seq_len"]].tobytes() for k in range(run["nwin"])]


def _check_map(run, bits):
    """the map against the restatement over the windows the fold read; full hash: equal, cut hash: equal or unmerged"""
    want = fc.first_index_map(_device_seqs(run))
    got = run["map"]
    assert got.dtype == np.int32 and got.shape == want.shape
    if bits == 0:
        assert np.array_equal(got, want), (got.tolist(), want.tolist())
        assert run["duplicates"] == int((want >= 0).sum())
    else:
        assert ((got == want) | (got == -1)).all(), (got.tolist(), want.tolist())
        assert run["duplicates"] == int((got >= 0).sum())
    return want


_FOLDS = {}      # (bytes, span, model) -> the oracle's fold, shared by every case and test of the module


def _oracle_fold(oracle, seq, span, model):
    key = (seq, span, model)
    if key not in _FOLDS:
        _FOLDS[key] = oracle.lfold(seq, span, model=model)
    return _FOLDS[key]


@pytest.fixture(scope="module")
def baseline(gpu_ctx, oracle):
    """(case name, model) -> (case, the run with dedup off), checked against the CPU oracle once: windows, structure lines, MFEs, loci"""
    done = {}

    def get(name, model):
        if (name, model) in done:
            return done[(name, model)]
        case = fc.CASES[name]()
        off = _run(gpu_ctx, case, False, model=model)
        assert off["duplicates"] == 0 and (off["map"] == -1).all() and len(off["map"]) == off["nwin"]
        win = fc.oracle_windows(oracle, case)
        seqs = fc.window_seqs(win)
        assert off["nwin"] == len(seqs) and _device_seqs(off) == seqs
        assert (off["fold"]["status"] == 0).all()
        structs = []
        for k, s in enumerate(seqs):
            ref = _oracle_fold(oracle, s, case["span"], model)
            assert _window_lines(off["fold"], k) == ref["lines"] and int(off["fold"]["mfe"][k]) == ref["mfe"], (name, model, k)
            structs.append(oracle.structures_from_lines(ref["lines"], 55))
        ocase = {"cfg": {"MIN_MATURE_LEN": 18, "MAX_MATURE_LEN": 23, "ALLOW_3NT_OVERHANG": "N", "ALLOW_NO_STAR_EXPRESSION": "Y"}, "win": win,
                 "sample_names": ["s0"], "alns": case["alns"]}
        _, result = run_predict(ocase, oracle, structs)
        pred = off["pred"]
        got = [[case["names"][m["tid"]], int(m["fold_s"]), int(m["fold_e"]), int(m["mat_s"]), int(m["mat_e"]), int(m["star_s"]), int(m["star_e"]),
                pred["text"][i, :int(m["ss_len"])].tobytes().decode(), records.STRAND[m["strand"]], bool(m["has_star"])] for i, m in enumerate(pred["result"])]
        assert got == [mirna_record(m, case["names"]) for _, m in result], (name, model)
        done[(name, model)] = (case, off)
        return done[(name, model)]
    return get


@pytest.mark.parametrize("bits", [0, 4])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", list(fc.CASES))
def test_dedup_on_equals_off_and_the_oracle(gpu_ctx, baseline, name, model, bits):
    case, off = baseline(name, model)
    at_least, want_map = fc.EXPECT[name]
    print("%s %s: %d windows, fallbacks / dense / overflow %s with dedup off" % (name, model, off["nwin"], off["counters"]))
    if model == MODELS[0]:
        assert all(c >= m for c, m in zip(off["counters"], at_least)), off["counters"]
    on = _run(gpu_ctx, case, True, bits=bits, model=model)
    want = _check_map(on, bits)
    assert want.tolist() == want_map
    _same_outputs(on, off)


SCHEDULES = {"chunks-of-1-tailfree": dict(overlap=1, tailfree=1), "chunks-of-1-ordered": dict(overlap=1, tailfree=0),
             "chunks-of-2-tailfree": dict(overlap=2, tailfree=1), "ring-slots-of-1-tailfree": dict(overlap=3, tailfree=1, capacity=3),
             "ring-slots-of-1-ordered": dict(overlap=3, tailfree=0, capacity=3), "sub-batches-of-1": dict(overlap=0, capacity=1),
             "sub-batches-of-3": dict(overlap=0, capacity=3)}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["spread-over-chunks", "tandem-over-line-capacity", "microsatellite-dense", "gc-generic"])
def test_representative_and_duplicate_in_different_chunks_and_sub_batches(gpu_ctx, baseline, name, model, schedule):
    """Chunks and sub-batches of one to three windows: a duplicate's representative is folded in another chunk, ring slot or sub-batch, the dense
    and generic hand-offs come from any of them, and the counters are what the default schedule without dedup reports."""
    case, off = baseline(name, model)
    kw = SCHEDULES[schedule]
    on = _run(gpu_ctx, case, True, model=model, **kw)
    if model == MODELS[0] and kw["overlap"] > 0:
        assert on["chunks"] >= 2
    else:
        assert on["chunks"] == 0
    _check_map(on, 0)
    _same_outputs(on, off)
    on4 = _run(gpu_ctx, case, True, bits=4, model=model, **kw)
    _check_map(on4, 4)
    _same_outputs(on4, off)


@pytest.mark.parametrize("bits", [0, 4])
def test_the_map_is_the_same_on_every_call(gpu_ctx, baseline, bits):
    case, off = baseline("spread-over-chunks", MODELS[0])
    a = _run(gpu_ctx, case, True, bits=bits, folds=3)
    b = _run(gpu_ctx, case, True, bits=bits)
    for m in a["maps"] + b["maps"]:
        assert np.array_equal(m, a["maps"][0])
    _check_map(a, bits)
    _same_outputs(a, off)
    _same_outputs(b, off)


def test_switch_and_setters(gpu_ctx, baseline):
    case, off = baseline("short-both-strands", MODELS[0])
    for bad in (-1, 2):
        with pytest.raises(capi.MirpError):
            gpu_ctx._check(gpu_ctx.lib.mirp_set_fold_dedup(gpu_ctx.h, bad), "mirp_set_fold_dedup")
    for bad in (-1, 65):
        with pytest.raises(capi.MirpError):
            gpu_ctx.set_fold_dedup_hash_bits(bad)
    on = _run(gpu_ctx, case, True)                       # the default is on
    assert on["duplicates"] == 2 and on["map"].tolist() == [-1, -1, 0, -1, 1, -1]
    again_off = _run(gpu_ctx, case, False)               # and off forgets the map of the fold before it
    assert again_off["duplicates"] == 0 and (again_off["map"] == -1).all()
    _same_outputs(again_off, off)
    # fold_batch folds every sequence it is given, repeated or not: the hand-off counts of repeated sequences stay per sequence
    gc = "G" * 150 + "C" * 150
    gpu_ctx.fold_batch_raw([gc, gc, gc], 300, 96)
    assert gpu_ctx.last_fold_fallbacks() == 3
