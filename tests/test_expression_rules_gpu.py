"""GPU: the expression half of predict_kernel -- d_expression, the pass / fail tree, the winner among structures and matures -- on the planted cases
of tests/expression_cases.py, against its plain restatement (which tests/test_expression_rules_cpu.py pins to direct calls of the reference).
Everything compared is an integer.  Then the same windows tiled to more than three per workgroup of the production launch: a workgroup's second
and third window, served with the LDS tables of the first."""
import random

import numpy as np
import pytest

from mir_prefer_amd import records
from tests import expression_cases as ec

pytestmark = pytest.mark.gpu
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (allow_3nt, allow_no_star)
FILTER = 4                                          # the filter kernel's family of mirp_last_jobs_per_slot
MIRNA_FIELDS = ("window", "tid", "fold_s", "fold_e", "mat_s", "mat_e", "star_s", "star_e", "strand", "has_star", "line", "ss_off", "ss_len", "reserved",
                "total_depth_mature", "total_depth_star")


def params(n_samples, allow_3nt, allow_no_star):
    return (n_samples, ec.MIN_MATURE, ec.MAX_MATURE, allow_3nt, allow_no_star, ec.MINLEN)


def groups():
    """{n_samples: indices of the planted cases with that many samples}"""
    cases, _ = ec.planted()
    out = {}
    for k, c in enumerate(cases):
        out.setdefault(c["n_samples"], []).append(k)
    return out


def sat(x):
    return min(x, ec.I32_MAX)


def want_records(c, t, structs):
    """the -d records the restatement states for one window, as {(mature, structure): fields 3 ..}, and its per-window fields"""
    out = {}
    for (mi, si), p in t["pairs"].items():
        line, off, ln = structs[si][:3]
        r = [line, off, ln, p["code"], p["flags"]]
        if p["code"] == 0:
            star_s, star_e, fold_s, fold_e = p["geom"]
            k = p["counters"]
            r += [fold_s, fold_e, star_s, star_e, sat(k["this"]), sat(k["anti"]), sat(k["mature"]), sat(k["iso"]), sat(k["star"])] + [sat(x) for x in k["imp"]]
            r += [k["distance"]] + k["each"]
        out[(mi, si)] = r
    return out, [t["n_structs"], t["any_in_range"], len(t["mirnas"])]


def got_records(rec):
    """{window: {(mature, structure): fields 3 ..}}, {window: per-window fields}"""
    pairs, perw = {}, {}
    for r in rec.tolist():
        if r[1] < 0:
            assert r[0] not in perw
            perw[r[0]] = r[2:5]
        else:
            d = pairs.setdefault(r[0], {})
            assert (r[1], r[2]) not in d
            d[(r[1], r[2])] = r[3:8] + (r[8:] if r[6] == 0 else [])
    return pairs, perw


def check(cases, truths, mir, nm, st, rec):
    assert (st == 0).all()
    pairs, perw = got_records(rec)
    assert sorted(perw) == list(range(len(cases)))
    for k, (c, t) in enumerate(zip(cases, truths)):
        want, want_w = want_records(c, t, ec.structures_of(c))
        assert perw[k] == want_w, c["name"]
        got = pairs.get(k, {})
        assert sorted(got) == sorted(want), c["name"]
        for key in want:
            assert got[key] == want[key], (c["name"], key)
        assert nm[k] == len(t["mirnas"]), c["name"]
        for j, m in enumerate(t["mirnas"]):
            assert [int(mir[k, j][f]) for f in MIRNA_FIELDS] == [k] + [m[f] for f in MIRNA_FIELDS[1:]], (c["name"], j)


_runs = {}


def run(gpu_ctx, ns, combo):
    """the planted windows of one sample count through predict_batch_reasons, one call, kept for the tests that share it"""
    key = (ns,) + combo
    if key not in _runs:
        cases, rec = ec.planted()
        idx = groups()[ns]
        sub = [cases[k] for k in idx]
        W, M, raw = ec.batch(sub)
        _runs[key] = (idx, sub, (W, M, raw), gpu_ctx.predict_batch_reasons(W, M, rec, raw, params(ns, *combo)))
    return _runs[key]


@pytest.mark.parametrize("allow_3nt,allow_no_star", COMBOS)
def test_records_and_mirnas_equal_the_restatement(allow_3nt, allow_no_star, gpu_ctx):
    combo = (allow_3nt, allow_no_star)
    truth = ec.truth(*combo)
    assert sorted(groups()) == sorted(set(ec.SAMPLE_COUNTS) | {3})
    for ns in sorted(groups()):
        idx, sub, _, (mir, nm, st, rec) = run(gpu_ctx, ns, combo)
        assert rec.shape[1] == 21 + ns
        check(sub, [truth[k] for k in idx], mir, nm, st, rec)


def test_the_kernel_without_the_reasons_gives_the_same_mirnas(gpu_ctx):
    _, rec = ec.planted()
    for combo in COMBOS:
        idx, sub, (W, M, raw), (mir, nm, st, _) = run(gpu_ctx, 2, combo)
        mir0, nm0, st0 = gpu_ctx.predict_batch(W, M, rec, raw, params(2, *combo))
        assert (st0 == 0).all() and (nm0 == nm).all()
        live = np.arange(records.MAX_MIRNA_PER_WINDOW)[None, :] < nm[:, None]
        assert (mir0[live] == mir[live]).all() and live.sum() > 20


def test_one_window_per_call_gives_the_records_of_the_batch(gpu_ctx):
    _, rec = ec.planted()
    idx, sub, (W, M, raw), (mir, nm, st, rr) = run(gpu_ctx, 2, (1, 1))
    pairs, perw = got_records(rr)
    # (a call's record pool holds 96 records per window and 1,024 more: the window of 70 lines x 70 matures runs in company only)
    small = [k for k, c in enumerate(sub) if len(c["lines"]) * len(c["matures"]) <= 500]
    picks = sorted(random.Random(20261020).sample(small, len(sub) // 10))
    heavy = [k for k, c in enumerate(sub) if c["tags"].get("select") == "last" or c["tags"].get("matures") == "seventy_one_line"][:2]
    for k in sorted(set(picks + heavy)):
        W1, M1, raw1 = ec.batch([sub[k]])
        mir1, nm1, st1, rr1 = gpu_ctx.predict_batch_reasons(W1, M1, rec, raw1, params(2, 1, 1))
        p1, w1 = got_records(rr1)
        assert st1[0] == 0 and w1[0] == perw[k] and p1.get(0, {}) == pairs.get(k, {}), sub[k]["name"]
        assert nm1[0] == nm[k]
        for f in MIRNA_FIELDS[1:]:
            assert (mir1[0, :nm1[0]][f] == mir[k, :nm[k]][f]).all(), (sub[k]["name"], f)


def test_window_with_more_matures_than_the_table_is_its_matures_one_by_one(gpu_ctx):
    """70 candidate matures: the kernel's table holds 64, the window is run again with room for all.  Its miRNA list is that of its matures as 70
    one-mature windows, in stable depth-descending order, the first eight (outcomes per mature are independent, only the order matters)."""
    _, rec = ec.planted()
    idx, sub, _, (mir, nm, st, _) = run(gpu_ctx, 2, (1, 1))
    seen = 0
    for k, c in enumerate(sub):
        if c["tags"].get("matures") != "seventy_one_line":
            continue
        order = sorted(range(70), key=lambda j: -c["matures"][j][3])
        W1, M1, raw1 = ec.batch([dict(c, matures=[c["matures"][j]]) for j in order])
        mir1, nm1, st1 = gpu_ctx.predict_batch(W1, M1, rec, raw1, params(2, 1, 1))
        assert (st1 == 0).all() and (nm1 <= 1).all()
        single = mir1[nm1 == 1, 0][:records.MAX_MIRNA_PER_WINDOW]
        assert nm[k] == len(single)
        for f in MIRNA_FIELDS[1:]:
            assert (mir[k, :nm[k]][f] == single[f]).all(), (c["name"], f)
        seen += nm[k] >= 2
    assert seen >= 2


# ---------------------------------------------------------------------------------------------------- a workgroup's second and third window
PRED_SLOTS = 16384          # min(windows, 64 x 256 CUs) workgroups; workgroup b serves the windows b, b + 16384, b + 32768, ...
COPY_STEP = 2000000         # coordinates of one copy of the planted windows to the next: beyond both contigs' planted stretches


def test_workgroups_serve_three_windows(gpu_ctx):
    """The planted two-sample windows tiled to more than 3 x 16,384, every copy at coordinates of its own with its own reads.  Order: the heavy
    windows first (70 lines x 70 matures with both capacity re-runs, 70 lines, twelve and seventy matures), so that the first workgroups go from
    such a window to a one-line window and then to whatever the shuffle gives.  Every copy's records and miRNAs are those of its original (pinned
    to the restatement above), moved by the copy's offset."""
    cases, rec = ec.planted()
    idx, sub_all, _, (_, nm_a, _, rr_a) = run(gpu_ctx, 2, (1, 1))
    keep = [k for k, c in enumerate(sub_all) if max(len(l[0]) for l in c["lines"]) <= ec.STRIDE]          # without the 520-nt lines of the sample cases
    sub = [sub_all[k] for k in keep]
    W0, M0, raw0 = ec.batch(sub)
    mir0, nm0, st0, rr0 = gpu_ctx.predict_batch_reasons(W0, M0, rec, raw0, params(2, 1, 1))
    pa, wa = got_records(rr_a)
    p0, w0 = got_records(rr0)
    assert raw0["stride"] == ec.STRIDE and (st0 == 0).all() and (nm0 == nm_a[keep]).all()
    assert all(p0.get(j, {}) == pa.get(k, {}) and w0[j] == wa[k] for j, k in enumerate(keep))          # the originals are the records pinned above
    B = len(sub)
    copies = -(-(3 * PRED_SLOTS + 1) // B)
    N = copies * B
    heavy = [k for k, c in enumerate(sub) if len(c["lines"]) > 1 or len(c["matures"]) > 2]
    light = [k for k in range(B) if k not in set(heavy)]
    assert len(heavy) >= 10 and all(len(sub[k]["lines"]) == 1 for k in light)
    heavy.sort(key=lambda k: -len(sub[k]["lines"]) * len(sub[k]["matures"]))
    tiles = [(k, c) for k in heavy for c in range(copies)]
    rest = [(k, c) for k in light for c in range(copies)]
    random.Random(5).shuffle(rest)
    tiles += rest
    assert len(tiles) == N and 3 * PRED_SLOTS < N and len(heavy) * copies < PRED_SLOTS
    orig = np.array([k for k, _ in tiles])
    off = np.array([c for _, c in tiles], dtype=np.int64) * COPY_STEP
    # windows, matures, fold output
    W = W0[orig].copy()
    W["ws"] += off; W["we"] += off; W["loc_s"] += off; W["loc_e"] += off
    cnt = W0["n_matures"][orig].astype(np.int64)
    W["mature_off"] = np.cumsum(cnt) - cnt
    src = np.concatenate([np.arange(W0["mature_off"][k], W0["mature_off"][k] + W0["n_matures"][k]) for k in orig])
    M = M0[src].copy()
    moff = np.repeat(off, cnt)
    M["start"] += moff; M["end"] += moff
    raw = {"lines": raw0["lines"][orig], "ss": raw0["ss"][orig], "n_lines": raw0["n_lines"][orig], "stride": raw0["stride"], "max_lines": raw0["max_lines"]}
    # records: every copy of all planted reads (those of the other sample counts lie in no window of this call)
    assert int(rec["pos"].max()) < COPY_STEP and int(rec["pos"].max()) + copies * COPY_STEP < 2 ** 31
    A = np.tile(rec, copies)
    A["pos"] += np.repeat(np.arange(copies, dtype=np.int64) * COPY_STEP, len(rec)).astype(np.int32)
    A = A[np.lexsort((A["pos"], A["tid"]))]
    mir, nm, st, rr = gpu_ctx.predict_batch_reasons(W, M, A, raw, params(2, 1, 1))
    launches, per_slot = gpu_ctx.last_jobs_per_slot(FILTER)
    print("filter kernel: %d windows, %d launches, %d windows per workgroup, %d records" % (N, launches, per_slot, len(rr)))
    assert per_slot == -(-N // PRED_SLOTS) >= 4 and launches >= 2          # exact for 256 CUs: 3 full rounds of the workgroups and a part of a fourth
    assert (st == 0).all() and (nm == nm0[orig]).all()
    # miRNAs: those of the original, moved
    live = np.arange(records.MAX_MIRNA_PER_WINDOW)[None, :] < nm[:, None]
    want = mir0[orig].copy()
    for f in ("fold_s", "fold_e", "mat_s", "mat_e", "star_s", "star_e"):
        want[f] += off[:, None].astype(np.int32)
    want["window"] = np.arange(N, dtype=np.int32)[:, None]
    assert (mir[live] == want[live]).all() and live.sum() > 100 * copies
    # records: those of the original in (window, mature, structure) order, window renumbered, coordinates moved where the pair has any
    def ordered(r):
        return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]
    r0 = ordered(rr0)
    first = np.searchsorted(r0[:, 0], np.arange(B))
    count = np.searchsorted(r0[:, 0], np.arange(B), side="right") - first
    rows = np.concatenate([np.arange(first[k], first[k] + count[k]) for k in orig])
    want = r0[rows].copy()
    nrec = count[orig]
    want[:, 0] = np.repeat(np.arange(N), nrec)
    moved = (want[:, 1] >= 0) & (want[:, 6] == 0)
    want[moved, 8:12] += np.repeat(off, nrec)[moved, None].astype(np.int32)
    got = ordered(rr)
    assert got.shape == want.shape
    coords = (want[:, 1] < 0) | (want[:, 6] == 0)          # a pair without coordinates (a get_maturestar_info failure) is compared up to its flags
    assert (got[:, :8] == want[:, :8]).all() and (got[coords] == want[coords]).all()
    # the record of the call after: a small call resets it
    gpu_ctx.predict_batch(W0[:5], M0, rec, {k: (v[:5] if isinstance(v, np.ndarray) else v) for k, v in raw0.items()}, params(2, 1, 1))
    assert gpu_ctx.last_jobs_per_slot(FILTER) == (1, 1)
