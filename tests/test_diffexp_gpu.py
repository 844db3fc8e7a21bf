"""GPU tests of the differential-expression verb (mirp_diffexp, diffexp_kernels.hip) against restatement (a) of
tests/diffexp_restatement.py: n = 0, 1, 2; k_A = 0 and k_A = n; n + 1 and either side of k_A at C - 1, C, C + 1 and 2 C + 1 terms (the device cuts
the terms into chunks outwards from k_A); k_A at the mode; the mirror tie; the Poisson case; r < 1; denominators that overflow (p exactly 0); a
feature of 2^20 + 3 reads beside light ones; waves that serve three jobs and more; a seeded sweep of 2,000 features x (3 + 3) samples under the
four dispersion modes; determinism; the refusals; and the command line on a matrix that `loci` wrote in the same test.

The tolerance on p.  Restatement (a) differs from the 60-digit restatement (b) by at most WORST_A_VS_B (relative) over these inputs, the feature
of 2^20 + 3 reads and every feature of the sweep under every mode included (profiles/tools/diffexp_error.py --every 1, 8,020 tests;
tests/test_diffexp_cpu.py asserts it again for n <= 65,536 on every tenth feature of the sweep and on the worst one).  The device may differ
from (a) by 64 times that: it adds in another order and its log and exp are good to 1 ulp where libm's are to half of one.  An implementation
that forms u from differences of lgamma values is off by 1e-9 and more at n = 10^6, orders of magnitude beyond this."""
import math
import os

import numpy as np
import pytest

from mir_prefer_amd import capi, diffexp
from tests import diffexp_restatement as R

pytestmark = pytest.mark.gpu

C = capi.DIFFEXP_CHUNK
SUM = 6                                              # the sum kernel's family of mirp_last_jobs_per_slot
WORST_A_VS_B = 1.54e-12                              # measured 1.531e-12 (feature 1113 of the sweep under "feature", p = 1.5e-234; 1.7e-13 without it)
TOL = 64 * WORST_A_VS_B                              # 9.86e-11
MOMENT_TOL = 1e-12


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return np.where(got == want, 0.0, r)


def jobs_of(ka, kb):
    ka, kb = np.asarray(ka, dtype=np.int64), np.asarray(kb, dtype=np.int64)
    return int(np.where(ka + kb > 0, (kb + 1 + C - 1) // C + (ka + C - 1) // C, 0).sum())


def check(ctx, counts, sf, groups, mode, phi=0.0, min_mean=10.0, pseudo=0.5, tag=""):
    """One call against restatement (a): counts exactly, moments and dispersions at MOMENT_TOL, p at TOL; prints the worst figures."""
    counts = np.asarray(counts, dtype=np.uint64)
    got, stats = ctx.diffexp(counts, sf, groups, mode, phi, min_mean, pseudo)
    want, phi_c = R.diffexp_numpy(counts, sf, groups, mode, phi, min_mean, pseudo)
    assert (got["k_a"] == want["k_a"]).all() and (got["k_b"] == want["k_b"]).all()
    n = (want["k_a"] + want["k_b"]).astype(np.int64)
    assert stats["features"] == len(counts) and stats["tested"] == int((n > 0).sum()) and stats["terms"] == int((n[n > 0] + 1).sum())
    assert stats["jobs"] == jobs_of(want["k_a"], want["k_b"])
    worst = {f: float(rel(got[f], want[f]).max()) if len(counts) else 0.0 for f in ("base_mean", "mean_a", "mean_b", "dispersion")}
    tested = n > 0
    fc = float(rel(got["log2fc"][tested], want["log2fc"][tested]).max()) if tested.any() else 0.0
    pe = rel(got["p"], want["p"])
    print("diffexp %s: phi_c %.17g (restatement %.17g), worst relative difference: moments %s log2fc %.3g p %.3g (feature %d)"
          % (tag, stats["phi_c"], phi_c, worst, fc, float(pe.max()) if len(pe) else 0.0, int(pe.argmax()) if len(pe) else -1))
    assert max(worst.values()) <= MOMENT_TOL and fc <= 1e-11, (worst, fc)
    assert abs(stats["phi_c"] - phi_c) <= MOMENT_TOL * max(abs(phi_c), 1e-300)
    assert (got["p"][~tested] == -1.0).all() and (want["p"][~tested] == -1.0).all()
    assert (pe <= TOL).all(), (tag, int(pe.argmax()), float(pe.max()), got["p"][pe.argmax()], want["p"][pe.argmax()])
    assert ((got["p"][tested] >= 0) & (got["p"][tested] <= 1)).all()
    return got, stats


# ---------------------------------------------------------------------------------------------------- 1: the sizes at which the kernels can go wrong
def test_single_cases_match_the_restatement(gpu_ctx):
    seen = {}
    for case in R.single_cases():
        name, ka, kb, sa, sb, phi = case
        got, stats = check(gpu_ctx, [[ka, kb]], [sa, sb], [0, 1], "fixed", phi, tag=name)
        assert float(got["dispersion"][0]) == phi
        seen[name] = float(got["p"][0])
    assert seen["n0"] == -1.0 and seen["overflow"] == 0.0 and seen["overflow_nb"] == 0.0 and 0 < seen["tiny_p"] < 1e-150
    assert seen["n1a"] == 1.0 and seen["mode"] == 1.0
    # the mirror tie: with equal groups t(a) = t(n - a), so both tails count and p is twice the tail up to the observed split
    one_tail = sum(math.comb(10, a) for a in range(0, 4)) / 1024.0               # 3 of 10 at equal size factors: a = 0 .. 3 and 7 .. 10
    assert abs(seen["mirror_pois"] - 2 * one_tail) <= 1e-14


def test_one_heavy_feature_beside_light_ones(gpu_ctx):
    _, ka, kb, sa, sb, phi = R.BIG
    counts = [[3, 4], [ka, kb], [0, 0], [10, 2]]
    got, stats = check(gpu_ctx, counts, [sa, sb], [0, 1], "fixed", phi, tag="2^20 + 3")
    assert ka + kb == (1 << 20) + 3 and stats["jobs"] == 2 + ((kb + 1 + C - 1) // C + (ka + C - 1) // C) + 0 + 2
    assert gpu_ctx.last_jobs_per_slot(SUM) == (1, 1)
    alone, _ = gpu_ctx.diffexp(counts[1:2], [sa, sb], [0, 1], "fixed", phi)
    assert alone.tobytes() == got[1:2].tobytes()


def test_waves_serve_three_jobs_and_more(gpu_ctx):
    counts, sf, groups = R.sweep(seed=21, features=7000)
    got, stats = check(gpu_ctx, counts, sf, groups, "fixed", 0.25, tag="slot reuse")
    launches, per_slot = gpu_ctx.last_jobs_per_slot(SUM)
    assert stats["jobs"] > 3 * 4096 and launches == 1 and per_slot >= 3, (stats, launches, per_slot)
    # the row of a feature does not depend on the jobs its wave served before
    for lo in (0, 1, 3333, 6999):
        alone, _ = gpu_ctx.diffexp(counts[lo:lo + 1], sf, groups, "fixed", 0.25)
        assert alone.tobytes() == got[lo:lo + 1].tobytes(), lo
    assert gpu_ctx.last_jobs_per_slot(SUM) == (1, 1)


# ---------------------------------------------------------------------------------------------------- 2: the sweep
@pytest.fixture(scope="module")
def sweep():
    return R.sweep()


@pytest.mark.parametrize("mode", R.MODES)
def test_sweep_under_every_dispersion_mode(gpu_ctx, sweep, mode):
    counts, sf, groups = sweep
    got, stats = check(gpu_ctx, counts, sf, groups, mode, 0.3, tag="sweep " + mode)
    assert np.allclose(sf, diffexp.size_factors(counts, "mor"), rtol=1e-14, atol=0)
    assert stats["tested"] < stats["features"] == 2000                         # some features have no read at all
    again, stats2 = gpu_ctx.diffexp(counts, sf, groups, mode, 0.3)
    assert again.tobytes() == got.tobytes() and stats2 == stats               # determinism: byte for byte
    # the order of the samples within the call is free: groups interleaved, the same test
    perm = [0, 3, 1, 4, 2, 5]
    mixed, _ = check(gpu_ctx, counts[:, perm], sf[perm], [groups[j] for j in perm], mode, 0.3, tag="sweep %s, groups interleaved" % mode)
    assert (mixed["k_a"] == got["k_a"]).all() and (mixed["k_b"] == got["k_b"]).all()


def test_nothing_to_test_and_refusals(gpu_ctx):
    none, stats = gpu_ctx.diffexp(np.zeros((0, 4), np.uint64), [1, 1, 1, 1], [0, 0, 1, 1])
    assert len(none) == 0 and stats == {"features": 0, "tested": 0, "jobs": 0, "terms": 0, "phi_c": 0.0}
    got, stats = gpu_ctx.diffexp(np.zeros((3, 2), np.uint64), [1, 1], [0, 1], "fixed", 0.1)
    assert (got["p"] == -1.0).all() and stats["tested"] == 0 and stats["jobs"] == 0 and gpu_ctx.last_jobs_per_slot(SUM) == (0, 0)
    ok = np.array([[5, 6, 7, 8]], dtype=np.uint64)
    for counts, sf, groups, mode, phi, mm, ps, why in (
            (ok, [1, 1, 1, 1], [0, 0, 0, 0], "max", 0, 10, 0.5, "without a sample"),
            (ok, [1, 1, 0, 1], [0, 0, 1, 1], "max", 0, 10, 0.5, "size factor 3"),
            (ok, [1, 1, np.inf, 1], [0, 0, 1, 1], "max", 0, 10, 0.5, "size factor 3"),
            (ok, [1, 1, 1, 1], [0, 0, 1, 2], "max", 0, 10, 0.5, "group 4"),
            (ok, [1, 1, 1, 1], [0, 0, 1, 1], 4, 0, 10, 0.5, "mode"),
            (ok, [1, 1, 1, 1], [0, 0, 1, 1], "fixed", -1.0, 10, 0.5, "phi"),
            (ok, [1, 1, 1, 1], [0, 0, 1, 1], "max", 0, np.nan, 0.5, "min_mean"),
            (ok, [1, 1, 1, 1], [0, 0, 1, 1], "max", 0, 10, -0.5, "pseudo"),
            (ok[:, :2], [1, 1], [0, 1], "max", 0, 10, 0.5, "two or more samples"),
            (ok[:, :1], [1], [0], "fixed", 0, 10, 0.5, "n_samples"),
            (np.array([[1 << 40, 1, 1, 1]], dtype=np.uint64), [1, 1, 1, 1], [0, 0, 1, 1], "max", 0, 10, 0.5, "2^40"),
            (np.full((3, 4), (1 << 39), dtype=np.uint64), [1, 1, 1, 1], [0, 0, 1, 1], "max", 0, 10, 0.5, "terms"),
            (ok, [1, 1, 1, 1], [0, 0, 1, 1], "max", 0, 1000, 0.5, "no common dispersion")):
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.diffexp(counts, sf, groups, mode, phi, mm, ps)
        assert why in str(e.value), (why, str(e.value))
    # mode "feature" needs no common dispersion
    got, stats = gpu_ctx.diffexp(ok, [1, 1, 1, 1], [0, 0, 1, 1], "feature", 0, 1000)
    assert stats["phi_c"] == 0.0 and 0 < float(got["p"][0]) <= 1


# ---------------------------------------------------------------------------------------------------- 3: the command line on a matrix that loci wrote
def test_the_verb_on_a_matrix_of_loci(gpu_ctx, tmp_path):
    from tests.test_clusters_cpu import random_records
    from tests.test_clusters_gpu import _cli, write_sams
    names, lens = ["chrA", "chrB"], [40000, 25000]
    recs = random_records(np.random.RandomState(90), lens, 5, 9000, 300)
    sams = [str(tmp_path / ("s%d.sam" % i)) for i in range(5)]
    write_sams(sams, names, lens, recs)
    bed = tmp_path / "bins.bed"
    bed.write_text("".join("%s\t%d\t%d\tbin_%s_%d\n" % (c, s, s + 500, c, s) for c, ln in zip(names, lens) for s in range(0, ln - 500, 500)))
    r = _cli("mir_prefer_amd.loci", ["-o", "study", str(bed)] + sams, tmp_path)
    assert r.returncode == 0, r.stderr
    matrix = tmp_path / "study.counts.tsv"
    cols = matrix.read_text().split("\n")[0].split("\t")[1:]
    assert len(cols) == 5
    a, b = [cols[0], cols[2], cols[4]], [cols[3], cols[1]]
    r = _cli("mir_prefer_amd.diffexp", ["-a", ",".join(a), "-b", b[0], "-b", b[1], "--min-mean", "2", str(matrix)], tmp_path)
    assert r.returncode == 0, r.stderr
    base = tmp_path / "study.diffexp"
    feats, counts = diffexp.read_matrix(str(matrix), a, b)
    sf = diffexp.size_factors(counts, "mor")
    assert np.allclose(sf, R.size_factors_plain(counts.tolist(), "mor"), rtol=1e-13, atol=0)
    want, phi_c = R.diffexp_numpy(counts, sf, [0, 0, 0, 1, 1], "max", 0.0, 2.0, 0.5)
    padj = np.array(R.bh_plain(want["p"].tolist()))
    lines = (base.with_suffix(".diffexp.tsv")).read_bytes().split(b"\n")
    assert lines[0] + b"\n" == diffexp.TSV_HEADER and lines[-1] == b"" and len(lines) == len(feats) + 2
    fields = ("base_mean", "mean_a", "mean_b", "log2fc", "dispersion", "p")
    tested = 0
    for i, line in enumerate(lines[1:-1]):
        sp = line.decode().split("\t")
        assert sp[0] == feats[i] and len(sp) == 8                              # the non-numeric bytes are exact
        for f, text in zip(fields, sp[1:7]):
            w = float(want[f][i])
            if f == "p" and w < 0:
                assert text == "NA" and sp[7] == "NA"
            else:
                assert abs(float(text) - w) <= (1e-3 if f == "p" else 1e-5) * abs(w), (i, f, text, w)      # %.3e and %.6g keep 4 and 6 digits
        if want["p"][i] >= 0:
            tested += 1
            assert abs(float(sp[7]) - padj[i]) <= 1e-3 * padj[i]
    assert tested > 50
    norm = (tmp_path / "study.diffexp.norm.tsv").read_text().split("\n")
    assert norm[0].split("\t") == ["name"] + a + b and len(norm) == len(feats) + 2
    y = counts.astype(np.float64) / sf
    for i in (0, len(feats) // 2, len(feats) - 1):
        sp = norm[1 + i].split("\t")
        assert sp[0] == feats[i] and all(abs(float(t) - v) <= 0.00051 for t, v in zip(sp[1:], y[i]))
    fac = (tmp_path / "study.diffexp.factors.tsv").read_text().split("\n")
    assert fac[0] + "\n" == diffexp.FACTORS_HEADER.decode() and [l.split("\t")[:3] for l in fac[1:-1]] == \
        [[s, "A" if j < 3 else "B", str(int(counts[:, j].sum()))] for j, s in enumerate(a + b)]
    assert all(abs(float(l.split("\t")[3]) - s) <= 1e-9 * s for l, s in zip(fac[1:-1], sf))
    err = r.stderr.decode()
    assert err.startswith("diffexp: %d features, %d tested, " % (len(feats), tested)) and "written to" in err
    # a refused run removes the files of the earlier one
    r = _cli("mir_prefer_amd.diffexp", ["-a", ",".join(a), "-b", ",".join(b), "--min-mean", "1e9", str(matrix)], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and "common dispersion" in r.stderr.decode()
    assert not any(os.path.exists(p) for p in diffexp.output_paths(str(base)))
