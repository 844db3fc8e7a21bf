"""CPU tests of the differential-expression verb: worked examples as literals (a 2 x 2 matrix by hand, median-of-ratios size
factors over an even and an odd number of usable features, every dispersion mode, Benjamini-Hochberg); restatement (a) of
tests/diffexp_restatement.py against the 60-digit restatement (b) on the inputs of the GPU tests (every single case with n <= 65,536, every
tenth feature of the sweep and the worst one under the four modes), with the error bound the GPU tolerance is derived from and the distance every term keeps from
the slack 1 + 1e-7; (a) against scipy's exact binomial test in the Poisson case; the float64 moments against exact rationals; the matrix reader
with every refused line; the struct layouts against the C header, the new symbol and the unchanged ABI version; the kernels' resources; and the
option errors of the command line, which exit 2 without opening a device."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd import capi, diffexp
from tests import diffexp_restatement as R
from tests.test_clusters_cpu import ROOT

WORST_A_VS_B = 1.54e-12          # as tests/test_diffexp_gpu.py has it: measured over all inputs by profiles/tools/diffexp_error.py --every 1
WORST_FEATURE = 1113             # of the sweep, under --dispersion feature (p = 1.5e-234): where that figure comes from


# ---------------------------------------------------------------------------------------------------- worked examples
def test_two_by_two_by_hand():
    # k_A = 1, k_B = 3, equal size factors, Poisson: t(a) ~ C(4, a); u <= u(1) at a = 0, 1, 3, 4 -> p = (1 + 4 + 4 + 1) / 16
    n, ka, ra, rb, cr = R.single_params(("", 1, 3, 1.0, 1.0, 0.0))
    assert (n, ka, ra, rb, cr) == (4, 1, -1.0, -1.0, 1.0)
    assert R.p_numpy(n, ka, ra, rb, cr) == 10 / 16 and float(R.p_mp(n, ka, ra, rb, cr)[0]) == 10 / 16
    # size factors 1 and 3: a read falls to A with probability 1 / 4; t(a) ~ C(4, a) 3^(4 - a) = 81, 108, 54, 12, 1; observed a = 2 -> (54 + 12 + 1) / 256
    n, ka, ra, rb, cr = R.single_params(("", 2, 2, 1.0, 3.0, 0.0))
    assert cr == 1.0 / 3.0 and abs(R.p_numpy(n, ka, ra, rb, cr) - 67 / 256) <= 1e-15
    # dispersion 1 with one sample each: r = 1, the counts are geometric and every split of n is equally likely at equal size factors -> p = 1
    n, ka, ra, rb, cr = R.single_params(("", 2, 5, 1.0, 1.0, 1.0))
    assert (ra, rb, cr) == (1.0, 1.0, 1.0) and abs(R.p_numpy(n, ka, ra, rb, cr) - 1.0) <= 1e-15
    # the 2 x 2 matrix end to end: means, log2fc with the pseudo-count, the untested second feature
    got, phi = R.diffexp_numpy([[1, 3], [0, 0]], [1.0, 1.0], [0, 1], "fixed", 0.0, pseudo=0.5)
    assert got["base_mean"].tolist() == [2.0, 0.0] and got["mean_a"].tolist() == [1.0, 0.0] and got["mean_b"].tolist() == [3.0, 0.0]
    assert got["log2fc"].tolist() == [math.log2(3.5 / 1.5), 0.0] and got["p"].tolist() == [0.625, -1.0] and phi == 0.0
    assert diffexp.adjust(got["p"]).tolist() == [0.625, -1.0]


def test_median_of_ratios_even_and_odd():
    # two usable features (the zero row is left out): the median is the mean of the two log ratios
    counts = np.array([[2, 8], [0, 5], [9, 1]], dtype=np.uint64)
    want = [math.exp((math.log(2 / 4) + math.log(9 / 3)) / 2), math.exp((math.log(8 / 4) + math.log(1 / 3)) / 2)]
    assert np.allclose(diffexp.size_factors(counts, "mor"), want, rtol=1e-15, atol=0)
    assert np.allclose(R.size_factors_plain(counts.tolist(), "mor"), want, rtol=1e-15, atol=0)
    # three usable features: the middle ratio
    counts = np.array([[2, 8], [4, 4], [9, 1], [3, 0]], dtype=np.uint64)
    assert np.allclose(diffexp.size_factors(counts, "mor"), [1.0, 1.0], rtol=1e-15, atol=0)
    counts = np.array([[2, 8], [1, 4], [9, 1]], dtype=np.uint64)
    assert np.allclose(diffexp.size_factors(counts, "mor"), [0.5, 2.0], rtol=1e-15, atol=0)
    assert np.allclose(R.size_factors_plain(counts.tolist(), "mor"), [0.5, 2.0], rtol=1e-15, atol=0)
    # total: column sums over their geometric mean; none: ones
    assert np.allclose(diffexp.size_factors(counts, "total"), [12 / math.sqrt(12 * 13), 13 / math.sqrt(12 * 13)], rtol=1e-15, atol=0)
    assert np.allclose(R.size_factors_plain(counts.tolist(), "total"), diffexp.size_factors(counts, "total"), rtol=1e-15, atol=0)
    assert diffexp.size_factors(counts, "none").tolist() == [1.0, 1.0]
    with pytest.raises(ValueError) as e:
        diffexp.size_factors(np.array([[0, 3], [4, 0]], dtype=np.uint64), "mor")
    assert "--norm total" in str(e.value)
    with pytest.raises(ValueError):
        diffexp.size_factors(np.array([[0, 3], [0, 1]], dtype=np.uint64), "total")


def test_moments_and_every_dispersion_mode():
    # y = counts (size factors 1): feature 0 A {10, 14} B {20, 28}; feature 1 flat; feature 2 below --min-mean
    counts = [[10, 14, 20, 28], [50, 50, 50, 50], [1, 0, 2, 1]]
    sf, groups = [1.0, 1.0, 1.0, 1.0], [0, 0, 1, 1]
    m = R.moments_numpy(counts, sf, groups)
    assert m["q"].tolist() == [18.0, 50.0, 1.0] and m["qa"].tolist() == [12.0, 50.0, 0.5] and m["qb"].tolist() == [24.0, 50.0, 1.5]
    # v = ((2^2 + 2^2) + (4^2 + 4^2)) / 2 = 20, z = 18 -> alpha = 2 / 324; flat: (0 - 50) / 2500; (0.5 + 0.5) / 2 = 0.5, z = 1 -> -0.5
    assert m["alpha"].tolist() == [2 / 324, -0.02, -0.5] and m["ka"].tolist() == [24, 100, 1] and m["kb"].tolist() == [48, 100, 3]
    assert R.common_dispersion(m["q"], m["alpha"], 10.0) == max(0.0, (2 / 324 - 0.02) / 2) == 0.0
    assert R.common_dispersion(m["q"], m["alpha"], 0.5) == 0.0 and R.common_dispersion(m["q"], m["alpha"], 18.0) == 0.0
    assert R.common_dispersion(m["q"], m["alpha"], 51.0) is None
    assert R.common_dispersion([20, 30, 40], [0.1, 0.5, 0.3], 10.0) == 0.3 and R.common_dispersion([20, 30, 40, 5], [0.1, 0.5, 0.3, 9.0], 10.0) == 0.3
    assert R.common_dispersion([20, 30, 40, 50], [0.1, 0.5, 0.3, 0.2], 10.0) == 0.25
    a = [0.4, 0.1, -0.2]
    assert R.dispersions(a, 0, 7.0, 0.25).tolist() == [0.4, 0.25, 0.25] and R.dispersions(a, 1, 7.0, 0.25).tolist() == [0.25, 0.25, 0.25]
    assert R.dispersions(a, 2, 7.0, 0.25).tolist() == [0.4, 0.1, 0.0] and R.dispersions(a, 3, 7.0, 0.25).tolist() == [7.0, 7.0, 7.0]
    for mode, want in (("max", [2 / 324, 0.0, 0.0]), ("common", [0.0, 0.0, 0.0]), ("feature", [2 / 324, 0.0, 0.0]), ("fixed", [0.3, 0.3, 0.3])):
        got, phi_c = R.diffexp_numpy(counts, sf, groups, mode, 0.3)
        assert got["dispersion"].tolist() == want and phi_c == (0.3 if mode == "fixed" else 0.0)
    # the parameters: s_A = s_B = 2, sigma = 2 -> r = 4 / (2 phi) = 2 / phi; equal groups -> pi_A / pi_B = 1
    k = R.constants(sf, groups)
    assert (k["n_a"], k["n_b"], k["dof"], k["mean_inv_sf"], k["s_a"], k["sig_b"]) == (2, 2, 2, 1.0, 2.0, 2.0)
    assert R.nb_params(18.0, 0.5, k) == (4.0, 4.0, 1.0) and R.nb_params(18.0, 0.0, k) == (-1.0, -1.0, 1.0)
    with pytest.raises(ValueError):
        R.diffexp_numpy(counts, sf, groups, "max", 0.0, min_mean=1000.0)
    assert R.diffexp_numpy(counts, sf, groups, "feature", 0.0, min_mean=1000.0)[1] == 0.0


def test_float_moments_against_exact_rationals():
    counts, sf, groups = R.sweep()
    m = R.moments_numpy(counts, sf, groups)
    for i in range(0, len(counts), 7):
        q, qa, qb, alpha = R.moments_exact(counts[i].tolist(), sf.tolist(), groups)
        for got, want in ((m["q"][i], q), (m["qa"][i], qa), (m["qb"][i], qb)):
            assert abs(Fraction(float(got)) - want) <= Fraction(1, 10 ** 14) * abs(want)
        # v - z cancels: the error of alpha is relative to v / q^2 + z / q^2, not to alpha
        scale = abs(alpha) + 2 * Fraction(float(np.mean(1.0 / sf))) / q if q else Fraction(1)
        assert abs(Fraction(float(m["alpha"][i])) - alpha) <= Fraction(1, 10 ** 13) * scale, i


def test_benjamini_hochberg_literal():
    p = [0.01, 0.04, -1.0, 0.03, 0.5, 0.002]
    want = [0.025, 0.05, -1.0, 0.05, 0.5, 0.01]            # m = 5: 0.002 * 5 / 1, 0.01 * 5 / 2, min(0.03 * 5 / 3, 0.04 * 5 / 4), 0.05, 0.5
    assert np.allclose(diffexp.adjust(p), want, rtol=1e-15, atol=0) and np.allclose(R.bh_plain(p), want, rtol=1e-15, atol=0)
    assert diffexp.adjust([]).tolist() == [] and diffexp.adjust([-1.0, -1.0]).tolist() == [-1.0, -1.0]
    assert diffexp.adjust([0.9, 0.8]).tolist() == [0.9, 0.9] and diffexp.adjust([0.0, 1.0]).tolist() == [0.0, 1.0]
    rs = np.random.RandomState(5)
    q = np.where(rs.uniform(size=300) < 0.1, -1.0, rs.uniform(size=300) ** 3)
    assert np.allclose(diffexp.adjust(q), R.bh_plain(q.tolist()), rtol=1e-14, atol=0)


# ---------------------------------------------------------------------------------------------------- (a) against (b), (a) against scipy
def _a_against_b(name, n, ka, ra, rb, cr):
    got = R.p_numpy(n, ka, ra, rb, cr)
    truth, near = R.p_mp(n, ka, ra, rb, cr)
    assert float(near) >= 1e-9, (name, float(near))        # no term so near the slack that two roundings could take different sides
    if truth < 1e-300:
        assert got == 0.0, (name, got)                     # the denominator overflows a double
        return 0.0
    return float(abs(got - truth) / truth)


def test_single_cases_a_against_b():
    cases = R.single_cases()
    assert all(ka + kb <= 65536 for _, ka, kb, _, _, _ in cases) and len({c[0] for c in cases}) == len(cases)
    assert sum(R.BIG[1:3]) == (1 << 20) + 3
    worst = {c[0]: _a_against_b(c[0], *R.single_params(c)) for c in cases if c[1] + c[2] > 0}
    print("worst relative error of (a) against (b):", max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) <= WORST_A_VS_B
    # what the cases are there for
    sizes = {(ka + kb + 1, kb + 1, ka) for _, ka, kb, _, _, _ in cases}
    for total in (R.C - 1, R.C, R.C + 1, 2 * R.C + 1):
        assert {(total, total, 0), (total, 1, total - 1)} <= sizes                         # k_A = 0 and k_A = n
    for side in (R.C - 1, R.C, R.C + 1):
        assert any(r == side for _, r, _ in sizes) and any(l == side for _, _, l in sizes)    # either side of k_A at C - 1, C, C + 1 terms
    assert any(ra < 1 and ra >= 0 for ra in (R.single_params(c)[2] for c in cases))


def test_sweep_a_against_b():
    counts, sf, groups = R.sweep()
    k, m = R.constants(sf, groups), R.moments_numpy(counts, sf, groups)
    worst = 0.0
    for mode in range(4):
        phi_c = 0.3 if mode == 3 else R.common_dispersion(m["q"], m["alpha"], 10.0)
        d = R.dispersions(m["alpha"], mode, 0.3, phi_c)
        for i in sorted(set(range(0, len(d), 10)) | {WORST_FEATURE}):
            ka, kb = int(m["ka"][i]), int(m["kb"][i])
            if ka + kb:
                worst = max(worst, _a_against_b("%d/%d" % (mode, i), ka + kb, ka, *R.nb_params(m["q"][i], d[i], k)))
    print("worst relative error of (a) against (b) on the sweep:", worst)
    assert 0.9 * WORST_A_VS_B <= worst <= WORST_A_VS_B                 # the bound is the measured error, not a loose one


def test_poisson_case_is_the_exact_binomial_test():
    stats = pytest.importorskip("scipy.stats")
    for n, ka, sa, sb in ((50, 17, 1.0, 1.0), (50, 25, 1.0, 1.0), (1000, 430, 1.0, 1.2), (1000, 0, 0.01, 1.0), (20000, 9700, 1.0, 1.05), (7, 7, 2.0, 1.0)):
        _, _, ra, rb, cr = R.single_params(("", ka, n - ka, sa, sb, 0.0))
        want = stats.binomtest(ka, n, sa / (sa + sb)).pvalue
        assert abs(R.p_numpy(n, ka, ra, rb, cr) - want) <= 1e-12 * want, (n, ka)


# ---------------------------------------------------------------------------------------------------- the matrix reader and the files
def test_read_matrix_and_refused_lines(tmp_path):
    path = tmp_path / "m.counts.tsv"
    path.write_bytes(b"name\ts1\ts2\tskip\ts3\r\nf1\t1\t2\tx\t3\r\nf 2\t0\t10\t\t1099511627775\n")
    names, counts = diffexp.read_matrix(str(path), ["s3"], ["s1", "s2"])
    assert names == ["f1", "f 2"] and counts.dtype == np.uint64 and counts.tolist() == [[3, 1, 2], [1099511627775, 0, 10]]
    head = "name\ts1\ts2\n"
    for text, line, why in ((head + "f1\t1\n", 2, "2 columns where the header has 3"), (head + "f1\t1\t2\t3\n", 2, "4 columns"),
                            (head + "f1\t1\t2\nf2\t1\tx\n", 3, "x is not a non-negative whole number"), (head + "f1\t-1\t2\n", 2, "-1 is not"),
                            (head + "f1\t1.5\t2\n", 2, "1.5 is not"), (head + "f1\t\t2\n", 2, "an empty field is not"),
                            (head + "f1\t1e3\t2\n", 2, "1e3 is not"), (head + "f1\t1\t2\nf2\t3\t4\nf1\t5\t6\n", 4, "the feature name f1 occurs twice"),
                            ("name\ts1\ts2\ts1\nf1\t1\t2\t3\n", 1, "the column name s1 occurs twice"), (head + "f1\t1\t1099511627776\n", 2, "2^40 or more"),
                            (head + "f1\t1\t2\n\n", 3, "1 columns where the header has 3"), ("", 1, "no header"), ("name\n", 1, "at least one sample"),
                            ("name\ts1\ts3\nf1\t1\t2\n", 1, "there is no column s2")):
        path.write_text(text)
        with pytest.raises(ValueError) as e:
            diffexp.read_matrix(str(path), ["s1"], ["s2"])
        assert str(e.value).startswith("%s line %d: " % (path, line)) and why in str(e.value), (text, str(e.value))
    fac = tmp_path / "f.tsv"
    fac.write_text("s2\t2.5\n\ns1\t0.5\nother\t1\n")
    assert diffexp.read_size_factors(str(fac), ["s1", "s2"]).tolist() == [0.5, 2.5]
    for text, why in (("s1\t0\ns2\t1\n", "line 1"), ("s1\t1\ns2\tx\n", "line 2"), ("s1\t1\ns1\t1\n", "occurs twice"), ("s1\t1\n", "no size factor for the sample s2"),
                      ("s1\t1\t3\ns2\t1\n", "line 1"), ("s1\tinf\ns2\t1\n", "line 1"), ("s1\tnan\ns2\t1\n", "line 1")):
        fac.write_text(text)
        with pytest.raises(ValueError) as e:
            diffexp.read_size_factors(str(fac), ["s1", "s2"])
        assert why in str(e.value), (text, str(e.value))


def test_worked_files():
    rows = np.zeros(3, capi.DIFFEXP_DTYPE)
    rows["base_mean"], rows["mean_a"], rows["mean_b"] = [2.0, 0.0, 1234567.0], [1.0, 0.0, 1000000.25], [3.0, 0.0, 1469133.75]
    rows["log2fc"], rows["dispersion"], rows["p"] = [math.log2(3.5 / 1.5), 0.0, 0.5], [0.0, 0.1, 1 / 3], [0.625, -1.0, 1.5e-300]
    counts = np.array([[1, 3], [0, 0], [7, 9]], dtype=np.uint64)
    tsv, norm, fac = diffexp.format_files(["a", "b b", "c"], counts, ["s1", "s2"], 1, np.array([0.5, 2.0]), rows, diffexp.adjust(rows["p"]))
    assert tsv == (b"name\tbaseMean\tmeanA\tmeanB\tlog2fc\tdispersion\tp\tpadj\n"
                   b"a\t2\t1\t3\t1.22239\t0\t6.250e-01\t6.250e-01\n"
                   b"b b\t0\t0\t0\t0\t0.1\tNA\tNA\n"
                   b"c\t1.23457e+06\t1e+06\t1.46913e+06\t0.5\t0.333333\t1.500e-300\t3.000e-300\n")
    assert norm == b"name\ts1\ts2\na\t2.000\t1.500\nb b\t0.000\t0.000\nc\t14.000\t4.500\n"
    assert fac == b"sample\tgroup\tcolumn_sum\tsize_factor\ns1\tA\t8\t0.5\ns2\tB\t12\t2\n"
    assert diffexp.output_paths("x") == ["x.tsv", "x.norm.tsv", "x.factors.tsv"]
    assert diffexp.output_base(None, "d/study.counts.tsv") == "d/study.diffexp" and diffexp.output_base(None, "m.txt") == "m.txt.diffexp"
    assert diffexp.output_base("o.tsv", "m") == "o" and diffexp.output_base("o", "m") == "o"


# ---------------------------------------------------------------------------------------------------- the ABI
def test_abi_entries_are_declared(tmp_path):
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_diffexp(", "MirpDiffexpOpts", "MirpDiffexpRow", "MIRP_DIFFEXP_CHUNK", "MIRP_DIFFEXP_MAX_FEATURES", "MIRP_DIFFEXP_MAX_COUNT"):
        assert name in header
    assert capi.ABI_VERSION == 17

    def define(name):
        return int(re.search(r"#define %s\s+(\d+)" % name, header).group(1))
    assert define("MIRP_DIFFEXP_CHUNK") == capi.DIFFEXP_CHUNK == R.C and capi.DIFFEXP_CHUNK % 64 == 0
    assert define("MIRP_DIFFEXP_MAX_FEATURES") == capi.DIFFEXP_MAX_FEATURES == diffexp.MAX_FEATURES == 1 << 24
    assert define("MIRP_DIFFEXP_MAX_COUNT") == capi.DIFFEXP_MAX_COUNT == diffexp.MAX_COUNT == 1 << 40
    assert define("MIRP_MAX_SAMPLES") == diffexp.MAX_SAMPLES and capi.DIFFEXP_MODES == R.MODES and capi.DIFFEXP_MODES[:3] == diffexp.MODES
    assert len(capi.DIFFEXP_STATS) == 5
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the struct layout with")
    of = ["size_factor", "group", "n_samples", "mode", "phi", "min_mean", "pseudo"]
    rf = ["base_mean", "mean_a", "mean_b", "log2fc", "dispersion", "p", "k_a", "k_b"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirprefer.h"\nint main(void) {\n'
                   ' printf("%zu %zu", sizeof(MirpDiffexpOpts), sizeof(MirpDiffexpRow));\n' +
                   "".join(' printf(" %%zu", offsetof(MirpDiffexpOpts, %s));\n' % f for f in of) +
                   "".join(' printf(" %%zu", offsetof(MirpDiffexpRow, %s));\n' % f for f in rf) + ' printf("\\n");\n return 0;\n}\n')
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got[:2] == [ctypes.sizeof(capi.DiffexpOpts), capi.DIFFEXP_DTYPE.itemsize] == [48, 64]
    assert got[2:9] == [getattr(capi.DiffexpOpts, f).offset for f in of] and [f for f, _ in capi.DiffexpOpts._fields_] == of
    assert got[9:] == [capi.DIFFEXP_DTYPE.fields[f][1] for f in rf] and list(capi.DIFFEXP_DTYPE.names) == rf


def test_the_library_exports_the_symbol():
    lib = capi.load_library()
    assert lib.mirp_diffexp.restype is ctypes.c_int and lib.mirp_abi_version() == 17
    # arguments are checked before a device is touched: a null context is refused
    assert lib.mirp_diffexp(None, None, 0, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "mir-prefer_amd", "csrc", "diffexp_kernels.hip"),
           "-o", str(tmp_path / "diffexp_kernels.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    report, name = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    # 128 VGPRs keep the 4 waves per SIMD (16 per CU) that the capped grid of the wave-per-job kernels asks for
    for kernel in ("de_prep_kernel", "de_param_kernel", "de_chunk_kernel", "de_start_kernel", "de_sum_kernel", "de_reduce_kernel"):
        mine = [v for k, v in report.items() if kernel in k]
        assert len(mine) == 1 and mine[0]["ScratchSize"] == 0 and mine[0]["VGPRs"] <= 128, (kernel, mine)


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.diffexp"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))


def test_option_errors_exit_2_before_a_device(tmp_path, capsys):
    m = tmp_path / "study.counts.tsv"
    m.write_text("name\tr1\tr2\tl1\nf\t1\t2\t3\n")
    s = str(m)
    many = ",".join("c%d" % i for i in range(200))
    bad = [[], ["-a", "r1", "-b", "l1", "--dispersion", "0"], ["-a", "r1", s], ["-b", "l1", s], ["-a", "r1,,r2", "-b", "l1", s], ["-a", "", "-b", "l1", s],
           ["-a", "r1,r1", "-b", "l1", s], ["-a", "r1,r2", "-b", "r2,l1", s], ["-a", "r1", "-b", "l1", s], ["-a", "r1", "-b", "l1", "--dispersion", "common", s],
           ["-a", "r1,r2", "-b", "l1", "--dispersion", "-0.1", s], ["-a", "r1,r2", "-b", "l1", "--dispersion", "nan", s],
           ["-a", "r1,r2", "-b", "l1", "--dispersion", "trend", s], ["-a", "r1,r2", "-b", "l1", "--norm", "tmm", s],
           ["-a", "r1,r2", "-b", "l1", "--min-mean", "-1", s], ["-a", "r1,r2", "-b", "l1", "--min-mean", "x", s], ["-a", "r1,r2", "-b", "l1", "--pseudo", "-1", s],
           ["-a", "r1,r2", "-b", "l1", "--pseudo", "inf", s], ["-a", "r1,r2", "-b", "l1", "--device", "-1", s], ["-a", "r1,r2", "-b", "l1", "-o", "", s],
           ["-a", "r1,r2", "-b", "l1", "--size-factors", "", s], ["-a", "r1,r2", "-b", "l1", s, s], ["-a", many, "-b", many.replace("c", "d"), s],
           ["-a", "r1,r2", "-b", "l1", "-x", s]]
    for args in bad:
        with pytest.raises(SystemExit) as e:
            diffexp.parse_args(args)
        assert e.value.code == 2, args
    assert "give --dispersion a number" in capsys.readouterr().err
    for args in (bad[0], bad[7], bad[8], bad[13]):
        r = run_cli(args, tmp_path)
        assert r.returncode == 2 and b"Error: " not in r.stderr, (args, r.stderr)
    assert list(tmp_path.glob("*.tsv")) == [m]
    o, matrix, a, b, disp, base = diffexp.parse_args(["-a", "r1,r2", "-a", "r3", "-b", "l1", s])
    assert (matrix, a, b, disp, base) == (s, ["r1", "r2", "r3"], ["l1"], (0, 0.0), str(tmp_path / "study.diffexp"))
    assert (o.norm, o.min_mean, o.pseudo, o.device, o.size_factors) == ("mor", 10.0, 0.5, 0, None)
    assert diffexp.parse_args(["-a", "r1", "-b", "l1", "--dispersion", "0", s])[4] == (3, 0.0)
    assert diffexp.parse_args(["-a", "r1", "-b", "l1", "--dispersion", "2.5e-1", "-o", "x/out.tsv", s])[4:] == ((3, 0.25), "x/out")
    assert [diffexp.parse_args(["-a", "r1,r2", "-b", "l1", "--dispersion", d, s])[4][0] for d in ("max", "common", "feature")] == [0, 1, 2]
    with pytest.raises(SystemExit) as e:
        diffexp.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--group-a", "--group-b", "--output", "--norm", "--size-factors", "--dispersion", "--min-mean", "--pseudo", "--device"):
        assert opt in text


def test_missing_and_refused_inputs_exit_255_and_leave_no_output(tmp_path):
    m, fac = tmp_path / "study.counts.tsv", tmp_path / "f.tsv"
    fac.write_text("r1\t1\nr2\t1\n")
    stale = diffexp.output_paths(str(tmp_path / "study.diffexp"))
    ab = ["-a", "r1,r2", "-b", "l1"]
    for text, args, why in (("name\tr1\tr2\tl1\nf\t1\t2\t3\n", ab + [str(tmp_path / "nope.counts.tsv")], "nope.counts.tsv does not exist"),
                            ("name\tr1\tr2\tl1\nf\t1\t2\t3\n", ab + ["--size-factors", str(tmp_path / "nope.tsv"), str(m)], "nope.tsv does not exist"),
                            ("name\tr1\tr2\tl1\nf\t1\t2\t3\ng\t1\t2\n", ab + [str(m)], "study.counts.tsv line 3: 3 columns where the header has 4"),
                            ("name\tr1\tr2\tl1\nf\t1\t2\t3\ng\t1\tzwei\t3\n", ab + [str(m)], "study.counts.tsv line 3: zwei is not"),
                            ("name\tr1\tr2\tl1\nf\t1\t2\t3\nf\t1\t2\t3\n", ab + [str(m)], "study.counts.tsv line 3: the feature name f occurs twice"),
                            ("name\tr1\tr2\tr1\nf\t1\t2\t3\n", ab + [str(m)], "study.counts.tsv line 1: the column name r1 occurs twice"),
                            ("name\tr1\tr2\tl2\nf\t1\t2\t3\n", ab + [str(m)], "study.counts.tsv line 1: there is no column l1"),
                            ("name\tr1\tr2\tl1\nf\t1\t0\t3\n", ab + [str(m)], "--norm total"),
                            ("name\tr1\tr2\tl1\nf\t1\t0\t3\n", ab + ["--norm", "total", str(m)], "no read at all"),
                            ("name\tr1\tr2\tl1\nf\t1\t2\t3\n", ab + ["--size-factors", str(fac), str(m)], "no size factor for the sample l1")):
        m.write_text(text)
        for p in stale:
            open(p, "w").write("stale\n")
        r = run_cli(args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (args, r.stderr)
        if "does not exist" not in why:
            assert not any(os.path.exists(p) for p in stale)
    probe = ("import sys\nfrom mir_prefer_amd import diffexp\nrc = diffexp.main(['-a', 'r1,r2', '-b', 'l1', %r])\n"
             "print(rc, 'mir_prefer_amd.capi' in sys.modules)\n" % str(m))
    m.write_text("name\tr1\tr2\tl1\nf\t1\t2\n")
    r = subprocess.run([sys.executable, "-c", probe], cwd=str(tmp_path), capture_output=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
    assert r.stdout.split() == [b"255", b"False"], (r.stdout, r.stderr)            # a refused matrix never loads the library
