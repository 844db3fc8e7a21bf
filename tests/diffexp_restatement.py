"""The definition of DESIGN.md §32 (differential expression between two groups) twice, and the inputs that the CPU and the GPU tests share.

(a) numpy float64.  The moments and the parameters of the test are written in the device's order of operations (sums over the samples in column
    order, the same products and quotients), so they are the device's doubles bit for bit wherever the device uses no fused multiply-add.  The
    test itself carries ln u outwards from the observed split k_A with `cumsum` of ln rho and adds the terms with numpy's pairwise sum.
(b) exact rational moments (fractions) and the test in mpmath at 60 digits by the same recurrence on u itself, u(a + 1) = u(a) rho(a): the truth.
    It takes the parameters r_A, r_B and pi_A / pi_B as the doubles of (a), so the difference between (a) and (b) is the error of summing in
    doubles, not of the parameters.

The test conditions on n = k_A + k_B.  With rho(a) = t(a + 1) / t(a) = (n - a) / (a + 1) * (a + r_A) / (n - a - 1 + r_B) * pi_A / pi_B (the second
factor is 1 in the Poisson case), u(k_A) = 1, D = the sum of u over a = 0 .. n, N = the sum of the u <= 1 + 1e-7, p = N / D; 0 where D overflows."""
import math
from fractions import Fraction

import numpy as np

SLACK = 1.0 + 1e-7
C = 4096                     # capi.DIFFEXP_CHUNK
MODES = ("max", "common", "feature", "fixed")


# ---------------------------------------------------------------------------------------------------- host rules
def size_factors_plain(counts, norm):
    """The size factors in plain Python: counts a list of rows of whole numbers (used samples only)."""
    S = len(counts[0])
    if norm == "none":
        return [1.0] * S
    if norm == "total":
        tot = [sum(r[j] for r in counts) for j in range(S)]
        if min(tot) == 0:
            raise ValueError("zero column")
        g = math.exp(sum(math.log(t) for t in tot) / S)
        return [t / g for t in tot]
    rows = [r for r in counts if min(r) > 0]
    if not rows:
        raise ValueError("no usable feature")
    out = []
    logs = [[math.log(k) for k in r] for r in rows]
    means = [sum(l) / S for l in logs]
    for j in range(S):
        d = sorted(l[j] - m for l, m in zip(logs, means))
        h = len(d) // 2
        out.append(math.exp(d[h] if len(d) % 2 else (d[h - 1] + d[h]) / 2))
    return out


def bh_plain(p):
    """Benjamini-Hochberg over the entries >= 0 (the tested features); -1 stays -1."""
    idx = sorted((i for i in range(len(p)) if p[i] >= 0), key=lambda i: p[i])
    m = len(idx)
    out = [-1.0] * len(p)
    best = 1.0
    for rank in range(m, 0, -1):
        i = idx[rank - 1]
        best = min(best, p[i] * m / rank)
        out[i] = best
    return out


# ---------------------------------------------------------------------------------------------------- constants, moments, parameters (device order)
def constants(sf, groups):
    """What the host sums in sample order: n_a, n_b, dof, mean of 1 / s, s_A, s_B, sigma_A, sigma_B."""
    k = dict(n_a=0, n_b=0, s_a=0.0, s_b=0.0, sig_a=0.0, sig_b=0.0)
    inv = 0.0
    for s, g in zip(np.asarray(sf, dtype=np.float64).tolist(), groups):
        inv += 1.0 / s
        x = "b" if g else "a"
        k["n_" + x] += 1
        k["s_" + x] += s
        k["sig_" + x] += s * s
    k["mean_inv_sf"] = inv / len(groups)
    k["dof"] = (k["n_a"] - 1 if k["n_a"] >= 2 else 0) + (k["n_b"] - 1 if k["n_b"] >= 2 else 0)
    return k


def moments_numpy(counts, sf, groups):
    """-> dict of float64 / uint64 arrays: q, qa, qb, alpha (the raw dispersion), ka, kb; the sums run over the columns in order, as on the device."""
    counts = np.asarray(counts, dtype=np.uint64).reshape(-1, len(groups))
    sf = np.asarray(sf, dtype=np.float64)
    k = constants(sf, groups)
    F, S = counts.shape
    y = counts.astype(np.float64) / sf
    tot, sa, sb = np.zeros(F), np.zeros(F), np.zeros(F)
    ka, kb = np.zeros(F, dtype=np.uint64), np.zeros(F, dtype=np.uint64)
    for j in range(S):
        tot = tot + y[:, j]
        if groups[j]:
            sb, kb = sb + y[:, j], kb + counts[:, j]
        else:
            sa, ka = sa + y[:, j], ka + counts[:, j]
    q, qa, qb = tot / float(S), sa / float(k["n_a"]), sb / float(k["n_b"])
    ss = np.zeros(F)
    for j in range(S):
        if (k["n_b"] if groups[j] else k["n_a"]) < 2:
            continue
        d = y[:, j] - (qb if groups[j] else qa)
        ss = ss + d * d
    alpha = np.zeros(F)
    if k["dof"] > 0:
        pos = q > 0
        v, z = ss[pos] / float(k["dof"]), q[pos] * k["mean_inv_sf"]
        alpha[pos] = (v - z) / (q[pos] * q[pos])
    return dict(q=q, qa=qa, qb=qb, alpha=alpha, ka=ka, kb=kb)


def moments_exact(row, sf, groups):
    """One feature in exact rationals of the given doubles -> (q, qa, qb, alpha) as Fractions."""
    S = len(groups)
    y = [Fraction(int(c)) / Fraction(float(s)) for c, s in zip(row, sf)]
    ia, ib = [j for j in range(S) if not groups[j]], [j for j in range(S) if groups[j]]
    q, qa, qb = sum(y) / S, sum(y[j] for j in ia) / len(ia), sum(y[j] for j in ib) / len(ib)
    dof = sum(len(g) - 1 for g in (ia, ib) if len(g) >= 2)
    if q == 0 or dof == 0:
        return q, qa, qb, Fraction(0)
    ss = sum((y[j] - m) ** 2 for g, m in ((ia, qa), (ib, qb)) if len(g) >= 2 for j in g)
    z = q * sum(1 / Fraction(float(s)) for s in sf) / S
    return q, qa, qb, (ss / dof - z) / (q * q)


def common_dispersion(q, alpha, min_mean):
    """max(0, the median raw dispersion of the features with q >= min_mean); None without such a feature."""
    keep = np.sort(np.asarray(alpha)[np.asarray(q) >= min_mean])
    if len(keep) == 0:
        return None
    h = len(keep) // 2
    return max(0.0, float(keep[h]) if len(keep) % 2 else float((keep[h - 1] + keep[h]) / 2.0))


def dispersions(alpha, mode, phi, phi_c):
    alpha = np.asarray(alpha, dtype=np.float64)
    if mode == 0:
        return np.where(alpha > phi_c, alpha, phi_c)
    if mode == 1:
        return np.full(len(alpha), float(phi_c))
    if mode == 2:
        return np.where(alpha > 0.0, alpha, 0.0)
    return np.full(len(alpha), float(phi))


def nb_params(q, d, k):
    """One feature: base mean q, dispersion d, constants k -> (r_A, r_B, pi_A / pi_B); r < 0 marks the Poisson case."""
    q, d = float(q), float(d)
    if not (d > 0.0 and q > 0.0):                      # q = 0: a feature without reads, which is not tested
        return -1.0, -1.0, k["s_a"] / k["s_b"]
    mu_a, mu_b = q * k["s_a"], q * k["s_b"]
    ra = (k["s_a"] * k["s_a"]) / (d * k["sig_a"])
    rb = (k["s_b"] * k["s_b"]) / (d * k["sig_b"])
    return ra, rb, (mu_a / (ra + mu_a)) / (mu_b / (rb + mu_b))


# ---------------------------------------------------------------------------------------------------- the test
def lnrho(n, ra, rb, cr, a):
    """ln rho(a) for an int64 array a, 0 <= a < n, in the device's order of operations."""
    x, m = a.astype(np.float64), (n - a).astype(np.float64)
    ratio = m / (x + 1.0)
    if ra >= 0.0:
        ratio = ratio * ((x + ra) / ((m - 1.0) + rb))
    return np.log(ratio * cr)


def p_numpy(n, ka, ra, rb, cr):
    """(a): p of one feature; -1.0 for n = 0."""
    n, ka = int(n), int(ka)
    if n == 0:
        return -1.0
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        right = np.cumsum(lnrho(n, ra, rb, cr, np.arange(ka, n, dtype=np.int64)))               # ln u(ka + 1 .. n)
        left = np.cumsum(-lnrho(n, ra, rb, cr, np.arange(ka - 1, -1, -1, dtype=np.int64)))       # ln u(ka - 1 .. 0)
        u = np.exp(np.concatenate([[0.0], right, left]))
        D = float(np.sum(u))
        N = float(np.sum(u[u <= SLACK]))
    return 0.0 if math.isinf(D) else N / D


def p_mp(n, ka, ra, rb, cr, dps=60):
    """(b): (p as an mpf, the smallest |u / (1 + 1e-7) - 1| over the terms other than k_A) of one feature with the parameters taken as exact doubles."""
    import mpmath
    n, ka = int(n), int(ka)
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        A, B, Cr, slack = mpf(ra), mpf(rb), mpf(cr), mpf(1) + mpf(10) ** -7

        def rho(a):
            r = mpf(n - a) / (a + 1) * Cr
            return r * (a + A) / (n - a - 1 + B) if ra >= 0.0 else r
        N = D = mpf(1)
        near = mpf(1)                                 # k_A itself is 1e-7 away
        for lo, hi, step in ((ka, n, 1), (ka - 1, -1, -1)):
            u = mpf(1)
            for a in range(lo, hi, step):
                u = u * rho(a) if step == 1 else u / rho(a)
                D += u
                if u <= slack:
                    N += u
                near = min(near, abs(u / slack - 1))
        return N / D, near


def diffexp_numpy(counts, sf, groups, mode, phi=0.0, min_mean=10.0, pseudo=0.5):
    """(a) end to end: -> (dict of arrays base_mean, mean_a, mean_b, log2fc, dispersion, p, k_a, k_b, alpha, the common dispersion or phi)."""
    if isinstance(mode, str):
        mode = MODES.index(mode)
    m = moments_numpy(counts, sf, groups)
    k = constants(sf, groups)
    phi_c = float(phi) if mode == 3 else common_dispersion(m["q"], m["alpha"], min_mean)
    if phi_c is None:
        if mode != 2:
            raise ValueError("no feature with a mean of min_mean or more")
        phi_c = 0.0
    d = dispersions(m["alpha"], mode, phi, phi_c)
    p = np.empty(len(d))
    for i in range(len(d)):
        ka, kb = int(m["ka"][i]), int(m["kb"][i])
        p[i] = p_numpy(ka + kb, ka, *nb_params(m["q"][i], d[i], k))
    with np.errstate(divide="ignore", invalid="ignore"):
        fc = np.log2((m["qb"] + pseudo) / (m["qa"] + pseudo))
    return dict(base_mean=m["q"], mean_a=m["qa"], mean_b=m["qb"], log2fc=fc, dispersion=d, p=p, k_a=m["ka"], k_b=m["kb"], alpha=m["alpha"]), phi_c


# ---------------------------------------------------------------------------------------------------- shared inputs
def _sf_near(ka, kb):
    """Size factors that put the observed split about two standard deviations from the expected one, so that p is neither 1 nor 0."""
    return float(ka + 2.0 * math.sqrt(ka + 1.0) + 1.0), float(kb + 1.0)


def single_cases():
    """One sample per group and a fixed dispersion: (name, k_A, k_B, s_A, s_B, phi).  Then r_A = r_B = 1 / phi.  The chunks of the device run outwards
    from k_A (right: n - k_A + 1 terms, left: k_A terms), so the sizes around C are set on either side as well as on n + 1."""
    out = [("n0", 0, 0, 1.0, 1.0, 0.1), ("n1a", 1, 0, 1.0, 1.0, 0.1), ("n1b", 0, 1, 1.0, 2.0, 0.0), ("n2", 1, 1, 1.5, 1.0, 0.3),
           ("n2a", 2, 0, 1.0, 1.0, 0.0), ("ka0", 0, 500, 0.02, 1.0, 0.1), ("kan", 500, 0, 1.0, 0.02, 0.1),
           ("mode", 500, 500, 1.0, 1.0, 0.05), ("mirror_nb", 30, 70, 1.0, 1.0, 0.2), ("mirror_pois", 3, 7, 1.0, 1.0, 0.0),
           ("mirror_far", 4000, 4300, 2.0, 2.0, 0.0), ("pois", 180, 260, 1.0, 1.25, 0.0), ("pois_big", 30000, 31000, 1.0, 1.02, 0.0),
           ("r_small", 40, 90, 1.0, 1.0, 5.0), ("r_small0", 0, 300, 1.0, 1.0, 8.0), ("r_small_big", 9000, 200, 1.0, 1.0, 3.0),
           ("overflow", 0, 5000, 1.0, 1.0, 0.0), ("overflow_nb", 60000, 5, 1.0, 1.0, 1e-4), ("tiny_p", 100, 900, 1.0, 1.0, 0.0),
           ("nb_60000", 27000, 33000, 1.0, 1.1, 0.02)]
    for n in (C - 2, C - 1, C, 2 * C):                                   # n + 1 = C - 1, C, C + 1, 2C + 1
        kas = {0, n, C - 1, C, C + 1, n - C + 2, n - C + 1, n - C}       # first / last term of a chunk, either side at C - 1, C, C + 1 terms
        for ka in sorted(x for x in kas if 0 <= x <= n):
            sa, sb = _sf_near(ka, n - ka)
            out.append(("n%d_ka%d" % (n, ka), ka, n - ka, sa, sb, 0.0 if (n + ka) % 3 == 0 else 0.04))
    return out


BIG = ("big", 500000, 548579, 1.0, 1.0, 0.01)      # n = 2^20 + 3: one feature spread over the grid (mpmath: profiles/tools/diffexp_error.py)


def single_params(case):
    """A case of single_cases -> (n, k_A, r_A, r_B, pi_A / pi_B), by way of the moments as the device takes it."""
    _, ka, kb, sa, sb, phi = case
    m = moments_numpy([[ka, kb]], [sa, sb], [0, 1])
    return (ka + kb, ka) + nb_params(m["q"][0], phi, constants([sa, sb], [0, 1]))


def sweep(seed=20, features=2000):
    """Seeded negative-binomial counts of `features` features x (3 + 3) samples: -> (uint64 counts, size factors of --norm mor, groups)."""
    rs = np.random.RandomState(seed)
    mu = np.clip(np.exp(rs.normal(3.2, 1.6, features)), 0.05, 2500.0)
    phi = 0.05 + 1.0 / np.sqrt(mu + 1.0) * rs.uniform(0.2, 1.0, features)
    fold = np.where(rs.uniform(size=features) < 0.15, np.exp(rs.normal(0.0, 1.0, features)), 1.0)
    depth = np.array([0.7, 1.0, 1.3, 0.9, 1.1, 1.4])
    groups = [0, 0, 0, 1, 1, 1]
    mean = mu[:, None] * depth[None, :] * np.where(np.array(groups)[None, :] == 1, fold[:, None], 1.0)
    size = (1.0 / phi)[:, None]
    counts = rs.negative_binomial(size, size / (size + mean)).astype(np.uint64)
    ok = (counts > 0).all(axis=1)
    ln = np.log(counts[ok].astype(np.float64))
    sf = np.exp(np.median(ln - ln.mean(axis=1, keepdims=True), axis=0))
    return counts, sf, groups
