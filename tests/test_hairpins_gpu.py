"""GPU tests of the known-hairpin comparison (mirp_hairpin_align, mir_prefer_amd.hairpins).  Every comparison is exact equality
with the restatement of test_hairpins_cpu.py: hit records, cigars, hit counts per query and the bytes of both files."""
import os
import random
import subprocess
import sys

import pytest

from tests.test_hairpins_cpu import DEFAULT, as_records, hits_text, random_seq, restate, summary_text
from tests.test_targets_cpu import ROOT

pytestmark = pytest.mark.gpu

SETTINGS = (DEFAULT, (1, 2, 0, 1), (3, 4, 8, 2))


def cut(hits, per_query, k):
    """the restated hits after -k"""
    if k == 0:
        return hits
    out, seen = [], {}
    for h in hits:
        seen[h["query"]] = seen.get(h["query"], 0) + 1
        if seen[h["query"]] <= k:
            out.append(h)
    return out


def run(ctx, queries, known, par=DEFAULT, min_score=60, max_lines=0, capacity=0):
    recs, cigars = ctx.hairpin_align(queries, known, match=par[0], mismatch=par[1], gap_open=par[2], gap_extend=par[3], min_score=min_score,
                                     max_lines=max_lines, capacity=capacity)
    assert not recs["reserved"].any()
    return [tuple(r) for r in recs.tolist()], cigars, ctx.hairpin_last_stats()


def check(ctx, queries, known, par=DEFAULT, min_score=60, max_lines=0, capacity=0, want=None):
    hits, per_query = want if want is not None else restate(queries, known, par, min_score)
    recs, cigars, stats = run(ctx, queries, known, par, min_score, max_lines, capacity)
    w_recs, w_cigars = as_records(cut(hits, per_query, max_lines))
    assert len(recs) == len(w_recs)
    for got, gc, exp, ec in zip(recs, cigars, w_recs, w_cigars):
        assert got == exp and gc == ec, (got, gc, exp, ec)
    assert stats["per_query"] == per_query and stats["hits"] == sum(per_query)
    assert (stats["queries"], stats["known"], stats["pairs"]) == (len(queries), len(known), len(queries) * len(known))
    assert stats["cells"] == sum(len(q) for q in queries) * sum(len(k) for k in known)
    return recs, cigars, stats


def test_pins_on_the_device(gpu_ctx):
    recs, cigars, _ = run(gpu_ctx, ["ACGUACGUACGU"], ["ACGU"], min_score=1)
    assert recs == [(0, 0, 8, 1, 4, 1, 4, 4, 0, 0, 0, 0)] and cigars == ["4="]
    recs, cigars, _ = run(gpu_ctx, ["GGGAAACCC"], ["GGGCCC"], (2, 3, 0, 1), min_score=1)
    assert recs == [(0, 0, 9, 1, 9, 1, 6, 6, 0, 1, 3, 0)] and cigars == ["3=3I3="]
    assert run(gpu_ctx, ["NNNN", "acgt"], ["NNNN", "ACGU"], min_score=1)[:2] == ([(1, 1, 8, 1, 4, 1, 4, 4, 0, 0, 0, 0)], ["4="])
    assert run(gpu_ctx, [], ["ACGU"])[0] == [] and run(gpu_ctx, ["ACGU"], [])[0] == []


def test_lengths(gpu_ctx):
    from mir_prefer_amd import capi
    R = capi.HAIRPIN_STRIP
    rng = random.Random(251)
    k_lens = [1, 2, R - 1, R, R + 1, 63, 64, 65, 100]
    queries = [random_seq(rng, n, "ACG") for n in range(1, 2 * R + 3)]
    known = [random_seq(rng, n, "ACG") for n in k_lens]
    _, _, stats = check(gpu_ctx, queries, known, min_score=1)
    assert stats["hits"] > 250
    few = [queries[0], queries[R], queries[2 * R + 1]]
    for count in (1, 63, 64, 65, 129):
        check(gpu_ctx, few, [random_seq(rng, k_lens[x % len(k_lens)], "ACG") for x in range(count)], min_score=1)
    # one wave that holds lengths 1 and 300 together, in either order of the file
    mixed = [random_seq(rng, 1 if x % 2 else 300, "ACG") for x in range(64)]
    check(gpu_ctx, few + [random_seq(rng, 40, "ACG")], mixed, min_score=1)


def mixture(seed, n_q=40, n_k=600, q_len=(60, 300), k_len=(40, 400)):
    rng = random.Random(seed)
    queries = [random_seq(rng, rng.randint(*q_len)) for _ in range(n_q)]
    known = []
    for x in range(n_k):
        L = rng.randint(*k_len)
        if x % 5:
            known.append(random_seq(rng, L))
            continue
        q = rng.choice(queries)
        kind = (x // 5) % 5
        if kind == 0:          # substitutions
            s = list(q)
            for _ in range(rng.randint(1, len(q) // 8)):
                s[rng.randrange(len(s))] = rng.choice("ACGU")
            s = "".join(s)
        elif kind == 1:        # 1 to 3 indels of 1..6 bases
            s = q
            for _ in range(rng.randint(1, 3)):
                at, g = rng.randrange(1, len(s) - 7), rng.randint(1, 6)
                s = s[:at] + (random_seq(rng, g) if rng.random() < 0.5 else "") + s[at + (0 if rng.random() < 0.5 else g):]
        elif kind == 2:        # a shared 21-mer only
            at = rng.randrange(len(q) - 21)
            body = random_seq(rng, max(L, 30))
            cut_at = rng.randrange(len(body) - 21)
            s = body[:cut_at] + q[at:at + 21] + body[cut_at + 21:]
        elif kind == 3:        # an exact copy
            s = q
        else:                  # a copy extended on both sides
            s = random_seq(rng, rng.randint(1, 40)) + q + random_seq(rng, rng.randint(1, 40))
        known.append(s[:400])

    def sprinkle(s):
        s = list(s)
        for p in range(len(s)):
            r = rng.random()
            if r < 0.01:
                s[p] = "N"
            elif r < 0.05:
                s[p] = s[p].lower()
            elif r < 0.10 and s[p] == "U":
                s[p] = "T"
        return "".join(s)
    return [sprinkle(q) for q in queries], [sprinkle(k) for k in known]


@pytest.fixture(scope="module")
def mixtures():
    queries, known = mixture(2501)
    cache = {}

    def get(par):
        if par not in cache:
            cache[par] = restate(queries, known, par, 60)
        return cache[par]
    return queries, known, get


@pytest.mark.parametrize("par", SETTINGS)
def test_seeded_mixtures(gpu_ctx, mixtures, par):
    queries, known, get = mixtures
    want = get(par)
    assert sum(want[1]) >= 60 and any(h["gap_opens"] for h in want[0]) and any(h["mismatches"] for h in want[0])
    for k in (0, 1, 3):
        check(gpu_ctx, queries, known, par, 60, max_lines=k, want=want)


def test_ties(gpu_ctx):
    queries = ["A" * 50, "AC" * 30, "GGGAAACCC", "GGGCCC", "ACGU" * 3, "AAAACGGGG", "A" * 20]
    known = ["A" * 20, "AC" * 10, "GGGCCC", "GGGAAACCC", "ACGU", "AAAAUGGGG", "A" * 50, "CCCAAAGGG"]
    for par in ((2, 3, 0, 1), (4, 2, 0, 1), (4, 5, 0, 1), DEFAULT, (1, 1, 1, 1)):
        recs, cigars, _ = check(gpu_ctx, queries, known, par, min_score=1)
    by = {(r[0], r[1]): (r, c) for r, c in zip(*run(gpu_ctx, queries, known, (2, 3, 0, 1), min_score=1)[:2])}
    assert by[(0, 0)][0][3:7] == (1, 20, 1, 20) and by[(1, 1)][0][3:7] == (1, 20, 1, 20) and by[(4, 4)][0][3:7] == (1, 4, 1, 4)
    assert by[(2, 2)][1] == "3=3I3=" and by[(3, 3)][1] == "3=3D3="


def test_long(gpu_ctx):
    rng = random.Random(3000)
    q = random_seq(rng, 3000)
    s = list(q)
    for _ in range(30):
        s[rng.randrange(3000)] = rng.choice("ACGU")
    s = "".join(s)
    for _ in range(5):
        at, g = rng.randrange(100, 2800), rng.randint(1, 6)
        s = s[:at] + random_seq(rng, g) + s[at:] if rng.random() < 0.5 else s[:at] + s[at + g:]
    s = (s + random_seq(rng, 3000))[:3000]
    recs, cigars, stats = check(gpu_ctx, [q], [s, "G"], min_score=1)
    assert recs[0][2] > 5000 and recs[0][9] >= 4 and stats["cells"] == 3000 * 3001


def test_composition(gpu_ctx):
    queries, known = mixture(77, n_q=30, n_k=300, q_len=(40, 110), k_len=(30, 120))
    want = restate(queries, known, DEFAULT, 18)
    assert sum(want[1]) > 200
    base = check(gpu_ctx, queries, known, DEFAULT, 18, want=want)
    assert base[2]["score_passes"] == 1 and base[2]["trace_passes"] == 1
    # alone, query by query
    alone = []
    for qi, q in enumerate(queries):
        recs, cigars, _ = run(gpu_ctx, [q], known, DEFAULT, 18)
        alone += [((qi,) + r[1:], c) for r, c in zip(recs, cigars)]
    assert alone == list(zip(base[0], base[1]))
    # the known file shuffled, compared after mapping the indices back
    order = list(range(len(known)))
    random.Random(5).shuffle(order)
    recs, cigars, _ = run(gpu_ctx, queries, [known[x] for x in order], DEFAULT, 18)
    back = sorted((((r[0], order[r[1]]) + r[2:], c) for r, c in zip(recs, cigars)), key=lambda t: (t[0][0], -t[0][2], t[0][1]))
    assert back == list(zip(base[0], base[1]))
    # forced capacities: one query per scoring pass and one hit per traceback pass, then a few of each
    for capacity, k in ((8 * len(known), 0), (10000, 2), (70000, 0)):
        recs, cigars, stats = check(gpu_ctx, queries, known, DEFAULT, 18, max_lines=k, capacity=capacity, want=want)
        assert stats["score_passes"] > 1 and stats["trace_passes"] > 1 and stats["passes"] == stats["score_passes"] + stats["trace_passes"]
        if k == 0:
            assert (recs, cigars) == base[:2]


def test_refusals(gpu_ctx):
    from mir_prefer_amd import capi
    ok = ["ACGUACGU"]
    for queries, known, side, record in (([b"ACGU", b"", b"GGGG"], ok, "query", 2), ([b"ACGU", b"A" * 3001], ok, "query", 2), ([b"AC\x80U"], ok, "query", 1),
                                         (ok, [b"ACGU", b""], "known", 2), (ok, [b"A" * 3001], "known", 1), (ok, [b"ACGU", b"AC\xffU"], "known", 2)):
        with pytest.raises(capi.MirpError) as e:
            gpu_ctx.hairpin_align(queries, known)
        assert "(-10)" in str(e.value) and "%s record %d:" % (side, record) in str(e.value), str(e.value)
    with pytest.raises(capi.MirpError):
        gpu_ctx.hairpin_align(ok, ok, min_score=0)
    recs, cigars = gpu_ctx.hairpin_align(["A" * 3000], ["A" * 3000, "acgtNNxx"], min_score=1)
    assert recs["score"].tolist() == [6000, 2] and cigars == ["3000=", "1="]


# ---------------------------------------------------------------------------------------------------- the command
def _cli(args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.hairpins"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _fasta(names, seqs, width=60):
    return "".join(">%s some text\n%s\n" % (n, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for n, s in zip(names, seqs))


def test_the_command(tmp_path):
    queries, known = mixture(9, n_q=6, n_k=60, q_len=(60, 120), k_len=(40, 150))
    queries.append("ACGUACGUAAAACCCCGGGGUUUU" * 3)
    known.append(queries[-1])                                   # an identical pair
    q_names = ["pre%d" % x for x in range(len(queries))]
    species = ["ath", "osa", "zma"]
    k_names = ["%s-MIR%d%s" % (species[x % 3], 150 + x // 7, "abcdefg"[x % 7]) for x in range(len(known))]
    fa, kn, kn2 = tmp_path / "pre.fa", tmp_path / "hairpin.fa", tmp_path / "more.fa"
    fa.write_text(_fasta(q_names, queries))
    kn.write_text(_fasta(k_names[:40], known[:40]) + ">ath-MIR999 too long\n%s\n>ath-MIR998 empty\n\n" % ("A" * 3001))
    kn2.write_text(_fasta(k_names[40:], known[40:]))

    def expected(keep, min_score=30, k=0):
        names, seqs = [k_names[x] for x in keep], [known[x] for x in keep]
        hits, per = restate(queries, seqs, DEFAULT, min_score)
        hits = cut(hits, per, k)
        return hits_text(q_names, queries, names, seqs, hits), summary_text(q_names, queries, names, seqs, hits, per)

    r = _cli(["-s", "30", str(fa), str(kn), str(kn2)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    out, summ = tmp_path / "pre.fa.hairpins.tsv", tmp_path / "pre.fa.hairpins.summary.tsv"
    want = expected(range(len(known)))
    assert out.read_text() == want[0] and summ.read_text() == want[1]
    assert "\tidentical\t" in want[1] and "\thomolog\t" in want[1] and "\tnovel\t" in want[1]
    assert b"%d queries, %d known sequences kept (2 skipped)" % (len(queries), len(known)) in r.stderr and b"1 identical" in r.stderr
    # --species, -k, -o: the summary follows the hits file; the skipped count is taken before the species filter
    (tmp_path / "t").mkdir()
    r = _cli(["-s", "30", "-k", "2", "--species", "ath,zma", "-o", "t/x.tsv", str(fa), str(kn), str(kn2)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    keep = [x for x in range(len(known)) if x % 3 != 1]
    want = expected(keep, k=2)
    assert (tmp_path / "t" / "x.tsv").read_text() == want[0] and (tmp_path / "t" / "x.summary.tsv").read_text() == want[1]
    assert b"%d known sequences kept (2 skipped)" % len(keep) in r.stderr
    # an empty known set: every query is novel
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    r = _cli(["-o", "t/e.tsv", str(fa), str(empty)], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "t" / "e.tsv").read_text() == hits_text([], [], [], [], [])
    assert (tmp_path / "t" / "e.summary.tsv").read_text() == "".join("%s\t%d\tnovel\t.\t.\t.\t.\t.\t.\t0\t.\n" % (n, len(q)) for n, q in zip(q_names, queries))
    # refusals: status 255, the file and the record named, no output left, not even an earlier run's; option errors: status 2
    for text, record in ((">a\nACGU\n>b\n\n", 2), (">a\n%s\n" % ("A" * 3001), 1), (">a\nAC\xe9U\n", 1)):
        bad = tmp_path / "t" / "bad.fa"
        bad.write_bytes(text.encode("latin-1"))
        for nm in ("bad.fa.hairpins.tsv", "bad.fa.hairpins.summary.tsv"):
            (tmp_path / "t" / nm).write_text("old\n")
        r = _cli([str(bad), str(kn)], tmp_path)
        assert r.returncode == 255 and b"Error: " in r.stderr and b"bad.fa: record %d:" % record in r.stderr, r.stderr.decode()
        assert not list((tmp_path / "t").glob("bad.fa.*"))
    # a byte >= 0x80 in a known record is a refusal too, also in a record that --species drops, and in the rest of a header line
    for text in (">ath-MIR1\nACGU\n>osa-MIR2\nAC\xe9U\n", ">ath-MIR1\nACGU\n>ath-MIR2 caf\xe9\nACGU\n"):
        badk = tmp_path / "t" / "badk.fa"
        badk.write_bytes(text.encode("latin-1"))
        (tmp_path / "t" / "y.tsv").write_text("old\n")
        r = _cli(["--species", "ath", "-o", "t/y.tsv", str(fa), str(kn), str(badk)], tmp_path)
        assert r.returncode == 255 and b"badk.fa: record 2: a byte >= 0x80" in r.stderr, r.stderr.decode()
        assert not list((tmp_path / "t").glob("y.*"))
    assert _cli([str(tmp_path / "none.fa"), str(kn)], tmp_path).returncode == 255
    assert _cli(["-o", "nodir/x.tsv", str(fa), str(kn)], tmp_path).returncode == 255 and not (tmp_path / "nodir").exists()
    assert _cli(["--gap-extend", "0", str(fa), str(kn)], tmp_path).returncode == 2
