"""GPU tests of `targets -u` (mirp_target_scan with accessibility): a handful of miRNAs against a few short transcripts with sites
on both strands, sites within the flanks' reach of a contig's ends, and a contig shorter than a window.  The `upe` column is compared with
unpaired_batch on the windows this test extracts in Python from the lines' own coordinates (test_unpaired_cpu.site_window, worked by hand there),
formatted the same way, and with the masked restatement, whose values keep 1e-6 away from a rounding boundary of the third decimal (asserted);
the other columns with the same run without -u; the -k cut and forced pass capacities with the bytes of the unsplit run; other flanks; a refused
run; and one run of the command line."""
import multiprocessing
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_targets_bulge_cpu import KIND_M, KIND_T, bulged_site
from tests.test_targets_cpu import ROOT, target_of_mirna, write_fasta
from tests.test_unpaired_cpu import format_upe, site_window, upe_job

pytestmark = pytest.mark.gpu
MIRS = [b"UUCCACAGCUUUCUUGAACUG", b"UGACAGAAGAGAGUGAGCAC", b"UCGGACCAGGCUUCAUUCCCC", b"UGGAGAAGCAGGGCACGUGCA", b"AGAAUCUUGAUGAUGCUGCAU"]
OPTIONS = (dict(), dict(bulge=True), dict(energy=True), dict(bulge=True, energy=True))


def _scan(ctx, tmp_path, d, **kw):
    out = tmp_path / "out.tsv"
    res = ctx.target_scan(str(d / "m.fa"), [str(d / "t.fa")], str(out), both_strands=True, **kw)
    return out.read_bytes(), res


@pytest.fixture(scope="module")
def upe_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("upe")
    rng = np.random.RandomState(2420)
    texts = {name: bytearray(b"ACGT"[c] for c in rng.randint(0, 4, n)) for name, n in (("t1", 300), ("t2", 90), ("t3", 36))}

    def put(name, o, m, strand, kind=None):
        site = target_of_mirna(m, strand) if kind is None else bulged_site(m, strand, kind, 16)
        texts[name][o:o + len(site)] = site
    put("t1", 30, MIRS[0], 0)
    put("t1", 80, MIRS[1], 1)
    put("t1", 130, MIRS[2], 0, KIND_M)              # miRNA position 16 without a partner
    put("t1", 180, MIRS[3], 1, KIND_T)              # an unpaired target base after the partner of position 16
    put("t1", 230, MIRS[4], 0)
    texts["t1"][60:80] = bytes(texts["t1"][60:80]).lower()
    texts["t1"][124] = ord("N")                     # inside the window of the site at 130
    texts["t1"][215:230] = target_of_mirna(MIRS[4], 1)[:15]          # a partner for the site at 230: a hairpin over the site
    put("t2", 0, MIRS[0], 1)                        # at the contig's first base
    put("t2", 30, MIRS[2], 0)
    put("t2", 90 - 20, MIRS[1], 0)                  # at its last
    put("t3", 6, MIRS[3], 0)                        # a contig shorter than a window
    write_fasta(d / "t.fa", [(name, bytes(seq)) for name, seq in texts.items()])
    (d / "m.fa").write_bytes(b"".join(b">mir%d\n%s\n" % (i, m) for i, m in enumerate(MIRS)))
    return d, {name.encode(): bytes(seq) for name, seq in texts.items()}


def windows_of(data, contigs, flanks=(17, 13)):
    """the window of every line of a targets file -> [(window, lo, hi)]"""
    out = []
    for ln in data.split(b"\n")[1:-1]:
        f = ln.split(b"\t")
        out.append(site_window(contigs[f[1]], int(f[2]), int(f[3]), f[4].decode(), *flanks))
    return out


def last_column(data):
    return [ln.split(b"\t")[-1].decode() for ln in data.split(b"\n")[1:-1]]


def without_last_column(data):
    return b"".join(b"\t".join(ln.split(b"\t")[:-1]) + b"\n" for ln in data.split(b"\n")[:-1])


def test_upe_column_is_the_window_s_accessibility(gpu_ctx, upe_input, tmp_path):
    d, contigs = upe_input
    seen = {}
    for kw in OPTIONS:
        got, res = _scan(gpu_ctx, tmp_path, d, accessibility=True, **kw)
        plain, res0 = _scan(gpu_ctx, tmp_path, d, **kw)
        assert got.split(b"\n")[0].endswith(b"\tupe") and not plain.split(b"\n")[0].endswith(b"\tupe")
        assert without_last_column(got) == plain, kw
        assert {k: v for k, v in res.items() if k != "seconds"} == {k: v for k, v in res0.items() if k != "seconds"} and len(res["seconds"]) == 5
        wins = windows_of(got, contigs)
        assert len(wins) == res["sites"] >= 9
        recs = gpu_ctx.unpaired_batch([w for w, _, _ in wins], [lo for _, lo, _ in wins], [hi for _, _, hi in wins])
        assert last_column(got) == [format_upe(float(u)) for u in recs["upe"]], kw
        for w, u in zip(wins, last_column(got)):
            seen[w] = u
    # what the cases cover: both strands, windows clipped at either end of a contig, a contig shorter than a window, both kinds of bulge
    rows = [ln.split(b"\t") for ln in got.split(b"\n")[1:-1]]
    assert {f[4] for f in rows} == {b"+", b"-"} and {f[11][:1] for f in rows} >= {b".", b"t", b"m"}
    assert any(f[1] == b"t2" and int(f[2]) == 1 for f in rows) and any(f[1] == b"t2" and int(f[3]) == 90 for f in rows)
    assert any(f[1] == b"t3" for f in rows) and min(len(w) for w, _, _ in seen) < 40 and max(len(w) for w, _, _ in seen) >= 51
    assert any(float(u) > 15.0 for u in seen.values()) and any(float(u) < 3.5 for u in seen.values())          # the site under the planted hairpin, an open one
    # the restatement of every window: no value at a rounding boundary, and the same three decimals
    jobs = sorted(seen)
    with multiprocessing.get_context("spawn").Pool(14) as pool:
        want = pool.map(upe_job, jobs, chunksize=1)
    for j, r in zip(jobs, want):
        x = r["upe"] * 1000
        assert abs(x - np.floor(x) - 0.5) >= 1e-6, (j, r)
        assert seen[j] == format_upe(r["upe"]), (j, r)


def planned_passes(uncut, k, cap):
    """the passes of a run from its uncut lines: one when the keys fit; otherwise the bins (miRNA, score) up to the score at which
    a miRNA's first k lines are reached, packed in order while they fit"""
    bins = {}
    for ln in uncut.split(b"\n")[1:-1]:
        f = ln.split(b"\t")
        bins.setdefault(f[0], {}).setdefault(float(f[5]), 0)
        bins[f[0]][float(f[5])] += 1
    if sum(sum(b.values()) for b in bins.values()) <= cap:
        return 1
    passes = pend = 0
    for m in sorted(bins, key=lambda name: int(name[3:])):
        cum = 0
        for score in sorted(bins[m]):
            cnt = bins[m][score]
            assert cnt <= cap            # no bin is split by offsets in these cases
            if pend + cnt > cap:
                passes, pend = passes + 1, 0
            pend += cnt
            cum += cnt
            if k and cum >= k:
                break
    return passes + (pend > 0)


def test_cut_and_capacities_give_the_same_bytes(gpu_ctx, upe_input, tmp_path):
    d, _ = upe_input
    kw = dict(bulge=True, energy=True, max_sites=2)
    whole, res = _scan(gpu_ctx, tmp_path, d, accessibility=True, **kw)
    uncut, _ = _scan(gpu_ctx, tmp_path, d, accessibility=True, bulge=True, energy=True)
    assert res["sites"] == whole.count(b"\n") - 1 < uncut.count(b"\n") - 1 and set(whole.split(b"\n")) <= set(uncut.split(b"\n"))
    seen = set()
    try:
        for cap in (0, 4, 7, 40):
            gpu_ctx.set_target_capacity(cap)
            got, res = _scan(gpu_ctx, tmp_path, d, accessibility=True, **kw)
            _, res0 = _scan(gpu_ctx, tmp_path, d, **kw)
            want = planned_passes(uncut, 2, cap or 1 << 26)
            print("capacity %d: %d passes (%d without -u, %d planned)" % (cap, res["passes"], res0["passes"], want))
            assert got == whole, cap
            assert res["passes"] == res0["passes"] == want, (cap, res, res0)
            seen.add(want)
    finally:
        gpu_ctx.set_target_capacity(0)
    assert 1 in seen and len(seen) >= 3          # the forced capacities split the run, each differently


def test_other_flanks(gpu_ctx, upe_input, tmp_path):
    d, contigs = upe_input
    base, _ = _scan(gpu_ctx, tmp_path, d, accessibility=True, bulge=True)
    for flanks in ((0, 0), (30, 5), (0, 95), (95, 0)):
        got, _ = _scan(gpu_ctx, tmp_path, d, accessibility=True, bulge=True, flanks=flanks)
        assert without_last_column(got) == without_last_column(base)
        wins = windows_of(got, contigs, flanks)
        recs = gpu_ctx.unpaired_batch([w for w, _, _ in wins], [lo for _, lo, _ in wins], [hi for _, _, hi in wins])
        assert last_column(got) == [format_upe(float(u)) for u in recs["upe"]], flanks
        if flanks == (0, 0):
            assert all(hi - lo + 1 == len(w) for w, lo, hi in wins)
        else:
            assert last_column(got) != last_column(base)
    again, _ = _scan(gpu_ctx, tmp_path, d, accessibility=True, bulge=True)          # the flanks of one call do not outlive it
    assert again == base


def test_a_refused_run_leaves_no_file(gpu_ctx, upe_input, tmp_path):
    from mir_prefer_amd import capi
    d, _ = upe_input
    out = tmp_path / "out.tsv"
    out.write_bytes(b"an earlier run\n")
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">ok\n" + MIRS[0] + b"\n>short\nACGU\n")
    with pytest.raises(capi.MirpError) as e:
        gpu_ctx.target_scan(str(bad), [str(d / "t.fa")], str(out), accessibility=True)
    assert "(-10)" in str(e.value) and not out.exists()
    with pytest.raises(capi.MirpError):
        gpu_ctx.target_scan(str(d / "m.fa"), [str(d / "t.fa")], str(out), accessibility=True, flanks=(90, 6))
    assert not out.exists()
    o = capi.TargetOpts()
    o.max_half_score, o.accessibility = 8, 2
    import ctypes as C
    arr = (C.c_char_p * 1)(os.fsencode(str(d / "t.fa")))
    assert gpu_ctx.lib.mirp_target_scan(gpu_ctx.h, os.fsencode(str(d / "m.fa")), arr, 1, C.byref(o), os.fsencode(str(out)), None, None) == -1
    assert not out.exists()


def test_command_line(gpu_ctx, upe_input, tmp_path):
    d, _ = upe_input
    want, _ = _scan(gpu_ctx, tmp_path, d, accessibility=True, bulge=True, flanks=(5, 3))
    r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets", "-u", "-b", "-g", "--flank-up", "5", "--flank-down", "3", "-o", str(tmp_path / "cli.tsv"),
                        str(d / "m.fa"), str(d / "t.fa")], cwd=str(tmp_path), capture_output=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "cli.tsv").read_bytes() == want
    assert b"sites written to" in r.stderr
