"""CPU tests of the piece boundaries of a pass's text (mir-prefer_amd/csrc/text_pieces.h, used by site_lines.h): a small driver that includes the
header and nothing else of the project is compiled with the host C++ compiler, walks lists of line sizes the way site_finish_pass does and
prints the pieces, which are compared with a restatement in Python and checked for the properties a sink relies on.

A scenario is the piece size, the read that fails (0: none) and the line sizes; a size of 0 is a key that -k cut.  Lines: `i0 i1 len` per piece,
then `E rc`."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "text_pieces.h"

int main() {
    long long piece, fail_at, n;
    while (std::scanf("%lld %lld %lld", &piece, &fail_at, &n) == 3) {
        std::vector<long long> toff((size_t)n + 1, 0);
        for (long long i = 0; i < n; i++) {
            long long s = 0;
            if (std::scanf("%lld", &s) != 1) return 2;
            toff[(size_t)i + 1] = toff[(size_t)i] + s;
        }
        long long reads = 0;
        int rc = 0;
        for (long long i0 = 0, base = 0; i0 < n && rc == 0;) {
            const auto read = [&](long long i, long long* v) -> int {
                if (i <= i0 || i > n) return 99;                  // outside what the header may ask for
                if (++reads == fail_at) return 7;
                *v = toff[(size_t)i];
                return 0;
            };
            long long i1 = -1, end = -1;
            rc = mirp::text_piece_end(i0, n, base, toff[(size_t)n], piece, read, &i1, &end);
            if (rc) break;
            std::printf("%lld %lld %lld\n", i0, i1, end - base);
            i0 = i1;
            base = end;
        }
        std::printf("E %d\n", rc);
    }
    return 0;
}
"""


def _build(d, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / ("driver" + "".join(f.replace("=", "_").replace(",", "_") for f in flags))
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "mir-prefer_amd", "csrc"), str(d / "driver.cpp"), "-o", str(exe)])

    def run(scenarios):
        """scenarios: (piece, fail_at, sizes) each -> ([(i0, i1, len), ...], rc) of each"""
        text = "".join("%d %d %d\n%s\n" % (piece, fail_at, len(sizes), " ".join(map(str, sizes))) for piece, fail_at, sizes in scenarios)
        p = subprocess.run([str(exe)], input=text.encode(), capture_output=True, timeout=60)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        res, cur = [], []
        for ln in p.stdout.decode().split("\n")[:-1]:
            if ln.startswith("E "):
                res.append((cur, int(ln[2:])))
                cur = []
            else:
                cur.append(tuple(map(int, ln.split())))
        assert not cur and len(res) == len(scenarios)
        return res
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("text_pieces"), [])


def restate(piece, sizes):
    """the pieces, greedily: a piece runs to the last boundary within the piece size (the end of the text when the rest fits)"""
    toff = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
    out, i0, n = [], 0, len(sizes)
    while i0 < n:
        i1 = n if toff[n] - toff[i0] <= piece else max([i0 + 1] + [i for i in range(i0 + 1, n) if toff[i] - toff[i0] <= piece])
        out.append((i0, i1, toff[i1] - toff[i0]))
        i0 = i1
    return out


def _properties(piece, sizes, pieces):
    n = len(sizes)
    assert [p[0] for p in pieces] == [0] * bool(pieces) + [p[1] for p in pieces[:-1]] and (pieces[-1][1] if pieces else 0) == n      # tile [0, n) in order
    for k, (i0, i1, ln) in enumerate(pieces):
        assert i1 > i0 and ln == sum(sizes[i0:i1]) and ln <= piece
        if k + 1 < len(pieces):                                  # maximal: the next non-empty line does not fit
            nxt = next(s for s in sizes[i1:] if s > 0)
            assert ln + nxt > piece


def _sizes(rng, n):
    s = [rng.randint(0, 50) for _ in range(n)]
    for where in rng.sample(("start", "middle", "end"), rng.randint(0, 3)):       # runs of keys that -k cut
        run = rng.randint(1, max(1, n // 3))
        a = 0 if where == "start" else n - run if where == "end" else rng.randint(0, max(0, n - run))
        for i in range(max(0, a), min(n, a + run)):
            s[i] = 0
    return s


def _scenarios(seed, count):
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = rng.randint(0, 3) if k % 5 == 0 else rng.randint(0, 200)
        sizes = _sizes(rng, n)
        total, longest = sum(sizes), max(sizes + [1])
        piece = rng.choice((longest, longest + 1, max(longest, total), max(longest, total - 1), max(longest, total // 2), rng.randint(longest, max(longest, total))))
        out.append((max(1, piece), 0, sizes))
    return out


def test_hand_cases(driver):
    cases = [(10, 0, []), (10, 0, [0, 0, 0]), (10, 0, [10]), (10, 0, [4, 6, 1]), (10, 0, [0, 0, 5, 5, 0, 0, 5, 0]), (5, 0, [5, 5, 5]), (100, 0, [3, 0, 4])]
    want = [[], [(0, 3, 0)], [(0, 1, 10)], [(0, 2, 10), (2, 3, 1)], [(0, 6, 10), (6, 8, 5)], [(0, 1, 5), (1, 2, 5), (2, 3, 5)], [(0, 3, 7)]]
    got = driver(cases)
    assert [g[0] for g in got] == want and all(g[1] == 0 for g in got)
    for (piece, _, sizes), w in zip(cases, want):
        assert restate(piece, sizes) == w


def test_random_lists_against_the_restatement(driver):
    scenarios = _scenarios(20271, 400)
    got = driver(scenarios)
    multi = 0
    for (piece, _, sizes), (pieces, rc) in zip(scenarios, got):
        assert rc == 0 and pieces == restate(piece, sizes), (piece, sizes)
        _properties(piece, sizes, pieces)
        multi += len(pieces) > 2
    assert multi > 100


def test_a_failing_read_stops_the_walk(driver):
    scenarios = [s for s in _scenarios(20272, 200) if len(restate(s[0], s[2])) > 2]
    assert len(scenarios) > 30
    whole = driver(scenarios)
    failing = [(piece, k, sizes) for (piece, _, sizes) in scenarios for k in (1, 2, 5)]
    got = driver(failing)
    stopped = 0
    for (piece, k, sizes), (pieces, rc) in zip(failing, got):
        full = restate(piece, sizes)
        assert pieces == full[:len(pieces)]
        assert rc in (0, 7) and (rc == 7 or pieces == full)          # rc 0: the walk needed fewer than k reads
        stopped += rc == 7
    assert stopped > 30 and all(rc == 0 for _, rc in whole)


def test_abi_entries_are_declared():
    """the piece knob and the sort hooks the GPU tests use (test_text_pieces_gpu.py, test_device_sort_gpu.py): declared, defined and bound"""
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    csrc = os.path.join(ROOT, "mir-prefer_amd", "csrc")
    defined = "".join(open(os.path.join(csrc, f)).read() for f in ("mirp_api.cpp", "mirp_pipeline.cpp"))
    binding = open(os.path.join(ROOT, "mir-prefer_amd", "capi.py")).read()
    for name in ("mirp_set_text_piece", "mirp_text_pieces_last", "mirp_sort_alns", "mirp_sort_records", "mirp_sort_u64"):
        assert name + "(" in header and name + "(" in defined and name in binding, name
    assert "typedef struct { uint64_t key; uint32_t a, b; } MirpSortRec;" in header
    assert "lowered only to test the piece path; no output depends on it" in header.lower().replace("\n * ", " ")
    assert "#define MIRP_ABI_VERSION 17 " in open(os.path.join(csrc, "mirp_api.cpp")).read()          # only entries are added
    from mir_prefer_amd import capi
    assert capi.ABI_VERSION == 17 and capi.SORT_REC_DTYPE.itemsize == 16 and capi.SORT_REC_DTYPE.names == ("key", "a", "b")
    # the two literals are gone: both piece loops read the context's size
    for f, text in (("site_lines.h", "c->text_piece_bytes()"), ("mirp_ctx.h", "c->text_piece_bytes()")):
        src = open(os.path.join(csrc, f)).read()
        assert text in src and "c->text_pieces++" in src, f
    assert "1ll << 30, read_toff" not in open(os.path.join(csrc, "site_lines.h")).read()


def test_the_driver_is_clean_under_the_host_sanitizers(tmp_path):
    run = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    scenarios = _scenarios(20273, 100) + [(p, 3, s) for p, _, s in _scenarios(20274, 30)]
    for (piece, k, sizes), (pieces, rc) in zip(scenarios, run(scenarios)):
        full = restate(piece, sizes)
        assert pieces == full[:len(pieces)] and (rc == 7 or pieces == full)
