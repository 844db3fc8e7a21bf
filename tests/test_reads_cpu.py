"""Host tests of the read preparation commands (mir_prefer_amd.reads): the two converters byte for byte against the reference's scripts
(tests/golden/reads.json.gz, tests/golden/tools/gen_reads_golden.py), the scripts' argument errors (exit 255, nothing written), and the collapse
refusing to run without a GPU."""
import io
import os
import subprocess
import sys

import pytest

from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = gu.load_json("reads.json.gz")


def _run(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.reads"] + args, cwd=cwd, capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _write_cases(tmp_path, cases):
    (tmp_path / "names.txt").write_text("".join(c["prefix"] + "\n" for c in cases))
    paths = []
    for c in cases:
        p = tmp_path / (c["name"] + ".txt")
        p.write_bytes(c["input"].encode("latin-1"))
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("cmd", ["mirdeep2", "readcount"])
def test_converters_match_reference_scripts(tmp_path, cmd):
    cases = GOLD[cmd]
    paths = _write_cases(tmp_path, cases)
    r = _run([cmd, str(tmp_path / "names.txt")] + paths, tmp_path)
    assert r.returncode == 0, r.stderr
    for c, p in zip(cases, paths):
        assert open(p + ".processed", "rb").read() == c["output"].encode("latin-1"), c["name"]
    out = r.stdout.decode()
    for p in paths:
        assert "Start processing file %s\n" % p in out and "Finish file %s\n" % p in out
    assert out.endswith("DONE\n\n") and "unique reads" not in out


def test_collapse_fixtures_agree_with_a_dict_restatement():
    """The fixtures hold what the reference's collapse does; the plain restatement the GPU tests use must say the same."""
    for c in GOLD["collapse"]:
        want, n = restate_collapse(c["input"].encode("latin-1"), c["prefix"])
        assert want == c["output"].encode("latin-1") and n == c["unique"], c["name"]


def restate_collapse(data, prefix):
    """process-reads-fasta.py:60-80 as a plain dict (ASCII input): -> (.processed bytes, unique reads)."""
    d = {}
    for line in io.StringIO(data.decode("latin-1"), newline=None):
        if line.startswith(">"):
            continue
        k = line.strip()
        d[k] = d.get(k, 0) + 1
    return "".join(">%s_r%d_x%d\n%s\n" % (prefix, i, c, k) for i, (k, c) in enumerate(d.items())).encode("latin-1"), len(d)


@pytest.mark.parametrize("cmd", ["collapse", "mirdeep2", "readcount"])
def test_argument_errors_exit_255_and_write_nothing(tmp_path, cmd):
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_bytes(b"ACGT\n")
    b.write_bytes(b"ACGT\n")
    names = tmp_path / "names.txt"
    names.write_text("S1\n\n  S2  \n")
    before = sorted(os.listdir(tmp_path))
    for args in ([cmd, str(names), str(a)],                                 # two names, one file
                 [cmd, str(names), str(a), str(tmp_path / "missing.fa")],  # a file is missing
                 [cmd, str(names)],                                         # no file
                 [cmd],                                                     # nothing
                 [cmd, "--device"],
                 [cmd, str(tmp_path / "no_names.txt"), str(a)]):            # the name list is missing
        r = _run(args, tmp_path)
        assert r.returncode == 255, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, args
    r = _run(["squash", str(names), str(a), str(b)], tmp_path)
    assert r.returncode == 255 and sorted(os.listdir(tmp_path)) == before


def test_collapse_without_gpu_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a = tmp_path / "a.fa"
    a.write_bytes(b">r\nACGT\nACGT\n")
    (tmp_path / "names.txt").write_text("S1\n")
    r = _run(["collapse", str(tmp_path / "names.txt"), str(a)], tmp_path)
    assert r.returncode != 0
    assert b"GPU" in r.stderr and b"no CPU path" in r.stderr
    assert not os.path.exists(str(a) + ".processed")
