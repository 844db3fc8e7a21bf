"""CPU test of the structure rules on words (mir-prefer_amd/csrc/ss_words.h, the rules of predict_kernel and homolog_eval_kernel): the stand-alone check
program tests/tools/ss_words_check.cpp, which includes the header and the character-by-character restatement of every rule, is compiled with the host C++
compiler under -fsanitize=address,undefined and run as an executable of its own.  It compares find / rfind / count / clip / partner / is_stem_loop /
good_bifurcation / duplex_code / get_maturestar_info / duplex_stats result by result on

  * every string over . ( ) up to length 11, as a view at offsets 0, 1, 15, 16, 17, 31, 32, 33, 63, 64 and 65 of a longer random line,
  * seeded random balanced and unbalanced strings of 15-17, 31-33, 63-65, 127-129, 325, 350 and 3,000 characters, whole and as pieces at odd offsets,
  * hairpin loops and partner pairs placed across one and across two word boundaries,
  * duplex inputs of 20 to 200 characters, on both sides of the 64-character register path (the program fails unless both were taken),
  * the duplex figures of a passing structure (ssw_duplex_stats: prime5, total_bps, total_dots) over every interval of the exhaustive views that holds a
    bracket, on the hairpins across word boundaries, and on hairpins in lines of 60 to 3,000 characters shifted so that each of the five positions the
    figures are made of lands on characters 31-33, 63-65 and in the line's last word, with the interval on either arm,

and exits non-zero at the first difference.  Every staged line is a heap block of exactly its words, so a read past a line is a sanitizer error."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mir-prefer_amd", "csrc")


def test_the_header_has_no_dependencies_and_no_access_per_character():
    src = open(os.path.join(CSRC, "ss_words.h")).read()
    assert re.findall(r"^\s*#\s*include\b.*$", src, re.M) == []
    # the kernels hold none of the rules themselves: they reach the text only through the header
    for f in ("predict_kernel.hip", "homolog_kernels.hip", "predict_device.h"):
        text = open(os.path.join(CSRC, f)).read()
        assert "operator[](int" not in text and not re.search(r"\bd_(find|rfind|count|partner|is_stem_loop|good_bifurcation|duplex_code|maturestar)\(", text), f
        assert "hm_duplex_stats" not in text, f


def test_every_rule_equals_its_restatement_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "ss_words_check"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "tools", "ss_words_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "exhaustive: 2922920 views" in p.stdout                                    # 11 offsets x sum of 3^k, k = 0 .. 11
    m = re.search(r"duplex inputs of 20 \.\. 200 characters: (\d+) of at most 64, (\d+) longer; register path taken (\d+) times, word path (\d+) times", p.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), p.stdout
    codes = dict((int(a), int(b)) for a, b in re.findall(r" (\d+):(\d+)", p.stdout.split("codes seen:")[1].splitlines()[0]))
    assert sum(1 for c in range(1, 13) if codes.get(c, 0) > 0) >= 8 and codes[0] > 1000, codes
    m = re.search(r"^duplex figures: (\d+) comparisons, (\d+) with prime5 == 0$", p.stdout, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, p.stdout
    assert re.search(r"^OK \d+ comparisons$", p.stdout, re.M)
