#!/usr/bin/env python3
"""Dev-only (build container): golden vectors for the read preparation commands (mir_prefer_amd.reads).

Runs the reference's three scripts -- scripts/process-reads-fasta.py, convert-mirdeep2-fasta.py, convert-readcount-file.py -- with python3 in a
temporary directory on hand-made edge cases and seeded random files, and stores every input with the script's .processed output (and its stdout
count of unique reads for the collapse).  Usage: gen_reads_golden.py <reference checkout>.  Output: tests/golden/reads.json.gz"""
import gzip, json, os, random, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)

COLLAPSE_CASES = {
    "lone_cr": b"ACGT\rTT\nACGT\n",
    "raw_first_byte": b" >x\n>x\n >x\n",
    "strip_set": b"\x1cACGT\nACGT \n\tACGT\x0b\n\x0c\x1d\x1e\x1fACGT\r\n ACGT\t \n",
    "blank_lines": b"\n\nACGT\n\n   \n\t\n",
    "no_final_newline": b"ACGT\nTTGA\nACGT",
    "case": b"acgt\nACGT\nAcGt\nacgt\n",
    "other_bytes": b"NNRYKM\nAC\x00GT\nAC\x00GT\n~!@#$%^&*()\n\x00\n\x7f\n",
    "multi_line_seq": b">r1\nACGTACGT\nACGT\n>r2\nACGTACGT\n>r3\nACGT\nTT\n",
    "empty": b"",
    "headers_only": b">a\n>b\r\n>c",
    "newline_mix": b"A\r\nB\rA\nB\r\n\r\r\n\rA",
    "final_lone_cr": b"ACGT\r",
    "crlf_only": b"\r\n\r\n",
    "long_lines": (b"ACGU" * 1250 + b"\n") * 3 + b"ACGU" * 1249 + b"\n" + (b"ACGU" * 1250)[:-1] + b"A\n",
    "lengths_around_16": b"".join(b"A" * k + b"\n" for k in range(0, 70)) + b"".join(b"A" * k + b"\n" for k in range(69, -1, -1)),
    "header_variants": b">\n>>\n> x\n\n>",
}

MIRDEEP2_CASES = {
    "plain": b">seq_1_x100\nACGT\n>seq_2_x5\nTTGCA\n",
    "crlf_and_cr": b">a_x3\r\nAC\r\n>b_x7\rGG\r>c_x1 \nTT",
    "weird": b">weird\nAA\n>xx_x12x\nCC\n>x\n\n>y_x 4 \t\nA x B\n",
    "empty": b"",
}

READCOUNT_CASES = {
    "plain": b"ACGT 10\nTTT\t5\n",
    "blank_and_single": b"\n   \nACGT\t 3 \nTTT\nGG 1 2\n\t\n",
    "newline_mix": b"AC 2\r\nGT 4\rTT 9",
    "empty": b"",
}


def rand_reads(r, n_lines, crlf=False):
    alpha = "ACGTN"
    pool = ["".join(r.choice(alpha) for _ in range(r.randint(15, 40))) for _ in range(max(1, n_lines // 8))]
    lines = []
    for k in range(n_lines):
        if r.random() < 0.3:
            lines.append(">read_%d" % k)
        elif r.random() < 0.7:
            lines.append(pool[min(int(r.paretovariate(1.1)) - 1, len(pool) - 1)])
        else:
            s = "".join(r.choice(alpha + "acgt") for _ in range(r.randint(0, 50)))
            lines.append(r.choice(["", " ", "\t"]) + s + r.choice(["", " ", "\x0b"]))
    eols = ["\n", "\r\n", "\r"] if crlf else ["\n"]
    return "".join(x + r.choice(eols) for x in lines).encode()


def run_script(ref, script, files, tmp):
    names = os.path.join(tmp, "names.txt")
    with open(names, "w") as f:
        f.write("".join("S%d\n" % k for k in range(len(files))))
    paths = []
    for k, data in enumerate(files):
        p = os.path.join(tmp, "in%d.txt" % k)
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    out = subprocess.run([sys.executable, os.path.join(ref, "scripts", script), names] + paths, capture_output=True, check=True, text=True).stdout
    res = []
    for p in paths:
        with open(p + ".processed", "rb") as f:
            res.append(f.read())
    unique = {}
    for line in out.splitlines():
        if line.startswith("File ") and line.endswith(" unique reads"):
            w = line.split()
            unique[w[1]] = int(w[3])
    return res, [unique.get(p) for p in paths]


def main():
    ref = sys.argv[1]
    r = random.Random(29)
    collapse = dict(COLLAPSE_CASES)
    for k in range(4):
        collapse["random_%d" % k] = rand_reads(r, r.choice([200, 3000, 20000]), crlf=k % 2 == 1)
    gold = {}
    for cmd, script, cases in (("collapse", "process-reads-fasta.py", collapse), ("mirdeep2", "convert-mirdeep2-fasta.py", MIRDEEP2_CASES),
                               ("readcount", "convert-readcount-file.py", READCOUNT_CASES)):
        with tempfile.TemporaryDirectory() as tmp:
            outs, unique = run_script(ref, script, list(cases.values()), tmp)
        gold[cmd] = [{"name": n, "prefix": "S%d" % k, "input": i.decode("latin-1"), "output": o.decode("latin-1"), "unique": u}
                     for k, ((n, i), o, u) in enumerate(zip(cases.items(), outs, unique))]
    with gzip.open(os.path.join(GOLD, "reads.json.gz"), "wt") as f:
        json.dump(gold, f)
    print({k: len(v) for k, v in gold.items()})


if __name__ == "__main__":
    main()
