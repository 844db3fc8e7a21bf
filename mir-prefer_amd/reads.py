"""Read preparation before the pipeline: the three scripts the reference ships under scripts/ to give reads ids that carry their depth
(`Sample_rA_xN`, parsed at miR_PREFeR.py:242-253).

    python -m mir_prefer_amd.reads {collapse|mirdeep2|readcount} [--device N] samplenamelist file1 [file2 ...]

collapse   process-reads-fasta.py:60-80 -- uncollapsed FASTA -> one record per distinct read, A from 0 in order of first occurrence, B = count.
           On the GPU (mirp_collapse_reads, reads_kernels.hip), one device context for all files, processed in order; there is no CPU path.
mirdeep2   convert-mirdeep2-fasta.py:50-63 -- miRDeep2 collapsed FASTA (`..._xN` ids) -> renamed ids, C from 1; other lines copied.
readcount  convert-readcount-file.py:47-60 -- "read count" lines -> FASTA, C from 1.

Every input file X gives X.processed next to it.  Argument errors (names and files differ in number, a file is missing, too few arguments)
exit with status 255 before anything is written, as the scripts' sys.exit(-1) does."""
import os
import sys

COMMANDS = ("collapse", "mirdeep2", "readcount")
USAGE = "Usage: python -m mir_prefer_amd.reads {collapse|mirdeep2|readcount} [--device N] <samplenamelist> <file1> <file2> .. <fileN>\n"
# the scripts read and write in text mode: universal newlines in, "\n" out; surrogateescape carries any byte through the two converters unchanged
_TEXT = {"encoding": "utf-8", "errors": "surrogateescape"}


def read_sample_names(path):
    """samplenamelist: stripped lines, blank lines skipped (the scripts' `if line.strip(): prefix.append(line.strip())`)."""
    with open(path, **_TEXT) as f:
        return [line.strip() for line in f if line.strip()]


def convert_mirdeep2(name, prefix):
    with open(name + ".processed", "w", newline="\n", **_TEXT) as outf, open(name, **_TEXT) as f:
        count = 1
        for line in f:
            if line.startswith(">"):
                outf.write(">" + prefix + "_r" + str(count) + "_x" + line.split("x")[-1].strip() + "\n")
                count += 1
            else:
                outf.write(line)


def convert_readcount(name, prefix):
    with open(name + ".processed", "w", newline="\n", **_TEXT) as outf, open(name, **_TEXT) as f:
        count = 1
        for line in f:
            if not line.strip():
                continue
            sp = line.split()
            outf.write(">" + prefix + "_r" + str(count) + "_x" + sp[-1].strip() + "\n")
            outf.write(sp[0] + "\n")
            count += 1


def _fail(msg):
    sys.stderr.write(msg)
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in COMMANDS:
        return _fail(USAGE)
    cmd, rest = argv[0], argv[1:]
    device = 0
    if rest and (rest[0] == "--device" or rest[0].startswith("--device=")):
        val = rest[0].split("=", 1)[1] if "=" in rest[0] else (rest[1] if len(rest) > 1 else "")
        rest = rest[1:] if "=" in rest[0] else rest[2:]
        if not val.isdigit():
            return _fail(USAGE)
        device = int(val)
    if len(rest) < 2:
        return _fail(USAGE)
    if not os.path.isfile(rest[0]):
        return _fail("Error: file " + rest[0] + " does not exist!!!\n")
    prefix = read_sample_names(rest[0])
    names = rest[1:]
    if len(prefix) != len(names):
        return _fail("Error: number of sample/tissue names in the samplenamelist file must be the same as the number of input fasta files.\n")
    for name in names:
        if not os.path.exists(name):
            return _fail("Error: file " + name + " does not exist!!!\n")

    if cmd == "collapse":
        from . import capi
        try:
            ctx = capi.Context(device)
        except capi.MirpError as e:
            return _fail("Error: collapse runs on the GPU and none is usable (%s); there is no CPU path.\n" % e)
        try:
            unique = []
            for name, p in zip(names, prefix):
                sys.stdout.write("Start processing file " + name + "\n")
                sys.stdout.flush()
                try:
                    res = ctx.collapse_reads(name, p, name + ".processed")
                except capi.MirpError as e:
                    return _fail("Error: %s\n" % e)
                sys.stdout.write("Finish file " + name + "\n")
                unique.append((name, res["n_unique"]))
            for name, n in unique:
                sys.stdout.write("File " + name + " has " + str(n) + " unique reads\n")
        finally:
            ctx.close()
    else:
        convert = convert_mirdeep2 if cmd == "mirdeep2" else convert_readcount
        for name, p in zip(names, prefix):
            sys.stdout.write("Start processing file " + name + "\n")
            convert(name, p)
            sys.stdout.write("Finish file " + name + "\n")
    sys.stdout.write("DONE\n\n")
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
