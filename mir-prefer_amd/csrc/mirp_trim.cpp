// C-ABI of the read trimming (mirp_trim_reads): argument checks and the output file on the host; trim_kernels.hip parses, trims and
// emits on the device.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <string>
#include "mirp_fasta.h"

// Trims one FASTQ / FASTA text held in host memory and writes the FASTA of the kept reads to out_path.  out_path is opened only once every refusal
// has been ruled out; on a refusal or a later error the file at out_path is removed, a partial one or one left by an earlier run, so a refused
// input has no output.
extern "C" int mirp_trim_reads(mirp_ctx* c, const char* data, int64_t n, const char* name, const MirpTrimOpts* o, const char* out_path, int64_t stats[7],
                               double seconds[6]) {
    if (!c) return -1;
    c->text_pieces = 0;
    c->t_paths[0] = c->t_paths[1] = 0;
    if ((!data && n > 0) || n < 0 || !name || !o || !out_path) return fail(c, -1, "mirp_trim_reads: bad argument");
    if (o->adapter_len < 0 || o->adapter_len > 64 || o->error_permille < 0 || o->error_permille > 999 || o->quality_cutoff < 0 || o->quality_cutoff > 93 ||
        o->min_length < 0 || o->max_length < 0 || (o->max_length > 0 && o->max_length < o->min_length) ||
        (o->adapter_len > 0 && (o->min_overlap < 1 || o->min_overlap > o->adapter_len)) || (o->discard_untrimmed && o->adapter_len == 0))
        return fail(c, -1, "mirp_trim_reads: bad options");
    for (int k = 0; k < o->adapter_len; k++)
        if (!std::strchr("ACGTacgt", o->adapter[k]) || o->adapter[k] == 0) return fail(c, -1, "mirp_trim_reads: the adapter is not ACGT");
    HIPCHK(c, hipSetDevice(c->device));
    double sec[6] = {0, 0, 0, 0, 0, 0};
    long long st[7];
    mirp::OutFile out(out_path);              // opened by the first piece of text, after every refusal
    auto sink = [&](const char* p, size_t len) -> int { return out.write(p, len) ? 0 : fail(c, -8, std::string("cannot write ") + out_path); };
    if (int rc = mirp_device_trim_reads(c, data, (long long)n, name, *o, sink, st, sec)) return rc;
    if (!out.commit()) return fail(c, -8, std::string("cannot write ") + out_path);          // nothing kept: the output is an empty file
    if (stats) for (int i = 0; i < 7; i++) stats[i] = st[i];
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}

extern "C" int mirp_trim_last_paths(const mirp_ctx* c, int64_t out[2]) {
    if (!c || !out) return -1;
    out[0] = c->t_paths[0];
    out[1] = c->t_paths[1];
    return 0;
}
