// C-ABI of the library profile (mirp_libqc_reads, mirp_libqc_last_table): argument checks on the host; libqc_kernels.hip counts,
// walks and tabulates on the device, on the records that trim_kernels.hip parses.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include "mirp_ctx.h"

extern "C" int mirp_libqc_reads(mirp_ctx* c, const char* data, int64_t n, const char* name, const MirpLibqcOpts* o, MirpLibqcFound* found, int64_t stats[4],
                                int64_t raw_len[1025], int64_t cycles[1024 * 6], int64_t insert[1025 * 6], double seconds[6]) {
    if (!c) return -1;
    c->q_have_table = false;
    c->t_paths[0] = c->t_paths[1] = 0;
    if ((!data && n > 0) || n < 0 || !name || !o) return fail(c, -1, "mirp_libqc_reads: bad argument");
    if (o->adapter_len < 0 || o->adapter_len > 64 || o->error_permille < 0 || o->error_permille > 999 || o->min_overlap < 0 || o->min_overlap > 64 ||
        o->sample < 1 || o->sample > (1ll << 26))
        return fail(c, -1, "mirp_libqc_reads: bad options");
    for (int k = 0; k < o->adapter_len; k++)
        if (!std::strchr("ACGTacgt", o->adapter[k]) || o->adapter[k] == 0) return fail(c, -1, "mirp_libqc_reads: the adapter is not ACGT");
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(long long) == sizeof(int64_t), "the tables are passed through as they are");
    if (int rc = mirp_device_libqc_reads(c, data, (long long)n, name, *o, found, (long long*)stats, (long long*)raw_len, (long long*)cycles, (long long*)insert,
                                         seconds))
        return rc;
    c->q_have_table = true;
    return 0;
}

extern "C" int mirp_libqc_last_table(mirp_ctx* c, uint32_t out[1 << 24]) {
    if (!c || !out || !c->q_have_table) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    return mirp_device_libqc_table(c, out);
}
