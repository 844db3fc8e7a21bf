// trigger_kernels.hip: the trigger scan of DESIGN.md §29 over packed genome contigs (mirp_triggers.cpp parses the files and checks the loci).
// pk / amb / cst / cstart as mirp_device_target_scan takes them; mi: the masks of make_mirna with the cleavage rule; mlen: the miRNAs' lengths;
// loci: checked against the contigs.  stats = {miRNAs, interval bases, sites, windows evaluated, records of the phase length (0 when there is no
// site: the units are not built then), units kept}; seconds = {upload, site scan + sort, units, windows + download}.
#pragma once
#include <vector>
#include "mirp_ctx.h"

int mirp_device_trigger_scan(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                             const std::vector<unsigned long long>& cstart, const std::vector<TgMirna>& mi, const std::vector<unsigned char>& mlen,
                             const MirpTriggerLocus* loci, long long n_loci, const MirpTriggerOpts& o, const int32_t* kmin, MirpTrigger** triggers,
                             int64_t* n_triggers, int64_t* site_counts, long long stats[6], double seconds[4]);
