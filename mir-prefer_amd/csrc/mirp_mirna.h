// The miRNA FASTA of DESIGN.md §14 and the per-miRNA masks of the scans (mirp_targets.cpp), shared by mirp_target_scan, mirp_degradome_scan
// and mirp_annotate_scan.
#pragma once
#include <string>
#include <vector>
#include "mirp_ctx.h"

namespace mirp {

struct Mirnas {
    std::string names;                  // concatenated
    std::vector<long long> noff{0};
    std::vector<unsigned char> codes;   // 32 per miRNA: 0..3 = A C G U, 4 = unknown
    std::vector<int> lens;
};

// parses path with §14's rules and appends its records to M; refusals (-10) name the 1-based record.  With `skipped` (the known sequences of
// §19) a record whose length is outside 12..32 is dropped and counted there instead of refused, and the caller bounds the number of records.
int parse_mirnas(mirp_ctx* c, const char* path, Mirnas& M, long long* skipped = nullptr);
// the masks of one miRNA (codes cd[0 .. L)); anchored: plus strand only, miRNA position i at window position 32 - i
TgMirna make_mirna(const unsigned char* cd, int L, bool cleavage, bool anchored);

}  // namespace mirp
