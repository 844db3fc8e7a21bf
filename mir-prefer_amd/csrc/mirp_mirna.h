// The miRNA FASTA of DESIGN.md §14 and the per-miRNA masks of the scans (mirp_targets.cpp), shared by mirp_target_scan and mirp_degradome_scan.
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

// parses path with §14's rules; refusals (-10) name the 1-based record
int parse_mirnas(mirp_ctx* c, const char* path, Mirnas& M);
// the masks of one miRNA (codes cd[0 .. L)); anchored: plus strand only, miRNA position i at window position 32 - i
TgMirna make_mirna(const unsigned char* cd, int L, bool cleavage, bool anchored);

}  // namespace mirp
