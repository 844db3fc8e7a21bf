// FASTA reading shared by the C-ABI translation units: whole-file reads, the universal-newline line walk, and the parse and 2-bit packing of
// reference / target FASTA files (mirp_align_index, mirp_target_scan).
#pragma once
#include <cstdio>
#include <string>
#include <vector>
#include "mirp_ctx.h"

namespace mirp {

inline bool fa_ws(unsigned char ch) { return ch == 32 || (ch >= 9 && ch <= 13) || (ch >= 0x1c && ch <= 0x1f); }   // str.strip() / str.split(), ASCII

int read_whole(mirp_ctx* c, const char* path, std::string& buf);

// The output file of a run: there when the run ended well and otherwise not, not even one an earlier run left at the path.  It is opened by
// open() or the first write(); commit() closes it (an unopened one as an empty file); discard() closes and removes it, and a guard that goes
// without commit() discards.  open, write and commit return false when the file cannot be written.
class OutFile {
    std::string path_;
    FILE* f_ = nullptr;
    bool committed_ = false;

  public:
    explicit OutFile(const char* path) : path_(path) {}
    OutFile(const OutFile&) = delete;
    OutFile& operator=(const OutFile&) = delete;
    ~OutFile() { if (!committed_) discard(); }
    bool open() { return f_ || (f_ = std::fopen(path_.c_str(), "wb")) != nullptr; }
    bool write(const char* p, size_t len) { return open() && (len == 0 || std::fwrite(p, 1, len, f_) == len); }
    bool commit() {
        if (!open()) return false;
        committed_ = std::fclose(f_) == 0;
        f_ = nullptr;
        return committed_;
    }
    void discard() {
        if (f_) std::fclose(f_);
        f_ = nullptr;
        committed_ = false;
        std::remove(path_.c_str());
    }
};

// Calls fn(raw, begin, end) for every line of buf (ends at \n, \r\n or a lone \r: Python's universal newlines; an empty line between \r and \n is
// harmless to every parser here).  [begin, end) is the line stripped of surrounding whitespace; raw is its first byte.  fn returns nonzero to stop.
template <class F>
int for_lines(const std::string& buf, F fn) {
    const char* p = buf.data();
    const char* end = p + buf.size();
    while (p < end) {
        const char* q = p;
        while (q < end && *q != '\n' && *q != '\r') q++;
        const char* a = p;
        const char* b = q;
        while (a < b && fa_ws((unsigned char)*a)) a++;
        while (b > a && fa_ws((unsigned char)b[-1])) b--;
        if (int rc = fn(p, a, b)) return rc;
        p = q < end ? q + 1 : q;
    }
    return 0;
}

// first word of a header line (after '>')
inline std::string first_word(const char* raw, const char* b) {
    const char* a = raw + 1;
    while (a < b && fa_ws((unsigned char)*a)) a++;
    const char* z = a;
    while (z < b && !fa_ws((unsigned char)*z)) z++;
    return std::string(a, z);
}

// Reference / target FASTA files parsed in order and packed.  Positions are global over the concatenation of the contigs (< 2^32).
//   pk   2-bit bases (A C G T in either case = 0..3), 16 per u32, base i at bits 2 (i % 16); (total + 15) / 16 + 2 words
//   amb  1 bit per position: any other character, and every position past the end; cst: 1 bit per contig start; (total + 31) / 32 + 2 words each
//   names / lens per contig; blob = the names concatenated, noff[0 .. n] their offsets, cstart[0 .. n] the contigs' first positions (cstart[n] = total)
struct PackedFasta {
    std::vector<unsigned> pk, amb, cst;
    std::vector<std::string> names;
    std::vector<long long> lens;
    std::string blob;
    std::vector<long long> noff;
    std::vector<unsigned long long> cstart;
    long long total = 0;
};
// The contig name is the first word of the header; contigs of length 0 are dropped with a warning on stderr; duplicate names, empty names and
// 2^32 bases or more are refused (-10).
int pack_fasta(mirp_ctx* c, const char* const* paths, int n_paths, PackedFasta& out);

}  // namespace mirp
