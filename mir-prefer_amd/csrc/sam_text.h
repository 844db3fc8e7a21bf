// What the SAM tokenizers share (mirp_ingest.cpp, mirp_isomirs.cpp): the mapped file, the contig name table, the header of a file (@SQ table,
// sample name, start of the body), the cut of a body into per-thread chunks and the fields every record is read with (flag, read-id depth, contig).
#pragma once
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace samtext {

struct Mapped {
    const char* p = nullptr;
    size_t n = 0;
    int fd = -1;
    bool open(const char* path) {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) return false;
        n = (size_t)st.st_size;
        if (n == 0) { p = ""; return true; }
        void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return false;
        (void)madvise(m, n, MADV_SEQUENTIAL);
        p = (const char*)m;
        return true;
    }
    ~Mapped() {
        if (p && n) munmap((void*)p, n);
        if (fd >= 0) ::close(fd);
    }
};

// contig name -> index: open addressing over FNV-1a of the name bytes (no allocation per line)
struct NameTable {
    std::vector<std::string> names;
    std::vector<int> slot;      // -1 = empty
    unsigned mask = 0;
    static unsigned hash(const char* s, size_t n) { unsigned h = 2166136261u; for (size_t k = 0; k < n; k++) { h ^= (unsigned char)s[k]; h *= 16777619u; } return h; }
    void build() {
        unsigned cap = 16;
        while (cap < 4 * names.size() + 8) cap <<= 1;
        slot.assign(cap, -1); mask = cap - 1;
        for (size_t t = 0; t < names.size(); t++) {
            unsigned h = hash(names[t].data(), names[t].size()) & mask;
            while (slot[h] >= 0) { if (names[slot[h]] == names[t]) break; h = (h + 1) & mask; }
            if (slot[h] < 0) slot[h] = (int)t;      // a repeated @SQ name keeps its first index
        }
    }
    int find(const char* s, size_t n) const {
        unsigned h = hash(s, n) & mask;
        while (slot[h] >= 0) {
            const std::string& c = names[slot[h]];
            if (c.size() == n && std::memcmp(c.data(), s, n) == 0) return slot[h];
            h = (h + 1) & mask;
        }
        return -1;
    }
};

inline bool parse_uint(const char* s, const char* e, long* out) {
    if (s >= e) return false;
    long v = 0;
    for (; s < e; s++) { const unsigned d = (unsigned)(*s - '0'); if (d > 9) return false; v = v * 10 + d; if (v > 0x7fffffffffffL / 16) return false; }
    *out = v;
    return true;
}

// depth of a read id: ^\S+_x([0-9]+)  (get_read_depth_fromID_as_string, MP:242-253): greedy \S+ -> the LAST "_x" that digits follow; -1 = none
inline long read_id_depth(const char* id, const char* ide) {
    for (const char* t = ide - 1; t > id + 2; t--) {
        if (*t >= '0' && *t <= '9' && t[-1] == 'x' && t[-2] == '_') {
            long v = 0;
            for (const char* d = t; d < ide && *d >= '0' && *d <= '9'; d++) { v = v * 10 + (*d - '0'); if (v > 0xffffffffL) { v = 0xffffffffL; break; } }
            return v;
        }
    }
    return -1;
}

// CPUs this process may actually use: the affinity mask and the cgroup quota, not the box's core count (a container on a 256-thread host is often granted
// 8 or 16; 256 tokenizer threads on 16 CPUs only add switches).
inline int usable_cpus() {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0 && k < n) n = k; }
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = ""; long long per = 0;
        if (std::fscanf(f, "%31s %lld", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0) {
            const int k = (int)((std::atoll(q) + per - 1) / per);
            if (k > 0 && k < n) n = k;
        }
        std::fclose(f);
    }
    return n;
}

// The header of one mapped file: with `first`, its @SQ lines fill tab.names / lens (get_length_from_sam, MP:500-509: @SQ order of the FIRST file
// defines the contig indices); *sample = the sample name from the first alignment line (get_samplename_from_sam, MP:3300-3308).  -> the start of the body.
inline const char* read_header(const char* b, const char* e, bool first, NameTable* tab, std::vector<int64_t>* lens, std::string* sample) {
    const char* s = b;
    while (s < e && *s == '@') {
        const char* le = (const char*)memchr(s, '\n', (size_t)(e - s));
        if (!le) le = e;
        if (first && le - s > 3 && s[1] == 'S' && s[2] == 'Q') {
            std::string line(s, le), sn;
            long ln = -1;
            size_t p = 0;
            while (p < line.size()) {
                size_t t = line.find('\t', p);
                if (t == std::string::npos) t = line.size();
                if (line.compare(p, 3, "SN:") == 0) sn = line.substr(p + 3, t - p - 3);
                if (line.compare(p, 3, "LN:") == 0) ln = strtol(line.c_str() + p + 3, nullptr, 10);
                p = t + 1;
            }
            while (!sn.empty() && (sn.back() == '\r' || sn.back() == '\n')) sn.pop_back();
            if (!sn.empty() && ln >= 0) { tab->names.push_back(sn); lens->push_back(ln); }
        }
        s = le < e ? le + 1 : e;
    }
    const char* t = s;
    while (t < e && *t != '\t' && *t != '\n') t++;
    std::string id(s, t), sname;
    std::vector<size_t> us;
    for (size_t k = 0; k < id.size(); k++) if (id[k] == '_') us.push_back(k);
    if (us.size() >= 2) sname = id.substr(0, us[us.size() - 2]);
    *sample = sname;
    return s;
}

// [s, e) cut at line starts into at most n_threads chunks of at least 1 MiB: cuts[0 .. nt]
inline std::vector<const char*> cut_body(const char* s, const char* e, int n_threads) {
    const size_t body = (size_t)(e - s);
    const int nt = (int)std::min<size_t>((size_t)n_threads, std::max<size_t>(1, body / (1 << 20)));
    std::vector<const char*> cuts(nt + 1);
    cuts[0] = s; cuts[nt] = e;
    for (int k = 1; k < nt; k++) {
        const char* c = s + body * k / nt;
        const char* le = (const char*)memchr(c, '\n', (size_t)(e - c));
        cuts[k] = le ? le + 1 : e;
    }
    return cuts;
}

}  // namespace samtext
