// The pieces in which the text of a pass leaves the device (site_lines.h): lines i0 .. i1 - 1 whose bytes, toff[i1] - toff[i0], stay within the piece
// size.  Host only: no HIP, no context; the offsets are read through a callable, since they live on the device.
#pragma once

namespace mirp {

// The piece that starts at line i0 < n, where toff[i0] = base and toff[n] = bytes: *i1 = the last index in (i0, n] with toff[*i1] - base <= piece, and
// at least i0 + 1 (a line longer than a piece is a piece of its own); *end = toff[*i1].  read(i, &v) sets v = toff[i] for i0 < i <= n and returns 0;
// its nonzero return ends the search and is returned.
template <class Read>
int text_piece_end(long long i0, long long n, long long base, long long bytes, long long piece, Read read, long long* i1, long long* end) {
    *i1 = n;
    *end = bytes;
    if (bytes - base <= piece) return 0;
    long long a = i0 + 1, z = n - 1;
    while (a < z) {
        const long long md = (a + z + 1) >> 1;
        long long v = 0;
        if (int rc = read(md, &v)) return rc;
        if (v - base <= piece) a = md; else z = md - 1;
    }
    *i1 = a;
    return read(a, end);
}

}  // namespace mirp
