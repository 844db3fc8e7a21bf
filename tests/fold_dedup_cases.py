"""Inputs of the fold-dedup tests (test_fold_dedup_cpu.py, test_fold_dedup_gpu.py): small genomes with read stacks placed so that the candidate
stage writes windows that repeat each other byte for byte, or nearly do.  No GPU is needed to build them.

A case is a dict: contigs [(name, uint8 array)], alns (ALN_DTYPE, sorted), order, cut, gap, L (PRECURSOR_LEN of the candidate stage), span and
max_lines of the fold.  `window_seqs` gives the byte strings of its windows from the CPU oracle, `first_index_map` the restatement of the map the
device builds: for every window the first index of its byte string if that is an earlier window, else -1."""
import numpy as np

from mir_prefer_amd import synth

CUT, GAP = 10, 100


def _random_contig(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, n)].copy()


def _stack(tid, pos, strand):
    """three isomiRs on one strand: a read adds min(depth, cutoff) to the coverage and the threshold is strict, so one read never makes a peak"""
    return [(tid, pos, 60, 21, strand, 0), (tid, pos, 20, 22, strand, 0), (tid, pos + 1, 15, 21, strand, 0)]


def _wide(tid, pos, strand):
    """four overlapping stacks: a locus of more than 60 nt, which gets one centred window of L nt instead of an L / R pair of L + 25"""
    return [r for k in range(4) for r in _stack(tid, pos + 16 * k, strand)]


def _case(contigs, reads, L, span=None, max_lines=96):
    alns = np.array(reads, dtype=synth.ALN_DTYPE) if reads else np.zeros(0, dtype=synth.ALN_DTYPE)
    alns = alns[np.lexsort((alns["pos"], alns["tid"]))] if len(alns) else alns      # stable: equal positions keep their order
    names = [n for n, _ in contigs]
    return {"contigs": contigs, "alns": alns, "order": np.argsort(np.array(names, dtype=object), kind="stable").astype(np.int32), "cut": CUT, "gap": GAP,
            "L": L, "span": span or L, "max_lines": max_lines, "names": names}


def _plant(seq, at, segment):
    segment = np.frombuffer(segment, dtype=np.uint8) if isinstance(segment, bytes) else segment
    n = min(len(segment), len(seq) - at)      # a segment at a contig end is cut off there
    seq[at:at + n] = segment[:n]


def short_both_strands():
    """one locus of 53 nt with a peak on either strand (a peak's strand is the strand of most of its reads): (+,L) (-,L) (+,L) (+,R) (-,L) (-,R), the generator's own two duplicates"""
    rng = np.random.RandomState(1401)
    c = _random_contig(rng, 3000)
    return _case([("c1", c)], _stack(0, 1500, 0) + _stack(0, 1530, 1), 100)


def planted_segment():
    """a 340-nt segment at three places, one of them on a second contig, reads at equal offsets: every L / R window lies inside the segment, so the
    second and third copies' windows repeat the first's at other coordinates.  Near misses that must not merge: a fourth copy whose R window differs
    in its last base, a fifth whose R window is clipped by the contig end (a prefix of the full one), a sixth that is soft-masked."""
    rng = np.random.RandomState(1402)
    seg = _random_contig(rng, 340)
    c1, c2 = _random_contig(rng, 6000), _random_contig(rng, 2600)
    L, off = 100, 160                       # the stack starts at segment offset 160: L window = [82, 207), R window = [135, 260) of the segment
    places = [(0, 700), (0, 1900), (1, 500), (0, 3100), (1, 2600 - 240), (0, 4300)]
    reads = []
    for k, (tid, at) in enumerate(places):
        _plant((c1, c2)[tid], at, seg if k != 5 else np.frombuffer(seg.tobytes().lower(), dtype=np.uint8))
        reads += _stack(tid, at + off + 1, 0)        # 1-based positions
    c1[3100 + 259] = ord("A") if c1[3100 + 259] != ord("A") else ord("C")      # the last base of the fourth copy's R window
    return _case([("c1", c1), ("c2", c2)], reads, L)


def tandem_over_line_capacity():
    """a (GTGG)n stretch at two places in the same phase under equal read stacks: its windows give more structure lines than max_lines = 8"""
    rng = np.random.RandomState(1403)
    c = _random_contig(rng, 4000)
    reads = []
    for at in (800, 2400):
        _plant(c, at, b"GTGG" * 85)
        reads += _stack(0, at + 161, 0)
    reads += _stack(0, 3500, 0)            # an ordinary locus behind them
    return _case([("c1", c)], reads, 100, max_lines=8)


def microsatellite_for_the_dense_pass():
    """an (AT)n stretch at two places under wide loci: two equal windows of 350 nt whose split candidates overflow the candidate pool"""
    rng = np.random.RandomState(1404)
    c = _random_contig(rng, 4000)
    reads = []
    for at in (600, 2200):
        _plant(c, at, b"AT" * 300)
        reads += _wide(0, at + 261, 0)
    reads += _stack(0, 3500, 0)
    return _case([("c1", c)], reads, 350, span=300)


def gc_for_the_generic_kernel():
    """G175 C175 at two places: two equal windows of 350 nt whose energies leave the 16-bit range of the LDS-resident kernels"""
    rng = np.random.RandomState(1405)
    c = _random_contig(rng, 4000)
    reads = []
    for at in (600, 2200):
        _plant(c, at, b"G" * 300 + b"C" * 300)
        reads += _wide(0, at + 261, 0)
    reads += _stack(0, 3500, 0)
    return _case([("c1", c)], reads, 350, span=300)


def every_window_a_copy():
    """one segment at seven places under wide loci: seven windows, all equal to the first"""
    rng = np.random.RandomState(1406)
    seg = _random_contig(rng, 200)
    c = _random_contig(rng, 4000)
    reads = []
    for k in range(7):
        _plant(c, 300 + 500 * k, seg)
        reads += _wide(0, 300 + 500 * k + 61, 0)
    return _case([("c1", c)], reads, 100)


def no_duplicate():
    """nine loci on one strand each in a random genome"""
    rng = np.random.RandomState(1407)
    c = _random_contig(rng, 6000)
    reads = []
    for k in range(9):
        reads += (_wide if k % 3 == 0 else _stack)(0, 400 + 600 * k, k & 1)
    return _case([("c1", c)], reads, 100)


def empty():
    rng = np.random.RandomState(1408)
    return _case([("c1", _random_contig(rng, 2000))], [], 100)


def spread_over_chunks():
    """the planted segment's windows and the generator's duplicates, 18 windows: with chunks and sub-batches of two or three windows a duplicate
    and its representative seldom share one"""
    a, b = planted_segment(), short_both_strands()
    c1 = np.concatenate([a["contigs"][0][1], b["contigs"][0][1]])
    shift = len(a["contigs"][0][1])
    reads = [tuple(r) for r in a["alns"].tolist()] + [(0, r[1] + shift) + tuple(r[2:]) for r in b["alns"].tolist()]
    return _case([("c1", c1), a["contigs"][1]], reads, 100)


CASES = {"short-both-strands": short_both_strands, "planted-segment": planted_segment, "tandem-over-line-capacity": tandem_over_line_capacity,
         "microsatellite-dense": microsatellite_for_the_dense_pass, "gc-generic": gc_for_the_generic_kernel, "every-window-a-copy": every_window_a_copy,
         "no-duplicate": no_duplicate, "empty": empty, "spread-over-chunks": spread_over_chunks}


# what a case is there for, under the default model: (fallbacks, dense, overflow) of its fold at least, and the map
EXPECT = {"short-both-strands": ((0, 0, 0), [-1, -1, 0, -1, 1, -1]),
          "planted-segment": ((0, 0, 0), [-1, -1, 0, 1, 0, -1, -1, -1, 0, 1, 0, -1]),
          "tandem-over-line-capacity": ((0, 0, 4), [-1, -1, 0, 1, -1, -1]),
          "microsatellite-dense": ((0, 2, 0), [-1, 0, -1, -1]),
          "gc-generic": ((2, 0, 0), [-1, 0, -1, -1]),
          "every-window-a-copy": ((0, 0, 0), [-1, 0, 0, 0, 0, 0, 0]),
          "no-duplicate": ((0, 0, 0), [-1] * 15),
          "empty": ((0, 0, 0), []),
          "spread-over-chunks": ((0, 0, 0), [-1, -1, 0, 1, 0, -1, -1, -1, -1, -1, 8, -1, 9, -1, 0, 1, 0, -1])}



def oracle_windows(oracle, case):
    """the CPU oracle's candidate stage on the case -> its `win` dict"""
    lens = np.array([len(s) for _, s in case["contigs"]], dtype=np.int64)
    _, peaks = oracle.coverage_peaks(case["alns"], lens, case["cut"])
    return oracle.make_windows(peaks, case["alns"], case["contigs"], case["order"], case["gap"], case["L"], case["cut"] * 0.5)


def window_seqs(win):
    return [win["seq"][b["seq_off"]:b["seq_off"] + b["seq_len"]].tobytes() for b in win["windows"]]


def first_index_map(seqs):
    """dup_of as the issue defines it: the lowest earlier index with the same bytes, -1 for the first window of every distinct byte string"""
    first, out = {}, np.full(len(seqs), -1, dtype=np.int32)
    for w, s in enumerate(seqs):
        if first.setdefault(s, w) != w:
            out[w] = first[s]
    return out
