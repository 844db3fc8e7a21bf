"""The window families of tests/test_fold_diag_idx_gpu.py and, without a GPU, the properties that make each of them a case of the fill kernel's
diagonal loop: what a wave does once per barrier interval whatever the diagonal holds, the intervals whose list of paired cells is empty, and the
lane fill (idle lanes of a diagonal's last block of 64 paired cells take the first cells of the next diagonal) from the first interior-loop diagonal on.

Everything here is computed from the sequences alone -- the paired cells of a diagonal are the (i, i + d) whose bases can pair -- except the energy
bound, which comes from the CPU oracle's MFEs: a window whose energies leave the kernel's 16-bit tables (FIN_LIMIT in fold_lds_common.h: |c| <= 28000)
is handed to the generic kernel and would prove nothing about the candidate-pool pass.  No family here is G/C-only; the bound is asserted for the
longest windows of every family, whose energies are the largest."""
import random

PAIRS = {("A", "U"), ("U", "A"), ("G", "C"), ("C", "G"), ("G", "U"), ("U", "G")}
FIN_LIMIT = 28000      # fold_lds_common.h
MAXLOOP = 30
FIRST_A1 = 6           # first diagonal with interior loops (TURN + 3)


def two_letter(seed, ab, n):
    r = random.Random(seed)
    return "".join(r.choice(ab) for _ in range(n))


def uniform(seed, n):
    return two_letter(seed, "ACGU", n)


def ends_only(n):
    """a window whose only possible pair joins its two ends"""
    return "G" + "A" * (n - 2) + "C"


def short_windows():
    """one uniform window of every length 5 .. 80"""
    return [uniform(5000 + n, n) for n in range(5, 81)]


SHORT_SPANS = [300, 40] + list(range(6, 13))


def long_windows():
    """n = 197 .. 200 (the cell count n - d crosses multiples of 64 on the first diagonals) and 320 .. 350: a uniform and a G/U-only window each"""
    out = []
    for n in list(range(197, 201)) + list(range(320, 351)):
        out += [uniform(6000 + n, n), two_letter(6500 + n, "GU", n)]
    return out


def quadruples():
    """16 x (long GC-rich, poly-A, 5 nt, long uniform): folded 40 times over in this order, several windows per workgroup"""
    r = random.Random(1600)
    seqs = []
    for _ in range(16):
        n1, n2 = r.randint(300, 350), r.randint(280, 350)
        gc_rich = "".join(r.choice("GC") if r.random() < 0.65 else r.choice("AU") for _ in range(n1))
        seqs += [gc_rich, "A" * r.randint(150, 350), uniform(r.randrange(1 << 30), 5), uniform(r.randrange(1 << 30), n2)]
    return seqs


def unpaired_windows():
    """poly-A and pairs-at-the-two-ends-only windows of every length 64 .. 350"""
    out = []
    for n in range(64, 351):
        out += ["A" * n, ends_only(n)]
    return out


def gu_windows():
    """a G/U-only window of every length 64 .. 350: half of the cells of every diagonal pair"""
    return [two_letter(7000 + n, "GU", n) for n in range(64, 351)]


def rampup_windows():
    """uniform windows of 30 .. 45 nt, eight of each length: the whole fold lies on the first diagonals (6 .. 35), where not every loop size exists yet"""
    return [uniform(8000 + 16 * n + k, n) for n in range(30, 46) for k in range(8)]


FAMILIES = {"short": short_windows, "long": long_windows, "quadruples": quadruples, "unpaired": unpaired_windows, "gu": gu_windows, "rampup": rampup_windows}


def paired_counts(s, span):
    """{d: paired cells of diagonal d} for the diagonals with interior loops, 6 .. D"""
    n = len(s)
    D = min(span - 1, n - 1)
    return {d: sum((s[i], s[i + d]) in PAIRS for i in range(n - d)) for d in range(FIRST_A1, D + 1)}


def blocks_per_interval(counts, from_first):
    """Blocks of 64 paired cells per diagonal under the lane fill: the idle lanes of a diagonal's last block take the first cells of the next diagonal,
    from the first interior-loop diagonal on (from_first) or once every loop size exists (d - 6 >= MAXLOOP).  Returns ({d: blocks}, cells that went ahead
    on a diagonal d with d - 6 < MAXLOOP)."""
    done, out, ahead_early = 0, {}, 0
    last = max(counts) if counts else 0
    for d in sorted(counts):
        rem = counts[d] - done
        nblk = (rem + 63) // 64
        out[d] = nblk
        mix = (from_first or d - FIRST_A1 >= MAXLOOP) and d + 1 <= last
        done = min(nblk * 64 - rem, counts[d + 1]) if mix else 0
        if done and d - FIRST_A1 < MAXLOOP:
            ahead_early += done
    return out, ahead_early


def test_every_family_stays_inside_the_16_bit_tables(oracle):
    for name, make in FAMILIES.items():
        seqs = make()
        assert not any(set(s) <= set("GC") and len(s) > 5 for s in seqs), name      # no G/C-only family
        worst = 0
        for s in sorted(seqs, key=len)[-6:]:
            worst = max(worst, abs(oracle.lfold(s, 300)["mfe"]))
        print("%s: %d windows, largest |MFE| of the six longest %d (limit %d)" % (name, len(seqs), worst, FIN_LIMIT))
        # Every finite cell of c is the energy of a structure closed by a pair, which the exterior loop can take as it stands for its end terms (terminal
        # AU, mismatch: below 100), so no cell lies further below the MFE than that; positive cells are single loops (a few thousand at most).  An fML cell
        # is a row of k such structures at ML_intern each (-90 in this model): with k <= n / 7 = 50 it lies less than 5,000 below the MFE, against a table
        # limit of -31,500.  4,000 between the largest |MFE| and FIN_LIMIT covers both.
        assert worst + 4000 < FIN_LIMIT, (name, worst)


def test_unpaired_windows_have_only_empty_intervals():
    for s in unpaired_windows():
        c = paired_counts(s, 300)
        assert sum(c.values()) <= 1, s      # (the ends-only pair lies on diagonal n - 1, inside the fill for n <= 300)
        blocks, _ = blocks_per_interval(c, True)
        assert sum(1 for b in blocks.values() if b == 0) >= len(blocks) - 1


def test_gu_windows_reach_three_blocks_and_mix_on_the_first_diagonals():
    three = mixed = 0
    for s in gu_windows():
        c = paired_counts(s, 300)
        blocks, early = blocks_per_interval(c, True)
        three += any(v >= 129 for v in c.values()) and max(blocks.values()) >= 3
        mixed += early > 0
    assert three >= 50 and mixed == len(gu_windows()), (three, mixed)


def test_uniform_windows_have_intervals_whose_list_went_ahead():
    """rem == 0 with cells on the diagonal: the lanes that went ahead used the list up"""
    n_empty = 0
    for s in long_windows()[0::2] + quadruples()[3::4]:
        c = paired_counts(s, 300)
        blocks, _ = blocks_per_interval(c, True)
        n_empty += sum(1 for d, b in blocks.items() if b == 0 and c[d] > 0)
    assert n_empty >= 100, n_empty


def test_rampup_windows_lie_on_the_first_diagonals_and_mix_there():
    changed = 0
    for s in rampup_windows():
        c = paired_counts(s, 300)
        assert max(c) <= 44      # (up to n = 36 no diagonal lies past the first 30)
        _, early = blocks_per_interval(c, True)
        _, late = blocks_per_interval(c, False)
        assert late == 0
        changed += early > 0
    assert changed >= len(rampup_windows()) * 3 // 4, changed


def test_short_windows_cover_the_first_wraps_of_the_buffer_cycles():
    """The kernel's buffers turn with d % 3 (keys, lists, DML rows), d % 6 (list lengths) and d & 31 (ring rows; the rows with (d & 31) < 10 have a mirror):
    windows of 5 .. 80 nt end their fill on every diagonal 4 .. 79 -- before the first wrap of each cycle, on it and past it -- and the spans 6 .. 12
    end it on the diagonals 5 .. 11."""
    last = {min(300 - 1, len(s) - 1) for s in short_windows()}
    assert last == set(range(4, 80))
    assert {32, 33, 41, 42} <= last and set(range(4, 12)) <= last
    assert {min(sp - 1, 79) for sp in SHORT_SPANS} == {79, 39} | set(range(5, 12))
