"""Inputs shared by the CPU and the GPU tests of the NAT search: planted complementary regions in random transcripts, and the
pinned cases.  A case is (transcripts, options); what it must give is stated where it is used."""
import random

from tests import nats_restatement as R


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def other(rng, base):
    return rng.choice([c for c in "ACGT" if c != base])


def mutate(rng, s, subs=0.0, indels=()):
    """s with a fraction of substitutions and with indels (offset, +n: n bases inserted before it; -n: n bases deleted from it on)."""
    out = [other(rng, c) if rng.random() < subs else c for c in s]
    for at, n in sorted(indels, reverse=True):
        if n > 0:
            out[at:at] = [rng.choice("ACGT") for _ in range(n)]
        else:
            del out[at:at - n]
    return "".join(out)


def plant(rng, A, at_a, B, at_b, region):
    """A with `region` at 0-based at_a and B with its reverse complement at at_b; the bases around both copies are made unable to extend it."""
    rc = R.revcomp(region)
    A = A[:at_a] + region + A[at_a + len(region):]
    B = B[:at_b] + rc + B[at_b + len(rc):]
    # the 12 bases before the region in A face the 12 after rc in B, and the other way round
    A, B = list(A), list(B)
    for t in range(12):
        if at_a - 1 - t >= 0 and at_b + len(rc) + t < len(B):
            B[at_b + len(rc) + t] = other(rng, R.COMPLEMENT[A[at_a - 1 - t]])
        if at_a + len(region) + t < len(A) and at_b - 1 - t >= 0:
            B[at_b - 1 - t] = other(rng, R.COMPLEMENT[A[at_a + len(region) + t]])
    return "".join(A), "".join(B)


def perfect_region(seed=1, n=300, m=280, at_a=70, at_b=95, length=120):
    """Two transcripts with one perfect complementary region: -> (transcripts, (a_start, a_end, b_start, b_end))."""
    rng = random.Random(seed)
    A, B = rand_seq(rng, n), rand_seq(rng, m)
    A, B = plant(rng, A, at_a, B, at_b, rand_seq(rng, length))
    return [A, B], (at_a + 1, at_a + length, at_b + 1, at_b + length)


def seeded_inputs(seed):
    """Random transcripts over ACGTN and AT with planted regions, and random options: what the two statements and the device must agree on."""
    rng = random.Random(seed)
    n_seqs = rng.randint(3, 12)
    seqs = []
    for _ in range(n_seqs):
        kind = rng.random()
        n = rng.choice([0, 1, 11, 12, 13, 47, 48, 49]) if kind < 0.15 else rng.randint(20, 400)
        seqs.append(rand_seq(rng, n, "AT" if kind > 0.8 else "ACGTN" if kind > 0.6 else "ACGT"))
    for _ in range(rng.randint(1, 5)):          # planted regions, some diverged
        a, b = rng.sample(range(n_seqs), 2)
        length = rng.randint(14, 90)
        if len(seqs[a]) <= length + 2 or len(seqs[b]) <= length + 2:
            continue
        region = rand_seq(rng, length)
        copy = mutate(rng, region, subs=rng.choice([0, 0, 0.05, 0.1]), indels=[(rng.randrange(length), rng.choice([-2, -1, 1, 2, 3]))] if rng.random() < 0.4 else ())
        at_a, at_b = rng.randrange(len(seqs[a]) - length), rng.randrange(len(seqs[b]) - len(copy) + 1) if len(seqs[b]) >= len(copy) else 0
        seqs[a] = seqs[a][:at_a] + region + seqs[a][at_a + length:]
        rc = R.revcomp(copy)
        seqs[b] = (seqs[b][:at_b] + rc + seqs[b][at_b + len(rc):])[:max(len(seqs[b]), at_b + len(rc))]
    opts = dict(seed=rng.choice([12, 12, 13, 16]), band=rng.choice([16, 16, 32, 64]), max_occ=rng.choice([1, 2, 5, 200]), min_seeds=rng.choice([1, 1, 2, 3]),
                match=rng.randint(1, 4), mismatch=rng.randint(1, 5), gap=rng.randint(1, 13), min_score=rng.randint(8, 40), min_length=rng.randint(1, 30))
    return seqs, opts


def n_in_seed():
    """A perfect region of 40 nt with an unknown letter at its offset 20 in A: of the 25 seeds of 16 nt the 16 that hold it are gone, 9 are left."""
    seqs, where = perfect_region(seed=2, n=150, m=140, at_a=30, at_b=50, length=40)
    A = seqs[0]
    return [A[:50] + "N" + A[51:], seqs[1]], dict(seed=16, band=16, min_score=30, min_length=10), where


def occurrence_edge():
    """A 16-mer v that occurs three times in the forward sense (transcripts 0, 2 and 3) and rc(v) once (transcript 1): seeds with max_occ 3, not with 2."""
    rng = random.Random(3)
    v = "ACGGTCATTGCAGTCA"
    seqs = [rand_seq(rng, 60) for _ in range(4)]
    seqs[0], seqs[1] = plant(rng, seqs[0], 20, seqs[1], 25, v)
    seqs[2] = seqs[2][:10] + v + seqs[2][26:]
    seqs[3] = seqs[3][:33] + v + seqs[3][49:]
    return seqs, dict(seed=16, band=16, min_score=48, min_length=16)


def two_seeds():
    """A perfect region of 13 nt under k = 12: two seed hits in one bin."""
    seqs, where = perfect_region(seed=4, n=80, m=90, at_a=22, at_b=31, length=13)
    return seqs, dict(seed=12, band=16, min_score=39, min_length=13), where


def end_cell_ties():
    """A region over C and G between flanks of A only, in both transcripts, so that nothing extends it and nothing else pairs.  Twice in A, 8 apart,
    against one copy in B: two maximal cells with different i, the smaller i wins (a 21..50).  Once in A against two copies in B: two maximal
    cells of one i, the smaller j wins, which is the copy nearer to B's 3' end (b 69..98)."""
    rng = random.Random(5)
    region = rand_seq(rng, 30, "CG")
    rc = R.revcomp(region)
    first = ["A" * 20 + region + "A" * 8 + region + "A" * 20, "A" * 30 + rc + "A" * 30]
    second = ["A" * 20 + region + "A" * 20, "A" * 30 + rc + "A" * 8 + rc + "A" * 30]
    return (first, second), dict(seed=12, band=64, min_score=90, min_length=30)


def traceback_ties():
    """Two regions S + x + T between flanks that pair with nothing, under match 3, mismatch 5, gap 2.  First: A holds AA where B' holds A, between
    an S that does not end in A and a T that does not begin with it; the unpaired A can be either one, the diagonal is preferred on the way
    back, so the first A is the unpaired one: 20=1I21=.  Second: A holds A where B' holds T; two gaps (4) cost less than the mismatch (5), and on
    the way back (i - 1, j) comes before (i, j - 1): 20=1D1I20=."""
    S, T = "GTCAGCTAGCATCGATCGTC", "GCATGCTAGTCGATCAGCTG"
    fa, fb = "T" * 15, "A" * 15          # the flanks of A and of B'
    first = [fa + S + "AA" + T + fa, R.revcomp(fb + S + "A" + T + fb)]
    second = [fa + S + "A" + T + fa, R.revcomp(fb + S + "T" + T + fb)]
    return (first, second), dict(seed=12, band=16, match=3, mismatch=5, gap=2, min_score=60, min_length=30)


def two_copies_in_b():
    """One region of A against two copies in B, 150 apart: two records."""
    rng = random.Random(6)
    region = rand_seq(rng, 50)
    A, B = rand_seq(rng, 200), rand_seq(rng, 400)
    A, B = plant(rng, A, 60, B, 40, region)
    A, B = plant(rng, A, 60, B, 240, region)
    return [A, B], dict(seed=12, band=16, min_score=100, min_length=40)


def two_bins():
    """A region of 40 + 40 nt with one base deleted from B's copy between the halves, placed so that the halves' diagonals are 127 and 128: the bins 1
    and 2 of W = 64 are both candidates, their bands both hold the whole region, and the selection leaves one record."""
    rng = random.Random(7)
    region = rand_seq(rng, 81)
    copy = region[:40] + region[41:]
    A, B = rand_seq(rng, 200), rand_seq(rng, 200)
    # the first half's k-mers lie on diagonal e = at_a + at_b + 79, the second half's on e + 1 (e = x + p + k - 3 for the 1-based forward
    # positions x in A and p in B of a k-mer and its reverse complement)
    k, at_a, at_b = 12, 10, 38
    rc = R.revcomp(copy)
    A = A[:at_a] + region + A[at_a + 81:]
    B = B[:at_b] + rc + B[at_b + 80:]
    return [A, B], dict(seed=k, band=64, min_score=150, min_length=60)


def drifting_region(W, drift, seed=8):
    """A region whose first 30 nt seed the last diagonal of a bin of W, followed by 60 nt that `drift` bases inserted in A move `drift` diagonals up:
    within the band up to drift = W, past its edge from W + 1 on.  For a small gap penalty, under which the alignment bridges the insertion.
    -> transcripts."""
    rng = random.Random(seed * 1000 + drift)
    head, tail = rand_seq(rng, 30), rand_seq(rng, 60)
    in_a = head + rand_seq(rng, drift) + tail
    in_b = R.revcomp(head + tail)
    A, B = rand_seq(rng, 120 + 3 * W), rand_seq(rng, 120 + 3 * W)
    at_a = 20
    at_b = 30 + (W - 1 - (at_a + 30 + 89)) % W          # the head's diagonal is e = at_a + at_b + 89
    A = A[:at_a] + in_a + A[at_a + len(in_a):]
    B = B[:at_b] + in_b + B[at_b + len(in_b):]
    return [A, B]


def length_ladder(k, W, seed=9):
    """Transcripts of 1, k-1, k, k+1, W-1, W, W+1, 3W-1, 3W, 3W+1 nt, every one the reverse complement of a prefix of one long transcript, which
    comes last: each is one region against it."""
    rng = random.Random(seed)
    long_one = rand_seq(rng, 3 * W + 40)
    lengths = [1, k - 1, k, k + 1, W - 1, W, W + 1, 3 * W - 1, 3 * W, 3 * W + 1]
    return [R.revcomp(long_one[7:7 + n]) for n in lengths] + [long_one]


def corner_seeds(k, W, seed=10):
    """Two pairs whose only seeds are the first k-mer of A with the last of B' (and the other way round): the lowest and the highest diagonal a
    seed can lie on, e = k - 1 and e = n + m - k - 1, in the first and the last bins, whose bands lie partly outside the matrix."""
    rng = random.Random(seed)
    v, w = rand_seq(rng, k), rand_seq(rng, k)
    A = v + rand_seq(rng, 2 * W + 11) + w
    # B' = revcomp(B) must end with v and start with w: B = revcomp(B') starts with rc(v) and ends with rc(w)
    B = R.revcomp(v) + rand_seq(rng, 2 * W + 29) + R.revcomp(w)
    return [A, B]
