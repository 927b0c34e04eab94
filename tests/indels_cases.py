"""The planted samples of the indels tests, in plain Python and numpy: the probe of tests/test_indels_cpu.py (run there through the model
chain and in tests/test_gpu_indels.py on the device) and the hand-worked cases as small genes with error-free mates."""
import numpy as np

from tests import synth

A, C, G, T = (ord(c) for c in "ACGT")


def tile(hap, L, step, first_strand=0):
    """error-free mates of L bases cut from the haplotype every `step` bases, alternating strands"""
    hap = np.frombuffer(bytes(hap), dtype=np.uint8)
    out = []
    for n, a in enumerate(range(0, len(hap) - L + 1, step)):
        m = hap[a:a + L].copy()
        out.append(synth.revcomp(m) if (n + first_strand) & 1 else m)
    return out


def planted_probe(seed=7):
    """(record, batch): one 700-base record with the run A x 8 at [200, 208) and the repeat CAG x 4 at [400, 412); the sample has one A
    more, one CAG less and GATTACA in front of base 550; 100-base mates every 3 bases on alternating strands"""
    rec = bytearray(synth.random_seq(np.random.default_rng(seed), 700).tobytes())
    rec[199:209] = b"C" + b"A" * 8 + b"G"
    rec[399:413] = b"T" + b"CAG" * 4 + b"T"
    rec[549:551] = b"CG"                                                          # (GATTACA|G: the left block takes the shared G, the raw event sits at 551)
    rec = bytes(rec)
    hap = rec[:204] + b"A" + rec[204:403] + rec[406:550] + b"GATTACA" + rec[550:]
    return rec, synth.batch_from_lists(tile(hap, 100, 3))


def _gene(rng, n):
    return bytearray(synth.random_seq(rng, n).tobytes())


def hand_cases(seed=5, step=3):
    """[(name, record bytes, [mates], the key (x, kind, len, letters) the case plants or None)]: one event per gene, 400 bases in front
    of it and behind it.  Mates are 100 bases every `step` bases across the event, on both strands; the cases with a repeat in front of
    the event take mates long enough to hold it with 60 bases on either side"""
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, rec, hap, key, L=100, at=400):
        lo, hi = max(0, at - L - 20), min(len(hap), at + L + 40)
        cases.append((name, bytes(rec), tile(bytes(hap)[lo:hi], L, step), key))

    def other(*bases):
        return next(c for c in (A, C, G, T) if c not in bases)

    # insertions of 12 (tabled) and 13 (long) unique bases, one with an N
    for n in (12, 13):
        rec = _gene(rng, 800)
        ins = _gene(rng, n)
        ins[-1] = other(rec[399])
        add("ins%d" % n, rec, rec[:400] + ins + rec[400:], (400, 1, n, bytes(ins).decode()) if n == 12 else None)
    rec = _gene(rng, 800)
    add("insN", rec, rec[:400] + b"ACNGT" + rec[400:], None)
    # deletions of min_intron - 1 (tabled) and min_intron (not) bases at min_intron = 20
    for n in (19, 20):
        rec = _gene(rng, 800)
        rec[399] = other(rec[399 + n])
        add("del%d" % n, rec, rec[:400] + rec[400 + n:], (400, 0, n, "*") if n == 19 else None)
    # five other bases where the record has three: closure leaves it open
    rec = _gene(rng, 800)
    junk = bytes([other(rec[400]), other(rec[401]), other(rec[402]), other(rec[402]), other(rec[403])])
    add("complex", rec, rec[:400] + junk + rec[403:], None)
    # Runs in front of the event.  A window inside a run is no unique k-mer, so the blocks on either side reach k - 1 bases into the run
    # and the rest of it is a gap of R = run - 2 (k - 1) read bases (less what is deleted) that only closure can give to the left block:
    # R <= 64 and G >= R.  So through the pipeline a shift is at most 64 + k - 1 bases and an insertion moves only in a run of at
    # most 2 (k - 1).  Three bases less in runs of 82, 83, 84 and 99 bases: shifts of 63, 64, 65 (the edge of the kernel's 64 comparisons
    # per pass) and 80; a base more in a run of 30
    for run in (82, 83, 84, 99):
        rec = _gene(rng, 400)
        rec[-1] = other(A)
        tail = _gene(rng, 400)
        tail[0] = other(A)
        rec = rec + b"A" * run + tail
        add("del_run%d" % run, rec, rec[:400] + b"A" * (run - 3) + rec[400 + run:], (400, 0, 3, "*"), L=run + 120, at=400 + run)
    # A shift that stops at a record N: an N in front of a run, the sample with a C there and one A less.  The left block's unique
    # k-mers lie in front of the N; closure prices the C against the N as not a match and still gives the run's inside to the left
    # block, so the raw event sits at the run's right end and moves left by run - (k - 1) bases, up to the N: shifts of 13 and 33.
    # (One A more cannot be planted this way: it leaves G < R, a complex gap)
    for run in (30, 50):
        rec = _gene(rng, 400)
        tail = _gene(rng, 400)
        tail[0] = other(A)
        rec = rec + b"N" + b"A" * run + tail
        add("del_N_run%d" % run, rec, rec[:400] + b"C" + b"A" * (run - 1) + rec[401 + run:], (401, 0, 1, "*"), L=run + 120, at=401 + run)
    rec = _gene(rng, 400)
    rec[-1] = other(A)
    tail = _gene(rng, 400)
    tail[0] = other(A)
    rec = rec + b"A" * 30 + tail
    add("ins_run30", rec, rec[:400] + b"A" * 31 + rec[430:], (400, 1, 1, "A"), L=150, at=430)
    # a two-base unit more in 12 units: the shift exceeds the event's length, the comparison passes from the inserted bases into the record
    rec = _gene(rng, 400)
    rec[-1] = other(T)
    tail = _gene(rng, 400)
    tail[0] = other(C)
    rec = rec + b"CT" * 12 + tail
    add("unit2x12", rec, rec[:400] + b"CT" * 13 + rec[424:], (400, 1, 2, "CT"), L=150, at=424)
    return cases
