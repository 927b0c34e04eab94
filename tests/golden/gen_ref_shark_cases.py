#!/usr/bin/env python3
"""Generates tests/golden/ref_shark_cases.npz by running the REAL reference CLI (oracle/_ref/shark_ref, built by
`make -C oracle ref` where the reference tree is present: main.cpp compiled in place against our sdsl stand-in) with
`-t 1` on a fixed grid of whole-program cases.  The file holds each case's inputs (FASTA, one or two FASTQ, the options)
and the reference's outputs (stdout ssv, both output FASTQ); tests/test_reference_shark.py replays them through the oracle
and tests/test_gpu_reference_cases.py through the HIP path.  Inputs are stored, not seeds.

The grid (tests/ref_cases.py builds the inputs) is aimed at what the example truth files do not pin:
  k          1 2 3 4 5 11 15 16 17 18 21 30 31 (every gene holds a palindromic k-mer for even k)
  filter     saturated (1, 64, 1000 bits), not powers of two (12 345, 2^20+1, 3 000 017), 2^16 ... 2^26, and a few
             cases at 2^33 (`-b 1`, no override: the product CLI replays those)
  references shared halves and exact copies (ties), a reverse-complement gene, a contained gene, a repeat inside a gene,
             records shorter than k / all N / empty (quirk A: they still take a gene number), lower case, IUPAC letters
             and '.', multi-line records with descriptions, more than 65 536 records (uint16 gene numbers wrap)
  options    c in {0, 1/3, 0.5, 0.6, 2/3, 0.75, 0.9, 1} with c*len on, just below and just above the covered bases;
             -s with and without ties; -q in {0 1 20 40 93 94 95 127 128 222 223 256 300} (`char` wrap) with
             qualities on and either side of the threshold
  reads      empty, shorter than k, >= k bytes but < k valid bases, N runs cutting k-mers, N first/last, lower case,
             reverse strand, substitutions, chimeras, off-target; single-end and paired (unequal and empty mates);
             lengths 31-33, 63-65, 127-129, 150, 151, 250, 300, 600, 1000 in mixed batches
  batches    the kernel is chosen per batch from its longest read, and the uniform kernels only for batches of one length:
             uniform batches of every length in UNIFORM, single-end and paired (U = 2 ... 10 and the long path; 2^24 bits,
             where a tiny index also has the exact table in LDS, or a size that is not a power of two), and ragged
             batches whose longest read sits on each unroll boundary (RAGGED_MAX)

Excluded inputs, on which the reference itself is undefined:
  * bytes >= 0x80 and NUL in FASTA or FASTQ: `to_int[seq[p]]` indexes with a plain `char`, and mask_seq walks qual.l
    over a string that a NUL has cut short;
  * quality lines shorter than their sequence;
  * under -q, bytes below '@' in reads (a masked byte, base - 64, would index `to_int` below 0)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import ref_cases as rc  # noqa: E402

SHARK_REF = os.path.join(ROOT, "oracle", "_ref", "shark_ref")
KS = (1, 2, 3, 4, 5, 11, 15, 16, 17, 18, 21, 30, 31)
CS = (0.0, 1 / 3, 0.5, 0.6, 2 / 3, 0.75, 0.9, 1.0)
QS = (0, 1, 20, 40, 93, 94, 95, 127, 128, 222, 223, 256, 300)
LENGTHS = (31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 151, 250, 300, 600, 1000)
SHORT = (40, 60, 75, 100, 150)
# uniform batches at k = 17: single-end slots L - 16, paired 8*ceil(L/8) + L - 16; 64 slots per unroll step, 640 at most
UNIFORM = (31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 151, 250, 300, 350, 500, 600)
# of these, a filter size that is not a power of two (position table by modulo); the others 2^24 bits, where a tiny index
# also gets the exact table in LDS
UNIFORM_MOD = (32, 64, 128, 150, 350, 500)
# (longest mate 1, longest mate 2, reads): single-end maxima at 64*U and 64*U + 1 slots for U = 2 ... 10, and pairs at 640 / 649
RAGGED_MAX = tuple((64 * u + 16 + d, 0, 14) for u in (2, 3, 4, 5, 6, 8, 10) for d in (0, 1)) + ((328, 328, 10), (329, 329, 10))


def std_case(rng, name, k, bf_bits, n_genes=5, features=(), paired=True, n_reads=120, lengths=SHORT, c=0.6, q=0, single=False,
             lo=120, hi=500, width=0, cfrac=None, uniform=None, p_edge=0.1):
    genes = rc.make_genes(rng, n_genes, lo, hi, k, features)
    mq = rc.threshold(q)
    reads = rc.make_reads(rng, genes, n_reads, k, lengths, paired, mq is not None, mq if mq is not None else 0, cfrac=cfrac,
                          uniform=uniform, p_edge=p_edge)
    return rc.case(name, genes, reads, k, c, q, single, bf_bits, fasta_width=width, rng=rng)


def many_records_case(rng):
    """4 genes, 65 532 filler records (no k-mer: `N`), 4 more genes: 65 540 records, and the last 4 genes' uint16 numbers
    (65 536 ... 65 539) wrap onto 0..3"""
    k = 17
    front = rc.make_genes(rng, 4, 200, 400, k)
    back = [("w%d" % i, "", s) for i, (_, _, s) in enumerate(rc.make_genes(rng, 4, 200, 400, k))]
    filler = [("x", "", b"N")] * (65536 - len(front))
    genes = front + filler + back
    reads = rc.make_reads(rng, front + back, 150, k, SHORT, True, False, 0)
    return rc.case("records_65540", genes, reads, k, 0.6, bf_bits=1 << 22)


def grid():
    rng = np.random.default_rng(20261016)
    cases = []
    for i, k in enumerate(KS):                                          # k
        cases.append(std_case(rng, "k%d" % k, k, (1 << 20) if k > 5 else (1 << 12) + 1, paired=i % 2 == 0,
                              features=("ties",) if i % 3 == 0 else (), n_reads=60))
    sat_k = (5, 11, 17)
    for j, bits in enumerate((1, 64, 1000)):                            # saturated filters
        for kk in sat_k[j:j + 2]:
            cases.append(std_case(rng, "bits%d_k%d" % (bits, kk), kk, bits, n_genes=4, n_reads=60, features=("ties",), c=0.3))
    for j, bits in enumerate((12345, (1 << 20) + 1, 3000017)):          # not powers of two
        cases.append(std_case(rng, "bits%d" % bits, (11, 17, 21)[j], bits, n_genes=8, n_reads=70))
    for e in range(16, 27):                                             # powers of two
        cases.append(std_case(rng, "pow%d" % e, (17, 31, 15, 21, 16)[e % 5], 1 << e, n_genes=6,
                              paired=e % 2 == 0, features=("revcomp",) if e % 3 == 0 else (), n_reads=50))
    for j in range(4):                                                  # -b 1: the product CLI replays these
        cases.append(std_case(rng, "gib%d" % j, (17, 31, 11, 21)[j], rc.GIB_BITS, n_genes=6, n_reads=100, paired=j != 1,
                              features=(("ties",), ("quirk", "dirty"), ("revcomp", "contained"), ())[j], q=(0, 0, 20, 0)[j],
                              single=j == 3, lengths=SHORT + (300,) if j == 0 else SHORT))
    for j, feat in enumerate((("ties",), ("revcomp",), ("contained",), ("quirk",), ("dirty",), ("quirk", "dirty", "ties"))):
        kk = (17, 21, 15, 17, 11, 5)[j]                                 # references
        cases.append(std_case(rng, "ref_" + "_".join(feat), kk, 1 << 22, n_genes=6, features=feat, n_reads=80, c=0.5,
                              width=-1 if j % 2 else 0))
    cases.append(std_case(rng, "multiline", 17, 1 << 21, n_genes=8, width=-1, n_reads=80))
    cases.append(many_records_case(rng))
    for c in CS:                                                        # -c around c * len
        cases.append(std_case(rng, "c%.4f" % c, 17, 1 << 24, n_genes=4, paired=False, n_reads=90, c=c,
                              lengths=(60, 64, 90, 99, 100, 120, 150, 151), cfrac=c or 0.2))
    for single in (False, True):                                        # -s, with ties and without
        for feat in (("ties",), ()):
            cases.append(std_case(rng, "s%d_%s" % (single, "ties" if feat else "plain"), 17, 1 << 22, n_genes=4,
                                  features=feat + ("revcomp",), single=single, c=0.4, n_reads=80))
    for q in QS:                                                        # -q, with its char wrap
        cases.append(std_case(rng, "q%d" % q, 17, 1 << 22, n_genes=4, q=q, paired=q % 2 == 0, n_reads=60, c=0.5))
    for paired in (False, True):                                        # read lengths around the kernels' specialisations
        cases.append(std_case(rng, "len_%s" % ("pe" if paired else "se"), 17, 1 << 24, n_genes=4, lo=1500, hi=2500,
                              paired=paired, n_reads=60, lengths=LENGTHS))
    cases.append(std_case(rng, "len_k31_pe", 31, 1 << 24, n_genes=4, lo=1500, hi=2500, n_reads=40, lengths=LENGTHS))
    for L in UNIFORM:                                                   # uniform batches: one specialisation each
        for paired in (False, True):
            cases.append(std_case(rng, "uni%d_%s" % (L, "pe" if paired else "se"), 17, 3000017 if L in UNIFORM_MOD else 1 << 24,
                                  n_genes=4, lo=800, hi=1500, paired=paired, n_reads=max(8, 1600 // L), lengths=(L,),
                                  uniform=(L, L), q=20 if L % 3 == 0 else 0))
    for L1, L2, n_reads in RAGGED_MAX:                                  # ragged batches whose longest read sits on a boundary
        cs = std_case(rng, "ragged%d_%d" % (L1, L2), 17, 1 << 22, n_genes=4, lo=800, hi=1500, paired=L2 > 0, n_reads=n_reads,
                      lengths=(40, 100, L1 - 30, L1), p_edge=0.0)
        r1 = rc.parse_fastq(cs["fq1"])
        r1[0] = (r1[0][0], r1[0][1][:L1].ljust(L1, b"N"), r1[0][2][:L1].ljust(L1, b"I"))    # the first read holds the maximum
        assert max(len(r[1]) for r in r1) == L1
        cs["fq1"] = b"".join(b"@%s\n%s\n+\n%s\n" % r for r in r1)
        if L2:
            r2 = rc.parse_fastq(cs["fq2"])
            r2[0] = (r2[0][0], r2[0][1][:L2].ljust(L2, b"N"), r2[0][2][:L2].ljust(L2, b"I"))
            assert max(len(r[1]) for r in r2) <= L2
            cs["fq2"] = b"".join(b"@%s\n%s\n+\n%s\n" % r for r in r2)
        cases.append(cs)
    return cases


def main():
    assert os.path.exists(SHARK_REF), "oracle/_ref/shark_ref missing: run `make -C oracle ref`"
    cases = grid()
    with tempfile.TemporaryDirectory() as d:
        for cs in cases:
            cs["ssv"], cs["out1"], cs["out2"] = rc.run_case(SHARK_REF, cs, d, env_bits="REF_BF_BITS")
    rc.save(cases)
    n_assoc = sum(cs["ssv"].count(b"\n") for cs in cases)
    print("wrote %s: %d cases, %d associations, %d bytes" % (os.path.basename(rc.CASES_NPZ), len(cases), n_assoc,
                                                              os.path.getsize(rc.CASES_NPZ)))


if __name__ == "__main__":
    main()
