"""The case table of pairs mode's tests (include/shark_hip.h, "pairs"), in plain Python and numpy: pairs built directly from one record --
mate 1 = rec[a:a + L] or its reverse complement, mate 2 likewise -- so that every class, every tie-break and every edge of the fragment
length occurs.  tests/test_pairs_cpu.py holds the table against the model on the CPU, tests/test_gpu_pairs.py runs it on the GPU.

The record: U, 1 500 random bases for the unspliced cases; two spliced genes of tests/spliced_synth.py (one intron each) behind it for the
cases across junctions, 100 random bases between them and 300 behind."""
import numpy as np

from tests import synth
from tests.spliced_synth import spliced_gene

MIN_INTRON = 20
MAX_FRAG = 300
N_BINS = 1024
L = 60


def s_min_for(k):
    return 3 if k == 5 else 8


def _sub(m, *at):
    m = m.copy()
    for i in at:
        m[i] = synth.ACGT[(int(np.searchsorted(synth.ACGT, m[i])) + 1) % 4]
    return m


def pair_cases(k, seed=1, n_bins=N_BINS):
    """(record, names, mates1, mates2, expect): expect[name] = the fields of the pair record the case was built for (cls, left, frag,
    introns, proper, tlen = tend - tstart; a subset), true at k = 17 where a mate of 60 bases cut from the record aligns end to end"""
    rng = np.random.default_rng(seed)
    U = synth.random_seq(rng, 1500)
    (r1, t1), (r2, t2) = spliced_gene(rng, 1, k), spliced_gene(rng, 1, k)
    rec = np.concatenate([U, r1, synth.random_seq(rng, 100), r2, synth.random_seq(rng, 300)])
    o1, o2 = len(U), len(U) + len(r1) + 100
    i1, i2 = len(r1) - len(t1), len(r2) - len(t2)                 # the two introns' lengths (exons of 70 on either side)
    rc = synth.revcomp
    junk = lambda n: synth.random_seq(rng, n)                    # noqa: E731
    weak = lambda a: np.concatenate([U[a:a + 20], junk(40)])     # noqa: E731  (20 - k + 1 windows at most: below s_min at k = 17 and 31)
    F = lambda a, n=L: U[a:a + n].copy()                         # noqa: E731
    R = lambda a, n=L: rc(U[a:a + n])                            # noqa: E731
    cases = [
        ("inward", F(100), R(300), dict(cls=3, left=0, frag=260, tlen=260, introns=0, proper=1)),
        ("inward, mates swapped", R(300), F(100), dict(cls=3, left=1, frag=260, tlen=260, proper=1)),
        ("outward", R(100), F(300), dict(cls=4, left=0, frag=0, tlen=260, proper=0)),
        ("tandem on strand 0", F(100), F(300), dict(cls=5, left=0, frag=0, tlen=260, proper=0)),
        ("tandem on strand 1", R(300), R(100), dict(cls=5, left=1, frag=0, tlen=260, proper=0)),
        # s_F <= s_R but e_F > e_R: outward by the definition; equal starts: the smaller e is left
        ("dovetail, equal starts", F(100), R(100, 50), dict(cls=4, left=1, frag=0, tlen=60)),
        ("R inside F", F(100), R(110, 40), dict(cls=4, left=0, frag=0, tlen=60)),
        ("F inside R", F(110, 40), R(100), dict(cls=4, left=1, frag=0, tlen=60)),
        ("R starts in front of F", F(110), R(100), dict(cls=4, left=1, frag=0, tlen=70)),
        ("equal starts, F ends first", F(100, 50), R(100), dict(cls=3, left=0, frag=60, tlen=60)),
        ("equal starts and ends", F(100), R(100), dict(cls=3, left=0, frag=60, tlen=60, proper=1)),
        ("equal starts and ends, mates swapped", R(100), F(100), dict(cls=3, left=0, frag=60, tlen=60, proper=1)),
        ("mate 2 off target", F(100), junk(L), dict(cls=1, left=0, frag=0, tlen=60, proper=0)),
        ("mate 1 off target", junk(L), R(300), dict(cls=2, left=1, frag=0, tlen=60, proper=0)),
        ("mate 2 below s_min", F(100), rc(weak(500)), dict(cls=1, left=0)),
        ("mate 1 below s_min", weak(500), R(300), dict(cls=2, left=1)),
        ("both below s_min", weak(500), rc(weak(700)), dict(cls=0, left=0, frag=0, tlen=0, introns=0, proper=0)),
        # a substitution within k of the 5' end silences the windows over it: the block stops short, the clip is put back
        ("clipped 5' end of F", _sub(F(100), 3), R(300), dict(cls=3, frag=260, tlen=256)),
        ("clipped 5' end of R", F(100), rc(_sub(F(300), 56)), dict(cls=3, frag=260, tlen=256)),
        ("both 5' ends clipped", _sub(F(100), 3), rc(_sub(F(300), 56)), dict(cls=3, frag=260, tlen=252)),
        # both mates across the one junction of the first spliced gene: the union counts the intron once
        ("one junction, both mates", t1[40:100].copy(), rc(t1[45:105]), dict(cls=3, left=0, introns=i1, frag=65, tlen=65 + i1, proper=1)),
        ("two junctions", t1[40:100].copy(), rc(t2[40:100]), dict(cls=3, left=0, introns=i1 + i2, tlen=o2 + 100 + i2 - (o1 + 40))),
        ("junction in F only", t1[40:100].copy(), rc(r2[0:60]), dict(cls=3, left=0, introns=i1)),
        # five record bases missing in the mate: a gap below min_intron is a deletion, not an intron, and stays in the fragment
        ("deletion below min_intron", np.concatenate([U[800:830], U[835:865]]), R(1000), dict(cls=3, introns=0, frag=260, tlen=260)),
        ("frag == max_frag", F(200), R(200 + MAX_FRAG - L), dict(cls=3, frag=MAX_FRAG, proper=1)),
        ("frag == max_frag + 1", F(200), R(201 + MAX_FRAG - L), dict(cls=3, frag=MAX_FRAG + 1, proper=0)),
    ]
    # the last in-range bin, the overflow bin's first value and beyond, at the caller's n_bins (64: the mates overlap)
    for name, frag in (("frag == n_bins - 2", n_bins - 2), ("frag == n_bins - 1", n_bins - 1), ("frag beyond the bins", n_bins + 70)):
        cases.append((name, F(100), R(100 + frag - L), dict(cls=3, frag=frag, tlen=frag)))
    names = [c[0] for c in cases]
    return rec, names, [c[1] for c in cases], [c[2] for c in cases], {c[0]: c[3] for c in cases}


def case_batch(k, seed=1, n_bins=N_BINS):
    rec, names, m1, m2, expect = pair_cases(k, seed, n_bins)
    return rec, names, synth.batch_from_lists(m1, m2), expect


def check_expectations(names, pairs, gene_off, expect, every=1):
    """the table's non-vacuity: association j * every of read i carries what case i was built for (a reference of `every` equal genes)"""
    gene_off = np.asarray(gene_off)
    for i, name in enumerate(names):
        assert int(gene_off[i + 1]) - int(gene_off[i]) == every, (name, "associations")
        p = pairs[int(gene_off[i])]
        for field, v in expect[name].items():
            got = int(p["tend"]) - int(p["tstart"]) if field == "tlen" else int(p[field])
            assert got == v, (name, field, got, v, p)
