"""References and reads of the spliced-depth, junction-table and pileup tests: records of a few hundred bases with one to four introns,
mates of 60 to 120 bytes cut from the spliced transcript (they cross one to five junctions: five diagonals and more exceed m = 4) or
from the record itself (none)."""
import numpy as np

from tests import synth


def spliced_gene(rng, n_introns, k):
    """(record, transcript): n_introns + 1 exons with introns of 30 to 60 bases between them"""
    lo, hi = (18, 40) if k <= 17 else (k + 3, k + 20)
    exons = [synth.random_seq(rng, int(rng.integers(lo, hi))) for _ in range(n_introns + 1)]
    exons[0] = synth.random_seq(rng, 70)
    exons[-1] = synth.random_seq(rng, 70)
    parts = []
    for i, e in enumerate(exons):
        if i:
            parts.append(synth.random_seq(rng, int(rng.integers(30, 61))))
        parts.append(e)
    return np.concatenate(parts), np.concatenate(exons)


def spliced_reads(rng, genes, n, paired=True, ragged=True, sub=0.01, qual=False, lower=0.0):
    """genes: [(record, transcript)].  Per mate: 70 % from the transcript, 10 % from the record (unspliced; flush with either end now
    and then), 8 % with two bases deleted, 8 % with six bases repeated (its two record spans overlap), 4 % random; either strand"""
    m1s, m2s, q1, q2 = [], [], [], []
    for i in range(n):
        rec, tr = genes[int(rng.integers(0, len(genes)))]
        mates = []
        for _ in range(2):
            L = int(rng.integers(60, 121)) if ragged else 100
            u = rng.random()
            src = tr if (u < 0.7 or u >= 0.8) else rec
            L = min(L, len(src) - 8)
            a = int(rng.integers(0, len(src) - L + 1))
            if src is rec and rng.random() < 0.4:
                a = 0 if rng.random() < 0.5 else len(src) - L
            m = src[a:a + L].copy()
            if 0.8 <= u < 0.88:
                m = np.concatenate([src[a:a + L // 2], src[a + L // 2 + 2:a + L + 2]])
            elif 0.88 <= u < 0.96:
                m = np.concatenate([src[a:a + L // 2], src[a + L // 2 - 6:a + L - 6]])
            elif u >= 0.96:
                m = synth.random_seq(rng, L)
            s = rng.random(len(m)) < sub
            m[s] = synth.ACGT[rng.integers(0, 4, size=int(s.sum()))]
            lc = rng.random(len(m)) < lower
            m[lc] |= 0x20
            mates.append(synth.revcomp(m) if rng.random() < 0.5 else m)
        m1s.append(mates[0]); m2s.append(mates[1])
        if qual:
            for lst, m in ((q1, mates[0]), (q2, mates[1])):
                q = np.where(rng.random(len(m)) < 0.9, rng.integers(20, 42, size=len(m)), rng.integers(2, 20, size=len(m)))
                lst.append((q + 33).astype(np.uint8))
    return synth.batch_from_lists(m1s, m2s if paired else None, q1 if qual else None, q2 if (qual and paired) else None)
