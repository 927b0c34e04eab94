"""The yardstick for pairs mode (shk_pairs_enable / shk_pairs_last / shk_fragments_get / `shark --sam-pairs` / `shark --fragments`) --
include/shark_hip.h "pairs".

Written from the header's text alone, on top of alignment records (capi.ALIGNMENT_DTYPE: the device's own or tests/align_model.py's),
the mates' lengths and gene_off:

  per mate   the record's blocks as a list; an intron is the SET of the record coordinates between two blocks.
  union      the union of Python sets -- no intervals, no sorting, no overlaps to subtract.
  class      the header's sentences as they stand, one `if` each.
  state      two plain lists of Python integers.
  text       --sam-pairs rewrites three fields of align_model.sam_lines' lines (imported, not edited); --fragments is printed.

Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.align_model import sam_lines

CLASS_NAMES = ("none", "mate1", "mate2", "inward", "outward", "tandem")
L_MAX = (1 << 31) - 1


def mapq_of(n):
    """the STAR scale with 60 for a unique read"""
    if n == 1:
        return 60
    if n == 2:
        return 3
    if n in (3, 4):
        return 1
    return 0


def mate_ends(rec, L, min_intron):
    """None for a mate without a block; else a dict: s, e, cl, cr, strand and the set of intron coordinates"""
    n = int(rec["n_blocks"])
    if n < 1:
        return None
    blocks = [tuple(int(v) for v in rec["block"][r]) for r in range(n)]
    L = min(int(L), L_MAX)
    first, last = blocks[0], blocks[-1]
    introns = set()
    for A, B in zip(blocks, blocks[1:]):
        G = B[0] - (A[0] + A[2])
        if G >= min_intron:
            introns |= set(range(A[0] + A[2], B[0]))
    return {"s": first[0], "e": last[0] + last[2], "cl": first[1], "cr": L - (last[1] + last[2]), "strand": int(rec["strand"]), "introns": introns}


def pair_record(recs, lengths, n_assoc_of_read, min_intron, max_frag, wrong=None):
    """one capi.PAIR_DTYPE record from the two mates' alignment records.  wrong: a named WRONG implementation (the CPU tests show that
    the cases tell each from the model): 'sum' introns summed instead of united, 'noclip' frag without the clips, 'tie1' the last
    tie-break to mate 1 (index 1), 'proper4' proper on outward pairs as well"""
    out = np.zeros((), dtype=capi.PAIR_DTYPE)
    out["mapq"] = mapq_of(int(n_assoc_of_read))
    m = [mate_ends(recs[t], lengths[t], min_intron) for t in range(2)]
    have = [t for t in range(2) if m[t] is not None]
    if not have:
        return out                                               # cls 0: every other field 0
    if len(have) == 1:
        cls = 1 if have[0] == 0 else 2
        left = have[0]
    else:
        if m[0]["strand"] != m[1]["strand"]:
            F, R = (m[0], m[1]) if m[0]["strand"] == 0 else (m[1], m[0])
            cls = 3 if (F["s"] <= R["s"] and F["e"] <= R["e"]) else 4
        else:
            cls = 5
        key = [(m[t]["s"], m[t]["e"], t if wrong != "tie1" else 1 - t) for t in range(2)]
        left = 0 if key[0] < key[1] else 1
    tstart = min(m[t]["s"] for t in have)
    tend = max(m[t]["e"] for t in have)
    if wrong == "sum":
        introns = sum(len(m[t]["introns"]) for t in have)
    else:
        introns = len(set().union(*[m[t]["introns"] for t in have]))
    frag = 0
    if cls == 3:
        frag = (tend - tstart) - introns + (0 if wrong == "noclip" else F["cl"] + R["cr"])
    proper = int((cls == 3 or (wrong == "proper4" and cls == 4)) and frag <= max_frag)
    out["cls"], out["left"], out["proper"] = cls, left, proper
    out["tstart"], out["tend"], out["introns"], out["frag"] = tstart, tend, introns, frag & 0xFFFFFFFF   # (a wrong implementation can go below 0)
    return out


def mate_lengths(batch):
    """(n, 2) lengths in bytes; mate 2 of a single-end batch: 0"""
    off1 = np.asarray(batch["off1"]).astype(np.int64)
    out = np.zeros((len(off1) - 1, 2), dtype=np.int64)
    out[:, 0] = np.diff(off1)
    if batch.get("off2") is not None:
        out[:, 1] = np.diff(np.asarray(batch["off2"]).astype(np.int64))
    return out


def expected_pairs(records, batch, gene_off, min_intron, max_frag, wrong=None):
    """(n_assoc,) records of capi.PAIR_DTYPE -- what SharkHip.pairs_last hands out.  records: (n_assoc, 2) of capi.ALIGNMENT_DTYPE"""
    gene_off = np.asarray(gene_off).astype(np.int64)
    lengths = mate_lengths(batch)
    out = np.zeros(int(gene_off[-1]) if len(gene_off) else 0, dtype=capi.PAIR_DTYPE)
    for i in range(len(gene_off) - 1):
        a, b = int(gene_off[i]), int(gene_off[i + 1])
        for j in range(a, b):
            out[j] = pair_record(records[j], lengths[i], b - a, min_intron, max_frag, wrong)
    return out


class Fragments:
    """the fragments state: classes[6] and hist[n_bins], Python integers"""

    def __init__(self, n_bins):
        assert 2 <= n_bins <= 4096
        self.n_bins = n_bins
        self.reset()

    def reset(self):
        self.classes = [0] * 6
        self.hist = [0] * self.n_bins

    def add(self, pairs, gene_off):
        """one counted batch: its pair records and its gene_off"""
        gene_off = np.asarray(gene_off).astype(np.int64)
        for i in range(len(gene_off) - 1):
            a, b = int(gene_off[i]), int(gene_off[i + 1])
            for j in range(a, b):
                cls = int(pairs[j]["cls"])
                self.classes[cls] += 1
                if cls == 3 and b - a == 1:
                    self.hist[min(int(pairs[j]["frag"]), self.n_bins - 1)] += 1
        return self

    def arrays(self):
        return np.array(self.hist, dtype=np.uint64), np.array(self.classes, dtype=np.uint64)

    def text(self):
        """the file `shark --fragments` writes: six class lines, one line per non-zero bin below the overflow bin, the overflow bin"""
        return fragments_text(self.hist, self.classes)


def fragments_text(hist, classes):
    lines = ["class %s %d" % (CLASS_NAMES[c], int(classes[c])) for c in range(6)]
    n_bins = len(hist)
    lines += ["frag %d %d" % (b, int(hist[b])) for b in range(n_bins - 1) if int(hist[b])]
    lines.append("frag >=%d %d" % (n_bins - 1, int(hist[n_bins - 1])))
    return "".join(ln + "\n" for ln in lines)


def sam_pairs_lines(ids, raw_mates, raw_quals, gene_off, gene_ids, records, pairs, legend, paired, min_intron=20, wrong=None):
    """the lines of `shark --sam --sam-pairs`: align_model.sam_lines' with MAPQ the record's mapq, 0x2 on both mates' lines iff proper,
    TLEN = tend - tstart on the left mate's line and its negative on the other's for cls 3, 4 and 5 (0 for cls 1 and 2); everything
    else on the line as it is.  pairs: expected_pairs' array at the same min_intron"""
    lines = sam_lines(ids, raw_mates, raw_quals, gene_off, gene_ids, records, legend, paired, min_intron)
    # the same walk sam_lines makes: which (association, mate) each line belongs to
    owners = [(j, t) for i in range(len(ids)) for j in range(int(gene_off[i]), int(gene_off[i + 1])) for t in range(2 if paired else 1)
              if records[j][t]["n_blocks"]]
    assert len(owners) == len(lines)
    out = []
    for (j, t), ln in zip(owners, lines):
        f = ln.split("\t")
        p = pairs[j]
        flag = int(f[1])
        if p["proper"] or (wrong == "proper4" and p["cls"] == 4):
            flag |= 0x2
        tlen = 0
        if int(p["cls"]) in (3, 4, 5):
            span = int(p["tend"]) - int(p["tstart"])
            tlen = span if t == int(p["left"]) else -span
        f[1], f[4], f[8] = str(flag), str(int(p["mapq"])), str(tlen)
        out.append("\t".join(f))
    return out
