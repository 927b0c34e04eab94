"""The yardstick for end extension (shk_alignments_extend) and aligned pileup (shk_pileup_enable_aligned) -- include/shark_hip.h,
"alignments" step 3a and "ALIGNED PILEUP".

Written from the header's text on top of tests/align_model.py (the record before extension, the oriented read, the record's codes,
step 4's kinds) and tests/pileup_model.py's layout:

  overhang   one string per end: the kind of every overhang base ('=' a match, 'X' a mismatch, '.' neither), nearest the block first
  scorer     best_extension: the running totals of the whole string at once (numpy cumsum), the bonus added to the last total where the
             overhang ends with the mate, the FIRST largest total wins (np.argmax's rule: ties to the smallest e, e = 0 scores 0)
  naive      naive_extension: every e priced from scratch, base by base, O(H^2); the CPU tests hold the two against each other
  counting   the blocks' matches and mismatches counted anew over the extended blocks
  pileup     from the final records alone: every base of every block is one observation at its record coordinate

No passes of 64, no packed keys, no carried scalars: it shares no idea with the kernel.

Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.align_model import _kind, mate_alignment, oriented_codes, record_codes, to_record
from tests.depth_model import model_layout
from tests.placement_model import masked_mates


def check_params(P, B):
    if not (0 <= P <= 15 and 0 <= B <= 15):
        raise ValueError("mismatch_penalty and end_bonus lie in 0 .. 15")


def overhang(read, rec, q, x, step):
    """(kinds, to_end): the kinds of the overhang bases read[q], read[q + step], ... against rec[x], rec[x + step], ... as far as both
    the mate and the record go (H of them), and whether the overhang ends with the MATE (so that e == H earns the bonus)"""
    L, len_g = len(read), len(rec)
    left_q = (L - q) if step > 0 else (q + 1)
    left_x = (len_g - x) if step > 0 else (x + 1)
    H = max(0, min(left_q, left_x))
    kinds = "".join(_kind(int(read[q + step * t]), int(rec[x + step * t])) for t in range(H))
    return kinds, left_q <= left_x


def best_extension(kinds, to_end, P, B):
    """the e in 0 .. len(kinds) of largest score, ties to the smallest e"""
    if not kinds:
        return 0
    value = {"=": 1, "X": -P, ".": 0}
    totals = np.concatenate([[0], np.cumsum([value[c] for c in kinds], dtype=np.int64)])
    if to_end:
        totals[-1] += B
    return int(np.argmax(totals))


def naive_extension(kinds, to_end, P, B):
    """the same, every e priced from scratch"""
    best_e, best = 0, 0
    for e in range(1, len(kinds) + 1):
        s = 0
        for t in range(e):
            s += 1 if kinds[t] == "=" else (-P if kinds[t] == "X" else 0)
        if to_end and e == len(kinds):
            s += B
        if s > best:
            best_e, best = e, s
    return best_e


def extend_alignment(al, mate, record, P, B, stats=None, scorer=best_extension):
    """mate_alignment's tuple after step 3a at penalty P (>= 1) and bonus B; stats: 'left', 'right' count the ends that gained
    bases, 'gained' the mates that did, 'bases' the bases gained"""
    n, strand, _, _, blocks = al
    if n == 0:
        return al
    read, rec = oriented_codes(mate, strand), record_codes(record)
    blocks = [list(b) for b in blocks]
    x0, q0, _ = blocks[0]
    kinds, to_end = overhang(read, rec, q0 - 1, x0 - 1, -1)
    e_left = scorer(kinds, to_end, P, B)
    blocks[0] = [x0 - e_left, q0 - e_left, blocks[0][2] + e_left]
    x, q, ln = blocks[-1]
    kinds, to_end = overhang(read, rec, q + ln, x + ln, +1)
    e_right = scorer(kinds, to_end, P, B)
    blocks[-1][2] += e_right
    if stats is not None:
        stats["left"] = stats.get("left", 0) + (e_left > 0)
        stats["right"] = stats.get("right", 0) + (e_right > 0)
        stats["gained"] = stats.get("gained", 0) + (e_left + e_right > 0)
        stats["bases"] = stats.get("bases", 0) + e_left + e_right
    matches = mismatches = 0
    for x, q, ln in blocks:
        assert 0 <= x and x + ln <= len(rec) and 0 <= q and q + ln <= len(read)
        for t in range(ln):
            kind = _kind(int(read[q + t]), int(rec[x + t]))
            matches += kind == "="
            mismatches += kind == "X"
    return (n, strand, matches, mismatches, [tuple(b) for b in blocks])


def mate_alignment_extended(mate, rows, k, s_min, record, P, B, stats=None, scorer=best_extension):
    """align_model.mate_alignment followed by step 3a; P == 0: the step is off"""
    check_params(P, B)
    al = mate_alignment(mate, rows, k, s_min, record)
    return al if P == 0 else extend_alignment(al, mate, record, P, B, stats, scorer)


def expected_alignments_extended(model, batch, gene_off, gene_ids, rows, s_min, P, B, min_quality=0, stats=None):
    """align_model.expected_alignments with the step: (n_assoc, 2) records of capi.ALIGNMENT_DTYPE"""
    if s_min < 1:
        raise ValueError("min_support must be at least 1")
    gene_off = np.asarray(gene_off)
    out = np.zeros((int(gene_off[-1]) if len(gene_off) else 0, 2), dtype=capi.ALIGNMENT_DTYPE)
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            record = model.records.get(int(gene_ids[j]), b"")
            for t, mate in enumerate(pair):
                if mate is not None:
                    out[j, t] = to_record(mate_alignment_extended(mate, rows[j, t], model.k, s_min, record, P, B, stats))
    return out


def expected_aligned_pileup(model, batch, gene_off, gene_ids, records, min_quality=0):
    """(counts, mates, block_bases) of one batch under aligned pileup, from the batch's final alignment records alone: uint32
    (n_bases, 4) observations in model_layout(model)'s order, the mates with a block, and the number of block bases whose read byte
    is a base (= counts.sum())"""
    gs = model_layout(model)
    counts = np.zeros((int(gs[-1]), 4), dtype=np.uint32)
    gene_off = np.asarray(gene_off)
    mates = bearing = 0
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            a = int(gs[int(gene_ids[j])])
            for t, mate in enumerate(pair):
                r = records[j, t]
                if mate is None or not int(r["n_blocks"]):
                    continue
                mates += 1
                read = oriented_codes(mate, int(r["strand"]))
                for b in range(int(r["n_blocks"])):
                    x, q, ln = (int(v) for v in r["block"][b])
                    for u in range(ln):
                        c = int(read[q + u])
                        if c < 4:
                            counts[a + x + u, c] += 1
                            bearing += 1
    return counts, mates, bearing
