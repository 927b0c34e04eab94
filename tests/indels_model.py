"""The yardstick for indels mode (shk_indels_enable / shk_indels_get / shk_indels_stats / `shark --indels`) -- include/shark_hip.h
"indels".

Written from the header's text over the alignment records of tests/align_model.py (capi.ALIGNMENT_DTYPE), the masked mates of
tests/placement_model.py and the records:

  gaps       every consecutive pair of a record's blocks, classified by (R, G) in plain Python.
  read       the mate turned into the record's orientation once (align_model.oriented_codes); an insertion's bases are a slice of it.
  shifting   left-normalisation ONE BASE AT A TIME: a deletion [x, x + G) moves to [x - 1, x - 1 + G) iff the base that enters on the
             left equals the base that leaves on the right; an insertion moves one to the left iff the record base in front of it equals
             its last base, and its sequence rotates by one.  No comparison of T[i] with T[i + R], no 64-wide pass.
  table      a dict keyed (gene, x, kind, len, seq) -> [fwd, rev].

Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.align_model import oriented_codes, record_codes
from tests.placement_model import masked_mates

MAX_INS = 12
STAT_NAMES = capi.INDEL_STAT_NAMES


def new_stats():
    return {name: 0 for name in STAT_NAMES}


def shift_left(kind, x, length, seq, rec):
    """(x, seq, d) of the left-normalised event.  kind 0: the deletion of rec[x : x + length]; kind 1: the insertion of seq (a list of
    codes 0 .. 3) in front of rec[x].  rec: record_codes of the gene's record"""
    seq = list(seq)
    d = 0
    while x > 0 and rec[x - 1] < 4:
        if kind == 0:
            if rec[x - 1] != rec[x - 1 + length]:
                break
        else:
            if rec[x - 1] != seq[-1]:
                break
            seq = [seq[-1]] + seq[:-1]
        x -= 1
        d += 1
    return x, seq, d


def pack(seq):
    return sum(int(b) << (2 * t) for t, b in enumerate(seq))


def unpack(seq, length):
    return [(int(seq) >> (2 * t)) & 3 for t in range(length)]


def record_events(rec, mate, record, min_intron, stats, shifts=None):
    """the tabled events of one alignment record (one capi.ALIGNMENT_DTYPE item) of one masked mate (bytes, or None) against its gene's
    record (bytes): [(x, kind, len, seq)] left-normalised; stats (new_stats()) is counted up.  shifts: a list that receives every d"""
    n = int(rec["n_blocks"])
    if n >= 1:
        stats["mates"] += 1
    if n < 2:
        return []
    blocks = [tuple(int(v) for v in rec["block"][r]) for r in range(n)]
    read = oriented_codes(mate, int(rec["strand"]))
    rcodes = record_codes(record)
    out = []
    for (xA, qA, lA), (xB, qB, lB) in zip(blocks, blocks[1:]):
        xa, qa = xA + lA, qA + lA
        R, G = qB - qa, xB - xa
        assert R >= 0 and G >= 0 and xB + lB <= len(record)
        if R == 0:
            if not 1 <= G < min_intron:
                continue
            stats["deletions"] += 1
            x, _, d = shift_left(0, xa, G, [], rcodes)
            out.append((x, 0, G, 0))
        elif G >= 1:
            stats["complex_gaps"] += 1
            continue
        else:
            if R > MAX_INS:
                stats["long_insertions"] += 1
                continue
            s = [int(v) for v in read[qa:qa + R]]
            if any(v >= 4 for v in s):
                stats["nonbase_insertions"] += 1
                continue
            stats["insertions"] += 1
            x, s, d = shift_left(1, xa, R, s, rcodes)
            out.append((x, 1, R, pack(s)))
        if shifts is not None:
            shifts.append(d)
    return out


def expected_indels(records, batch, gene_off, gene_ids, gene_records, min_intron, min_quality=0, table=None, stats=None, shifts=None):
    """(table, stats) of one batch from its alignment records ((n_assoc, 2) of capi.ALIGNMENT_DTYPE: the model's or the device's own):
    table {(gene, x, kind, len, seq): [fwd, rev]}, stats new_stats()'s dict; both are added to when given (several batches)"""
    table = {} if table is None else table
    stats = new_stats() if stats is None else stats
    gene_off = np.asarray(gene_off)
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            for t, mate in enumerate(pair):
                if mate is None:
                    continue
                rec = records[j, t]
                for x, kind, length, seq in record_events(rec, mate, gene_records.get(g, b""), min_intron, stats, shifts):
                    table.setdefault((g, x, kind, length, seq), [0, 0])[int(rec["strand"]) & 1] += 1
    return table, stats


def table_array(table, min_mates=0):
    """the table as shk_indels_get hands it out: capi.INDEL_DTYPE records sorted by (gene, x, kind, len, seq)"""
    keys = sorted(key for key, (f, r) in table.items() if f + r >= min_mates)
    out = np.zeros(len(keys), dtype=capi.INDEL_DTYPE)
    for n, key in enumerate(keys):
        out[n] = key + (table[key][0], table[key][1], 0)
    return out


def indel_lines(arr, legend):
    """the lines of `shark --indels`: <gene> <x> <I|D> <len> <seq> <fwd> <rev>, seq as letters on the record's strand, * for a deletion"""
    return ["%s %d %s %d %s %d %d" % (legend[int(e["gene"])], int(e["x"]), "DI"[int(e["kind"])], int(e["len"]),
                                      "".join("ACGT"[b] for b in unpack(e["seq"], int(e["len"]))) if int(e["kind"]) else "*",
                                      int(e["fwd"]), int(e["rev"])) for e in arr]


def check_entry(e, lengths):
    """shk_indels_add's SHK_ERR_ARG rules for one entry (gene, x, kind, len, seq, fwd, rev, reserved); lengths[g] = len_g"""
    gene, x, kind, length, seq, _, _, reserved = (int(v) for v in e)
    if gene >= len(lengths) or kind > 1 or reserved:
        return False
    if kind == 0 and not (1 <= length <= 65535 and seq == 0):
        return False
    if kind == 1 and not (1 <= length <= MAX_INS and seq >> (2 * length) == 0):
        return False
    return x < lengths[gene] and x + (length if kind == 0 else 0) <= lengths[gene]
