"""The yardstick for rescue mode (shk_rescue_enable / shk_rescue_last / `shark --sam-rescue`) -- include/shark_hip.h "rescue".

Written from the header's text alone, on top of alignment records (capi.ALIGNMENT_DTYPE: the device's own or tests/align_model.py's),
the masked mates of tests/placement_model.py and the records' bytes:

  anchor   the record's blocks as a list; I_A is a sum over the gaps that are introns.
  window   lo and hi as the header writes them, Python integers.
  cost     the target turned into the record's orientation once, then every candidate's L_T record bases as one row of a table
           (numpy's sliding window), each base's kind looked up and the row counted in full: no packing, no early exit -- the
           saturation is a minimum afterwards.
  best     a sort of (cost, tie) tuples; cost2 is the second entry's cost.

No passes of 64, no keys, no masks: it shares no idea with the kernel.  Test infrastructure only."""
import numpy as np

from shark_amd import capi
from tests.placement_model import _to_int, masked_mates

MIN_LEN, MAX_LEN = 32, 512
L_MAX = (1 << 31) - 1

WRONG = ("no_introns", "no_clip", "tie_far", "neither_matches", "second_in_pass", "no_complement")


def _codes(seq):
    """codes 0 .. 3 per byte, 4 for a byte that is no base"""
    to_int = np.asarray(_to_int(), dtype=np.int16)
    c = to_int[np.frombuffer(bytes(seq), dtype=np.uint8)]         # 0: no base; 1 .. 4
    return np.where(c == 0, 4, c - 1).astype(np.int16)


def target_codes(mate, strand, wrong=None):
    """the mate (bytes behind the -q mask) in the record's orientation on `strand`: codes 0 .. 3, 4 for a byte that is no base"""
    c = _codes(mate)
    if not strand:
        return c
    c = c[::-1]
    if wrong == "no_complement":
        return c
    return np.where(c < 4, 3 - c, 4).astype(np.int16)


def anchor_ends(rec, L, min_intron):
    n = int(rec["n_blocks"])
    blocks = [tuple(int(v) for v in rec["block"][r]) for r in range(n)]
    first, last = blocks[0], blocks[-1]
    introns = 0
    for A, B in zip(blocks, blocks[1:]):
        G = B[0] - (A[0] + A[2])
        if G >= min_intron:
            introns += G
    L = min(int(L), L_MAX)
    return {"s": first[0], "e": last[0] + last[2], "cl": first[1], "cr": L - (last[1] + last[2]), "I": introns, "strand": int(rec["strand"])}


def window(A, L_T, len_g, max_frag, wrong=None):
    I = 0 if wrong == "no_introns" else A["I"]
    cl, cr = (0, 0) if wrong == "no_clip" else (A["cl"], A["cr"])
    if A["strand"] == 0:
        lo = max(A["s"], A["e"] - L_T, 0)
        hi = min(A["s"] - cl + I + max_frag - L_T, len_g - L_T)
    else:
        lo = max(A["e"] + cr - I - max_frag, 0)
        hi = min(A["s"], A["e"] - L_T, len_g - L_T)
    return lo, hi


def kinds(read, rows):
    """per target base '=' a match, 'X' a mismatch, '.' neither (step 4), as an array of characters; rows: the record bases under the
    target, one row per candidate"""
    return np.where((read == 4) | (rows == 4), ".", np.where(read == rows, "=", "X"))


def rescue_association(recs, mates, record, min_intron, max_frag, max_cost, min_gap, wrong=None, detail=None):
    """(the two mates' alignment records afterwards, the rescue record) of one association.  recs: its two capi.ALIGNMENT_DTYPE records;
    mates: (mate 1, mate 2 or None) as masked bytes; record: the gene's bytes.  detail: a dict that receives lo, hi, best and the
    candidates' saturated costs (for the messages of the GPU tests)"""
    out = np.array([recs[0], recs[1]], dtype=capi.ALIGNMENT_DTYPE)
    rs = np.zeros((), dtype=capi.RESCUE_DTYPE)
    has = [int(recs[t]["n_blocks"]) >= 1 for t in range(2)]
    if has[0] == has[1] or mates[1] is None:
        return out, rs
    a, t = (0, 1) if has[0] else (1, 0)
    L_T = min(len(mates[t]), L_MAX)
    if not MIN_LEN <= L_T <= MAX_LEN:
        return out, rs
    A = anchor_ends(recs[a], len(mates[a]), min_intron)
    strand_T = 1 - A["strand"]
    rec = _codes(record)
    lo, hi = window(A, L_T, len(rec), max_frag, wrong)
    n_cand = max(0, hi - lo + 1)
    cap = max_cost + min_gap
    rs["n_cand"] = n_cand
    if n_cand == 0:
        rs["state"], rs["cost"], rs["cost2"] = 1, cap + 1, cap + 1
        return out, rs
    read = target_codes(mates[t], strand_T, wrong)
    rows = np.lib.stride_tricks.sliding_window_view(rec[lo:hi + L_T], L_T)    # row x - lo: record bases x .. x + L_T - 1
    kk = kinds(read, rows)
    costs = (kk != "=").sum(axis=1) if wrong != "neither_matches" else (kk == "X").sum(axis=1)
    cands = []
    for x in range(lo, hi + 1):
        cost = min(int(costs[x - lo]), cap + 1)
        nearer = x if A["strand"] == 0 else -x                    # the smaller frag first
        cands.append((cost, -nearer if wrong == "tie_far" else nearer, x))
    cands.sort()
    cost, _, best = cands[0]
    others = cands[1:]
    if wrong == "second_in_pass":
        others = [c for c in others if (c[2] - lo) // 64 == (best - lo) // 64]
    cost2 = others[0][0] if others else cap + 1
    rs["cost"], rs["cost2"] = cost, cost2
    if detail is not None:
        detail.update(lo=lo, hi=hi, best=best, costs={x: c for c, _, x in cands})
    if cost > max_cost:
        rs["state"] = 2
    elif cost2 - cost < min_gap:
        rs["state"] = 3
    else:
        rs["state"] = 4 + t
        kk = kinds(read, rows[best - lo])
        new = np.zeros((), dtype=capi.ALIGNMENT_DTYPE)
        new["n_blocks"], new["strand"] = 1, strand_T
        new["matches"], new["mismatches"] = int((kk == "=").sum()), int((kk == "X").sum())
        new["block"][0] = (best, 0, L_T)
        out[t] = new
    return out, rs


def expected_rescue(records, batch, gene_off, gene_ids, gene_records, min_intron, max_frag, max_cost, min_gap, min_quality=0, wrong=None, details=None):
    """((n_assoc, 2) alignment records afterwards, (n_assoc,) records of capi.RESCUE_DTYPE) -- what SharkHip.alignments_last and
    rescue_last hand out with the mode on.  records: the alignment records with the mode off; gene_records: {gene: bytes}"""
    gene_off = np.asarray(gene_off).astype(np.int64)
    n_assoc = int(gene_off[-1]) if len(gene_off) else 0
    out = np.array(records, dtype=capi.ALIGNMENT_DTYPE).reshape(n_assoc, 2).copy()
    rs = np.zeros(n_assoc, dtype=capi.RESCUE_DTYPE)
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            d = {} if details is not None else None
            out[j], rs[j] = rescue_association(records[j], pair, gene_records.get(int(gene_ids[j]), b""), min_intron, max_frag, max_cost, min_gap, wrong, d)
            if details is not None:
                details[j] = d
    return out, rs


def sam_rescue_lines(lines, owners, rescues):
    """the lines of `shark --sam --sam-rescue` from the lines the rescued records give without the tag: YR:i:<cost> appended behind NM:i: on
    a rescued mate's line.  owners: per line its (association, mate)"""
    out = []
    for ln, (j, t) in zip(lines, owners):
        if int(rescues[j]["state"]) == 4 + t:
            ln += "\tYR:i:%d" % int(rescues[j]["cost"])
        out.append(ln)
    return out
