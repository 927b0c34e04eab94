"""The yardstick for alignments mode (shk_alignments_enable / shk_alignments_last / shk_alignment_cigar / `shark --sam`) --
include/shark_hip.h "alignments".

Written from the header's text on top of tests/segments_model.py's rows (m = 4) and the masked mates of tests/placement_model.py:

  pieces    an int8 array over the gene's record, -1 everywhere.  The kept spans are visited in sorted order and a span writes its
            own number only where the array still holds -1: ownership by FIRST WRITER.  A span's piece is what carries its number.
  read      the mate turned into the record's orientation ONCE (strand 1: reversed and complemented), as codes 0 .. 3 and 4 for a
            byte that is no base; from then on read coordinate q is simply index q of that array.
  trimming  a second per-mate array, over the read: which read bases a block has taken.  A piece keeps the coordinates whose read
            base lies behind every taken one.
  closure   an explicit loop over the splits s = 0 .. R, each priced base by base.
  text      one operation letter per read base and per skipped record base, written out and then run-length encoded.

No running reach, no cursor arithmetic on intervals, no masks, no minimum over packed keys: it shares no idea with the kernel.

Test infrastructure only."""
import itertools

import numpy as np

from shark_amd import capi
from tests.placement_model import _to_int, masked_mates

MAX_CLOSE = 64


def oriented_codes(mate, strand):
    """the mate (bytes behind the -q mask) in the record's orientation: uint8 codes 0 .. 3 = A, C, G, T on the record's strand, 4 for
    a byte that is no base"""
    to_int = np.asarray(_to_int(), dtype=np.int16)
    c = to_int[np.frombuffer(bytes(mate), dtype=np.uint8)]      # 0: no base; 1 .. 4
    if strand:
        c = c[::-1]
        return np.where(c == 0, 4, 3 - (c - 1)).astype(np.uint8)
    return np.where(c == 0, 4, c - 1).astype(np.uint8)


def record_codes(record):
    """the header's r per record base: 0 .. 3, every other byte 4"""
    to_int = np.asarray(_to_int(), dtype=np.int16)
    c = to_int[np.frombuffer(bytes(record), dtype=np.uint8)]
    return np.where(c == 0, 4, c - 1).astype(np.uint8)


def _kind(b, r):
    """'=' a match, 'X' a mismatch, '.' neither (step 4)"""
    if b == 4 or r == 4:
        return "."
    return "=" if b == r else "X"


def mate_alignment(mate, rows, k, s_min, record, stats=None, gaps=None):
    """(n_blocks, strand, matches, mismatches, [(x, q, len)]) of one masked mate (bytes) with its segment rows (strand, pos, support,
    first, last; rank order) against its gene's record (bytes).  stats: a dict whose 'trimmed', 'closed', 'open_insertion',
    'open_wide' and 'dropped' are counted up (blocks that lost bases to trimming, gaps closed, gaps left open with G < R, with
    R > 64, pieces that yielded no block); gaps: a list that receives (R, G, closed) of every gap with R >= 1"""
    L, len_g = len(mate), len(record)
    spans = capi.kept_spans(rows, L, k, s_min)
    if not spans:
        return (0, 0, 0, 0, [])
    strand = int(rows[0][0])
    read = oriented_codes(mate, strand)
    rec = record_codes(record)
    # 1. pieces: first writer
    owner = np.full(len_g, -1, dtype=np.int8)
    for n, (lo, hi, pos) in enumerate(spans):
        xs = np.arange(max(lo, 0), max(min(hi, len_g), 0))
        owner[xs[owner[xs] == -1]] = n
    # 2. trimming: a piece keeps the coordinates whose read base lies behind every read base taken so far
    taken = np.zeros(L, dtype=bool)
    blocks = []
    for n, (lo, hi, pos) in enumerate(spans):
        xs = np.nonzero(owner == n)[0]
        if len(xs) == 0:
            continue
        assert (np.diff(xs) == 1).all()                          # (a piece is an interval)
        qs = xs - pos
        assert qs.min() >= 0 and qs.max() < L                    # (the header: a span lies inside [pos, pos + L))
        behind = int(np.nonzero(taken)[0].max()) + 1 if taken.any() else 0
        keep = qs >= behind
        if not keep.any():
            if stats is not None:
                stats["dropped"] = stats.get("dropped", 0) + 1
            continue
        if stats is not None and not keep.all():
            stats["trimmed"] = stats.get("trimmed", 0) + 1
        xs, qs = xs[keep], qs[keep]
        taken[qs] = True
        blocks.append([int(xs[0]), int(qs[0]), len(xs)])
    # 3. gap closure, gap by gap
    for A, B in zip(blocks, blocks[1:]):
        R = B[1] - (A[1] + A[2])
        G = B[0] - (A[0] + A[2])
        assert R >= 0 and G >= 0
        if R == 0:
            continue
        if gaps is not None:
            gaps.append((R, G, not (R > MAX_CLOSE or G < R)))
        if R > MAX_CLOSE or G < R:
            if stats is not None:
                key = "open_wide" if R > MAX_CLOSE else "open_insertion"
                stats[key] = stats.get(key, 0) + 1
            continue
        q0, xa, xb = A[1] + A[2], A[0] + A[2], B[0]
        best_s, best_cost = None, None
        for s in range(R + 1):
            cost = 0
            for t in range(R):
                x = xa + t if t < s else xb - R + t
                cost += _kind(int(read[q0 + t]), int(rec[x])) != "="
            if best_cost is None or cost <= best_cost:           # (<=: ties go to the largest s)
                best_s, best_cost = s, cost
        A[2] += best_s
        B[0] -= R - best_s
        B[1] -= R - best_s
        B[2] += R - best_s
        if stats is not None:
            stats["closed"] = stats.get("closed", 0) + 1
    # 4. counting
    matches = mismatches = 0
    for x, q, n in blocks:
        for t in range(n):
            kind = _kind(int(read[q + t]), int(rec[x + t]))
            matches += kind == "="
            mismatches += kind == "X"
    return (len(blocks), strand, matches, mismatches, [tuple(b) for b in blocks])


def to_record(al):
    """mate_alignment's tuple as one capi.ALIGNMENT_DTYPE record"""
    out = np.zeros((), dtype=capi.ALIGNMENT_DTYPE)
    n, strand, m, x, blocks = al
    if n:
        out["n_blocks"], out["strand"], out["matches"], out["mismatches"] = n, strand, m, x
        for r, b in enumerate(blocks):
            out["block"][r] = b
    return out


def expected_alignments(model, batch, gene_off, gene_ids, rows, s_min, min_quality=0, stats=None):
    """(n_assoc, 2) records of capi.ALIGNMENT_DTYPE -- what SharkHip.alignments_last hands out.  rows:
    expected_segments(model, batch, gene_off, gene_ids, 4, min_quality)[1]"""
    if s_min < 1:
        raise ValueError("min_support must be at least 1")
    gene_off = np.asarray(gene_off)
    out = np.zeros((int(gene_off[-1]) if len(gene_off) else 0, 2), dtype=capi.ALIGNMENT_DTYPE)
    for i, pair in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            record = model.records.get(int(gene_ids[j]), b"")
            for t, mate in enumerate(pair):
                if mate is not None:
                    out[j, t] = to_record(mate_alignment(mate, rows[j, t], model.k, s_min, record, stats))
    return out


def cigar(rec, L, min_intron=20):
    """(CIGAR, NM) of one record for a mate of L bytes by the header's walk, written out letter by letter: one letter per read base
    (S, M, I) and per skipped record base (N, D), then run-length encoded -- adjacent equal operations merge by themselves"""
    n = int(rec["n_blocks"])
    if n == 0:
        return "*", 0
    blocks = [tuple(int(v) for v in rec["block"][r]) for r in range(n)]
    letters = "S" * blocks[0][1]
    edits = int(rec["mismatches"])
    for r, (x, q, ln) in enumerate(blocks):
        if r:
            px, pq, pl = blocks[r - 1]
            R, G = q - (pq + pl), x - (px + pl)
            assert R >= 0 and G >= 0
            letters += "I" * R
            edits += R
            if G >= min_intron:
                letters += "N" * G
            else:
                letters += "D" * G
                edits += G
        letters += "M" * ln
    last = blocks[-1]
    assert last[1] + last[2] <= L
    letters += "S" * (L - (last[1] + last[2]))
    assert sum(c in "SMI" for c in letters) == L
    return "".join("%d%s" % (len(list(run)), op) for op, run in itertools.groupby(letters)), edits


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def sam_seq(raw, strand):
    """SEQ of a mate's raw bytes: as they are on strand 0; on strand 1 reversed, A<->T and C<->G complemented with the case kept, every
    other byte N"""
    raw = bytes(raw)
    if not strand:
        return raw.decode("latin-1")
    return bytes(_COMP[c] if c in b"ACGTacgt" else ord("N") for c in raw[::-1]).decode("latin-1")


def sam_header(legend, model, nidx):
    lines = ["@HD\tVN:1.6\tSO:unsorted"]
    for g in range(nidx):
        lines.append("@SQ\tSN:%s\tLN:%d" % (legend[g], len(model.records.get(g, b""))))
    return lines


def sam_lines(ids, raw_mates, raw_quals, gene_off, gene_ids, records, legend, paired, min_intron=20):
    """the alignment lines of `shark --sam`: one per association and mate with n_blocks > 0, input order, a read's associations in
    gene_ids order, mate 1 before mate 2.  ids: the read ids as --placements prints them; raw_mates[i] = (mate 1 bytes, mate 2 bytes or
    None), raw_quals likewise or None (FASTA input); records: expected_alignments' array"""
    lines = []
    for i, rid in enumerate(ids):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            recs = records[j]
            pos = [int(r["block"][0][0]) + 1 if r["n_blocks"] else 0 for r in recs]
            for t in range(2 if paired else 1):
                r, other = recs[t], recs[1 - t]
                if not r["n_blocks"]:
                    continue
                flag = 0x100 if j > int(gene_off[i]) else 0
                if r["strand"]:
                    flag |= 0x10
                if paired:
                    flag |= 0x1 | (0x40 if t == 0 else 0x80)
                    if not other["n_blocks"]:
                        flag |= 0x8
                    elif other["strand"]:
                        flag |= 0x20
                raw = raw_mates[i][t]
                cg, nm = cigar(r, len(raw), min_intron)
                mate_has = paired and other["n_blocks"]
                qual = "*"
                if raw_quals is not None:
                    q = bytes(raw_quals[i][t])
                    qual = (q[::-1] if r["strand"] else q).decode("latin-1")
                lines.append("\t".join([rid, str(flag), legend[int(gene_ids[j])], str(pos[t]), "255", cg, "=" if mate_has else "*",
                                        str(pos[1 - t]) if mate_has else "0", "0", sam_seq(raw, int(r["strand"])), qual, "NM:i:%d" % nm]))
    return lines


def verify_sam_line(line, fasta):
    """what any consumer can check with nothing but the line and the FASTA ({name: record bytes}): the CIGAR consumes len(SEQ) query
    bases and stays inside the record, and NM recomputed from SEQ against the record over M, plus the I and D lengths, is the tag.
    (A base counts as an edit iff both it and the record's base are A, C, G or T in either case and they differ: the header's step 4.)"""
    import re
    f = line.split("\t")
    assert len(f) >= 12, line
    rec = bytes(fasta[f[2]]).upper()
    seq = f[9].upper().encode("latin-1")
    ops = re.findall(r"(\d+)([MIDNS])", f[5])
    assert "".join(n + o for n, o in ops) == f[5] and ops, f[5]
    assert all(a[1] != b[1] for a, b in zip(ops, ops[1:])), f[5]              # (adjacent equal operations are merged)
    assert all(int(n) > 0 for n, _ in ops), f[5]
    x, q, nm = int(f[3]) - 1, 0, 0
    assert x >= 0
    for n, o in ops:
        n = int(n)
        if o == "S":
            q += n
        elif o == "I":
            q += n
            nm += n
        elif o == "D":
            x += n
            nm += n
        elif o == "N":
            x += n
        else:
            assert x + n <= len(rec), (line, len(rec))
            for t in range(n):
                a, b = seq[q + t:q + t + 1], rec[x + t:x + t + 1]
                nm += a in (b"A", b"C", b"G", b"T") and b in (b"A", b"C", b"G", b"T") and a != b
            x += n
            q += n
    assert q == len(seq), line
    assert f[11] == "NM:i:%d" % nm, (line, nm)
    assert f[10] == "*" or len(f[10]) == len(seq)
    return nm
