"""The yardstick for shk_placement_last: per association (read, gene) of a batch and per mate the diagonal of the gene's record
that most of the mate's k-mers lie on -- (strand, pos, support), include/shark_hip.h "placement".

Written from the semantics, in plain Python over bytes; it does not go near the Bloom filter.  From oracle/pyoracle.py it takes
the alphabet (so_to_int) and FastqSplitter's join and quality mask (so_join_mask), as candidates_model.py does.

  record of gene g   main.cpp:160-187: the counter advances for every record except one that is at least k long and has no valid
                     k-mer; the record of g is the one with a valid k-mer that was numbered g (at most one)
  window             k characters that are all bases under to_int; f its k-mer, r the reverse complement, min(f, r) the canonical
                     k-mer, f <= r the orientation bit; f == r takes no part
  vote of slot p     iff the canonical k-mer has exactly ONE window x in the record: (strand, pos), strand = xor of the orientation
                     bits, pos = x - p (strand 0) or x + p + k - L (strand 1)
  placement          most votes; ties: strand 0 first, then the smaller pos; support = votes; none: (0, 0, 0)

Test infrastructure only."""
import ctypes as C

import numpy as np

_TO_INT = None


def _to_int():
    global _TO_INT
    if _TO_INT is None:
        from oracle import pyoracle
        L = pyoracle.lib()
        _TO_INT = [int(L.so_to_int(bytes([c]))) for c in range(256)]
    return _TO_INT


def windows(seq, k):
    """[(p, canonical k-mer, orientation bit)] over the valid, non-palindromic windows of a byte string"""
    to_int = _to_int()
    out = []
    mask = (1 << (2 * k)) - 1
    fw = rc = run = 0
    for end, ch in enumerate(seq):
        code = to_int[ch]
        if code == 0:
            run = 0
            continue
        code -= 1
        fw = ((fw << 2) | code) & mask
        rc = (rc >> 2) | ((3 - code) << (2 * k - 2))
        run += 1
        if run >= k and fw != rc:
            out.append((end - k + 1, min(fw, rc), 1 if fw < rc else 0))
    return out


def gene_records(fasta_seqs, k):
    """{gene id: record bytes} by the numbering of main.cpp:160-187"""
    to_int = _to_int()
    recs, nidx = {}, 0
    for s in fasta_seqs:
        s = bytes(s)
        has = False
        run = 0
        for ch in s:
            run = run + 1 if to_int[ch] else 0
            if run >= k:
                has = True
                break
        if len(s) >= k and not has:
            continue                     # (`continue` at :166: the counter stays)
        if has:
            recs[nidx] = s
        nidx += 1
    return recs


class PlacementModel:
    def __init__(self, fasta_seqs, k):
        self.k = int(k)
        self.records = gene_records(fasta_seqs, self.k)
        self._maps = {}

    def kmer_map(self, g):
        """canonical k-mer -> [(x, orientation bit)] over the record of g (palindromic windows left out)"""
        m = self._maps.get(g)
        if m is None:
            m = {}
            for x, canon, o in windows(self.records.get(g, b""), self.k):
                m.setdefault(canon, []).append((x, o))
            self._maps[g] = m
        return m

    def place_mate(self, g, mate):
        """(strand, pos, support) of one masked mate (bytes) against the record of g"""
        k, L = self.k, len(mate)
        m = self.kmer_map(g)
        votes = {}
        for p, canon, o in windows(mate, k):
            occ = m.get(canon)
            if occ is None or len(occ) != 1:
                continue
            x, xo = occ[0]
            strand = o ^ xo
            pos = x - p if strand == 0 else x + p + k - L
            votes[(strand, pos)] = votes.get((strand, pos), 0) + 1
        if not votes:
            return (0, 0, 0)
        (strand, pos), sup = min(votes.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))
        return (strand, pos, sup)


def masked_mates(batch, min_quality):
    """per read of a SoA batch (tests/synth.py) its mates as the classifier sees them: (mate 1, mate 2 or None), bytes behind the
    -q mask (so_join_mask over the pair, cut at the joiner again)"""
    from oracle import pyoracle
    L = pyoracle.lib()
    off1 = np.ascontiguousarray(batch["off1"], dtype=np.uint64)
    n = len(off1) - 1
    paired = batch.get("seq2") is not None
    off2 = np.ascontiguousarray(batch["off2"], dtype=np.uint64) if paired else None
    s1 = bytes(np.ascontiguousarray(batch["seq1"], dtype=np.uint8)) if n else b""
    s2 = bytes(np.ascontiguousarray(batch["seq2"], dtype=np.uint8)) if paired else b""
    q1 = bytes(np.ascontiguousarray(batch["qual1"], dtype=np.uint8)) if batch.get("qual1") is not None else None
    q2 = bytes(np.ascontiguousarray(batch["qual2"], dtype=np.uint8)) if (paired and batch.get("qual2") is not None) else None
    mq = int(min_quality) & 0xFF
    if mq and q1 is None:
        raise ValueError("-q %d and the batch has no qualities" % min_quality)
    for i in range(n):
        a, b = int(off1[i]), int(off1[i + 1])
        m1, k1 = s1[a:b], (q1[a:b] if q1 is not None else None)
        m2, k2 = None, None
        if paired:
            a2, b2 = int(off2[i]), int(off2[i + 1])
            m2, k2 = s2[a2:b2], (q2[a2:b2] if q2 is not None else None)
        buf = C.create_string_buffer(len(m1) + (len(m2) if paired else 0) + 2)
        m = L.so_join_mask(m1, len(m1), k1, m2, len(m2) if paired else 0, k2, int(paired), bytes([mq]), buf)
        j = buf.raw[:m]
        yield (j[:len(m1)], j[len(m1) + 1:] if paired else None)


def expected_placements(model, batch, gene_off, gene_ids, min_quality=0):
    """(n_assoc, 2, 3) int64 (strand, pos, support) per association and mate -- what SharkHip.placement_last hands out"""
    gene_off = np.asarray(gene_off)
    out = np.zeros((int(gene_off[-1]) if len(gene_off) else 0, 2, 3), dtype=np.int64)
    for i, (m1, m2) in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            out[j, 0] = model.place_mate(g, m1)
            if m2 is not None:
                out[j, 1] = model.place_mate(g, m2)
    return out


def placement_lines(ids, gene_off, gene_ids, placements, legend, paired):
    """the lines of `shark --placements`: <read> <gene> <strand1> <pos1> <support1> [<strand2> <pos2> <support2>]"""
    lines = []
    for i, rid in enumerate(ids):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            parts = [rid, legend[int(gene_ids[j])]] + [str(int(v)) for v in placements[j, 0]]
            if paired:
                parts += [str(int(v)) for v in placements[j, 1]]
            lines.append(" ".join(parts))
    return lines
