"""The yardstick for shk_segments_last and for the junctions computed from it -- include/shark_hip.h "segments".

Written from the semantics, in plain Python over bytes, on placement_model.py's definitions of record, window and vote:

  keys of a mate      every distinct (strand, pos) that received a vote, with support = its votes, first / last = the smallest /
                      largest voting slot
  ranking             support descending, then strand 0 first, then the smaller pos (rank 0 is the mate's placement)
  reported            the first m ranks and n_keys = the number of distinct keys; empty slots all 0
  span [lo, hi)       strand 0: pos + first, pos + last + k; strand 1: pos + L - k - last, pos + L - first
  junctions of a mate the reported segments with support >= s_min on rank 0's strand, sorted by (lo, hi); consecutive (A, B) with
                      pos_B > pos_A: (donor = hi_A, acceptor = lo_B, intron = pos_B - pos_A, overlap = hi_A + intron - lo_B)

Test infrastructure only."""
import numpy as np

from tests.placement_model import PlacementModel, masked_mates, windows


class SegmentsModel(PlacementModel):
    def mate_keys(self, g, mate):
        """every key of one masked mate (bytes) against the record of g, ranked: [(strand, pos, support, first, last)]"""
        k, L = self.k, len(mate)
        m = self.kmer_map(g)
        keys = {}
        for p, canon, o in windows(mate, k):
            occ = m.get(canon)
            if occ is None or len(occ) != 1:
                continue
            x, xo = occ[0]
            strand = o ^ xo
            pos = x - p if strand == 0 else x + p + k - L
            e = keys.get((strand, pos))
            if e is None:
                keys[(strand, pos)] = [1, p, p]
            else:
                e[0] += 1
                e[1] = min(e[1], p)
                e[2] = max(e[2], p)
        ranked = sorted(keys.items(), key=lambda kv: (-kv[1][0], kv[0][0], kv[0][1]))
        return [(s, pos, sup, first, last) for (s, pos), (sup, first, last) in ranked]

    def mate_segments(self, g, mate, m):
        """(n_keys, m rows (strand, pos, support, first, last)) -- what leaves the device for one mate"""
        keys = self.mate_keys(g, mate)
        rows = keys[:m] + [(0, 0, 0, 0, 0)] * (m - min(m, len(keys)))
        return len(keys), rows


def span(seg, L, k):
    strand, pos, _, first, last = (int(v) for v in seg)
    return (pos + first, pos + last + k) if strand == 0 else (pos + L - k - last, pos + L - first)


def junctions(rows, L, k, s_min=8):
    """[(donor, acceptor, intron, overlap)] of one mate of L bytes from its reported rows"""
    rows = [tuple(int(v) for v in r) for r in rows if int(r[2]) >= 1]
    if not rows:
        return []
    kept = []
    for r in rows:
        if r[2] >= s_min and r[0] == rows[0][0]:
            lo, hi = span(r, L, k)
            kept.append((lo, hi, r[1]))
    kept.sort(key=lambda t: (t[0], t[1]))
    out = []
    for a, b in zip(kept, kept[1:]):
        if b[2] > a[2]:
            intron = b[2] - a[2]
            out.append((a[1], b[0], intron, a[1] + intron - b[0]))
    return out


def expected_segments(model, batch, gene_off, gene_ids, m, min_quality=0):
    """((n_assoc, 2) uint32 n_keys, (n_assoc, 2, m, 5) int64 rows) -- what SharkHip.segments_last hands out"""
    gene_off = np.asarray(gene_off)
    n_assoc = int(gene_off[-1]) if len(gene_off) else 0
    keys = np.zeros((n_assoc, 2), dtype=np.uint32)
    rows = np.zeros((n_assoc, 2, m, 5), dtype=np.int64)
    for i, mates in enumerate(masked_mates(batch, min_quality)):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            for t, mate in enumerate(mates):
                if mate is not None:
                    keys[j, t], rows[j, t] = model.mate_segments(g, mate, m)
    return keys, rows


def mate_lengths(batch):
    """(n, 2) lengths in bytes of the mates of a SoA batch (0 for mate 2 of a single-end batch)"""
    off1 = np.asarray(batch["off1"], dtype=np.int64)
    out = np.zeros((len(off1) - 1, 2), dtype=np.int64)
    out[:, 0] = np.diff(off1)
    if batch.get("seq2") is not None:
        out[:, 1] = np.diff(np.asarray(batch["off2"], dtype=np.int64))
    return out


def segment_lines(ids, gene_off, gene_ids, keys, rows, legend, paired):
    """the lines of `shark --segments`: <read> <gene> and per mate <n_keys> and m x <strand> <pos> <support> <first> <last>"""
    lines = []
    for i, rid in enumerate(ids):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            parts = [rid, legend[int(gene_ids[j])]]
            for t in range(2 if paired else 1):
                parts.append(str(int(keys[j, t])))
                parts += [str(int(v)) for r in rows[j, t] for v in r]
            lines.append(" ".join(parts))
    return lines


def junction_lines(gene_off, gene_ids, rows, lengths, k, legend, s_min=8):
    """the lines of `shark --junctions`: <gene> <donor> <acceptor> <intron> <mates>, sorted by gene index, donor, acceptor"""
    table = {}
    for i in range(len(gene_off) - 1):
        for j in range(int(gene_off[i]), int(gene_off[i + 1])):
            g = int(gene_ids[j])
            for t in range(2):
                for donor, acceptor, intron, _ in junctions(rows[j, t], int(lengths[i, t]), k, s_min):
                    key = (g, donor, acceptor)
                    was = table.get(key, (intron, 0))
                    table[key] = (min(was[0], intron), was[1] + 1)    # (mates that disagree on the intron -- an indel next to the junction: the smallest)
    return ["%s %d %d %d %d" % (legend[g], d, a, table[(g, d, a)][0], table[(g, d, a)][1]) for g, d, a in sorted(table)]
