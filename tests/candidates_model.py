"""The yardstick for shk_candidates_last: per read (pair) of a batch the reference's per-read map gene -> (cov, nk)
(ReadAnalyzer.hpp:39-88), ranked as ReadAnalyzer.hpp:90-102 would pick its entries if each winner were removed in turn: cov
descending, then nk descending, then gene id ascending (the map's iteration order among equals).

Written from the semantics, with what oracle/pyoracle.py already exposes: FastqSplitter's join and quality mask
(so_join_mask), the filter's answer per k-mer (get_index, index_kmer) and, as a check on every read it computes,
ReadAnalyzer::operator() itself (so_analyze_read): the model's top (cov, nk) must be the oracle's (max, maxk), its len the
oracle's len, and its leading tie group the genes the oracle keeps at c = 0 -- so the model cannot drift from the oracle
unnoticed.  Test infrastructure only."""
import ctypes as C

import numpy as np

from tests.evidence_model import handworked_batch, handworked_cases  # noqa: F401  (re-exported for the tests)

SHK_MAX_CANDIDATES = 8
_TO_INT = None


def _to_int():
    """kmer_utils.hpp's to_int: 0 for a character that is no base, else 1 + the base's 2-bit code"""
    global _TO_INT
    if _TO_INT is None:
        from oracle import pyoracle
        L = pyoracle.lib()
        _TO_INT = [int(L.so_to_int(bytes([c]))) for c in range(256)]
    return _TO_INT


def read_map(oracle_shark, joined, index_kmer=None):
    """The walk of ReadAnalyzer.hpp:39-88 over one joined and masked string: (len, {gene: [cov, nk, last]}).

    len counts the valid characters (:46-49); a read with len < k has an empty map (:50).  The k-mers are rolled over the
    string, forward and reverse complement side by side (kmer_utils.hpp:73-79), and start again behind an invalid character
    (:66-71; build_kmer, kmer_utils.hpp:57-71, finds the next k valid characters in a row), so a k-mer is looked up exactly
    where the last k characters are all valid.  For every id of the canonical k-mer's list index_kmer[start..end]
    (bloomfilter.h:78-102; an id may be listed several times on an index of more than 65 536 records):
      the read's FIRST valid k-mer (:51-62), with pos one past its end:  cov += min(k, pos - last); nk = 1; last = pos - 1
      every later one (:72-86), with pos its last character's index:     cov += min(k, pos - last); nk += 1; last = pos
    where a new entry starts as (0, 0, 0) and `pos - last` is taken in unsigned arithmetic as the reference takes it."""
    to_int = _to_int()
    k = int(oracle_shark.k)
    if index_kmer is None:
        index_kmer = oracle_shark.index_kmer()
    ln = sum(1 for ch in joined if to_int[ch] > 0)
    genes = {}
    if ln < k:
        return ln, genes
    mask = (1 << (2 * k)) - 1
    fw = rc = 0
    run = 0          # valid characters in a row up to here
    first = True
    for end, ch in enumerate(joined):
        code = to_int[ch]
        if code == 0:
            run = 0
            fw = rc = 0
            continue
        code -= 1
        fw = ((fw << 2) | code) & mask
        rc = (rc >> 2) | ((3 - code) << (2 * k - 2))
        run += 1
        if run < k:
            continue
        start, stop = oracle_shark.get_index(min(fw, rc))
        pos = end + 1 if first else end
        for j in range(start, stop + 1):
            e = genes.setdefault(int(index_kmer[j]), [0, 0, 0])
            e[0] += min(k, (pos - e[2]) & 0xFFFFFFFF)
            if first:
                e[1] = 1
                e[2] = pos - 1
            else:
                e[1] += 1
                e[2] = pos
        first = False
    return ln, genes


def rank(genes):
    """[(gene, cov, nk)] by cov descending, nk descending, gene ascending"""
    return sorted(((g, e[0], e[1]) for g, e in genes.items()), key=lambda t: (-t[1], -t[2], t[0]))


def joined_reads(oracle_shark, batch):
    """the joined and masked string of every read (pair) of a SoA batch (tests/synth.py), as FastqSplitter hands it on"""
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
    mq = int(oracle_shark.min_quality) & 0xFF                       # the reference's `char min_quality` (argument_parser.hpp:144)
    if mq and q1 is None:
        raise ValueError("the oracle masks by quality (-q %d) and the batch has none" % oracle_shark.min_quality)
    for i in range(n):
        a, b = int(off1[i]), int(off1[i + 1])
        m1, k1 = s1[a:b], (q1[a:b] if q1 is not None else None)
        m2, k2 = None, None
        if paired:
            a2, b2 = int(off2[i]), int(off2[i + 1])
            m2, k2 = s2[a2:b2], (q2[a2:b2] if q2 is not None else None)
        buf = C.create_string_buffer(len(m1) + (len(m2) if paired else 0) + 2)
        m = L.so_join_mask(m1, len(m1), k1, m2, len(m2) if paired else 0, k2, int(paired), bytes([mq]), buf)
        yield buf.raw[:m]


def expected_candidates(oracle_shark, batch, m):
    """oracle_shark: an oracle.pyoracle.Shark with its index built; batch: the SoA dict of tests/synth.py; m: 1 .. 8.
    Returns (reads, entries): an (n, 2) uint32 array (len, n_genes) and an (n, m, 3) uint32 array (gene, cov, nk) in rank
    order with empty slots (0, 0, 0) last -- what shk_candidates_last hands out."""
    assert 1 <= m <= SHK_MAX_CANDIDATES
    index_kmer = oracle_shark.index_kmer()
    reads, entries = [], []
    for joined in joined_reads(oracle_shark, batch):
        ln, genes = read_map(oracle_shark, joined, index_kmer)
        ranked = rank(genes)
        # the model is pinned to the oracle on every read it computes
        kept, mx, mk, oln = oracle_shark.analyze(joined)
        assert ln == oln, (joined, ln, oln)
        assert (ranked[0][1:] if ranked else (0, 0)) == (mx, mk), (joined, ranked[:2], mx, mk)
        head = [g for g, cv, nk in ranked if (cv, nk) == (mx, mk)]
        if float(oracle_shark.c) == 0.0 and not oracle_shark.single:
            assert head == kept, (joined, head, kept)          # (max >= 0 * len always holds: the oracle keeps the whole tie group)
        elif kept:
            assert head == kept, (joined, head, kept)          # (what it keeps at another c, if anything, is that group too)
        reads.append((ln, len(ranked)))
        row = [list(t) for t in ranked[:m]] + [[0, 0, 0]] * (m - min(m, len(ranked)))
        entries.append(row)
    n = len(reads)
    return (np.array(reads, dtype=np.uint32).reshape(n, 2), np.array(entries, dtype=np.uint32).reshape(n, m, 3))


def tie_group(entries_row):
    """the leading entries of one read that share entry 0's (cov, nk): the genes the ordinary path returns when the read passes"""
    row = np.asarray(entries_row)
    if row.shape[0] == 0 or row[0, 2] == 0:
        return []
    return [int(g) for g, cv, nk in row if nk != 0 and (cv, nk) == (row[0, 1], row[0, 2])]


def thresholded(reads, entries, c, single):
    """ReadAnalyzer.hpp:104 applied on the host to records with a COMPLETE leading tie group (m large enough): per read the
    genes the ordinary path returns"""
    out = []
    for (ln, n_genes), row in zip(np.asarray(reads), np.asarray(entries)):
        grp = tie_group(row)
        ok = bool(grp) and float(row[0, 1]) >= float(c) * float(ln) and (not single or len(grp) == 1)
        out.append(grp if ok else [])
    return out


def candidate_lines(ids, reads, entries, legend):
    """the lines of `shark --candidates`: <id> <len> <n_genes> and <gene> <cov> <nk> per filled entry"""
    lines = []
    for rid, (ln, ng), row in zip(ids, np.asarray(reads), np.asarray(entries)):
        parts = [rid, str(int(ln)), str(int(ng))]
        for g, cv, nk in row:
            if nk == 0:
                break
            parts += [legend[int(g)], str(int(cv)), str(int(nk))]
        lines.append(" ".join(parts))
    return lines
