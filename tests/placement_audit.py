"""Entry-by-entry audit of the placement table ptab / pdir (shark_internal.hpp at DeviceIndex) against a model built
from the FASTA records and k alone.

`TableModel` states what the table must hold: per distinct (gene, canonical k-mer) pair of the reference its smallest global
position, its number of windows and -- for a pair with exactly one window -- that window's offset in its record and orientation;
from these the expected ptab (entries sorted by (pl_hash32, smallest global position)), ptab_n, ptab_lg, pdir and gene_start,
word for word.  The semantics are those of tests/placement_model.py (the pure-Python definition, which test_placement_audit.py
holds this model against pair by pair); the alphabet comes from oracle/pyoracle.py (so_to_int).  Nothing in the model comes from
the arrays under audit.

`audit(arrays, pmeta, gene_start, model)` returns a list of findings, each a string that starts with the array's name and the
index ("ptab[257]: ..."); an empty list means the table is right.  It compares the arrays exactly, names what differs (a pair
that is missing or appears twice, a wrong z word, a wrong gene, an entry out of order, a pdir word, the bucket count, a
gene_start entry), and runs the readers' lookup (pl_vote, placement_common.hpp) over the read-back arrays for every pair of the
model and for a sample of pairs the reference does not have.

`arrays` maps "ptab" and "pdir" to the arrays as shk_debug_index_array returns them (uint32; ptab four words per entry, the spare
entry behind ptab_n included), `pmeta` is {"ptab_lg", "ptab_n"}, `gene_start` is SharkHip.depth_layout().  numpy only; no GPU."""
import functools

import numpy as np

from tests import repeat_refs as rr
from tests import synth
from tests.index_audit import _report

U64 = np.uint64
XP1, XP2, XP3, XP4, XP5 = (U64(v) for v in (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                                            0x27D4EB2F165667C5))
AMBIGUOUS = 0xFFFFFFFF       # PTAB_AMBIGUOUS
MIN_LG = 6
MAX_BUCKET_SCAN = 4096       # entries of one bucket the lookup walks before it calls the directory broken


def _rotl(v, r):
    return (v << U64(r)) | (v >> U64(64 - r))


def xxh64_u64(v):
    """XXH64 (seed 0) of the 8 bytes of each uint64 of `v` (little endian) -- so_get_hash / xxh64_u64 of kmer_device.hpp"""
    v = np.asarray(v, dtype=U64)
    with np.errstate(over="ignore"):
        k1 = _rotl(v * XP2, 31) * XP1
        h = (XP5 + U64(8)) ^ k1
        h = _rotl(h, 27) * XP1 + XP4
        h ^= h >> U64(33)
        h = h * XP2
        h ^= h >> U64(29)
        h = h * XP3
        h ^= h >> U64(32)
    return h


def combined_word(gene, canon):
    """the word pl_hash32 hashes: canon ^ (gene + 1) * XP1"""
    with np.errstate(over="ignore"):
        return np.asarray(canon, dtype=U64) ^ ((np.asarray(gene, dtype=U64) + U64(1)) * XP1)


def pl_hash32(gene, canon):
    """placement_common.hpp: the top 32 bits of XXH64 over the k-mer with the gene folded in; int64 arrays of values < 2^32"""
    return (xxh64_u64(combined_word(gene, canon)) >> U64(32)).astype(np.int64)


def canonical_kmers(codes, k):
    """(fw, rc) per start position of a code array (0 .. 3), first base most significant; positions behind len - k hold rubbish"""
    n = len(codes)
    pad = np.concatenate([codes, np.zeros(k, dtype=codes.dtype)]).astype(U64)
    fw, rc = np.zeros(n, dtype=U64), np.zeros(n, dtype=U64)
    for j in range(k):
        c = pad[j:j + n]
        fw = (fw << U64(2)) | c
        rc |= (U64(3) - c) << U64(2 * j)
    return fw, rc


def random_canonical_kmers(rng, k, n):
    """up to n distinct canonical k-mers that are not their own reverse complement (uint64, sorted)"""
    v = rng.integers(0, 1 << (2 * k), size=n, dtype=np.uint64) if 4 ** k > 4 * n else np.arange(4 ** k, dtype=np.uint64)
    rc = np.zeros(len(v), dtype=U64)
    for j in range(k):                                     # base j from the right is the complement's base j from the left
        rc |= (U64(3) - ((v >> U64(2 * j)) & U64(3))) << U64(2 * (k - 1 - j))
    return np.unique(np.minimum(v, rc)[v != rc])


@functools.lru_cache(maxsize=None)
def find_collision(k, gene_a=0, gene_b=0, seed=1, n=600000):
    """two different pairs (gene_a, A), (gene_b, B) of canonical k-mers with equal pl_hash32, or None: a seeded search over n random
    canonical k-mers (all of them for a small k).  Deterministic.  With gene_a == gene_b the two k-mers differ; A < B then."""
    c = random_canonical_kmers(np.random.default_rng(seed), k, n)
    ha = pl_hash32(gene_a, c)
    if gene_a == gene_b:
        order = np.argsort(ha, kind="stable")
        hs = ha[order]
        hit = np.flatnonzero(hs[1:] == hs[:-1])
        if not len(hit):
            return None
        i = hit[0]
        return int(c[order[i]]), int(c[order[i + 1]])
    hb = pl_hash32(gene_b, c)
    order = np.argsort(hb, kind="stable")
    at = np.searchsorted(hb[order], ha)
    ok = np.flatnonzero((at < len(c)) & (hb[order][np.minimum(at, len(c) - 1)] == ha))
    if not len(ok):
        return None
    i = ok[0]
    return int(c[i]), int(c[order[at[i]]])


def kmer_bytes(v, k):
    """the k bases of k-mer value v, upper case"""
    return bytes(b"ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


class TableModel:
    """what ptab, pdir and gene_start must hold for these FASTA records at this k"""

    def __init__(self, fasta_seqs, k):
        from oracle import pyoracle
        L = pyoracle.lib()
        self.k = k = int(k)
        recs = [bytes(r) for r in fasta_seqs]
        n_rec = len(recs)
        rec_len = np.array([len(r) for r in recs], dtype=np.int64)
        rec_off = np.concatenate([[0], np.cumsum(rec_len)]).astype(np.int64)
        total = self.total = int(rec_off[-1])
        text = np.frombuffer(b"".join(recs), dtype=np.uint8)
        to_int = np.array([L.so_to_int(bytes([c])) for c in range(256)], dtype=np.int64)      # 0 = no base, else code + 1
        code = to_int[text] - 1
        rec_of = np.repeat(np.arange(n_rec, dtype=np.int64), rec_len)
        pos = np.arange(total, dtype=np.int64)
        fits = pos + k <= rec_off[1:][rec_of] if total else np.zeros(0, bool)
        nobase = np.concatenate([[0], np.cumsum(code < 0)])
        valid = fits & (nobase[np.minimum(pos + k, total)] - nobase[pos] == 0)
        fw, rc = canonical_kmers(np.maximum(code, 0), k)
        self.n_palindromic = int((valid & (fw == rc)).sum())
        # the numbering of the records (main.cpp:160-187): a record of at least k bases without any valid window takes no id
        has = np.zeros(n_rec, dtype=bool)
        has[rec_of[valid]] = True
        takes = ~((rec_len >= k) & ~has)
        gene_of_rec = np.cumsum(takes) - takes
        self.nidx = int(takes.sum())
        gs = np.zeros(self.nidx + 1, dtype=np.uint64)
        gs[gene_of_rec[has] + 1] = rec_len[has]
        self.gene_start = np.cumsum(gs).astype(np.uint64)
        self.ids_without_record = self.nidx - int(has.sum())
        # the windows that take part, and their pairs
        vx = np.flatnonzero(valid & (fw != rc))
        self.n_windows = len(vx)
        w_gene = gene_of_rec[rec_of[vx]]
        w_canon = np.minimum(fw[vx], rc[vx])
        w_orient = (fw[vx] < rc[vx]).astype(np.int64)
        w_x = vx - rec_off[rec_of[vx]]
        # by (gene, k-mer, position): the positions ascend already and so do their genes, so two stable sorts do it
        order = np.argsort(w_canon, kind="stable")
        order = order[np.argsort(w_gene[order].astype(np.uint16 if self.nidx <= 65536 else np.int64), kind="stable")]
        g_s, c_s = w_gene[order], w_canon[order]
        first = np.flatnonzero(np.concatenate([[True], (g_s[1:] != g_s[:-1]) | (c_s[1:] != c_s[:-1])])) if len(vx) else np.zeros(0, np.int64)
        count = np.diff(np.concatenate([first, [len(vx)]]))
        head = order[first]                                   # the pair's window with the smallest global position
        p_gene, p_canon, p_first = w_gene[head], w_canon[head], vx[head]
        p_z = np.where(count == 1, w_x[head] | (w_orient[head] << 31), AMBIGUOUS)
        p_hash = pl_hash32(p_gene, p_canon)
        # the table's order: (hash, smallest global position)
        t = np.argsort((p_hash.astype(U64) << U64(32)) | p_first.astype(U64))         # (positions are below 2^32)
        self.gene, self.canon, self.first, self.count, self.z, self.hash = p_gene[t], p_canon[t], p_first[t], count[t], p_z[t], p_hash[t]
        n = self.n = len(t)
        self.n_ambiguous = int((self.count > 1).sum())
        same = self.hash[1:] == self.hash[:-1]
        self.n_hash_groups = int((same & ~np.concatenate([[False], same[:-1]])).sum())     # hash groups of two or more pairs
        self.ptab = np.zeros((n, 4), dtype=np.uint32)
        self.ptab[:, 0] = (self.canon & U64(0xFFFFFFFF)).astype(np.uint32)
        self.ptab[:, 1] = (self.canon >> U64(32)).astype(np.uint32)
        self.ptab[:, 2] = self.z.astype(np.uint32)
        self.ptab[:, 3] = self.gene.astype(np.uint32)
        lg = MIN_LG
        while (1 << lg) < 2 * n:
            lg += 1
        self.lg = lg
        self.pdir = make_pdir(self.hash, lg)
        self._e_canon, self._e_gene = self.canon, self.gene.astype(np.int64)

    def entry_of(self, gene, canon):
        """index of the model's entry for each (gene, k-mer), -1 where the reference does not have the pair (a walk through the
        model's own directory)"""
        gene, canon = np.asarray(gene, dtype=np.int64), np.asarray(canon, dtype=U64)
        found, at, _ = _find(self._e_canon, self._e_gene, self.pdir, self.lg, self.n, gene, canon)
        assert found.max(initial=0) <= 1
        return at


def make_pdir(hashes, lg):
    """pdir as allocated for entries with these (ascending) hashes: 2^lg + 2 words, word b = the first entry whose bucket is >= b for
    b = 0 .. 2^lg, the spare word 0"""
    pdir = np.zeros((1 << lg) + 2, dtype=np.uint32)
    pdir[:(1 << lg) + 1] = np.searchsorted(np.asarray(hashes, dtype=np.int64) >> (32 - lg), np.arange((1 << lg) + 1), side="left")
    return pdir


def _entries(ptab_words, n):
    e = np.asarray(ptab_words, dtype=np.uint32)[:4 * n].reshape(n, 4)
    canon = e[:, 0].astype(U64) | (e[:, 1].astype(U64) << U64(32))
    return e, canon, e[:, 2].astype(np.int64), e[:, 3].astype(np.int64)


def _z_text(z):
    return "ambiguous" if z == AMBIGUOUS else "x=%d orientation=%d" % (z & 0x7FFFFFFF, z >> 31)


def _find(e_canon, e_gene, pdir, lg, n, gene, canon):
    """pl_vote's walk for arrays of pairs: bucket b = hash >> (32 - lg), entries pdir[b] .. pdir[b + 1] compared in full (k-mer and
    gene).  (number of entries found, index of the last one found or -1, findings about a directory the walk cannot follow)"""
    out = []
    b = pl_hash32(gene, canon) >> (32 - lg)
    pd = np.asarray(pdir).astype(np.int64)
    first, last = pd[b], pd[b + 1]
    _report(out, "pdir", (last > n) | (first > last), lambda i: "bucket [%d, %d) of a table of %d entries" % (first[i], last[i], n), b)
    first, last = np.minimum(first, n), np.minimum(last, n)
    span = int((last - first).max()) if len(b) else 0
    if span > MAX_BUCKET_SCAN:
        out.append("pdir[%d]: a bucket of %d entries" % (int(b[np.argmax(last - first)]), span))
        span = MAX_BUCKET_SCAN
    found = np.zeros(len(b), dtype=np.int64)
    where = np.full(len(b), -1, dtype=np.int64)
    live = np.arange(len(b))
    for j in range(max(span, 0)):
        live = live[first[live] + j < last[live]]
        a = first[live] + j
        hit = (e_canon[a] == canon[live]) & (e_gene[a] == gene[live])
        found[live[hit]] += 1
        where[live[hit]] = a[hit]
    return found, where, out


def lookup(ptab_words, pdir, lg, n, gene, canon):
    """the readers' lookup for arrays of pairs over the read-back arrays: (number of entries found, z of the last one found or -1,
    findings about the directory)"""
    e, e_canon, e_z, e_gene = _entries(ptab_words, n)
    found, where, out = _find(e_canon, e_gene, pdir, lg, n, np.asarray(gene, dtype=np.int64), np.asarray(canon, dtype=U64))
    return found, np.where(where >= 0, e_z[np.maximum(where, 0)] if n else 0, -1), out


def audit(arrays, pmeta, gene_start, model, n_absent=20000, seed=1):
    out, m = [], model
    ptab, pdir = np.asarray(arrays["ptab"]), np.asarray(arrays["pdir"])
    lg, n = int(pmeta["ptab_lg"]), int(pmeta["ptab_n"])
    # ---- the scalars and the sizes
    if n != m.n:
        out.append("pmeta[1]: ptab_n %d, expected %d" % (n, m.n))
    if lg != m.lg:
        out.append("pmeta[0]: ptab_lg %d (%d buckets), expected %d" % (lg, 1 << lg, m.lg))
    if len(ptab) != 4 * (n + 1):
        return out + ["ptab[0]: %d words for ptab_n %d, expected %d" % (len(ptab), n, 4 * (n + 1))]
    if not 0 < lg < 32 or len(pdir) != (1 << lg) + 2:
        return out + ["pdir[0]: %d words for ptab_lg %d" % (len(pdir), lg)]
    # ---- gene_start
    gs = np.asarray(gene_start).astype(np.int64)
    if len(gs) != len(m.gene_start):
        out.append("gene_start[0]: %d entries, expected %d" % (len(gs), len(m.gene_start)))
    else:
        want_gs = m.gene_start.astype(np.int64)
        _report(out, "gene_start", gs != want_gs, lambda i: "%d, expected %d" % (gs[i], want_gs[i]))
    # ---- the entries against the model's pairs
    e, canon, z, gene = _entries(ptab, n)
    idx = m.entry_of(gene, canon)
    known = idx >= 0
    # an entry in the place of a model entry with the same k-mer and another gene word: the gene is wrong, not the pair foreign
    same_place = np.zeros(n, dtype=bool)
    if n == m.n:
        same_place = ~known & (canon == m.canon) & (gene != m.gene)
        _report(out, "ptab", same_place, lambda i: "gene %d, expected %d (k-mer %#x)" % (gene[i], m.gene[i], int(canon[i])))
    _report(out, "ptab", ~known & ~same_place, lambda i: "pair (gene %d, k-mer %#x) is not in the reference" % (gene[i], int(canon[i])))
    times = np.bincount(idx[known], minlength=m.n)
    _report(out, "ptab", times == 0,
            lambda i: "pair (gene %d, k-mer %#x, first at position %d) is missing: this is its place in the expected table" % (m.gene[i], int(m.canon[i]), m.first[i]))
    second = np.flatnonzero(known)[times[idx[known]] > 1]
    _report(out, "ptab", second, lambda i: "pair (gene %d, k-mer %#x) appears %d times" % (gene[i], int(canon[i]), times[idx[i]]))
    kz = np.flatnonzero(known)
    bad_z = kz[z[kz] != m.z[idx[kz]]]
    _report(out, "ptab", bad_z, lambda i: "z word %s, expected %s (gene %d, k-mer %#x, %d windows)"
            % (_z_text(int(z[i])), _z_text(int(m.z[idx[i]])), gene[i], int(canon[i]), m.count[idx[i]]))
    # ---- the order: (hash, smallest global position), the hash from the entry's own words as pl_dir_kernel takes it
    h = pl_hash32(gene, canon)
    fp = np.where(known, m.first[np.maximum(idx, 0)] if m.n else 0, -1)
    prev_h, prev_fp = h[:-1], fp[:-1]
    back = (h[1:] < prev_h) | ((h[1:] == prev_h) & known[1:] & known[:-1] & (fp[1:] <= prev_fp))
    _report(out, "ptab", np.flatnonzero(back) + 1, lambda i: "out of order: (hash %#x, first position %d) behind (hash %#x, first position %d)"
            % (h[i], fp[i], h[i - 1], fp[i - 1]))
    # ---- the directory
    if lg == m.lg:
        _report(out, "pdir", pdir != m.pdir, lambda i: "%d, expected %d" % (pdir[i], m.pdir[i]))
    else:
        own = make_pdir(np.sort(h), lg)
        _report(out, "pdir", pdir != own, lambda i: "%d, the entries' own hashes give %d" % (pdir[i], own[i]))
    # ---- whatever the named checks did not name
    if n == m.n and not out and not np.array_equal(e, m.ptab):
        _report(out, "ptab", (e != m.ptab).any(axis=1), lambda i: "%s, expected %s" % (e[i].tolist(), m.ptab[i].tolist()))
    # ---- the readers' lookup, for every pair of the reference ...
    found, fz, notes = lookup(ptab, pdir, lg, n, m.gene, m.canon)
    out += notes
    _report(out, "lookup", found == 0, lambda i: "pair (gene %d, k-mer %#x) is not found in its bucket" % (m.gene[i], int(m.canon[i])))
    _report(out, "lookup", found > 1, lambda i: "pair (gene %d, k-mer %#x) is found %d times" % (m.gene[i], int(m.canon[i]), found[i]))
    _report(out, "lookup", (found == 1) & (fz != m.z), lambda i: "pair (gene %d, k-mer %#x) answers %s, expected %s"
            % (m.gene[i], int(m.canon[i]), _z_text(int(fz[i])), _z_text(int(m.z[i]))))
    # ---- ... and for pairs it does not have: its k-mers under another gene id, and random k-mers
    rng = np.random.default_rng(seed)
    a_gene, a_canon = [], []
    if m.n:
        pick = rng.integers(0, m.n, size=n_absent)
        for other in (m.gene[pick] + 1, np.maximum(m.gene[pick] - 1, 0), np.full(n_absent, m.nidx), rng.integers(0, max(m.nidx, 1), size=n_absent)):
            a_gene.append(other)
            a_canon.append(m.canon[pick])
    a_gene.append(rng.integers(0, max(m.nidx, 1) + 1, size=n_absent))
    a_canon.append(rng.integers(0, 1 << (2 * m.k), size=n_absent, dtype=np.uint64))
    a_gene, a_canon = np.concatenate(a_gene), np.concatenate(a_canon)
    absent = m.entry_of(a_gene, a_canon) < 0
    a_gene, a_canon = a_gene[absent], a_canon[absent]
    found, _, notes = lookup(ptab, pdir, lg, n, a_gene, a_canon)
    out += [x for x in notes if x not in out]
    _report(out, "lookup", found > 0, lambda i: "pair (gene %d, k-mer %#x) is not in the reference and is found" % (a_gene[i], int(a_canon[i])))
    return out


def pull(h):
    """(arrays, pmeta, gene_start) of a SharkHip built with keep_positions"""
    arrays = {name: h.debug_index_array(name) for name in ("ptab", "pdir")}
    pmeta = dict(zip(h.DEBUG_PMETA, (int(x) for x in h.debug_index_array("pmeta"))))
    return arrays, pmeta, h.depth_layout()


# ---------------------------------------------------------------------------------------------------------------------------
# the case table: references at the smallest shapes at which the builder can still go wrong, each with what it must contain
# (a reference that lost its edge fails its case).  needs: "ambiguous" a pair with two or more windows, "group" a hash group of
# two or more pairs, "palindrome" a window that is its own reverse complement, "noid" an id without a record, "empty" no pair at all.
# ---------------------------------------------------------------------------------------------------------------------------
N = ord("N")
KS = (5, 16, 17, 31)
COLLISION_KS = (9, 17, 31)
ACROSS_KS = (9, 16, 17, 31)                              # (k = 5 has 512 canonical k-mers a gene: no two pairs share 32 bits of hash)
TILE_TOTALS = (1, None, 4095, 4096, 4097, 8193)          # None: k bases
MANY_TILES_TOTAL = 1024 * 4096 + 4097


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _rc(s):
    return bytes(synth.revcomp(np.frombuffer(bytes(s), np.uint8)))


def _join(*parts):
    return b"".join(bytes(p) for p in parts)


def ref_example(k, example_dir):
    import os
    return [s for _, s in synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))]


def ref_collision_interleaved(k, _=None):
    """gene 0: A ... B ... A, gene 1: B ... A ... A ... B for two k-mers of equal pl_hash32 in gene 0: the builder's walks must pass
    a foreign pair to find their own"""
    a, b = (kmer_bytes(v, k) for v in find_collision(k))
    rng = _rng(700, k)
    s = lambda: synth.random_seq(rng, int(rng.integers(30, 200)))  # noqa: E731
    return [_join(s(), a, s(), b, s(), a, s()), _join(s(), b, s(), a, s(), a, s(), b, s())]


def ref_collision_across_genes(k, _=None):
    """A in gene 0 and B in gene 1 with pl_hash32(0, A) == pl_hash32(1, B)"""
    a, b = (kmer_bytes(v, k) for v in find_collision(k, 0, 1))
    rng = _rng(710, k)
    s = lambda: synth.random_seq(rng, int(rng.integers(30, 200)))  # noqa: E731
    return [_join(s(), a, s()), _join(s(), b, s())]


def both_strands_kmer(k):
    return bytes(synth.random_seq(_rng(720, k), k - 2)) + b"CC"        # (ends in CC, its reverse complement starts with GG: no palindrome)


def ref_both_strands(k, _=None):
    """a k-mer and its reverse complement in one record (ambiguous), and the same in two different records (two unique entries with
    opposite orientation)"""
    km = both_strands_kmer(k)
    rng = _rng(721, k)
    s = lambda: synth.random_seq(rng, int(rng.integers(20, 60)))  # noqa: E731
    return [_join(s(), km, s(), _rc(km), s()), _join(s(), km, s()), _join(s(), _rc(km), s())]


def ref_record_ends(k, _=None):
    """records that end at concatenated positions 255, 256, 257 and 256 + k - 1, then one that fills up to 1 100 bases"""
    rng = _rng(730, k)
    lens = [255, 1, 1, k - 2]
    assert list(np.cumsum(lens)) == [255, 256, 257, 256 + k - 1]
    return [bytes(synth.random_seq(rng, n)) for n in lens + [1100 - sum(lens)]]


def ref_short_records(k, _=None):
    """records of 0, k - 1, k and k + 1 bases, an all-N record of at least k bases (takes no id), an all-N record shorter than k (takes
    an id, has no record), an empty first and last record"""
    rng = _rng(740, k)
    r = lambda n: bytes(synth.random_seq(rng, n))  # noqa: E731
    return [b"", r(100), b"", r(k - 1), r(k), b"N" * (k + 2), r(k + 1), r(200), b"N" * min(3, k - 1), r(150), b""]


def ref_only_n(k, _=None):
    return [b"N" * (k + 5), b"N" * (k - 1), b"n" * (2 * k)]


def ref_only_short(k, _=None):
    rng = _rng(750, k)
    return [bytes(synth.random_seq(rng, k - 1)), b"", bytes(synth.random_seq(rng, 1)), bytes(synth.random_seq(rng, k - 1))]


def ref_only_palindromes(k, _=None):
    assert k % 2 == 0
    return [b"AT" * 40, b"CG" * k]


def ref_one_record(total):
    def make(k, _=None):
        n = k if total is None else total
        return [bytes(synth.random_seq(_rng(760, k, n), n))]
    return make


def ref_repeats(k, _=None):
    """low-complexity runs (homopolymers of up to 1 000 bases, (AT)n: even-k palindromes), a tandem array, paralog families with a
    duplicate and a reverse complement, poly-A carriers"""
    rng = _rng(770, k)
    genes, _m = rr.compose(rr.low_complexity(rng, rr.plain(rng, 12, 200, 500)[0], k), rr.tandem(rng, 37, 12, True), rr.families(rng, 2, 3, 400, 0.95),
                           rr.poly_a_carriers(rng, 10))
    return [bytes(g) for g in genes]


def ref_lower_and_n(k, _=None):
    """5 % lower case, an N every few hundred bases"""
    rng = _rng(780, k)
    out = []
    for g in synth.make_genes(rng, 20, 300, 800, share_every=4):
        g = g.copy()
        g[200:200 + 2 * k] = g[40:40 + 2 * k]                  # (a stretch twice in the gene: ambiguous pairs, in differing case)
        g[rng.random(len(g)) < 0.05] |= 0x20
        g[np.flatnonzero(rng.random(len(g)) < 1 / 300.0)] = N
        g[len(g) // 2] = ord("n")
        out.append(bytes(g))
    return out


def ref_many_tiles(k=17, _=None):
    """1024 * 4096 + 4097 bases in about 2 000 records: more than 1 024 scan tiles, a ptab_lg of 23"""
    rng = _rng(790)
    cuts = np.sort(rng.choice(np.arange(1, MANY_TILES_TOTAL), size=1999, replace=False))
    s = synth.random_seq(rng, MANY_TILES_TOTAL)
    return [bytes(p) for p in np.split(s, cuts)]


def _check_interleaved(m, k):
    a, b = find_collision(k)
    ea, eb = m.entry_of([0, 1], [a, a]), m.entry_of([0, 1], [b, b])
    assert (ea >= 0).all() and (eb >= 0).all()
    assert m.hash[ea[0]] == m.hash[eb[0]] and abs(int(ea[0]) - int(eb[0])) == 1                 # one hash group
    assert m.count[ea].tolist() == [2, 2] and m.count[eb].tolist() == [1, 2]


def _check_across(m, k):
    a, b = find_collision(k, 0, 1)
    e = m.entry_of([0, 1], [a, b])
    assert (e >= 0).all() and m.hash[e[0]] == m.hash[e[1]] and e[1] == e[0] + 1 and m.gene[e].tolist() == [0, 1]


def _check_both_strands(m, k):
    km = both_strands_kmer(k)
    w = TableModel([km], k)                                     # (the k-mer alone: its canonical form and orientation)
    e = m.entry_of([0, 1, 2], [w.canon[0]] * 3)
    assert (e >= 0).all() and m.count[e].tolist() == [2, 1, 1]
    assert sorted((m.z[e[1:]] >> 31).tolist()) == [0, 1] and (m.z[e[1]] >> 31) == (w.z[0] >> 31)


def _check_empty(m, k):
    assert m.n == 0 and m.lg == MIN_LG and not m.pdir.any()


def _case(name, ref, ks, needs, check=None, small=True, at_k=None):
    """one case per k; at_k: {k: what the reference must contain at that k on top of `needs`}"""
    return [{"id": "%s-k%d" % (name, k), "ref": ref, "k": k, "needs": frozenset(needs) | frozenset((at_k or {}).get(k, ())), "check": check, "small": small}
            for k in ks]


CASES = (_case("example", ref_example, KS, ["ambiguous"])
         + _case("collision-interleaved", ref_collision_interleaved, COLLISION_KS, ["ambiguous", "group"], _check_interleaved)
         + _case("collision-across-genes", ref_collision_across_genes, ACROSS_KS, ["group"], _check_across)
         + _case("both-strands", ref_both_strands, KS, ["ambiguous"], _check_both_strands)
         + _case("record-ends", ref_record_ends, KS, ["noid"])
         + _case("short-records", ref_short_records, KS, ["noid"])
         + _case("only-N", ref_only_n, KS, ["empty", "noid"], _check_empty)
         + _case("only-short", ref_only_short, KS, ["empty", "noid"], _check_empty)
         + _case("only-palindromes", ref_only_palindromes, (16,), ["empty", "palindrome"], _check_empty)
         + [c for t in TILE_TOTALS for c in _case("total-%s" % ("k" if t is None else t), ref_one_record(t), KS, [])]
         + _case("repeats", ref_repeats, KS, ["ambiguous"], at_k={16: ["palindrome"]})
         + _case("lower-and-N", ref_lower_and_n, KS, ["ambiguous"])
         + _case("many-tiles", ref_many_tiles, (17,), [], small=False))


def declared(m, needs):
    """what of `needs` the model's reference does not have (empty: the reference still has its edge)"""
    have = {"ambiguous": m.n_ambiguous > 0, "group": m.n_hash_groups > 0, "palindrome": m.n_palindromic > 0, "noid": m.ids_without_record > 0,
            "empty": m.n == 0}
    return sorted(x for x in needs if not have[x])
