"""Entry-by-entry audit of the derived index arrays against a first-principles model.

`Model` is built from the FASTA records, k, bf_bits and the CPU oracle alone: per base position of the concatenated records
whether a k-mer starts there, its value, strand, filter position, rank and gene list.  Nothing in it comes from the arrays under
audit.  `audit_<array>(model, arrays, meta)` returns a list of violations, each a string that starts with the array's name and
the index ("refpay[257]: ...").  Exact equality wherever the content is determined, invariants where the order of the build's
atomic operations is free (which slot of its probe path a key of `tab` sits in).  numpy and ctypes only; no GPU.

`arrays` maps a name to the array as shk_debug_index_array returns it (SharkHip.debug_index_array), `meta` is
SharkHip.debug_index_meta()."""
import ctypes as C

import numpy as np

TAB_OVERFLOW = 1 << 30
TAB_PAYLOAD = 0x3FFFFFFF
NONE32 = 0xFFFFFFFF          # REFPAY_NONE, REFEXT_NONE, an unset occurrence of atab
REFEXT_CLIP = 254
LTAB_SLOT_LG, LTAB_GROUP_LG, LTAB_ESC = 15, 13, 0x1FFF
MAX_REPORT = 6               # violations listed per check (the first ones; the count is in the last line)

ARRAYS = ("rank_w", "ent", "ids", "sum32", "lsum32", "lbig32", "tab", "atab", "ltab", "ref2", "refpay", "refext", "refmul")


def _report(out, name, bad, what, idx=None):
    """append "<name>[i]: what(i)" for the first indices of the boolean / index array `bad`"""
    bad = np.asarray(bad)
    where = np.flatnonzero(bad) if bad.dtype == bool else bad
    for n, i in enumerate(where[:MAX_REPORT]):
        j = int(i if idx is None else idx[i])
        out.append("%s[%d]: %s" % (name, j, what(int(i)) if callable(what) else what))
    if len(where) > MAX_REPORT:
        out.append("%s[...]: %d such entries in all" % (name, len(where)))


class Model:
    """what the index must say about every base position of the reference, from the records and the oracle"""

    def __init__(self, oracle, o, records, k, bf_bits):
        """oracle: the pyoracle module; o: its Shark(k, bf_bits) with `records` built"""
        L = oracle.lib()
        self.k, self.bf_bits = k, bf_bits
        recs = [bytes(r) for r in records]
        self.rec_len = np.array([len(r) for r in recs], dtype=np.int64)
        self.rec_off = np.concatenate([[0], np.cumsum(self.rec_len)]).astype(np.int64)
        total = self.total = int(self.rec_off[-1])
        self.bytes = np.frombuffer(b"".join(recs), dtype=np.uint8)
        # so_to_int: 0 = invalid, else code + 1
        to_int = np.array([L.so_to_int(bytes([c])) for c in range(256)], dtype=np.int64)
        code = to_int[self.bytes] - 1
        self.code = code
        self.rec_of = np.repeat(np.arange(len(recs), dtype=np.int64), self.rec_len)
        rec_end = self.rec_off[1:][self.rec_of] if total else np.zeros(0, np.int64)
        x = np.arange(total, dtype=np.int64)
        inval = np.concatenate([[0], np.cumsum(code < 0)])
        fits = x + k <= rec_end
        xe = np.minimum(x + k, total)
        self.valid = fits & (inval[xe] - inval[x] == 0)
        # forward value of the k-mer starting at x (first base most significant)
        pad = np.concatenate([np.maximum(code, 0), np.zeros(k, np.int64)]).astype(np.uint64)
        fw = np.zeros(total, dtype=np.uint64)
        for j in range(k):
            fw = (fw << np.uint64(2)) | pad[j:j + total]
        vx = np.flatnonzero(self.valid)
        self.vx = vx
        self.fw = fw
        rc = np.zeros(total, dtype=np.uint64)
        rc[vx] = [L.so_revcompl(int(v), k) for v in fw[vx]]
        self.rc = rc
        self.strand = ~(fw < rc) & self.valid                 # 1 = the reverse complement is the stored form (fw == rc included)
        self.canon = np.where(fw < rc, fw, rc)
        pos = np.zeros(total, dtype=np.uint64)
        pos[vx] = [L.so_get_hash(int(v)) % bf_bits for v in self.canon[vx]]
        self.pos = pos
        # the oracle's filter: its set bits in ascending order (rank r <-> setbits[r])
        words = o.bf_words()
        self.n_words = len(words)
        nz = np.flatnonzero(words)
        self.nz_words, self.nz_counts = nz, np.bitwise_count(words[nz]).astype(np.int64)
        bits = np.unpackbits(words[nz].view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
        wi, bi = np.nonzero(bits)
        self.setbits = (nz[wi].astype(np.uint64) << np.uint64(6)) | bi.astype(np.uint64)
        self.n_set = len(self.setbits)
        if self.n_set != o.num_kmer():
            raise AssertionError("model: %d set bits in the oracle's words, the oracle says %d" % (self.n_set, o.num_kmer()))
        rank = np.searchsorted(self.setbits, pos[vx])
        if len(vx) and (rank.max() >= self.n_set or not np.array_equal(self.setbits[rank], pos[vx])):
            raise AssertionError("model: a reference k-mer whose bit the oracle's filter does not have")
        self.rank = np.full(total, -1, dtype=np.int64)
        self.rank[vx] = rank
        if len(np.unique(rank)) != self.n_set:
            raise AssertionError("model: a set bit of the oracle's filter that no reference k-mer hits")
        # the oracle's lists, rank by rank
        self.ids = o.index_kmer().astype(np.uint16)
        self.tot_idx = len(self.ids)
        off = np.full(self.n_set + 1, -1, dtype=np.int64)
        off[self.n_set] = self.tot_idx
        end = np.full(self.n_set, -1, dtype=np.int64)
        _, first = np.unique(rank, return_index=True)
        for i in first:
            s, e = o.get_index(int(self.canon[vx[i]]))
            off[rank[i]], end[rank[i]] = s, e + 1
        if not np.array_equal(off[1:], end) or off[0] != 0:
            raise AssertionError("model: the oracle's lists do not tile its id array")
        self.off = off
        self.list_len = np.diff(off)
        self.gene0 = self.ids[off[:-1]].astype(np.int64)
        # the reference's gene numbering (a record of at least k bases without any valid k-mer does not advance the number)
        has = np.zeros(len(recs), dtype=bool)
        has[self.rec_of[vx]] = True
        g, self.gene_of_rec = 0, np.zeros(len(recs), dtype=np.int64)
        for r in range(len(recs)):
            self.gene_of_rec[r] = g
            if not (self.rec_len[r] >= k and not has[r]):
                g += 1
        self.nidx = g
        if o.nidx is not None and o.nidx != g:
            raise AssertionError("model: %d genes by the numbering rule, the oracle counted %d" % (g, o.nidx))
        # per position: single-gene list?, its length
        self.plen = np.zeros(total, dtype=np.int64)
        self.plen[vx] = self.list_len[rank]
        self.single = self.valid & (self.plen == 1)
        self.multi_R = int(self.plen[self.plen > 1].sum())    # ids the per-position copies of the multi-gene lists take

    def list_at(self, x):
        r = self.rank[x]
        return self.ids[self.off[r]:self.off[r + 1]]

    def perpos_expected(self):
        """the per-position copies are built unless they would take more than 16 ids per base (index_build.hip)"""
        return self.multi_R <= 16 * self.total


def _ent_fields(ent_words):
    w = np.asarray(ent_words, dtype=np.uint32)
    return w[0::2].astype(np.int64), (w[1::2] & 0xFFFF).astype(np.int64), (w[1::2] >> 16).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
def audit_rank_w(m, A, meta):
    out, a = [], A["rank_w"]
    nw = meta["bf_words64"]
    if len(a) != nw + 2:
        return ["rank_w[0]: %d words, expected %d" % (len(a), nw + 2)]
    exp = np.zeros(nw + 2, dtype=np.int64)
    exp[m.nz_words + 1] = m.nz_counts
    np.cumsum(exp[:nw + 1], out=exp[:nw + 1])                 # exclusive prefix; entry nw = n_set; the word behind it stays 0
    diff = a.astype(np.int64) != exp
    diff[nw] = False
    _report(out, "rank_w", diff, lambda i: "%d, expected %d" % (a[i], exp[i]))
    if int(a[nw]) != m.n_set:
        out.append("rank_w[%d]: last entry %d is not n_set %d" % (nw, a[nw], m.n_set))
    return out


def audit_ent(m, A, meta):
    out = []
    start, ln, g0 = _ent_fields(A["ent"])
    if meta["n_set"] != m.n_set or len(start) < m.n_set + 1:
        return ["ent[0]: n_set %d / %d entries, the oracle has %d set bits" % (meta["n_set"], len(start), m.n_set)]
    n = m.n_set
    _report(out, "ent", start[:n] != m.off[:n], lambda i: "start %d, expected %d" % (start[i], m.off[i]))
    elen = np.minimum(m.list_len, 0xFFFF)
    _report(out, "ent", ln[:n] != elen, lambda i: "len %d, expected %d" % (ln[i], elen[i]))
    _report(out, "ent", g0[:n] != m.gene0, lambda i: "gene0 %d, expected %d" % (g0[i], m.gene0[i]))
    if (start[n], ln[n], g0[n]) != (m.tot_idx, 0, 0):
        out.append("ent[%d]: sentinel {%d, %d, %d}, expected {%d, 0, 0}" % (n, start[n], ln[n], g0[n], m.tot_idx))
    return out


def audit_ids(m, A, meta):
    out, ids = [], A["ids"]
    if meta["tot_idx"] != m.tot_idx or len(ids) < m.tot_idx:
        return ["ids[0]: tot_idx %d / %d ids, the oracle has %d" % (meta["tot_idx"], len(ids), m.tot_idx)]
    _report(out, "ids", ids[:m.tot_idx] != m.ids, lambda i: "%d, expected %d" % (ids[i], m.ids[i]))
    return out


def _audit_summary(name, shift_key, n_bits, m, A, meta):
    out, a = [], A[name]
    sh = meta[shift_key]
    bits = n_bits if n_bits is not None else m.bf_bits >> sh
    if len(a) != (bits + 31) // 32 + 2:
        return ["%s[0]: %d words, expected %d" % (name, len(a), (bits + 31) // 32 + 2)]
    exp = np.zeros(len(a), dtype=np.uint32)
    j = np.unique(m.setbits >> np.uint64(sh)).astype(np.int64)
    np.bitwise_or.at(exp, j >> 5, (np.uint32(1) << (j & 31).astype(np.uint32)))
    _report(out, name, (a & ~exp) != 0, lambda i: "bits %#x set over clear filter ranges (or in the padding)" % int(a[i] & ~exp[i]))
    _report(out, name, (exp & ~a) != 0, lambda i: "bits %#x clear over set filter bits" % int(exp[i] & ~a[i]))
    return out


def audit_sum32(m, A, meta):
    return _audit_summary("sum32", "sum_shift", None, m, A, meta)


def audit_lsum32(m, A, meta):
    return _audit_summary("lsum32", "lsum_shift", 1 << 18, m, A, meta)


def audit_lbig32(m, A, meta):
    return _audit_summary("lbig32", "lbig_shift", 1 << 20, m, A, meta)


def expected_low(m, rk):
    """the low word of a table slot (tab and ktab alike) whose key has the filter position of rank rk: the gene of a single-gene
    list, else multi | rank"""
    rk = np.asarray(rk, dtype=np.int64)
    return np.where(m.list_len[rk] == 1, m.gene0[rk], (1 << 31) | rk)


def _tab_decode(tab, lg):
    """valid slots of the table body: slot index, bucket, displacement, home, decoded position"""
    nb = 1 << lg
    body = tab[:2 * nb]
    hi = (body >> np.uint64(32)).astype(np.int64)
    lo = (body & np.uint64(0xFFFFFFFF)).astype(np.int64)
    validm = (hi & 0x80) != 0
    idx = np.flatnonzero(validm)
    d = hi[idx] & 0x7F
    home = ((idx >> 1) - d) & (nb - 1)
    p = ((hi[idx] >> 8).astype(np.uint64) << np.uint64(lg)) | home.astype(np.uint64)
    return hi, lo, validm, idx, d, home, p


def audit_tab(m, A, meta):
    out, tab, lg = [], A["tab"], meta["tab_lg"]
    nb = 1 << lg
    if lg == 0 or len(tab) != 2 * nb + 2:
        return ["tab[0]: %d slots for tab_lg %d" % (len(tab), lg)]
    hi, lo, validm, idx, d, home, p = _tab_decode(tab, lg)
    body = tab[:2 * nb]
    _report(out, "tab", ~validm & (body != 0), lambda i: "%#x in a slot without the valid bit" % int(body[i]))
    _report(out, "tab", d >= 64, lambda i: "displacement %d" % d[i], idx)
    # the keys are the filter's set bits, each once
    order = np.argsort(p, kind="stable")
    ps = p[order]
    dup = np.flatnonzero(ps[1:] == ps[:-1]) + 1
    _report(out, "tab", dup, lambda i: "position %d is a key more than once" % int(ps[i]), idx[order])
    r = np.searchsorted(m.setbits, p)
    known = (r < m.n_set) & (m.setbits[np.minimum(r, max(m.n_set - 1, 0))] == p) if m.n_set else np.zeros(len(p), bool)
    _report(out, "tab", ~known, lambda i: "key %d is not a set bit of the filter" % int(p[i]), idx)
    have = np.zeros(m.n_set, dtype=bool)
    have[r[known]] = True
    _report(out, "tab", ~have, lambda i: "set bit %d (rank %d, home bucket %d) is not a key" % (int(m.setbits[i]), i, int(m.setbits[i]) & (nb - 1)),
            (m.setbits & np.uint64(nb - 1)).astype(np.int64) * 2)
    # a displaced key passed only full buckets
    full = validm[0::2] & validm[1::2]
    c = np.concatenate([[0], np.cumsum(np.tile(full, 2))])
    dd = np.minimum(d, nb)
    _report(out, "tab", (d > 0) & (c[home + dd] - c[home] != dd), lambda i: "displaced by %d past a bucket with a free slot (home %d)" % (d[i], home[i]), idx)
    # the overflow mark: slot 0 of exactly the buckets that are the home of a displaced key
    want = np.zeros(nb, dtype=bool)
    want[home[(d > 0) & (d < 64)]] = True
    got = (lo[0::2] & TAB_OVERFLOW) != 0
    _report(out, "tab", want & ~got, "overflow mark missing (a key of this home bucket sits further down)", np.arange(nb) * 2)
    _report(out, "tab", got & ~want, "overflow mark without a displaced key of this home bucket", np.arange(nb) * 2)
    _report(out, "tab", (lo[1::2] & TAB_OVERFLOW) != 0, "overflow mark in slot 1", np.arange(nb) * 2 + 1)
    # the low word: the gene of a single-gene list, else multi | rank
    rk = r[known]
    exp = expected_low(m, rk)
    low = lo[idx[known]] & ~TAB_OVERFLOW
    _report(out, "tab", low != exp, lambda i: "low word %#x, expected %#x (rank %d)" % (low[i], exp[i], rk[i]), idx[known])
    for i in (2 * nb, 2 * nb + 1):
        if int(tab[i]) != 0:
            out.append("tab[%d]: spare bucket holds %#x" % (i, int(tab[i])))
    return out


def audit_atab(m, A, meta):
    out, tab, atab, lg = [], A["tab"], A["atab"], meta["tab_lg"]
    nb = 1 << lg
    if len(atab) != len(tab) or len(tab) != 2 * nb + 2:
        return ["atab[0]: %d slots, tab has %d" % (len(atab), len(tab))]
    _report(out, "atab", (atab >> np.uint64(32)) != (tab >> np.uint64(32)),
            lambda i: "high word %#x, tab's is %#x" % (int(atab[i]) >> 32, int(tab[i]) >> 32))
    hi, lo, validm, idx, d, home, p = _tab_decode(tab, lg)
    alo = (atab & np.uint64(0xFFFFFFFF)).astype(np.int64)
    unset = np.ones(len(atab), dtype=bool)
    unset[idx] = False
    _report(out, "atab", unset & (alo != NONE32), lambda i: "occurrence %#x in a slot that holds no key (spare bucket included)" % alo[i])
    # smallest x | strand << 31 over the occurrences of each key
    occ = np.full(m.n_set, NONE32, dtype=np.int64)
    np.minimum.at(occ, m.rank[m.vx], m.vx | (m.strand[m.vx].astype(np.int64) << 31))
    r = np.searchsorted(m.setbits, p)
    known = (r < m.n_set) & (m.setbits[np.minimum(r, max(m.n_set - 1, 0))] == p) if m.n_set else np.zeros(len(p), bool)
    got, exp = alo[idx[known]], occ[r[known]]
    _report(out, "atab", got == NONE32, "unset in a valid slot", idx[known])
    _report(out, "atab", (got != exp) & (got != NONE32),
            lambda i: "occurrence x=%d strand=%d, expected x=%d strand=%d" % (got[i] & 0x7FFFFFFF, got[i] >> 31, exp[i] & 0x7FFFFFFF, exp[i] >> 31), idx[known])
    return out


def audit_ref2(m, A, meta):
    out, a = [], A["ref2"]
    n_dw = (m.total + 15) // 16
    if meta["ref_total"] != m.total or len(a) != n_dw + 4:
        return ["ref2[0]: %d dwords for ref_total %d, the reference has %d bases" % (len(a), meta["ref_total"], m.total)]
    codes = np.zeros((n_dw + 4) * 16, dtype=np.uint32)
    codes[:m.total] = np.maximum(m.code, 0)
    exp = np.zeros(n_dw + 4, dtype=np.uint32)
    c = codes.reshape(-1, 16)
    for j in range(16):
        exp |= c[:, j] << np.uint32(2 * j)
    _report(out, "ref2", a != exp, lambda i: "%#010x, expected %#010x" % (a[i], exp[i]))
    return out


def audit_refpay(m, A, meta):
    """refpay, and what its multi-gene payloads point at: ent[n_set + 1 ..) and ids[tot_idx ..) when the per-position copies were built"""
    out, a = [], A["refpay"].astype(np.int64)
    total, n_set, tot = m.total, m.n_set, m.tot_idx
    if meta["ref_total"] != total or len(a) != total + 8:
        return ["refpay[0]: %d words for ref_total %d, the reference has %d bases" % (len(a), meta["ref_total"], total)]
    body = a[:total]
    _report(out, "refpay", ~m.valid & (body != NONE32), lambda i: "%#x where no valid k-mer starts" % body[i])
    _report(out, "refpay", a[total:] != NONE32, lambda i: "padding holds %#x" % a[total + i], np.arange(total, total + 8))
    _report(out, "refpay", m.valid & (body == NONE32), "REFPAY_NONE where a valid k-mer starts")
    sx = np.flatnonzero(m.single)
    _report(out, "refpay", body[sx] != m.gene0[m.rank[sx]], lambda i: "%#x, expected the gene %d of a single-gene list" % (body[sx[i]], m.gene0[m.rank[sx[i]]]), sx)
    mx = np.flatnonzero(m.valid & ~m.single)
    start, ln, g0 = _ent_fields(A["ent"])
    ids = A["ids"]
    perpos = meta["ent_len"] > n_set + 1
    if not perpos:
        exp = (1 << 31) | m.rank[mx]
        _report(out, "refpay", body[mx] != exp, lambda i: "%#x, expected multi | rank %d" % (body[mx[i]], m.rank[mx[i]]), mx)
        return out
    if meta["ent_len"] != n_set + 1 + total + 1 or len(start) != meta["ent_len"]:
        return out + ["ent[%d]: %d entries for a per-position layout of %d positions" % (n_set + 1, len(start), total)]
    exp = (1 << 31) | (n_set + 1 + mx)
    _report(out, "refpay", body[mx] != exp, lambda i: "%#x, expected multi | per-position entry %d" % (body[mx[i]], n_set + 1 + mx[i]), mx)
    # the copies tile ids[tot_idx, tot_idx + R) in x order
    lens = np.where(m.valid & ~m.single, m.plen, 0)
    offs = tot + np.concatenate([[0], np.cumsum(lens)])
    R = int(offs[-1]) - tot
    pe = slice(n_set + 1, n_set + 1 + total + 1)
    _report(out, "ent", start[pe] != offs, lambda i: "per-position start %d, expected %d" % (start[n_set + 1 + i], offs[i]), np.arange(n_set + 1, n_set + 2 + total))
    elen = np.concatenate([np.minimum(lens, 0xFFFF), [0]])
    _report(out, "ent", ln[pe] != elen, lambda i: "per-position len %d, expected %d" % (ln[n_set + 1 + i], elen[i]), np.arange(n_set + 1, n_set + 2 + total))
    eg0 = np.zeros(total + 1, dtype=np.int64)
    eg0[mx] = m.gene0[m.rank[mx]]
    _report(out, "ent", g0[pe] != eg0, lambda i: "per-position gene0 %d, expected %d" % (g0[n_set + 1 + i], eg0[i]), np.arange(n_set + 1, n_set + 2 + total))
    if len(ids) != meta["ids_len"] or len(ids) < tot + R:
        return out + ["ids[%d]: %d ids, the per-position copies need %d" % (tot, len(ids), tot + R)]
    if R:
        # expected copy: for every multi position, in x order, the oracle's list
        src = np.repeat(m.off[m.rank[mx]], lens[mx]) + (np.arange(R) - np.repeat(offs[mx] - tot, lens[mx]))
        expc = m.ids[src]
        _report(out, "ids", ids[tot:tot + R] != expc, lambda i: "copy holds %d, expected %d" % (ids[tot + i], expc[i]), np.arange(tot, tot + R))
    return out


def _runs(valid):
    """per position: valid positions directly in front of / behind it (unclipped; 0 where invalid)"""
    n = len(valid)
    x = np.arange(n)
    last_bad = np.maximum.accumulate(np.where(~valid, x, -1))
    left = np.where(valid, x - last_bad - 1, 0)
    nb = np.where(~valid, x, n)
    next_bad = np.minimum.accumulate(nb[::-1])[::-1]
    right = np.where(valid, next_bad - x - 1, 0)
    return left, right


def audit_refext(m, A, meta):
    out, a = [], A["refext"].astype(np.int64)
    total = m.total
    if len(a) != total + 8:
        return ["refext[0]: %d words, the reference has %d bases" % (len(a), total)]
    _report(out, "refext", a[total:] != NONE32, lambda i: "padding holds %#x" % a[total + i], np.arange(total, total + 8))
    left, right = _runs(m.valid)
    left, right = np.minimum(left, REFEXT_CLIP), np.minimum(right, REFEXT_CLIP)
    cs = np.concatenate([[0], np.cumsum(m.single)])
    x = np.arange(total)
    reach = (cs[x + right + 1] - cs[x - left]) > 0 if total else np.zeros(0, bool)
    g = m.gene_of_rec[m.rec_of] if total else np.zeros(0, np.int64)
    exp = np.where(m.valid & reach, g | (left << 16) | (right << 24), NONE32)
    body = a[:total]
    _report(out, "refext", (body != exp) & (exp == NONE32), lambda i: "%#x, expected REFEXT_NONE (no k-mer starts here, or no single-gene list within reach)" % body[i])
    _report(out, "refext", (body != exp) & (exp != NONE32),
            lambda i: "gene %d left %d right %d (%#x), expected gene %d left %d right %d" % (body[i] & 0xFFFF, (body[i] >> 16) & 0xFF, body[i] >> 24, body[i], g[i], left[i], right[i]))
    return out


def audit_refmul(m, A, meta):
    out, a = [], A["refmul"]
    n_w = (m.total + 31) // 32 + 2
    if len(a) != n_w:
        return ["refmul[0]: %d words, expected %d" % (len(a), n_w)]
    bits = np.ones(n_w * 32, dtype=np.uint8)
    bits[:m.total] = ~m.single
    exp = np.packbits(bits, bitorder="little").view(np.uint32)
    _report(out, "refmul", a != exp, lambda i: "%#010x, expected %#010x (bits %d..%d of %d positions)" % (a[i], exp[i], 32 * i, 32 * i + 31, m.total))
    return out


def ltab_lookup(img, mul, pos, bf_mask):
    """lds_table.hpp's two-read lookup rule, for arrays of positions: (found, payload)"""
    T = img[:1 << LTAB_SLOT_LG].astype(np.int64)
    D = img[1 << LTAB_SLOT_LG:].view(np.uint16).astype(np.int64)
    pos = np.asarray(pos, dtype=np.uint64)
    tagmask = bf_mask >> LTAB_SLOT_LG
    gmask = tagmask & ((1 << LTAB_GROUP_LG) - 1)
    lo = (pos & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tag = (pos >> np.uint64(LTAB_SLOT_LG)).astype(np.int64) & tagmask
    d = D[(lo >> LTAB_SLOT_LG) & gmask]
    e = T[(lo + (tag >> LTAB_GROUP_LG) * mul + d) & ((1 << LTAB_SLOT_LG) - 1)]
    return (e >> 13) == ((tag << 1) | 1), e & LTAB_ESC


def audit_ltab(m, A, meta, n_random=100000, seed=1):
    out, img = [], A["ltab"]
    if len(img) != (1 << LTAB_SLOT_LG) + (1 << LTAB_GROUP_LG) // 2:
        return ["ltab[0]: image of %d words" % len(img)]
    mask = m.bf_bits - 1
    found, pay = ltab_lookup(img, meta["ltab_mul"], m.setbits, mask)
    exp = np.where((m.list_len == 1) & (m.gene0 < LTAB_ESC), m.gene0, LTAB_ESC)
    _report(out, "ltab", ~found, lambda i: "set bit %d (rank %d) is not found" % (int(m.setbits[i]), i))
    _report(out, "ltab", found & (pay != exp), lambda i: "set bit %d answers %#x, expected %#x" % (int(m.setbits[i]), pay[i], exp[i]))
    rnd = np.random.default_rng(seed).integers(0, m.bf_bits, size=n_random, dtype=np.uint64)
    r = np.searchsorted(m.setbits, rnd)
    iskey = (r < m.n_set) & (m.setbits[np.minimum(r, m.n_set - 1)] == rnd)
    f, _ = ltab_lookup(img, meta["ltab_mul"], rnd, mask)
    _report(out, "ltab", f & ~iskey, lambda i: "position %d is not a set bit and is found" % int(rnd[i]))
    return out


AUDITS = {"rank_w": audit_rank_w, "ent": audit_ent, "ids": audit_ids, "sum32": audit_sum32, "lsum32": audit_lsum32, "lbig32": audit_lbig32,
          "tab": audit_tab, "atab": audit_atab, "ltab": audit_ltab, "ref2": audit_ref2, "refpay": audit_refpay, "refext": audit_refext,
          "refmul": audit_refmul}


def audit_all(m, A, meta):
    """every array `A` holds (non-empty), audited: {name: [violations]}"""
    return {name: AUDITS[name](m, A, meta) for name in ARRAYS if name in A and len(A[name])}


def pull(h):
    """every derived array of a built SharkHip and the scalars: (arrays, meta); arrays the index does not carry are left out"""
    meta = h.debug_index_meta()
    A = {}
    for name in ARRAYS:
        a = h.debug_index_array(name)
        if len(a):
            A[name] = a
    return A, meta
