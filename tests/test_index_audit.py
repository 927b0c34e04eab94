"""The index auditor (tests/index_audit.py) audited: a straightforward serial Python builder makes every derived array of a tiny
index the way DESIGN.md 2 describes it, the auditor must pass that, and it must name the array of every single-entry corruption
in the table below.  No GPU: this is the evidence that tests/test_gpu_index_audit.py is not vacuous."""
import numpy as np
import pytest

from tests import index_audit as ia

K, BF_BITS, TAB_LG = 11, 1 << 24, 9
SHIFTS = {"sum_shift": 8, "lsum_shift": 6, "lbig_shift": 7}     # (lsum32 / lbig32 keep their device sizes of 2^18 / 2^20 bits)
M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def xxh64_u64(v):
    """XXH64 of the 8 little-endian bytes of v, seed 0"""
    h = (P5 + 8) & M64
    k1 = (_rotl((v * P2) & M64, 31) * P1) & M64
    h ^= k1
    h = (_rotl(h, 27) * P1 + P4) & M64
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    return h ^ (h >> 32)


def tiny_records():
    rng = np.random.default_rng(2024)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seq = lambda n: acgt[rng.integers(0, 4, n)].copy()
    g0 = seq(150)
    g1 = seq(130)
    g1[30:90] = g0[50:110]                       # two genes sharing a stretch
    g1[110] = ord("N")
    short = seq(K - 4)                           # shorter than k: takes a gene number all the same
    only_n = np.full(K + 3, ord("N"), np.uint8)  # at least k long without a k-mer: takes none
    g2 = seq(320)                                # a run of more than 254 valid positions
    g2[5:12] |= 0x20                             # lower case
    g3 = np.concatenate([g0[20:20 + K + 6], seq(40)])
    return [bytes(x) for x in (g0, g1, short, only_n, g2, np.zeros(0, np.uint8), g3)]


def serial_build(records, k, bf_bits, tab_lg, shifts, perpos=True):
    """every derived array, one base / one key at a time"""
    code = {c: i for i, c in enumerate(b"ACGT")}
    code.update({c | 0x20: i for c, i in list(code.items())})
    data = b"".join(records)
    total = len(data)
    km = [None] * total                          # per position: (filter position, strand)
    rec_gene, gene_at, g, x0 = [], [0] * total, 0, 0
    for rec in records:
        has = False
        for s in range(len(rec) - k + 1):
            w = rec[s:s + k]
            if all(c in code for c in w):
                fw = rc = 0
                for c in w:
                    fw = fw << 2 | code[c]
                for c in reversed(w):
                    rc = rc << 2 | (3 - code[c])
                km[x0 + s] = (xxh64_u64(min(fw, rc)) % bf_bits, 0 if fw < rc else 1)
                has = True
        rec_gene.append(g)
        for s in range(len(rec)):
            gene_at[x0 + s] = g
        if not (len(rec) >= k and not has):
            g += 1
        x0 += len(rec)
    keys = sorted({e[0] for e in km if e})
    rank = {p: r for r, p in enumerate(keys)}
    lists = [[] for _ in keys]
    for x in range(total):
        if km[x] and gene_at[x] not in lists[rank[km[x][0]]]:
            lists[rank[km[x][0]]].append(gene_at[x])
    lists = [sorted(l) for l in lists]
    n_set, n_words = len(keys), ((bf_bits + 511) // 512) * 8
    A = {}
    # rank directory
    cnt = np.zeros(n_words + 2, np.uint32)
    for p in keys:
        cnt[(p >> 6) + 1] += 1
    A["rank_w"] = np.concatenate([np.cumsum(cnt[:n_words + 1]), [0]]).astype(np.uint32)
    # lists
    ent, ids = [], []
    for l in lists:
        ent.append((len(ids), min(len(l), 0xFFFF), l[0]))
        ids += l
    tot = len(ids)
    ent.append((tot, 0, 0))
    # summaries
    for name, key, bits in (("sum32", "sum_shift", None), ("lsum32", "lsum_shift", 1 << 18), ("lbig32", "lbig_shift", 1 << 20)):
        sh = shifts[key]
        a = np.zeros(((bits or bf_bits >> sh) + 31) // 32 + 2, np.uint32)
        for p in keys:
            a[(p >> sh) >> 5] |= np.uint32(1 << ((p >> sh) & 31))
        A[name] = a
    # position table: a key goes to the first bucket with a free slot on its path and marks its home when displaced
    nb = 1 << tab_lg
    tab = [0] * (2 * nb + 2)
    slot_of = {}
    for p in keys:
        l = lists[rank[p]]
        low = l[0] if len(l) == 1 else (1 << 31) | rank[p]
        home = p & (nb - 1)
        for d in range(64):
            b = (home + d) & (nb - 1)
            free = [s for s in (0, 1) if tab[2 * b + s] == 0]
            if free:
                tab[2 * b + free[0]] = (p >> tab_lg) << 40 | 1 << 39 | d << 32 | low
                slot_of[p] = 2 * b + free[0]
                if d:
                    tab[2 * home] |= ia.TAB_OVERFLOW
                break
        else:
            raise AssertionError("no place")
    A["tab"] = np.array(tab, np.uint64)
    # occurrences, payloads, the packed reference
    occ = [ia.NONE32] * (2 * nb + 2)
    refpay = [ia.NONE32] * (total + 8)
    for x in range(total):
        if km[x]:
            i = slot_of[km[x][0]]
            occ[i] = min(occ[i], x | km[x][1] << 31)
            refpay[x] = tab[i] & 0xFFFFFFFF & ~ia.TAB_OVERFLOW
    A["atab"] = np.array([(t >> 32) << 32 | o for t, o in zip(tab, occ)], np.uint64)
    ref2 = [0] * ((total + 15) // 16 + 4)
    for x, c in enumerate(data):
        ref2[x >> 4] |= code.get(c, 0) << (2 * (x & 15))
    A["ref2"] = np.array(ref2, np.uint32)
    if perpos:
        for x in range(total + 1):
            l = lists[refpay[x] & ia.TAB_PAYLOAD] if x < total and refpay[x] != ia.NONE32 and refpay[x] >> 31 else []
            ent.append((len(ids), len(l), l[0] if l else 0))
            if l:
                ids += l
                refpay[x] = 1 << 31 | (n_set + 1 + x)
    A["refpay"] = np.array(refpay, np.uint32)
    A["ent"] = np.array([w for s, n, g0 in ent for w in (s, n | g0 << 16)], np.uint32)
    A["ids"] = np.array(ids + [0] * 8, np.uint16)
    # surroundings
    single = lambda u: u != ia.NONE32 and u <= 0xFFFF
    refext = [ia.NONE32] * (total + 8)
    for x in range(total):
        if refpay[x] == ia.NONE32:
            continue
        left = right = 0
        while left < ia.REFEXT_CLIP and x - 1 - left >= 0 and refpay[x - 1 - left] != ia.NONE32:
            left += 1
        while right < ia.REFEXT_CLIP and x + 1 + right < total and refpay[x + 1 + right] != ia.NONE32:
            right += 1
        near = [refpay[y] for y in range(x - left, x + right + 1) if single(refpay[y])]
        if near:
            refext[x] = gene_at[x] | left << 16 | right << 24
            assert set(near) == {gene_at[x]}
    A["refext"] = np.array(refext, np.uint32)
    refmul = [0xFFFFFFFF] * ((total + 31) // 32 + 2)
    for x in range(total):
        if single(refpay[x]):
            refmul[x >> 5] &= ~(1 << (x & 31))
    A["refmul"] = np.array(refmul, np.uint32)
    # LDS table: a displacement per group, largest group first (lds_table.hpp)
    mul, NS, NG = 1021, 1 << 15, 1 << 13
    groups = {}
    for p in keys:
        l = lists[rank[p]]
        tag = p >> 15
        groups.setdefault(tag & (NG - 1), []).append(((p + (tag >> 13) * mul) & (NS - 1), tag, l[0] if len(l) == 1 and l[0] < 0x1FFF else 0x1FFF))
    T, D = [0] * NS, [0] * NG
    for gid in sorted(groups, key=lambda q: -len(groups[q])):
        ks = groups[gid]
        assert len({b for b, _, _ in ks}) == len(ks)
        d = next(d for d in range(NS) if all(T[(b + d) & (NS - 1)] == 0 for b, _, _ in ks))
        for b, tag, pay in ks:
            T[(b + d) & (NS - 1)] = tag << 14 | 1 << 13 | pay
        D[gid] = d
    A["ltab"] = np.concatenate([np.array(T, np.uint32), np.array(D, np.uint16).view(np.uint32)])
    meta = dict(shifts, tab_lg=tab_lg, ltab_mul=mul, ref_total=total, n_set=n_set, tot_idx=tot, pow2=1, wrap=0, ent_len=len(ent),
                ids_len=len(ids) + 8, bf_bits=bf_bits, bf_words64=n_words, sum_bits=bf_bits >> shifts["sum_shift"], ktab_lg=0)
    return A, meta


@pytest.fixture(scope="module")
def tiny(oracle):
    recs = tiny_records()
    o = oracle.Shark(k=K, bf_bits=BF_BITS)
    o.build(recs)
    m = ia.Model(oracle, o, recs, K, BF_BITS)
    A, meta = serial_build(recs, K, BF_BITS, TAB_LG, SHIFTS)
    return m, A, meta


def test_model_of_the_tiny_index(tiny):
    m, A, meta = tiny
    assert m.nidx == 6 and list(m.gene_of_rec) == [0, 1, 2, 3, 3, 4, 5]     # the all-N record takes no number, the empty one does
    assert (m.plen > 1).sum() >= 40 and m.single.sum() > 400
    left, _ = ia._runs(m.valid)
    assert left.max() > 256
    assert not m.valid[m.rec_off[2]:m.rec_off[4]].any()


def test_auditor_passes_the_serial_builder(tiny):
    m, A, meta = tiny
    res = ia.audit_all(m, A, meta)
    assert set(res) == set(ia.ARRAYS)
    assert {n: v for n, v in res.items() if v} == {}


def test_auditor_passes_the_fallback_layout(oracle, tiny):
    m = tiny[0]
    A, meta = serial_build(tiny_records(), K, BF_BITS, TAB_LG, SHIFTS, perpos=False)
    assert meta["ent_len"] == m.n_set + 1
    assert {n: v for n, v in ia.audit_all(m, A, meta).items() if v} == {}


# ---- single-entry corruptions: name -> (array the auditor must name, function(m, A, meta) that corrupts A in place) ----------
def _slots(A, meta):
    hi, lo, validm, idx, d, home, p = ia._tab_decode(A["tab"], meta["tab_lg"])
    return hi, lo, validm, idx, d, home, p


def _first(cond):
    i = np.flatnonzero(cond)
    assert len(i), "the tiny index has no entry for this corruption"
    return int(i[0])


def c_tab_tag_bit(m, A, meta):
    A["tab"][_first(_slots(A, meta)[2])] ^= np.uint64(1 << 43)


def c_tab_overflow_cleared(m, A, meta):
    lo = _slots(A, meta)[1]
    A["tab"][2 * _first(lo[0::2] & ia.TAB_OVERFLOW)] &= np.uint64(~ia.TAB_OVERFLOW & M64)


def c_tab_overflow_spurious(m, A, meta):
    hi, lo, validm = _slots(A, meta)[:3]
    A["tab"][2 * _first(validm[0::2] & ((lo[0::2] & ia.TAB_OVERFLOW) == 0))] |= np.uint64(ia.TAB_OVERFLOW)


def c_tab_overflow_slot1(m, A, meta):
    A["tab"][2 * _first(_slots(A, meta)[2][1::2]) + 1] |= np.uint64(ia.TAB_OVERFLOW)


def c_tab_displaced_past_free_slot(m, A, meta):
    hi, lo, validm, idx, d, home, p = _slots(A, meta)
    nb = 1 << meta["tab_lg"]
    # an undisplaced key in slot 1 whose next bucket has slot 1 free: moved there, marked at home -- only its path is wrong
    b = _first(validm[1::2][:nb - 1] & ((hi[1::2][:nb - 1] & 0x7F) == 0) & validm[0::2][1:] & ~validm[1::2][1:])
    A["tab"][2 * b + 3] = A["tab"][2 * b + 1] | np.uint64(1 << 32)
    A["tab"][2 * b + 1] = 0
    A["tab"][2 * b] |= np.uint64(ia.TAB_OVERFLOW)


def c_tab_duplicate_key(m, A, meta):
    validm = _slots(A, meta)[2]
    b = _first(validm[0::2] & ~validm[1::2])
    A["tab"][2 * b + 1] = A["tab"][2 * b] & np.uint64(~ia.TAB_OVERFLOW & M64)


def c_tab_lost_key(m, A, meta):
    hi, lo, validm = _slots(A, meta)[:3]
    A["tab"][2 * _first(validm[0::2] & ~validm[1::2] & ((lo[0::2] & ia.TAB_OVERFLOW) == 0))] = 0


def c_tab_swapped_gene(m, A, meta):
    hi, lo, validm = _slots(A, meta)[:3]
    A["tab"][_first(validm & (lo >> 31 == 0))] ^= np.uint64(1)


def c_tab_rank_off_by_one(m, A, meta):
    hi, lo, validm = _slots(A, meta)[:3]
    A["tab"][_first(validm & (lo >> 31 == 1))] += np.uint64(1)


def c_tab_displacement_bit(m, A, meta):
    A["tab"][_first(_slots(A, meta)[2])] |= np.uint64(1 << 38)


def c_tab_spare(m, A, meta):
    A["tab"][-1] = np.uint64(1 << 39)


def c_tab_stray_bits(m, A, meta):
    A["tab"][_first(~_slots(A, meta)[2])] = np.uint64(5)


def c_rank_off_by_one(m, A, meta):
    A["rank_w"][int(m.nz_words[3]) + 1] += 1


def c_rank_last(m, A, meta):
    A["rank_w"][meta["bf_words64"]] -= 1


def c_ent_start(m, A, meta):
    A["ent"][2 * 7] += 1


def c_ent_len(m, A, meta):
    A["ent"][2 * 7 + 1] += 1


def c_ent_gene0(m, A, meta):
    A["ent"][2 * 7 + 1] ^= 1 << 16


def c_ent_sentinel(m, A, meta):
    A["ent"][2 * m.n_set + 1] = 1


def c_ids_swapped_gene(m, A, meta):
    A["ids"][m.tot_idx - 1] ^= 1


def _c_sum_clear(name):
    def f(m, A, meta):
        w = _first(A[name])
        A[name][w] &= A[name][w] - np.uint32(1)
    return f


def _c_sum_set(name):
    def f(m, A, meta):
        A[name][_first(A[name] == 0)] |= np.uint32(1 << 9)
    return f


def _c_sum_pad(name):
    def f(m, A, meta):
        A[name][-1] = 1
    return f


def _key_slot(m, A, meta, rank):
    hi, lo, validm, idx, d, home, p = _slots(A, meta)
    return int(idx[_first(p == m.setbits[rank])])


def c_atab_not_smallest(m, A, meta):
    r, n = np.unique(m.rank[m.vx], return_counts=True)
    rk = int(r[_first(n > 1)])
    xs = m.vx[m.rank[m.vx] == rk]
    later = int(xs[1]) | int(m.strand[xs[1]]) << 31           # a true occurrence of the key, only not the smallest
    i = _key_slot(m, A, meta, rk)
    assert later != int(A["atab"][i]) & 0xFFFFFFFF
    A["atab"][i] = (A["atab"][i] >> np.uint64(32) << np.uint64(32)) | np.uint64(later)


def c_atab_wrong_strand(m, A, meta):
    A["atab"][_first(_slots(A, meta)[2])] ^= np.uint64(1 << 31)


def c_atab_high_word(m, A, meta):
    A["atab"][_first(_slots(A, meta)[2])] ^= np.uint64(1 << 41)


def c_atab_unset(m, A, meta):
    A["atab"][_first(_slots(A, meta)[2])] |= np.uint64(0xFFFFFFFF)


def c_atab_spare(m, A, meta):
    A["atab"][-2] = np.uint64(17)


def c_ref2_code(m, A, meta):
    A["ref2"][9] ^= np.uint32(1 << 12)


def c_ref2_tail(m, A, meta):
    assert m.total % 16
    A["ref2"][m.total // 16] |= np.uint32(1 << 30)


def c_ref2_pad(m, A, meta):
    A["ref2"][-1] = 1


def c_refpay_neighbour(m, A, meta):
    mx = np.flatnonzero(m.valid & ~m.single)
    x = int(mx[_first(np.diff(mx) == 1)])
    A["refpay"][x] += 1                                       # the next position's entry: a list of the same genes, but not this position's


def c_refpay_single_gene(m, A, meta):
    A["refpay"][_first(m.single)] ^= 1


def c_refpay_none_missing(m, A, meta):
    A["refpay"][_first(~m.valid)] = 0


def c_refpay_none_spurious(m, A, meta):
    A["refpay"][_first(m.valid)] = ia.NONE32


def c_refpay_pad(m, A, meta):
    A["refpay"][m.total + 7] = 0


def c_perpos_start(m, A, meta):
    A["ent"][2 * (m.n_set + 1 + m.total // 2)] += 1


def c_perpos_close(m, A, meta):
    A["ent"][2 * (m.n_set + 1 + m.total)] -= 1


def c_perpos_len(m, A, meta):
    A["ent"][2 * (m.n_set + 1 + _first(m.valid & ~m.single)) + 1] += 1


def c_perpos_gene0(m, A, meta):
    A["ent"][2 * (m.n_set + 1 + _first(m.valid & ~m.single)) + 1] ^= 1 << 16


def c_perpos_copy(m, A, meta):
    A["ids"][m.tot_idx + 1] ^= 1


def c_refext_left_at_record_start(m, A, meta):
    x = int(m.rec_off[4])
    assert m.valid[x] and (int(A["refext"][x]) >> 16) & 0xFF == 0
    A["refext"][x] += 1 << 16


def c_refext_clip_255(m, A, meta):
    left, _ = ia._runs(m.valid)
    x = _first(left >= 255)
    assert (int(A["refext"][x]) >> 16) & 0xFF == 254
    A["refext"][x] += 1 << 16


def c_refext_right(m, A, meta):
    A["refext"][_first(m.valid)] -= 1 << 24


def c_refext_gene(m, A, meta):
    A["refext"][_first(m.valid)] ^= 1


def c_refext_none_cleared(m, A, meta):
    A["refext"][_first(~m.valid)] = 0


def c_refext_pad(m, A, meta):
    A["refext"][m.total] = 0


def c_refmul_tail_bit(m, A, meta):
    A["refmul"][-1] &= np.uint32(0x7FFFFFFF)


def c_refmul_first_bit_behind(m, A, meta):
    assert m.total % 32
    A["refmul"][m.total // 32] &= np.uint32(~(1 << (m.total % 32)) & 0xFFFFFFFF)


def c_refmul_body_bit(m, A, meta):
    x = _first(m.single)
    A["refmul"][x >> 5] |= np.uint32(1 << (x & 31))


def c_refmul_multi_cleared(m, A, meta):
    x = _first(m.valid & ~m.single)
    A["refmul"][x >> 5] &= np.uint32(~(1 << (x & 31)) & 0xFFFFFFFF)


def c_ltab_payload(m, A, meta):
    A["ltab"][_first(A["ltab"][:1 << 15])] ^= np.uint32(1)


def c_ltab_lost_key(m, A, meta):
    A["ltab"][_first(A["ltab"][:1 << 15])] = 0


def c_ltab_false_match(m, A, meta):
    # an entry that answers for a position that is no key: the first random position the auditor tries, placed by the lookup's rule
    rnd = int(np.random.default_rng(1).integers(0, m.bf_bits, size=100000, dtype=np.uint64)[0])
    assert rnd not in set(int(p) for p in m.setbits)
    tag = rnd >> 15
    D = A["ltab"][1 << 15:].view(np.uint16)
    slot = (rnd + (tag >> 13) * meta["ltab_mul"] + int(D[tag & 8191])) & 32767
    assert A["ltab"][slot] == 0
    A["ltab"][slot] = tag << 14 | 1 << 13 | 3


CORRUPTIONS = {
    "tab: one tag bit": ("tab", c_tab_tag_bit),
    "tab: overflow mark cleared": ("tab", c_tab_overflow_cleared),
    "tab: spurious overflow mark": ("tab", c_tab_overflow_spurious),
    "tab: overflow mark in slot 1": ("tab", c_tab_overflow_slot1),
    "tab: displaced key leaves a free slot on its path": ("tab", c_tab_displaced_past_free_slot),
    "tab: duplicated key": ("tab", c_tab_duplicate_key),
    "tab: lost key": ("tab", c_tab_lost_key),
    "tab: swapped gene": ("tab", c_tab_swapped_gene),
    "tab: rank off by one": ("tab", c_tab_rank_off_by_one),
    "tab: displacement of 64": ("tab", c_tab_displacement_bit),
    "tab: spare bucket": ("tab", c_tab_spare),
    "tab: bits in an empty slot": ("tab", c_tab_stray_bits),
    "rank_w: off by one": ("rank_w", c_rank_off_by_one),
    "rank_w: last entry": ("rank_w", c_rank_last),
    "ent: start": ("ent", c_ent_start),
    "ent: len": ("ent", c_ent_len),
    "ent: gene0": ("ent", c_ent_gene0),
    "ent: sentinel": ("ent", c_ent_sentinel),
    "ids: swapped gene": ("ids", c_ids_swapped_gene),
    "sum32: bit cleared": ("sum32", _c_sum_clear("sum32")),
    "sum32: bit set": ("sum32", _c_sum_set("sum32")),
    "sum32: padding": ("sum32", _c_sum_pad("sum32")),
    "lsum32: bit cleared": ("lsum32", _c_sum_clear("lsum32")),
    "lsum32: bit set": ("lsum32", _c_sum_set("lsum32")),
    "lbig32: bit cleared": ("lbig32", _c_sum_clear("lbig32")),
    "lbig32: bit set": ("lbig32", _c_sum_set("lbig32")),
    "atab: a valid occurrence that is not the smallest": ("atab", c_atab_not_smallest),
    "atab: wrong strand": ("atab", c_atab_wrong_strand),
    "atab: high word": ("atab", c_atab_high_word),
    "atab: unset in a valid slot": ("atab", c_atab_unset),
    "atab: spare bucket": ("atab", c_atab_spare),
    "ref2: one code": ("ref2", c_ref2_code),
    "ref2: tail of the last dword": ("ref2", c_ref2_tail),
    "ref2: padding": ("ref2", c_ref2_pad),
    "refpay: a neighbour's list": ("refpay", c_refpay_neighbour),
    "refpay: gene of a single-gene list": ("refpay", c_refpay_single_gene),
    "refpay: none missing": ("refpay", c_refpay_none_missing),
    "refpay: none where a k-mer starts": ("refpay", c_refpay_none_spurious),
    "refpay: padding": ("refpay", c_refpay_pad),
    "ent: per-position start": ("ent", c_perpos_start),
    "ent: per-position closing entry": ("ent", c_perpos_close),
    "ent: per-position len": ("ent", c_perpos_len),
    "ent: per-position gene0": ("ent", c_perpos_gene0),
    "ids: per-position copy": ("ids", c_perpos_copy),
    "refext: left + 1 at a record start": ("refext", c_refext_left_at_record_start),
    "refext: extent clipped at 255": ("refext", c_refext_clip_255),
    "refext: right - 1": ("refext", c_refext_right),
    "refext: gene": ("refext", c_refext_gene),
    "refext: none cleared": ("refext", c_refext_none_cleared),
    "refext: padding": ("refext", c_refext_pad),
    "refmul: tail bit cleared": ("refmul", c_refmul_tail_bit),
    "refmul: first bit behind the reference cleared": ("refmul", c_refmul_first_bit_behind),
    "refmul: bit of a single-gene list set": ("refmul", c_refmul_body_bit),
    "refmul: bit of a multi-gene list cleared": ("refmul", c_refmul_multi_cleared),
    "ltab: payload": ("ltab", c_ltab_payload),
    "ltab: lost key": ("ltab", c_ltab_lost_key),
    "ltab: a non-key matches": ("ltab", c_ltab_false_match),
}


def test_corruption_table_covers_every_array():
    assert len(CORRUPTIONS) >= 15
    assert {a for a, _ in CORRUPTIONS.values()} == set(ia.ARRAYS)


@pytest.mark.parametrize("what", sorted(CORRUPTIONS))
def test_auditor_names_the_corrupted_array(tiny, what):
    m, A0, meta = tiny
    name, corrupt = CORRUPTIONS[what]
    A = {n: a.copy() for n, a in A0.items()}
    corrupt(m, A, meta)
    changed = [n for n in A if not np.array_equal(A[n], A0[n])]
    assert len(changed) == 1, changed
    res = ia.audit_all(m, A, meta)
    assert any(v.startswith(name + "[") for v in res[name] + [v for n in res for v in res[n] if v.startswith(name + "[")]), (what, res)
