"""Spliced ends (shk_splice_sites_set / shk_alignments_splice, `shark --splice-junctions`) on the GPU, against the model
(tests/splice_model.py), record by record, byte for byte.  The model writes every candidate's coordinates out in full; it is fed the
GPU's own gene_off / gene_ids, which are compared with the CPU oracle's first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth
from tests.extend_model import expected_aligned_pileup
from tests.segments_model import expected_segments
from tests.splice_cases import ONE_JUNCTION, cut, differs, junction_gene
from tests.splice_model import DEFAULTS, check_sites, expected_alignments_spliced
from tests.spliced_model import expected_junction_table, table_rows
from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_align import same_records
from tests.test_gpu_extend import state_is, sub
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import device_assoc
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu


def both(reads, m):
    reads += [np.array(m, dtype=np.uint8), synth.revcomp(np.array(m, dtype=np.uint8))]


def model_records(o, sm, batch, goff, gids, s_min, sites, params, P=0, B=0, q=0, stats=None):
    og, oi = o.classify(*_args(batch))
    assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
    rows = expected_segments(sm, batch, goff, gids, 4, q)[1]
    return expected_alignments_spliced(sm, batch, goff, gids, rows, s_min, sites, params, P, B, q, stats)


def set_step(h, sites, params):
    """the list and the parameters; an empty list drops the list, min_overhang 0 switches the step off"""
    h.splice_sites_set(np.array(sites, dtype=np.int64).reshape(-1, 3))
    if sites or params[0] == 0:
        h.alignments_splice(*params)


def classify_and_check(o, h, sm, batch, s_min, sites, params=DEFAULTS, P=0, B=0, q=0, stats=None):
    lengths = [len(sm.records[g]) for g in range(len(sm.records))]
    sites = check_sites(sites, lengths)
    set_step(h, sites, params)
    h.alignments_extend(P, B)
    goff, gids = h.classify(*_args(batch))
    want = model_records(o, sm, batch, goff, gids, s_min, sites if params[0] else [], params, P, B, q, stats)
    got = h.alignments_last()
    same_records(got, want)
    return goff, gids, got


def blocks_of(r):
    return [tuple(int(v) for v in r["block"][b]) for b in range(int(r["n_blocks"]))]


# ---------------------------------------------------------------------------
# 1. placement across one site
# ---------------------------------------------------------------------------
def test_placement_across_one_site(oracle):
    rng = np.random.default_rng(33)
    genes = [junction_gene(rng, 0), junction_gene(rng, 3)]
    o, h, sm = build_kb(oracle, genes, k=17)
    h.alignments_enable(8)
    reads = []
    for s in genes:
        for _, pieces, _, _ in ONE_JUNCTION:
            both(reads, cut(s, pieces))
    single = synth.batch_from_lists(reads)
    paired = synth.batch_from_lists(reads, reads[::-1])
    # without a list: the parent's records, one block each (tests/test_gpu_extend.py's case 4)
    _, gids, plain = classify_and_check(o, h, sm, single, 8, [], (0, 0, 0))
    assert gids.tolist() == [0] * 4 + [1] * 4 and all(int(r["n_blocks"]) == 1 for r in plain[:, 0])
    assert blocks_of(plain[0, 0]) == [(20, 0, 60)] and blocks_of(plain[2, 0]) == [(140, 10, 60)]
    st = {}
    _, _, got = classify_and_check(o, h, sm, single, 8, [(0, 80, 140), (1, 80, 140)], stats=st)
    for g in range(2):
        for n, (_, _, want, _) in enumerate(ONE_JUNCTION):
            for strand in range(2):
                r = got[4 * g + 2 * n + strand, 0]
                assert blocks_of(r) == want and int(r["strand"]) == strand and int(r["matches"]) == 70 and int(r["mismatches"]) == 0
    assert st["left_placed"] == st["right_placed"] == 4 and not got[:, 1].tobytes().strip(b"\0")
    classify_and_check(o, h, sm, paired, 8, [(0, 80, 140), (1, 80, 140)])
    # both descriptions of the microhomology's one placement listed: the tie goes to the largest donor
    _, _, got = classify_and_check(o, h, sm, single, 8, [(0, 80, 140), (1, 80, 140), (1, 83, 143)])
    for n, (_, _, _, want_tie) in enumerate(ONE_JUNCTION):
        assert blocks_of(got[4 + 2 * n, 0]) == want_tie and blocks_of(got[4 + 2 * n + 1, 0]) == want_tie
    # the list dropped again: the parent's records
    _, _, again = classify_and_check(o, h, sm, single, 8, [], DEFAULTS)
    assert again.tobytes() == plain.tobytes()


# ---------------------------------------------------------------------------
# 2. bounds
# ---------------------------------------------------------------------------
def test_bounds(oracle):
    """h = 1, min_overhang - 1, min_overhang, 48 and 49 at both ends on both strands; the donor at xe - B, xe - B - 1, xe + h - 1 and
    xe + h (by hand below); a far side that ends exactly at len_g and one base past it; the mirrors.  The floor is s_min = 40, so that
    an overhang of 48 bases (32 windows) stays silent beside a block of 60 (44 windows)"""
    rng = np.random.default_rng(34)
    S = 40
    s = junction_gene(rng, 0, 120, 60, 120)                      # exon [0, 120), intron [120, 180), exon [180, 300)
    # a second gene whose bases [100, 116) are repeated at [200, 216): a mate s2[40:100] + s2[200:221] votes on the first diagonal through
    # read base 76 (the repeat is one base short of a 17-mer), so xe = 116, h = 5, B = 16 and the donor 100 = xe - B costs nothing
    s2 = synth.random_seq(rng, 320)
    s2[200:216] = s2[100:116]
    s2[216] = differs(s2[116])
    s2[199] = differs(s2[99])
    # and its mirror: bases [120, 136) of s3 stand at [30, 46) as well: s3[25:30] + s3[120:196] has block 0 = {120, 5, 76}, h = 5, B = 16,
    # and the acceptor 136 = x0 + B (donor 46) costs nothing, while (47, 137) would cost one base if it were tried
    s3 = synth.random_seq(rng, 320)
    s3[30:46] = s3[120:136]
    s3[29] = differs(s3[119])
    s3[46] = differs(s3[136])
    # a gene that ends with its second exon: the far side of (80, 120) ends exactly at len_g for a mate that takes all of it
    s4 = np.concatenate([synth.random_seq(rng, 80), synth.random_seq(rng, 40), synth.random_seq(rng, 30)])
    o, h, sm = build_kb(oracle, [s, s2, s3, s4], k=17)
    h.alignments_enable(S)
    reads = []
    for hh in (1, 2, 3, 48, 49):
        both(reads, cut(s, ((60, 120), (180, 180 + hh))))
        both(reads, cut(s, ((120 - hh, 120), (180, 240))))
    both(reads, cut(s2, ((40, 100), (200, 221))))                # 20 .. 23
    both(reads, cut(s3, ((25, 30), (120, 196))))
    both(reads, cut(s, ((60, 120), (180, 195))))                 # 24, 25
    both(reads, cut(s, ((105, 120), (180, 240))))                # 26, 27
    both(reads, cut(s4, ((10, 80), (120, 150))))                 # 28, 29: the far side ends at len_g = 150
    both(reads, cut(s4, ((10, 80), (120, 132))))                 # 30, 31
    batch = synth.batch_from_lists(reads)
    junction = [(0, 120, 180)]
    for params in ((3, 2, 2), (1, 2, 1), (2, 0, 1), (48, 2, 2)):
        st = {}
        classify_and_check(o, h, sm, batch, S, junction + [(1, 100, 200), (2, 30, 120), (2, 46, 136), (3, 80, 120)], params, stats=st)
        assert st.get("left_placed", 0) >= 2 and st.get("right_placed", 0) >= 2, (params, st)
    # (3, 2, 2) by hand: h = 3 and 48 are placed, 1, 2 and 49 are not
    _, _, got = classify_and_check(o, h, sm, batch, S, junction, (3, 2, 2))
    for n, hh in enumerate((1, 2, 3, 48, 49)):
        for strand in range(2):
            r, left = got[4 * n + strand, 0], got[4 * n + 2 + strand, 0]
            if hh in (3, 48):
                assert blocks_of(r) == [(60, 0, 60), (180, 60, hh)] and blocks_of(left) == [(120 - hh, 0, hh), (180, hh, 60)], (hh, r, left)
            else:
                assert int(r["n_blocks"]) == 1 and int(left["n_blocks"]) == 1, (hh, r, left)
    # the donor's range: xe - B is a candidate (the block gives 16 bases back), one base further left is not; the acceptor's likewise
    _, _, plain = classify_and_check(o, h, sm, batch, S, [], (0, 0, 0))
    assert blocks_of(plain[20, 0]) == [(40, 0, 76)] and blocks_of(plain[22, 0]) == [(120, 5, 76)]
    _, _, got = classify_and_check(o, h, sm, batch, S, [(1, 100, 200), (2, 46, 136)], (3, 2, 2))
    assert blocks_of(got[20, 0]) == [(40, 0, 60), (200, 60, 21)] and blocks_of(got[21, 0]) == blocks_of(got[20, 0])
    assert blocks_of(got[22, 0]) == [(25, 0, 21), (136, 21, 60)] and blocks_of(got[23, 0]) == blocks_of(got[22, 0])
    _, _, got = classify_and_check(o, h, sm, batch, S, [(1, 99, 199), (2, 47, 137)], (3, 2, 2))
    assert all(int(got[j, 0]["n_blocks"]) == 1 for j in range(20, 24))
    # xe + h - 1: the overhang's last base alone crosses; xe + h: none does; the mirrors x0 - h + 1 and x0 - h
    # (one site at a time: two of one shift would be one placement)
    _, _, got = classify_and_check(o, h, sm, batch, S, [(0, 134, 194)], (3, 64, 0))
    assert blocks_of(got[24, 0]) == [(60, 0, 74), (194, 74, 1)] == blocks_of(got[25, 0])
    _, _, got = classify_and_check(o, h, sm, batch, S, [(0, 106, 166)], (3, 64, 0))
    assert blocks_of(got[26, 0]) == [(105, 0, 1), (166, 1, 74)] == blocks_of(got[27, 0])
    for site, j in (((0, 135, 195), 24), ((0, 105, 165), 26)):
        _, _, got = classify_and_check(o, h, sm, batch, S, [site], (3, 64, 0))
        assert int(got[j, 0]["n_blocks"]) == 1 and int(got[j + 1, 0]["n_blocks"]) == 1
    # the far side exactly at len_g, and past it
    _, _, got = classify_and_check(o, h, sm, batch, S, [(3, 80, 120)], (3, 2, 2))
    assert blocks_of(got[28, 0]) == [(10, 0, 70), (120, 70, 30)] and blocks_of(got[30, 0]) == [(10, 0, 70), (120, 70, 12)]
    _, _, got = classify_and_check(o, h, sm, batch, S, [(3, 80, 139)], (3, 64, 0))
    assert int(got[30, 0]["n_blocks"]) == 1                      # (139 + 12 = 151 > 150)


def test_a_block_of_at_most_16_bases(oracle):
    """k = 7, s_min = 3: blocks of 12 bases, so B = len - 1 = 11; both ends, both strands"""
    rng = np.random.default_rng(44)
    s = junction_gene(rng, 0)
    o, h, sm = build_kb(oracle, [s], k=7)
    h.alignments_enable(3)
    reads = []
    both(reads, cut(s, ((68, 80), (140, 146))))
    both(reads, cut(s, ((74, 80), (140, 152))))
    batch = synth.batch_from_lists(reads)
    _, _, plain = classify_and_check(o, h, sm, batch, 3, [], (0, 0, 0))
    assert blocks_of(plain[0, 0]) == [(68, 0, 12)] and blocks_of(plain[2, 0]) == [(140, 6, 12)]
    st = {}
    _, _, got = classify_and_check(o, h, sm, batch, 3, [(0, 80, 140)], stats=st)
    for strand in range(2):
        assert blocks_of(got[strand, 0]) == [(68, 0, 12), (140, 12, 6)] and blocks_of(got[2 + strand, 0]) == [(74, 0, 6), (140, 6, 12)]
    # a donor 11 bases inside the block is a candidate, one 12 bases inside is not (B = 11): max_cost 64 and min_gap 0 place whatever is one
    st = {}
    classify_and_check(o, h, sm, batch, 3, [(0, 69, 150)], (3, 64, 0), stats=st)
    assert st.get("right_no_candidate", 0) == 0 and st["right_attempted"] == 2
    st = {}
    classify_and_check(o, h, sm, batch, 3, [(0, 68, 150)], (3, 64, 0), stats=st)
    assert st["right_no_candidate"] == 2


def test_left_end_behind_a_closed_gap_at_a_small_k(oracle):
    """k = 7, s_min = 3: block 0 is a 12-base exon, two substituted bases follow and closure gives both to block 0 (every split costs
    2, the tie goes to the largest s), so step 3b sees block 0 = {80, 5, 14}: B = 13, and the evaluated bases include the two that
    closure added, which are not a match.  At max_cost 0 the end stays a clip; from max_cost 2 on it is placed.  (B from the 12-base
    span would evaluate 16 bases, find cost 0 and place the end at max_cost 0.)"""
    rng = np.random.default_rng(45)
    s = synth.random_seq(rng, 200)                               # exon A [0, 40), exon 1 [80, 92), exon 2 [140, 200)
    for t in range(4):
        s[79 - t] = differs(s[39 - t])                           # (the intron's end is not exon A's end)
    gap = [differs(s[92 + t], s[140 + t]) for t in range(2)]
    mate = np.concatenate([s[35:40], s[80:92], np.array(gap, np.uint8), s[142:180]])
    o, h, sm = build_kb(oracle, [s], k=7)
    h.alignments_enable(3)
    reads = []
    both(reads, mate)
    batch = synth.batch_from_lists(reads)
    _, _, plain = classify_and_check(o, h, sm, batch, 3, [], (0, 0, 0))
    assert blocks_of(plain[0, 0]) == [(80, 5, 14), (142, 19, 38)] == blocks_of(plain[1, 0])
    st = {}
    _, _, got = classify_and_check(o, h, sm, batch, 3, [(0, 40, 80)], (3, 0, 1), stats=st)
    assert got.tobytes() == plain.tobytes() and st == {"left_attempted": 2, "left_too_costly": 2}
    for P, B in ((0, 0), (4, 5)):
        _, _, got = classify_and_check(o, h, sm, batch, 3, [(0, 40, 80)], (3, 2, 2), P, B)
        assert blocks_of(got[0, 0]) == [(35, 0, 5), (80, 5, 14), (142, 19, 38)] == blocks_of(got[1, 0])
    # an acceptor at x0 + 13 is in range only with B from the closed block: (53, 93) is a candidate, (54, 94) is not
    st = {}
    classify_and_check(o, h, sm, batch, 3, [(0, 53, 93)], (3, 64, 0), stats=st)
    assert st.get("left_no_candidate", 0) == 0 and st["left_attempted"] == 2
    st = {}
    classify_and_check(o, h, sm, batch, 3, [(0, 54, 94)], (3, 64, 0), stats=st)
    assert st["left_no_candidate"] == 2


def test_left_end_at_the_records_first_base(oracle):
    """the left end's mirror of the record bound: a new block that starts exactly at record base 0 (d - n == 0) is placed; with one
    read base more in front of it the block would start at -1: the site is no candidate, and the end stays a clip -- tried all the
    same it would cost that one base and be placed"""
    rng = np.random.default_rng(46)
    s = junction_gene(rng, 0, 10, 60, 120)                       # exon [0, 10), intron [10, 70), exon [70, 190)
    o, h, sm = build_kb(oracle, [s], k=17)
    h.alignments_enable(8)
    reads = []
    both(reads, cut(s, ((0, 10), (70, 130))))
    both(reads, np.concatenate([[differs(s[0])], cut(s, ((0, 10), (70, 130)))]).astype(np.uint8))
    batch = synth.batch_from_lists(reads)
    st = {}
    _, _, got = classify_and_check(o, h, sm, batch, 8, [(0, 10, 70)], stats=st)
    for strand in range(2):
        assert blocks_of(got[strand, 0]) == [(0, 0, 10), (70, 10, 60)] and blocks_of(got[2 + strand, 0]) == [(70, 11, 60)]
    assert st["left_placed"] == 2 and st["left_no_candidate"] == 2
    st = {}
    _, _, got = classify_and_check(o, h, sm, batch, 8, [(0, 10, 70)], (3, 64, 0), stats=st)
    assert st["left_placed"] == 2 and st["left_no_candidate"] == 2 and blocks_of(got[3, 0]) == [(70, 11, 60)]


# ---------------------------------------------------------------------------
# 3. competition
# ---------------------------------------------------------------------------
def test_competition(oracle):
    rng = np.random.default_rng(35)

    def skipping_gene():
        e1, i1, e2, i2, e3 = (synth.random_seq(rng, n) for n in (80, 50, 50, 50, 80))
        e3[:4] = e2[:4]                                          # exon skipping: exon 3 begins like exon 2 for four bases, then differs twice
        e3[4], e3[5] = differs(e2[4]), differs(e2[5])
        for t in range(6):
            i1[t] = differs(e2[t], e3[t])
        return np.concatenate([e1, i1, e2, i2, e3])              # exons [0, 80), [130, 180), [230, 310)

    s, twin, with_n = skipping_gene(), skipping_gene(), skipping_gene()
    twin[80:86] = twin[130:136]                                  # the intron begins like the next exon
    with_n[135] = ord("N")
    o, h, sm = build_kb(oracle, [s, twin, with_n], k=17, min_quality=20)
    h.alignments_enable(8)
    reads, quals = [], []

    def add(m, q=None):
        for r, qq in ((np.array(m, np.uint8), q), (synth.revcomp(np.array(m, np.uint8)), None if q is None else q[::-1])):
            reads.append(r)
            quals.append(np.full(len(r), ord("I"), np.uint8) if qq is None else qq)

    add(cut(s, ((20, 80), (130, 134))))                          # 0: two acceptors, h = 4: a clip
    add(cut(s, ((20, 80), (130, 136))))                          # 2: h = 6: placed on exon 2
    # 4: the null candidate ties -- the substituted base silences the windows over the intron's six bases, which would else simply vote
    add(sub(cut(twin, ((20, 80), (130, 136))), 59))
    base = cut(s, ((20, 80), (130, 150)))
    own = [0] * 4 + [1] * 2 + [0] * 10 + [2] * 2
    for n in (1, 2, 3):                                          # 6, 8, 10: substitutions in the overhang
        add(sub(base, *[62 + 3 * t for t in range(n)]))
    m = base.copy()
    m[65] = ord("N")
    add(m)                                                       # 12
    q = np.full(80, ord("I"), np.uint8)
    q[[64, 66]] = ord("#")
    add(base.copy(), q)                                          # 14: two masked bytes
    add(cut(with_n, ((20, 80), (130, 150))))                     # 16: a record N under the overhang
    batch = synth.batch_from_lists(reads, None, quals)
    sites = [(0, 80, 130), (0, 80, 230), (1, 80, 130), (2, 80, 130)]
    for params in (DEFAULTS, (3, 2, 0), (3, 0, 1), (3, 3, 3), (3, 64, 0)):
        st = {}
        classify_and_check(o, h, sm, batch, 8, sites, params, q=20, stats=st)
    def at_own_gene(goff, gids, got):
        assert gids.tolist() == own
        return list(got[:, 0])

    st = {}
    goff, gids, got = classify_and_check(o, h, sm, batch, 8, sites, DEFAULTS, q=20, stats=st)
    mine = at_own_gene(goff, gids, got)
    n_blocks = [int(r["n_blocks"]) for r in mine]
    assert n_blocks[0:2] == [1, 1] and blocks_of(mine[2]) == [(20, 0, 60), (130, 60, 6)] and n_blocks[4:6] == [1, 1]
    assert n_blocks[6:12] == [2, 2, 2, 2, 1, 1] and n_blocks[12:18] == [2, 2, 2, 2, 2, 2]
    assert st["right_ambiguous"] >= 4 and st["right_too_costly"] >= 2, st
    # min_gap 0: the tie rule decides (the largest acceptor), and the intron's twin is placed
    goff, gids, got = classify_and_check(o, h, sm, batch, 8, sites, (3, 2, 0), q=20)
    mine = at_own_gene(goff, gids, got)
    assert blocks_of(mine[0]) == [(20, 0, 60), (230, 60, 4)] and int(mine[4]["n_blocks"]) == 2
    # max_cost 0: the N, the masked bytes and the record's N are each not a match
    goff, gids, got = classify_and_check(o, h, sm, batch, 8, sites, (3, 0, 1), q=20)
    assert [int(r["n_blocks"]) for r in at_own_gene(goff, gids, got)[12:18]] == [1] * 6


# ---------------------------------------------------------------------------
# 4. the block budget
# ---------------------------------------------------------------------------
def test_block_budget(oracle):
    rng = np.random.default_rng(36)
    ex = [synth.random_seq(rng, n) for n in (80, 40, 80, 60, 60)]
    introns = [synth.random_seq(rng, 50) for _ in range(4)]
    s = np.concatenate([ex[0], introns[0], ex[1], introns[1], ex[2], introns[2], ex[3], introns[3], ex[4]])
    sites = [(0, 80, 130), (0, 170, 220), (0, 300, 350), (0, 410, 460)]      # exons [0, 80), [130, 170), [220, 300), [350, 410), [460, 520)
    o, h, sm = build_kb(oracle, [s], k=17)
    h.alignments_enable(8)
    reads = []
    both(reads, cut(s, ((70, 80), (130, 170), (220, 230))))                             # one block becomes three
    both(reads, cut(s, ((70, 80), (130, 170), (220, 300), (350, 410), (460, 470))))     # three blocks, two placeable ends: the left only
    both(reads, cut(s, ((70, 80), (130, 170), (220, 300), (350, 410), (460, 520))))     # four blocks: untouched
    both(reads, cut(s, ((40, 80), (130, 170), (220, 230))))                             # two blocks and the right end
    batch = synth.batch_from_lists(reads)
    _, _, plain = classify_and_check(o, h, sm, batch, 8, [], (0, 0, 0))
    assert [int(r["n_blocks"]) for r in plain[:, 0]] == [1, 1, 3, 3, 4, 4, 2, 2]
    st = {}
    _, _, got = classify_and_check(o, h, sm, batch, 8, sites, stats=st)
    for strand in range(2):
        assert blocks_of(got[strand, 0]) == [(70, 0, 10), (130, 10, 40), (220, 50, 10)]
        assert blocks_of(got[2 + strand, 0]) == [(70, 0, 10)] + blocks_of(plain[2 + strand, 0]) and blocks_of(plain[2 + strand, 0])[0] == (130, 10, 40)
        assert got[4 + strand, 0].tobytes() == plain[4 + strand, 0].tobytes()
        assert blocks_of(got[6 + strand, 0]) == [(40, 0, 40), (130, 40, 40), (220, 80, 10)]
    assert st["left_placed"] == 4 and st["right_placed"] == 4
    classify_and_check(o, h, sm, synth.batch_from_lists(reads, reads[::-1]), 8, sites, P=4, B=5)


# ---------------------------------------------------------------------------
# 5. more candidates than lanes
# ---------------------------------------------------------------------------
def test_a_range_of_130_candidates(oracle):
    """130 listed sites whose donors all fall into one end's range [xe - 16, xe + h - 1] (h = 48: 64 donors, two or three acceptors
    each), the true one among them and a same-shift neighbour; and their mirror for a left end"""
    rng = np.random.default_rng(37)
    s = junction_gene(rng, 0, 120, 200, 120)                     # exon [0, 120), intron [120, 320), exon [320, 440)
    o, h, sm = build_kb(oracle, [s], k=17)
    h.alignments_enable(8)
    reads = []
    both(reads, cut(s, ((50, 120), (320, 368))))                 # xe = 120, h = 48: donors 104 .. 167
    both(reads, cut(s, ((72, 120), (320, 390))))                 # x0 = 320, h = 48: acceptors 273 .. 336
    batch = synth.batch_from_lists(reads)
    right = {(120, 320), (121, 321)}
    left = {(120, 320)}
    d = 104
    while len(right) < 130:
        right.add((d, 200 + (len(right) * 7) % 180 + (d - 104)))
        d = d + 1 if d < 167 else 104
    a = 273
    while len(left) < 130:
        left.add((20 + (len(left) * 5) % 90, a))
        a = a + 1 if a < 336 else 273
    for sites, name in ((right, "right"), (left, "left"), (right | left, "both")):
        st = {}
        lst = sorted((0, d, a) for d, a in sites if d < a)
        assert len(lst) >= 130
        _, _, got = classify_and_check(o, h, sm, batch, 8, lst, stats=st)
        if name != "left":
            assert blocks_of(got[0, 0]) == [(50, 0, 70), (320, 70, 48)] == blocks_of(got[1, 0])
        if name != "right":
            assert blocks_of(got[2, 0]) == [(72, 0, 48), (320, 48, 70)] == blocks_of(got[3, 0])
        classify_and_check(o, h, sm, batch, 8, lst, (3, 64, 0))


# ---------------------------------------------------------------------------
# 6. step 3a behind it, 7. aligned pileup, 8. pairs and rescue
# ---------------------------------------------------------------------------
def test_with_end_extension_and_aligned_pileup(oracle):
    rng = np.random.default_rng(38)
    s = junction_gene(rng, 3)                                    # (the intron's first three bases are exon 2's: what step 3a alone would take)
    o, h, sm = build_kb(oracle, [s], k=17)
    reads = []
    both(reads, sub(cut(s, ((20, 80), (140, 150))), 2))          # the right end is placed, the left extended through its substitution
    both(reads, sub(cut(s, ((70, 80), (140, 200))), 67))         # the left end is placed, the right extended
    both(reads, cut(s, ((20, 80), (140, 150))))
    batch = synth.batch_from_lists(reads)
    site = [(0, 80, 140)]
    h.alignments_enable(8)
    _, _, got = classify_and_check(o, h, sm, batch, 8, site, DEFAULTS, 4, 5)
    assert blocks_of(got[0, 0]) == [(20, 0, 60), (140, 60, 10)] and int(got[0, 0]["mismatches"]) == 1
    assert blocks_of(got[2, 0]) == [(70, 0, 10), (140, 10, 60)] and int(got[2, 0]["mismatches"]) == 1
    _, _, unext = classify_and_check(o, h, sm, batch, 8, site, DEFAULTS, 0, 0)
    assert blocks_of(unext[0, 0]) == [(23, 3, 57), (140, 60, 10)]
    # aligned pileup at the same floor, with and without the records; the placed overhang is counted at the acceptor side
    for with_records in (True, False):
        h.alignments_enable(8 if with_records else 0)
        h.pileup_enable_aligned(8)
        h.pileup_reset()
        set_step(h, site, DEFAULTS)
        h.alignments_extend(4, 5)
        goff, gids = h.classify(*_args(batch))
        recs = model_records(o, sm, batch, goff, gids, 8, site, DEFAULTS, 4, 5)
        counts, mates, bearing = expected_aligned_pileup(sm, batch, goff, gids, recs)
        state_is(h, counts, mates, bearing)
        pile = h.pileup_all()
        assert int(pile[140:150].sum()) == 10 * 6 and int(pile[80:140].sum()) == 0 and int(pile.sum()) == bearing == 6 * 70
        if with_records:
            same_records(h.alignments_last(), recs)
    # without the step the overhang's matching prefix lies in the intron and nothing of it at the acceptor side
    h.pileup_reset()
    set_step(h, [], DEFAULTS)
    goff, gids = h.classify(*_args(batch))
    recs = model_records(o, sm, batch, goff, gids, 8, [], (0, 0, 0), 4, 5)
    state_is(h, *expected_aligned_pileup(sm, batch, goff, gids, recs))
    pile = h.pileup_all()
    assert int(pile[80:83].sum()) == 3 * 4 and int(pile[140:143].sum()) == 2 * 3


def test_pairs_and_rescue_read_the_new_records(oracle):
    from tests.pairs_model import expected_pairs
    from tests.rescue_model import expected_rescue
    rng = np.random.default_rng(39)
    panel = [spliced_gene(rng, 2, 17) for _ in range(3)]
    records = [g for g, _ in panel]
    o, h, sm = build_kb(oracle, records, k=17)
    batch = spliced_reads(rng, panel, 120, ragged=True, sub=0.01)
    og, oi = o.classify(*_args(batch))
    rows = expected_segments(sm, batch, og, oi, 4)[1]
    sites = sorted({(g, d, d + i) for g, d, a, i, n in table_rows(expected_junction_table(batch, og, oi, rows, 17, 8))})
    h.alignments_enable(8)
    h.pairs_enable(20, 1000, 1024)
    st = {}
    goff, gids, got = classify_and_check(o, h, sm, batch, 8, sites, stats=st)
    assert st["mates_gained"] >= 5, st
    assert h.pairs_last().tobytes() == expected_pairs(got, batch, goff, 20, 1000).tobytes()
    h.rescue_enable(20, 1000, 8, 4)
    goff, gids = h.classify(*_args(batch))
    want_al, want_rs = expected_rescue(got, batch, goff, gids, {g: bytes(r) for g, r in enumerate(records)}, 20, 1000, 8, 4)
    assert h.alignments_last().tobytes() == want_al.tobytes() and h.rescue_last().tobytes() == want_rs.tobytes()
    assert h.pairs_last().tobytes() == expected_pairs(want_al, batch, goff, 20, 1000).tobytes()


# ---------------------------------------------------------------------------
# 9. inert
# ---------------------------------------------------------------------------
def test_the_step_is_inert_for_every_older_result(oracle):
    from shark_amd import SharkHip
    rng = np.random.default_rng(2028)
    panel = [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(6)]
    records = [g for g, _ in panel]
    batches = [spliced_reads(rng, panel, 150, ragged=False, sub=0.02), spliced_reads(rng, panel, 150, ragged=True, sub=0.02)]
    o, _, sm = build_kb(oracle, records, k=17)
    sites = set()
    for b in batches:
        og, oi = o.classify(*_args(b))
        rows = expected_segments(sm, b, og, oi, 4)[1]
        sites |= {(g, d, d + i) for g, d, a, i, n in table_rows(expected_junction_table(b, og, oi, rows, 17, 8))}
    sites = np.array(sorted(sites), dtype=np.int64)
    seen = {}
    for how in ("never", "on", "min_overhang 0", "list dropped"):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in records], keep_bases=True)
        h.evidence_enable(True)
        h.candidates_enable(4)
        h.placement_enable(True)
        h.segments_enable(2)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        h.pileup_enable(8)
        h.alignments_enable(8)
        h.alignments_extend(4, 5)
        h.pairs_enable(20, 1000, 1024)
        if how != "never":
            h.splice_sites_set(sites)
            h.alignments_splice(*DEFAULTS)
        if how == "min_overhang 0":
            h.alignments_splice(0, 2, 2)
        if how == "list dropped":
            h.splice_sites_set(np.zeros((0, 3), np.int64))
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            cr, ce = h.candidates_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                         keys.tobytes(), segs.tobytes()))
        seen[how] = (rows, h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.junctions_get().tobytes(), h.pileup_all().tobytes(),
                     h.pileup_mates(), h.variants().tobytes(), h.alignments_last().tobytes(), h.pairs_last().tobytes())
    assert seen["never"] == seen["min_overhang 0"] == seen["list dropped"]
    assert seen["never"][:-2] == seen["on"][:-2] and seen["never"][-2] != seen["on"][-2]


# ---------------------------------------------------------------------------
# 10. all four submit families and the repair paths
# ---------------------------------------------------------------------------
def test_all_four_families_and_a_repaired_batch(oracle):
    rng = np.random.default_rng(40)
    s = junction_gene(rng, 0)
    site = [(g, 80, 140) for g in range(6)]
    o, h, sm = build_kb(oracle, [s.copy() for _ in range(6)], k=17)
    reads = []
    for i in range(30):
        both(reads, cut(s, ((10 + i, 80), (140, 146 + i % 20))))
    batch = synth.batch_from_lists(reads[:30], reads[30:])
    h.alignments_enable(8)
    set_step(h, site, DEFAULTS)
    goff, gids = h.classify(*_args(batch))
    want = model_records(o, sm, batch, goff, gids, 8, site, DEFAULTS)
    assert int((want["n_blocks"] == 2).sum()) == 6 * 60
    same_records(h.alignments_last(), want)
    h.wait(h.submit(*_args(batch)))
    same_records(h.alignments_last(), want)
    dev = _to_device(batch)
    from shark_amd.capi import alignments_from_device
    device_assoc(h.classify_device(30, max_read_len=120, **_dev_ptrs(dev)))
    same_records(alignments_from_device(*h.alignments_last()), want)
    device_assoc(h.wait_device(h.submit_device(30, max_read_len=120, **_dev_ptrs(dev))))
    same_records(alignments_from_device(*h.alignments_last()), want)
    # more associations than a slot reserves (3 000 reads tied over 6 identical genes): the tail runs again in wait, the batch is stored
    # and -- under aligned pileup -- counted once
    h.pileup_enable_aligned(8)
    many = [reads[i % 60] for i in range(3000)]
    big = synth.batch_from_lists(many)
    goff, gids = h.classify(*_args(big))
    assert int(goff[-1]) == 18000
    got = h.alignments_last()
    small = synth.batch_from_lists(reads)
    sgoff, sgids = np.arange(0, 61, dtype=np.uint32), np.zeros(60, np.uint16)
    rows = expected_segments(sm, small, sgoff, sgids, 4)[1]
    one = expected_alignments_spliced(sm, small, sgoff, sgids, rows, 8, site, DEFAULTS)
    for i in (0, 1, 59, 60, 2999):
        for g in range(6):
            assert got[6 * i + g, 0].tobytes() == one[i % 60, 0].tobytes()
    per_gene = expected_aligned_pileup(sm, small, sgoff, sgids, one)[0][:220]
    pile = h.pileup_all()
    assert h.pileup_mates() == 18000 and all(np.array_equal(pile[220 * g:220 * (g + 1)], per_gene * 50) for g in range(6))
    # the length bound: mates longer than max_read_len send the batch through the other repair path
    long_reads = [np.concatenate([s[0:80], s[140:220]])] + reads[:29]
    lb = synth.batch_from_lists(long_reads, reads[30:])
    t = _to_device(lb)
    h.pileup_enable_aligned(0)
    goff, gids = device_assoc(h.wait_device(h.submit_device(30, max_read_len=100, **_dev_ptrs(t))))
    assert h.timing()["last_n_long"] > 0
    same_records(alignments_from_device(*h.alignments_last()), model_records(o, sm, lb, goff, gids, 8, site, DEFAULTS))


# ---------------------------------------------------------------------------
# 11. state rules
# ---------------------------------------------------------------------------
def test_state_rules(oracle):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(41)
    s = junction_gene(rng, 0)
    ok = np.array([(0, 80, 140)], dtype=np.int64)
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError, match="not finalized"):
        h.splice_sites_set(ok)
    with pytest.raises(SharkHipError, match="no site list"):
        h.alignments_splice(3, 2, 2)
    h.alignments_splice(0, 2, 2)                                 # (switching off needs nothing)
    o, h, sm = build_kb(oracle, [s, s[:100].copy()], k=17)
    with pytest.raises(SharkHipError, match="no site list"):
        h.alignments_splice(3, 2, 2)
    for bad in ([(2, 80, 140)], [(0, 0, 140)], [(0, 80, 80)], [(0, 140, 80)], [(0, 80, 220)], [(1, 50, 100)], [(0, 80, 140), (0, 80, 140)],
                [(0, 80, 140), (0, 80, 139)], [(1, 10, 20), (0, 80, 140)], [(0, 81, 140), (0, 80, 141)]):
        with pytest.raises(SharkHipError, match="shk_splice_sites_set"):
            h.splice_sites_set(np.array(bad, dtype=np.int64))
    with pytest.raises(SharkHipError, match="no site list"):    # (a refused list leaves none behind)
        h.alignments_splice(3, 2, 2)
    h.splice_sites_set(np.array([(0, 1, 219), (0, 80, 140), (1, 1, 99)], dtype=np.int64))
    h.splice_sites_set(np.array([(0, 80, 140)], dtype=capi_sites()).reshape(-1))      # (the record dtype as well; replaces the list)
    for bad in ((49, 2, 2), (3, 65, 2), (3, 2, 65), (1 << 31, 0, 0)):
        with pytest.raises(SharkHipError, match="shk_alignments_splice"):
            h.alignments_splice(*bad)
    h.alignments_splice(48, 64, 64)
    h.alignments_splice(*DEFAULTS)
    h.splice_sites_set(np.zeros((0, 3), np.int64))               # n == 0 drops the list and switches the step off
    with pytest.raises(SharkHipError, match="no site list"):
        h.alignments_splice(3, 2, 2)
    # tickets outstanding; the parameters are those the batch was submitted with
    h.alignments_enable(8)
    h.splice_sites_set(ok)
    h.alignments_splice(*DEFAULTS)
    reads = []
    both(reads, cut(s, ((20, 80), (140, 150))))
    b = synth.batch_from_lists(reads)
    tk = h.submit(*_args(b))
    for call in (lambda: h.splice_sites_set(ok), lambda: h.splice_sites_set(np.zeros((0, 3), np.int64)), lambda: h.alignments_splice(3, 2, 2),
                 lambda: h.alignments_splice(0, 0, 0)):
        with pytest.raises(SharkHipError, match="outstanding"):
            call()
    goff, gids = h.wait(tk)
    h.alignments_splice(0, 0, 0)
    got = h.alignments_last()
    same_records(got, model_records(o, sm, b, goff, gids, 8, [(0, 80, 140)], DEFAULTS))
    assert blocks_of(got[0, 0]) == [(20, 0, 60), (140, 60, 10)]
    h.classify(*_args(b))
    assert blocks_of(h.alignments_last()[0, 0]) == [(20, 0, 60)]


def capi_sites():
    from shark_amd import capi
    return capi.SPLICE_SITE_DTYPE


# ---------------------------------------------------------------------------
# 12. the command
# ---------------------------------------------------------------------------
def test_shark_splice_junctions_on_the_example(oracle, example_dir, tmp_path):
    """run 1 writes --junctions J; run 2 reads it: the SAM (and under --pileup-aligned the pileup) is the model's byte for byte from one
    worker, from two workers on one device and at another batch size; every line passes the verifier; the SAM differs from the run
    without the flag"""
    from types import SimpleNamespace
    from tests.align_model import sam_header, sam_lines
    from tests.depth_model import model_layout
    from tests.pileup_model import pileup_lines
    from tests.splice_cases import example_spliced
    from tests.test_align_cpu import _raw_mates
    from tests.test_gpu_align import _sam_file_is, run_shark
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    legend = [n.decode() for n, _ in fa]
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    ids = [i.decode() if isinstance(i, bytes) else str(i) for i, _, _ in r1]
    quals = [(bytes(a[2]), bytes(b[2])) for a, b in zip(r1, r2)]
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"), "-2", os.path.join(example_dir, "sample_2.fq"),
            "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    r = run_shark(base + ["--junctions", str(tmp_path / "J")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    seen = {}
    for P, B, flags in ((0, 0, []), (4, 5, ["--extend-ends", "--pileup-aligned", "--pileup"])):
        sm, batch, goff, gids, jlines, sites, plain, recs, st = example_spliced(oracle, fa, DEFAULTS, P, B)
        from tests.splice_model import sites_from_junction_lines
        assert sites_from_junction_lines((tmp_path / "J").read_text().split("\n"), legend, [len(q) for _, q in fa]) == sites
        fasta = {legend[g]: bytes(sm.records.get(g, b"")) for g in range(len(fa))}
        header = sam_header(legend, SimpleNamespace(records=dict(enumerate(fasta.values()))), len(fasta))
        lines = sam_lines(ids, _raw_mates(batch), quals, goff, gids, recs, legend, True)
        want = "".join(ln + "\n" for ln in header + lines).encode("latin-1")
        lines0 = sam_lines(ids, _raw_mates(batch), quals, goff, gids, plain, legend, True)
        want0 = "".join(ln + "\n" for ln in header + lines0).encode("latin-1")
        assert want != want0 and st["mates_gained"] > 100
        want_pu = "".join(ln + "\n" for ln in pileup_lines(expected_aligned_pileup(sm, batch, goff, gids, recs)[0], model_layout(sm, len(fa)), legend)).encode()
        for tag, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "700"]), ("c", ["--batch", "333", "--splice-min-overhang", "3", "--splice-max-cost", "2"])):
            name = "s%d%s" % (P, tag)
            fl = flags + [str(tmp_path / ("p" + tag))] if flags else []
            r = run_shark(base + ["--sam", str(tmp_path / name), "--splice-junctions", str(tmp_path / "J")] + fl + extra, str(tmp_path))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            _sam_file_is(tmp_path / name, want, fasta, len(lines))
            if flags:
                assert (tmp_path / ("p" + tag)).read_bytes() == want_pu
        r = run_shark(base + ["--sam", str(tmp_path / "s0")] + (flags + [str(tmp_path / "p0")] if flags else []), str(tmp_path))
        assert r.returncode == 0 and (tmp_path / "s0").read_bytes() == want0
        seen[P] = want
        if P == 0:
            plain_file = want0
    assert seen[0] != seen[4]
    # a list that names an unknown gene, or a site outside its record, names the line
    (tmp_path / "bad").write_text("%s 10 20 10 1\nnobody 10 20 10 1\n" % legend[0])
    r = run_shark(base + ["--sam", str(tmp_path / "sx"), "--splice-junctions", str(tmp_path / "bad")], str(tmp_path))
    assert r.returncode == 1 and b"line 2: unknown gene" in r.stderr
    (tmp_path / "bad").write_text("%s 10 20 999999 1\n" % legend[0])
    r = run_shark(base + ["--sam", str(tmp_path / "sx"), "--splice-junctions", str(tmp_path / "bad")], str(tmp_path))
    assert r.returncode == 1 and b"line 1: the site lies outside its record" in r.stderr
    # --splice-min-mates above every line's count leaves the step off: the file without the flag
    r = run_shark(base + ["--sam", str(tmp_path / "sm"), "--splice-junctions", str(tmp_path / "J"), "--splice-min-mates", "1000000"], str(tmp_path))
    assert r.returncode == 0 and (tmp_path / "sm").read_bytes() == plain_file
