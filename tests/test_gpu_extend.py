"""End extension (shk_alignments_extend) and aligned pileup (shk_pileup_enable_aligned) on the GPU, against the model
(tests/extend_model.py), record by record and counter by counter, byte for byte.  The model prices an overhang with one cumulative sum
and counts the pileup from the final records; it is fed the GPU's own gene_off / gene_ids, which are compared with the CPU oracle's
first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth
from tests.extend_model import expected_aligned_pileup, expected_alignments_extended
from tests.pileup_model import expected_pileup
from tests.segments_model import expected_segments
from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_align import same_records
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import device_assoc
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu

PB = ((4, 5), (1, 0), (15, 0), (4, 0), (1, 15))


def _differs(*bases):
    return next(c for c in synth.ACGT if all(c != b for b in bases))


def sub(m, *at):
    m = np.array(m, dtype=np.uint8)
    for i in at:
        m[i] = _differs(m[i])
    return m


def model_records(o, sm, batch, goff, gids, s_min, P, B, q=0, stats=None):
    og, oi = o.classify(*_args(batch))
    assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
    rows = expected_segments(sm, batch, goff, gids, 4, q)[1]
    return expected_alignments_extended(sm, batch, goff, gids, rows, s_min, P, B, q, stats)


def classify_and_check(o, h, sm, batch, s_min, P, B, q=0, stats=None):
    h.alignments_extend(P, B)
    goff, gids = h.classify(*_args(batch))
    want = model_records(o, sm, batch, goff, gids, s_min, P, B, q, stats)
    got = h.alignments_last()
    same_records(got, want)
    return goff, gids, got


# ---------------------------------------------------------------------------
# 1. records against the model: substitutions near the ends, the parameter sets, ties
# ---------------------------------------------------------------------------
def end_cases(rng, rec, L, k):
    """mates of L bases with one substitution at a read index near an end (0, 1, 4 and 15 -- overhangs that score exactly 0 at (1, 0),
    (4, 0) and (15, 0) --, k - 1, L - k, L - 2, L - 1, ...), with two in one overhang, and clean; each on both strands"""
    at = sorted({i for i in (0, 1, 4, 15, k - 1, L - k, L - 16, L - 5, L - 2, L - 1) if 0 <= i < L})
    pairs = [(3, 9), (1, k - 2), (L - 10, L - 4), (L - k + 1, L - 2), (0, L - 1)]
    reads = []
    for n, subs in enumerate([()] + [(i,) for i in at] + pairs):
        a = int(rng.integers(5, len(rec) - L - 5))
        m = sub(rec[a:a + L], *subs)
        reads += [m, synth.revcomp(m)]
    return reads, 2 * (1 + len(at))


@pytest.mark.parametrize("k,L", [(17, 100), (17, 61), (5, 60)])
def test_substitutions_near_the_ends_at_every_parameter_set(oracle, k, L):
    rng = np.random.default_rng(1000 + k + L)
    rec = synth.random_seq(rng, 450)
    o, h, sm = build_kb(oracle, [rec], k=k)
    h.alignments_enable(3)
    reads, n_single = end_cases(rng, rec, L, k)
    single = synth.batch_from_lists(reads)
    paired = synth.batch_from_lists(reads, reads[::-1])
    seen = {}
    for P, B in PB:
        st = {}
        _, _, got = classify_and_check(o, h, sm, single, 3, P, B, stats=st)
        assert not got[:, 1].tobytes().strip(b"\0")
        classify_and_check(o, h, sm, paired, 3, P, B)
        seen[(P, B)] = (got.tobytes(), st)
        # (at (15, 0) only an overhang of more than 16 bases pays for its substitution: index k - 1 and its mirror, at k = 17)
        need = 4 if (P, B) in ((4, 5), (1, 15)) else (1 if k == 17 or P < 15 else 0)
        assert st.get("left", 0) >= need and st.get("right", 0) >= need, (P, B, st)
    # the bonus decides (4, 5) against (4, 0), and the penalty (1, 0) against (15, 0)
    assert seen[(4, 5)][0] != seen[(4, 0)][0] and seen[(1, 0)][0] != seen[(15, 0)][0]
    # at (4, 5) a single substitution is always extended through: the clean mate and every mate with one substitution is one block over
    # all its L bases (the mates with two substitutions follow; what they give is the model's)
    h.alignments_extend(4, 5)
    goff, _ = h.classify(*_args(single))
    assert np.array_equal(goff[:n_single + 1], np.arange(n_single + 1))
    one = h.alignments_last()[:n_single, 0]
    assert (one["n_blocks"] == 1).all() and (one["block"][:, 0, 1] == 0).all() and (one["block"][:, 0, 2] == L).all()
    # P = 0: bit-identical to alignments mode without the call
    h.alignments_extend(0, 0)
    h.classify(*_args(single))
    off = h.alignments_last().tobytes()
    o2, h2, _ = build_kb(oracle, [rec], k=k)
    h2.alignments_enable(3)
    h2.classify(*_args(single))
    assert off == h2.alignments_last().tobytes() and off != seen[(4, 5)][0]
    assert h.last_kernel() == h2.last_kernel()


# ---------------------------------------------------------------------------
# 2. pass boundaries
# ---------------------------------------------------------------------------
def overhang_mate(rec, a, H, cut=None, tail=()):
    """rec[a : a + 40 + H]: 40 voting bases, then an overhang of H bases whose base 0 and bases 10, 26, 42, ... are substituted: no
    window of 17 votes in it, and the voting span ends exactly at read base 40, so the kernel scores an overhang of H bases.  cut: from
    overhang base `cut` on every second base is substituted as well (the best prefix ends there); tail: overhang bases substituted on top"""
    m = np.array(rec[a:a + 40 + H], dtype=np.uint8)
    xs = {0} | set(range(10, H, 16)) | set(tail)
    if cut is not None:
        xs |= set(range(cut, H, 2))
    return sub(m, *[40 + t for t in sorted(xs)])


def test_pass_boundaries_of_the_scorer(oracle):
    """overhangs of exactly 63, 64, 65 and 129 bases (the block before extension is checked to be the 40 voting bases) on the right and,
    against the reverse-complemented record, on the left, on both strands: the best prefix at the last lane of pass 1 (e = 64), at the
    first lane of pass 2 (e = 65), at 7 with a whole pass of net loss behind it, and at the mate's end with the bonus deciding.
    By hand at (4, 5), from the substituted bases 0, 10, 26, 42, 58, 74, ...: every stretch between two of them is at least 9 matches,
    so the whole overhang wins where nothing else is substituted (e = H); with every second base substituted from 64 (65) on, e = 64
    (65): five (six) matches behind base 58 pay for it; from 7 on, e = 7 (6 - 4 > 0).  Base H - 2 substituted on top: behind base 58
    (122) there are two substitutions and H - 60 (H - 124) matches, which the bonus of 5 carries for H = 64, 65, 129 (+1, +2, +2; at
    H = 63 it is a tie, so that case is left out); at (1, 0) the last two bases score -1 + 1, a tie that stays at e = H - 2."""
    rng = np.random.default_rng(64)
    rec = synth.random_seq(rng, 600)
    rc = synth.revcomp(rec)                                      # (on it the same mates have their overhang in front of the voting bases)
    reads, overhang, want_e, tail_case = [], [], [], []
    for H in (63, 64, 65, 129):
        cases = [(None, (), H)] + [(cut, (), cut) for cut in (64, 65, 7) if cut + 2 < H] + ([(None, (H - 2,), None)] if H != 63 else [])
        for cut, tail, e in cases:
            m = overhang_mate(rec, 100, H, cut, tail)
            reads += [m, synth.revcomp(m)]
            overhang += [H, H]
            want_e += [e, e]
    batch = synth.batch_from_lists(reads)
    assert {64, 65, 7, 63, 129} <= set(want_e)
    for record, left in ((rec, False), (rc, True)):
        o, h, sm = build_kb(oracle, [record], k=17)
        h.alignments_enable(8)
        # before extension: the 40 voting bases and nothing else, so the kernel's overhang is H bases exactly
        _, gids, plain = classify_and_check(o, h, sm, batch, 8, 0, 0)
        assert (gids == 0).all() and len(gids) == len(reads)
        for j, H in enumerate(overhang):
            r = plain[j, 0]
            assert int(r["n_blocks"]) == 1 and int(r["strand"]) == (j & 1) ^ left
            x, q, ln = (int(v) for v in r["block"][0])
            assert (q, ln) == ((H, 40) if left else (0, 40)), (j, r)
            assert H == (q if left else len(reads[j]) - (q + ln))
        for P, B in ((4, 5), (4, 0), (1, 0)):
            _, _, got = classify_and_check(o, h, sm, batch, 8, P, B)
            for j, (H, e) in enumerate(zip(overhang, want_e)):
                r = got[j, 0]
                x, q, ln = (int(v) for v in r["block"][0])
                got_e = ln - 40
                assert int(r["n_blocks"]) == 1 and got_e == (H - q if left else got_e) and (left or q == 0), (j, r)
                if e is not None and (P, B) == (4, 5):
                    assert got_e == e, (j, got_e, e, left)
                if e is None and (P, B) == (4, 5):
                    assert got_e == H, (j, got_e, H, left)
                if e is None and (P, B) == (1, 0):
                    assert got_e == H - 2, (j, got_e, H, left)


# ---------------------------------------------------------------------------
# 3. record ends, 4. junction overhangs, 5. non-bases
# ---------------------------------------------------------------------------
def test_record_ends_junction_overhangs_and_non_bases(oracle):
    rng = np.random.default_rng(33)
    rec = synth.random_seq(rng, 300)
    spliced = []                                                 # exon of 80, intron of 60, exon of 80; each gene its own exons
    for same in (0, 3):
        e1, intron, e2 = synth.random_seq(rng, 80), synth.random_seq(rng, 60), synth.random_seq(rng, 80)
        for t in range(4):
            intron[t] = e2[t] if t < same else _differs(e2[t])
        spliced.append(np.concatenate([e1, intron, e2]))
    with_n = rec.copy()
    with_n[[3, 296]] = ord("N")
    o, h, sm = build_kb(oracle, [rec] + spliced + [with_n[::-1].copy()], k=17, min_quality=20)
    h.alignments_enable(8)
    junk = synth.random_seq(rng, 12)
    reads, quals = [], []

    def add(m, q=None):
        for r, qq in ((m, q), (synth.revcomp(m), None if q is None else q[::-1])):
            reads.append(np.array(r, dtype=np.uint8))
            quals.append(np.full(len(r), ord("I"), np.uint8) if qq is None else qq)

    # 3. hanging over the record's first and its last base, with and without a substitution at the record's outermost bases
    add(np.concatenate([junk, rec[:70]]))
    add(np.concatenate([junk, sub(rec[:70], 0)]))
    add(np.concatenate([junk, sub(rec[:70], 2)]))
    add(np.concatenate([rec[-70:], junk]))
    add(np.concatenate([sub(rec[-70:], 69), junk[:3]]))
    # 4. ten bases past a junction: the intron's first bases differ from exon 2's, or exactly its first three agree
    for s in spliced:
        add(np.concatenate([s[20:80], s[140:150]]))
        add(np.concatenate([s[70:80], s[140:200]]))              # (and ten bases in front of one: the left end against the intron's end)
    # 5. N in the overhang, at its end, and bytes masked by -q
    m = sub(rec[100:180], 5, 74)
    for ns in ((2,), (0,), (0, 1), (78, 79), (77,), (79,)):
        mm = m.copy()
        mm[list(ns)] = ord("N")
        add(mm)
    for lowq in ((0, 1), (2, 3), (78, 79), (76,)):
        q = np.full(80, ord("I"), np.uint8)
        q[list(lowq)] = ord("#")
        add(m.copy(), q)
    # a record non-base under the overhang
    w = with_n[::-1]
    for cutout, at, n_at in ((w[0:80], 6, 3), (w[220:300], 73, 76)):
        mm = sub(cutout, at)
        assert mm[n_at] == ord("N")
        mm[n_at] = ord("A")                                      # (the read shows a base where the record has none)
        add(mm)
    batch = synth.batch_from_lists(reads, None, quals)
    for P, B in ((4, 5), (4, 0), (1, 1)):
        st = {}
        goff, gids, got = classify_and_check(o, h, sm, batch, 8, P, B, q=20, stats=st)
        assert st["left"] >= 5 and st["right"] >= 5, st
    # (4, 5), by hand: the clip at the record's ends remains and no bonus is earned there
    h.alignments_extend(4, 5)
    goff, gids = h.classify(*_args(batch))
    got = h.alignments_last()[:, 0]
    blocks = [tuple(int(v) for v in r["block"][0]) for r in got]
    assert blocks[0] == (0, 12, 70) and blocks[1] == (0, 12, 70)     # record on strand 0 / the mate's reverse: the same record
    assert blocks[2] == (1, 13, 69) and blocks[4] == (3, 15, 67)     # a substitution at the record's first base: nothing waits behind it
    assert blocks[6] == (230, 0, 70) and blocks[8] == (230, 0, 69)
    j = 10                                                           # the junction overhangs: e = 0 and e = 3, no bonus
    assert blocks[j] == (20, 0, 60) and blocks[j + 4] == (20, 0, 63)
    assert all(int(r["n_blocks"]) == 1 for r in got[:j + 8])


# ---------------------------------------------------------------------------
# 6. inert
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(2027)
    return [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(8)]


def test_everything_new_is_inert_for_every_older_result(oracle, panel):
    """every older mode on; extension beside them, and then extension with aligned pileup in owned pileup's stead, change none of the
    older results byte for byte (the pileup state itself holds the other kind in the third context, and the alignments are extended)"""
    from shark_amd import SharkHip
    rng = np.random.default_rng(41)
    records = [g for g, _ in panel]
    batches = [spliced_reads(rng, panel, 200, ragged=False, sub=0.03), spliced_reads(rng, panel, 200, ragged=True, sub=0.03)]
    seen = []
    for new in (0, 1, 2):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in records], keep_bases=True)
        h.placement_enable(True)
        h.segments_enable(2)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        if new == 2:
            h.pileup_enable_aligned(8)
        else:
            h.pileup_enable(8)
        h.alignments_enable(8)
        if new:
            h.alignments_extend(4, 5)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.placement_last().tobytes(), keys.tobytes(), segs.tobytes()))
        seen.append((rows, h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.junctions_get().tobytes(),
                     h.pileup_all().tobytes(), h.pileup_mates(), h.variants().tobytes(), h.alignments_last().tobytes()))
    assert seen[0][:-1] == seen[1][:-1] and seen[0][-1] != seen[1][-1]
    # aligned pileup on: genes, gene counts, shk_last_kernel, placements, segments, depth and junctions as before; the alignments are
    # the extended ones; the pileup state is of the other kind (its counts are held against the model in the tests below)
    assert seen[2][:5] == seen[0][:5] and seen[2][-1] == seen[1][-1] and seen[2][5] != seen[0][5] and seen[2][6] == seen[0][6] > 0


# ---------------------------------------------------------------------------
# 7. aligned pileup against the model
# ---------------------------------------------------------------------------
def aligned_model(o, sm, batch, goff, gids, s_min, P, B, q=0, stats=None):
    recs = model_records(o, sm, batch, goff, gids, s_min, P, B, q, stats)
    return recs, expected_aligned_pileup(sm, batch, goff, gids, recs, q)


def state_is(h, counts, mates, bearing=None):
    got = h.pileup_all()
    assert got.shape == counts.shape
    if not np.array_equal(got, counts):
        x = np.nonzero((got != counts).any(axis=1))[0]
        raise AssertionError("base %d: got %s, model %s (%d bases differ)" % (x[0], got[x[0]], counts[x[0]], len(x)))
    assert h.pileup_mates() == mates
    if bearing is not None:
        assert int(got.astype(np.uint64).sum()) == bearing


@pytest.mark.parametrize("twins", [False, True])
def test_aligned_pileup_with_trimming_closure_extension_and_ties(oracle, panel, twins):
    from tests.align_model import expected_alignments
    rng = np.random.default_rng(71 + twins)
    genes = panel[:3] + ([panel[0]] if twins else [])
    o, h, sm = build_kb(oracle, [g for g, _ in genes], k=17)
    batch = spliced_reads(rng, genes[:3], 250, sub=0.03)
    total = None
    for P, B, with_records in ((4, 5, False), (0, 0, True), (1, 0, True)):
        h.alignments_extend(P, B)
        h.alignments_enable(8 if with_records else 0)            # (with the records: one launch does both; without: none are stored)
        h.pileup_enable_aligned(8)
        goff, gids = h.classify(*_args(batch))
        st = {}
        rows = expected_segments(sm, batch, goff, gids, 4)[1]
        expected_alignments(sm, batch, goff, gids, rows, 8, stats=st)
        assert st.get("trimmed", 0) >= 1 and st.get("closed", 0) >= 1, st
        recs, (counts, mates, bearing) = aligned_model(o, sm, batch, goff, gids, 8, P, B)
        if with_records:
            same_records(h.alignments_last(), recs)
        total = counts if total is None else total + counts
        assert mates == int((recs["n_blocks"] > 0).sum()) > 200
        state_is(h, counts, mates, bearing)
        if twins:
            assert int(goff[-1]) > 250
        h.pileup_reset()
    # another floor than alignments mode's: two launches, each at its own
    h.alignments_extend(4, 5)
    h.alignments_enable(20)
    h.pileup_enable_aligned(8)
    goff, gids = h.classify(*_args(batch))
    same_records(h.alignments_last(), model_records(o, sm, batch, goff, gids, 20, 4, 5))
    _, (counts, mates, bearing) = aligned_model(o, sm, batch, goff, gids, 8, 4, 5)
    state_is(h, counts, mates, bearing)


def test_single_block_mates_without_extension_count_as_owned_pileup_through_all_four_families(oracle):
    rng = np.random.default_rng(77)
    genes = synth.make_genes(rng, 3, 400, 600)
    o, h, sm = build_kb(oracle, genes, k=17)
    cut = []
    for i in range(120):
        g = genes[i % 3]
        a = int(rng.integers(0, len(g) - 90))
        m = g[a:a + 90].copy()
        s = rng.random(90) < 0.03
        m[s] = synth.ACGT[rng.integers(0, 4, size=int(s.sum()))]
        cut.append(m if i & 1 else synth.revcomp(m))
    batch = synth.batch_from_lists(cut[:60], cut[60:])
    goff, gids = o.classify(*_args(batch))
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    owned, _, owned_mates = expected_pileup(sm, batch, goff, gids, rows, 8)
    h.pileup_enable_aligned(8)
    dev = _to_device(batch)
    n = 0
    h.classify(*_args(batch)); n += 1
    h.wait(h.submit(*_args(batch))); n += 1
    device_assoc(h.classify_device(60, max_read_len=120, **_dev_ptrs(dev))); n += 1
    device_assoc(h.wait_device(h.submit_device(60, max_read_len=120, **_dev_ptrs(dev)))); n += 1
    p = _dev_ptrs(dev)
    h.count_work(60, p["seq1"], p["off1"], p["seq2"], p["off2"])           # a measurement: not counted
    state_is(h, owned * n, owned_mates * n)
    # and with extension the state is the model's of the extended records
    h.pileup_reset()
    h.alignments_extend(4, 5)
    h.classify(*_args(batch))
    recs, (counts, mates, bearing) = aligned_model(o, sm, batch, goff, gids, 8, 4, 5)
    state_is(h, counts, mates, bearing)
    assert int(counts.sum()) > int(owned.sum())


def test_repair_paths_count_a_batch_once(oracle):
    """more associations than a slot reserves (3 000 reads tied over 6 identical genes), and mates of 1 500 bases behind max_read_len = 100:
    the tail runs again in wait, and the batch is counted there only"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    o, h, sm = build_kb(oracle, [twin.copy() for _ in range(6)], k=17)
    h.alignments_extend(4, 5)
    h.pileup_enable_aligned(8)
    reads = [sub(twin[(7 * i) % 200:(7 * i) % 200 + 100], 3) for i in range(3000)]
    batch = synth.batch_from_lists(reads)
    goff, gids = h.classify(*_args(batch))
    assert int(goff[-1]) == 18000
    small = synth.batch_from_lists(reads[:200])                  # reads repeat with period 200: the model prices one period on one gene
    sgoff, sgids = np.arange(0, 201, dtype=np.uint32), np.zeros(200, np.uint16)
    rows = expected_segments(sm, small, sgoff, sgids, 4)[1]
    recs = expected_alignments_extended(sm, small, sgoff, sgids, rows, 8, 4, 5)
    one = expected_aligned_pileup(sm, small, sgoff, sgids, recs)[0][:600]
    got = h.pileup_all()
    assert h.pileup_mates() == 18000 and all(np.array_equal(got[600 * g:600 * (g + 1)], one * 15) for g in range(6))
    assert int(one[:, :].sum()) == 200 * 100                     # every base of every mate: extended through the substitution
    # the length bound
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, sm = build_kb(oracle, long_genes, k=17)
    h.alignments_extend(4, 5)
    h.pileup_enable_aligned(8)
    mates = [np.concatenate([long_genes[i % 3][20 * i:20 * i + (1500 if i % 5 == 0 else 50)], long_genes[i % 3][2000 + 20 * i:2000 + 20 * i + (1500 if i % 5 == 0 else 50)]])
             for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    goff, gids = device_assoc(h.wait_device(h.submit_device(40, max_read_len=100, **_dev_ptrs(t))))
    assert h.timing()["last_n_long"] > 0
    _, (counts, n_mates, bearing) = aligned_model(o, sm, b, goff, gids, 8, 4, 5)
    state_is(h, counts, n_mates, bearing)


# ---------------------------------------------------------------------------
# 8. the tiling case
# ---------------------------------------------------------------------------
def test_tiling_every_read_offset_of_a_site(oracle):
    """L = 100, k = 17, s_min = 8: owned pileup shows the record's base 100 times and the other base 66 times; aligned pileup at (4, 5)
    shows 100 against 100, and the site is a variant at frac 1/2 only then (the figures are the model's: tests/test_extend_cpu.py)"""
    from tests.extend_cases import tiling_case
    rec, site, reads = tiling_case()
    o, h, sm = build_kb(oracle, [np.frombuffer(rec, np.uint8)], k=17)
    batch = synth.batch_from_lists(reads)
    r = b"ACGT".index(rec[site:site + 1])
    a = int(np.argmax([0 if b == r else 1 for b in range(4)]))  # (the substituted base is the first that differs)
    h.pileup_enable(8)
    h.classify(*_args(batch))
    n = h.pileup_all()[site]
    assert int(n[r]) == 100 and int(n[a]) == 66 and int(n.sum()) == 166
    assert site not in h.variants(8, 3, (1, 2))["x"].tolist()
    h.pileup_reset()
    h.alignments_extend(4, 5)
    h.pileup_enable_aligned(8)
    goff, gids = h.classify(*_args(batch))
    n = h.pileup_all()[site]
    assert int(n[r]) == 100 and int(n[a]) == 100 and int(n.sum()) == 200
    assert h.variants(8, 3, (1, 2))["x"].tolist() == [site]
    _, (counts, mates, bearing) = aligned_model(o, sm, batch, goff, gids, 8, 4, 5)
    state_is(h, counts, mates, bearing)
    assert mates == 200 and bearing == 200 * 100


# ---------------------------------------------------------------------------
# 9. state rules
# ---------------------------------------------------------------------------
def test_state_rules(oracle, panel):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    records = [g for g, _ in panel]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    h.alignments_extend(4, 5)                                   # needs no index
    for P, B in ((16, 0), (0, 16), (4, 1 << 31), (1 << 20, 5)):
        with pytest.raises(SharkHipError):
            h.alignments_extend(P, B)
    h.alignments_extend(15, 15)
    h.alignments_extend(0, 0)
    with pytest.raises(SharkHipError, match="not finalized"):
        h.pileup_enable_aligned(8)
    h.pileup_enable_aligned(0)
    o, h, sm = build_kb(oracle, records, keep_bases=False, k=17)
    with pytest.raises(SharkHipError, match="without shk_ref_keep_bases"):
        h.pileup_enable_aligned(8)                              # positions kept, bases not
    h.pileup_enable(8)                                          # (owned pileup needs no bases)
    o, h, sm = build_kb(oracle, records, k=17)
    b = spliced_reads(rng, panel, 60)
    # one state holds one kind: free to switch until a batch was counted, and again behind a reset
    h.pileup_enable(8)
    h.pileup_enable_aligned(8)
    h.pileup_enable(8)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError, match="other kind"):
        h.pileup_enable_aligned(8)
    h.pileup_enable(0)
    h.pileup_enable_aligned(0)                                  # (switching off is always allowed)
    h.pileup_reset()
    h.pileup_enable_aligned(8)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError, match="other kind"):
        h.pileup_enable(8)
    h.pileup_enable_aligned(8)
    h.pileup_reset()
    h.pileup_enable(8)
    h.pileup_reset()
    h.pileup_enable_aligned(8)
    # tickets outstanding
    tk = h.submit(*_args(b))
    for call in (lambda: h.alignments_extend(4, 5), lambda: h.alignments_extend(0, 0), lambda: h.pileup_enable_aligned(8), lambda: h.pileup_enable_aligned(0)):
        with pytest.raises(SharkHipError, match="outstanding"):
            call()
    h.wait(tk)
    assert h.pileup_mates() > 0
    # the parameters are those the batch was submitted with
    h.alignments_enable(8)
    h.alignments_extend(4, 5)
    tk = h.submit(*_args(b))
    goff, gids = h.wait(tk)
    h.alignments_extend(0, 0)
    same_records(h.alignments_last(), model_records(o, sm, b, goff, gids, 8, 4, 5))


# ---------------------------------------------------------------------------
# 10. the command
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mutated", [False, True])
def test_shark_extend_ends_and_pileup_aligned_on_theexample_alignments(oracle, example_dir, tmp_path, mutated):
    """`shark --sam --extend-ends --variants --pileup --pileup-aligned` on the bundled sample against the record and against §14's
    record with twelve substituted bases: the three files are the model's, byte for byte, from one worker, from two workers on one
    device and at another batch size; every SAM line passes the verifier"""
    import os
    from types import SimpleNamespace
    from tests.align_model import sam_header, sam_lines
    from tests.depth_model import model_layout
    from tests.pileup_model import pileup_lines
    from tests.test_align_cpu import _raw_mates
    from tests.extend_cases import example_alignments
    from tests.test_gpu_align import _sam_file_is, run_shark
    from tests.test_variants_cpu import mutated_example_records
    from tests.variants_model import expected_variants, variant_lines
    fa = mutated_example_records() if mutated else synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    sm, batch, goff, gids, recs, st = example_alignments(oracle, fa, 4, 5)
    legend = [n.decode() for n, _ in fa]
    fasta = {legend[g]: bytes(sm.records.get(g, b"")) for g in range(len(fa))}
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    ids = [i.decode() if isinstance(i, bytes) else str(i) for i, _, _ in r1]
    quals = [(bytes(a[2]), bytes(b[2])) for a, b in zip(r1, r2)]
    lines = sam_lines(ids, _raw_mates(batch), quals, goff, gids, recs, legend, True)
    header = sam_header(legend, SimpleNamespace(records=dict(enumerate(fasta.values()))), len(fasta))
    want_sam = "".join(ln + "\n" for ln in header + lines).encode("latin-1")
    counts = expected_aligned_pileup(sm, batch, goff, gids, recs)[0]
    gs = model_layout(sm, len(fa))
    want_pu = "".join(ln + "\n" for ln in pileup_lines(counts, gs, legend)).encode()
    want_va = "".join(ln + "\n" for ln in variant_lines(expected_variants(counts, [s for _, s in fa], gs), legend)).encode()
    with open(tmp_path / "ref.fa", "wb") as f:
        for name, seq in fa:
            f.write(b">" + name + b"\n" + seq + b"\n")
    base = ["-r", str(tmp_path / "ref.fa"), "-1", os.path.join(example_dir, "sample_1.fq"), "-2", os.path.join(example_dir, "sample_2.fq"),
            "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2"), "--extend-ends", "--pileup-aligned"]
    for tag, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "700"]), ("c", ["--batch", "333", "--extend-penalty", "4", "--extend-bonus", "5"])):
        r = run_shark(base + ["--sam", str(tmp_path / ("s" + tag)), "--variants", str(tmp_path / ("v" + tag)), "--pileup", str(tmp_path / ("p" + tag))] + extra,
                      str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        nms = _sam_file_is(tmp_path / ("s" + tag), want_sam, fasta, len(lines))
        assert (tmp_path / ("p" + tag)).read_bytes() == want_pu and (tmp_path / ("v" + tag)).read_bytes() == want_va
        assert (sum(nm > 0 for nm in nms) > 1000) == mutated
    if mutated:
        assert len(want_va.splitlines()) == 8                    # (tests/test_extend_cpu.py's figure)
    # other parameters give another file; aligned pileup alone (no --sam) writes the same pileup
    r = run_shark(base + ["--pileup", str(tmp_path / "pd")], str(tmp_path))
    assert r.returncode == 0 and (tmp_path / "pd").read_bytes() == want_pu
    r = run_shark(base[:-1] + ["--sam", str(tmp_path / "se"), "--extend-bonus", "0"], str(tmp_path))     # (without --pileup-aligned)
    assert r.returncode == 0 and (tmp_path / "se").read_bytes() != want_sam
    if mutated:
        # without the new flags the files are what they always were: alignments without extension, owned pileup
        from tests.pileup_model import expected_pileup as owned_pileup
        sm0, batch0, goff0, gids0, recs0, _ = example_alignments(oracle, fa, 0, 0)
        lines0 = sam_lines(ids, _raw_mates(batch0), quals, goff0, gids0, recs0, legend, True)
        want0 = "".join(ln + "\n" for ln in header + lines0).encode("latin-1")
        counts0 = owned_pileup(sm0, batch0, goff0, gids0, expected_segments(sm0, batch0, goff0, gids0, 4)[1], 8)[0]
        r = run_shark(base[:-2] + ["--sam", str(tmp_path / "s0"), "--pileup", str(tmp_path / "p0")], str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        _sam_file_is(tmp_path / "s0", want0, fasta, len(lines0))
        assert (tmp_path / "p0").read_bytes() == "".join(ln + "\n" for ln in pileup_lines(counts0, gs, legend)).encode()
        assert want0 != want_sam and len(lines0) == len(lines)
