"""Alignments mode on the GPU (shk_alignments_enable / shk_alignments_last): per association and mate the 64-byte record -- blocks,
strand, match and mismatch counts -- against the model (tests/align_model.py), record by record, byte for byte.  The model keeps
per-mate arrays with ownership by first writer, prices every split of a gap base by base and shares no idea with the kernel; it is fed
the GPU's own gene_off / gene_ids, which are compared with the CPU oracle's first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import synth
from tests.align_cases import geometry_case, geometry_conditions
from tests.align_model import expected_alignments, sam_header, verify_sam_line
from tests.segments_model import expected_segments
from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import device_assoc
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_records(got, want):
    assert got.dtype == capi.ALIGNMENT_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = [(j, t) for j in range(len(want)) for t in range(2) if got[j, t].tobytes() != want[j, t].tobytes()]
        j, t = bad[0]
        raise AssertionError("association %d mate %d: got %s, model %s (%d records differ)" % (j, t + 1, got[j, t], want[j, t], len(bad)))


def model_records(o, sm, batch, goff, gids, s_min, q=0, stats=None):
    """the model's records for the GPU's own associations, which must be the oracle's"""
    og, oi = o.classify(*_args(batch))
    assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
    rows = expected_segments(sm, batch, goff, gids, 4, q)[1]
    return expected_alignments(sm, batch, goff, gids, rows, s_min, q, stats)


def classify_and_check(o, h, sm, batch, s_min, q=0, stats=None):
    goff, gids = h.classify(*_args(batch))
    want = model_records(o, sm, batch, goff, gids, s_min, q, stats)
    got = h.alignments_last()
    same_records(got, want)
    return goff, gids, got


# ---------------------------------------------------------------------------
# 1. geometry
# ---------------------------------------------------------------------------
# The generator's seed per case: the first one (counting from 1) whose 150 pairs meet every non-vacuity condition of
# geometry_conditions, found with the model alone on the CPU (tools/align_seeds.py).  At k = 31 no seed up to 300 meets them all: a
# substitution shows as a mismatch only where windows of 31 vote on both sides of it inside one block, and a gap with more read than
# record bases needs two exons of the mate that both hold votes of 31 around the six repeated bases.  DROPPED names the one condition
# such a case is not asked for; its seed is the first that meets all the others.
SEEDS = {(5, "one gene"): 1, (5, "two genes"): 1, (5, "twins"): 1, (17, "one gene"): 4, (17, "two genes"): 1, (17, "twins"): 1,
         (31, "one gene"): 22, (31, "two genes"): 1, (31, "twins"): 1}
DROPPED = {(31, "one gene"): "mismatches", (31, "two genes"): "open insertion", (31, "twins"): "open insertion"}


@pytest.mark.parametrize("k", [5, 17, 31])
@pytest.mark.parametrize("ref", ["one gene", "two genes", "twins"])
def test_geometry_strands_indels_and_ties(oracle, k, ref):
    """mates over 0 to 5 junctions on both strands, with a deletion and with a repeat, 3 % substitutions; one gene, two genes, and two
    identical genes (every read tied over both: the two genes' records of a read are equal)"""
    genes, s_min, batch = geometry_case(k, ref, SEEDS[(k, ref)])
    o, h, sm = build_kb(oracle, [g for g, _ in genes], k=k)
    h.alignments_enable(s_min)
    stats = {}
    goff, gids, got = classify_and_check(o, h, sm, batch, s_min, stats=stats)
    cond = geometry_conditions(got, stats)
    print("aligned", int((got["n_blocks"] > 0).sum()), "by blocks", np.bincount(got["n_blocks"].ravel(), minlength=5).tolist(), stats,
          "with mismatches", int((got["mismatches"] > 0).sum()))
    for name, met in cond.items():
        assert met or DROPPED.get((k, ref)) == name, name
    if ref == "twins":
        assert int(goff[-1]) > 150
        for i in range(150):
            a, b = int(goff[i]), int(goff[i + 1])
            assert b - a in (0, 2) and (b == a or got[a].tobytes() == got[a + 1].tobytes())


# ---------------------------------------------------------------------------
# 2. lane passes
# ---------------------------------------------------------------------------
def test_lane_passes_record_ends_and_substitutions_at_the_pass_boundary(oracle):
    """unspliced mates of 17 .. 600 bytes (one window; around one and two passes of 64 block coordinates; past segments_kernel's 512
    cached slots) on both strands, flush with the record's start, flush with its end, and inside; s_min = 1.  One substitution at
    coordinates 63 and 64 of a block (the last lane of a pass, the first of the next).  A window that votes agrees with the record
    base for base, so an unspliced mate's block begins and ends with k matching bases: a substitution at the mate's first or last
    base moves the block's end behind it -- the base is clipped and must not be counted -- and with base 0 substituted as well, mate
    base 64 is coordinate 63 of the block."""
    rng = np.random.default_rng(64)
    rec = synth.random_seq(rng, 700)
    o, h, sm = build_kb(oracle, [rec], k=17)
    h.alignments_enable(1)

    def sub(m, *at):
        m = m.copy()
        for i in at:
            m[i] = synth.ACGT[(int(np.searchsorted(synth.ACGT, m[i])) + 1) % 4]
        return m

    # want: (x, q, len, mismatches), the same on either strand (q counts in the record's orientation).  A mate of 17 bytes has one
    # window: substituted it has no k-mer and no association, so it comes clean only
    reads, want = [], []
    for L in (17, 63, 64, 65, 128, 129, 600):
        for a in (0, 700 - L, 41):
            m = rec[a:a + L]
            cases = [(m.copy(), (a, 0, L, 0))]
            if L > 17:
                cases += [(sub(m, 0), (a + 1, 1, L - 1, 0)), (sub(m, L - 1), (a, 0, L - 1, 0))]
            if L >= 128:
                cases += [(sub(m, 63), (a, 0, L, 1)), (sub(m, 64), (a, 0, L, 1)), (sub(m, 0, 64), (a + 1, 1, L - 1, 1))]
            for mm, w in cases:
                reads += [mm, synth.revcomp(mm)]
                want += [w, w]
    batch = synth.batch_from_lists(reads)
    goff, gids, got = classify_and_check(o, h, sm, batch, 1)
    assert len(gids) == len(reads) and np.array_equal(goff, np.arange(len(reads) + 1))
    for j, w in enumerate(want):
        r = got[j, 0]
        assert not got[j, 1].tobytes().strip(b"\0")                               # single-end: mate 2 all zero
        assert (int(r["n_blocks"]), int(r["strand"]), int(r["matches"]), int(r["mismatches"])) == (1, j & 1, w[2] - w[3], w[3]), (j, r, w)
        assert tuple(int(v) for v in r["block"][0]) == w[:3] and not r["block"][1:].any(), (j, r, w)


# ---------------------------------------------------------------------------
# 3. closure edges on the device
# ---------------------------------------------------------------------------
def _differs(*bases):
    return next(c for c in synth.ACGT if all(c != b for b in bases))


def gap_read(rng, R, G, not_a=None, not_b=None):
    """(record, read): exon of 60, G intron bases, exon of 60; the read is the last 40 bases of the first exon, R junk bases, the first
    40 of the second.  not_a[t] / not_b[t]: whether junk base t differs from the record base under it on the left / the right block's
    diagonal (None: whatever random bases give); the junk's first base always differs on the left and its last on the right, so that
    no window over the junk votes and the gap is R read bases exactly.  With patterns the intron is written to fit (G >= 2 R); a
    pattern must not let 17 bases in a row match, or the windows over them vote and the gap is none"""
    e1, e2, intron, junk = (synth.random_seq(rng, n) for n in (60, 60, G, R))
    if not_a is not None:
        assert G >= 2 * R and not_a[0] and not_b[R - 1]
        for t in range(R):
            intron[t] = _differs(junk[t]) if not_a[t] else junk[t]
            intron[G - R + t] = _differs(junk[t]) if not_b[t] else junk[t]
    else:
        junk[0] = _differs(intron[0])
        junk[R - 1] = _differs(intron[G - 1], intron[0] if R == 1 else intron[G - 1])
    return np.concatenate([e1, intron, e2]), np.concatenate([e1[20:], junk, e2[:40]])


def test_closure_edges(oracle):
    """R = 1, 63, 64 close and R = 65 stays open; equal cost at two splits; the best split at s = 0 and at s = R; G == R + 1"""
    rng = np.random.default_rng(3)
    ones = lambda n: [1] * n  # noqa: E731
    cases = [("R=1", gap_read(rng, 1, 30), (1, 1)),
             ("R=63", gap_read(rng, 63, 100), (63, None)), ("R=64", gap_read(rng, 64, 100), (64, None)), ("R=65", gap_read(rng, 65, 100), None),
             # junk base 2 matches both diagonals, 1 the left only, 3 the right only: splits 2 and 3 both cost 2
             ("tie", gap_read(rng, 5, 40, [1, 0, 0, 1, 1], [1, 1, 0, 0, 1]), (5, 3)),
             ("s=0", gap_read(rng, 6, 40, ones(6), [0, 0, 0, 0, 0, 1]), (6, 0)),
             ("s=R", gap_read(rng, 6, 40, [1, 0, 0, 0, 0, 0], ones(6)), (6, 6)),
             # (every tenth base differs: s = 64 costs 7 and every other split more; mirrored for s = 0)
             ("s=R at 64", gap_read(rng, 64, 200, [int(t % 10 == 0) for t in range(64)], ones(64)), (64, 64)),
             ("s=0 at 64", gap_read(rng, 64, 200, ones(64), [int((63 - t) % 10 == 0) for t in range(64)]), (64, 0)),
             # (G == R is one diagonal, not a gap: the hand-worked cases of test_align_cpu.py have it)
             ("G=R+1", gap_read(rng, 5, 6), (5, None)), ("G=R-1", gap_read(rng, 5, 4), None)]
    records = [rec for _, (rec, _), _ in cases]
    o, h, sm = build_kb(oracle, records, k=17)
    h.alignments_enable(8)
    reads = []
    for _, (_, read), _ in cases:
        reads += [read, synth.revcomp(read)]
    batch = synth.batch_from_lists(reads)
    stats = {}
    goff, gids, got = classify_and_check(o, h, sm, batch, 8, stats=stats)
    assert np.array_equal(gids, np.repeat(np.arange(len(cases)), 2)), "every read lies on its own record"
    for c, (name, (rec, read), closed) in enumerate(cases):
        for j in (2 * c, 2 * c + 1):
            r = got[j, 0]
            b = [tuple(int(v) for v in r["block"][i]) for i in range(2)]
            assert int(r["n_blocks"]) == 2 and int(r["strand"]) == j & 1, (name, r)
            R_left = b[1][1] - (b[0][1] + b[0][2])
            if closed is None:                                # left open: the exons as they voted
                assert b[0] == (20, 0, 40) and b[1][1:] == (len(read) - 40, 40) and R_left == len(read) - 80, (name, r)
            else:
                R, s = closed
                assert R_left == 0 and b[0][:2] == (20, 0) and b[1][1] + b[1][2] == len(read) and b[0][2] + b[1][2] == len(read), (name, r)
                assert s is None or b[0][2] == 40 + s, (name, r, s)
    assert stats == {"closed": 2 * sum(c is not None for _, _, c in cases), "open_wide": 2, "open_insertion": 2}, stats


# ---------------------------------------------------------------------------
# 4. the -q mask, N, lower case
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(2026)
    return [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]


def test_masked_bytes_and_non_bases_count_as_neither(oracle, panel):
    rng = np.random.default_rng(11)
    o, h, sm = build_kb(oracle, [g for g, _ in panel], k=17, min_quality=20)
    h.alignments_enable(8)
    less = 0
    for paired, ragged in ((True, False), (False, True)):
        batch = spliced_reads(rng, panel, 200, paired=paired, ragged=ragged, qual=True, lower=0.2)
        _, _, got = classify_and_check(o, h, sm, batch, 8, q=20)
        total = got["block"][..., 2].sum(axis=-1)
        counted = got["matches"] + got["mismatches"]
        assert (counted <= total).all()
        less += int((counted < total).sum())
        if not paired:
            assert not got[:, 1].tobytes().strip(b"\0")
    assert less >= 1


# ---------------------------------------------------------------------------
# 5. cross-checks with the existing modes
# ---------------------------------------------------------------------------
def test_against_pileup_variants_and_segments_mode(oracle, panel):
    rng = np.random.default_rng(13)
    records = [g for g, _ in panel]
    spliced = spliced_reads(rng, panel, 200, sub=0.03)
    # unspliced mates with substitutions: one block each, nothing trimmed and nothing closed
    cut = []
    for i in range(200):
        g = records[i % len(records)]
        a = int(rng.integers(0, len(g) - 90))
        m = g[a:a + 90].copy()
        s = rng.random(90) < 0.03
        m[s] = synth.ACGT[rng.integers(0, 4, size=int(s.sum()))]
        cut.append(m if i & 1 else synth.revcomp(m))
    unspliced = synth.batch_from_lists(cut[:100], cut[100:])
    seen = {}
    for m in (0, 4, 2):
        for name, batch in (("spliced", spliced), ("unspliced", unspliced)):
            o, h, sm = build_kb(oracle, records, k=17)
            h.alignments_enable(8)
            h.pileup_enable(8)
            h.segments_enable(m)
            stats = {}
            goff, gids = h.classify(*_args(batch))
            got = h.alignments_last()
            if m == 0:
                same_records(got, model_records(o, sm, batch, goff, gids, 8, stats=stats))
                seen[name] = got.tobytes()
                # the records with blocks are the pileup mates
                assert int((got["n_blocks"] > 0).sum()) == h.pileup_mates() > 100
                # per gene the mismatches are at least the pileup's where no block lost a base to trimming or moved an end in a closure
                untouched = not stats.get("trimmed") and not stats.get("closed")
                assert untouched == (name == "unspliced"), stats
                if untouched:
                    per_gene = np.bincount(np.repeat(gids, 2), weights=got["mismatches"].ravel(), minlength=len(records)).astype(np.int64)
                    pile = h.variants_summary()["mismatches"].astype(np.int64)
                    assert (per_gene >= pile).all() and pile.sum() > 20, (per_gene, pile)
            else:                                                # segments mode's own launch serves (m = 4) or stands beside (m = 2)
                assert h.segments_last()[1].shape[2] == m and got.tobytes() == seen[name]


# ---------------------------------------------------------------------------
# 6. the four families
# ---------------------------------------------------------------------------
def test_all_four_families(oracle, panel):
    rng = np.random.default_rng(57)
    o, h, sm = build_kb(oracle, [g for g, _ in panel], k=17)
    batches = [spliced_reads(rng, panel, n, ragged=r, paired=p, sub=0.03) for n, r, p in ((200, False, True), (65, True, True), (150, True, False))]
    dev = [_to_device(b) for b in batches]
    h.alignments_enable(6)
    want = []
    for b in batches:                                            # host batches: pinned memory
        goff, gids = h.classify(*_args(b))
        want.append((goff, gids, model_records(o, sm, b, goff, gids, 6)))
        same_records(h.alignments_last(), want[-1][2])
    assert not want[2][2][:, 1].tobytes().strip(b"\0") and want[2][2][:, 0]["n_blocks"].any()     # single-end: mate 2 all zero
    # submit / wait with two tickets in flight: each wait hands out its own batch's records
    t0, t1 = h.submit(*_args(batches[0])), h.submit(*_args(batches[1]))
    for t, w in ((t0, want[0]), (t1, want[1])):
        goff, gids = h.wait(t)
        assert np.array_equal(goff, w[0]) and np.array_equal(gids, w[1])
        same_records(h.alignments_last(), w[2])

    def resident(i):
        return h.classify_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i]))

    def resident_submit(i):
        return h.wait_device(h.submit_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i])))

    for family in (resident, resident_submit):                   # resident batches: the records stay in device memory
        for i, w in enumerate(want):
            goff, gids = device_assoc(family(i))
            assert np.array_equal(goff, w[0]) and np.array_equal(gids, w[1])
            n, ptr = h.alignments_last()
            assert n == len(gids)
            same_records(capi.alignments_from_device(n, ptr), w[2])


def test_association_overflow_repair(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 reads tied over 6 identical genes -- the records come from the
    tail's second run in wait"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    o, h, sm = build_kb(oracle, [twin.copy() for _ in range(6)], k=17)
    h.alignments_enable(8)
    reads = [np.concatenate([twin[(7 * i) % 200:(7 * i) % 200 + 50], twin[300 + (7 * i) % 200:350 + (7 * i) % 200]]) for i in range(3000)]
    batch = synth.batch_from_lists(reads)
    goff, gids = h.classify(*_args(batch))
    assert int(goff[-1]) == 18000
    got = h.alignments_last()
    assert got.shape == (18000, 2) and (got[:, 0]["n_blocks"] == 2).all() and not got[:, 1].tobytes().strip(b"\0")
    # six equal records per read; the model answers for the first association of each (every 6th), which prices all of them
    assert all(got[g::6].tobytes() == got[0::6].tobytes() for g in range(1, 6))
    sub = synth.batch_from_lists(reads[:300])
    sgoff = np.arange(0, 301, dtype=np.uint32)
    rows = expected_segments(sm, sub, sgoff, np.zeros(300, np.uint16), 4)[1]
    same_records(got[0:1800:6], expected_alignments(sm, sub, sgoff, np.zeros(300, np.uint16), rows, 8))


def test_length_bound_repair(oracle):
    """mates of 3 000 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again): the records are the final ones"""
    rng = np.random.default_rng(29)
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, sm = build_kb(oracle, long_genes, k=17)
    h.alignments_enable(8)
    mates = [np.concatenate([long_genes[i % 3][20 * i:20 * i + (1500 if i % 5 == 0 else 50)], long_genes[i % 3][2000 + 20 * i:2000 + 20 * i + (1500 if i % 5 == 0 else 50)]])
             for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    goff, gids = device_assoc(h.wait_device(h.submit_device(40, max_read_len=100, **_dev_ptrs(t))))
    assert h.timing()["last_n_long"] > 0
    n, ptr = h.alignments_last()
    got = capi.alignments_from_device(n, ptr)
    same_records(got, model_records(o, sm, b, goff, gids, 8))
    assert (got["n_blocks"] == 2).all() and int(got["block"][..., 2].max()) >= 1500


# ---------------------------------------------------------------------------
# 7. state rules and inertness
# ---------------------------------------------------------------------------
def test_state_rules(oracle, panel):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    records = [g for g, _ in panel]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError, match="not finalized"):
        h.alignments_enable(8)                    # before finalize
    h.alignments_enable(0)                        # (switching off is always allowed)
    h.build([bytes(g) for g in records])
    with pytest.raises(SharkHipError, match="keep_positions"):
        h.alignments_enable(8)
    o, h, sm = build_kb(oracle, records, keep_bases=False, k=17)
    with pytest.raises(SharkHipError, match="without shk_ref_keep_bases"):
        h.alignments_enable(8)                    # positions kept, bases not
    h.pileup_enable(8)                            # (pileup needs no bases)
    o, h, sm = build_kb(oracle, records, k=17)
    with pytest.raises(SharkHipError):
        h.alignments_last()                       # no batch yet
    b = spliced_reads(rng, panel, 50)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.alignments_last()                       # that batch was submitted with the mode off
    h.alignments_enable(8)
    goff, gids, got = classify_and_check(o, h, sm, b, 8)
    # tickets outstanding
    tk = h.submit(*_args(b))
    for call in (lambda: h.alignments_enable(8), lambda: h.alignments_enable(0)):
        with pytest.raises(SharkHipError, match="outstanding"):
            call()
    h.wait(tk)
    same_records(h.alignments_last(), got)
    # the floor is the one the batch was submitted with
    h.alignments_enable(20)
    g20 = classify_and_check(o, h, sm, b, 20)[2]
    assert g20.tobytes() != got.tobytes()
    # behind shk_count_work nothing is handed out; a batch submitted with the mode off hands out none
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    with pytest.raises(SharkHipError):
        h.alignments_last()
    h.alignments_enable(0)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.alignments_last()
    # a wider index than ids can name
    wide = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    wide.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_bases=True)
    with pytest.raises(SharkHipError, match="65 536"):
        wide.alignments_enable(8)


def test_alignments_mode_is_inert(oracle, panel):
    """every older mode on; alignments switched on beside them changes none of their results, byte for byte"""
    from shark_amd import SharkHip
    rng = np.random.default_rng(41)
    records = [g for g, _ in panel]
    batches = [spliced_reads(rng, panel, 300, ragged=False), spliced_reads(rng, panel, 300, ragged=True)]
    seen = []
    for new in (False, True):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in records], keep_bases=True)
        h.evidence_enable(True)
        h.candidates_enable(4)
        h.placement_enable(True)
        h.segments_enable(2)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        h.pileup_enable(8)
        if new:
            h.alignments_enable(8)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            cr, ce = h.candidates_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                         keys.tobytes(), segs.tobytes()))
            if new:
                assert h.alignments_last()["n_blocks"].any()
        seen.append((rows, h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.depth_summary().tobytes(), h.junctions_get().tobytes(),
                     h.pileup_all().tobytes(), h.pileup_mates(), h.variants().tobytes(), h.variants_summary().tobytes()))
    assert seen[0] == seen[1] and len(seen[0][5]) > 0


# ---------------------------------------------------------------------------
# 8. the command
# ---------------------------------------------------------------------------
def run_shark(args, cwd):
    import subprocess
    return subprocess.run([os.path.join(ROOT, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def _sam_case(oracle, example_dir, tmp_path, fa):
    """(the command's arguments, the file the model expects, the FASTA as the verifier reads it) for the bundled sample against the
    records `fa`"""
    from types import SimpleNamespace
    from tests.test_align_cpu import _example_alignments
    recs, lines, fasta, stats = _example_alignments(oracle, fa)
    header = sam_header(list(fasta), SimpleNamespace(records=dict(enumerate(fasta.values()))), len(fasta))
    want = "".join(ln + "\n" for ln in header + lines).encode("latin-1")
    with open(tmp_path / "ref.fa", "wb") as f:
        for name, seq in fa:
            f.write(b">" + name + b"\n" + seq + b"\n")
    base = ["-r", str(tmp_path / "ref.fa"), "-1", os.path.join(example_dir, "sample_1.fq"), "-2", os.path.join(example_dir, "sample_2.fq"),
            "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    return base, want, fasta, len(lines)


def _sam_file_is(path, want, fasta, n_lines):
    got = path.read_bytes()
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        at = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        raise AssertionError("line %d of %d / %d: got %r, model %r" % (at, len(g), len(w), g[at:at + 1], w[at:at + 1]))
    body = [ln for ln in got.decode("latin-1").split("\n") if ln and not ln.startswith("@")]
    assert len(body) == n_lines
    return [verify_sam_line(ln, fasta) for ln in body]


def test_shark_sam_on_the_example(oracle, example_dir, tmp_path):
    """the file is the model's, byte for byte, from one worker, from two workers on one device, and at two batch sizes; every line
    passes the verifier, and the sample -- simulated from the record without errors -- shows no edit"""
    base, want, fasta, n = _sam_case(oracle, example_dir, tmp_path, synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa")))
    assert n == 3858
    for name, extra in (("s1", []), ("s2", ["--gpus", "2", "--devices", "0,0", "--batch", "700"]), ("s3", ["--batch", "333", "--sam-min-support", "8", "--sam-min-intron", "20"])):
        r = run_shark(base + ["--sam", str(tmp_path / name)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        nms = _sam_file_is(tmp_path / name, want, fasta, n)
        assert not any(nms)


def test_shark_sam_on_the_mutated_example_beside_the_other_outputs(oracle, example_dir, tmp_path):
    """against the record with twelve substituted bases the lines carry edits; --pileup, --variants and --segments beside --sam write
    the files they write without it, and the SAM file is the same beside them"""
    from tests.test_align_cpu import MUTATED_EXAMPLE_LINES_WITH_EDITS
    from tests.test_variants_cpu import mutated_example_records
    base, want, fasta, n = _sam_case(oracle, example_dir, tmp_path, mutated_example_records())
    many = ["--gpus", "2", "--devices", "0,0", "--batch", "700"]
    for name, extra in (("s1", []), ("s2", many), ("s3", ["--batch", "333"])):
        r = run_shark(base + ["--sam", str(tmp_path / name)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        nms = _sam_file_is(tmp_path / name, want, fasta, n)
        assert sum(nm > 0 for nm in nms) == MUTATED_EXAMPLE_LINES_WITH_EDITS
    others = lambda tag: ["--pileup", str(tmp_path / ("pu" + tag)), "--variants", str(tmp_path / ("va" + tag)), "--segments", str(tmp_path / ("sg" + tag))]  # noqa: E731
    r = run_shark(base + others("0") + many, str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    r = run_shark(base + others("1") + ["--sam", str(tmp_path / "s4")] + many, str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for f in ("pu", "va", "sg"):
        assert (tmp_path / (f + "1")).read_bytes() == (tmp_path / (f + "0")).read_bytes() and len((tmp_path / (f + "0")).read_bytes()) > 100, f
    _sam_file_is(tmp_path / "s4", want, fasta, n)


def test_shark_sam_single_end_fasta_sample(oracle, example_dir, tmp_path):
    """a single-end sample without qualities: no pair bits in FLAG, RNEXT `*`, QUAL `*`"""
    from tests.align_model import sam_lines
    from tests.segments_model import SegmentsModel
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    reads = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))[:500]
    with open(tmp_path / "sample.fa", "wb") as f:
        for rid, seq, _ in reads:
            f.write(b">" + rid + b"\n" + seq + b"\n")
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    nidx = o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in reads])
    goff, gids = o.classify(batch["seq1"], batch["off1"], None, None, None, None)
    sm = SegmentsModel([s for _, s in fa], 17)
    recs = expected_alignments(sm, batch, goff, gids, expected_segments(sm, batch, goff, gids, 4)[1], 8)
    legend = [n.decode() for n, _ in fa]
    lines = sam_lines([rid.decode() for rid, _, _ in reads], [(bytes(s), None) for _, s, _ in reads], None, goff, gids, recs, legend, False)
    fasta = {legend[g]: bytes(sm.records.get(g, b"")) for g in range(nidx)}
    want = "".join(ln + "\n" for ln in sam_header(legend, sm, nidx) + lines).encode("latin-1")
    assert len(lines) > 100 and {int(ln.split("\t")[1]) for ln in lines} <= {0, 16} and all(ln.split("\t")[10] == "*" for ln in lines)
    r = run_shark(["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", str(tmp_path / "sample.fa"), "-o", str(tmp_path / "o1"), "--sam", str(tmp_path / "s")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    _sam_file_is(tmp_path / "s", want, fasta, len(lines))
