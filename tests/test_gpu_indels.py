"""Indels mode on the GPU (shk_indels_enable / shk_indels_get / shk_indels_stats / shk_indels_add / shk_indels_reset, `shark --indels`):
the table and the seven counters, entry by entry, against the model (tests/indels_model.py), which shifts an event one base at a time and
shares no idea with the kernel.  The model runs on the model chain's alignment records (segments -> alignments, with steps 3b and 3a where
they are on) and, where a batch hands them out, on the device's own records; both must give the device's table.  Integers, no tolerances.

Some hand-worked cases of tests/test_indels_cpu.py cannot be planted through the pipeline.  A shift that reaches base 0 needs a left
block whose bases repeat at the event's period down to base 0, and such a block holds no unique k-mer.  A window inside a repeat is no
unique k-mer either, so a repeat's inside is a gap that only closure gives to the left block (R <= 64, G >= R): a shift is at most
64 + k - 1 bases -- 63, 64, 65 and 80 are planted, 130 cannot be -- and an insertion moves only in a repeat of at most 2 (k - 1) bases
(a run of 30 and twelve two-base units are planted, forty units cannot be).  A shift that stops at a record N is planted for deletions
(an N in front of a run: shifts of 13 and 33); one base more behind an N leaves G < R, a complex gap.  The model's rules for the cases
left out are checked there.

Run on the GPU box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from shark_amd import capi
from tests import synth
from tests.align_model import expected_alignments
from tests.indels_cases import hand_cases, planted_probe, tile
from tests.indels_model import check_entry, expected_indels, indel_lines, new_stats, pack, table_array
from tests.segments_model import SegmentsModel, expected_segments
from tests.splice_model import expected_alignments_spliced
from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import device_assoc, run_shark
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _seq(letters):
    return 0 if letters == "*" else pack([CODE[c] for c in letters])


class Want:
    """what the table and the counters must hold after the batches added so far"""

    def __init__(self, sm, s_min, min_intron=20, q=0, ext=(0, 0), sites=(), splice=(0, 0, 0)):
        self.sm, self.s_min, self.min_intron, self.q, self.ext, self.sites, self.splice = sm, s_min, min_intron, q, ext, list(sites), splice
        self.reset()

    def reset(self):
        self.table, self.stats, self.shifts = {}, new_stats(), []

    def records(self, batch, goff, gids):
        rows = expected_segments(self.sm, batch, goff, gids, 4, self.q)[1]
        if self.ext[0] or self.splice[0]:
            return expected_alignments_spliced(self.sm, batch, goff, gids, rows, self.s_min, self.sites, self.splice, self.ext[0], self.ext[1], self.q)
        return expected_alignments(self.sm, batch, goff, gids, rows, self.s_min, self.q)

    def add(self, o, batch, goff, gids, device_records=None, times=1):
        og, oi = o.classify(*_args(batch))
        assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
        recs = self.records(batch, goff, gids)
        if device_records is not None:
            # the model over the device's own records gives what it gives over the model chain's
            a = expected_indels(recs, batch, goff, gids, self.sm.records, self.min_intron, self.q)
            b = expected_indels(device_records, batch, goff, gids, self.sm.records, self.min_intron, self.q)
            assert a == b
        for _ in range(times):
            expected_indels(recs, batch, goff, gids, self.sm.records, self.min_intron, self.q, self.table, self.stats, self.shifts)

    def check(self, h, dropped=0):
        want = table_array(self.table)
        got = h.indels_get()
        assert got.dtype == capi.INDEL_DTYPE
        if got.tobytes() != want.tobytes():
            g, w = [tuple(int(v) for v in e) for e in got], [tuple(int(v) for v in e) for e in want]
            raise AssertionError("device only %s, model only %s" % (sorted(set(g) - set(w))[:5], sorted(set(w) - set(g))[:5]))
        st = dict(self.stats)
        st["dropped"] = dropped
        assert h.indels_stats() == st
        return got


def _keys(got):
    return {(int(e["gene"]), int(e["x"]), int(e["kind"]), int(e["len"]), int(e["seq"])): (int(e["fwd"]), int(e["rev"])) for e in got}


# ---------------------------------------------------------------------------
# 1. the planted truth and the hand-worked cases
# ---------------------------------------------------------------------------
def test_planted_truth_on_the_device(oracle):
    record, batch = planted_probe()
    o, h, sm = build_kb(oracle, [record], k=17)
    want = Want(sm, 8)
    h.indels_enable(8, 20, 64)
    h.alignments_enable(8)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids, h.alignments_last())
    got = _keys(want.check(h))
    assert sorted(got) == [(0, 200, 1, 1, _seq("A")), (0, 400, 0, 3, 0), (0, 550, 1, 7, _seq("GATTACA"))]
    assert all(f >= 3 and r >= 3 for f, r in got.values())
    assert [len(h.indels_get(m)) for m in (0, 16, 17, 20, 21)] == [3, 3, 2, 2, 0]


@pytest.fixture(scope="module")
def cases():
    return hand_cases()


@pytest.mark.parametrize("k", [17, 5])
def test_hand_worked_cases(oracle, cases, k):
    """one event per gene, error-free mates across it on both strands (tests/indels_cases.py): insertions of 12 and 13 bases and one
    with an N, deletions of min_intron - 1 and min_intron bases, a complex gap, three bases less in runs of 82, 83, 84 and 99 bases
    (shifts of 63, 64, 65 and 80), an A less in runs of 30 and 50 bases behind a record N (shifts of 13 and 33 that stop at the N), a base
    more in a run of 30, a two-base unit more in twelve units"""
    s_min = 8 if k == 17 else 3
    o, h, sm = build_kb(oracle, [rec for _, rec, _, _ in cases], k=k)
    want = Want(sm, s_min)
    h.indels_enable(s_min, 20, 1024)
    h.alignments_enable(s_min)
    batch = synth.batch_from_lists([m for _, _, mates, _ in cases for m in mates])
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids, h.alignments_last())
    got = _keys(want.check(h))
    print(k, want.stats, "keys", len(got), "shifts", sorted(set(want.shifts)))
    if k == 17:
        assert {0, 13, 16, 33, 63, 64, 65, 80} <= set(want.shifts)
        # every planted key is there, seen from both strands, and nothing else is in its gene
        for g, (name, _, _, key) in enumerate(cases):
            mine = {kk: v for kk, v in got.items() if kk[0] == g}
            if key is None:
                assert not mine, (name, mine)
            else:
                full = (g, key[0], key[1], key[2], _seq(key[3]))
                assert list(mine) == [full] and min(mine[full]) >= 5, (name, mine)
        st = want.stats
        assert st["long_insertions"] >= 10 and st["nonbase_insertions"] >= 10 and st["complex_gaps"] >= 10


def test_a_masked_base_inside_an_insertion(oracle):
    """-q 20: the mates whose inserted bases hold a base of quality 5 count under nonbase_insertions, the others are tabled"""
    _, rec, mates, key = hand_cases()[0]
    o, h, sm = build_kb(oracle, [rec], k=17, min_quality=20)
    want = Want(sm, 8, q=20)
    quals = []
    for n, m in enumerate(mates):
        q = np.full(len(m), 33 + 30, dtype=np.uint8)
        at = 400 + 5 - (280 + 3 * n)                                               # (the sixth inserted base: hand_cases' tiling)
        if n % 3 == 0 and 0 <= at < len(m):
            q[99 - at if n & 1 else at] = 33 + 5
        quals.append(q)
    batch = synth.batch_from_lists(mates, None, quals)
    h.indels_enable(8, 20, 64)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    got = _keys(want.check(h))
    assert list(got) == [(0, key[0], 1, 12, _seq(key[3]))] and want.stats["nonbase_insertions"] >= 3 and want.stats["insertions"] >= 10


# ---------------------------------------------------------------------------
# 2. a synthetic panel with errors
# ---------------------------------------------------------------------------
def _panel(seed, k, n_genes=3):
    rng = np.random.default_rng(seed)
    genes = [spliced_gene(rng, 1 + i % 3, k) for i in range(n_genes)]
    return rng, genes


def _introns(rec, tr):
    """[(donor, acceptor)] of a spliced_gene: the transcript's exons found again in the record, in order (an exon's first 15 bases are
    unique in the record; the left exon keeps what it shares with the intron's start)"""
    out, x, p = [], 0, 0
    while p < len(tr):
        while p < len(tr) and x < len(rec) and rec[x] == tr[p]:
            x, p = x + 1, p + 1
        if p < len(tr):
            nxt = rec.find(tr[p:p + 15], x)
            assert nxt > x
            out.append((x, nxt))
            x = nxt
    return out


def _marks(rec):
    n = len(rec)
    return n // 6, 2 * n // 6, 3 * n // 6, 4 * n // 6, 5 * n // 6


def _haplotype_reads(rng, genes, n):
    """mates from a haplotype of each gene's record that carries a few indels: an A more in the run and a TCA less in the repeat that
    _runs plants, a unique insertion of 3 bases (with an N in it for a fifth of the mates), a deletion of 5 and an insertion of 14;
    3 % substitutions, either strand"""
    out = []
    for rec, _ in genes:
        r = bytes(rec)
        a, b, c, d, e = _marks(r)
        haps = [np.frombuffer(r[:a] + b"A" + r[a:b] + r[b + 3:c] + ins + r[c:d] + r[d + 5:e] + bytes(synth.random_seq(rng, 14)) + r[e:], np.uint8)
                for ins in (b"GTC", b"GNC")]
        for _ in range(n):
            hap = haps[int(rng.random() < 0.2)]
            L = int(rng.integers(70, 121))
            at = int(rng.integers(0, len(hap) - L + 1))
            m = hap[at:at + L].copy()
            s = rng.random(L) < 0.03
            m[s] = synth.ACGT[rng.integers(0, 4, size=int(s.sum()))]
            out.append(synth.revcomp(m) if rng.random() < 0.5 else m)
    return out


def _runs(genes):
    """the genes with a run of six A planted at a sixth of the record and five TCA at a third: the haplotype's changes there move"""
    out = []
    for rec, tr in genes:
        rec = rec.copy()
        a, b = _marks(rec)[:2]
        rec[a - 1:a + 7] = np.frombuffer(b"CAAAAAAG", np.uint8)
        rec[b - 1:b + 16] = np.frombuffer(b"G" + b"TCA" * 5 + b"G", np.uint8)
        out.append((rec, tr))
    return out


@pytest.mark.parametrize("variant", ["plain", "extend", "splice"])
def test_a_panel_with_substitutions_and_a_haplotype_with_indels(oracle, variant):
    rng, plain_genes = _panel(91, 17)
    genes = _runs(plain_genes)
    ext = (4, 5) if variant != "plain" else (0, 0)
    o, h, sm = build_kb(oracle, [g for g, _ in genes], k=17)
    sites, splice = [], (0, 0, 0)
    if variant == "splice":
        sites = [(g, d, a) for g, (rec, tr) in enumerate(plain_genes) for d, a in _introns(bytes(rec), bytes(tr))]
        splice = (3, 2, 2)
    want = Want(sm, 8, ext=ext, sites=sites, splice=splice)
    h.alignments_extend(*ext)
    if splice[0]:
        assert len(sites) >= 3
        h.splice_sites_set(np.array(sites, dtype=np.int64))
        h.alignments_splice(*splice)
    h.indels_enable(8, 20, 4096)
    h.alignments_enable(8)
    b1 = spliced_reads(rng, genes, 150, sub=0.03)
    b2 = synth.batch_from_lists(_haplotype_reads(rng, genes, 80))
    for batch in (b1, b2):
        goff, gids = h.classify(*_args(batch))
        want.add(o, batch, goff, gids, h.alignments_last())
        want.check(h)
    st = want.stats
    print(variant, st, "keys", len(want.table), "shifts", sorted(set(want.shifts)))
    for name in ("mates", "deletions", "insertions", "complex_gaps", "long_insertions", "nonbase_insertions"):
        assert st[name] >= 1, name
    assert max(want.shifts) > 0


# ---------------------------------------------------------------------------
# 3. invariances
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    rng, genes = _panel(93, 17, 4)
    genes = _runs(genes)
    reads = _haplotype_reads(rng, genes, 40)
    b = spliced_reads(rng, genes, 100, sub=0.02)
    m1 = [b["seq1"][int(b["off1"][i]):int(b["off1"][i + 1])] for i in range(100)] + reads
    m2 = [b["seq2"][int(b["off2"][i]):int(b["off2"][i + 1])] for i in range(100)] + [synth.revcomp(np.asarray(r)) for r in reads]
    return genes, m1, m2


def _sub_batch(m1, m2, idx):
    return synth.batch_from_lists([m1[i] for i in idx], [m2[i] for i in idx])


def test_batches_of_1_7_and_64_and_the_four_families(oracle, sample):
    genes, m1, m2 = sample
    n = len(m1)
    o, h, sm = build_kb(oracle, [g for g, _ in genes], k=17)
    want = Want(sm, 8)
    h.indels_enable(8, 20, 4096)
    whole = _sub_batch(m1, m2, range(n))
    goff, gids = h.classify(*_args(whole))
    want.add(o, whole, goff, gids)
    one = want.check(h).copy()
    stats = h.indels_stats()
    assert len(one) >= 8 and stats["deletions"] >= 20 and stats["insertions"] >= 20
    for size in (7, 64, 1):
        h.indels_reset()
        assert len(h.indels_get()) == 0 and not any(h.indels_stats().values())
        for a in range(0, n, size):
            h.classify(*_args(_sub_batch(m1, m2, range(a, min(a + size, n)))))
        assert h.indels_get().tobytes() == one.tobytes() and h.indels_stats() == stats, size
    # the four families, one after the other into one table: host, host by ticket, resident, resident by ticket
    h.indels_reset()
    want.reset()
    h.classify(*_args(whole))
    h.wait(h.submit(*_args(whole)))
    t = _to_device(whole)
    r = h.classify_device(n, max_read_len=120, **_dev_ptrs(t))
    g3, i3 = device_assoc(r)
    assert np.array_equal(g3, goff) and np.array_equal(i3, gids)
    h.wait_device(h.submit_device(n, max_read_len=120, **_dev_ptrs(t)))
    want.add(o, whole, goff, gids, times=4)
    want.check(h)


def _everything(h, batch):
    """every other mode's records and states and the kernel's name for one host batch"""
    goff, gids = h.classify(*_args(batch))
    out = {"goff": goff.tobytes(), "gids": gids.tobytes(), "kernel": h.last_kernel(), "placement": h.placement_last().tobytes(),
           "segments": [a.tobytes() for a in h.segments_last()], "alignments": h.alignments_last().tobytes(), "pairs": h.pairs_last().tobytes(),
           "rescue": h.rescue_last().tobytes(), "depth": h.depth_all().tobytes(), "junctions": h.junctions_get().tobytes(),
           "pileup": h.pileup_all().tobytes(), "fragments": [np.asarray(a).tobytes() for a in h.fragments(64)],
           "gene_counts": np.asarray(h.gene_counts()).tobytes()}
    return out


def test_every_other_mode_is_the_same_with_the_mode_on_and_off(oracle, sample):
    genes, m1, m2 = sample
    batch = _sub_batch(m1, m2, range(len(m1)))
    seen = []
    for on in (False, True):
        o, h, sm = build_kb(oracle, [g for g, _ in genes], k=17)
        h.placement_enable(True)
        h.segments_enable(3)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        h.pileup_enable_aligned(8)
        h.alignments_enable(8)
        h.pairs_enable(20, 1000, 64)
        h.rescue_enable(20, 1000, 8, 4)
        if on:
            h.indels_enable(8, 20, 1024)
        seen.append(_everything(h, batch))
        if on:
            assert len(h.indels_get()) >= 8
    assert seen[0].keys() == seen[1].keys()
    for name in seen[0]:
        assert seen[0][name] == seen[1][name], name


def test_alignments_mode_at_the_same_floor_at_another_floor_and_off(oracle, sample):
    genes, m1, m2 = sample
    batch = _sub_batch(m1, m2, range(len(m1)))
    o, h, sm = build_kb(oracle, [g for g, _ in genes], k=17)
    want = Want(sm, 8)
    h.indels_enable(8, 20, 1024)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    base = want.check(h).copy()
    stats = h.indels_stats()
    for floor in (8, 3, 20):
        h.indels_reset()
        h.alignments_enable(floor)
        h.classify(*_args(batch))
        # alignments mode hands out its own floor's records whatever this mode reads
        rows = expected_segments(sm, batch, goff, gids, 4)[1]
        assert h.alignments_last().tobytes() == expected_alignments(sm, batch, goff, gids, rows, floor).tobytes()
        assert h.indels_get().tobytes() == base.tobytes() and h.indels_stats() == stats
    # rescue mode behind a shared launch: a rescued mate's one block is no gap and is not examined
    h.indels_reset()
    h.alignments_enable(8)
    h.pairs_enable(20, 1000, 64)
    h.rescue_enable(20, 1000, 8, 4)
    h.classify(*_args(batch))
    assert h.indels_get().tobytes() == base.tobytes() and h.indels_stats() == stats
    # another floor of this mode's own is another table
    h.rescue_enable(0, 0, 0, 0)
    h.pairs_enable(0, 0, 0)
    h.indels_reset()
    h.indels_enable(12, 20, 1024)
    want = Want(sm, 12)
    want.add(o, batch, *h.classify(*_args(batch)))
    want.check(h)


# ---------------------------------------------------------------------------
# 4. counts, probe chains, a full table
# ---------------------------------------------------------------------------
def test_several_hundred_observations_of_one_key(oracle):
    _, rec, mates, key = hand_cases(step=1)[0]
    o, h, sm = build_kb(oracle, [rec], k=17)
    want = Want(sm, 8)
    h.indels_enable(8, 20, 64)
    batch = synth.batch_from_lists(mates * 8)
    want.add(o, batch, *h.classify(*_args(batch)))
    got = _keys(want.check(h))
    assert list(got) == [(0, key[0], 1, 12, _seq(key[3]))] and sum(list(got.values())[0]) >= 300


@pytest.fixture(scope="module")
def many_keys():
    """200 genes with two unique events each, ten error-free mates across either: a few hundred distinct keys"""
    rng = np.random.default_rng(97)
    genes, mates = [], []
    for g in range(200):
        rec = bytearray(synth.random_seq(rng, 300).tobytes())
        rec[99] = ord("A") if rec[99 + 4] != ord("A") else ord("C")
        ins = b"GT" + bytes([next(c for c in b"ACGT" if c != rec[199])])
        hap = bytes(rec[:100] + rec[104:200]) + ins + bytes(rec[200:])
        genes.append(bytes(rec))
        mates += tile(hap[40:170], 100, 6, g) + tile(hap[130:270], 100, 8, g)
    return genes, synth.batch_from_lists(mates)


def test_long_probe_chains(oracle, many_keys):
    genes, batch = many_keys
    o, h, sm = build_kb(oracle, genes, k=17)
    want = Want(sm, 8)
    h.indels_enable(8, 20, 1 << 16)
    want.add(o, batch, *h.classify(*_args(batch)))
    n_keys = len(want.table)
    capacity = 64
    while capacity < 2 * n_keys:
        capacity *= 2
    assert 300 <= n_keys
    want.check(h)
    h.indels_reset()
    h.indels_enable(8, 20, capacity)                # (another capacity: allowed on a table that was reset)
    h.classify(*_args(batch))
    h.classify(*_args(batch))
    for v in want.table.values():
        v[0] *= 2
        v[1] *= 2
    want.stats = {name: 2 * v for name, v in want.stats.items()}
    want.check(h)


def test_a_full_table_is_an_error_and_reset_recovers(oracle, many_keys):
    from shark_amd import SharkHipError
    genes, batch = many_keys
    o, h, sm = build_kb(oracle, genes, k=17)
    want = Want(sm, 8)
    h.indels_enable(8, 20, 64)
    want.add(o, batch, *h.classify(*_args(batch)))
    assert len(want.table) > 64
    for _ in range(2):
        with pytest.raises(SharkHipError, match="full"):
            h.indels_get()
    st = h.indels_stats()
    assert st["dropped"] > 0 and st["deletions"] == want.stats["deletions"] and st["insertions"] == want.stats["insertions"]
    h.indels_reset()
    assert len(h.indels_get()) == 0
    small = synth.batch_from_lists([batch["seq1"][int(batch["off1"][i]):int(batch["off1"][i + 1])] for i in range(60)])
    want.reset()
    want.add(o, small, *h.classify(*_args(small)))
    assert 1 <= len(want.check(h)) <= 64


# ---------------------------------------------------------------------------
# 5. shk_indels_add
# ---------------------------------------------------------------------------
def test_two_contexts_summed_equal_one_over_all_reads(oracle, sample):
    from shark_amd import SharkHipError
    genes, m1, m2 = sample
    n = len(m1)
    halves = [_sub_batch(m1, m2, range(0, n, 2)), _sub_batch(m1, m2, range(1, n, 2))]
    ctx = []
    for b in halves:
        o, h, sm = build_kb(oracle, [g for g, _ in genes], k=17)
        h.indels_enable(8, 20, 1024)
        h.classify(*_args(b))
        ctx.append(h)
    o, one, sm = build_kb(oracle, [g for g, _ in genes], k=17)
    one.indels_enable(8, 20, 1024)
    for b in halves:
        one.classify(*_args(b))
    a, b = ctx
    a.indels_add(b.indels_get(), b.indels_stats())
    assert a.indels_get().tobytes() == one.indels_get().tobytes() and a.indels_stats() == one.indels_stats()
    assert len(a.indels_get()) > max(len(b.indels_get()), 4)
    # entries alone, and nothing at all
    before = a.indels_get().copy()
    a.indels_add(before)
    twice = a.indels_get()
    assert np.array_equal(twice["fwd"], 2 * before["fwd"]) and np.array_equal(twice["rev"], 2 * before["rev"]) and a.indels_stats() == one.indels_stats()
    a.indels_add(before[:0])
    # invalid entries are refused, with the entry's number, and nothing is added
    lengths = [len(g) for g, _ in genes]
    ok = before[:3].copy()
    for field, value in (("gene", len(genes)), ("x", lengths[int(ok[1]["gene"])]), ("kind", 2), ("len", 0), ("reserved", 1), ("seq", 1 << 24)):
        bad = ok.copy()
        bad[1][field] = value
        assert not check_entry(bad[1], lengths)
        with pytest.raises(SharkHipError, match="shk_indels_add: entry 1 "):
            a.indels_add(bad)
    assert all(check_entry(e, lengths) for e in before)
    assert a.indels_get().tobytes() == twice.tobytes()


# ---------------------------------------------------------------------------
# 6. state rules and texts
# ---------------------------------------------------------------------------
def test_state_rules_and_their_texts(oracle, sample):
    from shark_amd import SharkHip, SharkHipError
    genes, m1, m2 = sample
    records = [bytes(g) for g, _ in genes]
    b = _sub_batch(m1, m2, range(100, 140))
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError, match="shk_indels_enable: the index is not finalized"):
        h.indels_enable(8, 20, 64)
    h.indels_enable(0, 0, 0)                                                     # (off is always allowed)
    h.build(records, keep_positions=True)
    with pytest.raises(SharkHipError, match="shk_indels_enable: the index was finalized without shk_ref_keep_bases"):
        h.indels_enable(8, 20, 64)
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    h.build(records)
    with pytest.raises(SharkHipError, match="shk_indels_enable: the index was finalized without shk_ref_keep_positions"):
        h.indels_enable(8, 20, 64)
    o, h, sm = build_kb(oracle, records, k=17)
    for name, call in (("get", h.indels_get), ("stats", h.indels_stats), ("reset", h.indels_reset), ("add", lambda: h.indels_add(np.zeros(0, capi.INDEL_DTYPE)))):
        with pytest.raises(SharkHipError, match="shk_indels_%s: indels mode was never enabled on this context" % name):
            call()
    for min_intron in (0, 65536):
        with pytest.raises(SharkHipError, match="shk_indels_enable: min_intron is 1 .. 65535"):
            h.indels_enable(8, min_intron, 64)
    h.indels_enable(8, 20, 100)                                                  # (rounded up to 128)
    h.indels_enable(8, 20, 128)
    h.indels_enable(8, 30, 64)                                                   # (nothing submitted yet: allocated anew, another min_intron)
    h.indels_enable(8, 20, 64)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError, match=r"shk_indels_enable: another capacity than the table's \(shk_indels_reset first\)"):
        h.indels_enable(8, 20, 128)
    with pytest.raises(SharkHipError, match=r"shk_indels_enable: another min_intron than the table's \(shk_indels_reset first\)"):
        h.indels_enable(8, 21, 64)
    h.indels_enable(8, 20, 33)                                                   # (the same capacity after rounding)
    h.indels_enable(0, 0, 0)                                                     # (off: the arguments are ignored, the table stays)
    kept = h.indels_get().copy()
    h.classify(*_args(b))
    assert len(kept) >= 3 and h.indels_get().tobytes() == kept.tobytes()
    h.indels_enable(8, 20, 64)
    tk = h.submit(*_args(b))
    for name, call in (("enable", lambda: h.indels_enable(8, 20, 64)), ("enable", lambda: h.indels_enable(0, 0, 0)), ("get", h.indels_get),
                       ("stats", h.indels_stats), ("reset", h.indels_reset), ("add", lambda: h.indels_add(kept))):
        with pytest.raises(SharkHipError, match=r"shk_indels_%s: tickets are outstanding \(wait for them first\)" % name):
            call()
    h.wait(tk)
    twice = h.indels_get()
    assert np.array_equal(twice["fwd"], 2 * kept["fwd"]) and np.array_equal(twice["rev"], 2 * kept["rev"])
    # shk_count_work's batch and a wrongly vouched batch are not counted
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(40, p["seq1"], p["off1"], p["seq2"], p["off2"])
    tk = h.submit_device(40, max_read_len=120, uniform_len1=99, uniform_len2=99, **p)
    with pytest.raises(SharkHipError):
        h.wait_device(tk)
    assert h.indels_get().tobytes() == twice.tobytes()
    # after a reset both may change
    h.indels_reset()
    h.indels_enable(8, 21, 256)
    want = Want(sm, 8, 21)
    want.add(o, b, *h.classify(*_args(b)))
    want.check(h)
    wide = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    wide.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_positions=True)
    with pytest.raises(SharkHipError, match="65 536"):
        wide.indels_enable(8, 20, 64)


# ---------------------------------------------------------------------------
# 7. the command
# ---------------------------------------------------------------------------
def _model_lines(oracle, fa, batch, c, min_mates, s_min=8, min_intron=20):
    """the lines of `shark --indels` by the oracle's associations and the model chain"""
    o = oracle.Shark(k=17, c=c, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    goff, gids = o.classify(*_args(batch))
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    recs = expected_alignments(sm, batch, goff, gids, rows, s_min)
    table, stats = expected_indels(recs, batch, goff, gids, sm.records, min_intron)
    return indel_lines(table_array(table, min_mates), [n.decode() for n, _ in fa]), stats


def _write_sample(tmp_path, genes, batch):
    (tmp_path / "g.fa").write_text("".join(">g%d\n%s\n" % (i, bytes(g).decode()) for i, g in enumerate(genes)))
    paired = batch["seq2"] is not None
    for name, seq, off in (("1.fq", batch["seq1"], batch["off1"]),) + ((("2.fq", batch["seq2"], batch["off2"]),) if paired else ()):
        with open(tmp_path / name, "w") as f:
            for i in range(len(off) - 1):
                s = bytes(seq[int(off[i]):int(off[i + 1])]).decode()
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    return ["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq")] + (["-2", str(tmp_path / "2.fq")] if paired else []) + \
        ["-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]


def test_shark_indels_on_the_example_and_on_a_synthetic_sample(oracle, example_dir, sample, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq"), "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    genes, m1, m2 = sample
    syn_batch = _sub_batch(m1, m2, range(len(m1)))
    syn = _write_sample(tmp_path, [g for g, _ in genes], syn_batch) + ["-c", "0.3"]
    syn_fa = [(b"g%d" % i, bytes(g)) for i, (g, _) in enumerate(genes)]
    for tag, args, want in (("ex", base + ["--indels-min-mates", "1"], _model_lines(oracle, fa, batch, 0.6, 1)),
                            ("syn", syn, _model_lines(oracle, syn_fa, syn_batch, 0.3, 2))):
        lines, stats = want
        print(tag, "lines", len(lines), stats)
        r = run_shark(args + ["--indels", str(tmp_path / (tag + ".a"))], str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        plain = (tmp_path / (tag + ".a")).read_bytes()
        assert plain.decode().split("\n")[:-1] == lines
        assert ("Indels: %d aligned mates, %d deletions, %d insertions" % (stats["mates"], stats["deletions"], stats["insertions"])).encode() in r.stderr
        for n, extra in enumerate((["--gpus", "2", "--devices", "0,0", "--batch", "700"], ["--batch", "64", "--sam", str(tmp_path / "x.sam")],
                                   ["--gpus", "3", "--devices", "0,0,0", "--batch", "50", "--indels-capacity", "64"])):
            r = run_shark(args + ["--indels", str(tmp_path / ("%s.%d" % (tag, n)))] + extra, str(tmp_path))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            assert (tmp_path / ("%s.%d" % (tag, n))).read_bytes() == plain
    assert len(_model_lines(oracle, syn_fa, syn_batch, 0.3, 2)[0]) >= 5


def test_shark_indels_with_a_table_too_small_and_the_usage_errors(oracle, many_keys, tmp_path):
    genes, batch = many_keys
    syn = _write_sample(tmp_path, genes, batch) + ["-c", "0.3"]
    r = run_shark(syn + ["--indels", str(tmp_path / "full"), "--indels-capacity", "64"], str(tmp_path))
    assert r.returncode == 1 and b"--indels-capacity" in r.stderr and (tmp_path / "full").read_bytes() == b""
    # two workers whose tables fit one by one, but not their sum in worker 0's
    r = run_shark(syn + ["--indels", str(tmp_path / "sum"), "--indels-capacity", "256", "--gpus", "2", "--devices", "0,0", "--batch", "100"], str(tmp_path))
    assert r.returncode == 1 and b"--indels-capacity" in r.stderr and (tmp_path / "sum").read_bytes() == b""
    r = run_shark(syn + ["--indels", str(tmp_path / "ok"), "--indels-capacity", "1024"], str(tmp_path))
    assert r.returncode == 0 and (tmp_path / "ok").read_bytes().count(b"\n") == 400
    for flags in (["--indels-min-support", "8"], ["--indels-min-intron", "20"], ["--indels-min-mates", "2"], ["--indels-capacity", "64"]):
        r = run_shark(syn + flags, str(tmp_path))
        assert r.returncode == 1 and b"need --indels FILE" in r.stderr
    for flags, text in ((["--indels-min-support", "0"], b"--indels-min-support must be at least 1"), (["--indels-min-intron", "0"], b"--indels-min-intron must be 1 to 65535"),
                        (["--indels-min-intron", "65536"], b"--indels-min-intron must be 1 to 65535"), (["--indels-capacity", "0"], b"--indels-capacity must be in the range")):
        r = run_shark(syn + ["--indels", str(tmp_path / "u")] + flags, str(tmp_path))
        assert r.returncode == 1 and text in r.stderr
    # --extend-ends alone with --indels is accepted (the final blocks are the input)
    r = run_shark(syn + ["--indels", str(tmp_path / "ext"), "--extend-ends"], str(tmp_path))
    assert r.returncode == 0 and (tmp_path / "ext").read_bytes().count(b"\n") == 400


def test_shark_indels_honours_extend_ends_and_splice_junctions(oracle, tmp_path):
    """the command's table under --extend-ends and --splice-junctions is the model's over the final blocks with steps 3b and 3a on.
    Step 3a moves a mate's outer ends only and can make no gap; step 3b can: a fourth gene lists a 15-base intron, and the mates that
    cross it with 6 to 8 bases are a clip without the list and a deletion of 15 bases (below --indels-min-intron) with it"""
    rng, plain_genes = _panel(91, 17)
    genes = _runs(plain_genes)
    short = synth.random_seq(rng, 300)
    short[150] = ord("A") if short[165] != ord("A") else ord("C")
    records = [g for g, _ in genes] + [short]
    sites = sorted([(g, d, a) for g, (rec, tr) in enumerate(plain_genes) for d, a in _introns(bytes(rec), bytes(tr))] + [(3, 150, 165)])
    b1 = spliced_reads(rng, genes, 150, sub=0.03)
    m1 = [b1["seq1"][int(b1["off1"][i]):int(b1["off1"][i + 1])] for i in range(150)] + _haplotype_reads(rng, genes, 80)
    tr = np.concatenate([short[:150], short[165:]])
    m1 += [m if i & 1 else synth.revcomp(m) for i in range(12) for m in [tr[66 + i % 3:156 + i % 3]]]
    batch = synth.batch_from_lists(m1)
    syn = _write_sample(tmp_path, records, batch) + ["-c", "0.3"]
    (tmp_path / "sites.jn").write_text("".join("g%d %d %d %d 5\n" % (g, d, a, a - d) for g, d, a in sites))
    o = oracle.Shark(k=17, c=0.3, bf_bits=1 << 33)
    o.build([bytes(g) for g in records])
    goff, gids = o.classify(*_args(batch))
    sm = SegmentsModel([bytes(g) for g in records], 17)
    legend = ["g%d" % i for i in range(len(records))]
    seen = {}
    for tag, flags, ext, spl in (("plain", [], (0, 0), (0, 0, 0)), ("ext", ["--extend-ends"], (4, 5), (0, 0, 0)),
                                 ("both", ["--extend-ends", "--splice-junctions", str(tmp_path / "sites.jn")], (4, 5), (3, 2, 2))):
        want = Want(sm, 8, ext=ext, sites=sites, splice=spl)
        want.add(o, batch, goff, gids)
        lines = indel_lines(table_array(want.table, 2), legend)
        r = run_shark(syn + ["--indels", str(tmp_path / tag)] + flags, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert (tmp_path / tag).read_bytes().decode().split("\n")[:-1] == lines, tag
        seen[tag] = (lines, dict(want.stats))
        print(tag, len(lines), want.stats)
    assert seen["plain"] == seen["ext"] and not any(l.startswith("g3 ") for l in seen["plain"][0])
    assert [l for l in seen["both"][0] if l.startswith("g3 ")] == ["g3 150 D 15 * 6 6"]
