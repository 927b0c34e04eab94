"""Variants mode on the GPU (shk_ref_keep_bases, shk_pileup_add, shk_variants_get, shk_variants_summary, `shark --variants`): the
record bases on the device, the sites and the per-gene summary -- whole arrays, byte for byte -- against the model
(tests/variants_model.py), which walks the positions one at a time in Python integers and shares no idea with the kernels.  States are
loaded with pileup_reset + pileup_add, so the call is driven at its edges without reads; one test goes end to end on reads, where the
pileup itself is checked against tests/pileup_model.py first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import synth
from tests.segments_model import SegmentsModel
from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_pileup import Want
from tests.test_gpu_segments import _args
from tests.test_variants_cpu import mutated_example_pileup, mutated_example_records
from tests.variants_model import DEFAULTS, expected_recbase, expected_summary, expected_variants, variant_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = (1 << 32) - 1
# the sizes the implementation steps in (variants.hip, device_scan.hpp): positions per lane, per wavefront, per workgroup, and per tile
# of the scan over the wavefronts' counts (4 096 wavefronts)
LANE, WAVE, BLOCK, SCAN_TILE = 4, 256, 1024, 4096 * 256
PARAM_SETS = (DEFAULTS, (1, 1, 0, 1), (10, 2, 1, 2), (3, 3, 65535, 65535), (20, 1, 3, 7))


def build_kb(oracle, records, keep_bases=True, **kw):
    """(oracle index, context, model) over the same records; the context keeps the record bases"""
    from shark_amd import SharkHip
    kw.setdefault("c", 0.0)
    kw.setdefault("bf_bits", 1 << 26)
    k = kw.setdefault("k", 17)
    o = oracle.Shark(k=k, c=kw["c"], bf_bits=kw["bf_bits"], min_quality=kw.get("min_quality", 0))
    nidx = o.build([bytes(g) for g in records])
    h = SharkHip(**kw)
    assert h.build([bytes(g) for g in records], keep_positions=not keep_bases, keep_bases=keep_bases)["nidx"] == nidx   # (keep_bases implies keep_positions)
    return o, h, SegmentsModel([bytes(g) for g in records], k)


def record(rng, n, others=0.05):
    """n >= 1 random bases, a share of them lower case, N or another byte"""
    r = synth.random_seq(rng, n)
    u = rng.random(n)
    u[[0, -1]] = 1.0                                            # (the first and the last base stay plain bases)
    r[u < others] |= 0x20
    r[u < others / 2] = ord("N")
    r[u < others / 8] = ord("-")
    return r


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        i = next(i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError("record %d: got %s, model %s" % (i, got[i], want[i]))


def check_calls(h, sm, counts, param_sets=PARAM_SETS):
    """the sites and the summary of the state `counts` (already loaded) at every parameter set, against the model"""
    gs = h.depth_layout()
    n_sites = []
    for prm in param_sets:
        want = expected_variants(counts, sm.records, gs, prm)
        same(h.variants(prm[0], prm[1], (prm[2], prm[3])), want)
        same(h.variants_summary(prm[0], prm[1], (prm[2], prm[3])), expected_summary(counts, sm.records, gs, prm))
        n_sites.append(len(want))
    return n_sites


def load(h, counts, mates=M32):
    h.pileup_reset()
    h.pileup_add(counts, mates)
    assert np.array_equal(h.pileup_all(), counts) and h.pileup_mates() == mates


# count rows relative to the record's base: (n[r], then the three other bases in ascending order), chosen so that every edge of
# tests/test_variants_cpu.py's list occurs at DEFAULTS (8, 3, 1/5) and at (20, 1, 3/7)
TEMPLATES = (
    (0, 0, 0, 0), (12, 5, 0, 0), (14, 3, 0, 0),
    (16, 4, 0, 0), (17, 4, 0, 0), (16, 3, 0, 0), (15, 4, 0, 0),                 # n[alt] * 5 == T, and one observation either side
    (8, 6, 0, 0), (9, 6, 0, 0), (8, 0, 6, 6), (12, 9, 0, 0), (12, 0, 0, 8),     # 3/7 at its edge (T = 14, 21), one either side
    (4, 4, 0, 0), (3, 4, 0, 0), (5, 0, 0, 3), (5, 0, 2, 0), (6, 0, 2, 0),       # T == min_depth, min_depth - 1; n[alt] == min_alt, min_alt - 1
    (9, 4, 4, 4), (0, 4, 9, 9), (10, 3, 6, 5), (0, 0, 7, 7), (3, 5, 5, 2),      # ties to the smaller base; multi-allelic
    (M32, M32, M32, M32), (M32, M32, 0, 0), (M32, 0, M32 - 1, 0), (0, 0, 0, M32),
    (19, 1, 0, 0), (20, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0),
)
SITE_ROW = (0, 0, 0, 30)       # a site at every parameter set above, whatever the record's base


def crafted(rng, recbase):
    """a state over recbase: per position a template (mapped onto the record's base) or small random counts"""
    n = len(recbase)
    counts = rng.integers(0, 13, size=(n, 4), dtype=np.uint32)
    pick = rng.integers(0, 2 * len(TEMPLATES), size=n)
    for x in np.nonzero(pick < len(TEMPLATES))[0]:
        t = TEMPLATES[pick[x]]
        r = int(recbase[x]) & 3                                          # (a position without a base gets the row as it is)
        others = [b for b in range(4) if b != r]
        counts[x, r] = t[0]
        counts[x, others] = t[1:]
    return counts


def site_at(counts, recbase, x):
    r = int(recbase[x])
    assert r < 4, "position %d holds no base" % x
    counts[x] = 0
    counts[x, r] = SITE_ROW[0]
    counts[x, [b for b in range(4) if b != r][-1]] = SITE_ROW[3]


# ---------------------------------------------------------------------------
# 1. the record bases
# ---------------------------------------------------------------------------
def test_recbase_lengths_cases_and_the_numbering_quirk(oracle):
    """records of 0, 1, 3, 4 bases (below k = 5: their ids carry nothing), 5, 255, 256 and 257; lower case, N and other bytes; an all-N
    record, which does not advance the gene counter"""
    rng = np.random.default_rng(5)
    records = [record(rng, 5, 0.0), np.zeros(0, np.uint8), record(rng, 255, 0.3), record(rng, 1), np.full(60, ord("N"), np.uint8), record(rng, 3),
               record(rng, 256, 0.3), record(rng, 4), record(rng, 257, 0.3), np.frombuffer(b"acgtNnRryACGT-*\x01\xffACGTA", np.uint8)]
    o, h, sm = build_kb(oracle, records, k=5)
    assert sorted(sm.records) == [0, 2, 5, 7, 8] and h.index_info()["nidx"] == 9
    gs = h.depth_layout()
    total = int(gs[-1])
    assert total == 5 + 255 + 256 + 257 + 22
    got = h.debug_index_array("recbase")
    want = expected_recbase(sm.records)
    assert got.dtype == np.uint8 and len(got) % 4 == 0 and len(got) >= (total + 3) // 4 * 4 + 4      # (an aligned dword behind the end)
    assert np.array_equal(got[:total], want) and (got[total:] == 4).all()
    assert want[-22:].tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4, 0, 1, 2, 3, 4, 4, 4, 4, 0, 1, 2, 3, 0] and (want[:5] < 4).all()
    # without keep_bases: no array, and the calls say so while pileup works
    o2, h2, _ = build_kb(oracle, records, keep_bases=False, k=5)
    assert len(h2.debug_index_array("recbase")) == 0 and np.array_equal(h2.depth_layout(), gs)
    from shark_amd import SharkHip
    h3 = SharkHip(k=5, c=0.0, bf_bits=1 << 26)
    h3.build([bytes(r) for r in records])
    assert len(h3.debug_index_array("recbase")) == 0


# ---------------------------------------------------------------------------
# 2. the call on crafted states
# ---------------------------------------------------------------------------
SHORT = b"AC"      # a record below k = 5: its id has no base -- a zero-length gene
# record lengths per layout (k = 5; 0 stands for SHORT); the totals run around a lane's 4 positions, a wavefront's 256 and a workgroup's
# 1 024 and 4 096; gene boundaries fall inside a lane's four positions (5 | 250: base 5 is lane 1's second) and inside a wavefront
LAYOUTS = {5: [5], 255: [255], 256: [5, 0, 245, 0, 0, 6], 257: [257], 4095: [1021, 0, 3074], 4096: [1000, 0, 0, 3096], 4097: [4097],
           1289: [7, 0, 250, 0, 0, 513, 6, 5, 508]}


@pytest.mark.parametrize("total", sorted(LAYOUTS))
def test_crafted_states_over_small_layouts(oracle, total):
    rng = np.random.default_rng(total)
    lengths = LAYOUTS[total]
    records = [np.frombuffer(SHORT, np.uint8) if n == 0 else record(rng, n, 0.0 if n < 8 else 0.05) for n in lengths]
    o, h, sm = build_kb(oracle, records, k=5)
    gs = h.depth_layout()
    assert int(gs[-1]) == total == sum(lengths) and np.array_equal(np.diff(gs), lengths)
    recbase = expected_recbase(sm.records)
    assert np.array_equal(h.debug_index_array("recbase")[:total], recbase)
    h.pileup_enable(1)
    h.pileup_enable(0)                                        # (the state exists; the mode may be off)
    counts = crafted(rng, recbase)
    # sites at the first and the last base of every gene, hence of the array
    for g in range(len(gs) - 1):
        if gs[g + 1] > gs[g]:
            for x in (int(gs[g]), int(gs[g + 1]) - 1):
                if recbase[x] < 4:
                    site_at(counts, recbase, x)
    load(h, counts)
    n_sites = check_calls(h, sm, counts)
    first = h.variants()
    assert (int(first[0]["gene"]), int(first[0]["x"])) == (0, 0) and int(first[-1]["gene"]) == len(lengths) - 1 and int(first[-1]["x"]) == lengths[-1] - 1
    assert min(n_sites) >= 2
    # nothing, and everything
    load(h, np.zeros_like(counts), 0)
    assert check_calls(h, sm, np.zeros_like(counts), (DEFAULTS,)) == [0]
    full = np.full_like(counts, M32)
    load(h, full)
    assert check_calls(h, sm, full, ((M32, M32, 1, 4), (M32, M32, 16385, 65535))) == [int((recbase < 4).sum()), 0]


@pytest.mark.parametrize("lengths", [[1], [3], [1, 0, 3], [2, 2, 1]])
def test_crafted_states_over_tiny_layouts(oracle, lengths):
    """totals of 1, 3, 4 and 5 bases: k = 1, so that a record of one base carries an id (0: an empty record, a zero-length gene)"""
    rng = np.random.default_rng(sum(lengths))
    records = [synth.random_seq(rng, n) for n in lengths]
    o, h, sm = build_kb(oracle, records, k=1)
    gs = h.depth_layout()
    assert np.array_equal(np.diff(gs), lengths)
    recbase = expected_recbase(sm.records)
    got = h.debug_index_array("recbase")
    assert np.array_equal(got[:len(recbase)], recbase) and (got[len(recbase):] == 4).all() and len(got) % 4 == 0 and len(got) > len(recbase)
    h.pileup_enable(1)
    for trial in range(3):
        counts = crafted(rng, recbase)
        site_at(counts, recbase, 0)
        site_at(counts, recbase, len(recbase) - 1)
        load(h, counts)
        assert min(check_calls(h, sm, counts)) >= 1


def test_a_layout_that_crosses_every_tile_size_and_the_caps(oracle):
    """just over 2^20 bases in four records and a zero-length gene: more than 4 096 wavefronts, so the scan over their counts runs over
    two tiles; a wavefront in which all 256 positions are sites, one with none; sites either side of every boundary; cap == n - 1,
    cap == n, out == NULL.  Nine in ten of the record bytes are N (no part in anything), which keeps the model's walk short"""
    rng = np.random.default_rng(2 ** 20)
    lengths = [300001, 0, 500003, 248563, 137]
    assert sum(lengths) == SCAN_TILE + 128
    records = []
    for n in lengths:
        if n == 0:
            records.append(np.frombuffer(SHORT, np.uint8))
            continue
        r = synth.random_seq(rng, n)
        r[rng.random(n) < 0.9] = ord("N")
        r[:8] = synth.random_seq(rng, 8)
        r[-8:] = synth.random_seq(rng, 8)
        records.append(r)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    flat = np.concatenate(records[:1] + records[2:])
    # (whole wavefronts of bases: 700 holds sites only, 701 none, 4095 and 4096 lie either side of the scan's tile)
    for w in (700, 701, 4095, 4096):
        lo, hi = w * WAVE, min((w + 1) * WAVE + 4, len(flat))
        flat[lo:hi] = synth.random_seq(rng, hi - lo)
    at = 0
    for i, n in enumerate(lengths):
        if n:
            records[i] = flat[at:at + n]
            at += n
    o, h, sm = build_kb(oracle, records, k=5)
    gs = h.depth_layout()
    total = int(gs[-1])
    assert np.array_equal(gs, starts) and total == SCAN_TILE + 128
    recbase = expected_recbase(sm.records)
    assert np.array_equal(h.debug_index_array("recbase")[:total], recbase)
    counts = crafted(rng, recbase)
    counts[recbase == 4] = rng.integers(0, 40, size=(int((recbase == 4).sum()), 4), dtype=np.uint32)   # (what a position without a base holds is ignored)
    for x in range(700 * WAVE, 701 * WAVE):
        site_at(counts, recbase, x)
    counts[701 * WAVE:702 * WAVE] = 0
    edges = [0, total - 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 3, SCAN_TILE + 4, 4095 * WAVE, 4096 * WAVE - LANE, BLOCK * 300 - 1, BLOCK * 300]
    edges += [int(s) - d for s in starts[1:] for d in (1, 0) if 0 <= int(s) - d < total]
    for x in edges:
        if recbase[x] < 4:
            site_at(counts, recbase, x)
    h.pileup_enable(1)
    load(h, counts)
    want = expected_variants(counts, sm.records, gs, DEFAULTS)
    got = h.variants()
    same(got, want)
    same(h.variants_summary(), expected_summary(counts, sm.records, gs, DEFAULTS))
    flatx = gs[want["gene"]] + want["x"]
    assert int(((flatx >= 700 * WAVE) & (flatx < 701 * WAVE)).sum()) == WAVE and not ((flatx >= 701 * WAVE) & (flatx < 702 * WAVE)).any()
    assert {0, total - 1, SCAN_TILE - 1, SCAN_TILE} <= set(int(v) for v in flatx) and len(want) > 5000
    assert set(int(g) for g in want["gene"]) == {0, 2, 3, 4}
    # the caps, at the C ABI
    prm = capi.ShkVariantParams(*DEFAULTS)
    n = C.c_uint64(12345)
    assert h.L.shk_variants_get(h.h, C.byref(prm), None, 0, C.byref(n)) == 0 and n.value == len(want)
    out = np.zeros(len(want), dtype=capi.VARIANT_DTYPE)
    n = C.c_uint64(0)
    assert h.L.shk_variants_get(h.h, C.byref(prm), capi._ptr(out), len(want) - 1, C.byref(n)) == -1 and n.value == len(want) and not out.view(np.uint32).any()
    assert h.L.shk_variants_get(h.h, C.byref(prm), capi._ptr(out), len(want), C.byref(n)) == 0 and n.value == len(want)
    same(out, want)
    # a second parameter set over the same scratch memory: fewer sites, then more
    for prm2 in ((20, 1, 3, 7), (1, 1, 0, 1)):
        same(h.variants(prm2[0], prm2[1], prm2[2:]), expected_variants(counts, sm.records, gs, prm2))


# ---------------------------------------------------------------------------
# 3. shk_pileup_add
# ---------------------------------------------------------------------------
# pairs per batch, and the thresholds the planted positions are called at: the command's defaults, and lower ones at k = 31, where nearly
# all the depth over a substituted base comes from the generator's unspliced mates (one in ten)
E2E_READS = {5: 150, 17: 150, 31: 300}
E2E_PARAMS = {5: DEFAULTS, 17: DEFAULTS, 31: (3, 2, 1, 5)}


def e2e_case(k, seed, n=None):
    """genes, their records with planted substitutions, the planted positions (flat, gene after gene) and a batch of reads drawn from the
    UNMUTATED genes.  Per gene one substitution in each outer exon (70 bases), 31 to 38 bases from the exon's start -- a window of k <= 31
    votes on either side of it there, so a mate that lies over the exon keeps the base inside its span --, and four anywhere (one at
    k = 31, where a substitution silences 31 windows and two in one exon silence the exon)"""
    n = n or E2E_READS[k]
    rng = np.random.default_rng(seed)
    genes = [spliced_gene(rng, 1 + i, k) for i in range(3)]
    mutated, planted, at = [], [], 0
    for rec, _ in genes:
        m = rec.copy()
        xs = {31 + int(rng.integers(0, 8)), len(rec) - 70 + 31 + int(rng.integers(0, 8))}
        while len(xs) < (6 if k < 31 else 3):
            xs.add(int(rng.integers(0, len(rec))))
        for x in sorted(xs):
            m[x] = synth.ACGT[(int(np.searchsorted(synth.ACGT, m[x])) + 1 + int(rng.integers(0, 3))) % 4]
            planted.append(at + x)
        mutated.append(m)
        at += len(rec)
    batch = spliced_reads(rng, genes, n, sub=0.01)
    return genes, mutated, planted, batch


def test_pileup_add_host_device_and_two_contexts(oracle):
    from shark_amd import SharkHipError
    genes, mutated, planted, batch = e2e_case(17, 1)
    o, h, sm = build_kb(oracle, mutated, k=17)
    o2, h2, _ = build_kb(oracle, mutated, k=17)
    rng = np.random.default_rng(3)
    total = int(h.depth_layout()[-1])
    a = rng.integers(0, 1 << 32, size=(total, 4), dtype=np.uint32)
    b = rng.integers(0, 1000, size=(total, 4), dtype=np.uint32)
    h.pileup_enable(8)
    # from the host onto an empty state, from the device onto a non-empty one (modulo 2^32, element by element), the mate counter
    h.pileup_add(a, 5)
    assert np.array_equal(h.pileup_all(), a) and h.pileup_mates() == 5
    t = torch.from_numpy(b.view(np.int32)).to("cuda:0")
    h.pileup_add(None, 7, device_ptr=t.data_ptr())
    assert np.array_equal(h.pileup_all(), a + b) and h.pileup_mates() == 12
    h.pileup_add(b.reshape(-1), 0)                             # (flat, and no mates)
    assert np.array_equal(h.pileup_all(), a + b + b) and h.pileup_mates() == 12
    # wrong sizes
    for bad in (b[:-1], np.zeros((total + 1, 4), np.uint32), np.zeros(0, np.uint32)):
        with pytest.raises(SharkHipError):
            h.pileup_add(bad, 1)
    assert h.L.shk_pileup_add(h.h, None, 4 * total, 1, 0) == -1
    assert h.L.shk_pileup_add(h.h, C.c_void_p(t.data_ptr() + 4), 4 * total, 1, 1) == -1      # (a device pointer that is not 16-byte aligned)
    assert np.array_equal(h.pileup_all(), a + b + b) and h.pileup_mates() == 12
    # two contexts' accumulated states merged: the halves of a batch in two contexts sum to the whole batch in one
    h.pileup_reset()
    h2.pileup_enable(8)
    n = len(batch["off1"]) - 1
    halves = [synth.batch_from_lists([batch["seq1"][int(batch["off1"][i]):int(batch["off1"][i + 1])] for i in idx],
                                     [batch["seq2"][int(batch["off2"][i]):int(batch["off2"][i + 1])] for i in idx]) for idx in (range(0, n // 2), range(n // 2, n))]
    want = Want(sm, 8)
    want.add(o, halves[0], *h.classify(*_args(halves[0])))
    want.add(o, halves[1], *h2.classify(*_args(halves[1])))
    m2 = h2.pileup_mates()
    assert m2 > 0 and h.pileup_mates() > 0
    t = torch.zeros((total, 4), dtype=torch.int32, device="cuda:0")
    h2.pileup_all(device_ptr=t.data_ptr())
    h.pileup_add(None, m2, device_ptr=t.data_ptr())
    got = want.check(h)
    whole = Want(sm, 8)
    h2.pileup_reset()
    whole.add(o, batch, *h2.classify(*_args(batch)))
    assert np.array_equal(whole.check(h2), got) and whole.mates == want.mates
    same(h.variants(), h2.variants())
    # the guard trips when the sum of the mates passes 2^32 - 1, for every read-out, and reset clears it
    h.pileup_add(np.zeros((total, 4), np.uint32), M32 - want.mates)
    assert h.pileup_mates() == M32 and len(h.variants()) == len(h2.variants())
    h.pileup_add(np.zeros((total, 4), np.uint32), 1)
    for call in (h.pileup_all, h.variants, h.variants_summary):
        with pytest.raises(SharkHipError, match="2\\^32-1"):
            call()
    h.pileup_reset()
    assert h.pileup_mates() == 0 and len(h.variants()) == 0


# ---------------------------------------------------------------------------
# 4. end to end on reads
# ---------------------------------------------------------------------------
# The generator's seed per k: the first one (counting from 1) at which, by the models alone (tests/pileup_model.py, tests/variants_model.py
# on the CPU oracle's associations), at least 3 planted positions are called and at least one planted position is
# NOT called because fewer than min_depth mates show a base there (E2E_PARAMS).
SEEDS = {5: 1, 17: 1, 31: 1}


def planted_outcome(counts, sm, gs, planted, prm=DEFAULTS):
    """(called, too shallow): planted positions that are sites, and planted positions with T < min_depth"""
    v = expected_variants(counts, sm.records, gs, prm)
    sites = set(int(x) for x in gs[v["gene"]] + v["x"])
    return [x for x in planted if x in sites], [x for x in planted if int(counts[x].sum()) < prm[0]]


@pytest.mark.parametrize("k", [5, 17, 31])
def test_reads_against_records_with_planted_substitutions(oracle, k):
    genes, mutated, planted, batch = e2e_case(k, SEEDS[k])
    s_min = 3 if k == 5 else 8
    o, h, sm = build_kb(oracle, mutated, k=k)
    want = Want(sm, s_min)
    h.pileup_enable(s_min)
    want.add(o, batch, *h.classify(*_args(batch)))
    counts = want.check(h)                                     # the GPU's own pileup_all(), equal to the pileup model's
    gs = h.depth_layout()
    called, shallow = planted_outcome(counts, sm, gs, planted, E2E_PARAMS[k])
    print("k", k, "mates", want.mates, "planted", planted, "called", called, "too shallow", shallow)
    assert len(called) >= 3 and len(shallow) >= 1
    n_sites = check_calls(h, sm, counts, (E2E_PARAMS[k],) + PARAM_SETS)
    assert n_sites[0] >= len(called)
    # the call left the state as it was, and accumulation goes on behind it
    assert np.array_equal(h.pileup_all(), counts) and h.pileup_mates() == want.mates
    want.add(o, batch, *h.classify(*_args(batch)))
    counts2 = want.check(h)
    assert np.array_equal(counts2, 2 * counts)
    check_calls(h, sm, counts2, (DEFAULTS, (16, 6, 1, 5)))


# ---------------------------------------------------------------------------
# 5. state rules; 6. inertness
# ---------------------------------------------------------------------------
def test_state_rules(oracle):
    from shark_amd import SharkHip, SharkHipError
    genes, mutated, planted, batch = e2e_case(17, 1, n=50)
    records = [bytes(m) for m in mutated]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    for call in (h.variants, h.variants_summary, lambda: h.pileup_add(np.zeros(4, np.uint32), 0)):
        with pytest.raises(SharkHipError):                    # before finalize: no pileup state yet
            call()
    h.keep_bases()
    h.build(records)
    with pytest.raises(SharkHipError):
        h.keep_bases()                                        # finalized already
    with pytest.raises(SharkHipError):
        h.keep_positions()
    for call in (h.variants, h.variants_summary, lambda: h.pileup_add(np.zeros((int(h.depth_layout()[-1]), 4), np.uint32), 0)):
        with pytest.raises(SharkHipError, match="never enabled"):
            call()
    # without keep_bases: the calls refuse, pileup itself works
    o, h2, sm = build_kb(oracle, mutated, keep_bases=False, k=17)
    want = Want(sm, 8)
    h2.pileup_enable(8)
    want.add(o, batch, *h2.classify(*_args(batch)))
    want.check(h2)
    for call in (h2.variants, h2.variants_summary):
        with pytest.raises(SharkHipError, match="without shk_ref_keep_bases"):
            call()
    h2.pileup_add(h2.pileup_all(), 0)                         # (pileup_add needs the state alone)
    # bad parameters
    h.pileup_enable(8)
    for bad in ((0, 3, (1, 5)), (8, 0, (1, 5)), (8, 3, (1, 0)), (8, 3, (6, 5)), (8, 3, (1, 65536))):
        for call in (h.variants, h.variants_summary):
            with pytest.raises(SharkHipError):
                call(*bad)
    assert len(h.variants(1, 1, (0, 1))) == 0 and len(h.variants(M32, M32, (65535, 65535))) == 0
    assert h.L.shk_variants_get(h.h, None, None, 0, C.byref(C.c_uint64())) == -1
    prm = capi.ShkVariantParams(*DEFAULTS)
    assert h.L.shk_variants_get(h.h, C.byref(prm), None, 0, None) == -1
    assert h.L.shk_variants_summary(h.h, C.byref(prm), None, int(h.index_info()["nidx"]) + 1) == -1
    # tickets outstanding
    tk = h.submit(*_args(batch))
    for call in (h.variants, h.variants_summary, lambda: h.pileup_add(h2.pileup_all(), 0)):
        with pytest.raises(SharkHipError, match="tickets"):
            call()
    h.wait(tk)
    want.check(h)                                             # (the same batch over the same records)
    before = h.pileup_all()
    v = h.variants()
    s = h.variants_summary()
    assert len(v) > 0 and int(s["sites"].sum()) == len(v)
    assert np.array_equal(h.pileup_all(), before) and h.pileup_mates() == want.mates
    # the mode off: the state stays, and so do the read-outs
    h.pileup_enable(0)
    same(h.variants(), v)
    # fewer genes than the index has
    out = np.zeros(2, dtype=capi.GENE_VARIANTS_DTYPE)
    assert h.L.shk_variants_summary(h.h, C.byref(prm), capi._ptr(out), 2) == 0
    same(out, s[:2])


def test_keep_bases_is_inert(oracle):
    """keep_bases asked for and nothing called: every result of every mode equals a context's without it, byte for byte"""
    from shark_amd import SharkHip
    rng = np.random.default_rng(41)
    panel = [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]
    records = [bytes(g) for g, _ in panel]
    batches = [spliced_reads(rng, panel, 300, ragged=False), spliced_reads(rng, panel, 300, ragged=True)]
    seen = []
    for new in (False, True):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build(records, keep_positions=True, keep_bases=new)
        assert (len(h.debug_index_array("recbase")) > 0) == new
        h.evidence_enable(True)
        h.candidates_enable(4)
        h.placement_enable(True)
        h.segments_enable(2)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        h.pileup_enable(8)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            cr, ce = h.candidates_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                         keys.tobytes(), segs.tobytes()))
        seen.append((rows, h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.depth_summary().tobytes(), h.junctions_get().tobytes(),
                     h.pileup_all().tobytes(), h.pileup_mates(), h.probe_mode(), h.index_info()))
    assert seen[0] == seen[1] and len(seen[0][5]) > 0 and any(seen[0][6])


# ---------------------------------------------------------------------------
# 7. the command
# ---------------------------------------------------------------------------
def run_shark(args, cwd):
    return subprocess.run([os.path.join(ROOT, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def test_shark_variants_on_the_mutated_example(oracle, example_dir, tmp_path):
    records, legend, gs, counts, mates = mutated_example_pileup(oracle)
    want = "".join(ln + "\n" for ln in variant_lines(expected_variants(counts, records, gs), legend)).encode()
    assert want.count(b"\n") == 7
    with open(tmp_path / "mutated.fa", "wb") as f:
        for name, seq in mutated_example_records():
            f.write(b">" + name + b"\n" + seq + b"\n")
    base = ["-r", str(tmp_path / "mutated.fa"), "-1", os.path.join(example_dir, "sample_1.fq"), "-2", os.path.join(example_dir, "sample_2.fq"),
            "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    for extra in ([], ["--gpus", "2", "--devices", "0,0", "--batch", "700"]):
        r = run_shark(base + ["--variants", str(tmp_path / "va")] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert (tmp_path / "va").read_bytes() == want
    # other thresholds
    loose = (1, 1, 0, 1)
    want_loose = "".join(ln + "\n" for ln in variant_lines(expected_variants(counts, records, gs, loose), legend)).encode()
    r = run_shark(base + ["--variants", str(tmp_path / "vl"), "--variants-min-depth", "1", "--variants-min-alt", "1", "--variants-min-frac", "0/1", "--gpus", "2",
                          "--devices", "0,0"], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert (tmp_path / "vl").read_bytes() == want_loose and want_loose.count(b"\n") >= 7
    # with --pileup: the pileup file is what it is without --variants, and the variants are the same
    r = run_shark(base + ["--pileup", str(tmp_path / "pu")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    r = run_shark(base + ["--pileup", str(tmp_path / "pu2"), "--variants", str(tmp_path / "va2"), "--gpus", "2", "--devices", "0,0", "--batch", "700"], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert (tmp_path / "pu2").read_bytes() == (tmp_path / "pu").read_bytes() and len((tmp_path / "pu").read_bytes()) > 10000
    assert (tmp_path / "va2").read_bytes() == want
    # one pileup, one floor
    r = run_shark(base + ["--pileup", str(tmp_path / "pu3"), "--pileup-min-support", "3", "--variants", str(tmp_path / "va3")], str(tmp_path))
    assert r.returncode == 1 and b"must be equal" in r.stderr and not (tmp_path / "va3").exists()
