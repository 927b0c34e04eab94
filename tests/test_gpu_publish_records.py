"""The one path every record mode's results take to the host (publish_records_kernel, classify.hip): a host batch's records, read from
the context's pinned memory behind classify and behind submit / wait, are byte for byte the records the same batch leaves on the device
at the resident entry point.  The shapes are the smallest at which a copy of 16 bytes per lane with a word tail can go wrong: every
residue of the word count modulo 4 that records of 6 words (placements) and 10 m words (a pair's segment entries) reach, the empty batch,
per-read records of 3 words (evidence: all four residues), 2 and 3 m words (candidates), and a batch whose associations overflow the slot with all five
per-association modes on.  What the records ARE is the other GPU tests' business (each mode against its model); here the reference is the
resident read-back of the same library.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from shark_amd.capi import SHK_MAX_CANDIDATES, SHK_MAX_SEGMENTS
from tests import synth
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu

MIN_INTRON, MAX_FRAG, N_BINS, S_MIN = 20, 1000, 64, 8
L = 100


def tie_reference():
    """one gene of its own and the six identical genes of test_shared_stretch_and_six_way_tie: a pair from the first has one association,
    a pair from the twins six (more than SHK_INLINE_IDS: through the EMIT pass)"""
    rng = np.random.default_rng(17)
    gene = synth.random_seq(rng, 1100)
    twin = synth.random_seq(rng, 900)
    return gene, twin, [gene] + [twin.copy() for _ in range(6)]


def pairs_from(rec, starts):
    return [rec[a:a + L] for a in starts], [synth.revcomp(rec[a + 200:a + 200 + L]) for a in starts]


def batch_of(gene, twin, ones, sixes, none=0):
    """`ones` pairs from the single gene, `sixes` from the twins, `none` of random bases: ones + 6 sixes associations"""
    rng = np.random.default_rng(1000 + 100 * ones + 10 * sixes + none)
    a1, a2 = pairs_from(gene, [13 + 41 * i for i in range(ones)])
    b1, b2 = pairs_from(twin, [7 + 29 * i for i in range(sixes)])
    c = [synth.random_seq(rng, L) for _ in range(2 * none)]
    return synth.batch_from_lists(a1 + b1 + c[:none], a2 + b2 + c[none:])


def set_modes(h, seg_m, per_read_m=0):
    """the five per-association modes at seg_m entries per mate (0: all five off), evidence and candidates at per_read_m (0: off)"""
    on = seg_m != 0
    h.placement_enable(on)
    h.segments_enable(seg_m)
    if on:
        h.alignments_enable(S_MIN)
    h.pairs_enable(MIN_INTRON, MAX_FRAG, N_BINS if on else 0)
    h.rescue_enable(MIN_INTRON, MAX_FRAG if on else 0)
    if not on:
        h.alignments_enable(0)
    h.evidence_enable(per_read_m != 0)
    h.candidates_enable(per_read_m)


def host_records(h):
    """every per-association kind of the host batch handed out last, as bytes"""
    keys, entries = h.segments_last()
    return {"placement": h.placement_last().tobytes(), "segment keys": keys.tobytes(), "segment entries": entries.tobytes(),
            "alignments": h.alignments_last().tobytes(), "pairs": h.pairs_last().tobytes(), "rescue": h.rescue_last().tobytes()}


def device_records(h, r):
    """the same of the resident batch handed out last, read back from the device"""
    tot = int(r.n_assoc)
    goff, gids = np.zeros(int(r.n) + 1, np.uint32), np.zeros(tot, np.uint16)
    capi.hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        capi.hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    na, m, kp, ep = h.segments_last()
    assert na == tot
    keys, entries = capi.segments_from_device(na, m, kp, ep)
    rec = {"segment keys": keys.tobytes(), "segment entries": entries.tobytes()}
    for name, last, read in (("placement", h.placement_last, capi.placements_from_device), ("alignments", h.alignments_last, capi.alignments_from_device),
                             ("pairs", h.pairs_last, capi.pairs_from_device), ("rescue", h.rescue_last, capi.rescues_from_device)):
        na, ptr = last()
        assert na == tot, name
        rec[name] = read(na, ptr).tobytes()
    return goff, gids, rec


def same_everywhere(h, batch, n_assoc=None):
    """classify, submit / wait and the resident entry point on one batch: the same genes and, kind for kind, the same record bytes"""
    n = len(batch["off1"]) - 1
    t = _to_device(batch) if n else None
    if n:
        dgoff, dgids, want = device_records(h, h.classify_device(n, max_read_len=L, **_dev_ptrs(t)))
    goff, gids = h.classify(*_args(batch))
    if n_assoc is not None:
        assert int(goff[-1]) == len(gids) == n_assoc
    got = [host_records(h)]
    goff2, gids2 = h.wait(h.submit(*_args(batch)))
    got.append(host_records(h))
    assert np.array_equal(goff, goff2) and np.array_equal(gids, gids2)
    if not n:
        assert all(len(b) == 0 for g in got for b in g.values())
        return
    assert np.array_equal(goff, dgoff) and np.array_equal(gids, dgids)
    for how, g in zip(("classify", "submit / wait"), got):
        for kind in want:
            assert len(want[kind]) > 0 or len(gids) == 0
            assert g[kind] == want[kind], "%s: %s records differ from the resident batch's" % (how, kind)


@pytest.fixture(scope="module")
def tie_handle(oracle):
    gene, twin, records = tie_reference()
    o, h, _ = build_kb(oracle, records, k=17)
    return gene, twin, h


# (ones, sixes, unassigned pairs) -> 0, 1, 2, 3, 5 and 6 x 3 associations.  Records of 6 words (placements), 2 (segment headers) and 10 m (a
# pair's segment entries) end on a multiple of 4 words or 2 words behind one: odd and even counts give both, at less and at more than one
# 16-byte copy per array (per-read records of 3 words, which reach the odd residues, are the next test's)
COUNTS = [(0, 0, 1), (1, 0, 0), (2, 0, 1), (3, 0, 0), (5, 0, 0), (0, 3, 0)]


@pytest.mark.parametrize("seg_m", [1, 3, SHK_MAX_SEGMENTS])
def test_record_modes_host_equals_resident(tie_handle, seg_m):
    """placement, segments, alignments, pairs and rescue together on one handle; at seg_m below SHK_MAX_SEGMENTS the alignments read a
    second launch of segments_kernel into arrays of their own"""
    gene, twin, h = tie_handle
    set_modes(h, seg_m)
    for ones, sixes, none in COUNTS:
        same_everywhere(h, batch_of(gene, twin, ones, sixes, none), ones + 6 * sixes)
    same_everywhere(h, synth.batch_from_lists([], []), 0)     # the empty batch


@pytest.mark.parametrize("m", [1, SHK_MAX_CANDIDATES])
def test_evidence_and_candidates_host_equals_resident(tie_handle, m):
    """the per-read kinds at n = 1 .. 5: 3 n words of evidence, 2 n and 3 m n words of candidates"""
    gene, twin, h = tie_handle
    set_modes(h, 0, m)
    for n in (1, 2, 3, 4, 5):
        batch = batch_of(gene, twin, (n + 1) // 2, n // 2)
        t = _to_device(batch)
        h.classify_device(n, max_read_len=L, **_dev_ptrs(t))
        ev = np.zeros((n, 3), np.uint32)
        capi.hip_memcpy_dtoh(ev, h.evidence_last(), ev.nbytes)
        cn, cm, rp, ep = h.candidates_last()
        assert (cn, cm) == (n, m)
        reads, entries = np.zeros((n, 2), np.uint32), np.zeros((n, m, 3), np.uint32)
        capi.hip_memcpy_dtoh(reads, rp, reads.nbytes)
        capi.hip_memcpy_dtoh(entries, ep, entries.nbytes)
        assert ev[:, 1].all() and reads[:, 1].all()            # (every read has k-mers and a gene: no record is all zero)
        for how in ("classify", "submit / wait"):
            if how == "classify":
                h.classify(*_args(batch))
            else:
                h.wait(h.submit(*_args(batch)))
            hr, he = h.candidates_last()
            assert h.evidence_last().tobytes() == ev.tobytes(), "%s: evidence differs at n = %d" % (how, n)
            assert hr.tobytes() == reads.tobytes() and he.tobytes() == entries.tobytes(), "%s: candidates differ at n = %d" % (how, n)


def test_overflow_repair_with_all_record_modes(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 pairs tied over 6 identical genes with all five modes on.  The
    first pass is refused on the device and the tail runs again in wait: every kind's 18 000 records are the resident batch's, none of a
    first pass that held fewer"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    o, h, _ = build_kb(oracle, [twin.copy() for _ in range(6)], k=17)
    set_modes(h, SHK_MAX_SEGMENTS)
    a = [(7 * i) % 200 for i in range(3000)]
    batch = synth.batch_from_lists([twin[x:x + 50] for x in a], [synth.revcomp(twin[300 + x:350 + x]) for x in a])
    assert 6 * 3000 > 2 * 3000 + 4096 + (2 * 3000 + 4096) // 4 + 64      # beyond what the slot's first reservation holds
    same_everywhere(h, batch, 18000)
