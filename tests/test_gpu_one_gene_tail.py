"""The tail of a batch against an index of ONE record (shark_hip.hip, enqueue_tail; device_scan.hpp, exclusive_scan_assemble_one): the
scan of the per-read counts writes gene_off, fills gene_ids with id 0, writes the batch's counters and counts gene 0 -- no gather, no
EMIT pass, no histogram, no finalize launch.  No result may change: everything here is compared with the oracle by count and ids AND,
byte for byte, with a handle made under SHK_PLAIN_TAIL=1, which takes the sequence every other index takes.

One gene of 6 000 bases, k = 17, c = 0.6, 2 x 150 bp (the helpers of tests/test_gpu_triple_loads_results.py).
  * through the library around the scan's tile (4 096 items, the scan runs over n + 1): n = 0 ... 12 289, the assigned pairs all, none,
    every second, only the first, only the last; last_n_tie == 0.
  * the per-gene counter over two batches, and shk_count_work, which adds nothing.
  * the second run of the tail: a length bound that does not hold (CTR_LONG set, finish_classify redoes the tail): counted once.
  * a host batch through shk_classify and through submit / wait: the pinned arrays equal the resident call's.
  * placement mode: the records behind the tail equal the plain tail's.
  * control: a two-gene index never takes the path; equal to the oracle with and without the switch.
  * shk_debug_assemble_one against a host model in numpy: count[] of all ones, all zeros, a single one in the first, last and middle
    position of a tile, random 0 / 1; lengths 1, 4 095, 4 096, 4 097, 3 x 4 096 + 5; aligned and at element offsets 1 ... 3; a capacity
    of exactly the total (filled, no overflow) and of one less (CTR_OVERFLOW, no id written, nothing counted); CTR_LONG preset with
    and without skip_if_long (counted only without); the words behind the total and the guard bands behind the capacity unchanged.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth, views
from tests import test_gpu_triple_loads_results as T

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = [0, 1, 2, 3, 4094, 4095, 4096, 4097, 8191, 12289]
PATTERNS = ["all", "none", "every-second", "first", "last"]
N_POOL = max(SIZES)


def handle(monkeypatch, plain, genes=None, keep_positions=False):
    """a handle over the one gene (or `genes`); plain: made under SHK_PLAIN_TAIL=1 (the switch is read when the handle is created)"""
    from shark_amd import SharkHip
    for v in T.SWITCHES + ("SHK_PLAIN_TAIL",):
        monkeypatch.delenv(v, raising=False)
    if plain:
        monkeypatch.setenv("SHK_PLAIN_TAIL", "1")
    h = SharkHip(k=17, c=T.C, bf_bits=T.BF)
    h.build([bytes(g) for g in (genes or [T.the_gene()])], keep_positions=keep_positions)
    monkeypatch.delenv("SHK_PLAIN_TAIL", raising=False)
    return h


_pool = {}


def pool(oracle):
    """N_POOL pairs from the gene (all assigned) and N_POOL from elsewhere (none assigned), with the oracle's answers"""
    if not _pool:
        rng = np.random.default_rng(7100)
        A = T.answers(oracle, 17)
        hit = A.add([T.gene_pair(rng, 150, 150) for _ in range(N_POOL)])
        miss = A.add([T.elsewhere_pair(rng, 150, 150) for _ in range(N_POOL)])
        assert all(A.assigned(i) for i in hit) and not any(A.assigned(i) for i in miss)
        _pool["p"] = (A, hit, miss)
    return _pool["p"]


def pick(oracle, n, pattern):
    """-> (batch, (gene_off, gene_ids) of the oracle)"""
    A, hit, miss = pool(oracle)
    on = {"all": lambda i: True, "none": lambda i: False, "every-second": lambda i: i % 2 == 0, "first": lambda i: i == 0,
          "last": lambda i: i == n - 1}[pattern]
    return A.batch([hit[i] if on(i) else miss[i] for i in range(n)])


def resident(h, batch, max_read_len=150, reset=True):
    """-> (gene_off, gene_ids, n_assoc, the tensors that hold the batch, its pointers)"""
    e = views.embed(batch, views.shifts_of(0, 0))
    keep, p = views.to_device(e)
    if reset:
        h.gene_counts_reset()
    r = h.classify_device(e["n"], p["seq1"], p["off1"], p["seq2"], p["off2"], max_read_len=max_read_len)
    goff, gids = T.fetch(r)
    return goff, gids, int(r.n_assoc), keep, p


def equal_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


# ---------------------------------------------------------------------------
# through the library
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_around_the_scans_tile(oracle, monkeypatch, pattern):
    h, hp = handle(monkeypatch, False), handle(monkeypatch, True)
    for n in SIZES:
        b, want = pick(oracle, n, pattern)
        what = (pattern, n)
        goff, gids, tot, _, _ = resident(h, b)
        counters = h.gene_counts(T.N_COUNTERS)
        assert tot == len(want[1]) == int(goff[-1]) and len(goff) == n + 1, what
        T.same((goff, gids, counters), want, what)
        equal_bytes(goff, want[0], what)
        assert h.timing()["last_n_tie"] == 0 and h.timing()["last_n_long"] == 0, what
        pgoff, pgids, ptot, _, _ = resident(hp, b)
        assert ptot == tot, what
        equal_bytes(goff, pgoff, what)
        equal_bytes(gids, pgids, what)
        assert np.array_equal(counters, hp.gene_counts(T.N_COUNTERS)), what
    h.close()
    hp.close()


def test_the_per_gene_counter_over_two_batches_and_count_work(oracle, monkeypatch):
    b1, w1 = pick(oracle, 4097, "every-second")
    b2, w2 = pick(oracle, 8191, "all")
    got = []
    for plain in (False, True):
        h = handle(monkeypatch, plain)
        h.gene_counts_reset()
        _, _, t1, _, _ = resident(h, b1, reset=False)
        _, _, t2, keep, p = resident(h, b2, reset=False)
        c = h.gene_counts(T.N_COUNTERS)
        assert t1 == len(w1[1]) == 2049 and t2 == len(w2[1]) == 8191
        assert c.tolist() == [t1 + t2, 0, 0, 0], (plain, c.tolist())
        h.count_work(8191, p["seq1"], p["off1"], p["seq2"], p["off2"])
        assert np.array_equal(h.gene_counts(T.N_COUNTERS), c), (plain, "shk_count_work counted the batch")
        got.append(c)
        del keep
        h.close()
    assert np.array_equal(got[0], got[1])


def test_the_second_tail_run_counts_once(oracle, monkeypatch):
    """pairs of 2 x 600 bases behind max_read_len = 150: the speculative launch queues them (CTR_LONG), the histogram's rule skips the
    batch, finish_classify runs the general kernel and the tail again -- the batch is counted there, and only there"""
    rng = np.random.default_rng(7200)
    A = T.answers(oracle, 17)
    pairs = []
    for i in range(TILE + 40):
        L = 600 if i % 7 == 3 else 150
        pairs.append(T.gene_pair(rng, L, L) if i % 3 else T.elsewhere_pair(rng, L, L))
    b, want = A.batch(A.add(pairs))
    assert 0 < len(want[1]) < len(pairs)
    got = []
    for plain in (False, True):
        h = handle(monkeypatch, plain)
        goff, gids, tot, _, _ = resident(h, b, max_read_len=150)
        assert h.timing()["last_n_long"] > 0 and h.timing()["last_n_tie"] == 0
        assert tot == len(want[1])
        T.same((goff, gids, h.gene_counts(T.N_COUNTERS)), want, ("redo", plain))
        got.append((goff, gids))
        h.close()
    equal_bytes(got[0][0], got[1][0], "gene_off")
    equal_bytes(got[0][1], got[1][1], "gene_ids")


def test_host_batches(oracle, monkeypatch):
    """shk_classify and submit / wait: gene_off and gene_ids leave through pinned memory behind the tail"""
    h = handle(monkeypatch, False)
    for n, pattern in ((4097, "every-second"), (1, "all"), (3, "none"), (8191, "last")):
        b, want = pick(oracle, n, pattern)
        goff, gids, tot, _, _ = resident(h, b)
        h.gene_counts_reset()
        hgoff, hgids = h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"])
        t1 = h.submit(b["seq1"], b["off1"], b["seq2"], b["off2"])
        t2 = h.submit(b["seq1"], b["off1"], b["seq2"], b["off2"])
        for sgoff, sgids in ((hgoff, hgids), h.wait(t1), h.wait(t2)):
            equal_bytes(sgoff, goff, (n, pattern))
            equal_bytes(sgids, gids, (n, pattern))
            equal_bytes(sgoff, want[0], (n, pattern))
            assert np.array_equal(sgids, want[1])
        assert h.gene_counts(T.N_COUNTERS).tolist() == [3 * tot, 0, 0, 0]
    h.close()


def test_placement_mode_behind_the_tail(oracle, monkeypatch):
    from shark_amd import capi
    b, want = pick(oracle, 4097, "every-second")
    got = []
    for plain in (False, True):
        h = handle(monkeypatch, plain, keep_positions=True)
        h.placement_enable()
        goff, gids, tot, _, _ = resident(h, b)
        n_assoc, ptr = h.placement_last()
        assert n_assoc == tot == len(want[1])
        got.append((goff, gids, capi.placements_from_device(n_assoc, ptr)))
        h.close()
    equal_bytes(got[0][0], got[1][0], "gene_off")
    equal_bytes(got[0][1], got[1][1], "gene_ids")
    equal_bytes(got[0][2], got[1][2], "placement records")
    assert (got[0][2][:, :, 2] > 0).any(), "no mate of a batch from the gene was placed"


def test_control_two_genes(oracle, monkeypatch):
    """an index of two records takes the sequence it took, whatever the switch says: equal to the oracle both times"""
    rng = np.random.default_rng(7300)
    genes = [T.the_gene(), synth.random_seq(rng, 6000)]
    o = oracle.Shark(k=17, c=T.C, bf_bits=T.BF)
    o.build([bytes(g) for g in genes])
    m1, m2 = [], []
    for i in range(TILE + 3):
        if i % 3 == 2:
            a, c = T.elsewhere_pair(rng, 150, 150)
        else:
            g = genes[i % 3]
            s = int(rng.integers(0, 6000 - 360))
            a, c = g[s:s + 150].copy(), synth.revcomp(g[s + 200:s + 350])
        m1.append(a)
        m2.append(c)
    b = synth.batch_from_lists(m1, m2)
    wgoff, wgids = o.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], nthreads=4)
    o.close()
    assert set(wgids.tolist()) == {0, 1}
    for plain in (False, True):
        h = handle(monkeypatch, plain, genes=genes)
        goff, gids, tot, _, _ = resident(h, b)
        assert tot == len(wgids)
        T.same((goff, gids, h.gene_counts(T.N_COUNTERS)), (wgoff.astype(np.uint32), wgids.astype(np.uint16)), ("two genes", plain))
        h.close()


# ---------------------------------------------------------------------------
# the three launches alone, against a host model
# ---------------------------------------------------------------------------
LENGTHS = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
KINDS = ["ones", "zeros", "first", "last", "middle", "random"]
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (3, 0)]       # (count, gene_off): (0, 0) alone takes the 16-byte accesses


def counts_of(kind, n):
    """first / last / middle: a single one at the first position of the last tile, at the last position of a tile (the first whole
    tile's, else the array's), in the middle of the last tile"""
    t0 = (n - 1) // TILE * TILE
    a = np.zeros(n, np.uint32)
    if kind == "ones":
        a[:] = 1
    elif kind == "first":
        a[t0] = 1
    elif kind == "last":
        a[TILE - 1 if n >= TILE else n - 1] = 1
    elif kind == "middle":
        a[t0 + (n - t0) // 2] = 1
    elif kind == "random":
        a[:] = np.random.default_rng(n).integers(0, 2, size=n)
    return a


def model(count, cap, ctr_long, skip_if_long, count_genes, fill):
    total = int(count.sum(dtype=np.uint64))
    off = (np.cumsum(count, dtype=np.uint64) - count).astype(np.uint32)
    overflow = total > cap
    ids = np.full(cap, fill, np.uint16)
    if not overflow:
        ids[:total] = 0
    counters = np.zeros(16, np.uint32)
    counters[0], counters[2], counters[6], counters[7] = ctr_long, int(overflow), total & 0xFFFFFFFF, total >> 32
    added = total if count_genes and not overflow and not (skip_if_long and ctr_long) else 0
    return off, ids, counters, added


def check(h, count, cap, what, count_off=0, off_off=0, ctr_long=0, skip_if_long=False, count_genes=True):
    assert (h.DEBUG_CTR_LONG, h.DEBUG_CTR_OVERFLOW, h.DEBUG_CTR_ASSOC_LO, h.DEBUG_CTR_ASSOC_HI, h.DEBUG_COUNTER_WORDS) == (0, 2, 6, 7, 16)
    off, ids, counters, added, guards = h.debug_assemble_one(count, cap, count_off, off_off, ctr_long, skip_if_long, count_genes)
    woff, wids, wcounters, wadded = model(count, cap, ctr_long, skip_if_long, count_genes, h.DEBUG_FILL16)
    assert not guards.any(), (what, dict(zip(h.DEBUG_ASSEMBLE_GUARDS, guards.tolist())))
    assert np.array_equal(off, woff), (what, "gene_off differs at %d" % int(np.argmax(off != woff)))
    assert np.array_equal(ids, wids), (what, "gene_ids differs at %d of %d" % (int(np.argmax(ids != wids)), cap))
    assert np.array_equal(counters, wcounters), (what, counters.tolist(), wcounters.tolist())
    assert added == wadded, (what, added, wadded)


@pytest.fixture(scope="module")
def bare():
    """a context without an index: the entry point needs none"""
    from shark_amd import SharkHip
    h = SharkHip(k=17, c=T.C, bf_bits=1 << 20)
    yield h
    h.close()


@pytest.mark.parametrize("kind", KINDS)
def test_assemble_one_against_the_model(bare, kind):
    """the words of gene_ids behind the total stay what they were (37 of them here), and so do the guard bands behind the capacity"""
    for n in LENGTHS:
        count = counts_of(kind, n)
        total = int(count.sum())
        for co, oo in OFFSETS:
            check(bare, count, total + 37, (kind, n, co, oo), co, oo)
        for co, oo in OFFSETS[:2]:
            check(bare, count, total, (kind, n, co, oo, "capacity = total"), co, oo)
            if total:
                check(bare, count, total - 1, (kind, n, co, oo, "capacity = total - 1"), co, oo)


@pytest.mark.parametrize("n", LENGTHS)
def test_assemble_one_counts_by_the_histograms_rule(bare, n):
    count = counts_of("random" if n > 1 else "ones", n)
    total = int(count.sum())
    assert total > 0
    for co, oo in OFFSETS[:2]:
        for ctr_long in (0, 5):
            for skip in (False, True):
                for cg in (True, False):
                    check(bare, count, total + 9, (n, co, oo, ctr_long, skip, cg), co, oo, ctr_long, skip, cg)
        # an overflowing batch with long reads queued, counting asked for: nothing counted, nothing written
        check(bare, count, total - 1, (n, co, oo, "overflow + long"), co, oo, 5, False, True)
