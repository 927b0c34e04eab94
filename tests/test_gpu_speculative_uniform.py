"""Speculation on a uniform resident stream (shark_hip.hip, enqueue_classify): behind a batch that the device judged uniform,
shk_classify_device launches the next batch's uniform kernel for the same lengths at once and uniform_check_kernel looks at the offsets
beside it.  No result may change and nothing observable but shk_debug_last_speculation (0 not speculated, 1 speculated and held, 2
speculated and run again) and shk_timing's prepass_ms.

The flagship index: one gene of 20 kb, k = 17, c = 0.6.  Sequences of batches go through ONE context with classify_device(...,
max_read_len=L).  Every batch is compared with the oracle by count and ids and, byte for byte, with a second handle created under
SHK_NO_SPECULATE=1 that is sent the same sequence: gene_off, gene_ids and last_kernel() per batch, shk_gene_counts at the end.  The
expected value of shk_debug_last_speculation is asserted per batch.

  * n = 1, 2, 3, 4, 64, 193, 3 001 (the ends of a triple and of a 64-read block, a batch the grid does not divide) at 2 x 150 and
    1 x 150: three uniform batches of one shape, 0, 1, 1.
  * a uniform batch of other lengths (2 x 100) behind 2 x 150: the totals differ, the kernel's guard returns: 2, then 1.
  * compensating lengths, which pass the guard: reads 0 and 1 of 151 and 149 bases, the last two, two in the middle, in one mate only,
    the odd pair across a triple's boundary: 2 each, the oracle's result, counted once.
  * uniform, trimmed (100 - 150), uniform, uniform: 0, 2, 0, 1.
  * n grows from 64 to 3 001; a batch of n = 0 in between; paired, then single; qualities appear; max_read_len changes the
    specialisation; placement mode on and off; shk_count_work; offsets and bases at addresses that are not 16-byte aligned.
  * a mis-speculated batch with reads beyond the length bound: the batch runs again, and then finish_classify's long-read path runs the
    tail a third time -- counted once.  (The other slow path, more associations than gene_ids holds, cannot be reached on an index of
    one record: a read has at most one association there and gene_ids holds 2 n + 4 096 of them.  tests/test_gpu_one_gene_tail.py
    checks that flag through shk_debug_assemble_one.)

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # noqa: F401  (torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both)

from tests import synth, views
from tests import test_gpu_triple_loads_results as T

pytestmark = pytest.mark.gpu

K, C, BF = 17, 0.6, 1 << 30
SIZES = [1, 2, 3, 4, 64, 193, 3001]

_gene = []


def the_gene():
    if not _gene:
        _gene.append(synth.random_seq(np.random.default_rng(9100), 20000))
    return _gene[0]


def make_batch(seed, n, L1=150, L2=150, lens=None, quals=False):
    """n reads, every second one from the gene; L2 == 0: single-end; lens = {read: (l1, l2)} where a read has other lengths;
    callable lens(i) -> (l1, l2) for all of them"""
    rng = np.random.default_rng([seed, n, L1, L2])
    g = the_gene()
    m1, m2 = [], []
    for i in range(n):
        l1, l2 = (lens(i) if callable(lens) else (lens or {}).get(i, (L1, L2)))
        if i % 2 == 0:
            a = int(rng.integers(0, len(g) - l1 - l2 - 60))
            m1.append(g[a:a + l1].copy())
            m2.append(synth.revcomp(g[a + l1 + 50:a + l1 + 50 + l2]))
        else:
            m1.append(synth.random_seq(rng, l1))
            m2.append(synth.random_seq(rng, l2))
    if n == 0:
        b = {"seq1": np.zeros(0, np.uint8), "off1": np.zeros(1, np.uint64), "seq2": None, "off2": None, "qual1": None, "qual2": None}
        if L2:
            b["seq2"], b["off2"] = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
        return b
    q1 = [np.full(len(m), views.HI_Q, np.uint8) for m in m1] if quals else None
    q2 = [np.full(len(m), views.HI_Q, np.uint8) for m in m2] if quals and L2 else None
    return synth.batch_from_lists(m1, m2 if L2 else None, q1, q2)


class Pair:
    """the speculating handle, the one made under SHK_NO_SPECULATE=1, and the oracle"""

    def __init__(self, oracle, monkeypatch, keep_positions=False):
        from shark_amd import SharkHip
        for v in T.SWITCHES + ("SHK_PLAIN_TAIL", "SHK_NO_SPECULATE"):
            monkeypatch.delenv(v, raising=False)
        self.h = SharkHip(k=K, c=C, bf_bits=BF)
        self.h.build([bytes(the_gene())], keep_positions=keep_positions)
        monkeypatch.setenv("SHK_NO_SPECULATE", "1")
        self.hn = SharkHip(k=K, c=C, bf_bits=BF)
        self.hn.build([bytes(the_gene())], keep_positions=keep_positions)
        monkeypatch.delenv("SHK_NO_SPECULATE", raising=False)
        assert self.h.probe_mode() == self.hn.probe_mode() == "lds-table"
        self.o = oracle.Shark(k=K, c=C, bf_bits=BF)
        self.o.build([bytes(the_gene())])
        self.total = 0

    def run(self, b, expect, what, max_read_len=150, shifts=None):
        """one batch through both handles; -> the speculating handle's (gene_off, gene_ids)"""
        wgoff, wgids = self.o.classify(b["seq1"], b["off1"], b.get("seq2"), b.get("off2"), nthreads=2)
        e = views.embed(b, shifts or views.shifts_of())
        keep, p = views.to_device(e)
        got = []
        for h in (self.h, self.hn):
            r = h.classify_device(e["n"], p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"], max_read_len=max_read_len)
            got.append(T.fetch(r) + (h.last_kernel(), h.debug_last_speculation(), h.timing()["last_n_long"]))
        del keep
        (goff, gids, name, spec, n_long), (ngoff, ngids, nname, nspec, nn_long) = got
        assert (spec, nspec) == (expect, 0), (what, "speculation", spec, nspec, name)
        assert np.array_equal(np.diff(goff.astype(np.int64)), np.diff(wgoff.astype(np.int64))), (what, "counts differ from the oracle's")
        assert np.array_equal(gids, wgids.astype(np.uint16)), (what, "ids differ from the oracle's")
        assert goff.tobytes() == ngoff.tobytes() and gids.tobytes() == ngids.tobytes(), (what, "differs from SHK_NO_SPECULATE=1")
        assert name == nname and n_long == nn_long, (what, name, nname, n_long, nn_long)
        self.total += len(wgids)
        return goff, gids

    def close(self):
        """the per-gene counters of both handles: every batch once"""
        c, cn = self.h.gene_counts(T.N_COUNTERS), self.hn.gene_counts(T.N_COUNTERS)
        self.h.close()
        self.hn.close()
        self.o.close()
        assert c.tolist() == cn.tolist() == [self.total, 0, 0, 0], (c.tolist(), cn.tolist(), self.total)


@pytest.mark.parametrize("L2", [150, 0])
def test_three_uniform_batches_at_every_size(oracle, monkeypatch, L2):
    P = Pair(oracle, monkeypatch)
    first = True
    for n in SIZES:
        for j in range(3):
            # (behind the first size the stream is uniform already: a batch of another n is speculated on as well)
            P.run(make_batch(100 + j, n, 150, L2), 0 if first else 1, (L2, n, j))
            first = False
    assert "+three-pairs-if-they-fit" in P.h.last_kernel() and "device" in P.h.last_kernel() and "verdict=uniform" in P.h.last_kernel()
    P.close()


@pytest.mark.parametrize("L2", [150, 0])
def test_other_lengths_behind_a_uniform_batch(oracle, monkeypatch, L2):
    """2 x 100 behind 2 x 150: off[n] is not n x 150, the kernel's guard returns; the next batch is speculated on at the new lengths"""
    P = Pair(oracle, monkeypatch)
    for n in SIZES:
        P.run(make_batch(200, n, 150, L2), 0 if n == SIZES[0] else 1, (n, "2 x 150"))
        P.run(make_batch(201, n, 100, 100 if L2 else 0), 2, (n, "2 x 100"))
        P.run(make_batch(202, n, 100, 100 if L2 else 0), 1, (n, "2 x 100 again"))
        P.run(make_batch(203, n, 150, L2), 2, (n, "back to 2 x 150"))
    P.close()


def compensating(n, where, L2):
    """{read: (l1, l2)}: two reads whose lengths add up to two uniform ones.  The totals are those of a uniform batch, so the kernel's
    guard lets the launch through and only the check beside it finds the batch out"""
    m2 = (149, 151) if L2 else (0, 0)
    if where == "first":
        return {0: (151, m2[0]), 1: (149, m2[1])}
    if where == "last":
        return {n - 2: (151, m2[0]), n - 1: (149, m2[1])}
    if where == "middle":
        a = min(n // 2, n - 2)
        return {a: (151, m2[0]), a + 1: (149, m2[1])}
    if where == "one mate":
        return {n // 3: (151, L2), n // 3 + 1: (149, L2)}
    if where == "across a triple":                    # reads 2 and 3: the last of one triple, the first of the next
        return {2: (151, m2[0]), 3: (149, m2[1])}
    raise ValueError(where)


@pytest.mark.parametrize("where", ["first", "last", "middle", "one mate", "across a triple"])
def test_compensating_lengths(oracle, monkeypatch, where):
    P = Pair(oracle, monkeypatch)
    for L2 in (150, 0):
        first = True
        for n in [s for s in SIZES if s >= (4 if where == "across a triple" else 2)]:
            P.run(make_batch(300, n, 150, L2), 0 if first else 1, (where, L2, n, "uniform"))
            first = False
            P.run(make_batch(301, n, 150, L2, lens=compensating(n, where, L2)), 2, (where, L2, n, "compensating"))
            P.run(make_batch(302, n, 150, L2), 0, (where, L2, n, "uniform behind it"))
    P.close()


def test_uniform_trimmed_uniform_uniform(oracle, monkeypatch):
    P = Pair(oracle, monkeypatch)
    for L2 in (150, 0):
        for n in (193, 3001):
            rng = np.random.default_rng(n)
            cut = [(int(rng.integers(100, 151)), int(rng.integers(100, 151)) if L2 else 0) for _ in range(n)]
            P.run(make_batch(400, n, 150, L2), 0, (n, L2, "uniform"))
            P.run(make_batch(401, n, 150, L2, lens=lambda i: cut[i]), 2, (n, L2, "trimmed"))
            assert "verdict=uniform" not in P.h.last_kernel()
            P.run(make_batch(402, n, 150, L2), 0, (n, L2, "uniform behind trimmed"))
            P.run(make_batch(403, n, 150, L2), 1, (n, L2, "uniform again"))
            # (the next round starts behind a trimmed batch)
            P.run(make_batch(404, n, 150, L2, lens=lambda i: cut[i]), 2, (n, L2, "trimmed again"))
    P.close()


def test_what_ends_and_resumes_speculation(oracle, monkeypatch):
    P = Pair(oracle, monkeypatch)
    # n grows (slot_reserve grows); n = 0 in between
    P.run(make_batch(500, 64), 0, "n = 64")
    P.run(make_batch(501, 3001), 1, "n grows to 3 001")
    P.run(make_batch(502, 0), 0, "n = 0")
    P.run(make_batch(503, 193), 0, "behind n = 0")
    P.run(make_batch(504, 193), 1, "and on")
    # paired -> single -> paired
    P.run(make_batch(505, 193, 150, 0), 0, "single behind paired")
    P.run(make_batch(506, 193, 150, 0), 1, "single again")
    P.run(make_batch(507, 193), 0, "paired behind single")
    P.run(make_batch(508, 193), 1, "paired again")
    # qualities appear, and go
    P.run(make_batch(509, 193, quals=True), 0, "qualities appear")
    P.run(make_batch(510, 193, quals=True), 1, "qualities again")
    P.run(make_batch(511, 193), 0, "qualities gone")
    # another specialisation: 2 x 100 under the bound 150 (U = 5), then under the bound 100 (U = 3)
    P.run(make_batch(512, 193, 100, 100), 2, "2 x 100, bound 150")
    P.run(make_batch(513, 193, 100, 100), 1, "2 x 100, bound 150 again")
    P.run(make_batch(514, 193, 100, 100), 0, "2 x 100, bound 100", max_read_len=100)
    assert P.h.last_kernel().startswith("classify_uni_kernel<3,"), P.h.last_kernel()
    P.run(make_batch(515, 193, 100, 100), 1, "2 x 100, bound 100 again", max_read_len=100)
    # shk_count_work: never speculated, and nothing is speculated on behind it
    b = make_batch(516, 193, 100, 100)
    e = views.embed(b, views.shifts_of())
    keep, p = views.to_device(e)
    for h in (P.h, P.hn):
        before = h.gene_counts(T.N_COUNTERS)
        h.count_work(e["n"], p["seq1"], p["off1"], p["seq2"], p["off2"])
        assert h.debug_last_speculation() == 0
        assert np.array_equal(h.gene_counts(T.N_COUNTERS), before)
    del keep
    P.run(make_batch(517, 193, 100, 100), 0, "behind shk_count_work", max_read_len=100)
    P.run(make_batch(518, 193, 100, 100), 1, "and on", max_read_len=100)
    # no bound on the read length: a host round trip stands in the path anyway
    P.run(make_batch(519, 193, 100, 100), 0, "no bound", max_read_len=0)
    P.close()


def test_views_that_are_not_16_byte_aligned(oracle, monkeypatch):
    """offsets 8 bytes behind a 16-byte boundary (the check's item-by-item loop, the guard's loads), bases at byte shifts 1 ... 3"""
    P = Pair(oracle, monkeypatch)
    first = True
    for n in (3, 193, 3001):
        for s1, s2, o1, o2 in ((1, 3, 8, 8), (2, 1, 8, 0), (3, 2, 0, 8)):
            sh = views.shifts_of(s1, s2, 0, 0, o1, o2)
            P.run(make_batch(600, n), 0 if first else 1, (n, s1, s2, o1, o2, "uniform"), shifts=sh)
            first = False
            P.run(make_batch(601, n, lens=compensating(n, "first", 150)), 2, (n, s1, s2, o1, o2, "compensating"), shifts=sh)
            P.run(make_batch(602, n), 0, (n, s1, s2, o1, o2, "uniform behind it"), shifts=sh)
            P.run(make_batch(603, n), 1, (n, s1, s2, o1, o2, "uniform again"), shifts=sh)
    P.close()


def test_placement_mode_ends_speculation(oracle, monkeypatch):
    from shark_amd import capi
    P = Pair(oracle, monkeypatch, keep_positions=True)
    P.run(make_batch(700, 193), 0, "uniform")
    P.run(make_batch(701, 193), 1, "uniform again")
    for h in (P.h, P.hn):
        h.placement_enable()
    for j in range(2):
        P.run(make_batch(702 + j, 193), 0, ("placement mode", j))
        got = []
        for h in (P.h, P.hn):
            n_assoc, ptr = h.placement_last()
            got.append(capi.placements_from_device(n_assoc, ptr))
        assert got[0].tobytes() == got[1].tobytes() and len(got[0])
    for h in (P.h, P.hn):
        h.placement_enable(False)
    # (the batches in placement mode were judged by the device: the stream is still uniform)
    P.run(make_batch(704, 193), 1, "placement mode off")
    P.close()


def test_a_missed_batch_with_reads_beyond_the_bound(oracle, monkeypatch):
    """behind a uniform batch, one whose every seventh pair is 2 x 600 under max_read_len = 150: run again (the check says ragged), and
    the reads the fast kernels queued take finish_classify's path, which runs the tail once more -- the batch is counted once"""
    P = Pair(oracle, monkeypatch)
    P.run(make_batch(800, 193), 0, "uniform")
    P.run(make_batch(801, 193, lens=lambda i: (600, 600) if i % 7 == 3 else (150, 150)), 2, "long reads")
    assert P.h.timing()["last_n_long"] > 0
    P.run(make_batch(802, 193), 0, "uniform behind it")
    P.run(make_batch(803, 193), 1, "uniform again")
    P.close()
