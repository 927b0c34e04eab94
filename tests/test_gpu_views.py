"""The classify kernels on what callers may legally hand them and no other test does: device pointers into the middle of an allocation
at every byte shift (qualities at another shift than the sequence, offsets arrays on an 8-byte boundary), off[0] != 0, neighbouring
bytes that continue the gene under a read one base short of passing, reads exactly at ceil(c * len) - 1 and ceil(c * len) for c * len
just above an integer in fp64, and a slot's stale bytes behind a shorter batch.  The generators are tests/views.py; that their reads
sit where they claim is asserted on the CPU oracle in tests/test_views_cpu.py.  Everything is compared with np.array_equal.

Routes: the exact table in LDS (three pairs per staging pass with and without the tiles' round, several genes, with qualities), trimmed
batches class by class and by offsets, the LDS summary, the table modes (summary+table, table, table-mod) with the anchored extension and
anchor_verdict_kernel, plain filter words, the general kernel, 2 x 300 bp.  The minimiser-bucketed table (SHK_KTAB) is left out: how long
its smallest configuration takes to build on the device was not measured for this file, and the suite's time is a constraint.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import evidence_model, synth, views
from tests.pileup_model import expected_pileup
from tests.segments_model import SegmentsModel, expected_segments

pytestmark = pytest.mark.gpu

K, C = views.K, views.C

ALL_SWITCHES = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST", "SHK_NO_TRI",
                "SHK_NO_TRO", "SHK_CLS_MIN_FILL", "SHK_ANCHOR_ALWAYS", "SHK_NO_ANCHOR", "SHK_NO_REFEXT", "SHK_NO_PRE_VERDICT", "SHK_NO_SPARSE", "SHK_FORCE_TRO")
TABLE = {"SHK_NO_LDS_SUMMARY": "1", "SHK_ANCHOR_ALWAYS": "1"}


class Route:
    def __init__(self, name, env, mode=("lds-table",), uniform=(), not_uniform=(), trimmed=()):
        self.name, self.env, self.mode = name, env, mode
        self.n_genes, self.bf_bits, self.q, self.shapes = views.ROUTE_REFS[name]      # (shared with tests/test_views_cpu.py)
        self.uniform, self.not_uniform, self.trimmed = uniform, not_uniform, trimmed     # what last_kernel() must (not) say for such a batch

    def enter(self, monkeypatch):
        for v in ALL_SWITCHES:
            monkeypatch.delenv(v, raising=False)
        for name, v in self.env.items():
            monkeypatch.setenv(name, v)

    def build(self, oracle, c=C, k=K, evidence=False):
        genes = views.reference(self.n_genes)
        o = _oracle(oracle, self.n_genes, k, c, self.bf_bits, self.q)
        from shark_amd import SharkHip
        h = SharkHip(k=k, c=c, bf_bits=self.bf_bits, min_quality=self.q)
        h.build([bytes(g) for g in genes])
        if evidence:
            h.evidence_enable(True)
        else:
            assert h.probe_mode() in self.mode, (self.name, h.probe_mode())
        return genes, o, h

    def said(self, h, kind):
        """the route ran: what shk_last_kernel reports for a uniform / trimmed batch"""
        lk = h.last_kernel()
        if kind == "uniform":
            for s in self.uniform:
                assert s in lk, (self.name, s, lk)
            for s in self.not_uniform:
                assert s not in lk, (self.name, s, lk)
        else:
            for s in self.trimmed:
                assert s in lk, (self.name, s, lk)


UNI_TABLE = ("classify_uni_kernel", "+anchored-extension", "+pre-verdict")      # (uniform and trimmed batches alike)
ROUTES = [
    Route("three-pairs+tiles", {"SHK_TILE_FIRST": "1"}, uniform=("+three-pairs", "+tiles-first"), trimmed=("offsets", "+tiles-first")),
    Route("three-pairs", {"SHK_TILE_FIRST": "0"}, uniform=("+three-pairs",), not_uniform=("+tiles-first",), trimmed=("offsets",)),
    Route("several-genes", {}, uniform=(", 21, ", "+sparse-first-rounds"), trimmed=("classify_uni_kernel",)),
    Route("exact-table-q", {}, uniform=(", true, 21, ",), not_uniform=("+three-pairs",), trimmed=("classify_uni_kernel", ", true, 21, ")),
    Route("class-by-class", {"SHK_CLS_MIN_FILL": "1", "SHK_NO_TRO": "1"}, uniform=(", 21, ",), trimmed=("verdict=classes",)),
    Route("lds-summary", {"SHK_NO_LDS_TABLE": "1"}, mode=("lds-summary+table",), uniform=("classify_uni_kernel",), trimmed=("classify_uni_kernel",)),
    Route("summary+table", TABLE, mode=("summary+table", "table"), uniform=UNI_TABLE, trimmed=UNI_TABLE),
    Route("table", dict(TABLE, SHK_NO_SUMMARY="1"), mode=("table",), uniform=UNI_TABLE, trimmed=UNI_TABLE),
    Route("table-q", dict(TABLE, SHK_NO_SUMMARY="1"), mode=("table",), uniform=UNI_TABLE, trimmed=UNI_TABLE),
    Route("table-mod", dict(TABLE, SHK_NO_SUMMARY="1"), mode=("table-mod",), uniform=UNI_TABLE, trimmed=UNI_TABLE),
    Route("table-mod-q", dict(TABLE, SHK_NO_SUMMARY="1"), mode=("table-mod",), uniform=UNI_TABLE, trimmed=UNI_TABLE),
    Route("bit-vector", {"SHK_PROBE": "bitvector"}, mode=("bitvector", "summary+bitvector"), uniform=("classify_fast_kernel",), trimmed=("classify_fast_kernel",)),
    Route("2x300", {}, uniform=("classify_uni_kernel<10, ",), trimmed=("classify_uni_kernel<10, ",)),
    Route("2x300-table", TABLE, mode=("summary+table", "table"), uniform=("classify_uni_kernel<10, ", "+anchored-extension"),
          trimmed=("classify_uni_kernel<10, ", "+anchored-extension")),
]
assert [r.name for r in ROUTES] == list(views.ROUTE_REFS)
BY_NAME = {r.name: r for r in ROUTES}

# (seq1, seq2) shifts; the qualities sit at (seq1 + 1, seq2 + 2) mod 4, the offsets arrays at +0 / +8 in turn; last the aligned control
SHIFTS = [views.shifts_of(s1, s2, (s1 + 1) % 4, (s2 + 2) % 4, o1, o2) for (s1, s2), (o1, o2) in
          zip(((0, 0), (1, 3), (2, 1), (3, 2)), ((0, 8), (8, 0), (8, 8), (0, 8)))] + [views.shifts_of()]

_oracles = {}


def _oracle(oracle, n_genes, k, c, bf_bits, q):
    key = (n_genes, k, c, bf_bits, q)
    if key not in _oracles:
        o = oracle.Shark(k=k, c=c, bf_bits=bf_bits, min_quality=q)
        o.build([bytes(g) for g in views.reference(n_genes)])
        _oracles[key] = o
    return _oracles[key]


def _args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"]


def _read_back(r):
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    capi.hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        capi.hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    return goff, gids


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "gene_off differs at read %d" % int(np.argmax(got[0][:len(want[0])] != want[0])))
    assert np.array_equal(got[1], want[1]), what


def _max_len(batch):
    m = int(np.diff(batch["off1"].astype(np.int64)).max())
    return max(m, int(np.diff(batch["off2"].astype(np.int64)).max())) if batch["off2"] is not None else m


def _resident(h, batch, shifts, lead=None, trail=None, **kw):
    """classify_device on the embedded view; returns (gene_off, gene_ids)"""
    e = views.embed(batch, shifts, lead, trail)
    keep, p = views.to_device(e)
    r = h.classify_device(e["n"], p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"], max_read_len=_max_len(batch), **kw)
    out = _read_back(r)
    del keep
    return out


# ---------------------------------------------------------------------------
# 1. resident views on every route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.name)
def test_resident_views_on_every_route(oracle, monkeypatch, route):
    """ordinary reads + a ladder + hostile reads next to their neighbours, uniform and trimmed, resident in HBM at every byte shift of the
    sequences, the qualities at other shifts, the offsets arrays on 8-byte boundaries, between bytes that continue the gene under the
    batch's first and last read: shk_classify_device and shk_classify_device_submit / wait (three in flight; uniform batches with
    and without the caller's word for the lengths) return the oracle's associations, and the intended kernel ran"""
    route.enter(monkeypatch)
    genes, o, h = route.build(oracle)
    for L1, L2 in route.shapes:
        for trimmed in (False, True):
            batch, marked, lead, trail = views.mixed_case(genes, K, C, L1, L2, qual=route.q > 0, trimmed=trimmed)
            n = len(batch["off1"]) - 1
            assert 300 <= n <= 700 and len(marked) >= 10
            want = o.classify(*_args(batch), nthreads=2)
            assert 0 < int(want[0][-1]) < n
            kind = "trimmed" if trimmed else "uniform"
            _same(h.classify(*_args(batch)), want, (route.name, L1, L2, kind, "host"))
            route.said(h, kind)
            for j, sh in enumerate(SHIFTS):
                _same(_resident(h, batch, sh, lead, trail), want, (route.name, L1, L2, kind, "classify_device", sh))
                route.said(h, kind)
                assert ("verdict=uniform" in h.last_kernel()) == (not trimmed) or "classify_uni_kernel" not in h.last_kernel(), h.last_kernel()
            # the pipelined entry point, SHK_PIPE_DEPTH views in flight
            for first in range(0, len(SHIFTS), capi.SHK_PIPE_DEPTH):
                keep, tickets = [], []
                for j, sh in list(enumerate(SHIFTS))[first:first + capi.SHK_PIPE_DEPTH]:
                    e = views.embed(batch, sh, lead, trail)
                    t, p = views.to_device(e)
                    keep.append(t)
                    vouch = (not trimmed) and j % 2 == 0
                    tickets.append(h.submit_device(n, p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"], max_read_len=max(L1, L2),
                                                   uniform_len1=L1 if vouch else 0, uniform_len2=L2 if vouch else 0))
                for t in tickets:
                    _same(_read_back(h.wait_device(t)), want, (route.name, L1, L2, kind, "submit_device"))
                    route.said(h, kind)
    h.close()


def test_general_kernel_on_views(oracle, monkeypatch):
    """a few mates of 1 500 bases next to short ones: the long ones take the general kernel, from a view as from a whole allocation"""
    route = BY_NAME["table"]
    route.enter(monkeypatch)
    genes, o, h = route.build(oracle)
    batch, marked, lead, trail = views.mixed_case(genes, K, C, 150, 150, trimmed=True)
    reads = views.reads_of(batch)
    rng = np.random.default_rng(15)
    for j in (3, len(reads) // 2, len(reads) - 2):
        g = genes[j % len(genes)]
        long1 = np.resize(g, 1500).copy()
        long1[700:720] = synth.random_seq(rng, 20)
        reads[j] = (long1, synth.revcomp(g[:900]).copy(), None, None)
    batch = views.batch_of(reads)
    want = o.classify(*_args(batch), nthreads=2)
    _same(h.classify(*_args(batch)), want, "host")
    assert h.timing()["last_n_long"] == 3
    for sh in SHIFTS:
        _same(_resident(h, batch, sh, lead, trail), want, ("classify_device", sh))
        assert h.timing()["last_n_long"] == 3
    h.close()


# ---------------------------------------------------------------------------
# 2. exact thresholds on every route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.name)
def test_exact_thresholds_on_every_route(oracle, monkeypatch, route):
    """reads of designed coverage ceil(c * len) - 2 ... + 1 for products c * len that fp64 puts just above (below, on) an integer; with N
    and bases under -q outside the stretch (len and the threshold drop); uniform and ragged; host batches and resident views: the
    oracle's associations on every route"""
    route.enter(monkeypatch)
    qual = route.q > 0
    for c, length in views.pairs_of(route.name):
        genes, o, h = route.build(oracle, c=c)
        for k, _, _, invalid, ragged in [case for case in views.threshold_cases(route.name) if case[1:3] == (c, length)]:
            batch, design = views.ladder_case(genes, k, c, length, qual=qual, invalid=invalid, ragged=ragged)
            want = o.classify(*_args(batch), nthreads=2)
            n_pass = int((np.diff(want[0].astype(np.int64)) > 0).sum())
            assert 0 < n_pass < len(design)
            what = (route.name, c, length, invalid, ragged)
            _same(h.classify(*_args(batch)), want, what + ("host",))
            if not ragged and length in (300, 600):          # (2 x 150 and 2 x 300: the shapes the routes' kernels are named for)
                route.said(h, "uniform")
            _same(h.wait(h.submit(*_args(batch))), want, what + ("submit",))
            _same(_resident(h, batch, SHIFTS[1 + (int(invalid) + 2 * int(ragged)) % 3]), want, what + ("resident",))
        h.close()


@pytest.mark.parametrize("k,c,length", views.EVIDENCE_PAIRS)
def test_exact_thresholds_in_evidence_mode(oracle, monkeypatch, k, c, length):
    """ladder batches in evidence mode: (cov, nk, len) per read equal the oracle's numbers -- a leak that does not flip a decision still
    shows in them -- on indices in LDS and on table indices, with and without qualities, host batches and resident views"""
    from shark_amd import SharkHip
    cases = views.evidence_cases(k, c, length)
    for name in dict.fromkeys(case[0] for case in cases):
        route = BY_NAME[name]
        route.enter(monkeypatch)
        genes = views.reference(route.n_genes)
        o = _oracle(oracle, route.n_genes, k, c, route.bf_bits, route.q)
        h = SharkHip(k=k, c=c, bf_bits=route.bf_bits, min_quality=route.q)
        h.build([bytes(g) for g in genes])
        h.evidence_enable(True)
        for _, invalid, ragged in [case for case in cases if case[0] == name]:
            batch, design = views.ladder_case(genes, k, c, length, qual=route.q > 0, invalid=invalid, ragged=ragged)
            n = len(design)
            want = o.classify(*_args(batch), nthreads=2)
            ev = evidence_model.expected_evidence(o, batch)
            assert np.array_equal(ev[:, 2], [d[1] for d in design])
            _same(h.classify(*_args(batch)), want, (name, "host"))
            assert np.array_equal(h.evidence_last(), ev), (name, invalid, ragged, "host")
            e = views.embed(batch, SHIFTS[2 if invalid else 1])
            keep, p = views.to_device(e)
            r = h.classify_device(n, p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"], max_read_len=_max_len(batch))
            _same(_read_back(r), want, (name, "resident"))
            got = np.zeros((n, 3), np.uint32)
            capi.hip_memcpy_dtoh(got, h.evidence_last(), got.nbytes)
            assert np.array_equal(got, ev), (name, invalid, ragged, "resident")
        h.close()


# ---------------------------------------------------------------------------
# 3. uniform_check_kernel with offsets arrays on an 8-byte boundary
# ---------------------------------------------------------------------------
def test_uniform_check_with_offsets_on_an_8_byte_boundary(oracle, monkeypatch):
    """offsets arrays that start 8 bytes into an allocation take uniform_check_kernel's narrow body (one read per lane, the next offset from
    the neighbouring lane, lane 63's from memory): batch sizes on either side of its wave (64) and workgroup (1 024) edges, all reads
    equal or one a base shorter at those edges, in either mate, off1 / off2 / both displaced: the oracle's associations and the verdict
    of the aligned run of the same batch"""
    BY_NAME["class-by-class"].enter(monkeypatch)    # (SHK_NO_TRO=1 as in test_device_side_uniformity_check_finds_the_one_odd_read; SHK_CLS_MIN_FILL=1:
    #                                                   the verdict on a batch does not depend on the batch before it)
    L = 61
    rng = np.random.default_rng(2049)
    genes = views.reference(1)
    o = _oracle(oracle, 1, K, 0.5, 1 << 30, 0)
    from shark_amd import SharkHip
    h = SharkHip(k=K, c=0.5, bf_bits=1 << 30)
    h.build([bytes(g) for g in genes])
    assert h.probe_mode() == "lds-table"
    base = views.reads_of(synth.make_reads(rng, genes, 2049, read_len=L, paired=True, on_target=0.7))
    placements = [views.shifts_of(1, 2, 0, 0, o1, o2) for o1, o2 in ((0, 0), (8, 0), (0, 8), (8, 8))]
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049):
        for odd in [None] + sorted({i for i in (0, 63, 64, 1023, 1024, n - 1) if i < n}):
            for mate in ((0,) if odd is None else (0, 1)):
                reads = list(base[:n])
                if odd is not None:
                    r = list(reads[odd])
                    r[mate] = r[mate][:-1]
                    reads[odd] = tuple(r)
                batch = views.batch_of(reads)
                want = o.classify(*_args(batch), nthreads=2)
                verdicts = []
                for sh in placements:
                    _same(_resident(h, batch, sh), want, (n, odd, mate, sh["off1"], sh["off2"]))
                    verdicts.append(h.last_kernel().split("verdict=")[-1])
                assert len(set(verdicts)) == 1, (n, odd, mate, verdicts)
                assert (verdicts[0] == "uniform") == (odd is None or n == 1), (n, odd, mate, verdicts)      # (one read alone has one length)
    h.close()


# ---------------------------------------------------------------------------
# 4. off[0] != 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three-pairs", "table", "exact-table-q"])
def test_first_offset_not_zero(oracle, monkeypatch, name):
    """reads of one length per mate whose first offset is not 0 do not lie at i * L: the batch must not be read in the uniform layout.  Hostile
    bytes in [0, off[0]); host batches (classify, submit / wait) and resident ones"""
    route = BY_NAME[name]
    route.enter(monkeypatch)
    genes, o, h = route.build(oracle)
    batch, marked, lead, trail = views.mixed_case(genes, K, C, 150, 150, qual=route.q > 0)
    want = o.classify(*_args(batch), nthreads=2)

    def not_uniform():
        lk = h.last_kernel()
        assert "verdict=uniform" not in lk and ", true>" not in lk, lk

    for o1, o2 in ((1, 0), (0, 5), (8, 8), (150, 0), (0, 150), (150, 150), (5, 1)):
        b = views.with_first_offset(batch, o1, o2, lead)
        assert np.array_equal(o.classify(*_args(b), nthreads=2)[0], want[0])
        what = (name, o1, o2)
        _same(h.classify(*_args(b)), want, what + ("classify",))
        not_uniform()
        tickets = [h.submit(*_args(b)) for _ in range(capi.SHK_PIPE_DEPTH)]
        for t in tickets:
            _same(h.wait(t), want, what + ("submit",))
        _same(_resident(h, b, SHIFTS[4]), want, what + ("resident",))
        not_uniform()
        _same(_resident(h, b, SHIFTS[1], trail=trail), want, what + ("resident view",))
        not_uniform()
    h.close()


# ---------------------------------------------------------------------------
# 5. a slot's stale bytes behind a shorter host batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", views.STALE_ROUTES)
def test_stale_bytes_behind_a_host_batch(oracle, monkeypatch, name):
    """the slots' device buffers keep an earlier batch's bytes behind the current batch's end.  Batch A = batch B + reads whose first bytes
    continue the gene under B's last read (one base short of passing, flush with its mates' ends): after A has passed through every
    slot, B's results are still the oracle's -- uniform and trimmed, classify and three deep with submit / wait"""
    route = BY_NAME[name]
    route.enter(monkeypatch)
    genes, o, h = route.build(oracle)
    qual = route.q > 0
    for trimmed in (False, True):
        B, marked, lead, trail = views.mixed_case(genes, K, C, 150, 150, qual=qual, trimmed=trimmed, seed=5)
        rb = views.reads_of(B)
        assert marked[-1][0] == len(rb) - 1 and marked[-1][2] == "end"
        rng = np.random.default_rng(55)
        extra = views.reads_of(synth.make_reads(rng, genes, 40, read_len=150, paired=True, on_target=0.5, qual=qual))
        first = list(extra[0])
        for t in (0, 1):
            first[t] = first[t].copy()
            first[t][:len(trail[t])] = trail[t]
            if qual:                                   # (phred 40 over the continuation: -q must not hide a leaked base)
                first[2 + t] = first[2 + t].copy()
                first[2 + t][:len(trail[t])] = views.HI_Q
        extra[0] = tuple(first)
        A = views.batch_of(rb + extra)
        assert np.array_equal(A["seq1"][len(B["seq1"]):len(B["seq1"]) + len(trail[0])], trail[0])
        assert np.array_equal(A["seq2"][len(B["seq2"]):len(B["seq2"]) + len(trail[1])], trail[1])
        want_a, want_b = o.classify(*_args(A), nthreads=2), o.classify(*_args(B), nthreads=2)
        assert want_b[0][-1] == want_b[0][-2]          # B's last read does not pass
        for _ in range(capi.SHK_PIPE_DEPTH):
            _same(h.classify(*_args(A)), want_a, (name, trimmed, "A"))
        for _ in range(capi.SHK_PIPE_DEPTH):
            _same(h.classify(*_args(B)), want_b, (name, trimmed, "B"))
        for batch, want in ((A, want_a), (B, want_b)):
            tickets = [h.submit(*_args(batch)) for _ in range(capi.SHK_PIPE_DEPTH)]
            for t in tickets:
                _same(h.wait(t), want, (name, trimmed, "submit"))
    h.close()


# ---------------------------------------------------------------------------
# 6. the positional modes on a view
# ---------------------------------------------------------------------------
def test_positional_modes_on_a_view(oracle):
    """placement, segments (m = 4), depth, spliced depth, the junction table and pileup on one resident batch with qualities under -q 20:
    sequences at shifts (1, 3), qualities at (2, 1), offsets arrays at +8 -- every record and every accumulated array equals those of the
    same batch run from aligned buffers in a second context, and the pileup (which reads the mates' bytes and the quality mask itself)
    equals the model's"""
    from shark_amd import SharkHip
    from tests.spliced_synth import spliced_gene, spliced_reads
    rng = np.random.default_rng(2025)
    panel = [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]
    records = [bytes(g) for g, _ in panel]
    batch = spliced_reads(np.random.default_rng(66), panel, 400, ragged=True, sub=0.03, qual=True, lower=0.1)
    n = len(batch["off1"]) - 1
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 26, min_quality=20)
    o.build(records)
    sm = SegmentsModel(records, 17)
    seen = []
    for sh in (views.shifts_of(), views.shifts_of(1, 3, 2, 1, 8, 8)):
        h = SharkHip(k=17, c=0.0, bf_bits=1 << 26, min_quality=20)
        h.build(records, keep_positions=True)
        h.placement_enable(True)
        h.segments_enable(4)
        h.junctions_enable(8, 1024)
        h.pileup_enable(8)
        rows = []
        for spliced in (False, True):
            if spliced:
                h.depth_reset()
                h.depth_enable(0)
                h.depth_enable_spliced(8)
            else:
                h.depth_enable(1)
            e = views.embed(batch, sh)
            keep, p = views.to_device(e)
            r = h.classify_device(n, p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"], max_read_len=120)
            goff, gids = _read_back(r)
            na, m, kp, ep = h.segments_last()
            keys, segs = capi.segments_from_device(na, m, kp, ep)
            pn, pp = h.placement_last()
            pl = capi.placements_from_device(pn, pp)
            assert na == pn == len(gids) > n // 2
            assert h.depth_all().any() and h.depth_mates() > 0
            rows.append((goff.tobytes(), gids.tobytes(), keys.tobytes(), segs.tobytes(), pl.tobytes(), h.depth_all().tobytes(), h.depth_mates(),
                         h.depth_summary().tobytes()))
            if not spliced:
                _same((goff, gids), o.classify(*_args(batch), nthreads=2), "genes")
                want_rows = expected_segments(sm, batch, goff, gids, 4, 20)[1]
                assert np.array_equal(segs, want_rows)
                counts, lost, mates = expected_pileup(sm, batch, goff, gids, want_rows, 8, 20)
                assert np.array_equal(h.pileup_all(), counts) and h.pileup_mates() == mates and counts.any() and lost.any()
        junc = h.junctions_get()
        assert len(junc) > 0 and (junc["mates"] > 0).all()
        seen.append((rows, junc.tobytes(), h.pileup_all().tobytes(), h.pileup_mates()))
        h.close()
    assert seen[0] == seen[1]
    assert len(seen[0][1]) > 0
