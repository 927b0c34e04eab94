"""Spliced depth on the GPU (shk_depth_enable_spliced and depth mode's read-outs, `shark --depth --depth-spliced`): the accumulated
per-base depth, its summary and the mate counter -- whole arrays, np.array_equal -- against the model (tests/spliced_model.py), which
ORs a boolean mask per mate over its kept spans and shares no idea with the kernel.  The model is fed the GPU's own gene_off /
gene_ids, which are compared with the CPU oracle's first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import synth
from tests.depth_model import depth_lines, depth_summary, expected_depth, model_layout
from tests.segments_model import SegmentsModel, expected_segments, mate_lengths
from tests.spliced_model import add_to_table, expected_spliced_depth, table_rows
from tests.spliced_synth import spliced_gene, spliced_reads  # noqa: F401  (other test modules import them from here)
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# (references and reads: tests/spliced_synth.py)
def build(oracle, records, **kw):
    from shark_amd import SharkHip
    kw.setdefault("c", 0.0)
    kw.setdefault("bf_bits", 1 << 26)
    k = kw.setdefault("k", 17)
    o = oracle.Shark(k=k, c=kw["c"], bf_bits=kw["bf_bits"], min_quality=kw.get("min_quality", 0))
    nidx = o.build([bytes(g) for g in records])
    h = SharkHip(**kw)
    assert h.build([bytes(g) for g in records], keep_positions=True)["nidx"] == nidx
    return o, h, SegmentsModel([bytes(g) for g in records], k)


class Expected:
    """what the state must hold after the batches added so far: depth, mates, the junction table"""

    def __init__(self, sm, s_depth=8, s_junc=8, q=0):
        self.sm, self.s_depth, self.s_junc, self.q = sm, s_depth, s_junc, q
        self.reset()

    def reset(self):
        self.depth = np.zeros(int(model_layout(self.sm)[-1]), dtype=np.uint32)
        self.mates = 0
        self.table = {}
        self.overlapping = 0        # mates whose kept spans overlap in record coordinates
        self.n_spans = np.zeros(5, dtype=np.int64)   # mates by their number of kept spans

    def add(self, o, batch, goff, gids, times=1):
        og, oi = o.classify(*_args(batch))
        assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
        rows = expected_segments(self.sm, batch, goff, gids, 4, self.q)[1]
        d, m = expected_spliced_depth(self.sm, batch, goff, gids, rows, self.s_depth)
        self.depth += np.uint32(times) * d
        self.mates += times * m
        for _ in range(times):
            add_to_table(self.table, batch, goff, gids, rows, self.sm.k, self.s_junc)
        lengths = mate_lengths(batch)
        read_of = np.repeat(np.arange(len(goff) - 1), np.diff(goff))
        for j in range(len(gids)):
            for t in range(2):
                sp = capi.kept_spans(rows[j, t], int(lengths[read_of[j], t]), self.sm.k, self.s_depth)
                self.n_spans[len(sp)] += 1
                self.overlapping += any(b[0] < a[1] for a, b in zip(sp, sp[1:]))
        return d, m

    def check_depth(self, h):
        gs = h.depth_layout()
        assert np.array_equal(gs, model_layout(self.sm, h.index_info()["nidx"]))
        got = h.depth_all()
        assert got.dtype == np.uint32 and got.shape == self.depth.shape
        bad = np.nonzero(got != self.depth)[0]
        assert len(bad) == 0, "base %d: got %d, model %d (%d differ)" % (bad[0], got[bad[0]], self.depth[bad[0]], len(bad))
        assert h.depth_mates() == self.mates
        s = h.depth_summary()
        assert [tuple(int(v) for v in (r["len"], r["covered"], r["max"], r["sum"])) for r in s] == depth_summary(self.depth, gs)
        return got

    def check_table(self, h):
        got = [tuple(int(v) for v in r) for r in h.junctions_get()]
        assert got == table_rows(self.table), (got[:5], table_rows(self.table)[:5])
        return got


def device_assoc(r):
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    capi.hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        capi.hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    return goff, gids


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 17, 31])
@pytest.mark.parametrize("ref", ["one gene", "two genes", "twins"])
def test_spliced_mates_strands_indels_and_ties(oracle, k, ref):
    """mates over 0 to 5 junctions on both strands, with a deletion and with a repeat (overlapping record spans: each base once);
    one gene, two genes, and two identical genes (every read tied over both)"""
    rng = np.random.default_rng(1000 + 10 * k + len(ref))
    genes = [spliced_gene(rng, 4, k)] if ref == "one gene" else [spliced_gene(rng, 1 + i, k) for i in range(2)]
    if ref == "twins":
        genes = [genes[1], genes[1]]
    s_min = 3 if k == 5 else 8
    o, h, sm = build(oracle, [g for g, _ in genes], k=k)
    want = Expected(sm, s_min, s_min)
    h.depth_enable_spliced(s_min)
    batch = spliced_reads(rng, genes, 150)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    got = want.check_depth(h)
    assert want.mates > 100 and want.n_spans[2:].sum() > (40 if k <= 17 else 5) and got.any()          # (not vacuous: spliced mates were counted)
    if k <= 17:
        assert want.overlapping >= 1 and (ref != "one gene" or want.n_spans[4] >= 5)
    if ref == "twins":
        n = len(genes[0][0])
        assert np.array_equal(got[:n], got[n:]) and int(goff[-1]) > 150
    # the spliced depth is not the plain one: plain depth paints the introns
    plain, _ = expected_depth(sm, batch, goff, gids, s_min)
    assert not np.array_equal(plain, got)
    h.depth_reset()
    want.reset()
    want.check_depth(h)


def test_a_span_ending_at_the_record_end_leaves_the_next_gene_alone(oracle):
    rng = np.random.default_rng(3)
    genes = [spliced_gene(rng, 2, 17) for _ in range(2)]
    rec, tr = genes[0]
    o, h, sm = build(oracle, [g for g, _ in genes], k=17)
    want = Expected(sm)
    h.depth_enable_spliced(8)
    batch = synth.batch_from_lists([tr[-100:].copy() for _ in range(3)], [synth.revcomp(rec[-70:]) for _ in range(3)])
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    got = want.check_depth(h)
    n = len(rec)
    assert want.mates == 6 and got[n - 1] == 6 and not got[n:].any() and got[n - 70 - 20:n - 70 - 10].sum() == 0          # (the last intron stays empty)
    assert h.depth(0).tolist() == got[:n].tolist() and not h.depth(1).any()


# ---------------------------------------------------------------------------
# batch sizes, the four families, the repair paths
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(2025)
    return [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes_ragged_and_uniform(oracle, panel, n):
    rng = np.random.default_rng(7 * n)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    want = Expected(sm)
    h.depth_enable_spliced(8)
    for ragged, paired in ((False, True), (True, True), (True, False)):
        batch = spliced_reads(rng, panel, n, paired=paired, ragged=ragged)
        want.add(o, batch, *h.classify(*_args(batch)))
        want.check_depth(h)


def test_all_four_families_accumulate_and_reset(oracle, panel):
    rng = np.random.default_rng(53)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    batches = [spliced_reads(rng, panel, n, ragged=r) for n, r in ((200, False), (65, True), (150, True))]
    dev = [_to_device(b) for b in batches]

    def host(i):
        return h.classify(*_args(batches[i]))

    def resident(i):
        return device_assoc(h.classify_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i])))

    def resident_submit(i):
        return device_assoc(h.wait_device(h.submit_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i]))))

    want = Expected(sm, 6, 8)
    h.depth_enable_spliced(6)
    h.junctions_enable(8, 1024)
    total = None
    for family in (host, "pipeline", resident, resident_submit):
        if family == "pipeline":
            results = [h.wait(t) for t in [h.submit(*_args(b)) for b in batches]]
        else:
            results = [family(i) for i in range(3)]
        if total is None:
            for b, (goff, gids) in zip(batches, results):
                want.add(o, b, goff, gids)
            total = (want.depth.copy(), want.mates, {key: list(v) for key, v in want.table.items()})
        else:                                                   # (the model's answer for a batch is computed once)
            for b, (goff, gids) in zip(batches, results):
                og, oi = o.classify(*_args(b))
                assert np.array_equal(og, goff) and np.array_equal(oi, gids)
        got = want.check_depth(h)
        want.check_table(h)
        assert got.any() and len(want.table) > 10
        t = torch.zeros(len(got), dtype=torch.int32, device="cuda:0")
        assert h.depth_all(device_ptr=t.data_ptr()) == len(got)
        assert np.array_equal(t.cpu().numpy().view(np.uint32), got)
        h.depth_reset()
        h.junctions_reset()
        assert not h.depth_all().any() and h.depth_mates() == 0 and len(h.junctions_get()) == 0


def test_length_bound_repair_counts_once(oracle):
    """mates of 3 000 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again): counted there, and only there"""
    rng = np.random.default_rng(29)
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, sm = build(oracle, long_genes, k=17)
    want = Expected(sm)
    h.depth_enable_spliced(8)
    h.junctions_enable(8, 256)
    mates = [np.concatenate([long_genes[i % 3][20 * i:20 * i + (1500 if i % 5 == 0 else 50)], long_genes[i % 3][2000 + 20 * i:2000 + 20 * i + (1500 if i % 5 == 0 else 50)]])
             for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    goff, gids = device_assoc(h.wait_device(h.submit_device(40, max_read_len=100, **_dev_ptrs(t))))
    assert h.timing()["last_n_long"] > 0
    want.add(o, b, goff, gids)
    got = want.check_depth(h)
    want.check_table(h)
    assert want.mates == 80 and got[0] == 2 and sum(v[1] for v in want.table.values()) == 80
    b2 = synth.batch_from_lists([long_genes[0][100:160], long_genes[1][50:150]])
    want.add(o, b2, *h.classify(*_args(b2)))
    want.check_depth(h)


def test_association_overflow_repair_counts_once(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 reads tied over 6 identical genes"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    o, h, sm = build(oracle, [twin.copy() for _ in range(6)], k=17)
    want = Expected(sm)
    h.depth_enable_spliced(8)
    h.junctions_enable(8, 4096)
    reads = [np.concatenate([twin[(7 * i) % 200:(7 * i) % 200 + 50], twin[300 + (7 * i) % 200:350 + (7 * i) % 200]]) for i in range(3000)]
    batch = synth.batch_from_lists(reads)
    goff, gids = h.classify(*_args(batch))
    assert int(goff[-1]) == 18000
    want.add(o, batch, goff, gids)
    got = want.check_depth(h)
    want.check_table(h)
    assert want.mates == 18000 and all(np.array_equal(got[:600], got[600 * g:600 * g + 600]) for g in range(1, 6))
    assert sum(v[1] for v in want.table.values()) == 18000


# ---------------------------------------------------------------------------
# masks, the numbering quirk
# ---------------------------------------------------------------------------
def test_quality_mask_and_lower_case(oracle, panel):
    rng = np.random.default_rng(11)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17, min_quality=20)
    want = Expected(sm, 8, 8, q=20)
    h.depth_enable_spliced(8)
    h.junctions_enable(8, 1024)
    for paired, ragged in ((True, False), (False, True)):
        batch = spliced_reads(rng, panel, 200, paired=paired, ragged=ragged, qual=True, lower=0.2)
        want.add(o, batch, *h.classify(*_args(batch)))
    want.check_depth(h)
    want.check_table(h)
    assert want.mates > 100 and len(want.table) > 10


def test_record_numbering_quirk(oracle):
    """an all-N record (does not advance the counter), records shorter than k (advance it, carry nothing): their ids have length 0"""
    rng = np.random.default_rng(19)
    g = [spliced_gene(rng, 2, 17) for _ in range(4)]
    records = [np.full(60, ord("N"), np.uint8), g[0][0], synth.random_seq(rng, 9), g[1][0], np.full(40, ord("N"), np.uint8), g[2][0], g[3][0], synth.random_seq(rng, 5)]
    o, h, sm = build(oracle, records, k=17)
    assert sorted(sm.records) == [0, 2, 3, 4] and h.index_info()["nidx"] == 6
    want = Expected(sm)
    h.depth_enable_spliced(8)
    h.junctions_enable(8, 64)
    batch = spliced_reads(rng, g, 200)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    want.check_depth(h)
    got = want.check_table(h)
    assert want.mates > 100 and {r[0] for r in got} == {0, 2, 3, 4} and len(h.depth(1)) == 0


# ---------------------------------------------------------------------------
# state rules, inertness
# ---------------------------------------------------------------------------
def test_state_rules(oracle, panel):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    records = [g for g, _ in panel]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError):
        h.depth_enable_spliced(8)                 # before finalize
    h.depth_enable_spliced(0)                     # (switching off is always allowed)
    h.build([bytes(g) for g in records])
    with pytest.raises(SharkHipError):
        h.depth_enable_spliced(8)                 # finalized without keep_positions
    o, h, sm = build(oracle, records, k=17)
    want = Expected(sm)
    b = spliced_reads(rng, panel, 50)
    # plain <-> spliced: free on a clean state, refused on a dirty one, free again behind a reset
    h.depth_enable(1)
    h.depth_enable_spliced(8)
    goff, gids = h.classify(*_args(b))
    want.add(o, b, goff, gids)
    with pytest.raises(SharkHipError, match="other kind"):
        h.depth_enable(1)
    h.depth_enable(0)                             # off: either kind
    with pytest.raises(SharkHipError, match="other kind"):
        h.depth_enable(1)
    h.depth_enable_spliced(8)
    want.check_depth(h)
    h.depth_reset()
    h.depth_enable(1)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError, match="other kind"):
        h.depth_enable_spliced(8)
    h.depth_reset()
    h.depth_enable_spliced(8)
    h.classify(*_args(b))
    want.check_depth(h)
    # tickets outstanding
    tk = h.submit(*_args(b))
    for call in (lambda: h.depth_enable_spliced(8), lambda: h.depth_enable_spliced(0), h.depth_all, h.depth_reset):
        with pytest.raises(SharkHipError):
            call()
    h.wait(tk)
    want.add(o, b, goff, gids)
    want.check_depth(h)
    # shk_count_work's batch and a wrongly vouched batch count nothing
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    ub = spliced_reads(rng, panel, 64, ragged=False)
    t = _to_device(ub)
    tk = h.submit_device(64, max_read_len=120, uniform_len1=99, uniform_len2=99, **_dev_ptrs(t))
    with pytest.raises(SharkHipError):
        h.wait_device(tk)
    want.check_depth(h)
    # a wider index than ids can name
    wide = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    wide.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_positions=True)
    with pytest.raises(SharkHipError, match="65 536"):
        wide.depth_enable_spliced(8)


def test_modes_are_inert_and_plain_depth_is_unchanged(oracle, panel):
    """with both new modes on, every other result is what it is with them off; segments at m = 2 is handed out at m = 2; plain depth
    gives the depth model's answer"""
    from shark_amd import SharkHip
    rng = np.random.default_rng(41)
    records = [g for g, _ in panel]
    batches = [spliced_reads(rng, panel, 300, ragged=False), spliced_reads(rng, panel, 300, ragged=True)]
    seen = []
    for new in (False, True):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in records], keep_positions=True)
        h.evidence_enable(True)
        h.candidates_enable(4)
        h.placement_enable(True)
        h.segments_enable(2)
        if new:
            h.depth_enable_spliced(8)
            h.junctions_enable(8, 1024)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            assert segs.shape[2] == 2
            cr, ce = h.candidates_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                         keys.tobytes(), segs.tobytes()))
        seen.append((rows, h.gene_counts().tobytes()))
    assert seen[0] == seen[1]
    o, h, sm = build(oracle, records, k=17)
    # the junction table alone (no depth state), then plain depth beside it: the depth model's answer, as before
    h.junctions_enable(8, 1024)
    h.depth_enable(1)
    goff, gids = h.classify(*_args(batches[1]))
    depth, mates = expected_depth(sm, batches[1], goff, gids, 1)
    assert np.array_equal(h.depth_all(), depth) and h.depth_mates() == mates
    want = Expected(sm)
    want.add(o, batches[1], goff, gids)
    want.check_table(h)
    # segments mode at m = 4 serves the new modes with its one launch
    h.depth_reset()
    h.junctions_reset()
    h.depth_enable_spliced(8)
    h.segments_enable(4)
    goff, gids = h.classify(*_args(batches[1]))
    keys, segs = h.segments_last()
    assert np.array_equal(segs, expected_segments(sm, batches[1], goff, gids, 4)[1])
    want.check_depth(h)
    want.check_table(h)


# ---------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------
def run_shark(args, cwd):
    return subprocess.run([os.path.join(ROOT, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def test_shark_depth_spliced_on_the_example(oracle, example_dir, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    nidx = o.build([s for _, s in fa])
    goff, gids = o.classify(*_args(batch))
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    legend = [name.decode() for name, _ in fa]
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq"), "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    for ms, extras in ((8, ([], ["--gpus", "2", "--devices", "0,0", "--batch", "700"])), (1, (["--segments", str(tmp_path / "sg"), "--segments-max", "2"],))):
        depth, mates = expected_spliced_depth(sm, batch, goff, gids, rows, ms)
        want = "".join(ln + "\n" for ln in depth_lines(depth, model_layout(sm, nidx), legend)).encode()
        assert mates > 3000 and want.count(b"\n") > 100
        for extra in extras:
            r = run_shark(base + ["--depth", str(tmp_path / "dp"), "--depth-spliced", "--depth-min-support", str(ms)] + extra, str(tmp_path))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            got = (tmp_path / "dp").read_bytes()
            assert got == want, next((i, a, w) for i, (a, w) in enumerate(zip(got.split(b"\n"), want.split(b"\n"))) if a != w)
