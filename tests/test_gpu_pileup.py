"""Pileup mode on the GPU (shk_pileup_enable and its read-outs, `shark --pileup`): the accumulated counts[x][A, C, G, T] and the mate
counter -- whole arrays, np.array_equal -- against the model (tests/pileup_model.py), which keeps an int8 array per mate with
ownership by first writer and shares no idea with the kernel.  The model is fed the GPU's own gene_off / gene_ids, which are compared
with the CPU oracle's first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import synth
from tests.depth_model import depth_lines, model_layout
from tests.pileup_model import expected_pileup, pileup_lines
from tests.segments_model import SegmentsModel, expected_segments, junction_lines, mate_lengths
from tests.spliced_model import expected_spliced_depth
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import Expected, build, device_assoc, spliced_gene, spliced_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Want:
    """what the pileup state must hold after the batches added so far"""

    def __init__(self, sm, s_min=8, q=0):
        self.sm, self.s_min, self.q = sm, s_min, q
        self.reset()

    def reset(self):
        n = int(model_layout(self.sm)[-1])
        self.counts = np.zeros((n, 4), dtype=np.uint32)
        self.lost = np.zeros(n, dtype=np.uint32)
        self.mates = 0
        self.overlapping = 0                          # mates whose kept spans overlap in record coordinates
        self.n_spans = np.zeros(5, dtype=np.int64)    # mates by their number of kept spans

    def add(self, o, batch, goff, gids, stats=False):
        og, oi = o.classify(*_args(batch))
        assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
        rows = expected_segments(self.sm, batch, goff, gids, 4, self.q)[1]
        c, lost, m = expected_pileup(self.sm, batch, goff, gids, rows, self.s_min, self.q)
        self.counts += c
        self.lost += lost
        self.mates += m
        if stats:
            lengths = mate_lengths(batch)
            read_of = np.repeat(np.arange(len(goff) - 1), np.diff(goff))
            for j in range(len(gids)):
                for t in range(2):
                    sp = capi.kept_spans(rows[j, t], int(lengths[read_of[j], t]), self.sm.k, self.s_min)
                    self.n_spans[len(sp)] += 1
                    self.overlapping += any(b[0] < a[1] for a, b in zip(sp, sp[1:]))
        return rows

    def check(self, h):
        gs = h.depth_layout()
        assert np.array_equal(gs, model_layout(self.sm, h.index_info()["nidx"]))
        got = h.pileup_all()
        assert got.dtype == np.uint32 and got.shape == self.counts.shape
        bad = np.nonzero((got != self.counts).any(axis=1))[0]
        assert len(bad) == 0, "base %d: got %s, model %s (%d differ)" % (bad[0], got[bad[0]], self.counts[bad[0]], len(bad))
        assert np.array_equal(got, self.counts)
        assert h.pileup_mates() == self.mates
        return got


def revcomp_batch(b):
    """every mate of the batch replaced by its reverse complement"""
    def mates(seq, off):
        return [synth.revcomp(seq[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    return synth.batch_from_lists(mates(b["seq1"], b["off1"]), mates(b["seq2"], b["off2"]) if b.get("seq2") is not None else None)


# ---------------------------------------------------------------------------
# 1. geometry
# ---------------------------------------------------------------------------
# The generator's seed per case: the first one (counting from 1) whose 150 pairs meet every non-vacuity condition below, found with the
# model alone.  Most seeds do at k = 5 and k = 17.  At k = 31 a substitution shows only where windows of 31 vote on both sides of it
# inside one span of a mate of 60 to 120 bytes, which leaves 3 to 19 minority positions per batch on most seeds: hence 189 and 154.
SEEDS = {(5, "one gene"): 1, (5, "two genes"): 1, (5, "twins"): 1, (17, "one gene"): 4, (17, "two genes"): 1, (17, "twins"): 1,
         (31, "one gene"): 189, (31, "two genes"): 154, (31, "twins"): 5}


@pytest.mark.parametrize("k", [5, 17, 31])
@pytest.mark.parametrize("ref", ["one gene", "two genes", "twins"])
def test_geometry_strands_indels_and_ties(oracle, k, ref):
    """mates over 0 to 5 junctions on both strands, with a deletion and with a repeat (overlapping record spans: each base once, from
    the earlier span), 3 % substitutions; one gene, two genes, and two identical genes (every read tied over both)"""
    rng = np.random.default_rng(SEEDS[(k, ref)])
    genes = [spliced_gene(rng, 4, k)] if ref == "one gene" else [spliced_gene(rng, 1 + i, k) for i in range(2)]
    if ref == "twins":
        genes = [genes[1], genes[1]]
    s_min = 3 if k == 5 else 8
    o, h, sm = build(oracle, [g for g, _ in genes], k=k)
    want = Want(sm, s_min)
    h.pileup_enable(s_min)
    batch = spliced_reads(rng, genes, 150, sub=0.03)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids, stats=True)
    got = want.check(h)
    # not vacuous
    minority = int((got.sum(axis=1) - got.max(axis=1) > 0).sum())
    print("mates", want.mates, "by spans", want.n_spans.tolist(), "overlapping", want.overlapping, "minority positions", minority)
    assert want.mates > 100 and want.n_spans[2:].sum() >= 1
    if k <= 17:
        assert want.overlapping >= 1
    assert minority >= 20
    if ref == "twins":
        n = len(genes[0][0])
        assert np.array_equal(got[:n], got[n:]) and int(goff[-1]) > 150
    for g in range(len(genes)):
        a, b = int(h.depth_layout()[g]), int(h.depth_layout()[g + 1])
        assert np.array_equal(h.pileup(g), got[a:b])
    h.pileup_reset()
    want.reset()
    want.check(h)


# ---------------------------------------------------------------------------
# 2. lane passes
# ---------------------------------------------------------------------------
def test_lane_passes_and_record_ends(oracle):
    """unspliced mates of 17 .. 600 bytes (one window; around one and two passes of 64 coordinates; past segments_kernel's 512 cached
    slots), on both strands, flush with the record's start, flush with its end, and inside"""
    rng = np.random.default_rng(64)
    rec = synth.random_seq(rng, 700)
    o, h, sm = build(oracle, [rec], k=17)
    want = Want(sm, 1)
    h.pileup_enable(1)                                # (a mate of 17 bytes has one window)
    reads = []
    for L in (17, 63, 64, 65, 128, 129, 600):
        for a in (0, 700 - L, 41):
            reads += [rec[a:a + L].copy(), synth.revcomp(rec[a:a + L])]
    batch = synth.batch_from_lists(reads)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    got = want.check(h)
    # every mate is read whole and shows the record: per base as many observations as mates lie over it, all of the record's base
    depth = np.zeros(700, dtype=np.uint32)
    for L in (17, 63, 64, 65, 128, 129, 600):
        for a in (0, 700 - L, 41):
            depth[a:a + L] += 2
    assert want.mates == len(reads) == 42
    assert np.array_equal(got.sum(axis=1), depth) and np.array_equal(got[np.arange(700), np.searchsorted(synth.ACGT, rec)], depth)


# ---------------------------------------------------------------------------
# 3. batch sizes; 6. the four families; 7. the repair paths
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(2026)
    return [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes_ragged_and_uniform(oracle, panel, n):
    rng = np.random.default_rng(9 * n)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    want = Want(sm)
    h.pileup_enable(8)
    for ragged, paired in ((False, True), (True, True), (True, False)):
        batch = spliced_reads(rng, panel, n, paired=paired, ragged=ragged, sub=0.03)
        want.add(o, batch, *h.classify(*_args(batch)))
        want.check(h)
    assert n < 63 or want.mates > 0


def test_a_batch_and_its_reverse_complement_count_the_same(oracle, panel):
    rng = np.random.default_rng(12)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    want = Want(sm)
    h.pileup_enable(8)
    batch = spliced_reads(rng, panel, 200, sub=0.03)
    want.add(o, batch, *h.classify(*_args(batch)))
    fwd = want.check(h)
    fwd_mates = h.pileup_mates()
    h.pileup_reset()
    want.reset()
    rc = revcomp_batch(batch)
    want.add(o, rc, *h.classify(*_args(rc)))
    assert np.array_equal(want.check(h), fwd) and h.pileup_mates() == fwd_mates and fwd.any()


def test_all_four_families_accumulate_and_reset(oracle, panel):
    rng = np.random.default_rng(57)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    batches = [spliced_reads(rng, panel, n, ragged=r, sub=0.03) for n, r in ((200, False), (65, True), (150, True))]
    dev = [_to_device(b) for b in batches]

    def host(i):
        return h.classify(*_args(batches[i]))

    def resident(i):
        return device_assoc(h.classify_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i])))

    def resident_submit(i):
        return device_assoc(h.wait_device(h.submit_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i]))))

    want = Want(sm, 6)
    h.pileup_enable(6)
    first = True
    for family in (host, "pipeline", resident, resident_submit):
        if family == "pipeline":
            results = [h.wait(t) for t in [h.submit(*_args(b)) for b in batches]]
        else:
            results = [family(i) for i in range(3)]
        for b, (goff, gids) in zip(batches, results):
            if first:
                want.add(o, b, goff, gids)
            else:                                               # (the model's answer for a batch is computed once)
                og, oi = o.classify(*_args(b))
                assert np.array_equal(og, goff) and np.array_equal(oi, gids)
        first = False
        got = want.check(h)
        assert got.any()
        t = torch.zeros(got.shape, dtype=torch.int32, device="cuda:0")
        assert h.pileup_all(device_ptr=t.data_ptr()) == got.size
        assert np.array_equal(t.cpu().numpy().view(np.uint32), got)
        h.pileup_reset()
        assert not h.pileup_all().any() and h.pileup_mates() == 0


def test_length_bound_repair_counts_once(oracle):
    """mates of 3 000 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again): counted there, and only there"""
    rng = np.random.default_rng(29)
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, sm = build(oracle, long_genes, k=17)
    want = Want(sm)
    h.pileup_enable(8)
    mates = [np.concatenate([long_genes[i % 3][20 * i:20 * i + (1500 if i % 5 == 0 else 50)], long_genes[i % 3][2000 + 20 * i:2000 + 20 * i + (1500 if i % 5 == 0 else 50)]])
             for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    goff, gids = device_assoc(h.wait_device(h.submit_device(40, max_read_len=100, **_dev_ptrs(t))))
    assert h.timing()["last_n_long"] > 0
    want.add(o, b, goff, gids)
    got = want.check(h)
    assert want.mates == 80 and int(got[0].sum()) == 2
    b2 = synth.batch_from_lists([long_genes[0][100:160], long_genes[1][50:150]])
    want.add(o, b2, *h.classify(*_args(b2)))
    want.check(h)


def test_association_overflow_repair_counts_once(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 reads tied over 6 identical genes"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    o, h, sm = build(oracle, [twin.copy() for _ in range(6)], k=17)
    want = Want(sm)
    h.pileup_enable(8)
    reads = [np.concatenate([twin[(7 * i) % 200:(7 * i) % 200 + 50], twin[300 + (7 * i) % 200:350 + (7 * i) % 200]]) for i in range(3000)]
    batch = synth.batch_from_lists(reads)
    goff, gids = h.classify(*_args(batch))
    assert int(goff[-1]) == 18000
    want.add(o, batch, goff, gids)
    got = want.check(h)
    assert want.mates == 18000 and all(np.array_equal(got[:600], got[600 * g:600 * g + 600]) for g in range(1, 6))
    # (each half of a read lies whole on its diagonal; a diagonal that runs on over a base the other half happens to share reads it twice)
    assert int(got.sum()) >= 18000 * 100


# ---------------------------------------------------------------------------
# 5. consistency with spliced depth on the device
# ---------------------------------------------------------------------------
def test_channels_sum_to_spliced_depth_without_non_bases(oracle, panel):
    rng = np.random.default_rng(13)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17)
    want = Want(sm)
    h.pileup_enable(8)
    h.depth_enable_spliced(8)
    for paired, ragged in ((True, False), (True, True)):
        batch = spliced_reads(rng, panel, 200, paired=paired, ragged=ragged, sub=0.03)
        want.add(o, batch, *h.classify(*_args(batch)))
    got = want.check(h)
    assert not want.lost.any() and want.mates > 100
    assert np.array_equal(got.sum(axis=1, dtype=np.uint32), h.depth_all()) and h.pileup_mates() == h.depth_mates()


def test_non_bases_and_the_quality_mask_make_no_observation(oracle, panel):
    rng = np.random.default_rng(11)
    o, h, sm = build(oracle, [g for g, _ in panel], k=17, min_quality=20)
    want = Want(sm, 8, q=20)
    h.pileup_enable(8)
    h.depth_enable_spliced(8)
    for paired, ragged in ((True, False), (False, True)):
        batch = spliced_reads(rng, panel, 200, paired=paired, ragged=ragged, qual=True, lower=0.2)
        want.add(o, batch, *h.classify(*_args(batch)))
    got = want.check(h)
    depth = h.depth_all()
    total = got.sum(axis=1, dtype=np.uint32)
    assert want.mates > 100 and h.pileup_mates() == h.depth_mates()
    assert (total <= depth).all() and (total < depth).any() and np.array_equal(total + want.lost, depth)


# ---------------------------------------------------------------------------
# 8. the numbering quirk
# ---------------------------------------------------------------------------
def test_record_numbering_quirk(oracle):
    """an all-N record (does not advance the counter), records shorter than k (advance it, carry nothing): their ids have length 0"""
    rng = np.random.default_rng(19)
    g = [spliced_gene(rng, 2, 17) for _ in range(4)]
    records = [np.full(60, ord("N"), np.uint8), g[0][0], synth.random_seq(rng, 9), g[1][0], np.full(40, ord("N"), np.uint8), g[2][0], g[3][0], synth.random_seq(rng, 5)]
    o, h, sm = build(oracle, records, k=17)
    assert sorted(sm.records) == [0, 2, 3, 4] and h.index_info()["nidx"] == 6
    want = Want(sm)
    h.pileup_enable(8)
    batch = spliced_reads(rng, g, 200)
    goff, gids = h.classify(*_args(batch))
    want.add(o, batch, goff, gids)
    got = want.check(h)
    gs = h.depth_layout()
    assert want.mates > 100 and h.pileup(1).shape == (0, 4) and h.pileup(5).shape == (0, 4)
    assert all(h.pileup(x).any() and np.array_equal(h.pileup(x), got[int(gs[x]):int(gs[x + 1])]) for x in (0, 2, 3, 4))


# ---------------------------------------------------------------------------
# 9. state rules; 10. inertness
# ---------------------------------------------------------------------------
def test_state_rules(oracle, panel):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    records = [g for g, _ in panel]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError):
        h.pileup_enable(8)                        # before finalize
    h.pileup_enable(0)                            # (switching off is always allowed)
    h.build([bytes(g) for g in records])
    with pytest.raises(SharkHipError):
        h.pileup_enable(8)                        # finalized without keep_positions
    o, h, sm = build(oracle, records, k=17)
    for call in (h.pileup_all, h.pileup_mates, h.pileup_reset, lambda: h.pileup(0)):
        with pytest.raises(SharkHipError, match="never enabled"):
            call()
    want = Want(sm)
    b = spliced_reads(rng, panel, 50)
    h.pileup_enable(8)
    goff, gids = h.classify(*_args(b))
    want.add(o, b, goff, gids)
    want.check(h)
    # off keeps the state and adds nothing; on again goes on from it
    h.pileup_enable(0)
    h.classify(*_args(b))
    want.check(h)
    h.pileup_enable(8)
    # tickets outstanding
    tk = h.submit(*_args(b))
    for call in (lambda: h.pileup_enable(8), lambda: h.pileup_enable(0), h.pileup_all, lambda: h.pileup(0), h.pileup_mates, h.pileup_reset):
        with pytest.raises(SharkHipError):
            call()
    h.wait(tk)
    want.add(o, b, goff, gids)
    want.check(h)
    # shk_count_work's batch and a wrongly vouched batch count nothing
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    ub = spliced_reads(rng, panel, 64, ragged=False)
    t = _to_device(ub)
    tk = h.submit_device(64, max_read_len=120, uniform_len1=99, uniform_len2=99, **_dev_ptrs(t))
    with pytest.raises(SharkHipError):
        h.wait_device(tk)
    want.check(h)
    # a wider index than ids can name
    wide = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    wide.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_positions=True)
    with pytest.raises(SharkHipError, match="65 536"):
        wide.pileup_enable(8)


def test_pileup_is_inert_and_segments_at_four_serves_it(oracle, panel):
    """every older mode on; pileup switched on beside them changes none of their results, byte for byte"""
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
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        if new:
            h.pileup_enable(8)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            assert segs.shape[2] == 2
            cr, ce = h.candidates_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                         keys.tobytes(), segs.tobytes()))
        seen.append((rows, h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.depth_summary().tobytes(), h.junctions_get().tobytes()))
        if new:
            assert h.pileup_all().any()
    assert seen[0] == seen[1] and len(seen[0][5]) > 0
    # segments mode at m = 4 serves pileup with its one launch; the spliced modes' answers beside it are the models'
    o, h, sm = build(oracle, records, k=17)
    want, older = Want(sm), Expected(sm)
    h.pileup_enable(8)
    h.depth_enable_spliced(8)
    h.junctions_enable(8, 1024)
    h.segments_enable(4)
    goff, gids = h.classify(*_args(batches[1]))
    keys, segs = h.segments_last()
    assert np.array_equal(segs, want.add(o, batches[1], goff, gids))
    want.check(h)
    older.add(o, batches[1], goff, gids)
    older.check_depth(h)
    older.check_table(h)
    # pileup alone: segments_kernel runs for it into the context's own arrays
    o, h, sm = build(oracle, records, k=17)
    want = Want(sm)
    h.pileup_enable(8)
    want.add(o, batches[0], *h.classify(*_args(batches[0])))
    want.check(h)


# ---------------------------------------------------------------------------
# 11. the command
# ---------------------------------------------------------------------------
def run_shark(args, cwd):
    return subprocess.run([os.path.join(ROOT, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def test_shark_pileup_on_the_example(oracle, example_dir, tmp_path):
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
    gs = model_layout(sm, nidx)
    counts, _, mates = expected_pileup(sm, batch, goff, gids, rows, 8)
    want = "".join(ln + "\n" for ln in pileup_lines(counts, gs, legend)).encode()
    assert mates > 3000 and want.count(b"\n") > 1000
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq"), "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    for extra in ([], ["--gpus", "2", "--devices", "0,0", "--batch", "700"]):
        r = run_shark(base + ["--pileup", str(tmp_path / "pu")] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = (tmp_path / "pu").read_bytes()
        assert got == want, next((i, a, w) for i, (a, w) in enumerate(zip(got.split(b"\n"), want.split(b"\n"))) if a != w)
    # together with the other consumers of segments mode, and another floor
    counts3, _, _ = expected_pileup(sm, batch, goff, gids, rows, 3)
    want3 = "".join(ln + "\n" for ln in pileup_lines(counts3, gs, legend)).encode()
    depth, _ = expected_spliced_depth(sm, batch, goff, gids, rows, 8)
    want_depth = "".join(ln + "\n" for ln in depth_lines(depth, gs, legend)).encode()
    want_junc = "".join(ln + "\n" for ln in junction_lines(goff, gids, rows, mate_lengths(batch), 17, legend, 8)).encode()
    r = run_shark(base + ["--pileup", str(tmp_path / "pu3"), "--pileup-min-support", "3", "--depth", str(tmp_path / "dp"), "--depth-spliced", "--depth-min-support", "8",
                          "--junctions", str(tmp_path / "jn"), "--junctions-device"], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert (tmp_path / "pu3").read_bytes() == want3 and (tmp_path / "dp").read_bytes() == want_depth and (tmp_path / "jn").read_bytes() == want_junc
