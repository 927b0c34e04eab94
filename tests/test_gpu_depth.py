"""Depth mode on the GPU (shk_depth_enable and the read-outs, `shark --depth`): the accumulated per-base depth, its summary and the
mate counter -- whole arrays, np.array_equal -- against the model (tests/depth_model.py), which increments base by base from the
placement model and shares no idea with the kernels.  The model is fed the GPU's own gene_off / gene_ids, which are compared with
the CPU oracle's first.  No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from tests import synth
from tests.candidates_model import expected_candidates
from tests.depth_model import depth_lines, depth_summary, expected_depth, model_layout
from tests.evidence_model import expected_evidence
from tests.placement_model import PlacementModel, expected_placements
from tests.test_gpu_placement import _args, _dev_ptrs, _reads, _to_device

pytestmark = pytest.mark.gpu


def _build(oracle, genes, keep=True, **kw):
    from shark_amd import SharkHip
    kw.setdefault("c", 0.0)
    kw.setdefault("bf_bits", 1 << 26)
    k = kw.get("k", 17)
    o = oracle.Shark(k=k, c=kw["c"], bf_bits=kw["bf_bits"], min_quality=kw.get("min_quality", 0), single=kw.get("single", False))
    nidx = o.build([bytes(g) for g in genes])
    h = SharkHip(**kw)
    info = h.build([bytes(g) for g in genes], keep_positions=keep)
    assert info["nidx"] == nidx
    return o, h, PlacementModel([bytes(g) for g in genes], k)


def _want(o, model, batch, goff, gids, ms, q=0):
    """the model's (depth, mates) of one batch from the GPU's associations, once those agree with the oracle's"""
    og, oi = o.classify(*_args(batch))
    assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
    return expected_depth(model, batch, goff, gids, ms, q)


def _device_assoc(r):
    from shark_amd.capi import hip_memcpy_dtoh
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    return goff, gids


def _check_state(h, model, depth, mates):
    """every read-out against the expected accumulated state"""
    gs = h.depth_layout()
    assert np.array_equal(gs, model_layout(model, h.index_info()["nidx"]))
    got = h.depth_all()
    assert got.dtype == np.uint32 and got.shape == depth.shape
    bad = np.nonzero(got != depth)[0]
    assert len(bad) == 0, "base %d: got %d, model %d (%d differ)" % (bad[0], got[bad[0]], depth[bad[0]], len(bad))
    assert h.depth_mates() == mates
    s = h.depth_summary()
    assert [tuple(int(v) for v in (r["len"], r["covered"], r["max"], r["sum"])) for r in s] == depth_summary(depth, gs)
    assert not s["pad"].any()
    return got, gs


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
def _geometry_reads(rng, genes, k):
    """per gene: mates of 100 bases at both ends, flush and overhanging by 30, on both strands; one inside; one of k - 1 bases"""
    m1s, m2s = [], []
    for g in genes:
        n = len(g)
        over_start = np.concatenate([synth.random_seq(rng, 30), g[:70]])
        over_end = np.concatenate([g[n - 70:], synth.random_seq(rng, 30)])
        mates = [g[:100], g[n - 100:], over_start, over_end, g[100:200], g[50:50 + k - 1]]
        for m in mates:
            m1s.append(m.copy())
            m2s.append(synth.revcomp(m))
        for m in mates:                      # and the other way round: mate 1 reversed, mate 2 a different place
            m1s.append(synth.revcomp(m))
            m2s.append(g[150:250].copy())
    return synth.batch_from_lists(m1s, m2s)


@pytest.mark.parametrize("k", [5, 17, 31])
@pytest.mark.parametrize("n_genes", [1, 2])
def test_geometry_overhang_strands_and_min_support(oracle, k, n_genes):
    rng = np.random.default_rng(1000 + 10 * k + n_genes)
    genes = [synth.random_seq(rng, 300) for _ in range(n_genes)]
    o, h, model = _build(oracle, genes, k=k)
    batch = _geometry_reads(rng, genes, k)
    for ms in (1, 5, 1000):
        h.depth_enable(ms)
        goff, gids = h.classify(*_args(batch))
        depth, mates = _want(o, model, batch, goff, gids, ms)
        got, gs = _check_state(h, model, depth, mates)
        if ms == 1000:
            assert mates == 0 and not got.any()
        else:
            assert mates > 10 * n_genes and got[:5].all() and got[295:300].all()   # (not vacuous: both ends are covered)
        h.depth_reset()
        _check_state(h, model, np.zeros_like(depth), 0)


def test_a_mate_ending_at_the_record_end_leaves_the_next_gene_alone(oracle):
    rng = np.random.default_rng(3)
    genes = [synth.random_seq(rng, 300) for _ in range(2)]
    o, h, model = _build(oracle, genes, k=17)
    h.depth_enable(1)
    batch = synth.batch_from_lists([genes[0][200:300].copy() for _ in range(3)], [synth.revcomp(genes[0][180:300]) for _ in range(3)])
    goff, gids = h.classify(*_args(batch))
    depth, mates = _want(o, model, batch, goff, gids, 1)
    got, gs = _check_state(h, model, depth, mates)
    assert mates == 6 and got[299] == 6 and not got[300:].any() and got[:180].sum() == 0
    assert h.depth(0).tolist() == got[:300].tolist() and h.depth(1).tolist() == [0] * 300


# ---------------------------------------------------------------------------
# batch sizes, the four families, the repair paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes_ragged_and_uniform(oracle, n):
    rng = np.random.default_rng(7 * n)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17)
    h.depth_enable(1)
    total, total_mates = None, 0
    for ragged in (False, True):
        for paired in (True, False):
            batch = _reads(rng, genes, n, 100, 150, paired=paired, ragged=ragged)
            goff, gids = h.classify(*_args(batch))
            depth, mates = _want(o, model, batch, goff, gids, 1)
            total = depth if total is None else total + depth
            total_mates += mates
            _check_state(h, model, total, total_mates)


def test_all_four_families_accumulate_and_reset(oracle):
    rng = np.random.default_rng(53)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17)
    batches = [_reads(rng, genes, n, 100, 150, paired=True, ragged=r) for n, r in ((200, False), (65, True), (150, True), (100, False))]
    dev = [_to_device(b) for b in batches]
    wants = {}

    def want(i, goff, gids):
        if i not in wants:                                      # (the model's answer for a batch is computed once)
            wants[i] = _want(o, model, batches[i], goff, gids, 2)
        else:
            og, oi = o.classify(*_args(batches[i]))
            assert np.array_equal(og, goff) and np.array_equal(oi, gids)
        return wants[i]

    def host(i):
        return h.classify(*_args(batches[i]))

    def resident(i):
        return _device_assoc(h.classify_device(len(batches[i]["off1"]) - 1, max_read_len=150, **_dev_ptrs(dev[i])))

    def resident_submit(i):
        tk = h.submit_device(len(batches[i]["off1"]) - 1, max_read_len=150, **_dev_ptrs(dev[i]))
        return _device_assoc(h.wait_device(tk))

    h.depth_enable(2)
    for family in (host, "pipeline", resident, resident_submit):
        if family == "pipeline":
            tickets = [h.submit(*_args(batches[i])) for i in range(3)]
            results = [h.wait(t) for t in tickets]
        else:
            results = [family(i) for i in range(3)]
        acc = [want(i, *results[i]) for i in range(3)]
        depth, gs = _check_state(h, model, acc[0][0] + acc[1][0] + acc[2][0], acc[0][1] + acc[1][1] + acc[2][1])
        assert depth.any()
        t = torch.zeros(len(depth), dtype=torch.int32, device="cuda:0")
        assert h.depth_all(device_ptr=t.data_ptr()) == len(depth)
        assert np.array_equal(t.cpu().numpy().view(np.uint32), depth)
        h.depth_reset()
        d3, m3 = want(3, *(host(3) if family in (host, "pipeline") else family(3)))
        _check_state(h, model, d3, m3)
        h.depth_reset()


def test_length_bound_repair_counts_once(oracle):
    """reads of 3 000 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again): counted there, and only there"""
    rng = np.random.default_rng(29)
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, model = _build(oracle, long_genes, k=17)
    h.depth_enable(1)
    mates = [long_genes[i % 3][50 * i:50 * i + (3000 if i % 5 == 0 else 100)] for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    tk = h.submit_device(40, max_read_len=100, **_dev_ptrs(t))
    goff, gids = _device_assoc(h.wait_device(tk))
    assert h.timing()["last_n_long"] > 0
    depth, n_mates = _want(o, model, b, goff, gids, 1)
    got, _ = _check_state(h, model, depth, n_mates)
    assert n_mates == 80 and got[0] == 2
    b2 = _reads(rng, long_genes, 100, 100, 150, paired=True)
    goff, gids = h.classify(*_args(b2))
    d2, m2 = _want(o, model, b2, goff, gids, 1)
    _check_state(h, model, depth + d2, n_mates + m2)


def test_association_overflow_repair_counts_once(oracle):
    """more associations than a slot reserves: 3 000 reads tied over 6 identical genes of 600 bases; all six have the same depth"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    genes = [twin.copy() for _ in range(6)]
    o, h, model = _build(oracle, genes, k=17)
    h.depth_enable(1)
    batch = synth.batch_from_lists([twin[(7 * i) % 500:(7 * i) % 500 + 100] for i in range(3000)])
    goff, gids = h.classify(*_args(batch))
    assert int(goff[-1]) == 18000
    depth, mates = _want(o, model, batch, goff, gids, 1)
    got, gs = _check_state(h, model, depth, mates)
    assert mates == 18000 and all(np.array_equal(got[:600], got[600 * g:600 * g + 600]) for g in range(1, 6))
    b2 = synth.batch_from_lists([twin[i:i + 120] for i in range(0, 400, 9)])
    goff, gids = h.classify(*_args(b2))
    d2, m2 = _want(o, model, b2, goff, gids, 1)
    got, _ = _check_state(h, model, depth + d2, mates + m2)
    assert all(np.array_equal(got[:600], got[600 * g:600 * g + 600]) for g in range(1, 6))


# ---------------------------------------------------------------------------
# masks, the numbering quirk
# ---------------------------------------------------------------------------
def test_quality_mask_and_lower_case(oracle):
    rng = np.random.default_rng(11)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17, min_quality=20)
    h.depth_enable(3)
    total, total_mates = None, 0
    for paired, ragged in ((True, False), (True, True), (False, True)):
        batch = _reads(rng, genes, 200, 100, 150, paired=paired, ragged=ragged, qual=True, lower=0.2)
        goff, gids = h.classify(*_args(batch))
        depth, mates = _want(o, model, batch, goff, gids, 3, q=20)
        total = depth if total is None else total + depth
        total_mates += mates
    _check_state(h, model, total, total_mates)
    assert total_mates > 100


def test_record_numbering_quirk(oracle):
    """an all-N record (does not advance the counter), records shorter than k (advance it, carry nothing): their ids have length 0"""
    rng = np.random.default_rng(19)
    g = synth.make_genes(rng, 4, 500, 700)
    genes = [np.full(60, ord("N"), np.uint8), g[0], synth.random_seq(rng, 9), g[1], np.full(40, ord("N"), np.uint8), g[2], g[3], synth.random_seq(rng, 5)]
    o, h, model = _build(oracle, genes, k=17)
    assert sorted(model.records) == [0, 2, 3, 4] and h.index_info()["nidx"] == 6
    gs = h.depth_layout()
    assert np.array_equal(gs, model_layout(model, 6)) and gs[2] == gs[1] and gs[6] == gs[5] == sum(len(x) for x in g)
    h.depth_enable(1)
    batch = _reads(rng, g, 200, 100, paired=True)
    goff, gids = h.classify(*_args(batch))
    depth, mates = _want(o, model, batch, goff, gids, 1)
    _check_state(h, model, depth, mates)
    assert len(h.depth(1)) == 0 and len(h.depth(5)) == 0 and mates > 100


# ---------------------------------------------------------------------------
# state rules, inertness, all four modes
# ---------------------------------------------------------------------------
def test_state_rules(oracle):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    genes = synth.make_genes(rng, 5, 400, 600)
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError):
        h.depth_enable(1)                         # before finalize
    h.depth_enable(0)                             # (switching off is always allowed)
    h.build([bytes(g) for g in genes])
    with pytest.raises(SharkHipError):
        h.depth_enable(1)                         # finalized without keep_positions
    with pytest.raises(SharkHipError):
        h.depth_layout()
    o, h, model = _build(oracle, genes, k=17)
    assert np.array_equal(h.depth_layout(), model_layout(model, 5))      # the layout belongs to the index
    for read_out in (h.depth_all, h.depth_summary, h.depth_mates, h.depth_reset, lambda: h.depth(0)):
        with pytest.raises(SharkHipError):
            read_out()                            # never enabled on this context
    b = _reads(rng, genes, 50, 100, paired=True)
    h.depth_enable(1)
    goff, gids = h.classify(*_args(b))
    depth, mates = _want(o, model, b, goff, gids, 1)
    tk = h.submit(*_args(b))
    for call in (lambda: h.depth_enable(1), lambda: h.depth_enable(0), h.depth_all, h.depth_summary, h.depth_mates, h.depth_reset, lambda: h.depth(0)):
        with pytest.raises(SharkHipError):
            call()                                # tickets outstanding
    h.wait(tk)
    _check_state(h, model, 2 * depth, 2 * mates)
    # off keeps the state and stops the counting; on again goes on from it; shk_count_work's batch is not counted
    h.depth_enable(0)
    h.classify(*_args(b))
    _check_state(h, model, 2 * depth, 2 * mates)
    h.depth_enable(1)
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    _check_state(h, model, 2 * depth, 2 * mates)
    h.classify(*_args(b))
    _check_state(h, model, 3 * depth, 3 * mates)
    with pytest.raises(SharkHipError):
        h.depth(5)                                # no such gene
    # a batch whose caller vouched wrongly for its read lengths (a base too short: every access stays inside the buffers) is refused
    # in wait and not counted
    ub = _reads(rng, genes, 64, 100, 150, paired=True)
    t = _to_device(ub)
    tk = h.submit_device(64, max_read_len=150, uniform_len1=99, uniform_len2=149, **_dev_ptrs(t))
    with pytest.raises(SharkHipError):
        h.wait_device(tk)
    _check_state(h, model, 3 * depth, 3 * mates)


def test_more_than_65536_records_are_refused(oracle):
    from shark_amd import SharkHip, SharkHipError
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    h.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_positions=True)
    with pytest.raises(SharkHipError):
        h.depth_enable(1)
    with pytest.raises(SharkHipError):
        h.depth_layout()


def test_mode_off_is_inert_and_all_four_modes_agree(oracle):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(41)
    genes = synth.make_genes(rng, 100, 600, 1400)
    batches = [_reads(rng, genes, 300, 100, paired=True), _reads(rng, genes, 300, 100, 150, paired=True, ragged=True)]
    seen = []
    for depth in ("never", "off again", "on"):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in genes], keep_positions=True)
        h.placement_enable(True)
        if depth != "never":
            h.depth_enable(1)
        if depth == "off again":
            h.depth_enable(0)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.placement_last().tobytes()))
        seen.append((rows, h.gene_counts().tobytes()))
        if depth == "off again":
            assert h.depth_mates() == 0 and not h.depth_all().any()
    assert seen[0] == seen[1] == seen[2]
    # depth on, placement off: the kernel runs, nothing is handed out
    o, h, model = _build(oracle, genes, k=17)
    h.depth_enable(1)
    goff, gids = h.classify(*_args(batches[1]))
    with pytest.raises(SharkHipError):
        h.placement_last()
    depth, mates = _want(o, model, batches[1], goff, gids, 1)
    _check_state(h, model, depth, mates)
    # all four modes
    h.placement_enable(True)
    h.evidence_enable(True)
    h.candidates_enable(4)
    goff, gids = h.classify(*_args(batches[1]))
    assert np.array_equal(h.placement_last(), expected_placements(model, batches[1], goff, gids))
    assert np.array_equal(h.evidence_last(), expected_evidence(o, batches[1]))
    wr, we = expected_candidates(o, batches[1], 4)
    gr, ge = h.candidates_last()
    assert np.array_equal(gr, wr) and np.array_equal(ge, we)
    _check_state(h, model, 2 * depth, 2 * mates)


# ---------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------
def _run_shark(args, cwd):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([os.path.join(root, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def _expected_file(oracle, fasta, batch, k, c, legend, ms=1):
    o = oracle.Shark(k=k, c=c, bf_bits=1 << 33)
    nidx = o.build(fasta)
    goff, gids = o.classify(*_args(batch))
    model = PlacementModel(fasta, k)
    depth, mates = expected_depth(model, batch, goff, gids, ms)
    lines = depth_lines(depth, model_layout(model, nidx), legend)
    return "".join(ln + "\n" for ln in lines).encode(), mates


def test_shark_depth_on_the_example(oracle, example_dir, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    want, mates = _expected_file(oracle, [s for _, s in fa], batch, 17, 0.6, [name.decode() for name, _ in fa])
    assert mates > 3000 and want.count(b"\n") > 100
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq")]
    plain = _run_shark(base + ["-o", str(tmp_path / "p.1"), "-p", str(tmp_path / "p.2"), "--placements", str(tmp_path / "p.pl")], str(tmp_path))
    assert plain.returncode == 0, plain.stderr.decode()[-2000:]
    for tag, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "7"]),
                       ("c", ["--batch", "777", "--placements", str(tmp_path / "c.pl"), "--evidence", str(tmp_path / "c.ev"), "--candidates", str(tmp_path / "c.cd")])):
        o1, o2, dp = (tmp_path / ("%s.%s" % (tag, x)) for x in ("1.fq", "2.fq", "depth"))
        r = _run_shark(base + ["-o", str(o1), "-p", str(o2), "--depth", str(dp)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == plain.stdout
        assert o1.read_bytes() == (tmp_path / "p.1").read_bytes() and o2.read_bytes() == (tmp_path / "p.2").read_bytes()
        got = dp.read_bytes()
        assert got == want, next((i, a, w) for i, (a, w) in enumerate(zip(got.split(b"\n"), want.split(b"\n"))) if a != w)
    assert (tmp_path / "c.pl").read_bytes() == (tmp_path / "p.pl").read_bytes()


def test_shark_depth_synthetic_pairs_min_support_and_refusals(oracle, tmp_path):
    rng = np.random.default_rng(47)
    genes = synth.make_genes(rng, 50, 500, 900)
    n = 2000
    b = _reads(rng, genes, n, 100, 120, paired=True, ragged=True, lower=0.0)
    (tmp_path / "g.fa").write_text("".join(">g%d\n%s\n" % (i, bytes(g).decode()) for i, g in enumerate(genes)))
    for name, seq, off in (("1.fq", b["seq1"], b["off1"]), ("2.fq", b["seq2"], b["off2"])):
        with open(tmp_path / name, "w") as f:
            for i in range(n):
                s = bytes(seq[int(off[i]):int(off[i + 1])]).decode()
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    legend = ["g%d" % i for i in range(50)]
    base = ["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq"), "-2", str(tmp_path / "2.fq"), "-c", "0.3", "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    for ms, extras in ((1, ([], ["--gpus", "2", "--devices", "0,0", "--batch", "300"])), (20, (["--depth-min-support", "20"],))):
        want, mates = _expected_file(oracle, [bytes(g) for g in genes], b, 17, 0.3, legend, ms)
        for extra in extras:
            r = _run_shark(base + ["--depth", str(tmp_path / "dp")] + extra, str(tmp_path))
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            assert (tmp_path / "dp").read_bytes() == want and mates > 1000
    # a reference of more than 65 536 records: a message and exit code 1
    with open(tmp_path / "wide.fa", "w") as f:
        for i in range(65537):
            f.write(">w%d\nACGTACGTTGCATGCAAGCT\n" % i)
    r = _run_shark(["-r", str(tmp_path / "wide.fa"), "-1", str(tmp_path / "1.fq"), "-o", str(tmp_path / "o1"), "--depth", str(tmp_path / "dpw")], str(tmp_path))
    assert r.returncode == 1 and b"--depth is not available for a reference of more than 65536 records" in r.stderr
    # a path that cannot be opened
    r = _run_shark(base + ["--depth", str(tmp_path / "no" / "such" / "dp")], str(tmp_path))
    assert r.returncode == 1 and b"cannot open the depth file" in r.stderr
    # a file that cannot be written
    if os.path.exists("/dev/full"):
        r = _run_shark(base + ["--depth", "/dev/full"], str(tmp_path))
        assert r.returncode == 1 and b"cannot write the depth file" in r.stderr
