"""Evidence mode on the GPU (shk_evidence_enable / shk_evidence_last, `shark --evidence`): per read the best gene's coverage,
its k-mer count and the read's valid length, bit-exact against the CPU oracle (tests/evidence_model.py) -- and, through the
re-threshold property, against the kernels that never compute them.

Run on the GPU box with `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

from tests import synth
from tests.evidence_model import expected_evidence, handworked_batch, handworked_cases, handworked_evidence, passes
from tests.gpu_fixtures import probe  # noqa: F401  (the probe-structure variants)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVIDENCE_KERNELS = ("classify_fast_kernel<", "classify_general_kernel<")      # ... with "evidence" as the last template argument


def _is_evidence_kernel(name):
    return name.startswith(EVIDENCE_KERNELS) and name.endswith(", evidence>")


def _build_both(oracle, genes, **kw):
    from shark_amd import SharkHip
    o = oracle.Shark(k=kw.get("k", 17), c=kw.get("c", 0.6), bf_bits=kw.get("bf_bits", 1 << 33),
                     min_quality=kw.get("min_quality", 0), single=kw.get("single", False))
    nidx = o.build([bytes(g) for g in genes])
    h = SharkHip(**kw)
    info = h.build([bytes(g) for g in genes])
    assert info["nidx"] == nidx
    return o, h


def _args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"]


def _first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return "read %d: got %s, model %s (%d reads differ)" % (bad[0], got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad)) if len(bad) else ""


def _check_batch(o, h, batch, want=None):
    """one host batch through shk_classify with evidence on: genes equal the oracle's, evidence equals the model's, read for read"""
    og, oi = o.classify(*_args(batch))
    hg, hi = h.classify(*_args(batch))
    assert np.array_equal(og, hg) and np.array_equal(oi, hi)
    assert _is_evidence_kernel(h.last_kernel()) or len(batch["off1"]) == 1, h.last_kernel()
    ev = h.evidence_last()
    want = expected_evidence(o, batch) if want is None else want
    assert ev.shape == want.shape and ev.dtype == np.uint32
    assert np.array_equal(ev, want), _first_difference(ev, want)
    return ev, hg


def _to_device(b):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in b.items() if v is not None}
    torch.cuda.synchronize()
    return t


def _device_evidence(h, n):
    from shark_amd.capi import hip_memcpy_dtoh
    ptr = h.evidence_last()
    assert isinstance(ptr, int) and ptr != 0
    ev = np.empty((n, 3), np.uint32)
    if n:
        hip_memcpy_dtoh(ev, ptr, ev.nbytes)
    return ev


# ---------------------------------------------------------------------------
# hand-worked cases: against the file's own numbers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", handworked_cases(), ids=lambda c: c["name"])
def test_handworked_cases(case, probe):
    from shark_amd import SharkHip
    h = SharkHip(k=case["k"], c=case["c"], bf_bits=case["bf_bits"], min_quality=case["q"], single=case["single"])
    info = h.build([seq.encode() for _, seq in case["fasta"]])
    assert info["n_set_bits"] == case.get("set_bits", case["distinct_kmers"])
    h.evidence_enable(True)
    batch = handworked_batch(case)
    goff, gids = h.classify(*_args(batch))
    assert [list(map(int, gids[goff[i]:goff[i + 1]])) for i in range(len(case["reads"]))] == [r["genes"] for r in case["reads"]]
    ev = h.evidence_last()
    assert np.array_equal(ev, handworked_evidence(case)), (ev.tolist(), handworked_evidence(case).tolist())
    assert _is_evidence_kernel(h.last_kernel()), h.last_kernel()


# ---------------------------------------------------------------------------
# synthetic batches under every probe variant
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,bf_bits,q,shape", [
    (17, 1 << 26, 0, "paired-uniform"),
    (17, 1 << 26, 0, "paired-trimmed"),
    (17, 1 << 33, 0, "single-uniform"),
    (21, 1 << 24, 0, "single-trimmed"),
    (31, 1 << 26, 20, "paired-uniform"),
    (31, 1 << 26, 20, "paired-trimmed"),
    (17, 5 << 32, 0, "paired-uniform"),          # a filter size that is not a power of two
])
def test_synthetic_batches(oracle, probe, k, bf_bits, q, shape):
    rng = np.random.default_rng(1000 * k + q + len(shape))
    genes = synth.make_genes(rng, 24, 300, 2500, share_every=4)
    o, h = _build_both(oracle, genes, k=k, bf_bits=bf_bits, min_quality=q)
    h.evidence_enable(True)
    paired, var_len = shape.startswith("paired"), shape.endswith("trimmed")
    b = synth.make_reads(rng, genes, 1500, read_len=150, paired=paired, on_target=0.7, sub_rate=0.03, n_rate=0.004, lower_rate=0.01,
                         var_len=var_len, qual=q != 0)
    ev, _ = _check_batch(o, h, b)
    assert (ev[:, 1] > 0).sum() > 500 and (ev[:, 1] == 0).sum() > 100      # reads with a best gene, reads without a hit
    assert len(np.unique(ev[:, 2])) > 3                                     # N's (and masked bases) make the valid length vary


def test_short_reads_all_n_mates_and_the_empty_batch(oracle, probe):
    """(0, 0, len) for a read shorter than k, without a valid k-mer, or without a hit; len counts valid characters only"""
    rng = np.random.default_rng(77)
    genes = synth.make_genes(rng, 6, 400, 900)
    k = 19
    o, h = _build_both(oracle, genes, k=k, bf_bits=1 << 24)
    h.evidence_enable(True)
    g = genes[0]
    m1 = [b"", b"ACGT", b"N" * 100, b"A" * 18, bytes(g[:19]), bytes(g[:60]), bytes(g[100:160]), b"N" * 40, bytes(g[:18]) + b"N" + bytes(g[19:37]),
          bytes(synth.random_seq(rng, 90)), b"acgtn" * 10, bytes(g[200:290]).lower()]
    m2 = [b"", b"", b"N" * 3, b"", b"", b"N" * 60, bytes(synth.revcomp(g[100:200])), bytes(g[300:350]), b"", b"N", b"", bytes(g[10:12])]
    want_zero = [0, 1, 2, 3, 8, 9, 10]
    for paired in (True, False):
        b = synth.batch_from_lists(m1, m2 if paired else None)
        ev, _ = _check_batch(o, h, b)
        assert not ev[want_zero, :2].any()
        assert ev[2].tolist() == [0, 0, 0] and ev[3].tolist() == [0, 0, 18] and ev[4].tolist() == [19, 1, 19]
        assert ev[11, 1] > 0                                                   # lower case is valid (kmer_utils.hpp to_int)
    # n = 0: no records, and still the evidence of THAT batch
    empty = synth.batch_from_lists([], [])
    goff, gids = h.classify(*_args(empty))
    assert list(goff) == [0] and len(gids) == 0
    assert h.evidence_last().shape == (0, 3)


def test_ties_beyond_the_inline_ids(oracle, probe):
    """more than SHK_INLINE_IDS identical genes: the tie list is written by the (unchanged) tail, the evidence by the main pass"""
    from shark_amd.capi import SHK_INLINE_IDS
    rng = np.random.default_rng(11)
    core = synth.random_seq(rng, 600)
    genes = [core.copy() for _ in range(SHK_INLINE_IDS + 3)] + synth.make_genes(rng, 5, 300, 600)
    o, h = _build_both(oracle, genes, k=17, bf_bits=1 << 24)
    h.evidence_enable(True)
    b = synth.make_reads(rng, [core], 400, read_len=120, paired=True, on_target=1.0, sub_rate=0.01, n_rate=0.002)
    ev, goff = _check_batch(o, h, b)
    assert h.timing()["last_n_tie"] > 0
    assert (np.diff(goff.astype(np.int64)) == SHK_INLINE_IDS + 3).sum() > 200


def test_long_reads_through_the_general_kernel(oracle, probe):
    """reads beyond the fast kernel's slots: queued, then classified -- with their evidence -- by the general kernel"""
    rng = np.random.default_rng(13)
    genes = synth.make_genes(rng, 8, 3000, 9000, share_every=2)
    o, h = _build_both(oracle, genes, k=19, bf_bits=1 << 25)
    h.evidence_enable(True)
    m1, m2 = [], []
    for i in range(200):
        g = genes[i % len(genes)]
        L1, L2 = int(rng.integers(0, 2500)), int(rng.integers(0, 2500))
        st = int(rng.integers(0, len(g) - 2500))
        a = g[st:st + L1].copy()
        c = synth.revcomp(g[st:st + 2500])[:L2].copy()
        if i % 5 == 0 and L1:
            a[rng.integers(0, L1, size=max(1, L1 // 20))] = ord("N")
        m1.append(a.tobytes())
        m2.append(c.tobytes())
    b = synth.batch_from_lists(m1, m2)
    ev, _ = _check_batch(o, h, b)
    assert h.timing()["last_n_long"] > 0
    assert ev[:, 2].max() > 2000
    # the same reads resident in HBM with a length bound that does not hold: found after the fact, redone in wait
    t = _to_device(b)
    tk = h.submit_device(200, t["seq1"].data_ptr(), t["off1"].data_ptr(), t["seq2"].data_ptr(), t["off2"].data_ptr(), max_read_len=150)
    r = h.wait_device(tk)
    assert int(r.n_assoc) > 0 and h.timing()["last_n_long"] > 0
    assert np.array_equal(_device_evidence(h, 200), ev)
    r = h.classify_device(200, t["seq1"].data_ptr(), t["off1"].data_ptr(), t["seq2"].data_ptr(), t["off2"].data_ptr(), max_read_len=0)
    assert np.array_equal(_device_evidence(h, 200), ev)


def test_wrapped_index_of_more_than_65536_records(oracle):
    """more than 65 536 tiny records: ids wrap, lists carry multiplicities that change (cov, nk) -- the general kernel's WRAP
    instantiation, here with evidence"""
    rng = np.random.default_rng(65536)
    n_genes = 66500
    genes = [synth.random_seq(rng, int(rng.integers(40, 70))) for _ in range(n_genes)]
    rep = synth.random_seq(rng, 30)
    genes[65540] = np.concatenate([rep, synth.random_seq(rng, 5), rep, synth.random_seq(rng, 20)])   # k-mers twice inside a wrapped gene
    genes[65550] = np.concatenate([rep[:25], synth.random_seq(rng, 30)])
    genes[66000] = genes[464].copy()                                                                 # two genes behind one id
    genes[66499] = np.concatenate([genes[3][:35], genes[65539][:30]])
    o, h = _build_both(oracle, genes, k=17, bf_bits=1 << 30, c=0.3)
    h.evidence_enable(True)
    picks = [65540, 65550, 66000, 464, 66499, 3, 65539, 12, 65536, 65535, 1000, 66100]
    m1, m2 = [], []
    for g in picks * 25:
        s_ = genes[g]
        L = int(rng.integers(20, len(s_) + 1))
        st = int(rng.integers(0, len(s_) - L + 1))
        a_ = s_[st:st + L].copy()
        if rng.random() < 0.2:
            a_[int(rng.integers(0, L))] = ord("N")
        m1.append(a_.tobytes())
        m2.append(synth.revcomp(s_)[:int(rng.integers(17, len(s_) + 1))].tobytes())
    for _ in range(100):
        m1.append(synth.random_seq(rng, 60).tobytes())
        m2.append(synth.random_seq(rng, 60).tobytes())
    m1.append(np.concatenate([genes[65540], genes[66000], synth.random_seq(rng, 700), genes[66499]]).tobytes())   # and one for the long queue
    m2.append(synth.revcomp(np.concatenate([genes[65550], genes[464]])).tobytes())
    b = synth.batch_from_lists(m1, m2)
    ev, goff = _check_batch(o, h, b)
    assert h.last_kernel() == "classify_general_kernel<wrap, evidence>", h.last_kernel()
    assert h.timing()["last_n_long"] >= 1 and goff[-1] > 200
    _check_batch(o, h, synth.batch_from_lists(m1))                              # single-end


# ---------------------------------------------------------------------------
# the four entry-point families
# ---------------------------------------------------------------------------
def test_all_entry_point_families(oracle):
    from shark_amd import SharkHipError
    from shark_amd.capi import SHK_PIPE_DEPTH
    rng = np.random.default_rng(4242)
    genes = synth.make_genes(rng, 20, 400, 2500, share_every=3)
    o, h = _build_both(oracle, genes, k=17, bf_bits=1 << 30)
    with pytest.raises(SharkHipError, match="not allowed"):
        h.evidence_last()                                                       # no batch has been waited for
    h.evidence_enable(True)
    batches = [synth.make_reads(rng, genes, 900 + 150 * i, read_len=(150, 100, 125)[i % 3], paired=i != 4, on_target=0.6, sub_rate=0.03,
                                var_len=i in (1, 5)) for i in range(6)]
    batches.insert(3, synth.batch_from_lists([], []))
    want = [expected_evidence(o, b) for b in batches]
    genes_want = [o.classify(*_args(b)) if len(b["off1"]) > 1 else (np.zeros(1, np.uint32), np.zeros(0, np.uint16)) for b in batches]
    # shk_classify_submit / _wait: three batches in flight, each ticket's evidence read after its own wait
    tickets, seen = [], 0
    def drain():
        nonlocal seen
        gg, gi = h.wait(tickets.pop(0))
        ev = h.evidence_last()
        assert np.array_equal(gg, genes_want[seen][0]) and np.array_equal(gi, genes_want[seen][1])
        assert np.array_equal(ev, want[seen]), (seen, _first_difference(ev, want[seen]))
        seen += 1
    for b in batches:
        if len(tickets) == SHK_PIPE_DEPTH:
            with pytest.raises(SharkHipError, match="not allowed"):
                h.evidence_enable(False)                                        # tickets are outstanding
            drain()
        tickets.append(h.submit(b["seq1"], b["off1"], b["seq2"], b["off2"]))
    assert len(tickets) == SHK_PIPE_DEPTH
    while tickets:
        drain()
    assert seen == len(batches)
    # shk_classify_device and shk_classify_device_submit: the records live in device memory
    keep = [_to_device(b) for b in batches]
    def dev_args(i):
        t, b = keep[i], batches[i]
        paired = b["seq2"] is not None
        return (len(b["off1"]) - 1, t["seq1"].data_ptr(), t["off1"].data_ptr(), t["seq2"].data_ptr() if paired else 0, t["off2"].data_ptr() if paired else 0)
    for i in (0, 1, 4):
        r = h.classify_device(*dev_args(i), max_read_len=150 if i != 1 else 0)
        assert int(r.n_assoc) == len(genes_want[i][1])
        ev = _device_evidence(h, int(r.n))
        assert np.array_equal(ev, want[i]), (i, _first_difference(ev, want[i]))
    order = [0, 1, 2, 4, 5, 6]
    dtickets, dseen = [], 0
    def ddrain():
        nonlocal dseen
        i = order[dseen]
        r = h.wait_device(dtickets.pop(0))
        assert int(r.n_assoc) == len(genes_want[i][1])
        ev = _device_evidence(h, int(r.n))
        assert np.array_equal(ev, want[i]), (i, _first_difference(ev, want[i]))
        dseen += 1
    for i in order:
        if len(dtickets) == SHK_PIPE_DEPTH:
            ddrain()
        L = (150, 100, 125)[(i if i < 3 else i - 1) % 3]
        uniform = i in (0, 2, 4)                                                # (the caller may vouch for its lengths: evidence mode reads the offsets anyway)
        dtickets.append(h.submit_device(*dev_args(i), max_read_len=L, uniform_len1=L if uniform else 0,
                                        uniform_len2=L if uniform and batches[i]["seq2"] is not None else 0))
    while dtickets:
        ddrain()
    assert dseen == len(order)


# ---------------------------------------------------------------------------
# same genes on and off; which kernels ran
# ---------------------------------------------------------------------------
def test_same_genes_with_evidence_on_and_off(oracle, probe):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(99)
    genes = synth.make_genes(rng, 30, 300, 2000, share_every=5)
    h_on, h_off = SharkHip(k=17, c=0.6, bf_bits=1 << 28), SharkHip(k=17, c=0.6, bf_bits=1 << 28)
    for h in (h_on, h_off):
        h.build([bytes(g) for g in genes])
    h_on.evidence_enable(True)
    batches = [synth.make_reads(rng, genes, 2000, read_len=150, paired=True, on_target=0.6, sub_rate=0.04),
               synth.make_reads(rng, genes, 1200, read_len=120, paired=True, on_target=0.6, sub_rate=0.04, var_len=True),
               synth.make_reads(rng, genes, 800, read_len=100, paired=False, on_target=0.9, sub_rate=0.02)]
    off_kernels = []
    for b in batches:
        g_on = h_on.classify(*_args(b))
        assert h_on.last_kernel().startswith("classify_fast_kernel<") and h_on.last_kernel().endswith(", evidence>"), h_on.last_kernel()
        assert len(h_on.evidence_last()) == len(b["off1"]) - 1
        g_off = h_off.classify(*_args(b))
        off_kernels.append(h_off.last_kernel())
        assert "evidence" not in h_off.last_kernel()
        with pytest.raises(SharkHipError, match="not allowed"):
            h_off.evidence_last()
        assert np.array_equal(g_on[0], g_off[0]) and np.array_equal(g_on[1], g_off[1])
    assert np.array_equal(h_on.gene_counts(), h_off.gene_counts()) and h_on.gene_counts().sum() > 1000
    # off again: the kernels of a context that never had it on, and no evidence (not the last evidence batch's either)
    h_on.evidence_enable(False)
    for b, name in zip(batches, off_kernels):
        g_on = h_on.classify(*_args(b))
        g_off = h_off.classify(*_args(b))
        assert np.array_equal(g_on[0], g_off[0]) and np.array_equal(g_on[1], g_off[1])
        assert h_on.last_kernel() == h_off.last_kernel() and "evidence" not in h_on.last_kernel()
        with pytest.raises(SharkHipError, match="not allowed"):
            h_on.evidence_last()
    if probe == "auto":
        assert off_kernels[0].startswith("classify_uni_kernel<"), off_kernels[0]


# ---------------------------------------------------------------------------
# the re-threshold property: one evidence run at c = 0 answers for every c
# ---------------------------------------------------------------------------
RETHRESHOLD_CS = (0.3, 0.45, 0.6, 0.75, 0.9, 1.0)
RETHRESHOLD_SUB_RATES = (0.0, 0.02, 0.05, 0.08, 0.12)


def rethreshold_reads(rng, genes):
    """pairs of 2 x 150 bases cut from the genes with substitutions at RETHRESHOLD_SUB_RATES (a fifth of the reads at each): at
    k = 17 an isolated substitution uncovers one base, two within k of each other everything between them, so the rates spread
    cov / len from 1 (no substitution: the only way to pass c = 1.0) to below 0.3; the test asserts that spread with the oracle"""
    parts = [synth.make_reads(rng, genes, 600, read_len=150, paired=True, on_target=0.9, sub_rate=s, n_rate=0.0) for s in RETHRESHOLD_SUB_RATES]
    m = {}
    for key in ("seq1", "seq2"):
        m[key] = np.concatenate([p[key] for p in parts])
    n = sum(len(p["off1"]) - 1 for p in parts)
    off = np.arange(n + 1, dtype=np.uint64) * 150
    return {"seq1": m["seq1"], "off1": off, "seq2": m["seq2"], "off2": off.copy(), "qual1": None, "qual2": None}


RETHRESHOLD_PATHS = {
    # the index's automatic structure: twenty genes -> the exact table in LDS, bound cut, early decision, sparse first rounds
    "lds": {},
    # the position table through L2 (no LDS summary in front): the anchored extension and anchor_verdict_kernel in front of the table kernel
    "table+anchor": {"SHK_NO_LDS_SUMMARY": "1", "SHK_ANCHOR_ALWAYS": "1"},
    # ... and the minimiser-bucketed table, likewise
    "ktable+anchor": {"SHK_NO_LDS_SUMMARY": "1", "SHK_NO_SUMMARY": "1", "SHK_KTAB": "1", "SHK_ANCHOR_ALWAYS": "1"},
}


@pytest.mark.parametrize("path", list(RETHRESHOLD_PATHS))
def test_rethreshold_property(oracle, monkeypatch, path):
    """a read has associations in an ORDINARY run at confidence c -- classify_uni_kernel's bound cut and early decision, its
    anchored extension, anchor_verdict_kernel: the paths that never compute a coverage -- iff nk > 0 and
    (double)cov >= c * (double)len in one evidence run at c = 0.  `path` chooses which of those kernels the ordinary runs take;
    last_kernel() must say so."""
    from shark_amd import SharkHip
    for v in ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_ANCHOR_ALWAYS"):
        monkeypatch.delenv(v, raising=False)
    for name, v in RETHRESHOLD_PATHS[path].items():
        monkeypatch.setenv(name, v)
    rng = np.random.default_rng(2024)
    genes = synth.make_genes(rng, 20, 1000, 3000)
    b = rethreshold_reads(rng, genes)
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 28)
    o.build([bytes(g) for g in genes])
    model = expected_evidence(o, b)
    hit = model[model[:, 1] > 0]
    ratio = hit[:, 0].astype(np.float64) / hit[:, 2].astype(np.float64)
    for c in RETHRESHOLD_CS:                                                     # the reads fall on both sides of every c
        assert (ratio >= c).sum() >= 20 and (ratio < c).sum() >= 20, (c, int((ratio >= c).sum()), int((ratio < c).sum()))
    h0 = SharkHip(k=17, c=0.0, bf_bits=1 << 28)
    h0.build([bytes(g) for g in genes])
    h0.evidence_enable(True)
    goff0, _ = h0.classify(*_args(b))
    ev = h0.evidence_last()
    assert np.array_equal(ev, model), _first_difference(ev, model)
    assert np.array_equal(np.diff(goff0.astype(np.int64)) > 0, passes(ev, 0.0))
    h0.close()
    kernels = set()
    for c in RETHRESHOLD_CS:
        h = SharkHip(k=17, c=c, bf_bits=1 << 28)
        h.build([bytes(g) for g in genes])
        for _ in range(2):                                                       # (the second batch of a stream may take other kernels than the first)
            goff, _ = h.classify(*_args(b))
            print("c=%.2f %s: %s" % (c, path, h.last_kernel()))
            assert h.last_kernel().startswith("classify_uni_kernel<"), h.last_kernel()
            kernels.add((c, h.last_kernel()))
            has = np.diff(goff.astype(np.int64)) > 0
            want = passes(ev, c)
            assert np.array_equal(has, want), (c, h.last_kernel(), np.nonzero(has != want)[0][:5].tolist())
        h.close()
    if path == "lds":
        assert all("+anchored-extension" not in k and "+pre-verdict" not in k for _, k in kernels), kernels
    else:
        # every c ran with the anchored extension, and anchor_verdict_kernel ran in front of the table kernel for at least one
        assert all("+anchored-extension" in k for _, k in kernels), kernels
        assert any("+pre-verdict" in k for _, k in kernels), kernels


# ---------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------
def _run_shark(args, cwd):
    exe = os.path.join(ROOT, "shark_amd", "bin", "shark")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True)


def test_shark_evidence_on_the_example(oracle, example_dir, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    model = expected_evidence(o, synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2]))
    want = b"".join(b"%s %d %d %d\n" % (rid, e[0], e[1], e[2]) for (rid, _, _), e in zip(r1, model.tolist()))
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq")]
    plain = _run_shark(base + ["-o", str(tmp_path / "p1.fq"), "-p", str(tmp_path / "p2.fq"), "--gene-counts", str(tmp_path / "p.counts")], str(tmp_path))
    assert plain.returncode == 0, plain.stderr.decode()[-2000:]
    for tag, extra in (("a", []), ("b", ["--devices", "0,0", "--batch", "7"]), ("c", ["-t", "4", "--batch", "777"])):
        o1, o2, ev, gc = (tmp_path / ("%s.%s" % (tag, x)) for x in ("1.fq", "2.fq", "evidence", "counts"))
        r = _run_shark(base + ["-o", str(o1), "-p", str(o2), "--evidence", str(ev), "--gene-counts", str(gc)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == open(os.path.join(example_dir, "ENSG00000277117.truth.ssv"), "rb").read() == plain.stdout
        assert o1.read_bytes() == open(os.path.join(example_dir, "sharked.sample_1.truth.fq"), "rb").read()
        assert o2.read_bytes() == open(os.path.join(example_dir, "sharked.sample_2.truth.fq"), "rb").read()
        assert gc.read_bytes() == (tmp_path / "p.counts").read_bytes()
        got = ev.read_bytes()
        assert got.count(b"\n") == len(r1) == 5000
        assert got == want, next((i, a, w) for i, (a, w) in enumerate(zip(got.split(b"\n"), want.split(b"\n"))) if a != w)
