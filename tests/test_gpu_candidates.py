"""Candidates mode on the GPU (shk_candidates_enable / shk_candidates_last, `shark --candidates`): per read its best m genes in
the reference's ranking with their coverage and k-mer count, the read's valid length and the number of genes it hit --
entry for entry equal to the model (tests/candidates_model.py), which is pinned to the CPU oracle on every read it computes.
No tolerances anywhere.

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
from tests.candidates_model import (candidate_lines, expected_candidates, handworked_batch, handworked_cases, thresholded, tie_group)
from tests.gpu_fixtures import probe  # noqa: F401  (the probe-structure variants)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 2, 8)


def _is_candidates_kernel(name):
    return name.startswith(("classify_fast_kernel<", "classify_general_kernel<")) and name.endswith(", candidates>")


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
    got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    return "read %d: got %s, model %s (%d reads differ)" % (bad[0], got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad)) if len(bad) else ""


def _assert_equal(got, want):
    (gr, ge), (wr, we) = got, want
    assert gr.shape == wr.shape and ge.shape == we.shape and gr.dtype == ge.dtype == np.uint32, (gr.shape, wr.shape, ge.shape, we.shape)
    assert np.array_equal(gr, wr), "headers: " + _first_difference(gr, wr)
    assert np.array_equal(ge, we), "entries: " + _first_difference(ge, we)


def _check_batch(o, h, batch, m, want8=None):
    """one host batch through shk_classify with candidates on at m: genes equal the oracle's, candidates equal the model's"""
    h.candidates_enable(m)
    og, oi = o.classify(*_args(batch))
    hg, hi = h.classify(*_args(batch))
    assert np.array_equal(og, hg) and np.array_equal(oi, hi)
    assert _is_candidates_kernel(h.last_kernel()) or len(batch["off1"]) == 1, h.last_kernel()
    want8 = expected_candidates(o, batch, 8) if want8 is None else want8
    got = h.candidates_last()
    _assert_equal(got, (want8[0], want8[1][:, :m]))
    return want8, hg


def _check_all_m(o, h, batch):
    want8 = None
    for m in MS:
        want8, goff = _check_batch(o, h, batch, m, want8)
    return want8, goff


def _to_device(b):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in b.items() if v is not None}
    torch.cuda.synchronize()
    return t


def _device_candidates(h, n_want, m_want):
    from shark_amd.capi import hip_memcpy_dtoh
    n, m, p_reads, p_entries = h.candidates_last()
    assert (n, m) == (n_want, m_want)
    reads, entries = np.empty((n, 2), np.uint32), np.empty((n, m, 3), np.uint32)
    if n:
        assert isinstance(p_reads, int) and p_reads != 0 and isinstance(p_entries, int) and p_entries != 0
        hip_memcpy_dtoh(reads, p_reads, reads.nbytes)
        hip_memcpy_dtoh(entries, p_entries, entries.nbytes)
    return reads, entries


def _shared_genes(rng, n_genes, lo, hi):
    """genes with shared stretches: every third copies half of its predecessor, every other carries one common block, two are twins"""
    genes = synth.make_genes(rng, n_genes, lo, hi, share_every=3)
    common = synth.random_seq(rng, 80)
    for g in genes[::2]:
        g[30:110] = common
    genes[5] = genes[4].copy()
    return genes


# ---------------------------------------------------------------------------
# hand-worked cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", handworked_cases(), ids=lambda c: c["name"])
def test_handworked_cases(oracle, case, probe):
    from shark_amd import SharkHip
    o = oracle.Shark(k=case["k"], c=case["c"], bf_bits=case["bf_bits"], min_quality=case["q"], single=case["single"])
    o.build([seq.encode() for _, seq in case["fasta"]])
    h = SharkHip(k=case["k"], c=case["c"], bf_bits=case["bf_bits"], min_quality=case["q"], single=case["single"])
    h.build([seq.encode() for _, seq in case["fasta"]])
    batch = handworked_batch(case)
    want8 = expected_candidates(o, batch, 8)
    for m in MS:
        h.candidates_enable(m)
        goff, gids = h.classify(*_args(batch))
        assert [list(map(int, gids[goff[i]:goff[i + 1]])) for i in range(len(case["reads"]))] == [r["genes"] for r in case["reads"]]
        reads, entries = h.candidates_last()
        _assert_equal((reads, entries), (want8[0], want8[1][:, :m]))
        assert _is_candidates_kernel(h.last_kernel()), h.last_kernel()
        for i, r in enumerate(case["reads"]):
            assert int(reads[i, 0]) == r["len"] and entries[i, 0, 1:].tolist() == list(r["best"])
    if case["name"].startswith("two_identical_genes_"):
        assert entries[0, :3].tolist() == [[0, 16, 8], [1, 16, 8], [0, 0, 0]] and reads[0].tolist() == [16, 2]


# ---------------------------------------------------------------------------
# synthetic batches under every probe variant
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,bf_bits,q,shape", [
    (5, 4099, 0, "paired-uniform"),              # a filter of a few thousand bits: collisions make candidates
    (5, 1 << 12, 0, "single-trimmed"),
    (17, 1 << 20, 0, "paired-uniform"),
    (17, 1 << 26, 0, "paired-trimmed"),
    (17, 1 << 33, 20, "single-uniform"),
    (31, 1 << 14, 0, "paired-trimmed"),
    (31, 1 << 26, 20, "paired-uniform"),
])
def test_synthetic_batches(oracle, probe, k, bf_bits, q, shape):
    rng = np.random.default_rng(2000 * k + q + len(shape))
    genes = _shared_genes(rng, 24, 300, 1500)
    o, h = _build_both(oracle, genes, k=k, bf_bits=bf_bits, min_quality=q, c=0.0)
    paired, var_len = shape.startswith("paired"), shape.endswith("trimmed")
    b = synth.make_reads(rng, genes, 700, read_len=100 if k == 5 else 150, paired=paired, on_target=0.8, sub_rate=0.03, n_rate=0.004,
                         lower_rate=0.01, var_len=var_len, qual=q != 0)
    (reads, entries), _ = _check_all_m(o, h, b)
    assert (reads[:, 1] >= 2).sum() > 150                                       # several candidates
    assert sum(1 for row in entries if len(tie_group(row)) >= 2) >= 5           # ties at the head
    assert len(np.unique(reads[:, 0])) > 3                                      # N's (and masked bases) make the valid length vary


def test_short_reads_all_n_mates_and_the_empty_batch(oracle, probe):
    """n_genes = 0, the read's len and empty entries for a read shorter than k, without a valid k-mer, or without a hit"""
    rng = np.random.default_rng(77)
    genes = synth.make_genes(rng, 6, 400, 900)
    k = 19
    o, h = _build_both(oracle, genes, k=k, bf_bits=1 << 24)
    g = genes[0]
    m1 = [b"", b"ACGT", b"N" * 100, b"A" * 18, bytes(g[:19]), bytes(g[:60]), bytes(g[100:160]), b"N" * 40, bytes(g[:18]) + b"N" + bytes(g[19:37]),
          bytes(synth.random_seq(rng, 90)), b"acgtn" * 10, bytes(g[200:290]).lower()]
    m2 = [b"", b"", b"N" * 3, b"", b"", b"N" * 60, bytes(synth.revcomp(g[100:200])), bytes(g[300:350]), b"", b"N", b"", bytes(g[10:12])]
    want_zero = [0, 1, 2, 3, 8, 9, 10]
    for paired in (True, False):
        b = synth.batch_from_lists(m1, m2 if paired else None)
        (reads, entries), _ = _check_all_m(o, h, b)
        assert not reads[want_zero, 1].any() and not entries[want_zero].any()
        assert reads[2].tolist() == [0, 0] and reads[3].tolist() == [18, 0] and reads[4].tolist() == [19, 1]
        assert entries[4, 0].tolist() == [0, 19, 1] and not entries[4, 1:].any()
        assert reads[11, 1] > 0                                                # lower case is valid (kmer_utils.hpp to_int)
    # n = 0: no records, and still the candidates of THAT batch
    empty = synth.batch_from_lists([], [])
    h.candidates_enable(3)
    goff, gids = h.classify(*_args(empty))
    assert list(goff) == [0] and len(gids) == 0
    reads, entries = h.candidates_last()
    assert reads.shape == (0, 2) and entries.shape == (0, 3, 3)


def test_more_candidates_than_entries_and_long_tie_groups(oracle, probe):
    """a read with more than SHK_MAX_CANDIDATES candidates: n_genes says so and the entries are the best eight; a tie group
    longer than m; a tie group longer than SHK_INLINE_IDS, whose ordinary result still comes from the tie queue"""
    from shark_amd.capi import SHK_INLINE_IDS, SHK_MAX_CANDIDATES
    rng = np.random.default_rng(11)
    core = synth.random_seq(rng, 600)
    twins = [core.copy() for _ in range(SHK_INLINE_IDS + 2)]                    # six identical genes: ties of six
    partial = [np.concatenate([core[:100 + 25 * i], synth.random_seq(rng, 200)]) for i in range(8)]   # eight more that share a prefix of growing length
    genes = twins + partial + synth.make_genes(rng, 4, 300, 600)
    o, h = _build_both(oracle, genes, k=17, bf_bits=1 << 24, c=0.3)
    b = synth.make_reads(rng, [core[60:]], 600, read_len=120, paired=True, on_target=1.0, sub_rate=0.01, n_rate=0.002)
    (reads, entries), goff = _check_all_m(o, h, b)
    assert h.timing()["last_n_tie"] > 0
    assert (np.diff(goff.astype(np.int64)) == SHK_INLINE_IDS + 2).sum() > 100
    assert (reads[:, 1] > SHK_MAX_CANDIDATES).sum() > 100                        # more genes hit than entries handed out
    groups = [len(tie_group(row)) for row in entries]
    assert sum(1 for g in groups if g == SHK_INLINE_IDS + 2) > 100               # the whole group is in the eight entries ...
    full = entries[np.array(groups) == SHK_INLINE_IDS + 2]
    assert (full[:, :SHK_INLINE_IDS + 2, 0] == np.arange(SHK_INLINE_IDS + 2)).all()   # ... in ascending id order, the twins first
    assert (full[:, SHK_INLINE_IDS + 2, 2] > 0).sum() > 50                       # ... and behind it the runners-up


def test_long_reads_through_the_general_kernel(oracle, probe):
    """reads beyond the fast kernel's slots: queued, then classified -- with their candidates -- by the general kernel"""
    rng = np.random.default_rng(13)
    genes = synth.make_genes(rng, 8, 3000, 9000, share_every=2)
    o, h = _build_both(oracle, genes, k=19, bf_bits=1 << 25)
    m1, m2 = [], []
    for i in range(120):
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
    want8, _ = _check_batch(o, h, b, 8)
    assert h.timing()["last_n_long"] > 0
    assert want8[0][:, 0].max() > 2000 and (want8[0][:, 1] >= 2).sum() > 5
    # the same reads resident in HBM with a length bound that does not hold: found after the fact, redone in wait
    t = _to_device(b)
    h.candidates_enable(2)
    tk = h.submit_device(120, t["seq1"].data_ptr(), t["off1"].data_ptr(), t["seq2"].data_ptr(), t["off2"].data_ptr(), max_read_len=150)
    r = h.wait_device(tk)
    assert int(r.n_assoc) > 0 and h.timing()["last_n_long"] > 0
    _assert_equal(_device_candidates(h, 120, 2), (want8[0], want8[1][:, :2]))
    r = h.classify_device(120, t["seq1"].data_ptr(), t["off1"].data_ptr(), t["seq2"].data_ptr(), t["off2"].data_ptr(), max_read_len=0)
    _assert_equal(_device_candidates(h, 120, 2), (want8[0], want8[1][:, :2]))


def test_wrapped_index_of_more_than_65536_records(oracle):
    """more than 65 536 tiny records: ids wrap, lists carry multiplicities that change (cov, nk) -- the general kernel's WRAP
    instantiation, here with candidates: the entries are the reference's map entries (the construction of the evidence test)"""
    rng = np.random.default_rng(65536)
    n_genes = 66500
    genes = [synth.random_seq(rng, int(rng.integers(40, 70))) for _ in range(n_genes)]
    rep = synth.random_seq(rng, 30)
    genes[65540] = np.concatenate([rep, synth.random_seq(rng, 5), rep, synth.random_seq(rng, 20)])   # k-mers twice inside a wrapped gene
    genes[65550] = np.concatenate([rep[:25], synth.random_seq(rng, 30)])
    genes[66000] = genes[464].copy()                                                                 # two genes behind one id
    genes[66499] = np.concatenate([genes[3][:35], genes[65539][:30]])
    o, h = _build_both(oracle, genes, k=17, bf_bits=1 << 30, c=0.3)
    picks = [65540, 65550, 66000, 464, 66499, 3, 65539, 12, 65536, 65535, 1000, 66100]
    m1, m2 = [], []
    for g in picks * 12:
        s_ = genes[g]
        L = int(rng.integers(20, len(s_) + 1))
        st = int(rng.integers(0, len(s_) - L + 1))
        a_ = s_[st:st + L].copy()
        if rng.random() < 0.2:
            a_[int(rng.integers(0, L))] = ord("N")
        m1.append(a_.tobytes())
        m2.append(synth.revcomp(s_)[:int(rng.integers(17, len(s_) + 1))].tobytes())
    for _ in range(50):
        m1.append(synth.random_seq(rng, 60).tobytes())
        m2.append(synth.random_seq(rng, 60).tobytes())
    m1.append(np.concatenate([genes[65540], genes[66000], synth.random_seq(rng, 700), genes[66499]]).tobytes())   # and one for the long queue
    m2.append(synth.revcomp(np.concatenate([genes[65550], genes[464]])).tobytes())
    b = synth.batch_from_lists(m1, m2)
    (reads, entries), goff = _check_all_m(o, h, b)
    assert h.last_kernel() == "classify_general_kernel<wrap, candidates>", h.last_kernel()
    assert h.timing()["last_n_long"] >= 1 and goff[-1] > 100
    assert (reads[:, 1] >= 2).sum() > 5
    _check_batch(o, h, synth.batch_from_lists(m1), 8)                            # single-end


# ---------------------------------------------------------------------------
# the four entry-point families, the state rules
# ---------------------------------------------------------------------------
def test_all_entry_point_families_and_state_rules(oracle):
    from shark_amd import SharkHipError
    from shark_amd.capi import SHK_PIPE_DEPTH
    rng = np.random.default_rng(4242)
    genes = _shared_genes(rng, 20, 400, 2000)
    o, h = _build_both(oracle, genes, k=17, bf_bits=1 << 30)
    with pytest.raises(SharkHipError, match="not allowed"):
        h.candidates_last()                                                     # no batch has been waited for
    with pytest.raises(SharkHipError, match="invalid argument"):
        h.candidates_enable(9)                                                  # m > SHK_MAX_CANDIDATES: SHK_ERR_ARG
    h.classify(*_args(synth.make_reads(rng, genes, 50)))
    with pytest.raises(SharkHipError, match="not allowed"):
        h.candidates_last()                                                     # behind a batch submitted with the mode off
    m = 3
    h.candidates_enable(m)
    batches = [synth.make_reads(rng, genes, 500 + 100 * i, read_len=(150, 100, 125)[i % 3], paired=i != 4, on_target=0.6, sub_rate=0.03,
                                var_len=i in (1, 5)) for i in range(6)]
    batches.insert(3, synth.batch_from_lists([], []))
    want = []
    for b in batches:
        r8, e8 = expected_candidates(o, b, 8)
        want.append((r8, e8[:, :m]))
    genes_want = [o.classify(*_args(b)) if len(b["off1"]) > 1 else (np.zeros(1, np.uint32), np.zeros(0, np.uint16)) for b in batches]
    # shk_classify_submit / _wait: three batches in flight, each ticket's candidates read after its own wait
    tickets, seen = [], 0
    def drain():
        nonlocal seen
        gg, gi = h.wait(tickets.pop(0))
        got = h.candidates_last()
        assert np.array_equal(gg, genes_want[seen][0]) and np.array_equal(gi, genes_want[seen][1])
        _assert_equal(got, want[seen])
        seen += 1
    for b in batches:
        if len(tickets) == SHK_PIPE_DEPTH:
            with pytest.raises(SharkHipError, match="not allowed"):
                h.candidates_enable(0)                                          # tickets are outstanding
            with pytest.raises(SharkHipError, match="not allowed"):
                h.candidates_enable(5)
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
        _assert_equal(_device_candidates(h, int(r.n), m), want[i])
    h.count_work(*dev_args(0))
    with pytest.raises(SharkHipError, match="not allowed"):
        h.candidates_last()                                                     # shk_count_work hands out none
    order = [0, 1, 2, 4, 5, 6]
    dtickets, dseen = [], 0
    def ddrain():
        nonlocal dseen
        i = order[dseen]
        r = h.wait_device(dtickets.pop(0))
        assert int(r.n_assoc) == len(genes_want[i][1])
        _assert_equal(_device_candidates(h, int(r.n), m), want[i])
        dseen += 1
    for i in order:
        if len(dtickets) == SHK_PIPE_DEPTH:
            ddrain()
        L = (150, 100, 125)[(i if i < 3 else i - 1) % 3]
        uniform = i in (0, 2, 4)
        dtickets.append(h.submit_device(*dev_args(i), max_read_len=L, uniform_len1=L if uniform else 0,
                                        uniform_len2=L if uniform and batches[i]["seq2"] is not None else 0))
    while dtickets:
        ddrain()
    assert dseen == len(order)
    # off again: no candidates, not the last candidates batch's either
    h.candidates_enable(0)
    h.classify(*_args(batches[0]))
    assert "candidates" not in h.last_kernel()
    with pytest.raises(SharkHipError, match="not allowed"):
        h.candidates_last()


# ---------------------------------------------------------------------------
# consistency with what exists: the ordinary kernels, evidence mode
# ---------------------------------------------------------------------------
CONSISTENCY_PATHS = {
    "lds": ({}, 20),                                                                       # the exact table in LDS
    "table+anchor": ({"SHK_NO_LDS_SUMMARY": "1", "SHK_ANCHOR_ALWAYS": "1"}, 20),          # the position table behind anchor_verdict_kernel
}


@pytest.mark.parametrize("path", list(CONSISTENCY_PATHS))
@pytest.mark.parametrize("single", [False, True], ids=["all", "single"])
def test_consistency_with_the_ordinary_kernels_and_evidence(oracle, monkeypatch, path, single):
    """batches large enough that the mode-off run takes classify_uni_kernel (and, on the table path, anchor_verdict_kernel in
    front): genes and gene counts identical on and off; the leading tie group thresholded at c and --single on the host equals
    the ordinary kernels' associations; with evidence on as well, evidence[i] == (entries[i][0].cov, entries[i][0].nk, reads[i].len)"""
    from shark_amd import SharkHip
    for v in ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_ANCHOR_ALWAYS"):
        monkeypatch.delenv(v, raising=False)
    env, n_genes = CONSISTENCY_PATHS[path]
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    rng = np.random.default_rng(99 + n_genes)
    genes = _shared_genes(rng, n_genes, 1000, 3000)
    c = 0.6
    h_on, h_off = (SharkHip(k=17, c=c, bf_bits=1 << 28, single=single) for _ in range(2))
    for h in (h_on, h_off):
        h.build([bytes(g) for g in genes])
    h_on.candidates_enable(8)
    h_on.evidence_enable(True)
    n = 20000
    parts = [synth.make_reads(rng, genes, n // 4, read_len=150, paired=True, on_target=0.8, sub_rate=s, n_rate=0.0) for s in (0.0, 0.02, 0.06, 0.1)]
    off = np.arange(n + 1, dtype=np.uint64) * 150
    b = {"seq1": np.concatenate([p["seq1"] for p in parts]), "off1": off, "seq2": np.concatenate([p["seq2"] for p in parts]), "off2": off.copy(),
         "qual1": None, "qual2": None}
    off_kernels = set()
    for rep in range(3):                                                          # (the second batch of a stream may take other kernels than the first)
        g_off = h_off.classify(*_args(b))
        off_kernels.add(h_off.last_kernel())
        assert h_off.last_kernel().startswith("classify_uni_kernel<"), h_off.last_kernel()
        g_on = h_on.classify(*_args(b))
        assert h_on.last_kernel().startswith("classify_fast_kernel<") and h_on.last_kernel().endswith(", candidates>"), h_on.last_kernel()
        assert np.array_equal(g_on[0], g_off[0]) and np.array_equal(g_on[1], g_off[1])
        reads, entries = h_on.candidates_last()
        ev = h_on.evidence_last()
        assert np.array_equal(ev, np.stack([entries[:, 0, 1], entries[:, 0, 2], reads[:, 0]], axis=1))
        want = synth.assoc_lists(g_off[0], g_off[1])
        got = thresholded(reads, entries, c, single)
        groups = np.array([len(tie_group(row)) for row in entries])
        assert (groups < 8).all()                                                # (every tie group is complete in the eight entries)
        assert [list(map(int, w)) for w in want] == got
        assert sum(1 for w in want if len(w)) > n // 4 and sum(1 for w in want if not len(w)) > n // 8
    assert np.array_equal(h_on.gene_counts(), h_off.gene_counts()) and h_on.gene_counts().sum() > 1000
    if path != "lds":
        assert all("+anchored-extension" in k for k in off_kernels) and any("+pre-verdict" in k for k in off_kernels), off_kernels
    # a sample of the records against the model
    o = oracle.Shark(k=17, c=c, bf_bits=1 << 28, single=single)
    o.build([bytes(g) for g in genes])
    pick = np.arange(0, n, 40)
    sub = {"seq1": np.concatenate([b["seq1"][i * 150:(i + 1) * 150] for i in pick]), "off1": np.arange(len(pick) + 1, dtype=np.uint64) * 150,
           "seq2": np.concatenate([b["seq2"][i * 150:(i + 1) * 150] for i in pick]), "off2": np.arange(len(pick) + 1, dtype=np.uint64) * 150,
           "qual1": None, "qual2": None}
    _assert_equal((reads[pick], entries[pick]), expected_candidates(o, sub, 8))


# ---------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------
def _run_shark(args, cwd):
    exe = os.path.join(ROOT, "shark_amd", "bin", "shark")
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True)


def test_shark_candidates_on_the_example(oracle, example_dir, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    reads, entries = expected_candidates(o, synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2]), 8)
    legend = [name.decode() if isinstance(name, bytes) else name for name, _ in fa]
    ids = [rid.decode() if isinstance(rid, bytes) else rid for rid, _, _ in r1]
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq")]
    truth = open(os.path.join(example_dir, "ENSG00000277117.truth.ssv"), "rb").read()
    for tag, m, extra in (("a", 4, []), ("b", 1, ["--candidates-n", "1", "--gpus", "2", "--devices", "0,0", "--batch", "7"]),
                          ("c", 8, ["--candidates-n", "8", "-t", "4", "--batch", "777", "--evidence", "EVID"])):
        o1, o2, cd = (tmp_path / ("%s.%s" % (tag, x)) for x in ("1.fq", "2.fq", "candidates"))
        extra = [str(tmp_path / "c.evidence") if x == "EVID" else x for x in extra]
        r = _run_shark(base + ["-o", str(o1), "-p", str(o2), "--candidates", str(cd)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == truth
        assert o1.read_bytes() == open(os.path.join(example_dir, "sharked.sample_1.truth.fq"), "rb").read()
        assert o2.read_bytes() == open(os.path.join(example_dir, "sharked.sample_2.truth.fq"), "rb").read()
        got = cd.read_text().split("\n")
        want = candidate_lines(ids, reads, entries[:, :m], legend)
        assert got[-1] == "" and len(got) - 1 == len(r1) == 5000
        assert got[:-1] == want, next((i, a, w) for i, (a, w) in enumerate(zip(got, want)) if a != w)
    # with --evidence beside it: the two files agree line by line
    ev = (tmp_path / "c.evidence").read_text().split("\n")[:-1]
    for e_line, c_line in zip(ev, (tmp_path / "c.candidates").read_text().split("\n")[:-1]):
        rid, cov, nk, ln = e_line.split(" ")
        f = c_line.split(" ")
        assert f[0] == rid and f[1] == ln and ((cov, nk) == ("0", "0") if f[2] == "0" else (f[4], f[5]) == (cov, nk))
