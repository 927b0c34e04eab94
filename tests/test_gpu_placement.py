"""Placement mode on the GPU (shk_ref_keep_positions / shk_placement_enable / shk_placement_last): per association and mate the
best diagonal (strand, pos, support) -- association for association equal to the model (tests/placement_model.py), which is
written from the semantics and never asks the filter.  No tolerances anywhere.  After every batch the genes and offsets are
compared with the CPU oracle's as well.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from tests import repeat_refs, synth
from tests.candidates_model import expected_candidates
from tests.evidence_model import expected_evidence
from tests.placement_model import PlacementModel, expected_placements

pytestmark = pytest.mark.gpu


def _args(b):
    return b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"]


def _build(oracle, genes, keep=True, **kw):
    from shark_amd import SharkHip
    kw.setdefault("c", 0.0)
    o = oracle.Shark(k=kw.get("k", 17), c=kw["c"], bf_bits=kw.get("bf_bits", 1 << 26), min_quality=kw.get("min_quality", 0),
                     single=kw.get("single", False))
    kw.setdefault("bf_bits", 1 << 26)
    nidx = o.build([bytes(g) for g in genes])
    h = SharkHip(**kw)
    info = h.build([bytes(g) for g in genes], keep_positions=keep)
    assert info["nidx"] == nidx
    return o, h, PlacementModel([bytes(g) for g in genes], kw.get("k", 17))


def _to_device(b):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in b.items() if v is not None}
    torch.cuda.synchronize()
    return t


def _dev_ptrs(t):
    g = lambda k: t[k].data_ptr() if k in t else 0  # noqa: E731
    return dict(seq1=g("seq1"), off1=g("off1"), seq2=g("seq2"), off2=g("off2"), qual1=g("qual1"), qual2=g("qual2"))


def _device_result(h, r):
    from shark_amd.capi import hip_memcpy_dtoh, placements_from_device
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    na, ptr = h.placement_last()
    assert na == tot
    return goff, gids, placements_from_device(na, ptr)


def _first_difference(got, want):
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    return "association %d: got %s, model %s (%d differ)" % (bad[0], got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad)) if len(bad) else ""


def _compare(o, model, batch, goff, gids, got, q=0):
    og, oi = o.classify(*_args(batch))
    assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
    want = expected_placements(model, batch, goff, gids, q)
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got, want), _first_difference(got, want)
    return want


def _check_host(o, h, model, batch, q=0):
    h.placement_enable(True)
    goff, gids = h.classify(*_args(batch))
    return _compare(o, model, batch, goff, gids, h.placement_last(), q), goff, gids


# ---------------------------------------------------------------------------
# reads with placement content
# ---------------------------------------------------------------------------
def _mate(rng, g, L, kind):
    """one mate of L bases drawn from gene g: either strand; overhanging an end, with an indel, or chimeric (two places) by kind"""
    glen = len(g)
    if kind == "overhang-start":
        cut = int(rng.integers(1, max(2, L // 2)))
        m = np.concatenate([synth.random_seq(rng, cut), g[:max(0, L - cut)]])
    elif kind == "overhang-end":
        cut = int(rng.integers(1, max(2, L // 2)))
        m = np.concatenate([g[max(0, glen - (L - cut)):], synth.random_seq(rng, cut)])
    elif kind in ("chimera-equal", "chimera-unequal"):
        h1 = L // 2 if kind == "chimera-equal" else (2 * L) // 3
        a = int(rng.integers(0, max(1, glen - h1)))
        b = int(rng.integers(0, max(1, glen - (L - h1))))
        m = np.concatenate([g[a:a + h1], g[b:b + L - h1]])
    else:
        a = int(rng.integers(0, max(1, glen - L - 2)))
        m = g[a:a + L + 2].copy()
        if kind == "indel" and len(m) > 8:
            at = int(rng.integers(3, len(m) - 3))
            m = np.delete(m, at) if rng.random() < 0.5 else np.insert(m, at, synth.ACGT[rng.integers(0, 4)])
    m = m[:L]
    if len(m) < L:
        m = np.concatenate([m, synth.random_seq(rng, L - len(m))])
    m = m.copy()
    if rng.random() < 0.5:
        m = synth.revcomp(m)
    return m


KINDS = ("plain", "plain", "plain", "overhang-start", "overhang-end", "indel", "chimera-equal", "chimera-unequal")


def _reads(rng, genes, n, L1, L2=None, paired=True, ragged=False, sub=0.01, n_rate=0.003, lower=0.05, qual=False, on_target=0.8):
    m1s, m2s, q1, q2 = [], [], [], []
    for i in range(n):
        l1 = int(rng.integers(max(1, L1 // 2), L1 + 1)) if ragged else L1
        l2 = int(rng.integers(max(1, (L2 or L1) // 2), (L2 or L1) + 1)) if ragged else (L2 or L1)
        g = genes[int(rng.integers(0, len(genes)))]
        mates = []
        for L in (l1, l2):
            m = _mate(rng, g, L, KINDS[int(rng.integers(0, len(KINDS)))]) if rng.random() < on_target else synth.random_seq(rng, L)
            s = rng.random(L) < sub
            m[s] = synth.ACGT[rng.integers(0, 4, size=int(s.sum()))]
            m[rng.random(L) < n_rate] = ord("N")
            lo = rng.random(L) < lower
            m[lo] |= 0x20
            mates.append(m)
        m1s.append(mates[0]); m2s.append(mates[1])
        if qual:
            for lst, m in ((q1, mates[0]), (q2, mates[1])):
                q = np.where(rng.random(len(m)) < 0.9, rng.integers(20, 42, size=len(m)), rng.integers(2, 20, size=len(m)))
                lst.append((q + 33).astype(np.uint8))
    return synth.batch_from_lists(m1s, m2s if paired else None, q1 if qual else None, q2 if (qual and paired) else None)


# ---------------------------------------------------------------------------
# geometry and content over the index kinds
# ---------------------------------------------------------------------------
@pytest.fixture(params=["auto", "bitvector"])
def chain(request, monkeypatch):
    monkeypatch.delenv("SHK_PROBE", raising=False)
    if request.param == "bitvector":
        monkeypatch.setenv("SHK_PROBE", "bitvector")
    return request.param


@pytest.mark.parametrize("k", [5, 16, 17, 31])
def test_mate_lengths(oracle, chain, k):
    """mates of k - 1, k, k + 63, k + 64, 75, 100, 150 and 300 bases, unequal mates, paired and single, uniform batches of 65 reads"""
    rng = np.random.default_rng(100 + k)
    genes = synth.make_genes(rng, 100, 600, 1400) if k > 5 else synth.make_genes(rng, 3, 80, 160)
    o, h, model = _build(oracle, genes, k=k)
    assert ("bitvector" in h.probe_mode()) == (chain == "bitvector"), h.probe_mode()
    some = 0
    for L1, L2 in ((k - 1, k), (k, k + 63), (k + 63, k + 64), (k + 64, 75), (75, 100), (100, 150), (150, 300), (300, 150)):
        for paired in (True, False):
            batch = _reads(rng, genes, 65, L1, L2, paired=paired)
            want, goff, _ = _check_host(o, h, model, batch)
            some += int((want[:, :, 2] > 0).sum())
    assert some > 200          # (not vacuous: supported placements were compared)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_batch_sizes_ragged_and_uniform(oracle, n):
    rng = np.random.default_rng(7 * n)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17)
    for ragged in (False, True):
        for paired in (True, False):
            _check_host(o, h, model, _reads(rng, genes, n, 100, 150, paired=paired, ragged=ragged))


def test_long_single_end_read(oracle):
    """one read of 1 500 bases (more slots than the kernel keeps in LDS) next to short ones"""
    rng = np.random.default_rng(5)
    genes = synth.make_genes(rng, 20, 2000, 3000)
    o, h, model = _build(oracle, genes, k=17)
    g = genes[3]
    long_read = synth.revcomp(g[100:1600]).copy()
    long_read[700] = ord("N")
    chim = np.concatenate([g[50:900], g[1200:1850]])
    batch = synth.batch_from_lists([long_read, g[10:110], chim, synth.random_seq(rng, 1500)])
    want, goff, gids = _check_host(o, h, model, batch)
    assert want[0, 0].tolist()[:2] == [1, 100] and want[0, 0, 2] > 1400
    assert len(chim) == 1500 and want[int(goff[2]), 0, 2] > 700


def test_quality_mask_and_lower_case(oracle, chain):
    rng = np.random.default_rng(11)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17, min_quality=20)
    for paired, ragged in ((True, False), (True, True), (False, True)):
        _check_host(o, h, model, _reads(rng, genes, 200, 100, 150, paired=paired, ragged=ragged, qual=True, lower=0.2), q=20)


def test_one_gene_index_and_non_power_of_two_filter(oracle):
    rng = np.random.default_rng(13)
    genes = synth.make_genes(rng, 1, 1500, 1500)
    o, h, model = _build(oracle, genes, k=17, bf_bits=1 << 33)
    assert h.probe_mode() == "lds-table"
    _check_host(o, h, model, _reads(rng, genes, 300, 100, paired=True))
    _check_host(o, h, model, _reads(rng, genes, 300, 100, 150, paired=True, ragged=True))
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17, bf_bits=3 << 33)          # -b 3
    assert h.probe_mode().endswith("-mod")
    _check_host(o, h, model, _reads(rng, genes, 300, 100, 150, paired=True, ragged=True))


@pytest.mark.parametrize("ref", ["tandem", "families", "interspersed"])
def test_repeat_rich_references(oracle, ref):
    """many slots are ambiguous (a k-mer twice in one gene) or shared between genes"""
    rng = np.random.default_rng(len(ref))
    if ref == "tandem":
        genes, _ = repeat_refs.compose(repeat_refs.tandem(rng, 37, 12, True), repeat_refs.plain(rng, 5))
    elif ref == "families":
        genes, _ = repeat_refs.families(rng, 3, 4, 900, 0.95)
    else:
        genes, _ = repeat_refs.interspersed(rng, synth.make_genes(rng, 12, 400, 900), 200, 10, 0.1)
    o, h, model = _build(oracle, genes, k=17)
    want, goff, gids = _check_host(o, h, model, _reads(rng, genes, 400, 100, 120, paired=True, ragged=True, on_target=1.0))
    if ref == "tandem":
        # one gene with a tandem array beside genes that share nothing: one association per read, and in the array gene more than
        # a hundred k-mers that occur twice or more (no vote) under reads that were assigned to it
        assert sum(len(v) > 1 for v in model.kmer_map(0).values()) > 100 and int((gids == 0).sum()) > 30
    else:
        assert int(goff[-1]) > 400      # reads with several associations, each placed in its own record's coordinates


def test_shared_stretch_and_six_way_tie(oracle):
    """reads from a stretch two genes share (two associations, own coordinates each) and reads tied over 6 identical genes (more than
    SHK_INLINE_IDS: their genes come from the EMIT pass)"""
    rng = np.random.default_rng(17)
    genes = synth.make_genes(rng, 10, 800, 1200)
    genes[4][300:700] = genes[2][50:450]
    twin = synth.random_seq(rng, 900)
    genes += [twin.copy() for _ in range(6)]
    o, h, model = _build(oracle, genes, k=17)
    shared = [genes[2][100 + i:250 + i] for i in range(0, 200, 7)]
    tied = [twin[i:i + 150] for i in range(0, 700, 23)]
    m2 = [synth.revcomp(r) for r in shared + tied]
    batch = synth.batch_from_lists(shared + tied, m2)
    want, goff, gids = _check_host(o, h, model, batch)
    a = int(goff[0])
    assert gids[a:a + 2].tolist() == [2, 4] and want[a, 0].tolist() == [0, 100, 134] and want[a + 1, 0].tolist() == [0, 350, 134]
    assert want[a, 1].tolist() == [1, 100, 134]
    t = int(goff[len(shared)])
    assert gids[t:t + 6].tolist() == list(range(10, 16)) and all(want[t + j, 0].tolist() == [0, 0, 134] for j in range(6))


def test_record_numbering_quirk(oracle):
    """an all-N first record (does not advance the counter) and a record shorter than k (advances it, adds nothing)"""
    rng = np.random.default_rng(19)
    g = synth.make_genes(rng, 4, 500, 700)
    genes = [np.full(60, ord("N"), np.uint8), g[0], synth.random_seq(rng, 9), g[1], np.full(40, ord("N"), np.uint8), g[2], g[3]]
    o, h, model = _build(oracle, genes, k=17)
    assert sorted(model.records) == [0, 2, 3, 4]
    real = [g[0], g[1], g[2], g[3]]
    want, goff, gids = _check_host(o, h, model, _reads(rng, real, 200, 100, paired=True))
    assert set(map(int, gids)) == {0, 2, 3, 4}


# ---------------------------------------------------------------------------
# the four families, the repair paths
# ---------------------------------------------------------------------------
def test_submit_wait_pipeline(oracle):
    from shark_amd import SharkHipError
    rng = np.random.default_rng(23)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17)
    h.placement_enable(True)
    batches = [_reads(rng, genes, n, 100, 150, paired=True, ragged=r) for n, r in ((300, False), (65, True), (1, False), (500, True))]
    tickets = []
    for b in batches[:3]:
        tickets.append(h.submit(*_args(b)))
    for on in (True, False):               # tickets outstanding: neither direction
        with pytest.raises(SharkHipError):
            h.placement_enable(on)
    for i, b in enumerate(batches):
        goff, gids = h.wait(tickets[i])
        _compare(o, model, b, goff, gids, h.placement_last())
        if i == 0:
            tickets.append(h.submit(*_args(batches[3])))


def test_resident_families_and_length_bound_repair(oracle):
    rng = np.random.default_rng(29)
    genes = synth.make_genes(rng, 100, 600, 1400)
    o, h, model = _build(oracle, genes, k=17)
    h.placement_enable(True)
    for ragged in (False, True):
        b = _reads(rng, genes, 300, 100, 150, paired=True, ragged=ragged)
        t = _to_device(b)
        r = h.classify_device(300, max_read_len=150, **_dev_ptrs(t))
        _compare(o, model, b, *_device_result(h, r))
        tk = h.submit_device(300, max_read_len=150, **_dev_ptrs(t))
        _compare(o, model, b, *_device_result(h, h.wait_device(tk)))
    # a bound that does not hold: reads of 3 000 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again)
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, model = _build(oracle, long_genes, k=17)
    h.placement_enable(True)
    mates = [long_genes[i % 3][50 * i:50 * i + (3000 if i % 5 == 0 else 100)] for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    tk = h.submit_device(40, max_read_len=100, **_dev_ptrs(t))
    goff, gids, got = _device_result(h, h.wait_device(tk))
    want = _compare(o, model, b, goff, gids, got)
    assert want[int(goff[0]), 0].tolist() == [0, 0, 2984] and h.timing()["last_n_long"] > 0


def test_association_overflow_repair(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 reads tied over 6 identical genes"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    genes = [twin.copy() for _ in range(6)]
    o, h, model = _build(oracle, genes, k=17)
    reads = [twin[(7 * i) % 500:(7 * i) % 500 + 100] for i in range(3000)]
    batch = synth.batch_from_lists(reads)
    want, goff, gids = _check_host(o, h, model, batch)
    assert int(goff[-1]) == 18000 and want[6, 0].tolist() == [0, 7, 84]


# ---------------------------------------------------------------------------
# state rules, inertness, all three modes
# ---------------------------------------------------------------------------
def test_state_rules(oracle):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    genes = synth.make_genes(rng, 5, 400, 600)
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError):
        h.placement_enable(True)                  # before finalize
    h.build([bytes(g) for g in genes])
    with pytest.raises(SharkHipError):
        h.placement_enable(True)                  # finalized without keep_positions
    with pytest.raises(SharkHipError):
        h.keep_positions()                        # after finalize
    o, h, model = _build(oracle, genes, k=17)
    with pytest.raises(SharkHipError):
        h.placement_last()                        # before any wait
    b = _reads(rng, genes, 50, 100, paired=True)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.placement_last()                        # the mode was off
    _check_host(o, h, model, b)
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    with pytest.raises(SharkHipError):
        h.placement_last()                        # behind shk_count_work
    h.placement_enable(False)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.placement_last()


def test_mode_off_is_inert_and_all_three_modes_agree(oracle):
    from shark_amd import SharkHip
    rng = np.random.default_rng(41)
    genes = synth.make_genes(rng, 100, 600, 1400)
    batches = [_reads(rng, genes, 300, 100, paired=True), _reads(rng, genes, 300, 100, 150, paired=True, ragged=True)]
    seen = []
    for keep, on in ((False, False), (True, False), (True, True)):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in genes], keep_positions=keep)
        h.placement_enable(on)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel()))
        seen.append((rows, h.gene_counts().tobytes()))
    assert seen[0] == seen[1] == seen[2]
    o, h, model = _build(oracle, genes, k=17)
    h.evidence_enable(True)
    h.candidates_enable(4)
    want, goff, gids = _check_host(o, h, model, batches[1])
    assert np.array_equal(h.evidence_last(), expected_evidence(o, batches[1]))
    wr, we = expected_candidates(o, batches[1], 4)
    gr, ge = h.candidates_last()
    assert np.array_equal(gr, wr) and np.array_equal(ge, we)


# ---------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------
def _run_shark(args, cwd):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([os.path.join(root, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def test_shark_placements_on_the_example(oracle, example_dir, tmp_path):
    import os
    from tests.placement_model import placement_lines
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(*_args(batch))
    model = PlacementModel([s for _, s in fa], 17)
    want = placement_lines([rid.decode() for rid, _, _ in r1], goff, gids, expected_placements(model, batch, goff, gids),
                           [name.decode() for name, _ in fa], True)
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq")]
    plain = _run_shark(base + ["-o", str(tmp_path / "p.1"), "-p", str(tmp_path / "p.2")], str(tmp_path))
    assert plain.returncode == 0, plain.stderr.decode()[-2000:]
    files = {}
    for tag, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "7"]),
                       ("c", ["--batch", "777", "--evidence", str(tmp_path / "c.ev"), "--candidates", str(tmp_path / "c.cd")])):
        o1, o2, pl = (tmp_path / ("%s.%s" % (tag, x)) for x in ("1.fq", "2.fq", "placements"))
        r = _run_shark(base + ["-o", str(o1), "-p", str(o2), "--placements", str(pl)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == plain.stdout
        assert o1.read_bytes() == (tmp_path / "p.1").read_bytes() and o2.read_bytes() == (tmp_path / "p.2").read_bytes()
        files[tag] = pl.read_bytes()
        got = pl.read_text().split("\n")
        assert got[-1] == "" and len(got) - 1 == int(goff[-1]) == 1929
        assert got[:-1] == want, next((i, a, w) for i, (a, w) in enumerate(zip(got, want)) if a != w)
    assert files["a"] == files["b"] == files["c"]
    assert sum(1 for ln in want if int(ln.split(" ")[4]) > 0) > 1800          # (not vacuous)


def test_shark_placements_synthetic_pairs_and_refusals(oracle, tmp_path):
    from tests.placement_model import placement_lines
    rng = np.random.default_rng(43)
    genes = synth.make_genes(rng, 30, 500, 900)
    b = _reads(rng, genes, 400, 100, 120, paired=True, ragged=True, lower=0.0)
    (tmp_path / "g.fa").write_text("".join(">g%d\n%s\n" % (i, bytes(g).decode()) for i, g in enumerate(genes)))
    for name, seq, off in (("1.fq", b["seq1"], b["off1"]), ("2.fq", b["seq2"], b["off2"])):
        with open(tmp_path / name, "w") as f:
            for i in range(400):
                s = bytes(seq[int(off[i]):int(off[i + 1])]).decode()
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    o = oracle.Shark(k=17, c=0.3, bf_bits=1 << 33)
    o.build([bytes(g) for g in genes])
    goff, gids = o.classify(*_args(b))
    model = PlacementModel([bytes(g) for g in genes], 17)
    want = placement_lines(["r%d" % i for i in range(400)], goff, gids, expected_placements(model, b, goff, gids), ["g%d" % i for i in range(30)], True)
    base = ["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq"), "-2", str(tmp_path / "2.fq"), "-c", "0.3", "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    r = _run_shark(base + ["--placements", str(tmp_path / "pl")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert (tmp_path / "pl").read_text().split("\n")[:-1] == want and len(want) > 100
    # single-end: three fields per line
    r = _run_shark(["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq"), "-c", "0.3", "-o", str(tmp_path / "o1"), "--placements", str(tmp_path / "pl1")], str(tmp_path))
    assert r.returncode == 0 and all(len(ln.split(" ")) == 5 for ln in (tmp_path / "pl1").read_text().split("\n")[:-1])
    # a reference of more than 65 536 records: a message and exit code 1
    with open(tmp_path / "wide.fa", "w") as f:
        for i in range(65537):
            f.write(">w%d\nACGTACGTTGCATGCAAGCT\n" % i)
    r = _run_shark(["-r", str(tmp_path / "wide.fa"), "-1", str(tmp_path / "1.fq"), "-o", str(tmp_path / "o1"), "--placements", str(tmp_path / "plw")], str(tmp_path))
    assert r.returncode == 1 and b"more than 65536 records" in r.stderr
