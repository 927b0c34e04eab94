"""Segments mode on the GPU (shk_segments_enable / shk_segments_last): per association and mate the m diagonals with the most votes,
each with its first and last voting slot, and the number of distinct diagonals -- bit for bit equal to the model
(tests/segments_model.py), which is written from the semantics and never asks the filter.  Integers, no tolerances.  After every
batch the genes and offsets are compared with the CPU oracle's as well.

Run on the GPU box with `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import torch  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from tests import repeat_refs, synth
from tests.placement_model import PlacementModel, expected_placements
from tests.segments_model import SegmentsModel, expected_segments, junction_lines, mate_lengths, segment_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return o, h, SegmentsModel([bytes(g) for g in genes], kw.get("k", 17))


def _to_device(b):
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in b.items() if v is not None}
    torch.cuda.synchronize()
    return t


def _dev_ptrs(t):
    g = lambda k: t[k].data_ptr() if k in t else 0  # noqa: E731
    return dict(seq1=g("seq1"), off1=g("off1"), seq2=g("seq2"), off2=g("off2"), qual1=g("qual1"), qual2=g("qual2"))


def _device_result(h, r):
    from shark_amd.capi import hip_memcpy_dtoh, segments_from_device
    n, tot = int(r.n), int(r.n_assoc)
    goff, gids = np.zeros(n + 1, np.uint32), np.zeros(tot, np.uint16)
    hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    if tot:
        hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    na, m, kp, ep = h.segments_last()
    assert na == tot
    return goff, gids, segments_from_device(na, m, kp, ep)


def _compare(o, model, batch, goff, gids, got, m, q=0):
    og, oi = o.classify(*_args(batch))
    assert np.array_equal(og, goff) and np.array_equal(oi, gids), "genes differ from the oracle"
    wk, wr = expected_segments(model, batch, goff, gids, m, q)
    gk, gr = got
    assert gk.shape == wk.shape and gr.shape == wr.shape and gr.dtype == np.int64
    bad = np.nonzero((gk != wk).any(axis=1) | (gr != wr).reshape(len(wr), 2 * m * 5).any(axis=1))[0]
    assert len(bad) == 0, "association %d: got %s %s, model %s %s (%d differ)" % (bad[0], gk[bad[0]].tolist(), gr[bad[0]].tolist(), wk[bad[0]].tolist(),
                                                                                  wr[bad[0]].tolist(), len(bad))
    return wk, wr


def _check_host(o, h, model, batch, m=4, q=0):
    h.segments_enable(m)
    goff, gids = h.classify(*_args(batch))
    wk, wr = _compare(o, model, batch, goff, gids, h.segments_last(), m, q)
    return wk, wr, goff, gids


# ---------------------------------------------------------------------------
# reads: cut from several exons of a gene (1 to 3 junctions), with the placement tests' kinds mixed in
# ---------------------------------------------------------------------------
def _spliced(rng, g, L, n_junc):
    """L bases cut from n_junc + 1 exons of g, in record order, introns of 30 bases or more; either strand"""
    cuts = np.sort(rng.integers(12, max(13, L - 12), size=n_junc)) if n_junc else np.zeros(0, np.int64)
    sizes = np.diff(np.concatenate([[0], cuts, [L]])).astype(int)
    sizes = sizes[sizes > 0]
    room = len(g) - L
    gaps = np.sort(rng.integers(0, max(1, room), size=len(sizes)))
    parts, at, prev_gap = [], 0, 0
    for sz, gap in zip(sizes, gaps):
        gap = max(int(gap), prev_gap + (30 if parts else 0))
        parts.append(g[at + gap:at + gap + sz])
        at += sz
        prev_gap = gap
    m = np.concatenate(parts)[:L]
    if len(m) < L:
        m = np.concatenate([m, synth.random_seq(rng, L - len(m))])
    m = m.copy()
    return synth.revcomp(m) if rng.random() < 0.5 else m


def _reads(rng, genes, n, L1, L2=None, paired=True, ragged=False, sub=0.01, n_rate=0.003, lower=0.05, qual=False, on_target=0.85, max_junc=3):
    m1s, m2s, q1, q2 = [], [], [], []
    for i in range(n):
        l1 = int(rng.integers(max(1, L1 // 2), L1 + 1)) if ragged else L1
        l2 = int(rng.integers(max(1, (L2 or L1) // 2), (L2 or L1) + 1)) if ragged else (L2 or L1)
        g = genes[int(rng.integers(0, len(genes)))]
        mates = []
        for L in (l1, l2):
            if rng.random() < on_target and len(g) > L + 200:
                m = _spliced(rng, g, L, int(rng.integers(0, max_junc + 1)) if L >= 40 else 0)
            elif rng.random() < on_target:
                m = g[:L].copy() if len(g) >= L else np.concatenate([g, synth.random_seq(rng, L - len(g))])
            else:
                m = synth.random_seq(rng, L)
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


@pytest.fixture(scope="module")
def genes_2to5kb():
    return synth.make_genes(np.random.default_rng(2024), 6, 2000, 5000)


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 17, 31])
def test_k_and_mate_lengths(oracle, k):
    """mates with 0, 1, 63, 64, 65, 512, 513 and about 1 500 slots: the chunk of 64 slots and the 512 slots kept in LDS"""
    rng = np.random.default_rng(100 + k)
    genes = synth.make_genes(rng, 4, 2000, 3000) if k > 5 else synth.make_genes(rng, 2, 1600, 1700)
    o, h, model = _build(oracle, genes, k=k)
    slots = (0, 1, 63, 64, 65, 512, 513, 1500)
    some = multi = 0
    for s1, s2 in zip(slots, slots[1:] + slots[:1]):
        for paired in (True, False):
            batch = _reads(rng, genes, 6, s1 + k - 1, s2 + k - 1, paired=paired, lower=0.0, n_rate=0.001)
            wk, wr, _, _ = _check_host(o, h, model, batch)
            some += int((wr[:, :, 0, 2] > 0).sum())
            multi += int((wk > 1).sum())
    assert some > 60 and multi > 20          # (not vacuous: supported and spliced mates were compared)


@pytest.mark.parametrize("sub", [0.0, 0.01])
@pytest.mark.parametrize("paired", [True, False])
def test_spliced_reads(oracle, genes_2to5kb, sub, paired):
    """mates cut from one to four exons on either strand; the junctions the model derives are there"""
    from tests.segments_model import junctions
    rng = np.random.default_rng(7 + int(paired) + int(sub * 1000))
    o, h, model = _build(oracle, genes_2to5kb, k=17)
    batch = _reads(rng, genes_2to5kb, 300, 100, 150, paired=paired, sub=sub, n_rate=0.0, lower=0.0, on_target=1.0)
    wk, wr, goff, gids = _check_host(o, h, model, batch)
    lengths = mate_lengths(batch)
    read_of = np.repeat(np.arange(300), np.diff(goff))
    n_j = sum(len(junctions(wr[j, t], int(lengths[read_of[j], t]), 17, 8)) for j in range(len(gids)) for t in range(2))
    assert n_j > 150 and int((wk >= 3).sum()) > 30


@pytest.mark.parametrize("m", [1, 2, 4])
def test_more_keys_than_entries(oracle, genes_2to5kb, m):
    rng = np.random.default_rng(50 + m)
    o, h, model = _build(oracle, genes_2to5kb, k=17)
    batch = _reads(rng, genes_2to5kb, 200, 150, paired=True, on_target=1.0, max_junc=6)
    wk, wr, _, _ = _check_host(o, h, model, batch, m=m)
    assert wr.shape[2] == m and int((wk > m).sum()) > (20 if m < 4 else 5)


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_batch_sizes_ragged_and_uniform(oracle, genes_2to5kb, n):
    rng = np.random.default_rng(7 * n)
    o, h, model = _build(oracle, genes_2to5kb, k=17)
    for ragged in (False, True):
        _check_host(o, h, model, _reads(rng, genes_2to5kb, n, 100, 120, paired=True, ragged=ragged))


def test_quality_mask_and_lower_case(oracle, genes_2to5kb):
    rng = np.random.default_rng(11)
    o, h, model = _build(oracle, genes_2to5kb, k=17, min_quality=20)
    for paired, ragged in ((True, False), (False, True)):
        _check_host(o, h, model, _reads(rng, genes_2to5kb, 200, 100, 150, paired=paired, ragged=ragged, qual=True, lower=0.2), q=20)


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
    wk, wr, goff, gids = _check_host(o, h, model, _reads(rng, genes, 300, 100, 120, paired=True, ragged=True, on_target=1.0))
    assert int((wk > 1).sum()) > 30


def test_record_numbering_quirk(oracle):
    """an all-N first record (does not advance the counter) and a record shorter than k (advances it, adds nothing)"""
    rng = np.random.default_rng(19)
    g = synth.make_genes(rng, 4, 900, 1200)
    genes = [np.full(60, ord("N"), np.uint8), g[0], synth.random_seq(rng, 9), g[1], np.full(40, ord("N"), np.uint8), g[2], g[3]]
    o, h, model = _build(oracle, genes, k=17)
    assert sorted(model.records) == [0, 2, 3, 4]
    wk, wr, goff, gids = _check_host(o, h, model, _reads(rng, [g[0], g[1], g[2], g[3]], 200, 100, paired=True))
    assert set(map(int, gids)) == {0, 2, 3, 4}


# ---------------------------------------------------------------------------
# the four families, the repair paths
# ---------------------------------------------------------------------------
def test_submit_wait_pipeline(oracle, genes_2to5kb):
    from shark_amd import SharkHipError
    rng = np.random.default_rng(23)
    genes = genes_2to5kb
    o, h, model = _build(oracle, genes, k=17)
    h.segments_enable(3)
    batches = [_reads(rng, genes, n, 100, 150, paired=True, ragged=r) for n, r in ((300, False), (65, True), (1, False), (400, True))]
    tickets = [h.submit(*_args(b)) for b in batches[:3]]
    for m in (2, 0):                        # tickets outstanding: neither direction
        with pytest.raises(SharkHipError):
            h.segments_enable(m)
    for i, b in enumerate(batches):
        goff, gids = h.wait(tickets[i])
        _compare(o, model, b, goff, gids, h.segments_last(), 3)
        if i == 0:
            tickets.append(h.submit(*_args(batches[3])))


def test_resident_families_and_length_bound_repair(oracle, genes_2to5kb):
    rng = np.random.default_rng(29)
    genes = genes_2to5kb
    o, h, model = _build(oracle, genes, k=17)
    h.segments_enable(4)
    for ragged in (False, True):
        b = _reads(rng, genes, 300, 100, 150, paired=True, ragged=ragged)
        t = _to_device(b)
        r = h.classify_device(300, max_read_len=150, **_dev_ptrs(t))
        _compare(o, model, b, *_device_result(h, r), 4)
        tk = h.submit_device(300, max_read_len=150, **_dev_ptrs(t))
        _compare(o, model, b, *_device_result(h, h.wait_device(tk)), 4)
    # a bound that does not hold: mates of 1 800 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again)
    mates = [np.concatenate([genes[i % 6][20 * i:20 * i + (900 if i % 5 == 0 else 50)], genes[i % 6][1000 + 20 * i:1000 + 20 * i + (900 if i % 5 == 0 else 50)]])
             for i in range(40)]
    b = synth.batch_from_lists(mates, [synth.revcomp(m) for m in mates])
    t = _to_device(b)
    tk = h.submit_device(40, max_read_len=100, **_dev_ptrs(t))
    goff, gids, got = _device_result(h, h.wait_device(tk))
    wk, wr = _compare(o, model, b, goff, gids, got, 4)
    a = int(goff[0])
    assert wr[a, 0, :2, :2].tolist() == [[0, 0], [0, 100]] and wr[a, 0, :2, 2].min() >= 884 and wr[a, 0, 1, 4] == 1783 and h.timing()["last_n_long"] > 0


def test_association_overflow_repair(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 reads tied over 6 identical genes"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    genes = [twin.copy() for _ in range(6)]
    o, h, model = _build(oracle, genes, k=17)
    reads = [np.concatenate([twin[(7 * i) % 200:(7 * i) % 200 + 50], twin[300 + (7 * i) % 200:350 + (7 * i) % 200]]) for i in range(3000)]
    batch = synth.batch_from_lists(reads)
    wk, wr, goff, gids = _check_host(o, h, model, batch, m=2)
    assert int(goff[-1]) == 18000 and wr[6, 0, :, :2].tolist() == [[0, 7], [0, 257]] and wr[6, 0, :, 2].min() >= 34 and wk[6].tolist() == [2, 0]


# ---------------------------------------------------------------------------
# state rules, inertness, all modes
# ---------------------------------------------------------------------------
def test_state_rules(oracle):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    genes = synth.make_genes(rng, 5, 400, 600)
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError):
        h.segments_enable(4)                      # before finalize
    h.segments_enable(0)                          # (off is always allowed)
    h.build([bytes(g) for g in genes])
    with pytest.raises(SharkHipError):
        h.segments_enable(4)                      # finalized without keep_positions
    o, h, model = _build(oracle, genes, k=17)
    with pytest.raises(SharkHipError, match="SHK_MAX_SEGMENTS"):
        h.segments_enable(5)
    with pytest.raises(SharkHipError):
        h.segments_last()                         # before any wait
    b = _reads(rng, genes, 50, 100, paired=True)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.segments_last()                         # the mode was off
    _check_host(o, h, model, b)
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    with pytest.raises(SharkHipError):
        h.segments_last()                         # behind shk_count_work
    h.segments_enable(0)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.segments_last()
    # a wider index than ids can name: refused as placement mode is
    wide = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    wide.build([b"ACGTACGTTGCATGCAAGCT"] * 65537, keep_positions=True)
    with pytest.raises(SharkHipError, match="65 536"):
        wide.segments_enable(1)


def test_mode_off_is_inert_and_all_modes_agree(oracle, genes_2to5kb):
    from shark_amd import SharkHip
    from tests.candidates_model import expected_candidates
    from tests.evidence_model import expected_evidence
    rng = np.random.default_rng(41)
    genes = genes_2to5kb
    batches = [_reads(rng, genes, 300, 100, paired=True), _reads(rng, genes, 300, 100, 150, paired=True, ragged=True)]
    seen = []
    for m in (0, 1, 4):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in genes], keep_positions=True)
        h.placement_enable(True)
        h.segments_enable(m)
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.placement_last().tobytes()))
        seen.append((rows, h.gene_counts().tobytes()))
    assert seen[0] == seen[1] == seen[2]
    # every mode at once: segment 0 is the placement record, and the other modes' records are what they are without segments
    o, h, model = _build(oracle, genes, k=17)
    h.evidence_enable(True)
    h.candidates_enable(4)
    h.placement_enable(True)
    h.depth_enable(1)
    wk, wr, goff, gids = _check_host(o, h, model, batches[1])
    pl = h.placement_last()
    assert np.array_equal(pl, wr[:, :, 0, :3]) and np.array_equal(pl, expected_placements(PlacementModel([bytes(g) for g in genes], 17), batches[1], goff, gids))
    assert np.array_equal(h.evidence_last(), expected_evidence(o, batches[1]))
    cr, ce = expected_candidates(o, batches[1], 4)
    gr, ge = h.candidates_last()
    assert np.array_equal(gr, cr) and np.array_equal(ge, ce)
    assert h.depth_mates() == int((pl[:, :, 2] >= 1).sum())


# ---------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------
def _run_shark(args, cwd):
    return subprocess.run([os.path.join(ROOT, "shark_amd", "bin", "shark")] + args, cwd=cwd, capture_output=True)


def test_shark_segments_and_junctions_on_the_example(oracle, example_dir, tmp_path):
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    r1 = synth.read_fastq(os.path.join(example_dir, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(example_dir, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(*_args(batch))
    model = SegmentsModel([s for _, s in fa], 17)
    legend = [name.decode() for name, _ in fa]
    keys, rows = expected_segments(model, batch, goff, gids, 4)
    want = segment_lines([rid.decode() for rid, _, _ in r1], goff, gids, keys, rows, legend, True)
    want_j = junction_lines(goff, gids, rows, mate_lengths(batch), 17, legend, 8)
    base = ["-r", os.path.join(example_dir, "ENSG00000277117.fa"), "-1", os.path.join(example_dir, "sample_1.fq"),
            "-2", os.path.join(example_dir, "sample_2.fq")]
    plain = _run_shark(base + ["-o", str(tmp_path / "p.1"), "-p", str(tmp_path / "p.2")], str(tmp_path))
    assert plain.returncode == 0, plain.stderr.decode()[-2000:]
    files = {}
    for tag, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "7"]),
                       ("c", ["--batch", "777", "--placements", str(tmp_path / "c.pl"), "--depth", str(tmp_path / "c.dp")])):
        o1, o2, sg, jn = (tmp_path / ("%s.%s" % (tag, x)) for x in ("1.fq", "2.fq", "segments", "junctions"))
        r = _run_shark(base + ["-o", str(o1), "-p", str(o2), "--segments", str(sg), "--junctions", str(jn)] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == plain.stdout
        assert o1.read_bytes() == (tmp_path / "p.1").read_bytes() and o2.read_bytes() == (tmp_path / "p.2").read_bytes()
        files[tag] = (sg.read_bytes(), jn.read_bytes())
        got = sg.read_text().split("\n")
        assert got[-1] == "" and len(got) - 1 == int(goff[-1]) == 1929
        assert got[:-1] == want, next((i, a, w) for i, (a, w) in enumerate(zip(got, want)) if a != w)
        assert jn.read_text().split("\n")[:-1] == want_j
    assert files["a"] == files["b"] == files["c"]
    assert len(want_j) >= 2 and sum(int(ln.split(" ")[4]) for ln in want_j) > 500          # (not vacuous)
    # --junctions alone, another floor and fewer entries per mate
    r = _run_shark(base + ["-o", str(tmp_path / "d.1"), "-p", str(tmp_path / "d.2"), "--junctions", str(tmp_path / "d.jn"), "--junctions-min-support", "12",
                           "--segments-max", "2"], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    k2, r2_ = expected_segments(model, batch, goff, gids, 2)
    assert (tmp_path / "d.jn").read_text().split("\n")[:-1] == junction_lines(goff, gids, r2_, mate_lengths(batch), 17, legend, 12)


def test_shark_segments_synthetic_pairs_and_refusals(oracle, genes_2to5kb, tmp_path):
    rng = np.random.default_rng(43)
    genes = genes_2to5kb
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
    model = SegmentsModel([bytes(g) for g in genes], 17)
    legend = ["g%d" % i for i in range(len(genes))]
    keys, rows = expected_segments(model, b, goff, gids, 3)
    want = segment_lines(["r%d" % i for i in range(400)], goff, gids, keys, rows, legend, True)
    want_j = junction_lines(goff, gids, rows, mate_lengths(b), 17, legend, 8)
    base = ["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq"), "-2", str(tmp_path / "2.fq"), "-c", "0.3", "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    outs = []
    for extra in ([], ["--gpus", "2", "--devices", "0,0", "--batch", "37"]):
        r = _run_shark(base + ["--segments", str(tmp_path / "sg"), "--junctions", str(tmp_path / "jn"), "--segments-max", "3"] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert (tmp_path / "sg").read_text().split("\n")[:-1] == want and len(want) > 100
        assert (tmp_path / "jn").read_text().split("\n")[:-1] == want_j and len(want_j) > 50
        outs.append(((tmp_path / "sg").read_bytes(), (tmp_path / "jn").read_bytes()))
    assert outs[0] == outs[1]
    # single-end: one mate's fields per line
    r = _run_shark(["-r", str(tmp_path / "g.fa"), "-1", str(tmp_path / "1.fq"), "-c", "0.3", "-o", str(tmp_path / "o1"), "--segments", str(tmp_path / "sg1")], str(tmp_path))
    assert r.returncode == 0 and all(len(ln.split(" ")) == 2 + 1 + 4 * 5 for ln in (tmp_path / "sg1").read_text().split("\n")[:-1])
    # a reference of more than 65 536 records: a message and exit code 1
    with open(tmp_path / "wide.fa", "w") as f:
        for i in range(65537):
            f.write(">w%d\nACGTACGTTGCATGCAAGCT\n" % i)
    for flag in ("--segments", "--junctions"):
        r = _run_shark(["-r", str(tmp_path / "wide.fa"), "-1", str(tmp_path / "1.fq"), "-o", str(tmp_path / "o1"), flag, str(tmp_path / "w")], str(tmp_path))
        assert r.returncode == 1 and b"more than 65536 records" in r.stderr
