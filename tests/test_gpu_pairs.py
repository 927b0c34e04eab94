"""Pairs mode on the GPU (shk_pairs_enable / shk_pairs_last / shk_fragments_get / shk_fragments_reset, `shark --sam-pairs`,
`shark --fragments`): per association the 32-byte pair record and, over the counted batches, the fragments state, against the model
(tests/pairs_model.py) byte for byte -- fed the device's own alignment records and, on the case table, the alignment model's as well.
No tolerances anywhere.

Run on the GPU box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import torch  # noqa: F401  torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import synth
from tests.align_model import sam_header
from tests.pairs_cases import MAX_FRAG, MIN_INTRON, N_BINS, case_batch, check_expectations, pair_cases, s_min_for
from tests.pairs_model import Fragments, expected_pairs
from tests.spliced_synth import spliced_gene, spliced_reads
from tests.test_gpu_align import model_records, run_shark, same_records
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import device_assoc
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu

GRID_LANES = 512 * 256          # pair_kernel's capped grid: more reads than this take the stride loop's second trip


def same_pairs(got, want):
    assert got.dtype == capi.PAIR_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
        raise AssertionError("association %d: got %s, model %s (%d records differ)" % (bad[0], got[bad[0]], want[bad[0]], len(bad)))


def same_state(h, model, n_bins):
    hist, classes = h.fragments(n_bins)
    mh, mc = model.arrays()
    assert np.array_equal(classes, mc), (classes, mc)
    assert np.array_equal(hist, mh), (np.nonzero(hist != mh)[0][:8], hist[hist != mh][:8], mh[hist != mh][:8])


def classify_pairs(h, batch, min_intron=MIN_INTRON, max_frag=MAX_FRAG):
    """(gene_off, gene_ids, the device's alignment records, its pair records, the model's pair records from the device's alignments)"""
    goff, gids = h.classify(*_args(batch))
    al, pr = h.alignments_last(), h.pairs_last()
    want = expected_pairs(al, batch, goff, min_intron, max_frag)
    same_pairs(pr, want)
    return goff, gids, al, pr


# ---------------------------------------------------------------------------
# (a) the case table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,ref", [(17, "one gene"), (17, "twins"), (5, "one gene"), (31, "one gene")])
def test_case_table(oracle, k, ref):
    """every class, tie-break and edge of the fragment length (tests/pairs_cases.py) on a gene of 2.4 kb at L = 60: the records equal the
    model's from the device's own alignment records and from the alignment model's; the twins give mapq 3 and no histogram entry"""
    rec, names, batch, expect = case_batch(k)
    every = 2 if ref == "twins" else 1
    o, h, sm = build_kb(oracle, [rec] * every, k=k)
    h.alignments_enable(s_min_for(k))
    h.pairs_enable(MIN_INTRON, MAX_FRAG, N_BINS)
    goff, gids, al, pr = classify_pairs(h, batch)
    al_model = model_records(o, sm, batch, goff, gids, s_min_for(k))
    same_records(al, al_model)
    same_pairs(pr, expected_pairs(al_model, batch, goff, MIN_INTRON, MAX_FRAG))
    print("k", k, ref, "classes", np.bincount(pr["cls"], minlength=6).tolist(), "proper", int(pr["proper"].sum()))
    if k == 17:
        check_expectations(names, pr, goff, expect, every)
        assert set(pr["cls"].tolist()) == {0, 1, 2, 3, 4, 5} and (pr["mapq"] == (3 if every == 2 else 60)).all()
    fr = Fragments(N_BINS).add(pr, goff)
    same_state(h, fr, N_BINS)
    if ref == "twins":
        assert sum(fr.hist) == 0 and fr.classes[3] > 0
    elif k == 17:
        assert fr.hist[N_BINS - 2] == 1 and fr.hist[N_BINS - 1] == 2


@pytest.mark.parametrize("k", [5, 31])
def test_spliced_batches_at_k5_and_k31(oracle, k):
    """the alignment tests' geometry batches (150 pairs over one to five junctions, both strands, 3 % substitutions) on records short
    enough for k = 5 to vote: whatever the alignments are, the pair records are the model's"""
    from tests.align_cases import geometry_case
    genes, s_min, batch = geometry_case(k, "two genes", 1)
    o, h, sm = build_kb(oracle, [g for g, _ in genes], k=k)
    h.alignments_enable(s_min)
    h.pairs_enable(MIN_INTRON, 120, 128)
    goff, gids, al, pr = classify_pairs(h, batch, max_frag=120)
    print("k", k, "classes", np.bincount(pr["cls"], minlength=6).tolist(), "proper", int(pr["proper"].sum()), "with introns", int((pr["introns"] > 0).sum()))
    assert len(set(pr["cls"].tolist())) >= 4 and (pr["introns"] > 0).any()
    same_state(h, Fragments(128).add(pr, goff), 128)


# ---------------------------------------------------------------------------
# (b) the histogram
# ---------------------------------------------------------------------------
def tiled_batch(rng, m1, m2, n, every):
    """n pairs: pair (i / every) of the set at every `every`-th place, off-target random mates of 60 bases elsewhere"""
    junk = synth.ACGT[rng.integers(0, 4, size=(2, n, 60))]
    a = [m1[(i // every) % len(m1)] if i % every == 0 else junk[0, i] for i in range(n)]
    b = [m2[(i // every) % len(m2)] if i % every == 0 else junk[1, i] for i in range(n)]
    return synth.batch_from_lists(a, b)


def test_histogram_accumulates_over_workgroups_stride_trips_and_batches(oracle):
    """64 bins, so that most of the table's fragments land in the overflow bin.  Batch 1: 700 pairs, more than one workgroup's 256
    lanes, every second one on target.  Batch 2: more pairs than the grid has lanes -- the stride loop's second trip and the flush of
    every workgroup of the capped grid --, one in 113 on target, the rest random.  The two accumulate; reset empties the state"""
    rng = np.random.default_rng(5)
    rec, names, m1, m2, expect = pair_cases(17, n_bins=64)
    o, h, sm = build_kb(oracle, [rec], k=17)
    h.alignments_enable(8)
    h.pairs_enable(MIN_INTRON, MAX_FRAG, 64)
    fr = Fragments(64)
    small = tiled_batch(rng, m1, m2, 700, 2)
    goff, gids, al, pr = classify_pairs(h, small)
    assert len(gids) == 350
    fr.add(pr, goff)
    same_state(h, fr, 64)
    assert fr.hist[62] >= 12 and fr.hist[63] > fr.hist[62] and sum(fr.hist) == fr.classes[3]
    after_one = fr.arrays()
    n = GRID_LANES + 700
    big = tiled_batch(rng, m1, m2, n, 113)
    goff, gids, al, pr = classify_pairs(h, big)
    # (a random mate now and then passes the 2^26-bit filter by a false positive: such a read is associated and aligns nowhere, class 0)
    on_target = (n + 112) // 113
    assert len(gids) >= on_target and int((pr["cls"] != 0).sum()) >= on_target - 45 and int(goff[GRID_LANES]) < len(gids) - 2, "on-target pairs behind the grid's last lane"
    fr.add(pr, goff)
    same_state(h, fr, 64)
    hist, classes = h.fragments(64)
    assert int(classes.sum()) == 350 + len(gids) and not np.array_equal(hist, after_one[0])
    h.fragments_reset()
    same_state(h, Fragments(64), 64)
    goff, gids, al, pr = classify_pairs(h, small)
    same_state(h, Fragments(64).add(pr, goff), 64)


# ---------------------------------------------------------------------------
# (c) the four families, a single-end batch
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def panel():
    rng = np.random.default_rng(2027)
    return [spliced_gene(rng, int(rng.integers(1, 5)), 17) for _ in range(12)]


def test_all_four_families_and_a_single_end_batch(oracle, panel):
    rng = np.random.default_rng(58)
    o, h, sm = build_kb(oracle, [g for g, _ in panel], k=17)
    batches = [spliced_reads(rng, panel, n, ragged=r, paired=p, sub=0.03) for n, r, p in ((200, False, True), (65, True, True), (150, True, False))]
    dev = [_to_device(b) for b in batches]
    h.alignments_enable(6)
    h.pairs_enable(MIN_INTRON, 150, 256)
    fr = Fragments(256)
    want = []
    for b in batches:                                            # host batches: pinned memory
        goff, gids, al, pr = classify_pairs(h, b, max_frag=150)
        want.append((goff, gids, pr))
        fr.add(pr, goff)
    assert set(want[2][2]["cls"].tolist()) == {0, 1} or set(want[2][2]["cls"].tolist()) == {1}          # single-end
    assert len(set(want[0][2]["cls"].tolist())) >= 4 and set(want[0][2]["proper"].tolist()) == {0, 1}
    t0, t1 = h.submit(*_args(batches[0])), h.submit(*_args(batches[1]))
    for t, w in ((t0, want[0]), (t1, want[1])):                  # two tickets in flight: each wait hands out its own batch's records
        goff, gids = h.wait(t)
        assert np.array_equal(goff, w[0]) and np.array_equal(gids, w[1])
        same_pairs(h.pairs_last(), w[2])
        fr.add(w[2], w[0])

    def resident(i):
        return h.classify_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i]))

    def resident_submit(i):
        return h.wait_device(h.submit_device(len(batches[i]["off1"]) - 1, max_read_len=120, **_dev_ptrs(dev[i])))

    for family in (resident, resident_submit):                   # resident batches: the records stay in device memory
        for i, w in enumerate(want):
            goff, gids = device_assoc(family(i))
            assert np.array_equal(goff, w[0]) and np.array_equal(gids, w[1])
            n, ptr = h.pairs_last()
            assert n == len(gids)
            same_pairs(capi.pairs_from_device(n, ptr), w[2])
            fr.add(w[2], w[0])
    same_state(h, fr, 256)                                       # every batch of every family counted once


# ---------------------------------------------------------------------------
# (d) the repair paths
# ---------------------------------------------------------------------------
def test_association_overflow_repair(oracle):
    """more associations than a slot reserves (two per read + 4 096): 3 000 pairs tied over 6 identical genes -- records and counts come
    from the tail's second run in wait, once"""
    rng = np.random.default_rng(31)
    twin = synth.random_seq(rng, 600)
    o, h, sm = build_kb(oracle, [twin.copy() for _ in range(6)], k=17)
    h.alignments_enable(8)
    h.pairs_enable(MIN_INTRON, MAX_FRAG, N_BINS)
    a = [(7 * i) % 200 for i in range(3000)]
    batch = synth.batch_from_lists([twin[x:x + 50] for x in a], [synth.revcomp(twin[300 + x:350 + x]) for x in a])
    goff, gids, al, pr = classify_pairs(h, batch)
    assert int(goff[-1]) == 18000 and (pr["cls"] == 3).all() and (pr["frag"] == 350).all() and (pr["mapq"] == 0).all() and (pr["proper"] == 0).all()
    hist, classes = h.fragments(N_BINS)
    assert classes.tolist() == [0, 0, 0, 18000, 0, 0] and int(hist.sum()) == 0


def test_length_bound_repair(oracle):
    """mates of 1 500 bases behind max_read_len = 100 are repaired in wait (general kernel, tail again): the records are the final ones
    and the batch is counted once"""
    rng = np.random.default_rng(29)
    long_genes = synth.make_genes(rng, 3, 4000, 5000)
    o, h, sm = build_kb(oracle, long_genes, k=17)
    h.alignments_enable(8)
    h.pairs_enable(MIN_INTRON, 5000, 4096)
    size = lambda i: 1500 if i % 5 == 0 else 50  # noqa: E731
    m1 = [long_genes[i % 3][10 * i:10 * i + size(i)] for i in range(40)]
    m2 = [synth.revcomp(long_genes[i % 3][2000 + 10 * i:2000 + 10 * i + size(i)]) for i in range(40)]
    b = synth.batch_from_lists(m1, m2)
    t = _to_device(b)
    goff, gids = device_assoc(h.wait_device(h.submit_device(40, max_read_len=100, **_dev_ptrs(t))))
    assert h.timing()["last_n_long"] > 0
    n, ptr = h.alignments_last()
    al = capi.alignments_from_device(n, ptr)
    n, ptr = h.pairs_last()
    pr = capi.pairs_from_device(n, ptr)
    same_pairs(pr, expected_pairs(al, b, goff, MIN_INTRON, 5000))
    assert len(pr) == 40 and (pr["cls"] == 3).all() and sorted(set(pr["frag"].tolist())) == [2050, 3500] and pr["proper"].all()
    fr = Fragments(4096).add(pr, goff)
    same_state(h, fr, 4096)
    assert fr.hist[2050] == 32 and fr.hist[3500] == 8


# ---------------------------------------------------------------------------
# (e) state and argument rules
# ---------------------------------------------------------------------------
def test_state_and_argument_rules(oracle, panel):
    from shark_amd import SharkHip, SharkHipError
    rng = np.random.default_rng(37)
    records = [g for g, _ in panel]
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError, match="not finalized"):
        h.pairs_enable()
    h.pairs_enable(n_bins=0)                      # (switching off is always allowed)
    for call in (lambda: h.fragments(1024), h.fragments_reset):
        with pytest.raises(SharkHipError, match="never enabled"):
            call()
    o, h, sm = build_kb(oracle, records, keep_bases=False, k=17)
    with pytest.raises(SharkHipError, match="without shk_ref_keep_bases"):
        h.pairs_enable()
    o, h, sm = build_kb(oracle, records, k=17)
    with pytest.raises(SharkHipError, match="alignments mode is off"):
        h.pairs_enable()
    h.alignments_enable(8)
    for bad in (dict(n_bins=1), dict(n_bins=4097), dict(min_intron=0)):
        with pytest.raises(SharkHipError, match="invalid argument|n_bins"):
            h.pairs_enable(**bad)
    with pytest.raises(SharkHipError):
        h.pairs_last()                            # no batch yet
    b = spliced_reads(rng, panel, 50)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.pairs_last()                            # that batch was submitted with the mode off
    h.pairs_enable(20, 300, 128)
    with pytest.raises(SharkHipError):
        h.fragments(64)                           # not the state's n_bins
    assert int(h.fragments(128)[1].sum()) == 0    # the first enable cleared the state
    h.pairs_enable(20, 300, 64)                   # another n_bins while nothing was counted: the state is allocated anew
    assert len(h.fragments(64)[0]) == 64
    goff, gids, al, pr = classify_pairs(h, b, 20, 300)
    with pytest.raises(SharkHipError, match="n_bins"):
        h.pairs_enable(20, 300, 128)              # ... and not behind a counted batch
    h.pairs_enable(25, 300, 64)                   # other parameters at the same n_bins are fine
    h.fragments_reset()
    h.pairs_enable(20, 300, 128)                  # behind a reset it is
    h.pairs_enable(20, 300, 64)
    # tickets outstanding
    tk = h.submit(*_args(b))
    for call in (lambda: h.pairs_enable(20, 300, 64), lambda: h.pairs_enable(n_bins=0), lambda: h.fragments(64), h.fragments_reset):
        with pytest.raises(SharkHipError, match="outstanding"):
            call()
    h.wait(tk)
    same_pairs(h.pairs_last(), pr)
    same_state(h, Fragments(64).add(pr, goff), 64)
    # shk_count_work: records are not handed out and the batch is not counted
    t = _to_device(b)
    p = _dev_ptrs(t)
    h.count_work(50, p["seq1"], p["off1"], p["seq2"], p["off2"])
    with pytest.raises(SharkHipError):
        h.pairs_last()
    same_state(h, Fragments(64).add(pr, goff), 64)
    # pairs mode off: no records, nothing counted; alignments mode off with pairs mode left on: the same
    h.pairs_enable(n_bins=0)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.pairs_last()
    h.pairs_enable(20, 300, 64)
    h.alignments_enable(0)
    h.classify(*_args(b))
    with pytest.raises(SharkHipError):
        h.pairs_last()
    same_state(h, Fragments(64).add(pr, goff), 64)
    with pytest.raises(SharkHipError, match="alignments mode is off"):
        h.pairs_enable(20, 300, 64)


# ---------------------------------------------------------------------------
# (f) inertness
# ---------------------------------------------------------------------------
def test_pairs_mode_is_inert(oracle, panel):
    """every older mode on; pairs mode switched on beside them changes none of their results, byte for byte"""
    from shark_amd import SharkHip
    rng = np.random.default_rng(41)
    records = [g for g, _ in panel]
    batches = [spliced_reads(rng, panel, 300, ragged=False), spliced_reads(rng, panel, 300, ragged=True)]
    seen = []
    for new in (False, True):
        h = SharkHip(k=17, c=0.6, bf_bits=1 << 26)
        h.build([bytes(g) for g in records], keep_bases=True)
        h.evidence_enable(True)
        h.candidates_enable(4)
        h.placement_enable(True)
        h.segments_enable(2)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        h.pileup_enable(8)
        h.alignments_enable(8)
        if new:
            h.pairs_enable()
        rows = []
        for b in batches:
            goff, gids = h.classify(*_args(b))
            keys, segs = h.segments_last()
            cr, ce = h.candidates_last()
            rows.append((goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                         keys.tobytes(), segs.tobytes(), h.alignments_last().tobytes()))
            if new:
                assert (h.pairs_last()["cls"] == 3).any()
        seen.append((rows, h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.depth_summary().tobytes(), h.junctions_get().tobytes(),
                     h.pileup_all().tobytes(), h.pileup_mates(), h.variants().tobytes(), h.variants_summary().tobytes()))
    assert seen[0] == seen[1] and len(seen[0][5]) > 0


# ---------------------------------------------------------------------------
# (g) the command
# ---------------------------------------------------------------------------
def _differ(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    at = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
    return "line %d of %d / %d: got %r, model %r" % (at, len(g), len(w), g[at:at + 1], w[at:at + 1])


@pytest.mark.parametrize("ref", ["example", "twins"])
def test_shark_sam_pairs_and_fragments(oracle, example_dir, tmp_path, ref):
    """--sam --sam-pairs and --fragments against the model, from one worker, from two workers on one device and at two batch sizes, byte
    for byte; without the new flags the SAM file is what it was"""
    from types import SimpleNamespace
    from tests.test_pairs_cpu import example_pairs
    fa = synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))
    if ref == "twins":
        fa = [(fa[0][0], fa[0][1]), (fa[0][0] + b"_twin", fa[0][1])]
    recs, pairs, goff, gids, sam, plain, fasta = example_pairs(oracle, fa)
    header = sam_header(list(fasta), SimpleNamespace(records=dict(enumerate(fasta.values()))), len(fasta))
    want_sam = "".join(ln + "\n" for ln in header + sam).encode("latin-1")
    want_plain = "".join(ln + "\n" for ln in header + plain).encode("latin-1")
    want_frag = Fragments(1024).add(pairs, goff).text().encode()
    assert want_sam != want_plain and (pairs["mapq"] == (3 if ref == "twins" else 60)).all()
    with open(tmp_path / "ref.fa", "wb") as f:
        for name, seq in fa:
            f.write(b">" + name + b"\n" + seq + b"\n")
    base = ["-r", str(tmp_path / "ref.fa"), "-1", os.path.join(example_dir, "sample_1.fq"), "-2", os.path.join(example_dir, "sample_2.fq"),
            "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2")]
    for name, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "700"]), ("c", ["--batch", "333"])):
        r = run_shark(base + ["--sam", str(tmp_path / ("s" + name)), "--sam-pairs", "--fragments", str(tmp_path / ("f" + name))] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = (tmp_path / ("s" + name)).read_bytes()
        assert got == want_sam, _differ(got, want_sam)
        got = (tmp_path / ("f" + name)).read_bytes()
        assert got == want_frag, _differ(got, want_frag)
    # --fragments alone switches alignments mode on by itself; --sam alone writes what it wrote
    r = run_shark(base + ["--fragments", str(tmp_path / "fd"), "--batch", "700"], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert (tmp_path / "fd").read_bytes() == want_frag
    r = run_shark(base + ["--sam", str(tmp_path / "sd")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = (tmp_path / "sd").read_bytes()
    assert got == want_plain, _differ(got, want_plain)
