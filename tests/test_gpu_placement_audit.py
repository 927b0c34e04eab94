"""The placement table ptab / pdir on the device, entry by entry, against a model built from the sequences (tests/placement_audit.py;
DESIGN.md 9).  Each case of the auditor's case table builds with keep_positions, reads back ptab, pdir, pmeta and the depth layout
and must audit clean; it also declares what its reference must contain, and a reference that lost its edge fails the case.  One
end-to-end test holds pl_vote's device code against the same model with reads of exactly k bases.  The auditor itself is tested
without a GPU in tests/test_placement_audit.py.

Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

from tests import placement_audit as pa
from tests import synth

pytestmark = pytest.mark.gpu

NAMES = ("ptab", "pdir", "pmeta")


def _build(recs, k, keep=True):
    from shark_amd import SharkHip
    h = SharkHip(k=k, c=0.6, bf_bits=1 << 26)
    info = h.build([bytes(r) for r in recs], keep_positions=keep)
    return h, info


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in pa.CASES])
def test_placement_table_matches_the_model(c, oracle, example_dir):
    k = c["k"]
    recs = c["ref"](k, example_dir)
    m = pa.TableModel(recs, k)
    assert pa.declared(m, c["needs"]) == []
    if c["check"]:
        c["check"](m, k)
    if not c["small"]:
        assert m.total == pa.MANY_TILES_TOTAL and m.total > 1024 * 4096 and m.lg == 23 and len(recs) == 2000
    h, info = _build(recs, k)
    assert info["nidx"] == m.nidx
    arrays, pmeta, gene_start = pa.pull(h)
    h.close()
    findings = pa.audit(arrays, pmeta, gene_start, m)
    assert findings == [], "\n".join(findings)


def test_case_table_covers_what_the_builder_branches_on():
    ids = {c["id"] for c in pa.CASES}
    for name, ks in (("example", pa.KS), ("collision-interleaved", pa.COLLISION_KS), ("collision-across-genes", pa.ACROSS_KS),("both-strands", pa.KS),
                     ("record-ends", pa.KS), ("short-records", pa.KS), ("only-N", pa.KS), ("only-short", pa.KS), ("only-palindromes", (16,)),
                     ("total-1", pa.KS), ("total-k", pa.KS), ("total-4095", pa.KS), ("total-4096", pa.KS), ("total-4097", pa.KS), ("total-8193", pa.KS),
                     ("repeats", pa.KS), ("lower-and-N", pa.KS), ("many-tiles", (17,))):
        assert {"%s-k%d" % (name, k) for k in ks} <= ids, name
    assert pa.KS == (5, 16, 17, 31) and pa.COLLISION_KS == (9, 17, 31) and pa.ACROSS_KS == (9, 16, 17, 31)
    for need in ("ambiguous", "group", "palindrome", "noid", "empty"):
        assert sum(need in c["needs"] for c in pa.CASES) >= 2, need


# ---------------------------------------------------------------------------
# pl_vote's device code against the model: every window of every record as a single-end read of exactly k bases
# ---------------------------------------------------------------------------
E2E = [c for c in pa.CASES if c["id"].startswith(("collision-", "both-strands-"))]


def k_reads(recs, k):
    """every window of every record: (reads, record of each, offset of each)"""
    reads, src, xs = [], [], []
    for r, rec in enumerate(recs):
        for x in range(len(rec) - k + 1):
            reads.append(rec[x:x + k])
            src.append(r)
            xs.append(x)
    return reads, np.array(src), np.array(xs)


def expected_k_read_placements(m, reads, src, xs, goff, gids):
    """(n_assoc, 3) (strand, pos, support) of reads of exactly k upper-case bases, from the model's table; (associations that voted,
    their reads, their genes)"""
    k = m.k
    codes = np.array([b"ACGT".index(ch) for rd in reads for ch in rd], dtype=np.uint64).reshape(len(reads), k)
    fw, rc = np.zeros(len(reads), np.uint64), np.zeros(len(reads), np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | codes[:, j]
        rc |= (np.uint64(3) - codes[:, j]) << np.uint64(2 * j)
    canon, orient = np.minimum(fw, rc), (fw < rc).astype(np.int64)
    read_of = np.repeat(np.arange(len(reads)), np.diff(np.asarray(goff).astype(np.int64)))
    g = np.asarray(gids).astype(np.int64)
    e = m.entry_of(g, canon[read_of])
    z = np.where(e >= 0, m.z[np.maximum(e, 0)], pa.AMBIGUOUS)                   # (no entry: a palindromic window, or a false positive of the filter)
    voted = z != pa.AMBIGUOUS
    want = np.zeros((len(g), 3), dtype=np.int64)
    want[voted, 0] = (z[voted] >> 31) ^ orient[read_of][voted]
    want[voted, 1] = z[voted] & 0x7FFFFFFF
    want[voted, 2] = 1
    # the same in plain words: in the read's own gene (0, x, 1) for a unique pair, (0, 0, 0) for an ambiguous or palindromic one
    own = g == src[read_of]
    assert int(own.sum()) == len(reads)                                          # every read is assigned to the gene it was cut from
    x_own = xs[read_of][own]
    count_own = np.where(e[own] >= 0, m.count[np.maximum(e[own], 0)], 0)
    assert np.array_equal(want[own], np.where((count_own == 1)[:, None], np.stack([np.zeros_like(x_own), x_own, np.ones_like(x_own)], axis=1), 0))
    return want, voted, read_of, g


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in E2E])
def test_reads_of_k_bases_are_placed_as_the_model_says(c, oracle, example_dir):
    k = c["k"]
    recs = c["ref"](k, example_dir)
    m = pa.TableModel(recs, k)
    assert m.nidx == len(recs) and m.ids_without_record == 0                    # (record r is gene r)
    reads, src, xs = k_reads(recs, k)
    h, _ = _build(recs, k)
    h.placement_enable(True)
    b = synth.batch_from_lists(reads)
    goff, gids = h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"])
    got = h.placement_last()
    h.close()
    assert got.shape == (int(goff[-1]), 2, 3) and not got[:, 1].any()           # single-end: the second mate is empty
    want, voted, read_of, g = expected_k_read_placements(m, reads, src, xs, goff, gids)
    bad = np.flatnonzero((got[:, 0] != want).any(axis=1))
    assert not len(bad), "association %d (read %d, gene %d): got %s, model %s (%d differ)" % (
        bad[0], read_of[bad[0]], g[bad[0]], got[bad[0], 0].tolist(), want[bad[0]].tolist(), len(bad))
    assert int(voted.sum()) > 200 and ("ambiguous" not in c["needs"] or int((~voted).sum()) >= 4)   # (not vacuous: votes and refusals were compared)


# ---------------------------------------------------------------------------
# no table at all: the modes still switch on, a batch returns support 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("only-N", 17), ("only-short", 5), ("only-palindromes", 16)])
def test_modes_over_an_empty_table(name, k, oracle, example_dir):
    c = next(c for c in pa.CASES if c["id"] == "%s-k%d" % (name, k))
    recs = c["ref"](k, example_dir)
    h, _ = _build(recs, k)
    assert int(h.debug_index_array("pmeta")[1]) == 0
    h.placement_enable(True)
    h.segments_enable(2)
    h.depth_enable_spliced(1)
    h.junctions_enable(1, 1024)
    h.pileup_enable(1)
    rng = np.random.default_rng(3)
    reads = [b"AT" * 20, b"CG" * 16, b"N" * 40, bytes(synth.random_seq(rng, 60)), bytes(synth.random_seq(rng, k)), b"A"]
    b = synth.batch_from_lists(reads, [bytes(synth.revcomp(np.frombuffer(r, np.uint8))) for r in reads])
    goff, gids = h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"])
    got = h.placement_last()
    keys, segs = h.segments_last()
    assert got.shape == (int(goff[-1]), 2, 3) and not got.any() and not keys.any() and not segs.any()
    assert h.depth_mates() == 0 and h.pileup_mates() == 0 and len(h.junctions_get()) == 0
    if name == "only-palindromes":
        assert int(goff[-1]) >= 2                                                # ((AT)n and (CG)n are assigned: their windows are in the filter)
    else:
        assert int(goff[-1]) == 0
    h.close()


# ---------------------------------------------------------------------------
# the builder's promise, and the names on an index without the table
# ---------------------------------------------------------------------------
def test_two_builds_give_the_same_bytes(oracle, example_dir):
    for cid in ("repeats-k17", "collision-interleaved-k17", "repeats-k5"):
        c = next(c for c in pa.CASES if c["id"] == cid)
        recs = c["ref"](c["k"], example_dir)
        seen = []
        for _ in range(2):
            h, _info = _build(recs, c["k"])
            arrays, pmeta, _gs = pa.pull(h)
            h.close()
            n = pmeta["ptab_n"]
            assert n > 0 and len(arrays["ptab"]) == 4 * (n + 1)
            seen.append((pmeta, arrays["ptab"][:4 * n].tobytes(), arrays["pdir"].tobytes()))   # (the spare entry behind ptab_n is never written)
        assert seen[0] == seen[1], cid


def test_names_have_size_zero_without_keep_positions(oracle):
    rng = np.random.default_rng(7)
    h, _ = _build(synth.make_genes(rng, 5, 300, 500), 17, keep=False)
    for name in NAMES:
        assert len(h.debug_index_array(name)) == 0, name
    assert len(h.debug_index_array("rank_w")) > 0 and len(h.debug_index_meta()) == 16         # (`meta` is what it was)
    h.close()
    h, _ = _build(synth.make_genes(rng, 5, 300, 500), 17, keep=True)
    sizes = [len(h.debug_index_array(name)) for name in NAMES]
    lg, n = (int(v) for v in h.debug_index_array("pmeta"))
    assert sizes == [4 * (n + 1), (1 << lg) + 2, 2] and n > 0
    h.close()
