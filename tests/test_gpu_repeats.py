"""GPU parity on repeat-rich references and long gene lists (tests/repeat_refs.py): paralog families, an element interspersed in
50 / 1 000 genes, low-complexity runs around k and around the anchored extension's 254 clip, tandem copies, a k-mer-saturated
neighbourhood of one minimiser, and one motif shared by 65 534 / 65 535 / 65 536 / 70 000 records -- gene lists at and beyond the
0xFFFF length sentinel of ListEntry, ties of 65 536 genes, wrapped ids with a multiplicity of 69 984.  Bit-exact against the CPU
oracle, through shk_classify and the device-resident entry point; every test asserts that its input reached what it is for.

Run on the GPU box with `pytest -m gpu`."""
import re

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both
    import torch
except Exception:  # pragma: no cover
    torch = None

from tests import repeat_refs as rr
from tests import synth
from tests.gpu_fixtures import probe  # noqa: F401
from tests.test_gpu_parity import _build_both, _compare_classify, _compare_index, _probe_every_kmer

pytestmark = pytest.mark.gpu

INLINE = 4          # SHK_INLINE_IDS (include/shark_hip.h)
CHAIN_ENV = ("SHK_PROBE", "SHK_NO_LDS_TABLE", "SHK_FORCE_GENERIC", "SHK_KTAB", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_TILE_FIRST",
             "SHK_ANCHOR_ALWAYS", "SHK_NO_ANCHOR", "SHK_NO_PRE_VERDICT", "SHK_NO_REFEXT", "SHK_KTAB_LOAD", "SHK_KTAB_STATS")


def _clean_env(monkeypatch, **env):
    for v in CHAIN_ENV:
        monkeypatch.delenv(v, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def _device(h, b, bound):
    """the batch resident in HBM through shk_classify_device -> (gene_off, gene_ids) on the host"""
    from shark_amd.capi import hip_memcpy_dtoh
    dev = torch.device("cuda:0")
    t = {kk: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for kk, v in b.items() if v is not None}
    pt = {kk: (t[kk].data_ptr() if kk in t else 0) for kk in b}
    n = len(b["off1"]) - 1
    torch.cuda.synchronize()
    r = h.classify_device(n, pt["seq1"], pt["off1"], pt["seq2"], pt["off2"], pt["qual1"], pt["qual2"], max_read_len=bound)
    goff = np.empty(n + 1, np.uint32)
    hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    gids = np.empty(int(r.n_assoc), np.uint16)
    if len(gids):
        hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    return goff, gids


def _max_len(b):
    return max([1] + [int(np.diff(b[o].astype(np.int64)).max()) for o in ("off1", "off2") if b[o] is not None and len(b[o]) > 1])


def _both_entries(o, h, b, want=None):
    """shk_classify and shk_classify_device (true bound, and 0 = unknown) against the oracle -> the oracle's (gene_off, gene_ids)"""
    if want is None:
        want = _compare_classify(o, h, b, nthreads=8)
    else:
        hg, hi = h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"])
        assert np.array_equal(want[0], hg), "gene_off differs at read %d" % int(np.argmax(want[0] != hg))
        assert np.array_equal(want[1], hi)
    tags = h.last_kernel()
    for bound in (_max_len(b), 0):
        dg, di = _device(h, b, bound)
        assert np.array_equal(want[0], dg), "classify_device(bound %d): gene_off differs at read %d" % (bound, int(np.argmax(want[0] != dg)))
        assert np.array_equal(want[1], di), bound
    return want[0], want[1], tags


def _counts(goff):
    return np.diff(goff.astype(np.int64))


# ---------------------------------------------------------------------------
# paralog families
# ---------------------------------------------------------------------------
def _family_reference(rng, big):
    fam = rr.families(rng, 3, 8, 1200, 0.97)
    return rr.compose(fam, rr.plain(rng, 20, 5500, 6500) if big else rr.plain(rng, 20, 400, 1100))


def _family_batches(rng, genes, marks, q):
    """2 x 150 uniform, 2 x 100 ragged, 1 x 76: pairs from every paralog (so the runner-up is a few bases behind), the exact duplicate
    and the reverse-complemented member, the random genes and from nowhere; substitutions, N, lower case, qualities on top"""
    out = []
    for L, ragged, paired in ((150, False, True), (100, True, True), (76, False, False)):
        pairs = []
        for m in marks:
            g = genes[m["gene"]]
            for s in rng.integers(0, len(g) - L - 60, 5):
                pairs.append(rr._pair(g, int(s), L, 60, bool(s & 1)))
        if len(genes) > len(marks):
            pairs += [rr._pair(genes[int(g)], int(rng.integers(0, len(genes[int(g)]) - L - 60)), L, 60, False) for g in rng.integers(len(marks), len(genes), 30)]
        pairs += [(synth.random_seq(rng, L), synth.random_seq(rng, L)) for _ in range(30)]
        pairs = rr.dress(rng, rr.pad_uniform(pairs, L, rng), 0.01, 0.002, 0.1)
        out.append(rr.batch(pairs, paired=paired, ragged_rng=rng if ragged else None, qual_rng=rng if q else None))
    return out


# the sides of the anchored extension's switches: what is set when the index is built / the batch launched
HOWS = {"pre": None, "off": "SHK_NO_PRE_VERDICT", "none": "SHK_NO_REFEXT", "noanchor": "SHK_NO_ANCHOR"}


def _check_anchor_tags(how, tags):
    """what shk_last_kernel must say on a table chain with SHK_ANCHOR_ALWAYS=1 under each side of the switches -> 1 (a check made)"""
    assert ("+pre-verdict" in tags) == (how == "pre"), (how, tags)
    assert ("+anchored-extension" in tags) == (how != "noanchor"), (how, tags)
    return 1


FAMILY_CHAINS = [("lds-summary+table", {}, 1 << 26, False),
                 ("table", {"SHK_NO_LDS_SUMMARY": "1", "SHK_NO_SUMMARY": "1"}, 1 << 26, False),
                 ("summary+table", {"SHK_NO_LDS_SUMMARY": "1"}, 1 << 28, True),
                 ("table-mod", {"SHK_NO_LDS_SUMMARY": "1"}, 3 << 24, False)]


@pytest.mark.parametrize("k", [17, 31])
@pytest.mark.parametrize("mode,env,bf_bits,big", FAMILY_CHAINS, ids=[c[0] for c in FAMILY_CHAINS])
def test_families(oracle, monkeypatch, mode, env, bf_bits, big, k):
    """3 families x 8 paralogs at 97 % identity (+ an exact duplicate, a reverse-complemented member, 20 random genes): the lead of the
    best gene over the runner-up is a few bases, ties where two paralogs agree under a read.  Every probe chain that an index takes by
    itself (asserted); with the anchored extension forced on: the verdict kernel in front (asserted by its tag), without it
    (SHK_NO_PRE_VERDICT), on an index without the extension's arrays (SHK_NO_REFEXT) and on one without the anchor table
    (SHK_NO_ANCHOR).  Of the product c in {0.3, 0.6, 0.9} x --single x -q {0, 20} a SELECTION of seven runs with the kernel in front --
    every value of each axis, each pair of c with --single or -q at least once in one direction -- and the other sides at
    (0.6, off, 0): every combination is an index build of its own on both sides."""
    rng = np.random.default_rng(7000 + k + (1 if big else 0))
    genes, marks = _family_reference(rng, big)
    seen_ties = 0
    checked = dict.fromkeys(HOWS, 0)
    for how in HOWS:
        _clean_env(monkeypatch, SHK_ANCHOR_ALWAYS="1", **env)
        if HOWS[how]:
            monkeypatch.setenv(HOWS[how], "1")
        for c, single, q in ((0.6, False, 0), (0.3, False, 0), (0.9, False, 0), (0.3, True, 0), (0.6, True, 20), (0.9, False, 20), (0.6, False, 20)):
            if how != "pre" and (c, single, q) != (0.6, False, 0):
                continue
            o, h, info = _build_both(oracle, genes, k=k, bf_bits=bf_bits, c=c, min_quality=q, single=single)
            assert h.probe_mode() == mode, h.probe_mode()
            for b in _family_batches(rng, genes, marks, q):
                goff, gids, tags = _both_entries(o, h, b)
                seen_ties += int((_counts(goff) > 1).sum())
                if "classify_uni_kernel" in tags and "SHK_NO_LDS_SUMMARY" in env:
                    checked[how] += _check_anchor_tags(how, tags)
            h.close()
            o.close()
    # (behind the LDS summary neither the extension nor the verdict kernel applies: nothing to check on that chain)
    assert "SHK_NO_LDS_SUMMARY" not in env or all(n >= 3 for n in checked.values()), checked
    assert seen_ties > 25, "paralogs, the duplicate and the reverse complement must tie under some reads"


@pytest.mark.parametrize("tile_first", ["0", "1"])
def test_one_family_in_lds(oracle, monkeypatch, tile_first):
    """one family small enough for the exact table in LDS (<= 26 000 set bits): near-ties through the sparse first rounds and the
    three-pairs kernel (asserted), under either setting of SHK_TILE_FIRST"""
    _clean_env(monkeypatch, SHK_TILE_FIRST=tile_first)
    rng = np.random.default_rng(7100)
    genes, marks = rr.families(rng, 1, 8, 1200, 0.97)
    for c, single in ((0.6, False), (0.3, True), (0.9, False)):
        o, h, info = _build_both(oracle, genes, k=17, bf_bits=1 << 30, c=c, single=single)
        assert info["n_set_bits"] <= 26000 and h.probe_mode() == "lds-table", (info["n_set_bits"], h.probe_mode())
        uni, rag, se = _family_batches(rng, genes, marks, 0)
        goff, _, tags = _both_entries(o, h, uni)
        assert "+three-pairs" in tags and "+sparse-first-rounds" in tags, tags      # (the tiles' round is for one-gene indices: the switch must change nothing here)
        assert (_counts(goff) > 1).sum() > 10 or single
        _both_entries(o, h, rag)
        _both_entries(o, h, se)
        h.close()
        o.close()


# ---------------------------------------------------------------------------
# an element interspersed in many genes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("carriers", [50, 1000])
def test_interspersed_element(oracle, probe, carriers):
    """a 200-base element in `carriers` genes, either strand, three fifths of the copies exact: reads swept across both of its
    boundaries, reads wholly inside it (a tie of every carrier of the conserved core at low c, nothing under --single), tens of
    thousands of ids through the tie queue and the EMIT pass; the per-gene counters are the histogram of what came back"""
    rng = np.random.default_rng(7200 + carriers)
    base, _ = rr.plain(rng, 20, 300, 800)
    genes, marks = rr.interspersed(rng, base, 200, carriers, 0.15)
    L = 100
    pairs = []
    for m in (marks[0], marks[1], marks[carriers // 2], marks[-1]):       # exact copies and diverged ones, whichever strand they got
        pairs += rr.sweep(genes, m["gene"], m["start"], L) + rr.sweep(genes, m["gene"], m["end"], L)
        pairs += rr.inside(genes, m["gene"], m["start"], m["end"], L, step=2)
    pairs += rr.pure(L) + rr.polya_tail(rng, L) + [(synth.random_seq(rng, L), synth.random_seq(rng, L)) for _ in range(40)]
    n_inside = 4 * 51
    uni = rr.batch(rr.pad_uniform(pairs, L, rng))
    rag = rr.batch(rr.dress(rng, pairs, 0.005, 0.002, 0.1), ragged_rng=rng)
    for c, single in ((0.3, False), (0.6, False), (0.3, True)):
        o, h, info = _build_both(oracle, genes, k=17, bf_bits=1 << 28, c=c, single=single)
        off, _ = h.copy_lists()
        assert np.diff(off.astype(np.int64)).max() >= sum(m["rate"] == 0.0 for m in marks) >= carriers // 2
        for b in (uni, rag):
            h.gene_counts_reset()
            goff, gids, _ = _both_entries(o, h, b)
            cnt = _counts(goff)
            if single:
                assert cnt.max() <= 1
            elif b is uni:
                assert cnt.max() >= carriers // 2, cnt.max()
                assert (cnt >= carriers // 2).sum() >= n_inside // 2
                assert h.timing()["last_n_tie"] > 0
            # three calls (host, device with a bound, device without): each counted once
            assert np.array_equal(h.gene_counts(1024), 3 * np.bincount(gids, minlength=1024)[:1024].astype(np.uint64))
        h.close()
        o.close()


# ---------------------------------------------------------------------------
# low complexity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 16, 17, 21, 31])
def test_low_complexity(oracle, probe, k):
    """homopolymer runs of k - 1 ... 1 000 bases, their complement, period-2 / 3 / (k - 1) repeats, runs cut by N and in lower case, at
    a record's ends, a record that is one run: reads swept over both ends of every run (uniform and trimmed batches), pure
    low-complexity reads, poly-A tails; and every reference k-mer as a read of its own -- where a lost or duplicated key shows"""
    rng = np.random.default_rng(7300 + k)
    genes, marks = rr.compose(rr.low_complexity(rng, [], k), rr.plain(rng, 6, 300, 800))
    L = 100
    pairs = rr.boundary_sweeps(genes, marks, L) + rr.pure(L) + rr.pure(60) + rr.polya_tail(rng, L)
    uni = rr.batch(rr.pad_uniform(pairs, L, rng))
    rag = rr.batch(rr.dress(rng, pairs[::3], 0.003, 0.002, 0.1), ragged_rng=rng, qual_rng=rng)      # (every third offset: the sweep itself is the uniform batch)
    o, h, info = _build_both(oracle, genes, k=k, bf_bits=1 << 26, c=0.5, min_quality=0)
    _compare_index(o, h, info)
    goff, _, _ = _both_entries(o, h, uni)
    assert (_counts(goff) >= 2).sum() > 30            # the poly-A / poly-T k-mer is in 11 records: reads that are mostly run tie
    og, n = _probe_every_kmer(o, h, genes, k, stride=1)
    assert int(og[-1]) >= n - 40                      # (every k-mer without N finds itself)
    h.close()
    o.close()
    o, h, info = _build_both(oracle, genes, k=k, bf_bits=1 << 26, c=0.3, min_quality=20)
    _both_entries(o, h, rag)
    h.close()
    o.close()


@pytest.mark.parametrize("L", [150, 300])
@pytest.mark.parametrize("env", [{"SHK_NO_LDS_SUMMARY": "1"}, {"SHK_NO_LDS_SUMMARY": "1", "SHK_NO_SUMMARY": "1"}], ids=["summary", "plain"])
def test_runs_beyond_the_extension_clip(oracle, monkeypatch, env, L):
    """runs of 253 ... 1 000 equal k-mers behind anchor_verdict_kernel and the anchored extension: `atab` keeps ONE occurrence of the
    run's k-mer and `refext` clips its extent at 254, so a read inside a longer run is anchored somewhere else in it than where it
    came from.  2 x 150 and 2 x 300, uniform and trimmed, swept over both ends of each run and stepping through it; with the kernel
    in front (asserted), without it, without the extension's arrays and without the anchor table (each side asserted by its tags)."""
    rng = np.random.default_rng(7400 + L)
    genes, marks = rr.compose(rr.low_complexity(rng, [], 17), rr.plain(rng, 12, 900, 2500))
    longs = [m for m in marks if m["kind"].startswith("homopolymer") and m["n"] >= 253]
    assert sorted(m["n"] for m in longs) == [253, 254, 255, 256, 300, 300, 1000]
    pairs = rr.boundary_sweeps(genes, longs, L, step=3)
    for m in longs:
        pairs += rr.inside(genes, m["gene"], max(0, m["start"] - 40), min(len(genes[m["gene"]]), m["end"] + 40), L, step=5)
    pairs += [rr._pair(genes[int(g)], int(rng.integers(0, 600)), L, 50, False) for g in rng.integers(len(genes) - 12, len(genes), 100)]
    uni = rr.batch(rr.pad_uniform(pairs, L, rng))
    rag = rr.batch(rr.dress(rng, pairs, 0.004, 0.001, 0.0), ragged_rng=rng)
    checked = dict.fromkeys(HOWS, 0)
    for how in HOWS:
        _clean_env(monkeypatch, SHK_ANCHOR_ALWAYS="1", **env)
        if HOWS[how]:
            monkeypatch.setenv(HOWS[how], "1")
        for c in (0.6, 0.2) if how == "pre" else (0.6,):
            o, h, info = _build_both(oracle, genes, k=17, bf_bits=1 << 26, c=c)
            assert h.probe_mode() in ("table", "summary+table"), h.probe_mode()
            for b in (uni, rag):
                goff, _, tags = _both_entries(o, h, b)
                assert goff[-1] > len(pairs) // 2
                if "classify_uni_kernel" in tags:
                    checked[how] += _check_anchor_tags(how, tags)
            h.close()
            o.close()
    assert all(n >= 2 for n in checked.values()), checked


def test_pure_poly_a_reads_against_many_poly_a_genes(oracle, probe):
    """A x L and T x L reads against a reference with an A or T run in 320 genes (one canonical k-mer, one list of 320), and against one
    without any"""
    rng = np.random.default_rng(7500)
    with_runs, _ = rr.poly_a_carriers(rng, 320)
    without, _ = rr.plain(rng, 40, 150, 400)
    pairs = []
    for L in (17, 40, 100, 150):
        pairs += rr.pure(L)
    pairs += rr.polya_tail(rng, 100) + [(synth.random_seq(rng, 100), synth.random_seq(rng, 100)) for _ in range(50)]
    pairs = [pairs[i % len(pairs)] for i in range(3 * len(pairs))]
    b = rr.batch(pairs)
    for genes, expect in ((with_runs, 320), (without, 0)):
        for c, single in ((0.0, False), (0.6, False), (0.6, True)):
            o, h, info = _build_both(oracle, genes, k=17, bf_bits=1 << 26, c=c, single=single)
            goff, _, _ = _both_entries(o, h, b)
            if not single:
                # (without such runs: nothing but what a random k-mer hits by chance at c = 0)
                assert (_counts(goff).max() == 320) if expect else (_counts(goff).max() <= INLINE), _counts(goff).max()
                assert (h.timing()["last_n_tie"] > 0) == (expect > 0)
            h.close()
            o.close()


# ---------------------------------------------------------------------------
# tandem copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("unit_len,copies,drift", [(40, 30, False), (150, 12, True), (400, 2, False), (97, 8, True), (64, 20, True)])
@pytest.mark.parametrize("chain", ["probe-auto", "probe-bitvector", "probe-no-lds-table", "probe-force-generic", "probe-ktable", "anchored"])
def test_tandem_copies(oracle, monkeypatch, chain, unit_len, copies, drift):
    """a unit 2 ... 30 times in one gene, exact and drifting by one substitution per copy: reads from each copy, reads spanning copies
    j / j + 1, reads spanning the last copy and the unique tail.  Under every probe variant, and ("anchored") on the position table with
    the anchored extension and the verdict kernel forced on and asserted: the anchor table keeps ONE occurrence per k-mer, so the anchor
    of a read from copy j names another copy, one base per unit away from the read in the drifted variant."""
    _clean_env(monkeypatch, **{"probe-auto": {}, "probe-bitvector": {"SHK_PROBE": "bitvector"}, "probe-no-lds-table": {"SHK_NO_LDS_TABLE": "1"},
                               "probe-force-generic": {"SHK_FORCE_GENERIC": "1"},
                               "probe-ktable": {"SHK_KTAB": "1", "SHK_NO_LDS_SUMMARY": "1", "SHK_NO_SUMMARY": "1"},
                               "anchored": {"SHK_NO_LDS_SUMMARY": "1", "SHK_ANCHOR_ALWAYS": "1"}}[chain])
    rng = np.random.default_rng(7600 + unit_len)
    tg, marks = rr.tandem(rng, unit_len, copies, drift)
    genes, marks = rr.compose((tg, marks), rr.plain(rng, 10, 400, 1500))
    assert len({bytes(genes[0][m["start"]:m["end"]]) for m in marks}) == (copies if drift else 1)
    for L in (100, 150):
        pairs = []
        for m in marks:
            pairs += rr.inside(genes, 0, m["start"], max(m["end"], min(m["start"] + L, marks[-1]["end"])), L, step=max(1, unit_len // 4))
            pairs += rr.sweep(genes, 0, m["end"], L, step=4)                   # across copy j / j + 1; the last one: across the tail
        pairs += rr.sweep(genes, 0, marks[0]["start"], L, step=2)
        pairs += [(synth.random_seq(rng, L), synth.random_seq(rng, L)) for _ in range(30)]
        o, h, info = _build_both(oracle, genes, k=17, bf_bits=1 << 26, c=0.6)
        goff, _, tags = _both_entries(o, h, rr.batch(rr.pad_uniform(pairs, L, rng)))
        assert (goff[1:] > goff[:-1]).sum() > len(pairs) // 2
        if chain == "anchored":
            assert h.probe_mode() in ("table", "summary+table") and "classify_uni_kernel" in tags, (h.probe_mode(), tags)
            _check_anchor_tags("pre", tags)
        _both_entries(o, h, rr.batch(rr.dress(rng, pairs[::2], 0.01, 0.002, 0.1), ragged_rng=rng))
        h.close()
        o.close()


# ---------------------------------------------------------------------------
# the minimiser-bucketed table with one overfull line
# ---------------------------------------------------------------------------
_STATS = re.compile(r"\[shk/ktab\] k=17 w=15 .* displaced=(\d+) .* longest path=(\d+) no place=(\d+) lost=(\d+)")


@pytest.mark.parametrize("bf_bits,load", [(1 << 30, None), (1 << 24, "50")])
def test_saturated_neighbourhood(oracle, monkeypatch, capfd, bf_bits, load):
    """all 48 k-mers around the 15-mer with the smallest hash share their minimiser, hence one 16-slot line of the minimiser-bucketed
    table: the build must displace (asserted from its SHK_KTAB_STATS line) and either keep the table or drop it -- parity with the
    oracle in both outcomes, on whole reads, on each k-mer of the neighbourhood, on every reference k-mer and on 10^5 random k-mers
    (on the 2^24-bit filter a quarter per cent of those are false positives, each a key of the table).  Observed on the
    MI355X (the table was kept both times; `pytest -s` prints the line):
      2^30-bit filter:                    lines=2^18 keys=245215 load=0.058 displaced=918 (0.37 %) longest path=4 no place=0 lost=0
      2^24-bit filter, SHK_KTAB_LOAD=50:  lines=2^21 keys=13935194 load=0.415 displaced=1185389 (8.51 %) longest path=17 no place=0 lost=0"""
    _clean_env(monkeypatch, SHK_KTAB="1", SHK_NO_LDS_SUMMARY="1", SHK_NO_SUMMARY="1", SHK_KTAB_STATS="1")
    if load:
        monkeypatch.setenv("SHK_KTAB_LOAD", load)
    rng = np.random.default_rng(7700)
    genes, marks = rr.compose(rr.saturated_neighbourhood(rng, 17, 15), rr.plain(rng, 30, 300, 1500))
    capfd.readouterr()
    o, h, info = _build_both(oracle, genes, k=17, bf_bits=bf_bits, c=0.0)
    err = capfd.readouterr().err
    m = _STATS.search(err)
    assert m, err
    print(m.group(0))
    displaced, longest, no_place, lost = (int(x) for x in m.groups())
    assert displaced > 0 and longest > 0
    assert h.probe_mode() == ("minimiser-table" if no_place == 0 and lost == 0 else "table")
    _compare_index(o, h, info)
    hood = [genes[x["gene"]][x["start"]:x["end"]] for x in marks if x["kind"] == "neighbour"]
    assert len(hood) == 48
    goff, _, _ = _both_entries(o, h, synth.batch_from_lists([bytes(x) for x in hood] + [bytes(synth.revcomp(x)) for x in hood]))
    assert (_counts(goff) >= 1).all()
    og, n = _probe_every_kmer(o, h, genes, 17, stride=1)
    assert int(og[-1]) >= n
    rnd = synth.ACGT[rng.integers(0, 4, size=(100_000, 17))]
    goff, _, tags = _both_entries(o, h, synth.batch_from_lists([bytes(x) for x in rnd]))
    if h.probe_mode() == "minimiser-table":
        assert ", 8, " in tags, tags
    if bf_bits == 1 << 24:
        assert (_counts(goff) > 0).sum() > 50, "false positives of the dense filter"
    pairs = rr.boundary_sweeps(genes, marks[::6], 100, step=5) + [(synth.random_seq(rng, 100), synth.random_seq(rng, 100)) for _ in range(200)]
    _both_entries(o, h, rr.batch(rr.pad_uniform(pairs, 100, rng)))
    _both_entries(o, h, rr.batch(pairs, ragged_rng=rng))
    h.close()
    o.close()


# ---------------------------------------------------------------------------
# batch-to-batch state
# ---------------------------------------------------------------------------
def test_repeat_rich_and_random_batches_alternate(oracle, monkeypatch):
    """one context, batches from an element's carriers / paralogs and batches of random reads in turn: the assigned fraction swings across
    the 15 % switch, the verdict kernel comes and goes (asserted) and every batch equals the oracle"""
    _clean_env(monkeypatch, SHK_NO_LDS_SUMMARY="1")
    rng = np.random.default_rng(7800)
    genes, marks = rr.compose(rr.families(rng, 2, 6, 1000, 0.97), rr.interspersed(rng, rr.plain(rng, 10, 400, 900)[0], 200, 60, 0.1))
    L = 150
    rich = []
    for m in marks[:14] + marks[14::6]:
        rich += rr.sweep(genes, m["gene"], m["start"], L, step=3) + rr.sweep(genes, m["gene"], m["end"], L, step=3)
    rich = rr.batch(rr.pad_uniform(rich, L, rng))
    n = len(rich["off1"]) - 1
    rand = rr.batch([(synth.random_seq(rng, L), synth.random_seq(rng, L)) for _ in range(n)])
    o, h, info = _build_both(oracle, genes, k=17, bf_bits=1 << 26, c=0.4)
    assert h.probe_mode() in ("table", "summary+table"), h.probe_mode()
    want = {id(b): o.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], nthreads=8) for b in (rich, rand)}
    seen = []
    for b in (rich, rand, rand, rich, rich, rand, rich, rand, rand, rich):
        wg, wi = want[id(b)]
        hg, hi = h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"])
        assert np.array_equal(wg, hg) and np.array_equal(wi, hi), len(seen)
        seen.append((float((wg[1:] > wg[:-1]).mean()), "+pre-verdict" in h.last_kernel()))
    assert max(f for f, _ in seen) > 0.5 and min(f for f, _ in seen) < 0.05
    assert seen[0][1]
    for (frac_before, _), (_, with_pre) in zip(seen, seen[1:]):
        assert with_pre == (frac_before >= 0.15), seen
    h.close()
    o.close()


# ---------------------------------------------------------------------------
# long gene lists: the 0xFFFF clip of ListEntry.len, ties of 65 536 genes, wrapped ids with multiplicity
# ---------------------------------------------------------------------------
LONG_SIZES = [65534, 65535, 65536, 70000]
MOTIF_AT = (0, 5, 31, 40, 62, 63, 64, 65, 66, 70, 90, 100, 110, 120, 125, 126, 127, 128, 129, 133)    # around the 64-read block boundaries
N_LONG_READS = 136
_long_cache = {}


def _long_reference(n_genes):
    """shared_motif(n_genes): 30 random bases, a 40-base motif, 30 random bases per record; 70 000: record 69 000 is A x 70 000 + 50
    random bases -- a wrapped gene (id 3464) that holds one k-mer 69 984 times"""
    if n_genes not in _long_cache:
        rng = np.random.default_rng(n_genes)
        genes, marks = rr.shared_motif(rng, n_genes)
        if n_genes == 70000:
            genes[69000] = np.concatenate([rr._unit_run("A", 70000), rr._seq("C"), synth.random_seq(rng, 49)])
        motif = genes[0][30:70].copy()
        m1, own = [], {}
        for i in range(N_LONG_READS):
            if i in MOTIF_AT:
                m1.append(motif)
            elif i % 9 == 1:
                own[i] = (i * 7919) % n_genes
                m1.append(genes[own[i]][:80])                             # flank + motif + flank of one gene
            elif i % 9 == 2:
                m1.append(rr._unit_run("A", 60))
            elif i % 9 == 3:
                own[i] = n_genes - 1 - i
                m1.append(genes[own[i]][10:90])
            elif i == 58:
                m1.append(np.zeros(0, np.uint8))
            elif i == 59 and n_genes == 70000:
                m1.append(np.concatenate([genes[69000][-50:], rr._unit_run("A", 30)]))   # the poly-A gene's unique tail + 30 A
            else:
                m1.append(synth.random_seq(rng, 80))
        m2 = [synth.revcomp(a) if i % 2 == 0 else np.zeros(0, np.uint8) for i, a in enumerate(m1)]
        _long_cache[n_genes] = (genes, motif, synth.batch_from_lists([bytes(a) for a in m1], [bytes(a) for a in m2]), {}, own)
    return _long_cache[n_genes]


def _long_oracle(oracle, n_genes, c, single):
    """the oracle's answer for the batch of _long_reference, computed once per (size, c, --single)"""
    genes, motif, b, memo, _ = _long_reference(n_genes)
    if (c, single) not in memo:
        o = oracle.Shark(k=17, c=c, bf_bits=1 << 30, single=single)
        o.build([bytes(g) for g in genes], nthreads=8)
        memo[(c, single)] = o.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], nthreads=16)
        o.close()
    return memo[(c, single)]


@pytest.mark.parametrize("n_genes", LONG_SIZES)
def test_long_list_index(oracle, n_genes):
    """the index itself: filter words, offsets and ids equal the oracle's in full (wrap mode: every list as a multiset, the device sorts
    by id), and the longest list is what the reference was built for -- n_genes entries, at and beyond 0xFFFF"""
    genes, motif, b, _, own = _long_reference(n_genes)
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 30)
    nidx = o.build([bytes(g) for g in genes], nthreads=8)
    from shark_amd import SharkHip
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 30)
    info = h.build([bytes(g) for g in genes])
    assert info["nidx"] == nidx == n_genes
    off, ids = h.copy_lists()
    lens = np.diff(off.astype(np.int64))
    if n_genes <= 65536:
        _compare_index(o, h, info)
        assert lens.max() == n_genes and (lens == n_genes).sum() == 40 - 17 + 1
        assert (lens.max() >= 0xFFFF) == (n_genes >= 65535)
    else:
        oi = o.index_kmer()
        assert info["n_set_bits"] == o.num_kmer() and info["tot_idx"] == len(oi) == len(ids)
        assert np.array_equal(o.bf_words(), h.copy_bf())
        cut = off.astype(np.int64)[1:-1]
        for x, y in zip(np.split(ids, cut), np.split(oi, cut)):
            if len(x) > 1:
                assert np.array_equal(x, np.sort(y))
        # the motif's lists: one entry per record that has the motif (69 999: ids 0 ... 4463 twice but for 3464); the poly-A k-mer: one id 69 984 times
        assert (lens == n_genes - 1).sum() == 24 and lens.max() == n_genes - 1
        pa = np.flatnonzero(lens == 70000 - 17 + 1)
        assert len(pa) == 1
        assert set(ids[off[pa[0]]:off[pa[0] + 1]].tolist()) == {69000 & 0xFFFF}
    h.close()
    o.close()


@pytest.mark.parametrize("n_genes", LONG_SIZES)
def test_long_list_classify(oracle, probe, n_genes):
    """one batch in which twenty 65 53x-way ties sit between ordinary reads and on both sides of the 64-read block boundaries, c = 0 and
    0.6, --single on and off, host and device-resident.  Without wrap the ids of a motif read are 0 ... n_genes - 1 ascending, which
    follows from ReadAnalyzer.hpp:90-108 alone (every gene has the same coverage and k-mer count) and is asserted without the oracle;
    with 70 000 genes the 4 463 ids that two motif records share count twice and win."""
    genes, motif, b, _, own = _long_reference(n_genes)
    # (each combination is an index of 65 53x records on both sides: the full product at 65 536, where the clip bites; its two
    #  opposite corners at the other sizes)
    for c, single in ((0.0, False), (0.6, True), (0.6, False), (0.0, True))[:4 if n_genes == 65536 else 2]:
        want = _long_oracle(oracle, n_genes, c, single)
        from shark_amd import SharkHip
        h = SharkHip(k=17, c=c, bf_bits=1 << 30, single=single)
        h.build([bytes(g) for g in genes])
        goff, gids, tags = _both_entries(None, h, b, want=want)
        cnt = _counts(goff)
        width = n_genes if n_genes <= 65536 else 4463          # (ids 0 ... 4463 are two records each; record 69 000 of them is the poly-A one)
        for i in MOTIF_AT:
            if single:
                assert cnt[i] == 0
            else:
                assert cnt[i] == width
                if n_genes <= 65536:
                    assert np.array_equal(gids[goff[i]:goff[i + 1]], np.arange(n_genes, dtype=np.uint16))
        assert len(own) >= 20
        for i, g in own.items():                                        # one gene's flank + motif + flank: that gene alone, under its (wrapped) id
            assert cnt[i] == 1 and int(gids[goff[i]]) == g & 0xFFFF, (i, g)
        rest = np.array(sorted(own))
        if not single:
            assert int(h.timing()["last_n_tie"]) == len(MOTIF_AT) and (cnt > INLINE).sum() == len(MOTIF_AT)
        else:
            want_m = _long_oracle(oracle, n_genes, 0.0, False)
            assert np.array_equal(_counts(want_m[0])[rest], cnt[rest])   # --single: the motif reads return nothing, the rest is unchanged
        # the kernel whose merge read the long lists: the variant's own (the ties' ids are then written by the general kernel's EMIT pass)
        if n_genes > 65536:
            assert "classify_general_kernel<wrap>" in tags, tags
        elif probe in ("bitvector", "force-generic"):
            assert "classify_fast_kernel" in tags, tags
        else:
            assert "classify_uni_kernel" in tags, tags
        h.close()


def test_long_list_result_outgrows_its_reserve(oracle):
    """twenty ties of 65 536: 1.3 million associations against a reserve of 2 n + 4096 -- the grow-and-redo path, then the same batch
    again on the buffers it left (the fast path); the per-gene counters count every association once, both times.  That the first call
    regrows and the second does not is inferred from the sizes (asserted below: the result is more than 100 reserves); the library
    exposes no counter of regrows."""
    genes, motif, b, _, own = _long_reference(65536)
    want = _long_oracle(oracle, 65536, 0.0, False)
    from shark_amd import SharkHip
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 30)
    h.build([bytes(g) for g in genes])
    assert int(want[0][-1]) > 20 * 65536 > 100 * (2 * N_LONG_READS + 4096)
    hist = np.bincount(want[1], minlength=65536).astype(np.uint64)
    h.gene_counts_reset()
    for rep in (1, 2):
        hg, hi = h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"])
        assert np.array_equal(want[0], hg) and np.array_equal(want[1], hi), rep
        assert "classify_uni_kernel" in h.last_kernel(), h.last_kernel()      # (the default chain: the position-table kernel's merge)
        assert np.array_equal(h.gene_counts(65536), rep * hist), rep
    # three such batches in flight
    tickets = [h.submit(b["seq1"], b["off1"], b["seq2"], b["off2"]) for _ in range(3)]
    for t in tickets:
        hg, hi = h.wait(t)
        assert np.array_equal(want[0], hg) and np.array_equal(want[1], hi)
    assert np.array_equal(h.gene_counts(65536), 5 * hist)
    h.close()


def test_reads_of_exactly_k_bases_on_the_motif(oracle, probe):
    """single-slot reads, every one a 65 536-way tie: batches of 1, 63, 64 and 65 of them -- the EMIT pass with that many work items.
    One index for the four batches; the oracle's answer is computed once for the 65 reads and shared by the probe variants (its answer
    for the first n reads is its answer for the batch of n: it classifies read by read); the device-resident entry point takes the
    batch of 65."""
    from shark_amd import SharkHip
    genes, motif, _, memo, _ = _long_reference(65536)
    reads = [bytes(motif[i % 24:i % 24 + 17]) if i % 2 == 0 else bytes(synth.revcomp(motif[i % 24:i % 24 + 17])) for i in range(65)]
    if "k-base reads" not in memo:
        o = oracle.Shark(k=17, c=1.0, bf_bits=1 << 30)
        o.build([bytes(g) for g in genes], nthreads=8)
        b = synth.batch_from_lists(reads)
        memo["k-base reads"] = o.classify(b["seq1"], b["off1"], nthreads=16)
        o.close()
    wg, wi = memo["k-base reads"]
    assert (_counts(wg) == 65536).all()
    h = SharkHip(k=17, c=1.0, bf_bits=1 << 30)
    h.build([bytes(g) for g in genes])
    for n_reads in (1, 63, 64, 65):
        b = synth.batch_from_lists(reads[:n_reads])
        if n_reads == 65:
            goff, gids, tags = _both_entries(None, h, b, want=(wg, wi))
        else:
            goff, gids = h.classify(b["seq1"], b["off1"])
            tags = h.last_kernel()
            assert np.array_equal(goff, wg[:n_reads + 1]) and np.array_equal(gids, wi[:n_reads * 65536]), n_reads
        assert int(h.timing()["last_n_tie"]) == n_reads
        assert np.array_equal(gids.reshape(n_reads, 65536), np.tile(np.arange(65536, dtype=np.uint16), (n_reads, 1)))
        assert ("classify_fast_kernel" if probe in ("bitvector", "force-generic") else "classify_uni_kernel") in tags, tags
    h.close()


# ---------------------------------------------------------------------------
# the reference program's recorded answers (tests/golden/ref_repeat_cases.npz), no oracle in the loop
# ---------------------------------------------------------------------------
def test_recorded_repeat_cases(probe):
    """one whole-program case per builder, recorded from the reference CLI: gene lists read by read and in order, host and
    device-resident entry points"""
    import os
    from shark_amd import SharkHip
    from tests import ref_cases as rc
    cases = rc.load(os.path.join(rc.GOLD, "ref_repeat_cases.npz"))
    assert [cs["name"] for cs in cases] == list(rr.BUILDER_CASES)
    for cs in cases:
        want = rc.associations(cs)
        goff = np.concatenate([[0], np.cumsum([len(a) for a in want])]).astype(np.uint32)
        gids = np.array([g for a in want for g in a], np.uint16)
        h = SharkHip(k=cs["k"], c=float(cs["c"]), bf_bits=cs["bf_bits"], min_quality=cs["q"], single=cs["single"])
        h.build([s for _, s in rc.parse_fasta(cs["fasta"])])
        _both_entries(None, h, rc.batch(cs), want=(goff, gids))
        h.close()
