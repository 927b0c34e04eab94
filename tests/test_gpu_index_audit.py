"""Every derived index array on the device, entry by entry, against the oracle (tests/index_audit.py).

Each case declares its reference, k, filter size and environment switches, AND the arrays and probe mode the build must produce:
an array that silently was not built fails the case.  The auditor itself is tested without a GPU in tests/test_index_audit.py."""
import os

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

from tests import index_audit as ia
from tests import repeat_refs as rr
from tests import synth

pytestmark = pytest.mark.gpu

CORE = frozenset({"rank_w", "ent", "ids"})
ANCH = frozenset({"atab", "ref2", "refpay", "refext", "refmul"})
TAB = CORE | {"tab"} | ANCH
LDS = TAB | {"lsum32", "ltab"}                 # a small index in a filter of 2^24 ... 2^33 bits
N = ord("N")


def _rng(seed):
    return np.random.default_rng(seed)


def _lower(rng, s, rate=0.05):
    s = s.copy()
    lo = (rng.random(len(s)) < rate) & (s != N)
    s[lo] |= 0x20
    return s


# ---- references -----------------------------------------------------------------------------------------------------------
def ref_example(example_dir):
    return [s for _, s in synth.read_fasta(os.path.join(example_dir, "ENSG00000277117.fa"))]


def ref_random(seed, n, lo, hi, share_every=0):
    return lambda _: synth.make_genes(_rng(seed), n, lo, hi, share_every=share_every)


def ref_record_ends(k, total):
    """records that end at concatenated positions 255, 256, 257 and 256 + k - 1, then one that fills up to `total` bases"""
    def make(_):
        rng = _rng(100 + k)
        lens = [255, 1, 1, k - 2]
        recs = [synth.random_seq(rng, n) for n in lens]
        recs.append(_lower(rng, synth.random_seq(rng, total - sum(lens))))
        assert list(np.cumsum(lens)) == [255, 256, 257, 256 + k - 1]
        return recs
    return make


def ref_n_at(k, t, total):
    """one record: an N at position t, and the last valid start of a later run at 512 + t (the same place in its 256-position block)"""
    def make(_):
        rng = _rng(200 + 7 * k + t)
        s = _lower(rng, synth.random_seq(rng, total))
        s[t] = N
        s[512 + t + k] = N
        return [synth.random_seq(rng, 0), s]
    return make


def ref_short_records(k):
    """records of 0, k - 1, k and k + 1 bases, one of only N that is at least k long (it takes no gene number: the records behind it
    are numbered one lower than they are counted) and one that is shorter"""
    def make(_):
        rng = _rng(300 + k)
        r = lambda n: synth.random_seq(rng, n)
        return [r(100), r(0), r(k - 1), r(k), np.full(k + 2, N, np.uint8), r(k + 1), r(200), np.full(min(3, k - 1), N, np.uint8),
                _lower(rng, r(150)), r(0)]
    return make


def ref_clip_runs(k):
    """records whose valid positions form runs of exactly 253, 254, 255 and 600"""
    def make(_):
        rng = _rng(400 + k)
        return [synth.random_seq(rng, n + k - 1) for n in (50, 253, 254, 255, 600)]
    return make


def ref_multi_run(k):
    """runs of more than 254 positions whose lists are all multi-gene (a prefix / a suffix two genes share), the nearest single-gene
    list just inside reach for some of their positions and just outside for others"""
    def make(_):
        rng = _rng(500 + k)
        pre, suf = synth.random_seq(rng, 300 + k), synth.random_seq(rng, 280 + k)
        r = lambda n: synth.random_seq(rng, n)
        return [np.concatenate([pre, r(60)]), np.concatenate([pre, r(90)]), np.concatenate([r(70), suf]), np.concatenate([r(40), suf])]
    return make


def ref_repeats(k):
    """low-complexity runs (homopolymers up to 1 000 bases, period 2 and 3: even-k palindromes, many occurrences per key, both strands),
    a tandem array and poly-A carriers"""
    def make(_):
        rng = _rng(600 + k)
        genes, _m = rr.compose(rr.low_complexity(rng, rr.plain(rng, 12, 200, 500)[0], k), rr.tandem(rng, 37, 12, True), rr.poly_a_carriers(rng, 10))
        genes.append(synth.revcomp(genes[0]))
        return genes
    return make


BIG = ref_random(7, 60, 1800, 2100)            # ~117 000 bases: the table outgrows 4 MiB, the 2^18-bit summary passes too much
DENSE = ref_random(8, 40, 100, 1500, 4)


def case(name, ref, k, bf_bits, arrays, mode, env=(), perpos=True):
    return pytest.param({"ref": ref, "k": k, "bf_bits": bf_bits, "env": dict(env), "arrays": frozenset(arrays), "mode": mode, "perpos": perpos}, id=name)


CASES = [
    case("example-k17-2^33", ref_example, 17, 1 << 33, LDS, "lds-table"),
    case("one-gene-k17-2^33", ref_random(1, 1, 2000, 2000), 17, 1 << 33, LDS, "lds-table"),
    case("genes-k31-2^26", ref_random(2, 24, 100, 1200, 4), 31, 1 << 26, LDS, "lds-table"),
    case("genes-k21-2^26", ref_random(3, 24, 100, 1200, 3), 21, 1 << 26, LDS, "lds-table"),
    case("dense-k17-2^18", DENSE, 17, 1 << 18, TAB, "table"),
    case("dense-k11-2^18", DENSE, 11, 1 << 18, TAB, "table"),
    case("long-lists-k5-2^12", DENSE, 5, 1 << 12, TAB, "table", perpos=False),
    case("mod-k17-1000003", DENSE, 17, 1000003, TAB, "table-mod"),
    case("mod-k21-1000003", ref_random(9, 30, 100, 1500, 3), 21, 1000003, TAB, "table-mod"),
    case("tab-dense-k17-2^26", ref_random(10, 50, 900, 1100), 17, 1 << 26, TAB | {"lsum32"}, "lds-summary+table", {"SHK_TAB_DENSE": "1"}),
    case("tab-dense-k11-2^18", DENSE, 11, 1 << 18, TAB, "table", {"SHK_TAB_DENSE": "1"}),
    case("no-lds-summary-k21-2^26", ref_random(3, 24, 100, 1200, 3), 21, 1 << 26, TAB, "table", {"SHK_NO_LDS_SUMMARY": "1"}),
    case("big-k17-2^26", BIG, 17, 1 << 26, TAB | {"sum32", "lbig32"}, "summary+table"),
    case("big-k31-2^26", BIG, 31, 1 << 26, TAB | {"sum32", "lbig32"}, "summary+table"),
    case("big-no-summary-k21-2^26", BIG, 21, 1 << 26, TAB | {"lbig32"}, "table", {"SHK_NO_SUMMARY": "1"}),
    case("big-no-lds-summary-k16-2^26", BIG, 16, 1 << 26, TAB | {"sum32"}, "summary+table", {"SHK_NO_LDS_SUMMARY": "1"}),
    case("no-refext-k17-2^26", ref_random(2, 24, 100, 1200, 4), 17, 1 << 26, LDS - {"refext", "refmul"}, "lds-table", {"SHK_NO_REFEXT": "1"}),
    case("no-anchor-k17-2^26", ref_random(2, 24, 100, 1200, 4), 17, 1 << 26, LDS - ANCH, "lds-table", {"SHK_NO_ANCHOR": "1"}),
    case("multi-run-k17", ref_multi_run(17), 17, 1 << 26, LDS, "lds-table"),
    case("multi-run-k11", ref_multi_run(11), 11, 1 << 26, LDS, "lds-table"),
    case("repeats-k16", ref_repeats(16), 16, 1 << 26, LDS, "lds-table"),
    case("repeats-k17", ref_repeats(17), 17, 1 << 26, LDS, "lds-table"),
    case("repeats-k17-2^18", ref_repeats(17), 17, 1 << 18, TAB, "table"),
]
for _k in (2, 16, 21):
    CASES.append(case("short-records-k%d" % _k, ref_short_records(_k), _k, 1 << 26, LDS, "lds-table"))
for _k in (16, 21):
    CASES.append(case("clip-runs-k%d" % _k, ref_clip_runs(_k), _k, 1 << 26, LDS, "lds-table"))
for _k, _total in ((2, 1024), (11, 1040), (17, 1023), (31, 999)):   # totals that are and are not multiples of 16 and 32
    CASES.append(case("record-ends-k%d" % _k, ref_record_ends(_k, _total), _k, 1 << 26, LDS, "lds-table"))
    for _t in sorted({255, 256, 257, 256 + _k - 1}):
        CASES.append(case("N-at-%d-k%d" % (_t, _k), ref_n_at(_k, _t, _total + 200), _k, 1 << 26, LDS, "lds-table"))


def test_case_table_audits_every_array_three_times():
    for name in ia.ARRAYS:
        n = sum(name in p.values[0]["arrays"] for p in CASES)
        assert n >= 3, (name, n)
    assert {p.values[0]["k"] for p in CASES} >= {2, 11, 16, 17, 21, 31}
    assert {p.values[0]["bf_bits"] for p in CASES} >= {1 << 33, 1 << 26, 1 << 18, 1 << 12, 1000003}
    envs = set().union(*[set(p.values[0]["env"]) for p in CASES])
    assert envs >= {"SHK_TAB_DENSE", "SHK_NO_LDS_SUMMARY", "SHK_NO_SUMMARY", "SHK_NO_REFEXT", "SHK_NO_ANCHOR"}


def build_case(c, oracle, example_dir, setenv):
    """(model, arrays, meta, mode) of a case; setenv(name, value) sets a switch for the build"""
    from shark_amd import SharkHip
    recs = [bytes(g) for g in c["ref"](example_dir)]
    assert sum(len(r) for r in recs) <= 125000
    for name, val in c["env"].items():
        setenv(name, val)
    o = oracle.Shark(k=c["k"], bf_bits=c["bf_bits"])
    o.build(recs)
    h = SharkHip(k=c["k"], bf_bits=c["bf_bits"])
    info = h.build(recs)
    assert info["nidx"] == o.nidx and info["n_set_bits"] == o.num_kmer()
    A, meta = ia.pull(h)
    mode = h.probe_mode()
    h.close()
    m = ia.Model(oracle, o, recs, c["k"], c["bf_bits"])
    o.close()
    return m, A, meta, mode


@pytest.mark.parametrize("c", CASES)
def test_index_arrays_match_the_oracle(c, oracle, example_dir, monkeypatch):
    m, A, meta, mode = build_case(c, oracle, example_dir, monkeypatch.setenv)
    assert mode == c["mode"], (mode, sorted(A))
    assert set(A) == c["arrays"], (sorted(set(A) ^ c["arrays"]), mode)
    assert meta["wrap"] == 0 and meta["pow2"] == int(c["bf_bits"] & (c["bf_bits"] - 1) == 0)
    if "refpay" in A:
        # the per-position copies of the multi-gene lists: built unless they would take more than 16 ids per base
        assert m.perpos_expected() == c["perpos"], (m.multi_R, m.total)
        assert (meta["ent_len"] > m.n_set + 1) == c["perpos"], meta
    res = ia.audit_all(m, A, meta)
    assert set(res) == c["arrays"]
    bad = {n: v for n, v in res.items() if v}
    assert not bad, bad


def test_multi_run_case_has_positions_out_of_reach(oracle, example_dir):
    """the declaration of the multi-run reference: valid positions with no single-gene list within 254 on either side, next to ones with"""
    recs = [bytes(g) for g in ref_multi_run(17)(example_dir)]
    o = oracle.Shark(k=17, bf_bits=1 << 26)
    o.build(recs)
    m = ia.Model(oracle, o, recs, 17, 1 << 26)
    left, right = ia._runs(m.valid)
    cs = np.concatenate([[0], np.cumsum(m.single)])
    x = np.arange(m.total)
    reach = cs[x + np.minimum(right, 254) + 1] - cs[x - np.minimum(left, 254)] > 0
    out = m.valid & ~reach
    assert out.sum() >= 20 and (m.valid & reach & ~m.single).sum() >= 500
    edge = np.flatnonzero(out[:-1] != out[1:])
    assert len(edge) >= 4                                       # reach ends inside the runs, on the prefixes and on the suffixes
