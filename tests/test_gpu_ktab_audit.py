"""The minimiser-bucketed table on the device (`shk_probe_mode()` = "minimiser-table"; DeviceIndex::ktab), audited entry by entry
(tests/ktab_audit.py) against the oracle's filter, and every key it holds probed through both classify entry points.

Per case: the filter words on the device equal the oracle's; the expected keys are every canonical k-mer whose bit the ORACLE's
words have set (pyoracle.filter_sweep: all 4^k values at k = 15 and 16; at k = 17 four slices of 2^28 values -- [0, 2^28) and one
starting at j 2^32 + 2^31 for j = 1, 2, 3, so that key bits above bit 31 are covered -- plus every reference k-mer, flagged "must be
stored", plus whatever else the table holds, each such key admitted only if the oracle's words have its bit); the low words come
from index_audit.Model; audit_ktab must find nothing.  The conditions a case is there for (palindromic keys, keys >= 2^32, a
crowded line, paths that wrap behind the last line) are shown on the CPU from the expected keys before the device is asked.
Then every stored key on both strands, and for every displaced key its three variants in the first and in the last base (mostly
non-keys that walk the same path), as single-end reads of k bases through shk_classify and device-resident: the oracle's answers.
Cases a and c also embed the keys in a ragged batch of 40-60 base reads (the other walk code).

A failure of the audit is the builder's (ktab_build_kernel, ktab_home), a failure of the probes with a clean audit the probe's
(classify_uni_rounds.inc).

Measured beside an MI355X, the sweep on 16 CPU threads (one thread: 2.1 s for the 2^30 values of k = 15):
  sweep    k = 15, all 2^30 values: 0.15 s    k = 16, all 2^32 values: 1.15 s (hence no slices at k = 16)    k = 17, 4 x 2^28: 0.4 s
  case     keys      displaced  longest path   audit    probes (reads)       ragged   whole case (with the reference, where not shared)
  a  k=15  360 282     1 605        2          0.23 s   0.11 s (730 194)     0.13 s   1.3 s
  b  k=16  339 574     1 513        3          0.22 s   0.08 s (688 226)       -      1.7 s    7 palindromic keys
  c  k=17  387 104     1 042        3          0.32 s   0.09 s (780 460)     0.28 s   1.5 s    217 943 keys >= 2^32
  d  k=15  360 282    21 539        9          0.17 s   0.09 s (849 798)       -      0.3 s    load 0.5, 2^16 lines
  e  k=17  387 104     1 384        4          0.32 s   0.10 s (782 512)       -      0.6 s    w = 14
  f  k=17  350 019     2 077        4          0.23 s   0.09 s (712 500)       -      1.2 s    34 paths wrap behind the last line
No violation in any of them.

Run on the GPU box with `pytest -m gpu`."""
import os
import time

import numpy as np
import pytest

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

from tests import index_audit, ktab_audit, repeat_refs, synth
from tests.ktab_audit import KTAB_C2, audit_ktab, ktab_home_model, revcompl, stored_keys
from tests.test_gpu_ktab import _hip, _ktab_env

pytestmark = pytest.mark.gpu

_U = np.uint64
CASES = {
    #      k   filter   reference        environment                how the expected keys are had
    "a": (15, 1 << 26, "plain", {}, "full"),
    "b": (16, 1 << 28, "plain", {}, "full"),
    "c": (17, 1 << 30, "saturated", {}, "slices"),
    "d": (15, 1 << 26, "plain", {"SHK_KTAB_LOAD": "50"}, "full"),
    "e": (17, 1 << 30, "saturated", {"SHK_KTAB_W": "14"}, "slices"),
    "f": (17, 1 << 30, "last-line", {}, "slices"),
}
RAGGED = ("a", "c")


def _threads():
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))


def _ranges(k, how):
    if how == "full":
        return [(0, 1 << (2 * k))]
    return [(0, 1 << 28)] + [((j << 32) + (1 << 31), (j << 32) + (1 << 31) + (1 << 28)) for j in (1, 2, 3)]


def _plain_genes(k, seed=1000):
    return synth.make_genes(np.random.default_rng(seed + k), 40, 300, 2000, share_every=3)


class _Reference:
    """what the oracle says about one reference: its filter, the model of index_audit, the swept keys.  Shared by the cases with
    the same k, filter and genes, and left unchanged by them."""

    def __init__(self, oracle, k, bf_bits, genes, how):
        self.k, self.bf_bits, self.genes = k, bf_bits, [bytes(g) for g in genes]
        self.o = oracle.Shark(k=k, c=0.0, bf_bits=bf_bits)
        self.o.build(self.genes)
        self.words = self.o.bf_words()
        self.m = index_audit.Model(oracle, self.o, self.genes, k, bf_bits)
        self.ranges = _ranges(k, how)
        t0 = time.perf_counter()
        swept = [oracle.filter_sweep(k, self.words, bf_bits, lo, hi, nthreads=_threads())[1] for lo, hi in self.ranges]
        self.sweep_s = time.perf_counter() - t0
        self.ref = np.unique(self.m.canon[self.m.vx])
        self.base = np.union1d(np.concatenate(swept), self.ref)
        self.oracle = oracle

    def in_filter(self, x):
        """does the ORACLE's filter have the bit of each k-mer of x?"""
        p = self.oracle.get_hash_many(x) % _U(self.bf_bits)
        return ((self.words[(p >> _U(6)).astype(np.int64)] >> (p & _U(63))) & _U(1)) != 0

    def low_of(self, keys):
        p = self.oracle.get_hash_many(keys) % _U(self.bf_bits)
        rk = np.searchsorted(self.m.setbits, p)
        assert np.array_equal(self.m.setbits[np.minimum(rk, self.m.n_set - 1)], p), "an expected key whose bit is not set"
        return index_audit.expected_low(self.m, rk)


_references = {}


def _reference(oracle, k, bf_bits, name, genes, how):
    key = (k, bf_bits, name)
    if key not in _references:
        _references[key] = _Reference(oracle, k, bf_bits, genes, how)
    return _references[key]


def _last_line_wmer(line_lg, w=15):
    """as repeat_refs.smallest_hash_wmer: the canonical w-mer with the smallest hash h whose line (h * KTAB_C2) >> (32 - line_lg)
    is the table's last"""
    inv = pow(repeat_refs.KTAB_C1, -1, 1 << 32)
    for h0 in range(1, 1 << 32, 1 << 22):
        h = np.arange(h0, h0 + (1 << 22), dtype=np.uint64)
        a = (h * _U(inv)) & _U(0xFFFFFFFF)
        line = ((h * _U(KTAB_C2)) & _U(0xFFFFFFFF)) >> _U(32 - line_lg)
        for i in np.flatnonzero((a < _U(1 << (2 * w))) & (line == _U((1 << line_lg) - 1))):
            s = repeat_refs._unpack(int(a[i]), w)
            if int(a[i]) <= repeat_refs._pack(synth.revcomp(s)) and repeat_refs.wmer_hash(s) == int(h[i]):
                return s
    raise AssertionError("no w-mer found")


def _ascii(x, k):
    """k-mers (first base most significant) as reads of k bases, back to back"""
    x = np.asarray(x, dtype=np.uint64)
    sh = (_U(2) * np.arange(k - 1, -1, -1, dtype=np.uint64))[None, :]
    return synth.ACGT[((x[:, None] >> sh) & _U(3)).astype(np.int64)]


def _both_entry_points(ref, h, seq, off, max_len):
    """the batch through shk_classify and device-resident: the oracle's answers, by the minimiser-table kernel"""
    from shark_amd.capi import hip_memcpy_dtoh
    n = len(off) - 1
    og, oi = ref.o.classify(seq, off, None, None, nthreads=_threads())
    hg, hi = h.classify(seq, off)
    assert ", 8, " in h.last_kernel(), h.last_kernel()
    assert np.array_equal(og, hg) and np.array_equal(oi, hi), "shk_classify differs from the oracle"
    dev = torch.device("cuda:0")
    ds, do = torch.from_numpy(seq).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
    r = h.classify_device(n, ds.data_ptr(), do.data_ptr(), max_read_len=max_len)
    assert ", 8, " in h.last_kernel(), h.last_kernel()
    dg = np.empty(n + 1, np.uint32)
    hip_memcpy_dtoh(dg, r.gene_off, dg.nbytes)
    di = np.empty(int(r.n_assoc), np.uint16)
    if len(di):
        hip_memcpy_dtoh(di, r.gene_ids, di.nbytes)
    assert np.array_equal(og, dg) and np.array_equal(oi, di), "shk_classify_device differs from the oracle"
    return int((np.diff(og.astype(np.int64)) > 0).sum())


@pytest.mark.parametrize("case", sorted(CASES))
def test_table_audit_and_every_key_probed(oracle, monkeypatch, capsys, case):
    k, bf_bits, refname, env, how = CASES[case]
    t_start = time.perf_counter()
    _ktab_env(monkeypatch)
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    w = min(int(env.get("SHK_KTAB_W", 15)), k)
    load = int(env.get("SHK_KTAB_LOAD", 9)) / 100.0
    kw = dict(k=k, c=0.0, bf_bits=bf_bits)
    # (case f: genes whose table stays well inside its size when the crafted ones are added -- 40 genes of this length put the
    #  builder's estimate within a few per cent of a doubling; seed 1000 + k would cross it)
    genes = _plain_genes(k, 4000 if refname == "last-line" else 1000)
    if refname == "saturated":
        genes = genes + repeat_refs.saturated_neighbourhood(np.random.default_rng(7), k, 15)[0]
    elif refname == "last-line":
        # build once for the table's size, craft the neighbourhood of a w-mer whose line is the last, build again
        h0 = _hip(**kw)
        h0.build([bytes(g) for g in genes])
        assert h0.probe_mode() == "minimiser-table"
        lg0 = h0.debug_ktab_meta()["ktab_lg"]
        h0.close()
        genes = genes + repeat_refs.saturated_neighbourhood(np.random.default_rng(8), k, 15, _last_line_wmer(lg0 - 3))[0]
        refname = "last-line-%d" % lg0
    ref = _reference(oracle, k, bf_bits, refname, genes, how)
    m = ref.m

    # ---- what the case is there for, shown on the CPU from the oracle's keys alone ----
    line_lg = ktab_audit.line_lg_rule(m.n_set, bf_bits, k, load)
    home, _ = ktab_home_model(ref.base, k, w, line_lg)
    per_bucket = np.bincount(home, minlength=8 << line_lg)
    per_line = np.bincount(home >> 3, minlength=1 << line_lg)
    if case == "b":
        assert (ref.base == revcompl(ref.base, k)).sum() >= 1
    if k == 17:
        assert (ref.base >= _U(1 << 32)).sum() >= 1
    if case == "c":
        assert per_line.max() >= 48                      # 16 slots: at least 32 of them leave the line
    if case == "d":
        assert per_bucket.max() >= 5                     # two slots a bucket: the fifth key of a home sits two lines down or further
    if case == "f":
        assert per_line[-1] >= 17                        # at least one leaves the LAST line: its path wraps to line 0

    # ---- the device's table ----
    h = _hip(**kw)
    info = h.build(ref.genes)
    assert h.probe_mode() == "minimiser-table"
    assert info["n_set_bits"] == m.n_set
    meta = h.debug_ktab_meta()
    assert meta["ktab_lg"] == line_lg + 3 and meta["ktab_w"] == w, (meta, line_lg, w)
    if case == "f":
        assert meta["ktab_lg"] == lg0
    assert h.debug_index_meta()["ktab_lg"] == meta["ktab_lg"]
    assert np.array_equal(h.copy_bf(), ref.words), "the filter on the device is not the oracle's"
    ktab = h.debug_index_array("ktab")
    t_audit = time.perf_counter()
    # the expected keys: swept ranges + reference k-mers, and outside the ranges whatever the table holds THAT THE ORACLE'S FILTER HAS
    slot, got = stored_keys(ktab, meta, k)
    extra = got[(got < _U(1 << (2 * k))) & (got <= revcompl(got, k))]
    inside = np.zeros(len(extra), dtype=bool)
    for lo, hi in ref.ranges:
        inside |= (extra >= _U(lo)) & (extra < _U(hi))
    extra = np.unique(extra[~inside])
    keys = np.union1d(ref.base, extra[ref.in_filter(extra)]) if len(extra) else ref.base
    low = ref.low_of(keys)
    viol, st = audit_ktab(ktab, meta, k, keys, low, ref.ranges, np.isin(keys, ref.ref))
    t_audit = time.perf_counter() - t_audit
    assert viol == [], viol
    assert st["keys"] == meta["ktab_keys"] == len(keys), (st, meta, len(keys))
    if how == "full":
        assert len(extra) == 0
    if case == "b":
        assert st["palindromic"] >= 1, st
    if k == 17:
        assert st["above_2_32"] >= 1, st
    if case == "c":
        assert st["displaced"] >= 32, st
    if case == "d":
        assert st["displaced"] >= int(np.maximum(per_bucket - 2, 0).sum()) > 100 and st["longest_path"] >= 2, st
    if case == "f":
        assert st["wrapped"] >= 1, st

    # ---- every stored key on both strands; the near misses of the displaced ones ----
    t_probe = time.perf_counter()
    khome, _ = ktab_home_model(got, k, w, line_lg)
    disp = got[(slot >> 4) != (khome >> 3)]
    assert len(disp) == st["displaced"]
    top = _U(2 * (k - 1))
    near = np.concatenate([disp ^ (_U(j) << top) for j in (1, 2, 3)] + [disp ^ _U(j) for j in (1, 2, 3)])
    reads = np.concatenate([got, revcompl(got, k), near])
    seq = np.ascontiguousarray(_ascii(reads, k).reshape(-1))
    off = np.arange(len(reads) + 1, dtype=np.uint64) * _U(k)
    hits = _both_entry_points(ref, h, seq, off, k)
    assert hits >= 2 * len(got)                           # (c = 0: a read that is a key is assigned)
    t_probe = time.perf_counter() - t_probe

    # ---- the same keys inside longer reads, ragged ----
    t_ragged = time.perf_counter()
    if case in RAGGED:
        rng = np.random.default_rng(99)
        n = len(got)
        lens = rng.integers(40, 61, size=n)
        roff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        rseq = synth.ACGT[rng.integers(0, 4, size=int(roff[-1]))]
        at = roff[:-1].astype(np.int64) + rng.integers(0, lens - k + 1)
        fwd = np.where(rng.integers(0, 2, size=n) == 1, got, revcompl(got, k))
        rseq[at[:, None] + np.arange(k)[None, :]] = _ascii(fwd, k)
        assert _both_entry_points(ref, h, np.ascontiguousarray(rseq), roff, 60) == n
    t_ragged = time.perf_counter() - t_ragged
    h.close()
    with capsys.disabled():
        print("\n[ktab audit %s] k=%d w=%d lines=2^%d keys=%d displaced=%d longest=%d wrapped=%d palindromic=%d above_2^32=%d | sweep %.2f s "
              "(shared per reference), audit %.2f s, probes %.2f s (%d reads), ragged %.2f s, case %.2f s"
              % (case, k, w, line_lg, st["keys"], st["displaced"], st["longest_path"], st["wrapped"], st["palindromic"], st["above_2_32"],
                 ref.sweep_s, t_audit, t_probe, len(reads), t_ragged, time.perf_counter() - t_start))


def test_no_table_reads_back_empty(monkeypatch):
    """an index without the table: "ktab" has size 0, the scalars are zero, and `meta` says the same"""
    _ktab_env(monkeypatch, on=False)
    genes = [bytes(g) for g in _plain_genes(15)[:5]]
    h = _hip(k=15, c=0.0, bf_bits=1 << 26)
    h.build(genes)
    assert h.probe_mode() != "minimiser-table"
    assert len(h.debug_index_array("ktab")) == 0
    assert h.debug_ktab_meta() == {"ktab_lg": 0, "ktab_w": 0, "ktab_keys": 0}
    assert h.debug_index_meta()["ktab_lg"] == 0
    h.close()
