"""Rescue mode on the GPU (shk_rescue_enable / shk_rescue_last, `shark --sam-rescue`): per association the 16-byte rescue record and the
rescued mates' alignment records, against the model (tests/rescue_model.py) bit for bit on the case table (tests/rescue_cases.py).  No
tolerances anywhere.  The model's results for the table are computed once per module and shared.

Run on the GPU box with `pytest -m gpu`."""
import os

import numpy as np
import pytest

import torch  # noqa: F401  torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both

from shark_amd import capi
from tests import synth
from tests.align_model import sam_header, verify_sam_line
from tests.pairs_model import Fragments, expected_pairs, sam_pairs_lines
from tests.rescue_cases import MAX_FRAG, MIN_INTRON, MIN_QUALITY, PARAMS, S_MIN, case_batch, check_expectations, make_decoy, reference
from tests.rescue_model import expected_rescue, sam_rescue_lines
from tests.test_gpu_align import model_records, run_shark, same_records
from tests.test_gpu_segments import _args, _dev_ptrs, _to_device
from tests.test_gpu_spliced_depth import device_assoc
from tests.test_gpu_variants import build_kb

pytestmark = pytest.mark.gpu

SCAN_LANES = 512 * 256          # rescue_scan_kernel's capped grid: more reads than this take the stride loop's second trip
RESCUE_WAVES = 512 * 4          # rescue_kernel's capped grid: more queue entries than this take its stride loop's second trip


def same_rescue(got_al, got_rs, want_al, want_rs, cases=None, goff=None, details=None):
    """alignment records and rescue records bit for bit; a mismatch names case, association, candidate, pass and lane"""
    assert got_rs.dtype == capi.RESCUE_DTYPE and got_rs.shape == want_rs.shape, (got_rs.shape, want_rs.shape)
    assert got_al.dtype == capi.ALIGNMENT_DTYPE and got_al.shape == want_al.shape, (got_al.shape, want_al.shape)
    if got_rs.tobytes() == want_rs.tobytes() and got_al.tobytes() == want_al.tobytes():
        return
    bad = [j for j in range(len(want_rs)) if got_rs[j].tobytes() != want_rs[j].tobytes() or got_al[j].tobytes() != want_al[j].tobytes()]
    j = bad[0]
    where = ""
    if goff is not None and cases is not None:
        i = int(np.searchsorted(np.asarray(goff), j, side="right")) - 1
        where = "case %r (%s), " % (cases[i % len(cases)]["name"], cases[i % len(cases)]["why"])
    if details is not None and details.get(j):
        d = details[j]
        x = d["best"]
        t = int(got_rs[j]["state"]) - 4
        gx = int(got_al[j, t]["block"][0][0]) if t in (0, 1) else None
        where += "model's best candidate x = %d (pass %d, lane %d, window [%d, %d]), device's x = %s%s, " % (
            x, (x - d["lo"]) // 64, (x - d["lo"]) % 64, d["lo"], d["hi"], gx,
            "" if gx is None or gx not in d["costs"] else " (pass %d, lane %d, model's cost there %d)" % ((gx - d["lo"]) // 64, (gx - d["lo"]) % 64, d["costs"][gx]))
    raise AssertionError("%sassociation %d: rescue record %s, model %s; alignment records %s, model %s (%d associations differ)" % (
        where, j, got_rs[j], want_rs[j], got_al[j], want_al[j], len(bad)))


class Table:
    """the case table at one k with the model's results: alignment records with the mode off, and per parameter set the records with it on"""

    def __init__(self, oracle, k, every=1):
        self.k, self.every = k, every
        self.rec, self.cases, self.batch = case_batch(k)
        self.genes = reference(every)
        self.o, self.h, self.sm = build_kb(oracle, self.genes, k=k, min_quality=MIN_QUALITY)
        self.goff, self.gids = self.o.classify(*_args(self.batch))
        self.al_off = model_records(self.o, self.sm, self.batch, self.goff, self.gids, S_MIN, MIN_QUALITY)
        self.details = {}
        self.on = {}

    def model(self, params):
        if params not in self.on:
            self.details[params] = {}
            self.on[params] = expected_rescue(self.al_off, self.batch, self.goff, self.gids, dict(enumerate(bytes(g) for g in self.genes)), *PARAMS[params],
                                              min_quality=MIN_QUALITY, details=self.details[params])
        return self.on[params]

    def enable(self, params="default", h=None):
        h = h or self.h
        h.alignments_enable(S_MIN)
        h.rescue_enable(*PARAMS[params])
        return h

    def check(self, al, rs, params="default"):
        want_al, want_rs = self.model(params)
        same_rescue(al, rs, want_al, want_rs, self.cases, self.goff, self.details[params])


@pytest.fixture(scope="module")
def table17(oracle):
    return Table(oracle, 17)


# ---------------------------------------------------------------------------
# (a) the case table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,every", [(17, 1), (17, 2), (31, 1)])
def test_case_table(oracle, table17, k, every):
    """every case of tests/rescue_cases.py at the three parameter sets: alignment records and rescue records are the model's bit for bit
    (from the alignment model's records, which the device's mode-off records equal); the twins are rescued independently"""
    t = table17 if (k, every) == (17, 1) else Table(oracle, k, every)
    h = t.h
    h.alignments_enable(S_MIN)
    goff, gids = h.classify(*_args(t.batch))
    assert np.array_equal(goff, t.goff) and np.array_equal(gids, t.gids)
    same_records(h.alignments_last(), t.al_off)
    with pytest.raises(Exception):
        h.rescue_last()                                             # that batch was submitted with the mode off
    for params in PARAMS:
        t.enable(params)
        goff, gids = h.classify(*_args(t.batch))
        assert np.array_equal(goff, t.goff) and np.array_equal(gids, t.gids)
        al, rs = h.alignments_last(), h.rescue_last()
        t.check(al, rs, params)
        seen = check_expectations(t.cases, params, al, rs, goff, every)
        print("k", k, "genes", every, params, "states", np.bincount(rs["state"], minlength=6).tolist())
        if params == "default":
            assert seen == {0, 1, 2, 3, 4, 5}


def test_a_single_end_batch_attempts_nothing(oracle, table17):
    rec, cases, batch = case_batch(17, single_end=True)
    h = table17.enable()
    goff, gids = h.classify(*_args(batch))
    rs = h.rescue_last()
    assert len(rs) == len(gids) > 0 and not rs.view(np.uint32).any()
    o = table17.o
    same_records(h.alignments_last(), model_records(o, table17.sm, batch, goff, gids, S_MIN, MIN_QUALITY))


# ---------------------------------------------------------------------------
# (b) the stride loops and the queue
# ---------------------------------------------------------------------------
def tiled(batch, times):
    out = {}
    for m in ("1", "2"):
        lens = np.diff(batch["off" + m].astype(np.int64))
        out["seq" + m] = np.tile(batch["seq" + m], times)
        out["qual" + m] = np.tile(batch["qual" + m], times)
        off = np.zeros(len(lens) * times + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.tile(lens, times))
        out["off" + m] = off
    return out


def test_more_reads_than_scan_lanes_and_more_attempts_than_rescue_waves(table17):
    """the table 2 500 times over: more reads than rescue_scan_kernel's grid has lanes and more attempted associations than rescue_kernel's
    grid has waves -- the second trips of both stride loops, the queue filled by every wave of the scan.  The records are the table's,
    tiled"""
    t = table17
    times = 2500
    n = len(t.cases) * times
    want_al, want_rs = t.model("default")
    attempted = int((want_rs["state"] != 0).sum()) * times
    assert n > SCAN_LANES and attempted > RESCUE_WAVES
    big = tiled(t.batch, times)
    h = t.enable()
    goff, gids = h.classify(*_args(big))
    assert np.array_equal(goff, np.arange(n + 1, dtype=goff.dtype)) and len(gids) == n
    al, rs = h.alignments_last(), h.rescue_last()
    same_rescue(al, rs, np.tile(want_al, (times, 1)), np.tile(want_rs, times), t.cases, goff)


# ---------------------------------------------------------------------------
# (c) the four families
# ---------------------------------------------------------------------------
def test_all_four_families(table17):
    t = table17
    h = t.enable()
    goff, gids = h.classify(*_args(t.batch))                        # shk_classify: pinned memory
    t.check(h.alignments_last(), h.rescue_last())
    t0, t1 = h.submit(*_args(t.batch)), h.submit(*_args(t.batch))   # two tickets in flight: each wait hands out its own batch's records
    for tk in (t0, t1):
        goff, gids = h.wait(tk)
        assert np.array_equal(goff, t.goff)
        t.check(h.alignments_last(), h.rescue_last())
    dev = _to_device(t.batch)
    n = len(t.cases)
    for family in (lambda: h.classify_device(n, max_read_len=600, **_dev_ptrs(dev)), lambda: h.wait_device(h.submit_device(n, max_read_len=120, **_dev_ptrs(dev)))):   # (the ticket family takes a bound the kernels are specialised for: the table's long mates are repaired in wait)
        goff, gids = device_assoc(family())                         # resident batches: the records stay in device memory
        assert np.array_equal(goff, t.goff) and np.array_equal(gids, t.gids)
        na, pa = h.alignments_last()
        nr, pr = h.rescue_last()
        assert na == nr == len(gids)
        t.check(capi.alignments_from_device(na, pa), capi.rescues_from_device(nr, pr))


# ---------------------------------------------------------------------------
# (d) the repair paths
# ---------------------------------------------------------------------------
def test_association_overflow_repair(oracle, table17):
    """more associations than a slot reserves (two per read + 4 096): the table 25 times over against six identical genes -- the records
    come from the tail's second run in wait; every gene's association is rescued as the one gene's is (tests/test_rescue_cpu.py: twins
    are rescued independently)"""
    t = table17
    times, genes = 25, 6
    n = len(t.cases) * times
    assert genes * n > 2 * n + 4096
    big = tiled(t.batch, times)
    o, h, sm = build_kb(oracle, [t.rec] * genes, k=17, min_quality=MIN_QUALITY)
    t.enable(h=h)
    goff, gids = h.classify(*_args(big))
    assert np.array_equal(goff, genes * np.arange(n + 1, dtype=np.int64)) and np.array_equal(gids, np.tile(np.arange(genes, dtype=gids.dtype), n))
    want_al, want_rs = t.model("default")
    same_rescue(h.alignments_last(), h.rescue_last(), np.tile(np.repeat(want_al, genes, axis=0), (times, 1)), np.tile(np.repeat(want_rs, genes), times))
    assert (want_rs["state"] >= 4).sum() >= 30


def test_length_bound_repair(table17):
    """the table's long mates behind max_read_len = 100 are repaired in wait (general kernel, tail again): the records are the final ones"""
    t = table17
    h = t.enable()
    dev = _to_device(t.batch)
    goff, gids = device_assoc(h.wait_device(h.submit_device(len(t.cases), max_read_len=100, **_dev_ptrs(dev))))
    assert h.timing()["last_n_long"] > 0
    assert np.array_equal(goff, t.goff) and np.array_equal(gids, t.gids)
    na, pa = h.alignments_last()
    nr, pr = h.rescue_last()
    t.check(capi.alignments_from_device(na, pa), capi.rescues_from_device(nr, pr))


# ---------------------------------------------------------------------------
# (e) shk_count_work, state and argument rules
# ---------------------------------------------------------------------------
def test_count_work_state_and_argument_rules(oracle, table17):
    from shark_amd import SharkHip, SharkHipError
    t = table17
    h = SharkHip(k=17, c=0.0, bf_bits=1 << 26)
    with pytest.raises(SharkHipError, match="not finalized"):
        h.rescue_enable()
    h.rescue_enable(max_frag=0)                                     # (switching off is always allowed)
    o, h, sm = build_kb(oracle, t.genes, keep_bases=False, k=17, min_quality=MIN_QUALITY)
    with pytest.raises(SharkHipError, match="without shk_ref_keep_bases"):
        h.rescue_enable()
    o, h, sm = build_kb(oracle, t.genes, k=17, min_quality=MIN_QUALITY)
    with pytest.raises(SharkHipError, match="alignments mode is off"):
        h.rescue_enable()
    h.alignments_enable(S_MIN)
    for bad in (dict(max_frag=4097), dict(min_intron=0), dict(max_cost=256), dict(min_gap=256)):
        with pytest.raises(SharkHipError, match="invalid argument|max_frag"):
            h.rescue_enable(**bad)
    for fine in (dict(max_frag=4096, max_cost=255, min_gap=255), dict(max_frag=1, max_cost=0, min_gap=0, min_intron=1)):
        h.rescue_enable(**fine)
    with pytest.raises(SharkHipError):
        h.rescue_last()                                             # no batch yet
    h.rescue_enable(max_frag=0)
    h.classify(*_args(t.batch))
    with pytest.raises(SharkHipError):
        h.rescue_last()                                             # that batch was submitted with the mode off
    off = h.alignments_last()
    same_records(off, t.al_off)
    h.rescue_enable(*PARAMS["default"])
    tk = h.submit(*_args(t.batch))
    for call in (lambda: h.rescue_enable(*PARAMS["default"]), lambda: h.rescue_enable(max_frag=0)):
        with pytest.raises(SharkHipError, match="outstanding"):
            call()
    h.wait(tk)
    t.check(h.alignments_last(), h.rescue_last())
    # shk_count_work: neither records are handed out behind it; with the mode switched off the same batch's alignment records are
    # bit-identical to those of a context on which the mode never ran
    dev = _to_device(t.batch)
    p = _dev_ptrs(dev)
    h.count_work(len(t.cases), p["seq1"], p["off1"], p["seq2"], p["off2"], p["qual1"], p["qual2"])
    for call in (h.rescue_last, h.alignments_last):
        with pytest.raises(SharkHipError):
            call()
    h.rescue_enable(max_frag=0)
    h.classify(*_args(t.batch))
    assert h.alignments_last().tobytes() == off.tobytes()
    with pytest.raises(SharkHipError):
        h.rescue_last()
    # alignments mode off with rescue mode left on: idle; switching on again is refused while it is off
    h.rescue_enable(*PARAMS["default"])
    h.alignments_enable(0)
    h.classify(*_args(t.batch))
    with pytest.raises(SharkHipError):
        h.rescue_last()
    with pytest.raises(SharkHipError, match="alignments mode is off"):
        h.rescue_enable(*PARAMS["default"])


# ---------------------------------------------------------------------------
# (f) pairs mode behind rescue mode
# ---------------------------------------------------------------------------
def test_pairs_mode_sees_the_rescued_mate(table17):
    """the pair records equal pairs_model applied to the rescued alignment records; a rescued pair is class 3 and proper, its frag the
    formula's, and it enters the histogram"""
    t = table17
    h = t.enable()
    h.pairs_enable(MIN_INTRON, MAX_FRAG, 1024)
    h.fragments_reset()
    goff, gids = h.classify(*_args(t.batch))
    al, rs, pr = h.alignments_last(), h.rescue_last(), h.pairs_last()
    t.check(al, rs)
    want = expected_pairs(t.model("default")[0], t.batch, goff, MIN_INTRON, MAX_FRAG)
    assert pr.tobytes() == want.tobytes()
    rescued = rs["state"] >= 4
    assert rescued.sum() > 30 and (pr["cls"][rescued] == 3).all() and (pr["proper"][rescued] == 1).all() and (pr["frag"][rescued] <= MAX_FRAG).all()
    j = int(goff[[c["name"] for c in t.cases].index("A on strand 0 as mate 1")])
    assert int(pr[j]["frag"]) == 700 + 100 - 500
    hist, classes = h.fragments(1024)
    mh, mc = Fragments(1024).add(want, goff).arrays()
    assert np.array_equal(hist, mh) and np.array_equal(classes, mc) and int(hist.sum()) >= int(rescued.sum())
    h.pairs_enable(n_bins=0)


# ---------------------------------------------------------------------------
# (g) inertness
# ---------------------------------------------------------------------------
def test_rescue_mode_is_inert(table17):
    """every older mode on.  A context on which rescue mode was switched on and off again gives what a context that never heard of it
    gives, byte for byte, shk_last_kernel included; with the mode on everything but the rescued mates' alignment records and their
    associations' pair records is the same"""
    from shark_amd import SharkHip
    t = table17
    seen = {}
    for how in ("never", "off again", "on"):
        h = SharkHip(k=17, c=0.0, bf_bits=1 << 26, min_quality=MIN_QUALITY)
        h.build([bytes(g) for g in t.genes], keep_bases=True)
        h.evidence_enable(True)
        h.candidates_enable(4)
        h.placement_enable(True)
        h.segments_enable(2)
        h.depth_enable_spliced(8)
        h.junctions_enable(8, 1024)
        h.pileup_enable(8)
        h.alignments_enable(S_MIN)
        h.pairs_enable(MIN_INTRON, MAX_FRAG, 1024)
        if how != "never":
            h.rescue_enable(*PARAMS["default"])
        if how == "off again":
            h.rescue_enable(max_frag=0)
        goff, gids = h.classify(*_args(t.batch))
        keys, segs = h.segments_last()
        cr, ce = h.candidates_last()
        hist, classes = h.fragments(1024)
        seen[how] = dict(fixed=(goff.tobytes(), gids.tobytes(), h.last_kernel(), h.evidence_last().tobytes(), cr.tobytes(), ce.tobytes(), h.placement_last().tobytes(),
                                keys.tobytes(), segs.tobytes(), h.gene_counts().tobytes(), h.depth_all().tobytes(), h.depth_mates(), h.depth_summary().tobytes(),
                                h.junctions_get().tobytes(), h.pileup_all().tobytes(), h.pileup_mates(), h.variants().tobytes(), h.variants_summary().tobytes()),
                         al=h.alignments_last(), pr=h.pairs_last(), frag=(hist.tobytes(), classes.tobytes()))
        if how == "on":
            rs = h.rescue_last()
    a, b, c = seen["never"], seen["off again"], seen["on"]
    assert a["fixed"] == b["fixed"] and a["al"].tobytes() == b["al"].tobytes() and a["pr"].tobytes() == b["pr"].tobytes() and a["frag"] == b["frag"]
    assert a["fixed"] == c["fixed"]
    for j in range(len(rs)):
        touched = int(rs[j]["state"]) >= 4
        for m in range(2):
            assert (a["al"][j, m].tobytes() == c["al"][j, m].tobytes()) == (not (touched and int(rs[j]["state"]) == 4 + m)), (j, m)
        assert (a["pr"][j].tobytes() == c["pr"][j].tobytes()) == (not touched), j
    assert (rs["state"] >= 4).sum() > 30 and a["frag"] != c["frag"]


# ---------------------------------------------------------------------------
# (h) the command
# ---------------------------------------------------------------------------
def _differ(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    at = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
    return "line %d of %d / %d: got %r, model %r" % (at, len(g), len(w), g[at:at + 1], w[at:at + 1])


def test_shark_sam_rescue(oracle, tmp_path):
    """--sam --sam-pairs --sam-rescue on the table written out as a sample, three times over: the model's file from one worker, from two
    workers on one device and at two batch sizes; every line passes the line-plus-FASTA verifier, the rescued lines carry YR:i:; without
    --sam-rescue the file is what --sam --sam-pairs wrote before the flag existed"""
    from types import SimpleNamespace
    from tests.segments_model import SegmentsModel
    rec, cases, one = case_batch(17)
    batch = tiled(one, 3)
    n = 3 * len(cases)
    ids = ["r%d" % i for i in range(n)]
    mates = lambda m: [bytes(batch["seq" + m][int(batch["off" + m][i]):int(batch["off" + m][i + 1])]) for i in range(n)]      # noqa: E731
    quals = lambda m: [bytes(batch["qual" + m][int(batch["off" + m][i]):int(batch["off" + m][i + 1])]) for i in range(n)]     # noqa: E731
    for m in ("1", "2"):
        with open(tmp_path / ("s_%s.fq" % m), "wb") as f:
            for rid, s, q in zip(ids, mates(m), quals(m)):
                f.write(b"@" + rid.encode() + b"\n" + s + b"\n+\n" + q + b"\n")
    with open(tmp_path / "ref.fa", "wb") as f:
        f.write(b">gene\n" + bytes(rec) + b"\n>decoy\n" + bytes(make_decoy()) + b"\n")
    o = oracle.Shark(k=17, c=0.0, bf_bits=1 << 33, min_quality=MIN_QUALITY)
    genes = {0: bytes(rec), 1: bytes(make_decoy())}
    o.build(list(genes.values()))
    goff, gids = o.classify(*_args(batch))
    sm = SegmentsModel(list(genes.values()), 17)
    al_off = model_records(o, sm, batch, goff, gids, S_MIN, MIN_QUALITY)
    al_on, rs = expected_rescue(al_off, batch, goff, gids, genes, *PARAMS["default"], min_quality=MIN_QUALITY)
    raw = list(zip(mates("1"), mates("2")))
    rq = list(zip(quals("1"), quals("2")))
    files = {}
    for name, al in (("off", al_off), ("on", al_on)):
        pairs = expected_pairs(al, batch, goff, MIN_INTRON, MAX_FRAG)
        lines = sam_pairs_lines(ids, raw, rq, goff, gids, al, pairs, ["gene", "decoy"], True, MIN_INTRON)
        if name == "on":
            owners = [(j, m) for i in range(n) for j in range(int(goff[i]), int(goff[i + 1])) for m in range(2) if al[j][m]["n_blocks"]]
            lines = sam_rescue_lines(lines, owners, rs)
            assert sum("\tYR:i:" in ln for ln in lines) == int((rs["state"] >= 4).sum()) > 90
            for ln in lines:
                verify_sam_line(ln, {"gene": genes[0], "decoy": genes[1]})
        header = sam_header(["gene", "decoy"], SimpleNamespace(records=genes), 2)
        files[name] = "".join(ln + "\n" for ln in header + lines).encode("latin-1")
    assert files["on"] != files["off"]
    base = ["-r", str(tmp_path / "ref.fa"), "-1", str(tmp_path / "s_1.fq"), "-2", str(tmp_path / "s_2.fq"), "-o", str(tmp_path / "o1"), "-p", str(tmp_path / "o2"),
            "-k", "17", "-c", "0", "-q", str(MIN_QUALITY), "--sam-min-support", str(S_MIN), "--sam-min-intron", str(MIN_INTRON), "--fragments-max", str(MAX_FRAG),
            "--sam-pairs"]
    for name, extra in (("a", []), ("b", ["--gpus", "2", "--devices", "0,0", "--batch", "40"]), ("c", ["--batch", "33"])):
        r = run_shark(base + ["--sam", str(tmp_path / ("s" + name)), "--sam-rescue"] + extra, str(tmp_path))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = (tmp_path / ("s" + name)).read_bytes()
        assert got == files["on"], _differ(got, files["on"])
    r = run_shark(base + ["--sam", str(tmp_path / "sd")], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = (tmp_path / "sd").read_bytes()
    assert got == files["off"], _differ(got, files["off"])
    # other costs: the flags reach the library
    r = run_shark(base + ["--sam", str(tmp_path / "se"), "--sam-rescue", "--rescue-max-cost", "0", "--rescue-min-gap", "1"], str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    al0, rs0 = expected_rescue(al_off, batch, goff, gids, genes, MIN_INTRON, MAX_FRAG, 0, 1, min_quality=MIN_QUALITY)
    assert (tmp_path / "se").read_bytes().count(b"\tYR:i:0\n") == int((rs0["state"] >= 4).sum()) > 0
