"""Rescue mode without a GPU: the model (tests/rescue_model.py) against records worked by hand, the case table (tests/rescue_cases.py)
against what each case was built for, named wrong implementations that the cases must tell from the model, the bundled example (on
which the mode attempts nothing), and the boundary (header, binding, library symbols, register file, command-line flags)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.align_model import expected_alignments
from tests.rescue_cases import CAP1, MIN_QUALITY, PARAMS, S_MIN, case_batch, check_expectations, reference
from tests.rescue_model import WRONG, expected_rescue, rescue_association
from tests.segments_model import SegmentsModel, expected_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")


def _rec(blocks, strand=0):
    out = np.zeros((), dtype=capi.ALIGNMENT_DTYPE)
    out["n_blocks"], out["strand"] = len(blocks), strand
    for r, b in enumerate(blocks):
        out["block"][r] = b
    return out


NONE = _rec([])


def _rs(rs):
    return tuple(int(rs[f]) for f in ("state", "cost", "cost2", "n_cand"))


# ---------------------------------------------------------------------------
# records worked by hand
# ---------------------------------------------------------------------------
def test_the_worked_example_of_the_header():
    rng = np.random.default_rng(3)
    rec = synth.random_seq(rng, 2000)
    m1 = rec[98:158].copy()                                       # (the record's {100, 2, 58}: two bases clipped on the left)
    t = rec[300:360].copy()
    for q in (10, 30, 50):
        t[q] = synth.ACGT[(int(np.searchsorted(synth.ACGT, t[q])) + 1) % 4]
    m2 = synth.revcomp(t)
    a = _rec([(100, 2, 58)], 0)
    detail = {}
    out, rs = rescue_association([a, NONE], (bytes(m1), bytes(m2)), bytes(rec), 20, 300, 8, 4, detail=detail)
    assert (detail["lo"], detail["hi"]) == (100, 338) and _rs(rs) == (5, 3, 13, 239)
    got = out[1]
    assert (int(got["n_blocks"]), int(got["strand"]), int(got["matches"]), int(got["mismatches"])) == (1, 1, 57, 3)
    assert tuple(int(v) for v in got["block"][0]) == (300, 0, 60) and not got["block"][1:].any()
    assert out[0].tobytes() == a.tobytes()
    # one of the three an N: the cost stays, the mismatches do not
    t[30] = ord("N")
    out, rs = rescue_association([a, NONE], (bytes(m1), bytes(synth.revcomp(t))), bytes(rec), 20, 300, 8, 4)
    assert _rs(rs) == (5, 3, 13, 239) and (int(out[1]["matches"]), int(out[1]["mismatches"])) == (57, 2)
    # pairs mode on the rescued records: the header's frag
    from tests.pairs_model import pair_record
    p = pair_record(out, (60, 60), 1, 20, 300)
    assert (int(p["cls"]), int(p["frag"]), int(p["proper"])) == (3, 262, 1)


def test_windows_states_and_ties_by_hand():
    rng = np.random.default_rng(4)
    rec = synth.random_seq(rng, 1000)
    rec[600:640] = rec[500:540]                                   # a copy 100 further on
    mate = lambda a, n: bytes(rec[a:a + n])                       # noqa: E731
    rcm = lambda a, n: bytes(synth.revcomp(rec[a:a + n]))         # noqa: E731
    run = lambda recs, mates, **kw: rescue_association(recs, mates, bytes(rec), kw.get("min_intron", 20), kw.get("max_frag", 300), 8, kw.get("min_gap", 4))  # noqa: E731
    f = _rec([(400, 0, 50)], 0)
    # not attempted: both, none, a single-end batch, a target of 31 or 513 bases
    for recs, mates in (([f, f], (mate(400, 50), mate(400, 50))), ([NONE, NONE], (mate(0, 50), mate(0, 50))), ([f, NONE], (mate(400, 50), None)),
                        ([f, NONE], (mate(400, 50), rcm(450, 31))), ([f, NONE], (mate(400, 50), b"A" * 513))):
        out, rs = run(recs, mates)
        assert _rs(rs) == (0, 0, 0, 0) and out[0].tobytes() == recs[0].tobytes() and out[1].tobytes() == recs[1].tobytes()
    # the tandem copy: ambiguous; at min_gap 0 the smaller frag -- the smaller x beside F, the larger beside R
    out, rs = run([f, NONE], (mate(400, 50), rcm(500, 40)))
    assert _rs(rs) == (3, 0, 0, 251) and out[1].tobytes() == NONE.tobytes()
    out, rs = run([f, NONE], (mate(400, 50), rcm(500, 40)), min_gap=0)
    assert _rs(rs) == (5, 0, 0, 251) and int(out[1]["block"][0][0]) == 500
    r = _rec([(700, 0, 50)], 1)
    out, rs = run([NONE, r], (mate(500, 40), rcm(700, 50)), min_gap=0)
    assert _rs(rs)[:3] == (4, 0, 0) and int(out[0]["block"][0][0]) == 600 and int(out[0]["strand"]) == 0
    # a spliced, clipped anchor on strand 0: s = 104, e = 354, cl = 4, I = 150: hi = 104 - 4 + 150 + 300 - 40
    sp = _rec([(104, 4, 46), (300, 50, 54)], 0)
    d = {}
    rescue_association([sp, NONE], (b"A" * 104, rcm(510, 40)), bytes(rec), 20, 300, 8, 4, detail=d)
    assert (d["lo"], d["hi"]) == (314, 510) and d["best"] == 510
    rescue_association([sp, NONE], (b"A" * 104, rcm(510, 40)), bytes(rec), 151, 300, 8, 4, detail=d)          # the gap is no intron
    assert (d["lo"], d["hi"]) == (314, 360)
    # ... and on strand 1: cr = 110 - 104 = 6: lo = 354 + 6 - 150 - 300 < 0, hi = min(104, 314)
    sp1 = _rec([(104, 4, 46), (300, 50, 54)], 1)
    rescue_association([sp1, NONE], (b"A" * 110, mate(20, 40)), bytes(rec), 20, 300, 8, 4, detail=d)
    assert (d["lo"], d["hi"]) == (0, 104) and d["best"] == 20
    rescue_association([sp1, NONE], (b"A" * 110, mate(20, 40)), bytes(rec), 20, 200, 8, 4, detail=d)
    assert (d["lo"], d["hi"]) == (10, 104)
    # an empty window, a window of one
    out, rs = run([_rec([(960, 0, 40)], 0), NONE], (mate(960, 40), rcm(900, 60)))
    assert _rs(rs) == (1, 13, 13, 0)
    out, rs = run([_rec([(960, 0, 40)], 0), NONE], (mate(960, 40), rcm(960, 40)))
    assert _rs(rs) == (5, 0, 13, 1)


# ---------------------------------------------------------------------------
# the case table on the CPU: oracle -> segments model -> alignment model -> rescue model
# ---------------------------------------------------------------------------
def _table(oracle, k, twins=False):
    rec, cases, batch = case_batch(k)
    records = [bytes(g) for g in reference(2 if twins else 1)]
    o = oracle.Shark(k=k, c=0.0, bf_bits=1 << 26, min_quality=MIN_QUALITY)
    o.build(records)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], batch["qual1"], batch["qual2"])
    sm = SegmentsModel(records, k)
    recs = expected_alignments(sm, batch, goff, gids, expected_segments(sm, batch, goff, gids, 4, MIN_QUALITY)[1], S_MIN, MIN_QUALITY)
    return cases, batch, goff, gids, recs, dict(enumerate(records))


@pytest.fixture(scope="module")
def table17(oracle):
    return _table(oracle, 17)


def _run(table, params="default", wrong=None, details=None):
    cases, batch, goff, gids, recs, genes = table
    return expected_rescue(recs, batch, goff, gids, genes, *PARAMS[params], min_quality=MIN_QUALITY, wrong=wrong, details=details)


@pytest.mark.parametrize("params", list(PARAMS))
def test_every_case_is_what_it_was_built_for(table17, params):
    cases, batch, goff, gids, recs, genes = table17
    out, rs = _run(table17, params)
    seen = check_expectations(cases, params, out, rs, goff)
    print(params, "states", np.bincount(rs["state"], minlength=6).tolist())
    if params == "default":
        assert seen == {0, 1, 2, 3, 4, 5}
        # the targets are silent and the anchors are not: exactly the associations built to be attempted are
        names = {c["name"] for c, r in zip(cases, rs) if r["state"] == 0}
        assert names == {"L_T = 31", "L_T = 513", "both mates placed", "no mate placed"}, names
        # passes and lanes: a winner in lane 0 of the first pass and in lane 63 of the last, n_cand on either side of 64 and 128
        assert {1, 63, 64, 65, 129, 512} <= set(rs["n_cand"].tolist())
    if params == "gap0":
        assert 3 not in seen
    # every record that is not a rescued mate's is untouched
    for j in range(len(rs)):
        for t in range(2):
            if int(rs[j]["state"]) != 4 + t:
                assert out[j, t].tobytes() == recs[j, t].tobytes()
            else:
                assert int(recs[j, t]["n_blocks"]) == 0 and int(out[j, t]["n_blocks"]) == 1


def test_the_table_at_k31(oracle):
    t = _table(oracle, 31)
    out, rs = _run(t)
    assert check_expectations(t[0], "default", out, rs, t[2]) == {0, 1, 2, 3, 4, 5}


def test_twins_are_rescued_independently(oracle, table17):
    t = _table(oracle, 17, twins=True)
    out, rs = _run(t)
    check_expectations(t[0], "default", out, rs, t[2], every=2)
    one_out, one_rs = _run(table17)
    assert rs[0::2].tobytes() == one_rs.tobytes() and rs[1::2].tobytes() == one_rs.tobytes()
    assert out[0::2].tobytes() == one_out.tobytes() and out[1::2].tobytes() == one_out.tobytes()


KILLS = {
    "no_introns": ("default", {"spliced anchor, target at hi"}),
    "no_clip": ("default", {"clipped 5' end of A on strand 0, target beyond hi", "clipped 5' end of A on strand 1, target below lo"}),
    "tie_far": ("gap0", {"tandem copy, A on strand 0", "tandem copy, A on strand 1", "near copy: best and second in one pass"}),
    "neither_matches": ("default", {"N in the target", "bases masked by -q", "record N under the target"}),
    "second_in_pass": ("default", {"tandem copy, A on strand 0", "tandem copy, A on strand 1", "copy apart by min_gap - 1"}),
    "no_complement": ("default", {"A on strand 0 as mate 1", "A on strand 0 as mate 2", "L_T = 32"}),
}


@pytest.mark.parametrize("wrong", WRONG)
def test_the_table_kills_named_wrong_implementations(table17, wrong):
    """the window without I_A, the window without cl / cr, the tie to the far candidate, "neither" counted as a match, the second best
    restricted to the best's own pass of 64, strand 1 without the complement: each differs from the model on the cases built against it"""
    params, must = KILLS[wrong]
    cases, batch, goff, gids, recs, genes = table17
    good_out, good_rs = _run(table17, params)
    bad_out, bad_rs = _run(table17, params, wrong=wrong)
    differ = {cases[i]["name"] for i in range(len(cases))
              if good_rs[int(goff[i])].tobytes() != bad_rs[int(goff[i])].tobytes() or good_out[int(goff[i])].tobytes() != bad_out[int(goff[i])].tobytes()}
    assert must <= differ, (wrong, differ)
    assert set(KILLS) == set(WRONG) and len(WRONG) >= 6


def test_costs_are_saturated(table17):
    """every reported cost is at most cap + 1, and a rescued mate's at most max_cost"""
    out, rs = _run(table17)
    assert int(rs["cost"].max()) == CAP1 and int(rs["cost2"].max()) == CAP1
    assert (rs["cost"][rs["state"] >= 4] <= PARAMS["default"][2]).all()


# ---------------------------------------------------------------------------
# the bundled example (no class 1 / 2 association)
# ---------------------------------------------------------------------------
def test_the_example_attempts_nothing(oracle):
    from tests.test_pairs_cpu import EXAMPLE, example_pairs
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    recs, pairs, goff, gids, sam, plain, fasta = example_pairs(oracle, fa)
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    out, rs = expected_rescue(recs, batch, goff, gids, dict(enumerate(s for _, s in fa)), 20, 1000, 8, 4)
    assert len(rs) == 1929 and not rs["state"].any() and not rs.view(np.uint32).any()
    assert out.tobytes() == np.asarray(recs).tobytes()
    assert int(((pairs["cls"] == 1) | (pairs["cls"] == 2)).sum()) == 0


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_rescue_enable", "shk_rescue_last")


def test_header_declares_and_binding_binds_the_new_calls():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "/* ---- rescue:" in text and text.index("/* ---- rescue:") > text.index("/* ---- pairs:")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    for s in ("shk_rescue", "shk_rescues"):
        assert re.search(r"\}\s*%s\s*;" % s, hdr), s
    assert re.search(r"#define\s+SHK_RESCUE_MIN_LEN\s+32\b", hdr) and re.search(r"#define\s+SHK_RESCUE_MAX_LEN\s+512\b", hdr)
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("rescue_enable", "rescue_last"):
        assert callable(getattr(SharkHip, name))
    assert callable(capi.rescues_from_device) and capi.RESCUE_DTYPE.itemsize == 16 and (capi.RESCUE_MIN_LEN, capi.RESCUE_MAX_LEN) == (32, 512)
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_the_kernels_register_lines_show_no_spills_no_scratch_and_two_workgroups_of_lds():
    text = open(os.path.join(ROOT, "profiles", "rescue_kernel_regs.txt")).read()
    for kernel in ("rescue_scan_kernel", "rescue_kernel"):
        line = next(ln for ln in text.split("\n") if ln.split(" ")[0] in (kernel, "shk::" + kernel))
        assert "spill v0 s0" in line and re.search(r"scratch\s+0\b", line), line
        assert int(re.search(r"lds\s+(\d+)", line).group(1)) * 2 <= 160 * 1024, line


def test_cli_flags():
    import subprocess
    cli = os.path.join(ROOT, "shark_amd", "bin", "shark")
    assert os.path.exists(cli), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    r = run("--sam-rescue")
    assert r.returncode == 1 and "--sam-rescue needs --sam FILE" in r.stderr
    for flag in ("--rescue-max-cost", "--rescue-min-gap"):
        r = run("--sam", "s", flag, "3")
        assert r.returncode == 1 and "need --sam-rescue" in r.stderr, flag
        r = run("--sam", "s", "--sam-rescue", flag, "256")
        assert r.returncode == 1 and "must be 0 to 255" in r.stderr, flag
    r = run("--sam", "s", "--sam-rescue", "--fragments-max", "4097")
    assert r.returncode == 1 and "--sam-rescue needs --fragments-max of 1 to 4096" in r.stderr
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stderr for s in ("--sam-rescue", "--rescue-max-cost N", "--rescue-min-gap N"))
