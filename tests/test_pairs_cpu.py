"""Pairs mode without a GPU: the model (tests/pairs_model.py) against records worked by hand, the case table (tests/pairs_cases.py)
against what each case was built for, the bundled example's figures, named wrong implementations that the cases must tell from the
model, the text forms, and the boundary (header, binding, library symbols, command-line flags)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.align_model import expected_alignments, sam_lines
from tests.pairs_cases import MAX_FRAG, MIN_INTRON, N_BINS, case_batch, check_expectations, s_min_for
from tests.pairs_model import CLASS_NAMES, Fragments, expected_pairs, fragments_text, mapq_of, pair_record, sam_pairs_lines
from tests.segments_model import SegmentsModel, expected_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")


def _rec(blocks, strand=0):
    out = np.zeros((), dtype=capi.ALIGNMENT_DTYPE)
    out["n_blocks"], out["strand"] = len(blocks), strand
    for r, b in enumerate(blocks):
        out["block"][r] = b
    return out


def _pair(a, b, la=60, lb=60, n=1, min_intron=20, max_frag=1000, wrong=None):
    p = pair_record([a, b], (la, lb), n, min_intron, max_frag, wrong)
    return tuple(int(p[f]) for f in ("cls", "left", "proper", "mapq", "tstart", "tend", "introns", "frag"))


NONE = _rec([])


# ---------------------------------------------------------------------------
# records worked by hand
# ---------------------------------------------------------------------------
def test_the_worked_example_of_the_header():
    m1 = _rec([(100, 2, 58)], 0)
    m2 = _rec([(300, 0, 20), (1400, 20, 37)], 1)
    #                          cls left proper mapq tstart tend introns frag
    assert _pair(m1, m2) == (3, 0, 1, 60, 100, 1437, 1080, 262)
    assert _pair(m2, m1) == (3, 1, 1, 60, 100, 1437, 1080, 262)
    assert _pair(m1, m2, max_frag=261)[2] == 0 and _pair(m1, m2, max_frag=262)[2] == 1
    # at min_intron 1081 the gap is a deletion: it stays in the fragment
    assert _pair(m1, m2, min_intron=1081, max_frag=2000) == (3, 0, 1, 60, 100, 1437, 0, 1342)
    assert _pair(m1, m2, min_intron=1080)[6] == 1080


def test_classes_left_and_the_tie_breaks_by_hand():
    f = lambda x, n=60: _rec([(x, 0, n)], 0)  # noqa: E731
    r = lambda x, n=60: _rec([(x, 0, n)], 1)  # noqa: E731
    assert _pair(NONE, NONE, n=3) == (0, 0, 0, 1, 0, 0, 0, 0)
    assert _pair(f(10), NONE) == (1, 0, 0, 60, 10, 70, 0, 0)
    assert _pair(NONE, r(10), 60, 60, 2) == (2, 1, 0, 3, 10, 70, 0, 0)
    assert _pair(f(10), r(200)) == (3, 0, 1, 60, 10, 260, 0, 250)
    assert _pair(r(10), f(200)) == (4, 0, 0, 60, 10, 260, 0, 0)                    # outward
    assert _pair(f(10), f(200))[:2] == (5, 0) and _pair(r(200), r(10))[:2] == (5, 1)
    # dovetail by the definition (s_F <= s_R, e_F > e_R), containment either way
    assert _pair(f(10), r(10, 50), 60, 50)[:2] == (4, 1)                         # equal s: the smaller e is left
    assert _pair(f(10), r(20, 40), 60, 40)[:2] == (4, 0)
    assert _pair(f(20, 40), r(10), 40, 60)[:2] == (4, 1)
    # equal s and e: mate 0, whichever strand it is on
    assert _pair(f(10), r(10))[:2] == (3, 0) and _pair(r(10), f(10))[:2] == (3, 0)
    assert _pair(f(10), r(10), wrong="tie1")[1] == 1
    assert [mapq_of(n) for n in (1, 2, 3, 4, 5, 9)] == [60, 3, 1, 1, 0, 0]


def test_the_union_of_introns_and_the_clips_by_hand():
    # both mates across the same intron [130, 1130): once
    a = _rec([(100, 0, 30), (1130, 30, 30)], 0)
    b = _rec([(110, 0, 20), (1130, 20, 40)], 1)
    assert _pair(a, b) == (3, 0, 1, 60, 100, 1170, 1000, 70)
    assert _pair(a, b, wrong="sum")[6] == 2000
    # different introns; partly overlapping introns count every base once
    c = _rec([(1150, 0, 20), (2170, 20, 40)], 1)
    assert _pair(a, c)[4:] == (100, 2210, 2000, 110)
    d = _rec([(100, 0, 30), (1100, 30, 30)], 0)       # [130, 1100)
    e = _rec([(120, 0, 30), (1200, 30, 30)], 1)       # [150, 1200): union [130, 1200)
    assert _pair(d, e)[6] == 1070
    # three introns in one mate, one shared
    g = _rec([(0, 0, 15), (100, 15, 15), (200, 30, 15), (300, 45, 15)], 0)
    h = _rec([(210, 0, 5), (300, 5, 55)], 1)
    assert _pair(g, h)[4:] == (0, 355, 85 * 3, 100)
    # a gap below min_intron is a deletion
    i = _rec([(100, 0, 30), (135, 30, 30)], 0)
    assert _pair(i, _rec([(300, 0, 60)], 1))[4:] == (100, 360, 0, 260)
    assert _pair(i, _rec([(300, 0, 60)], 1), min_intron=5)[4:] == (100, 360, 5, 255)
    # clips: F's left and R's right are put back; F's right and R's left are not
    fc = _rec([(104, 4, 50)], 0)                      # 4 clipped on the left, 6 on the right
    rc_ = _rec([(302, 2, 53)], 1)                     # 2 on the left, 5 on the right
    assert _pair(fc, rc_)[4:] == (104, 355, 0, 251 + 4 + 5)
    assert _pair(fc, rc_, wrong="noclip")[7] == 251
    # mate lengths beyond 2^31 - 1 are clamped as align_kernel clamps them
    assert _pair(_rec([(0, 0, 10)], 0), _rec([(5, 0, 10)], 1), 10, 1 << 33)[7] == 15 + (1 << 31) - 1 - 10


def test_fragments_state_and_text():
    fr = Fragments(8)
    pairs = np.zeros(5, dtype=capi.PAIR_DTYPE)
    pairs["cls"] = [3, 3, 3, 1, 3]
    pairs["frag"] = [6, 7, 400, 0, 2]
    fr.add(pairs, [0, 1, 2, 3, 3, 5])                 # the last read has two associations: counted by class, not in the histogram
    assert fr.classes == [0, 1, 0, 4, 0, 0] and fr.hist == [0, 0, 0, 0, 0, 0, 1, 2]
    assert fr.text() == "class none 0\nclass mate1 1\nclass mate2 0\nclass inward 4\nclass outward 0\nclass tandem 0\nfrag 6 1\nfrag >=7 2\n"
    assert fragments_text([0, 0], [0] * 6).endswith("class tandem 0\nfrag >=1 0\n")
    fr.reset()
    assert sum(fr.classes) == 0 and sum(fr.hist) == 0 and CLASS_NAMES[3] == "inward"


# ---------------------------------------------------------------------------
# the case table on the CPU: oracle -> segments model -> alignment model -> pairs model
# ---------------------------------------------------------------------------
def _table(oracle, k, twins=False, n_bins=N_BINS):
    rec, names, batch, expect = case_batch(k, n_bins=n_bins)
    records = [bytes(rec)] * (2 if twins else 1)
    o = oracle.Shark(k=k, c=0.0, bf_bits=1 << 26)
    o.build(records)
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel(records, k)
    recs = expected_alignments(sm, batch, goff, gids, expected_segments(sm, batch, goff, gids, 4)[1], s_min_for(k))
    return names, batch, expect, goff, gids, recs


@pytest.fixture(scope="module")
def table17(oracle):
    return _table(oracle, 17)


def test_every_case_is_what_it_was_built_for(table17):
    names, batch, expect, goff, gids, recs = table17
    pairs = expected_pairs(recs, batch, goff, MIN_INTRON, MAX_FRAG)
    check_expectations(names, pairs, goff, expect)
    assert set(pairs["cls"].tolist()) == {0, 1, 2, 3, 4, 5}
    assert set(pairs["left"].tolist()) == {0, 1} and set(pairs["proper"].tolist()) == {0, 1} and (pairs["mapq"] == 60).all()
    fr = Fragments(N_BINS).add(pairs, goff)
    assert fr.classes == np.bincount(pairs["cls"], minlength=6).tolist() and sum(fr.hist) == fr.classes[3]
    assert fr.hist[N_BINS - 2] == 1 and fr.hist[N_BINS - 1] == 2
    assert len(names) == len(goff) - 1


def test_the_overflow_bin_at_64_bins(oracle):
    names, batch, expect, goff, gids, recs = _table(oracle, 17, n_bins=64)
    pairs = expected_pairs(recs, batch, goff, MIN_INTRON, MAX_FRAG)
    check_expectations(names, pairs, goff, expect)
    fr = Fragments(64).add(pairs, goff)
    assert fr.hist[62] == 1 and fr.hist[63] > 2 and sum(fr.hist) == fr.classes[3]


def test_twins_halve_nothing_but_mapq_and_the_histogram(oracle, table17):
    names, batch, expect, goff, gids, recs = _table(oracle, 17, twins=True)
    pairs = expected_pairs(recs, batch, goff, MIN_INTRON, MAX_FRAG)
    check_expectations(names, pairs, goff, expect, every=2)
    assert (pairs["mapq"] == 3).all() and pairs[0::2].tobytes() == pairs[1::2].tobytes()
    fr = Fragments(N_BINS).add(pairs, goff)
    assert sum(fr.hist) == 0 and fr.classes[3] > 0
    one = expected_pairs(table17[5], table17[1], table17[3], MIN_INTRON, MAX_FRAG)
    for f in ("cls", "left", "proper", "tstart", "tend", "introns", "frag"):
        assert np.array_equal(pairs[0::2][f], one[f]), f


def _raw_mates(batch):
    off1, off2 = batch["off1"], batch["off2"]
    return [(bytes(batch["seq1"][int(off1[i]):int(off1[i + 1])]), bytes(batch["seq2"][int(off2[i]):int(off2[i + 1])])) for i in range(len(off1) - 1)]


@pytest.mark.parametrize("wrong,cases", [("sum", {"one junction, both mates"}), ("noclip", {"clipped 5' end of F", "clipped 5' end of R", "both 5' ends clipped"}),
                                         ("tie1", {"equal starts and ends", "equal starts and ends, mates swapped"}), ("proper4", {"outward", "dovetail, equal starts"})])
def test_the_table_kills_named_wrong_implementations(table17, wrong, cases):
    """introns summed instead of united, frag without the clips, the last tie-break to mate 1, 0x2 on outward pairs: each differs from the
    model on the cases built against it -- in the records and in the SAM lines"""
    names, batch, expect, goff, gids, recs = table17
    good = expected_pairs(recs, batch, goff, MIN_INTRON, MAX_FRAG)
    bad = expected_pairs(recs, batch, goff, MIN_INTRON, MAX_FRAG, wrong=wrong)
    differ = {names[i] for i in range(len(names)) if good[int(goff[i])].tobytes() != bad[int(goff[i])].tobytes()}
    assert cases <= differ, (wrong, differ)
    ids = ["r%d" % i for i in range(len(names))]
    args = (ids, _raw_mates(batch), None, goff, gids, recs)
    a = sam_pairs_lines(*args, good, ["g"], True, MIN_INTRON)
    b = sam_pairs_lines(*args, bad, ["g"], True, MIN_INTRON)
    # (the lines show left and proper; introns and frag only through proper)
    assert len(a) == len(b) and (a != b) == (wrong in ("tie1", "proper4"))


def test_sam_pairs_fields_on_the_table(table17):
    names, batch, expect, goff, gids, recs = table17
    pairs = expected_pairs(recs, batch, goff, MIN_INTRON, MAX_FRAG)
    ids = ["r%d" % i for i in range(len(names))]
    plain = sam_lines(ids, _raw_mates(batch), None, goff, gids, recs, ["g"], True, MIN_INTRON)
    lines = sam_pairs_lines(ids, _raw_mates(batch), None, goff, gids, recs, pairs, ["g"], True, MIN_INTRON)
    by_read = {}
    for ln, pl in zip(lines, plain):
        f, g = ln.split("\t"), pl.split("\t")
        assert g[4] == "255" and g[8] == "0" and not int(g[1]) & 0x2
        assert [v for n, v in enumerate(f) if n not in (1, 4, 8)] == [v for n, v in enumerate(g) if n not in (1, 4, 8)]
        assert int(f[1]) & ~0x2 == int(g[1]) and f[4] == "60"
        by_read.setdefault(f[0], []).append((int(f[1]), int(f[8])))
    for i, name in enumerate(names):
        got = by_read.get("r%d" % i, [])
        p = pairs[int(goff[i])]
        assert len(got) == (0, 1, 1, 2, 2, 2)[int(p["cls"])], name
        assert all(bool(fl & 0x2) == bool(p["proper"]) for fl, _ in got), name
        if len(got) == 2:
            span = int(p["tend"]) - int(p["tstart"])
            assert [t for _, t in got] == ([span, -span] if p["left"] == 0 else [-span, span]), name
        elif got:
            assert got[0][1] == 0, name
    assert any(fl & 0x2 for v in by_read.values() for fl, _ in v)


# ---------------------------------------------------------------------------
# the bundled example
# ---------------------------------------------------------------------------
# the model's figures at k = 17, c = 0.6, s_min = 8, min_intron = 20, max_frag = 1000, 1024 bins: 1 929 associations of 1 929 reads
EXAMPLE_CLASSES = [0, 0, 0, 995, 934, 0]
EXAMPLE_HIST_TOTAL = 995
EXAMPLE_PROPER = 784


def example_pairs(oracle, fa, min_intron=20, max_frag=1000):
    from tests.test_align_cpu import _example_alignments
    recs, lines, fasta, stats = _example_alignments(oracle, fa)
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    o.build([s for _, s in fa])
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    pairs = expected_pairs(recs, batch, goff, min_intron, max_frag)
    ids = [i.decode() if isinstance(i, bytes) else str(i) for i, _, _ in r1]
    quals = [(bytes(a[2]), bytes(b[2])) for a, b in zip(r1, r2)]
    legend = [n.decode() for n, _ in fa]
    sam = sam_pairs_lines(ids, _raw_mates(batch), quals, goff, gids, recs, pairs, legend, True, min_intron)
    return recs, pairs, goff, gids, sam, lines, fasta


def test_the_example_in_figures(oracle):
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    recs, pairs, goff, gids, sam, plain, fasta = example_pairs(oracle, fa)
    fr = Fragments(1024).add(pairs, goff)
    print("example: classes", fr.classes, "histogram total", sum(fr.hist), "overflow", fr.hist[-1], "proper", int(pairs["proper"].sum()),
          "median frag", int(np.median(pairs["frag"][pairs["cls"] == 3])))
    assert fr.classes == EXAMPLE_CLASSES and sum(fr.classes) == 1929
    assert sum(fr.hist) == EXAMPLE_HIST_TOTAL == fr.classes[3]          # one gene: every read has one association
    assert int(pairs["proper"].sum()) == EXAMPLE_PROPER
    assert len(sam) == len(plain) == 3858
    assert sum(int(ln.split("\t")[8]) for ln in sam) == 0             # a pair's two TLENs cancel


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_pairs_enable", "shk_pairs_last", "shk_fragments_get", "shk_fragments_reset")


def test_header_declares_and_binding_binds_the_new_calls():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "/* ---- pairs:" in text and text.index("/* ---- pairs:") > text.index("/* ---- alignments:")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    for s in ("shk_pair", "shk_pairs"):
        assert re.search(r"\}\s*%s\s*;" % s, hdr), s
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("pairs_enable", "pairs_last", "fragments", "fragments_reset"):
        assert callable(getattr(SharkHip, name))
    assert callable(capi.pairs_from_device) and capi.PAIR_DTYPE.itemsize == 32 and capi.PAIR_CLASS_NAMES == CLASS_NAMES
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_the_kernels_register_line_shows_no_spills_and_no_scratch():
    text = open(os.path.join(ROOT, "profiles", "pairs_kernel_regs.txt")).read()
    line = next(ln for ln in text.split("\n") if ln.startswith("pair_kernel<true>"))
    assert "spill v0 s0" in line and re.search(r"scratch\s+0\b", line), line


def test_cli_flags():
    import subprocess
    cli = os.path.join(ROOT, "shark_amd", "bin", "shark")
    assert os.path.exists(cli), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    run = lambda *a: subprocess.run([cli, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    r = run("--sam-pairs")
    assert r.returncode == 1 and "--sam-pairs needs --sam FILE" in r.stderr
    for flag in ("--fragments-max", "--fragments-bins", "--fragments-min-intron"):
        r = run(flag, "100")
        assert r.returncode == 1 and "need --fragments FILE" in r.stderr, flag
    for bins in ("1", "4097"):
        r = run("--fragments", "f", "--fragments-bins", bins)
        assert r.returncode == 1 and "--fragments-bins must be 2 to 4096" in r.stderr
    r = run("--fragments", "f", "--fragments-min-intron", "0")
    assert r.returncode == 1 and "--fragments-min-intron must be at least 1" in r.stderr
    r = subprocess.run([cli, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and all(s in r.stderr for s in ("--sam-pairs", "--fragments FILE", "--fragments-max N", "--fragments-bins N", "--fragments-min-intron N"))
