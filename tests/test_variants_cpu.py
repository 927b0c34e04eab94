"""Variants mode without a GPU: the model (tests/variants_model.py) on positions worked out by hand and on the bundled example indexed
against a copy of its record with a few substituted bases, the `--variants` line format, and the boundary -- the new symbols in
the header, the binding and the library, the new flags of the command."""
import os
import re
import subprocess

import numpy as np
import pytest

from shark_amd import capi
from tests import synth
from tests.depth_model import model_layout
from tests.pileup_model import expected_pileup
from tests.segments_model import SegmentsModel, expected_segments
from tests.variants_model import DEFAULTS, expected_recbase, expected_summary, expected_variants, position, variant_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")
A, C_, G, T = 0, 1, 2, 3
M32 = (1 << 32) - 1


def _sites(counts, record, params=DEFAULTS):
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1, 4)
    return expected_variants(counts, [record], [0, len(record)], params)


# ---------------------------------------------------------------------------
# the model on positions worked out by hand
# ---------------------------------------------------------------------------
def test_the_worked_example_of_the_header():
    assert position((12, 0, 5, 0), A, DEFAULTS) == (G, 17, True)            # 5 * 5 = 25 >= 1 * 17
    assert position((14, 0, 3, 0), A, DEFAULTS) == (G, 17, False)           # 3 * 5 = 15 <  17
    v = _sites([(12, 0, 5, 0), (14, 0, 3, 0)], b"AA")
    assert len(v) == 1 and tuple(v[0])[:4] == (0, 0, A, G) and v[0]["n"].tolist() == [12, 0, 5, 0]


def test_the_fraction_at_its_edge_and_one_observation_either_side():
    prm = (1, 1, 1, 5)
    assert position((16, 0, 4, 0), A, prm) == (G, 20, True)                 # 4 * 5 == 1 * 20
    assert position((17, 0, 4, 0), A, prm) == (G, 21, False)                # one more of the record's base: 20 < 21
    assert position((16, 0, 3, 0), A, prm) == (G, 19, False)                # one alt fewer: 15 < 19
    assert position((15, 0, 4, 0), A, prm) == (G, 19, True)                 # one of the record's base fewer: 20 >= 19
    assert position((16, 0, 5, 0), A, prm) == (G, 21, True)
    # 3/7: 3 * 14 == 7 * 6
    assert position((8, 6, 0, 0), A, (1, 1, 3, 7)) == (C_, 14, True) and position((9, 6, 0, 0), A, (1, 1, 3, 7)) == (C_, 15, False)
    # frac 0/1 never excludes, 1/1 asks for every observation
    assert position((100, 1, 0, 0), A, (1, 1, 0, 1))[2] and position((0, 9, 0, 0), A, (1, 1, 1, 1))[2] and not position((1, 9, 0, 0), A, (1, 1, 1, 1))[2]


def test_depth_and_alt_floors_at_their_edges():
    assert position((4, 0, 4, 0), A, (8, 3, 1, 5))[2] and not position((3, 0, 4, 0), A, (8, 3, 1, 5))[2]       # T == min_depth, min_depth - 1
    assert position((9, 0, 0, 3), A, (8, 3, 1, 5))[2] and not position((9, 0, 0, 2), A, (8, 3, 1, 5))[2]       # n[alt] == min_alt, min_alt - 1
    # T counts every channel, the record's own included
    assert position((0, 3, 3, 2), A, (8, 3, 1, 5)) == (C_, 8, True)


def test_alt_ties_go_to_the_smaller_base_and_never_to_the_record():
    assert position((9, 4, 4, 4), A, DEFAULTS)[0] == C_
    assert position((9, 4, 9, 9), A, DEFAULTS)[0] == G                       # (the record's own count does not compete)
    assert position((4, 9, 4, 4), C_, DEFAULTS)[0] == A
    assert position((3, 4, 9, 9), T, DEFAULTS)[0] == G
    assert position((0, 0, 0, 0), A, DEFAULTS) == (C_, 0, False) and position((0, 0, 0, 0), T, DEFAULTS) == (A, 0, False)
    # multi-allelic: the largest of the others is reported, the record shows all four counts
    v = _sites([(10, 3, 6, 5)], b"A")
    assert tuple(v[0])[:4] == (0, 0, A, G) and v[0]["n"].tolist() == [10, 3, 6, 5]
    v = _sites([(10, 3, 6, 7)], b"g")
    assert tuple(v[0])[:4] == (0, 0, G, A)


def test_non_bases_take_no_part_and_lower_case_counts(oracle):
    oracle.lib()
    rec = b"AcNg-t"
    assert expected_recbase([rec]).tolist() == [0, 1, 4, 2, 4, 3]
    assert expected_recbase({0: b"AC", 2: b"nT"}).tolist() == [0, 1, 4, 3]
    counts = np.array([(0, 9, 0, 0)] * 6, dtype=np.uint32)                 # nine mates show C everywhere
    v = _sites(counts, rec)
    assert v["x"].tolist() == [0, 3, 5] and v["ref"].tolist() == [A, G, T] and v["alt"].tolist() == [C_] * 3
    s = expected_summary(counts, [rec], [0, 6])
    assert tuple(s[0]) == (36, 27, 4, 3)                                    # four positions take part: 4 * 9 observed, 3 * 9 differ, 4 covered
    # two genes and an id without a record
    s = expected_summary(counts, {0: rec[:2], 2: rec[2:]}, [0, 2, 2, 6])
    assert [tuple(r) for r in s] == [(18, 9, 2, 1), (0, 0, 0, 0), (18, 18, 2, 2)]
    v = expected_variants(counts, {0: rec[:2], 2: rec[2:]}, [0, 2, 2, 6])
    assert [(int(r["gene"]), int(r["x"])) for r in v] == [(0, 0), (2, 1), (2, 3)]


def test_full_counters_need_a_64_bit_total():
    n = (M32, M32, M32, M32)
    assert position(n, A, (M32, M32, 1, 4)) == (C_, 4 * M32, True)          # M32 * 4 == 1 * 4 * M32, and T >= 2^32 - 1
    assert position(n, A, (M32, M32, 16385, 65535)) == (C_, 4 * M32, False)  # 16385 / 65535 > 1 / 4
    assert position((M32, M32, 0, 0), A, (M32, 1, 1, 2))[2] and not position((M32, M32 - 1, 0, 0), A, (M32, 1, 1, 2))[2]
    s = expected_summary([n, n], [b"AC"], [0, 2], (1, 1, 1, 4))
    assert tuple(s[0]) == (8 * M32, 6 * M32, 2, 2)
    for bad in ((0, 1, 1, 5), (1, 0, 1, 5), (1, 1, 1, 0), (1, 1, 6, 5), (1, 1, 1, 65536)):
        with pytest.raises(ValueError):
            expected_variants([n], [b"A"], [0, 1], bad)


def test_variant_lines_by_hand():
    v = np.zeros(2, dtype=capi.VARIANT_DTYPE)
    v[0] = (0, 7, A, G, (12, 0, 5, 0))
    v[1] = (2, 0, T, C_, (0, 4294967295, 0, 1))
    assert variant_lines(v, ["g one", "empty", "g2"]) == ["g one 7 A G 12 0 5 0", "g2 0 T C 0 4294967295 0 1"]
    assert variant_lines(v[:0], ["g"]) == []


# ---------------------------------------------------------------------------
# the model on the example, indexed against a record with substituted bases
# ---------------------------------------------------------------------------
# record positions of the example's one gene that get another base (the next one in A, C, G, T order): seven under 26 to 341 mates, four
# where no mate lies, and base 16, which 7 mates of the sample cover on the unmutated record -- the substitution silences the 13 windows
# of 17 over it, no span reaches it any more, and it is not called for lack of depth.  The count was found with the model
SUBSTITUTED = (16, 150, 1450, 3033, 5544, 5600, 6100, 9660, 9700, 12345, 14100, 17500)
EXAMPLE_SITES = 7


def mutated_example_records():
    """[(name, record)] of the example with SUBSTITUTED applied"""
    fa = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))
    rec = bytearray(fa[0][1])
    for x in SUBSTITUTED:
        rec[x] = b"ACGT"[(b"ACGT".index(bytes([rec[x]]).upper()) + 1) % 4]
    return [(fa[0][0], bytes(rec))] + list(fa[1:])


def mutated_example_pileup(oracle, s_min=8):
    """(records, legend, gene_start, counts, mates): the model's pileup of the bundled sample over the mutated record"""
    fa = mutated_example_records()
    r1 = synth.read_fastq(os.path.join(EXAMPLE, "sample_1.fq"))
    r2 = synth.read_fastq(os.path.join(EXAMPLE, "sample_2.fq"))
    o = oracle.Shark(k=17, c=0.6, bf_bits=1 << 33)
    nidx = o.build([s for _, s in fa])
    batch = synth.batch_from_lists([s for _, s, _ in r1], [s for _, s, _ in r2])
    goff, gids = o.classify(batch["seq1"], batch["off1"], batch["seq2"], batch["off2"], None, None)
    sm = SegmentsModel([s for _, s in fa], 17)
    rows = expected_segments(sm, batch, goff, gids, 4)[1]
    counts, _, mates = expected_pileup(sm, batch, goff, gids, rows, s_min)
    return [s for _, s in fa], [n.decode() for n, _ in fa], model_layout(sm, nidx), counts, mates


def test_the_example_shows_exactly_the_substituted_bases_it_covers(oracle):
    records, legend, gs, counts, mates = mutated_example_pileup(oracle)
    original = synth.read_fasta(os.path.join(EXAMPLE, "ENSG00000277117.fa"))[0][1]
    v = expected_variants(counts, records, gs)
    # the sample was simulated from the unmutated record without errors: a site is a substituted base, its alt the original base, and
    # a substituted base is a site iff its own pileup reaches the thresholds
    reach = [x for x in SUBSTITUTED if position(counts[x], b"ACGT".index(records[0][x:x + 1]), DEFAULTS)[2]]
    print("example: mates", mates, "sites", v["x"].tolist(), "depth at the substituted bases", [int(counts[x].sum()) for x in SUBSTITUTED])
    assert (v["gene"] == 0).all() and v["x"].tolist() == reach
    for r in v:
        x = int(r["x"])
        assert "ACGT"[int(r["alt"])] == chr(original[x]) and "ACGT"[int(r["ref"])] == chr(records[0][x])
        assert int(r["n"][int(r["ref"])]) == 0 and int(r["n"][int(r["alt"])]) == int(r["n"].sum()) >= 8
    assert len(v) == EXAMPLE_SITES and 0 < EXAMPLE_SITES < len(SUBSTITUTED)
    s = expected_summary(counts, records, gs)
    assert int(s[0]["sites"]) == EXAMPLE_SITES and int(s[0]["observed"]) == int(counts.sum())
    assert int(s[0]["mismatches"]) == sum(int(counts[x].sum()) for x in SUBSTITUTED)
    assert len(variant_lines(v, legend)) == EXAMPLE_SITES and variant_lines(v, legend)[0].startswith("ENSG00000277117 %d " % reach[0])


# ---------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------
NEW = ("shk_ref_keep_bases", "shk_pileup_add", "shk_variants_get", "shk_variants_summary")


def test_header_declares_and_binding_binds_the_new_calls():
    text = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    assert "/* ---- variants:" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    for s in ("shk_variant_params", "shk_variant", "shk_gene_variants"):
        assert re.search(r"\}\s*%s\s*;" % s, hdr), s
    from shark_amd import EXPORTS, SharkHip
    assert set(NEW) <= set(EXPORTS)
    for name in ("keep_bases", "pileup_add", "variants", "variants_summary"):
        assert callable(getattr(SharkHip, name))
    assert "recbase" in SharkHip.DEBUG_ARRAYS
    assert capi.VARIANT_DTYPE.itemsize == 32 and capi.GENE_VARIANTS_DTYPE.itemsize == 24
    import inspect
    assert "keep_bases" in inspect.signature(SharkHip.build).parameters
    assert os.path.exists(LIB), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    import ctypes as C
    lib = C.CDLL(LIB)
    for s in NEW:
        assert hasattr(lib, s), s


def test_cli_flags():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "-j4", "all"], check=True, stdout=subprocess.DEVNULL)
    run = lambda *a: subprocess.run([CLI, "-r", "x.fa", "-1", "y.fq"] + list(a), capture_output=True, text=True)  # noqa: E731
    for flag, value in (("--variants-min-support", "8"), ("--variants-min-depth", "8"), ("--variants-min-alt", "3"), ("--variants-min-frac", "1/5")):
        r = run(flag, value)
        assert r.returncode == 1 and "need --variants FILE" in r.stderr, flag
    for flag in ("--variants-min-support", "--variants-min-depth", "--variants-min-alt"):
        r = run("--variants", "v", flag, "0")
        assert r.returncode == 1 and flag + " must be at least 1" in r.stderr, flag
    for frac in ("6/5", "1/0", "1/65536", "1", "1/", "/5", "-1/5", "1/5x", "0.2"):
        r = run("--variants", "v", "--variants-min-frac", frac)
        assert r.returncode == 1 and "--variants-min-frac must be P/Q" in r.stderr, frac
    r = run("--variants", "v", "--pileup", "p", "--pileup-min-support", "3")
    assert r.returncode == 1 and "must be equal" in r.stderr
    r = run("--variants", "v", "--pileup", "p", "--variants-min-support", "3")
    assert r.returncode == 1 and "must be equal" in r.stderr
    r = run("--variants")
    assert r.returncode == 1 and "unknown argument" in r.stderr           # (a missing FILE)
    # accepted as far as the arguments go: the run then fails on its inputs
    r = run("--variants", "v", "--pileup", "p", "--pileup-min-support", "3", "--variants-min-support", "3", "--variants-min-frac", "0/1", "--variants-min-depth", "1")
    assert r.returncode == 1 and "must be" not in r.stderr and "need" not in r.stderr
    assert not os.path.exists("v") and not os.path.exists("p")
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--variants FILE", "--variants-min-support N", "--variants-min-depth N", "--variants-min-alt N", "--variants-min-frac P/Q"):
        assert flag in r.stderr, flag
    # pileup's own messages as they were
    r = run("--pileup-min-support", "8")
    assert r.returncode == 1 and "--pileup-min-support needs --pileup FILE" in r.stderr
