"""CPU tests (no GPU): the oracle against the REFERENCE PROGRAM's own answers.

 * tests/golden/ref_shark_cases.npz: whole-program cases recorded from the reference CLI (main.cpp compiled in place
   against our sdsl stand-in; tests/golden/gen_ref_shark_cases.py), replayed through oracle_cli and the oracle's batch
   API -- always run, the recording needs nothing from the reference tree
 * the sdsl stand-in's rank and select against numpy (always run)
 * live, when oracle/_ref/shark_ref has been built: the reference CLI on the example truth files, a seeded random
   differential run of oracle_cli against it on fresh cases, and the repeat-rich and long-list cases of tests/repeat_refs.py
   (gene lists of 65 534 ... 70 000 entries: the oracle's inline lists and rank support were never pinned there)
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ref_cases as rc
from tests import repeat_refs as rr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHARK_REF = os.path.join(ROOT, "oracle", "_ref", "shark_ref")
STANDIN_LIB = os.path.join(ROOT, "oracle", "libsdsl_standin.so")

CASES = rc.load()
needs_ref = pytest.mark.skipif(not os.path.exists(SHARK_REF), reason="oracle/_ref/shark_ref not built (reference tree absent)")


def test_fixture_covers_the_grid():
    """the recording holds what the generator's grid promises (a damaged or truncated file fails here first)"""
    ks = {cs["k"] for cs in CASES}
    assert {1, 2, 3, 4, 5, 11, 15, 16, 17, 18, 21, 30, 31} <= ks
    bits = {cs["bf_bits"] for cs in CASES}
    assert {1, 64, 1000, 12345, (1 << 20) + 1, rc.GIB_BITS} <= bits and all((1 << e) in bits for e in range(16, 27))
    assert {0, 1, 20, 40, 93, 94, 95, 127, 128, 222, 223, 256, 300} <= {cs["q"] for cs in CASES}
    assert {float(cs["c"]) for cs in CASES} >= {0.0, 1 / 3, 0.5, 0.6, 2 / 3, 0.75, 0.9, 1.0}
    assert any(cs["single"] for cs in CASES) and any(not cs["paired"] for cs in CASES)
    assert max(len(rc.parse_fasta(cs["fasta"])) for cs in CASES) > 65536
    uniform = {}
    for cs in CASES:                                    # batches in which every mate 1 (and every mate 2) has one length
        l1 = {len(s) for _, s, _ in rc.parse_fastq(cs["fq1"])}
        l2 = {len(s) for _, s, _ in rc.parse_fastq(cs["fq2"])} if cs["paired"] else {0}
        if len(l1) == len(l2) == 1:
            uniform.setdefault(cs["paired"], set()).update(l1)
    lengths = {31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 151, 250, 300, 350, 500, 600}
    assert lengths <= uniform.get(False, set()) and lengths <= uniform.get(True, set()), uniform
    longest = {max(len(s) for _, s, _ in rc.parse_fastq(cs["fq1"])) for cs in CASES if not cs["paired"]}
    assert {64 * u + 16 + d for u in (2, 3, 4, 5, 6, 8, 10) for d in (0, 1)} <= longest   # k = 17: 64 U and 64 U + 1 slots
    per = [rc.associations(cs) for cs in CASES]
    assert sum(len(a) for p in per for a in p) == sum(cs["ssv"].count(b"\n") for cs in CASES) > 5000
    assert sum(len(a) > 1 for p in per for a in p) > 200, "ties"


@pytest.mark.parametrize("cs", CASES, ids=[cs["name"] for cs in CASES])
def test_oracle_cli_reproduces_reference_case(oracle, cs, tmp_path):
    """oracle_cli (--bf-bits for the exact filter size) gives the reference's ssv and both FASTQ files byte for byte"""
    ssv, o1, o2 = rc.run_case(oracle.CLI_PATH, cs, str(tmp_path), bits_flag="--bf-bits")
    assert ssv == cs["ssv"]
    assert o1 == cs["out1"]
    assert o2 == cs["out2"]


@pytest.mark.parametrize("cs", CASES, ids=[cs["name"] for cs in CASES])
def test_oracle_batch_api_reproduces_reference_case(oracle, cs):
    """the batch API the GPU tests compare against gives the reference's gene lists, read by read"""
    o = oracle.Shark(k=cs["k"], c=float(cs["c"]), bf_bits=cs["bf_bits"], min_quality=cs["q"], single=cs["single"])
    try:
        o.build([s for _, s in rc.parse_fasta(cs["fasta"])])
        b = rc.batch(cs)
        goff, gids = o.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"], nthreads=2)
    finally:
        o.close()
    want = rc.associations(cs)
    got = [list(map(int, gids[goff[i]:goff[i + 1]])) for i in range(len(goff) - 1)]
    assert got == want
    assert rc.render(cs, got) == (cs["ssv"], cs["out1"], cs["out2"])


# ---------------------------------------------------------------------------
# the sdsl stand-in
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 1000003])
@pytest.mark.parametrize("density", [0.0, 0.01, 0.5, 1.0])
def test_standin_rank_select_against_numpy(oracle, n, density):
    """rank(i) = ones in [0, i) for every 0 <= i <= size(), select(j) = position of the j-th one (1-based)"""
    if not os.path.exists(STANDIN_LIB):
        oracle.build()
    L = C.CDLL(STANDIN_LIB)
    L.standin_rank_select.restype = C.c_uint64
    L.standin_rank_select.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(n * 7 + int(density * 100))
    bits = (rng.random(n) < density).astype(np.uint8)
    rank = np.zeros(n + 1, np.uint64)
    sel = np.zeros(max(n, 1), np.uint64)
    ones = L.standin_rank_select(bits.ctypes.data, n, rank.ctypes.data, sel.ctypes.data)
    assert ones == int(bits.sum())
    assert np.array_equal(rank, np.concatenate([[0], np.cumsum(bits)]).astype(np.uint64))
    assert np.array_equal(sel[:ones], np.flatnonzero(bits).astype(np.uint64))


# ---------------------------------------------------------------------------
# live against the reference CLI
# ---------------------------------------------------------------------------
@needs_ref
def test_shark_ref_reproduces_example_truth(example_dir, tmp_path):
    """the stand-in is faithful on the path the reference's own truth files pin (README.md:63-69 command line)"""
    import subprocess
    o1, o2 = tmp_path / "o1.fq", tmp_path / "o2.fq"
    r = subprocess.run([SHARK_REF, "-t", "1", "-r", os.path.join(example_dir, "ENSG00000277117.fa"),
                        "-1", os.path.join(example_dir, "sample_1.fq"), "-2", os.path.join(example_dir, "sample_2.fq"),
                        "-o", str(o1), "-p", str(o2)], capture_output=True, check=True, timeout=300)
    assert r.stdout == open(os.path.join(example_dir, "ENSG00000277117.truth.ssv"), "rb").read()
    assert o1.read_bytes() == open(os.path.join(example_dir, "sharked.sample_1.truth.fq"), "rb").read()
    assert o2.read_bytes() == open(os.path.join(example_dir, "sharked.sample_2.truth.fq"), "rb").read()


FEATURES = ("ties", "revcomp", "contained", "quirk", "dirty")
SMALL_BITS = (1, 2, 64, 1000, 4093, 12345, 1 << 16, (1 << 16) + 1, 1 << 18, 999983, 1 << 20, (1 << 20) + 1)
LENGTHS = (0, 1, 16, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 150, 151, 250, 300, 600)


def _draw_case(rng, i):
    k = int(rng.choice((1, 2, 3, 4, 5, 7, 11, 15, 16, 17, 18, 21, 24, 30, 31)))
    feats = tuple(f for f in FEATURES if rng.random() < 0.35)
    genes = rc.make_genes(rng, int(rng.integers(1, 7)), 30, 400, k, feats)
    q = int(rng.choice((0, 0, 0, 1, 20, 40, 60, 93, 94, 95, 127, 128, 200, 222, 223, 256, 300, 350)))
    mq = rc.threshold(q)
    paired = bool(rng.random() < 0.5)
    lengths = tuple(int(x) for x in rng.choice(LENGTHS, 4))
    reads = rc.make_reads(rng, genes, int(rng.integers(1, 40)), k, lengths, paired, mq is not None, mq or 0,
                          cfrac=float(rng.choice((0.3, 0.5, 0.75))) if rng.random() < 0.15 else None,
                          p_edge=0.2, sub=float(rng.choice((0.0, 0.01, 0.05))))
    c = float(rng.choice((0.0, 1 / 3, 0.4, 0.5, 0.6, 2 / 3, 0.75, 0.9, 1.0)))
    return rc.case("draw%d" % i, genes, reads, k, c, q, bool(rng.random() < 0.3), int(rng.choice(SMALL_BITS)),
                   fasta_width=int(rng.choice((0, -1))), rng=rng)


@needs_ref
@pytest.mark.parametrize("seed", [101, 202, 303, 404])
def test_live_differential_oracle_against_reference(oracle, seed, tmp_path):
    """fresh seeded draws over the grid's axes (small filters), oracle_cli against the reference CLI, byte for byte"""
    rng = np.random.default_rng(seed)
    n = 0
    for i in range(1200):
        cs = _draw_case(rng, i)
        want = rc.run_case(SHARK_REF, cs, str(tmp_path), env_bits="REF_BF_BITS")
        got = rc.run_case(oracle.CLI_PATH, cs, str(tmp_path), bits_flag="--bf-bits")
        assert got == want, "case %d (k=%d c=%s q=%d -s=%d bits=%d paired=%d)" % (
            i, cs["k"], cs["c"], cs["q"], cs["single"], cs["bf_bits"], cs["paired"])
        n += 1
    assert n == 1200


@needs_ref
@pytest.mark.parametrize("name", rr.BUILDER_CASES + rr.LONG_CASES)
def test_live_repeat_and_long_list_cases(oracle, name, tmp_path):
    """one case per builder of tests/repeat_refs.py and the four long-list cases (a motif in 65 534 / 65 535 / 65 536 / 70 000 records,
    the last with a wrapped record that holds one k-mer 69 984 times): oracle_cli against the reference CLI, byte for byte"""
    cs = rr.program_case(name)
    want = rc.run_case(SHARK_REF, cs, str(tmp_path), env_bits="REF_BF_BITS", timeout=600)
    got = rc.run_case(oracle.CLI_PATH, cs, str(tmp_path), bits_flag="--bf-bits", timeout=600)
    assert got == want
    widest = max(len(a) for a in rc.associations(cs, want[0]))
    if name in rr.LONG_CASES:
        n = int(name[5:])
        assert widest == (n if n <= 65536 else 4463)      # the tie the case is for, in the reference's own output
