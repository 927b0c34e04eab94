"""CPU tests of candidates mode: the model the GPU is held to (tests/candidates_model.py) is pinned to single-gene indices of
the oracle and to the hand-derived numbers of tests/golden/handworked.json; the two entry points and the three structs are
declared, exported and bound; the `shark` command knows --candidates and --candidates-n."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import synth
from tests.candidates_model import (expected_candidates, handworked_batch, handworked_cases, joined_reads, read_map, tie_group)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
CANDIDATES_SYMBOLS = ("shk_candidates_enable", "shk_candidates_last")


@pytest.fixture(scope="module")
def built():
    """the library and the command as build() leaves them"""
    assert os.path.exists(LIB) and os.path.exists(CLI), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    return True


def shared_stretch_corpus(seed, k, n_genes=12, n_pairs=400, read_len=60):
    """genes that share stretches (every third copies half of its predecessor, two are identical twins, all carry one common
    block) and pairs cut from them: several candidates per read, and ties at the head.  Every record has a valid k-mer."""
    rng = np.random.default_rng(seed)
    genes = synth.make_genes(rng, n_genes, 150, 400, share_every=3)
    common = synth.random_seq(rng, 50)
    for g in genes[::2]:
        g[20:70] = common
    genes[5] = genes[4].copy()                          # identical twins: every read of theirs ties at the head
    batch = synth.make_reads(rng, genes, n_pairs, read_len=read_len, paired=True, on_target=0.9, sub_rate=0.02, n_rate=0.004)
    return genes, batch


# (k, bf_bits): a roomy filter, and two small ones whose collisions make candidates of genes that share no k-mer with the read
SINGLE_GENE_CONFIGS = [(17, 1 << 20), (5, 4099), (31, 1 << 14)]


@pytest.mark.parametrize("k,bf_bits", SINGLE_GENE_CONFIGS)
def test_model_against_single_gene_indices(oracle, k, bf_bits):
    """Independent of the model's own algebra: whether gene g is in a bit's list depends on g's own k-mers only, so g's (cov, nk)
    on a read equals so_analyze_read's (max, maxk) on an index of the same k and bf_bits built from g's record alone -- and g is
    a candidate iff that index hits the read at all."""
    genes, batch = shared_stretch_corpus(100 + k, k)
    o = oracle.Shark(k=k, c=0.0, bf_bits=bf_bits)
    o.build([bytes(g) for g in genes])
    reads, entries = expected_candidates(o, batch, 8)
    joined = list(joined_reads(o, batch))
    n = len(joined)
    full = [read_map(o, j)[1] for j in joined]
    alone = []
    for g in genes:
        og = oracle.Shark(k=k, c=0.0, bf_bits=bf_bits)
        og.build([bytes(g)])
        alone.append([og.analyze(j)[1:3] for j in joined])
        og.close()
    bad = 0
    for i in range(n):
        for g in range(len(genes)):
            want = alone[g][i]
            got = tuple(full[i][g][:2]) if g in full[i] else (0, 0)
            bad += got != tuple(want)
        assert reads[i, 1] == sum(1 for g in range(len(genes)) if alone[g][i][1] > 0)
    assert bad == 0, "%d (read, gene) pairs disagree with the single-gene indices" % bad
    # the corpus is not vacuous
    several = int((reads[:, 1] >= 2).sum())
    ties = sum(1 for i in range(n) if len(tie_group(entries[i])) >= 2)
    print("k=%d bf_bits=%d: %d reads, %d with >= 2 candidates, %d tie at the head, %d with > 8" % (k, bf_bits, n, several, ties, int((reads[:, 1] > 8).sum())))
    assert several * 4 >= n and ties >= 5, (several, ties, n)
    # rank order, empty slots last and all zero
    for i in range(n):
        row = entries[i]
        filled = int((row[:, 2] > 0).sum())
        assert filled == min(8, int(reads[i, 1])) and not row[filled:].any()
        keys = [(-int(c), -int(nk), int(g)) for g, c, nk in row[:filled]]
        assert keys == sorted(keys) and len(set(int(g) for g in row[:filled, 0])) == filled


@pytest.mark.parametrize("case", handworked_cases(), ids=lambda c: c["name"])
def test_model_against_the_handworked_numbers(oracle, case):
    """entry 0 is `best`, the leading tie group is `genes` (where the read passes; with --single a lone one), len is `len`"""
    o = oracle.Shark(k=case["k"], c=case["c"], bf_bits=case["bf_bits"], min_quality=case["q"], single=case["single"])
    o.build([seq.encode() for _, seq in case["fasta"]])
    reads, entries = expected_candidates(o, handworked_batch(case), 8)
    for i, r in enumerate(case["reads"]):
        assert int(reads[i, 0]) == r["len"]
        assert [int(entries[i, 0, 1]), int(entries[i, 0, 2])] == list(r["best"])
        grp = tie_group(entries[i])
        passes = bool(grp) and float(entries[i, 0, 1]) >= case["c"] * float(reads[i, 0]) and (not case["single"] or len(grp) == 1)
        assert (grp if passes else []) == list(r["genes"]), (r["id"], grp, r["genes"])
        assert (int(reads[i, 1]) == 0) == (list(r["best"]) == [0, 0])
    if case["name"].startswith("two_identical_genes_"):
        assert entries[0, :3].tolist() == [[0, 16, 8], [1, 16, 8], [0, 0, 0]] and int(reads[0, 1]) == 2


def test_model_trims_to_m_and_handles_the_empty_batch(oracle):
    genes, batch = shared_stretch_corpus(7, 5, n_pairs=40)
    o = oracle.Shark(k=5, c=0.0, bf_bits=4099)
    o.build([bytes(g) for g in genes])
    r8, e8 = expected_candidates(o, batch, 8)
    for m in (1, 2):
        rm, em = expected_candidates(o, batch, m)
        assert np.array_equal(rm, r8) and np.array_equal(em, e8[:, :m]) and em.shape == (40, m, 3)
    assert (r8[:, 1] > 8).any()                          # n_genes is the map's size, not the number of entries handed out
    empty = {"seq1": np.zeros(0, np.uint8), "off1": np.zeros(1, np.uint64), "seq2": None, "off2": None, "qual1": None, "qual2": None}
    r0, e0 = expected_candidates(o, empty, 3)
    assert r0.shape == (0, 2) and e0.shape == (0, 3, 3) and r0.dtype == e0.dtype == np.uint32


# ---- the surface: these fail on a tree without the mode ---------------------------------------------------------------------
def test_candidates_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(LIB)
    from shark_amd import EXPORTS
    for s in CANDIDATES_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), "include/shark_hip.h does not declare %s" % s
        assert hasattr(lib, s), "libsharkhip.so does not export %s" % s
        assert s in EXPORTS
    # the records' layout is part of the ABI
    assert re.search(r"#define\s+SHK_MAX_CANDIDATES\s+8\b", code)
    assert re.search(r"typedef\s+struct\s+shk_candidate\s*\{\s*uint32_t\s+gene\s*,\s*cov\s*,\s*nk\s*;\s*\}\s*shk_candidate\s*;", code)
    assert re.search(r"typedef\s+struct\s+shk_read_candidates\s*\{\s*uint32_t\s+len\s*,\s*n_genes\s*;\s*\}\s*shk_read_candidates\s*;", code)
    m = re.search(r"typedef\s+struct\s+shk_candidates\s*\{(.*?)\}\s*shk_candidates\s*;", code, flags=re.S)
    assert m and re.search(r"uint64_t\s+n\s*;\s*uint32_t\s+m\s*;\s*const\s+shk_read_candidates\s*\*\s*reads\s*;\s*const\s+shk_candidate\s*\*\s*entries\s*;", m.group(1))
    from shark_amd import SharkHip, capi
    assert callable(getattr(SharkHip, "candidates_enable")) and callable(getattr(SharkHip, "candidates_last"))
    assert capi.SHK_MAX_CANDIDATES == 8
    assert [f for f, _ in capi.ShkCandidates._fields_] == ["n", "m", "reads", "entries"] and C.sizeof(capi.ShkCandidates) == 32
    # without a context both refuse their arguments instead of touching anything
    lib.shk_candidates_enable.restype = C.c_int
    lib.shk_candidates_enable.argtypes = [C.c_void_p, C.c_uint32]
    lib.shk_candidates_last.restype = C.c_int
    lib.shk_candidates_last.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.shk_candidates_enable(None, 4) == -1 and lib.shk_candidates_last(None, None) == -1      # SHK_ERR_ARG


def test_cli_usage_lists_candidates(built):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    tail = r.stderr[r.stderr.index("MI355X build only"):]
    assert re.search(r"^\s+--candidates FILE\s", tail, flags=re.M), tail
    assert re.search(r"^\s+--candidates-n M\s", tail, flags=re.M), tail


def test_cli_candidates_is_a_known_argument(built, tmp_path):
    r = subprocess.run([CLI, "--candidates", "x", "--candidates-n", "8"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "shark : missing required files" in r.stderr and "unknown argument" not in r.stderr
    assert not (tmp_path / "x").exists()      # nothing is opened before the arguments are complete


def _tiny_inputs(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "a.fq"
    fq.write_text("@r\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    return fa, fq


@pytest.mark.parametrize("args", [["--candidates-n", "0"], ["--candidates-n", "9"], ["--candidates-n"], ["--candidates-n", "x"]],
                         ids=["zero", "nine", "no-value", "no-number"])
def test_cli_candidates_n_out_of_range_is_a_usage_error(built, tmp_path, args):
    fa, fq = _tiny_inputs(tmp_path)
    r = subprocess.run([CLI, "-r", str(fa), "-1", str(fq), "--candidates", str(tmp_path / "c.txt")] + args, capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode == 1 and "Usage: shark" in r.stderr, r.stderr
    assert "--candidates-n must be in the range [1, 8]" in r.stderr or "unknown argument" in r.stderr
    assert not (tmp_path / "c.txt").exists() and r.stdout == ""


def test_cli_candidates_n_without_candidates_is_a_usage_error(built, tmp_path):
    fa, fq = _tiny_inputs(tmp_path)
    r = subprocess.run([CLI, "-r", str(fa), "-1", str(fq), "--candidates-n", "3"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1 and "Usage: shark" in r.stderr and "--candidates-n needs --candidates" in r.stderr, r.stderr


def test_cli_candidates_file_that_cannot_be_opened(built, tmp_path):
    fa, fq = _tiny_inputs(tmp_path)
    r = subprocess.run([CLI, "-r", str(fa), "-1", str(fq), "--candidates", str(tmp_path / "no" / "such" / "dir" / "c.txt")],
                       capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1 and "cannot open the candidates file" in r.stderr and "terminate called" not in r.stderr


def test_cli_candidates_leaves_an_earlier_file_alone_when_the_inputs_are_unreadable(built, tmp_path):
    """as --evidence: the file is created only once the samples are known to be readable"""
    fa, _ = _tiny_inputs(tmp_path)
    for opt in ("--candidates", "--evidence"):
        out = tmp_path / (opt.strip("-") + ".txt")
        out.write_text("from an earlier run\n")
        r = subprocess.run([CLI, "-r", str(fa), "-1", str(tmp_path / "missing.fq"), opt, str(out)], capture_output=True, text=True, timeout=60,
                           cwd=tmp_path)
        assert r.returncode == 1 and "cannot open the sample" in r.stderr, (opt, r.stderr)
        assert out.read_text() == "from an earlier run\n"


def test_cli_candidates_ends_as_evidence_does(built, tmp_path):
    """on a machine without a GPU both options end the same way: an error exit, no result lines on stdout, the file created (the
    inputs were readable) and empty; with one, both succeed with the same stdout"""
    fa, fq = _tiny_inputs(tmp_path)
    res = {}
    for opt in ("--candidates", "--evidence"):
        out = tmp_path / (opt.strip("-") + ".out")
        r = subprocess.run([CLI, "-r", str(fa), "-1", str(fq), opt, str(out)], capture_output=True, text=True, timeout=120, cwd=tmp_path)
        assert "terminate called" not in r.stderr and "unknown argument" not in r.stderr, (opt, r.stderr)
        res[opt] = (r.returncode, r.stdout, out.exists(), out.exists() and out.read_text() == "")
    assert res["--candidates"] == res["--evidence"], res
