"""CPU tests of the evidence mode's boundary: the model the GPU is held to (tests/evidence_model.py) reproduces the
hand-derived numbers of tests/golden/handworked.json, the two entry points are declared, exported and bound, and the
`shark` command knows --evidence."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.evidence_model import expected_evidence, handworked_batch, handworked_cases, handworked_evidence, passes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "shark_amd", "libsharkhip.so")
CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
EVIDENCE_SYMBOLS = ("shk_evidence_enable", "shk_evidence_last")


@pytest.fixture(scope="module")
def built():
    """the library and the command as build() leaves them"""
    assert os.path.exists(LIB) and os.path.exists(CLI), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    return True


@pytest.mark.parametrize("case", handworked_cases(), ids=lambda c: c["name"])
def test_model_reproduces_the_handworked_numbers(oracle, case):
    """`len` and `best` of every read of every hand-worked case: the yardstick itself, against numbers derived on paper"""
    o = oracle.Shark(k=case["k"], c=case["c"], bf_bits=case["bf_bits"], min_quality=case["q"], single=case["single"])
    o.build([seq.encode() for _, seq in case["fasta"]])
    got = expected_evidence(o, handworked_batch(case))
    assert np.array_equal(got, handworked_evidence(case)), (got.tolist(), handworked_evidence(case).tolist())
    if not case["single"]:
        # ... and the rule the numbers are for: a read has genes iff its best gene passes c * len
        assert passes(got, case["c"]).tolist() == [len(r["genes"]) > 0 for r in case["reads"]]


def test_model_on_an_empty_batch(oracle):
    o = oracle.Shark(k=17, bf_bits=1 << 20)
    o.build([b"ACGTACGTACGTACGTACGTACGTACGTAAAC"])
    got = expected_evidence(o, {"seq1": np.zeros(0, np.uint8), "off1": np.zeros(1, np.uint64), "seq2": None, "off2": None, "qual1": None, "qual2": None})
    assert got.shape == (0, 3) and got.dtype == np.uint32


def test_evidence_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "shark_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(LIB)
    from shark_amd import EXPORTS
    for s in EVIDENCE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), "include/shark_hip.h does not declare %s" % s
        assert hasattr(lib, s), "libsharkhip.so does not export %s" % s
        assert s in EXPORTS
    # the records' layout is part of the ABI: three uint32_t, in this order
    assert re.search(r"typedef\s+struct\s+shk_read_evidence\s*\{\s*uint32_t\s+cov\s*,\s*nk\s*,\s*len\s*;\s*\}\s*shk_read_evidence\s*;", code)
    from shark_amd import SharkHip
    assert callable(getattr(SharkHip, "evidence_enable")) and callable(getattr(SharkHip, "evidence_last"))
    # without a context both refuse their arguments instead of touching anything
    lib.shk_evidence_enable.restype = C.c_int
    lib.shk_evidence_enable.argtypes = [C.c_void_p, C.c_int]
    lib.shk_evidence_last.restype = C.c_int
    lib.shk_evidence_last.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.shk_evidence_enable(None, 1) == -1 and lib.shk_evidence_last(None, None) == -1      # SHK_ERR_ARG


def test_cli_usage_lists_evidence(built):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    tail = r.stderr[r.stderr.index("MI355X build only"):]
    assert re.search(r"^\s+--evidence FILE\s", tail, flags=re.M), tail


def test_cli_evidence_is_a_known_argument(built, tmp_path):
    r = subprocess.run([CLI, "--evidence", "x"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "shark : missing required files" in r.stderr and "unknown argument" not in r.stderr
    assert not (tmp_path / "x").exists()      # nothing is opened before the arguments are complete


def test_cli_evidence_file_that_cannot_be_opened(built, tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGTACGTACGTACGTACGTACGT\n")
    fq = tmp_path / "a.fq"
    fq.write_text("@r\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")
    r = subprocess.run([CLI, "-r", str(fa), "-1", str(fq), "--evidence", str(tmp_path / "no" / "such" / "dir" / "e.txt")],
                       capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 1 and "cannot open the evidence file" in r.stderr and "terminate called" not in r.stderr
