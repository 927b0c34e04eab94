"""The yardstick for shk_evidence_last: per read (pair) of a batch the three numbers the reference decides from
(ReadAnalyzer.hpp:90-104), computed by the CPU oracle -- FastqSplitter's join and quality mask (so_join_mask), then
ReadAnalyzer::operator() on the joined string (so_analyze_read, which returns max, maxk and len whether or not the read
passes c * len or --single).  Test infrastructure only."""
import ctypes as C
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_evidence(oracle_shark, batch):
    """oracle_shark: an oracle.pyoracle.Shark with its index built; batch: the SoA dict of tests/synth.py.
    Returns an (n, 3) uint32 array: cov (max), nk (maxk), len."""
    from oracle import pyoracle
    L = pyoracle.lib()
    off1 = np.ascontiguousarray(batch["off1"], dtype=np.uint64)
    n = len(off1) - 1
    paired = batch.get("seq2") is not None
    off2 = np.ascontiguousarray(batch["off2"], dtype=np.uint64) if paired else None
    s1 = bytes(np.ascontiguousarray(batch["seq1"], dtype=np.uint8)) if n else b""
    s2 = bytes(np.ascontiguousarray(batch["seq2"], dtype=np.uint8)) if paired else b""
    q1 = bytes(np.ascontiguousarray(batch["qual1"], dtype=np.uint8)) if batch.get("qual1") is not None else None
    q2 = bytes(np.ascontiguousarray(batch["qual2"], dtype=np.uint8)) if (paired and batch.get("qual2") is not None) else None
    mq = int(oracle_shark.min_quality) & 0xFF                       # the reference's `char min_quality` (argument_parser.hpp:144)
    if mq and q1 is None:
        raise ValueError("the oracle masks by quality (-q %d) and the batch has none" % oracle_shark.min_quality)
    out = np.zeros((n, 3), dtype=np.uint32)
    for i in range(n):
        a, b = int(off1[i]), int(off1[i + 1])
        m1, k1 = s1[a:b], (q1[a:b] if q1 is not None else None)
        m2, k2 = None, None
        if paired:
            a2, b2 = int(off2[i]), int(off2[i + 1])
            m2, k2 = s2[a2:b2], (q2[a2:b2] if q2 is not None else None)
        buf = C.create_string_buffer(len(m1) + (len(m2) if paired else 0) + 2)
        m = L.so_join_mask(m1, len(m1), k1, m2, len(m2) if paired else 0, k2, int(paired), bytes([mq]), buf)
        _, mx, mk, ln = oracle_shark.analyze(buf.raw[:m])
        out[i] = (mx, mk, ln)
    return out


def passes(evidence, c):
    """which reads have associations at confidence c (without --single): ReadAnalyzer.hpp:104 in the same double arithmetic"""
    ev = np.asarray(evidence)
    return (ev[:, 1] > 0) & (ev[:, 0].astype(np.float64) >= np.float64(c) * ev[:, 2].astype(np.float64))


# ---- tests/golden/handworked.json: the cases as batches, and the file's own numbers as evidence records ----
def handworked_cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "handworked.json")))["cases"]


def handworked_batch(case):
    from tests import synth
    paired = case["reads"][0]["m2"] is not None
    m1 = [r["m1"].encode() for r in case["reads"]]
    q1 = [r["q1"].encode() for r in case["reads"]]
    m2 = [r["m2"].encode() for r in case["reads"]] if paired else None
    q2 = [r["q2"].encode() for r in case["reads"]] if paired else None
    return synth.batch_from_lists(m1, m2, q1, q2)


def handworked_evidence(case):
    """the file's own numbers: cov, nk, len per read"""
    return np.array([[r["best"][0], r["best"][1], r["len"]] for r in case["reads"]], dtype=np.uint32).reshape(-1, 3)
