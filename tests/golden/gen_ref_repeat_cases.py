#!/usr/bin/env python3
"""Generates tests/golden/ref_repeat_cases.npz by running the REAL reference CLI (oracle/_ref/shark_ref, `make -C oracle ref`)
with `-t 1` on one small whole-program case per builder of tests/repeat_refs.py -- paralog families, an interspersed element,
low-complexity runs, tandem copies, the saturated neighbourhood of one minimiser, a motif shared by 300 records.  Same layout and
replay as tests/golden/ref_shark_cases.npz (tests/ref_cases.py); inputs are stored, not seeds.  The four long-list cases
(65 534 ... 70 000 records) are compared live only (tests/test_reference_shark.py): their outputs run to megabytes."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import ref_cases as rc  # noqa: E402
from tests import repeat_refs as rr  # noqa: E402

SHARK_REF = os.path.join(ROOT, "oracle", "_ref", "shark_ref")
OUT = os.path.join(HERE, "ref_repeat_cases.npz")


def main():
    assert os.path.exists(SHARK_REF), "oracle/_ref/shark_ref missing: run `make -C oracle ref`"
    cases = [rr.program_case(name) for name in rr.BUILDER_CASES]
    with tempfile.TemporaryDirectory() as d:
        for cs in cases:
            cs["ssv"], cs["out1"], cs["out2"] = rc.run_case(SHARK_REF, cs, d, env_bits="REF_BF_BITS")
    rc.save(cases, OUT)
    print("wrote %s: %d cases, %d associations, %d bytes" % (os.path.basename(OUT), len(cases), sum(cs["ssv"].count(b"\n") for cs in cases),
                                                              os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
