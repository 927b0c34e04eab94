"""Staging arithmetic (stage_bases.hpp: stage8 / stage16 / gather8) on the CPU, through shark_amd/bin/shark-stage-check: every byte
value 0..255 at every position of a 16-base and of an 8-base chunk, in 64 random contexts each, at every shift 0..3 of the alignbyte
front, plus chunks of one value, all-valid chunks in upper, lower and mixed case and random bytes -- both stream words and the
validity bits equal the word-at-a-time form with multiplies that the kernels ran before (the tool carries its own copy) and a
byte-by-byte definition; the header's two forms (the default and the one asked for by name) agree as well."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "shark_amd", "bin", "shark-stage-check")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "../bin/shark-stage-check"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


def run(tool, *args):
    p = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True)
    return p.returncode, json.loads(p.stdout)


@pytest.mark.parametrize("seed", [1, 2026])
def test_every_byte_value_at_every_position_and_shift(tool, seed):
    rc, r = run(tool, 64, seed)
    # 4 shifts x (256 values x N positions x 64 contexts + 256 one-value chunks + 4 x 4096 others)
    assert r["contexts"] == 64 and r["stage_mul"] == 0, r
    assert r["chunks16"] == 4 * (256 * 16 * 64 + 256 + 4 * 4096) and r["chunks8"] == 4 * (256 * 8 * 64 + 256 + 4 * 4096), r
    assert r["diff_mul"] == 0 and r["diff_bytes"] == 0 and r["diff_base_code"] == 0 and r["diff_gather8"] == 0 and r["diff_forms"] == 0, r
    assert rc == 0
