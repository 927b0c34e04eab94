"""The two stages of the k-mer keyed table's lookup (kmer_table.hpp: kxtab_candidate, kxtab_confirm) on the CPU, through
shark_amd/bin/shark-kxtab-check: among the adversarial non-keys of every key -- the values that land on the key's own slot with
another tag -- the ones that differ from it in the tag's bits 16 and 17 alone pass the 16-bit candidate stage, three per key, and the
confirm stage has to turn every one of them down; and for every probe the tool makes, keys included, candidate-and-confirm is the
one-call kxtab_lookup."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "shark_amd", "bin", "shark-kxtab-check")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "../bin/shark-kxtab-check"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


@pytest.mark.parametrize("n", [1, 1000, 40000])
def test_the_confirm_stage_turns_down_what_the_candidate_stage_lets_through(tool, n):
    r = json.loads(subprocess.run([tool, "random", str(n), "23", "200000", "0"], check=True, capture_output=True, text=True).stdout)
    assert r["built"] and r["keys"] == n and r["missing"] == 0, r
    # per key: the three values on its slot whose tag differs in the bits 16 and 17 (less the few that are keys themselves); the
    # random probes and the one-bit flips add chance agreements of 16 bits (about 2 in 100 000 probes)
    assert 3 * n - 8 <= r["candidate_non_keys"] <= 3 * n + 200 + r["flip_probes"] // 5000, r
    assert r["two_stage_diff"] == 0, r
    assert r["false_pos"] == 0 and r["false_neg"] == 0 and r["flip_false_pos"] == 0 and r["slot_false_pos"] == 0, r
