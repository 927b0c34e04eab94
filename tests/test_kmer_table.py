"""The k-mer keyed exact table of a one-gene index (shark_amd/csrc/kmer_table.hpp), checked on the CPU through the host-only tool
shark_amd/bin/shark-kxtab-check: the image is built for a key set and queried with the lookup rule the kernel uses.  Every key must
be found; a million random 34-bit values must be answered exactly as a set of the keys answers them; and so must the adversarial
non-keys of every key -- the key with any one of its 34 bits flipped, and the other values that share its slot before the
displacement and its group, which land on the key's own slot and differ from it in the stored tag alone."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "shark_amd", "bin", "shark-kxtab-check")
LTAB_BYTES = 4 * (1 << 15) + 2 * (1 << 13)      # what the exact-table kernels reserve in LDS (lds_table.hpp)


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(TOOL):
        subprocess.run(["make", "-C", os.path.join(ROOT, "shark_amd", "csrc"), "../bin/shark-kxtab-check"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


def run(tool, kind, n, seed, m=1000000, shuffle=0):
    return json.loads(subprocess.run([tool, kind, str(n), str(seed), str(m), str(shuffle)], check=True, capture_output=True, text=True).stdout)


def exact(r):
    assert r["missing"] == 0 and r["false_pos"] == 0 and r["false_neg"] == 0, r
    assert r["flip_false_pos"] == 0 and r["slot_false_pos"] == 0, r
    assert r["slots_used"] == r["keys"], r            # (no stored entry equals the empty encoding, no two keys share a slot)


@pytest.fixture(scope="module")
def capacity(tool):
    r = run(tool, "random", 1, 1, m=0)
    assert r["bytes"] <= LTAB_BYTES, r
    assert 43000 <= r["capacity"] <= 46000, r
    return r["capacity"]


@pytest.mark.parametrize("n", [1, 100, 20000, 40000, "capacity"])
def test_every_key_is_found_and_nothing_else(tool, capacity, n):
    n = capacity if n == "capacity" else n
    for seed in (1, 2, 3):     # (about one pair of multipliers in five works for 40 000 keys: several sets, several retries)
        r = run(tool, "random", n, 100 * seed + 7)
        assert r["built"] and r["keys"] == n, r
        exact(r)
        assert r["flip_probes"] >= 33 * n and r["slot_probes"] >= 30 * n and r["probes"] == 1000000, r


def test_one_key_more_than_the_capacity_is_refused(tool, capacity):
    assert run(tool, "random", capacity, 5, m=1000)["built"]
    assert not run(tool, "random", capacity + 1, 5, m=1000)["built"]


@pytest.mark.parametrize("kind", ["polya", "repeat"])
@pytest.mark.parametrize("n", [300, 3000, 30000])
def test_low_complexity_keys_are_exact_or_refused(tool, kind, n):
    """overlapping 17-mers of poly-A / of an AC repeat with a substitution every few dozen bases: few distinct keys, all close to one
    another (the key 0 among them) -- whatever the builder makes of them, never a wrong answer"""
    for seed in (1, 2):
        r = run(tool, kind, n, seed)
        assert 0 < r["keys"] <= n, r
        if r["built"]:
            exact(r)


def test_the_image_depends_on_the_set_alone(tool):
    a, b, c = (run(tool, "random", 30000, 11, m=1000, shuffle=s) for s in (0, 5, 6))
    assert a["built"] and a["image_hash"] == b["image_hash"] == c["image_hash"], (a, b, c)
    assert (a["m1"], a["m2"]) == (b["m1"], b["m2"]) == (c["m1"], c["m2"])
    assert run(tool, "random", 30000, 12, m=1000)["image_hash"] != a["image_hash"]
