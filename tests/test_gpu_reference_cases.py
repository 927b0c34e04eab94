"""GPU against the REFERENCE PROGRAM's recorded answers, with no oracle in the loop: every case of
tests/golden/ref_shark_cases.npz (recorded from the reference CLI by tests/golden/gen_ref_shark_cases.py) through the C ABI
under each probe-structure variant, host and device-resident entry points, gene lists compared read by read and in order;
the cases at 2^33 bits (`-b 1`) also through the product CLI, stdout and both FASTQ files byte for byte.

Run on the GPU box with `pytest -m gpu`."""
import os
import re

import numpy as np
import pytest

try:  # torch bundles its own HIP runtime: load it BEFORE libsharkhip so one runtime serves both
    import torch
except Exception:  # pragma: no cover
    torch = None

from tests import ref_cases as rc
from tests.gpu_fixtures import probe  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARK_CLI = os.path.join(ROOT, "shark_amd", "bin", "shark")
CASES = rc.load()


def _lists(goff, gids):
    return [list(map(int, gids[goff[i]:goff[i + 1]])) for i in range(len(goff) - 1)]


def _first_difference(got, want):
    i = next(i for i in range(len(want)) if got[i] != want[i])
    return "read %d: got %s, reference %s" % (i, got[i], want[i])


def _device_lists(h, b, max_len):
    from shark_amd.capi import hip_memcpy_dtoh
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in b.items() if v is not None}
    pt = {k: (t[k].data_ptr() if k in t else 0) for k in b}
    n = len(b["off1"]) - 1
    r = h.classify_device(n, pt["seq1"], pt["off1"], pt["seq2"], pt["off2"], pt["qual1"], pt["qual2"], max_read_len=max_len)
    goff = np.empty(n + 1, np.uint32)
    hip_memcpy_dtoh(goff, r.gene_off, goff.nbytes)
    gids = np.empty(int(r.n_assoc), np.uint16)
    if len(gids):
        hip_memcpy_dtoh(gids, r.gene_ids, gids.nbytes)
    torch.cuda.synchronize()
    return _lists(goff, gids)


_UNI = re.compile(r"classify_uni_kernel<(\d+), \d+, (?:true|false), \d+, (\w+)>")
_FAST = re.compile(r"classify_fast_kernel<(\d+), ")
ALL_U = {2, 3, 4, 5, 6, 8, 10}


def check_coverage(probe, seen):
    """the recorded cases must reach the kernel branches they are meant to judge under each probe variant.  seen: one
    (probe mode, shk_last_kernel, reads sent to the general kernel) per host-side batch"""
    modes = {m for m, _, _ in seen}
    uni = {(int(x.group(1)), x.group(2)) for _, k, _ in seen for x in [_UNI.search(k)] if x}
    fast = {int(x.group(1)) for _, k, _ in seen for x in [_FAST.search(k)] if x}
    assert any(n_long for _, _, n_long in seen), "no batch with reads beyond the largest specialisation"
    assert any("classify_general_kernel<wrap>" in k for _, k, _ in seen), "more than 65 536 genes"
    if probe in ("bitvector", "force-generic"):
        assert ALL_U <= fast, "classify_fast_kernel unrolls reached: %s" % sorted(fast)
    else:
        assert ALL_U <= {u for u, _ in uni}, "classify_uni_kernel unrolls reached: %s" % sorted(uni)
        assert {u for u, how in uni if how == "true"} >= {2, 3, 4, 5, 6, 8, 10}, "uniform batches: %s" % sorted(uni)
    if probe == "auto":
        assert {"lds-table", "table", "table-mod"} <= modes, modes
        assert any(m == "lds-table" and ", 21, true>" in k for m, k, _ in seen), "uniform batches on the exact table in LDS"
    if probe == "no-lds-table":
        assert "lds-table" not in modes and "lds-summary+table" in modes, modes
    if probe == "bitvector":
        assert modes <= {"bitvector", "bitvector-mod", "summary+bitvector"}, modes
    if probe == "ktable":
        assert "minimiser-table" in modes, modes


def test_reference_cases(probe):
    """all recorded cases, host and device-resident entry points (the device one with the true longest mate as bound); then
    whether they reached every specialisation, uniform batches, the long path and the probe structures of the variant"""
    from shark_amd import SharkHip
    seen = []
    for cs in CASES:
        want = rc.associations(cs)
        h = SharkHip(k=cs["k"], c=float(cs["c"]), bf_bits=cs["bf_bits"], min_quality=cs["q"], single=cs["single"])
        try:
            info = h.build([s for _, s in rc.parse_fasta(cs["fasta"])])
            assert info["n_records"] == len(rc.parse_fasta(cs["fasta"]))
            b = rc.batch(cs)
            got = _lists(*h.classify(b["seq1"], b["off1"], b["seq2"], b["off2"], b["qual1"], b["qual2"]))
            assert got == want, "%s (%s), classify: %s" % (cs["name"], probe, _first_difference(got, want))
            seen.append((h.probe_mode(), h.last_kernel(), int(h.timing()["last_n_long"])))
            max_len = max(int(np.diff(b[o].astype(np.int64)).max()) for o in ("off1", "off2") if b[o] is not None)
            got = _device_lists(h, b, max(max_len, 1))
            assert got == want, "%s (%s), classify_device: %s" % (cs["name"], probe, _first_difference(got, want))
        finally:
            h.close()
    check_coverage(probe, seen)


@pytest.mark.parametrize("cs", [cs for cs in CASES if cs["bf_bits"] == rc.GIB_BITS], ids=lambda cs: cs["name"])
def test_cli_reference_cases(cs, tmp_path):
    """the product CLI (-t 1, -b 1) on the recorded 2^33-bit cases: the reference's stdout and FASTQ files byte for byte"""
    ssv, o1, o2 = rc.run_case(SHARK_CLI, cs, str(tmp_path), timeout=300)
    assert ssv == cs["ssv"]
    assert o1 == cs["out1"]
    assert o2 == cs["out2"]
