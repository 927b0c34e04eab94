"""exclusive_scan_u32 and radix_sort_u64 on the device against the exact host models of tests/primitives_model.py, case table by
case table, through the test-only entry points shk_debug_scan_u32 / shk_debug_sort_u64 (SharkHip.debug_scan_u32 / debug_sort_u64).
Every device buffer lies between guard bands inside its own allocation; the entry points count the guard words that changed.

Exact equality throughout.  A failure names the case, the first differing index, the tile / thread-run / lane it falls in and the
expected and actual values there."""
import numpy as np
import pytest

from shark_amd import SharkHip
from tests import primitives_model as pm

pytestmark = pytest.mark.gpu

SCAN_GROUPS = pm.scan_groups()
SORT_GROUPS = pm.sort_groups()


@pytest.fixture(scope="module")
def ctx():
    h = SharkHip(k=17, c=0.6, bf_bits=1 << 16, device=0)      # (no index is built: the entry points work in any mode)
    yield h
    h.close()


def _guards(name, names, guards):
    bad = {k: int(v) for k, v in zip(names, guards) if v}
    assert not bad, "%s: guard words changed (band: count): %s" % (name, bad)


def _scan_id(g):
    n, io, oo, ip = g
    return "%s-in%d-%s" % ("n%d" % n if n else "small", io, "inplace" if ip else "out%d" % oo)


@pytest.mark.parametrize("group", list(SCAN_GROUPS), ids=_scan_id)
def test_scan(ctx, group):
    for c in SCAN_GROUPS[group]:
        name = pm.scan_case_name(c)
        a, want, want_total = pm.scan_expected(c.n, c.values)
        out, total, after, guards = ctx.debug_scan_u32(a, c.in_off, c.out_off, c.in_place)
        _guards(name, ctx.DEBUG_SCAN_GUARDS, guards)
        msg = pm.scan_mismatch(c, "out", want, out)
        assert msg is None, msg
        assert total == want_total, "%s: total 0x%x, expected 0x%x" % (name, total, want_total)
        msg = pm.scan_mismatch(c, "in afterwards", want if c.in_place else a, after)
        assert msg is None, msg


def test_scan_groups_cover_the_table():
    assert sum(len(v) for v in SCAN_GROUPS.values()) == len(pm.SCAN_CASES)
    assert sum(len(v) for v in SORT_GROUPS.values()) == len(pm.SORT_CASES) and list(SORT_GROUPS) == list(pm.SORT_END_BITS)


@pytest.mark.parametrize("end_bit", list(SORT_GROUPS))
def test_sort(ctx, end_bit):
    for c in SORT_GROUPS[end_bit]:
        name = pm.sort_case_name(c)
        keys = pm.sort_case_keys(c)
        want, want_buf = pm.sort_model(keys, c.end_bit)
        got, buf, guards = ctx.debug_sort_u64(keys, c.end_bit)
        _guards(name, ctx.DEBUG_SORT_GUARDS, guards)
        msg = pm.sort_mismatch(c, want, got)
        assert msg is None, msg
        assert buf == want_buf, "%s: result in buffer %d, expected %d (%d passes)" % (name, buf, want_buf, pm.sort_passes(c.end_bit))
        if c.n == 0:
            assert buf == 0, name
