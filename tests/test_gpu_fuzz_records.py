"""The randomised differential test of the record modes (tests/fuzz_records.py) as part of the `-m gpu` suite: a fixed-seed schedule of
cases with every mode on at once -- evidence, candidates, placement, segments, alignments with closure, extension and spliced ends,
rescue, pairs, depth or spliced depth, the junction table, owned or aligned pileup, variants, indels (at alignments mode's floor, at
another, or without alignments mode) -- through one of the four entry families, every record kind byte for byte and every accumulator
element for element against the models.  No tolerances.

tests/test_fuzz_records_cpu.py asserts, with the models alone, what this schedule covers; the last test here asserts on the device
that both repair paths and every entry family ran, indels mode among the modes.  The three wide cases take the second trip of the
stride loops of the kernels that run one wave per read (a) and one thread per read (b: the depth accumulators; c: indel_kernel).

Measured on an MI355X: MEASURED below.

Run on the GPU box with `pytest -m gpu`."""
import pytest

from tests import fuzz_records as fz

pytestmark = pytest.mark.gpu

# (bias, first seed, cases): chosen with the models alone until tests/test_fuzz_records_cpu.py's coverage conditions held
SCHEDULE = [("", 20261021, 36), ("splice", 20270021, 18), ("rescue", 20280021, 18), ("tie", 20290026, 12), ("indel", 20320076, 18)]
WIDE_A_SEED, WIDE_B_SEED, WIDE_C_SEED = 20300021, 20310021, 20330021
PER_TEST = 6
# MEASURED on an MI355X, both in one session, the file's share as the sum of its tests inside the suite's run: before indels mode and the
# `indel` bias 24.7 s of 767 s (19 of 1 317 tests); with them 31.6 s of 765 s (23 of 1 321 tests: the chunk with the overflow batch, now
# primed, 6.0 s, wide case (a) 5.4 + 3.6 + 2.4 s, wide case (b) 0.5 s, wide case (c) 0.9 s, every other test under 2.5 s), most of it
# the models on the CPU.  The file adds about 4 % to the suite

CHUNKS = [(bias, seed0 + at, min(PER_TEST, count - at)) for bias, seed0, count in SCHEDULE for at in range(0, count, PER_TEST)]
FACTS = {}       # (bias, seed) -> what run() reports of the case, for the last test


def run_case(oracle, bias, seed):
    if (bias, seed) not in FACTS:
        case = fz.draw(seed, bias)
        want = fz.expected(case, oracle)
        bad, facts = fz.run(case, oracle, want)
        assert not bad, "MISMATCH: %s\n%s" % (fz.describe(case), bad)
        facts.update(expect_overflow=want["expect_overflow"], expect_long=want["expect_long"], n=case["n"], indels=want["expect_indels"])
        FACTS[(bias, seed)] = facts
    return FACTS[(bias, seed)]


@pytest.mark.parametrize("bias,seed0,count", CHUNKS)
def test_fuzz_records(oracle, bias, seed0, count):
    for seed in range(seed0, seed0 + count):
        run_case(oracle, bias, seed)


WIDE_A = {}      # the case and what its variants share of the models' work (the associations, placements, segments, records per floor)


@pytest.mark.parametrize("pileup,ends", [("owned", "paired"), ("aligned", "paired"), ("aligned", "single-end")])
def test_wide_a_second_trip_of_the_wave_per_read_kernels(oracle, pileup, ends):
    """2 048 x PL_WAVES + 65 pairs of 60 to 100 bases from two spliced genes: placement_kernel, segments_kernel at m = 4, pileup_kernel
    and align_kernel (extension and spliced ends on) take a second trip for the reads from 8 192 on, whose mates no read of the first
    trip holds.  Owned pileup on one context, aligned pileup on a second, and the same batch once more single-end; the whole batch goes
    through the models"""
    if not WIDE_A:
        WIDE_A.update(case=fz.draw(WIDE_A_SEED, "wide"), memo={})
    case = WIDE_A["case"]
    assert case["n"] == fz.WIDE_A_PAIRS > fz.PL_MAX_BLOCKS * fz.PL_WAVES
    changes = {} if pileup == "owned" else {"pileup": ("aligned", case["modes"]["al_floor"])}
    if ends == "single-end":
        changes["single_end"] = True
    v = fz.variant(case, **changes)
    bad, facts = fz.run(v, oracle, fz.expected(v, oracle, memo=WIDE_A["memo"] if v["paired"] else None))
    assert not bad, "MISMATCH (%s, %s): %s\n%s" % (pileup, ends, fz.describe(v), bad)


def test_wide_b_second_trip_of_the_thread_per_read_accumulators(oracle):
    """2 048 x 256 + 321 pairs: depth_accumulate_kernel (plain depth on one context) and spliced_accumulate_kernel (spliced depth and the
    junction table on another) take a second trip.  The batch is a block of 1 021 model-checked pairs 513 times over and a remainder of
    836 pairs of other content; the second trip's 321 reads lie wholly in the remainder (513 x 1 021 = 523 773 < 2 048 x 256).  Depth, spliced depth and the junction table are SUMS OVER MATES,
    and a mate's contribution depends on the mate and its associations alone; so the state is 513 x model(block) + model(remainder),
    the table's mate counts times 513 -- exactly.  1 021 is prime: no power-of-two stride lines the tiles up with waves or workgroups"""
    case = fz.draw_wide_depth(WIDE_B_SEED)
    want = fz.expected_wide_depth(case, oracle)
    assert want["rest_only"] > 0 and want["rest_only_spliced"] > 0
    bad = fz.run_wide_depth(case, oracle, want)
    assert not bad, "MISMATCH (wide case b, seed %d): %s" % (WIDE_B_SEED, bad)


def test_wide_c_second_trip_of_indel_kernel(oracle):
    """(b)'s shape with content of its own: 2 048 x 256 + 321 pairs, a block of 1 021 model-checked pairs 513 times over and a remainder of
    836 pairs, most of them with a planted insertion or deletion in genes with low-complexity stretches.  Alignments mode is off and
    indels mode runs at a floor of its own: align_kernel stores into the context's private array at its largest size and indel_kernel's
    lanes take a second trip for the reads from 524 288 on.  The table's counts and the seven counters are sums over mates, so the state
    is 513 x model(block) + model(remainder) -- exactly.  tests/test_fuzz_records_cpu.py asserts what the second trip's pairs show"""
    case = fz.draw_wide_indels(WIDE_C_SEED)
    want = fz.expected_wide_indels(case, oracle)
    assert len(want["tail_only"]) > 0
    bad = fz.run_wide_indels(case, oracle, want)
    assert not bad, "MISMATCH (wide case c, seed %d): %s" % (WIDE_C_SEED, bad)


def test_schedule_ran_both_repair_paths_and_every_family(oracle):
    """test_fuzz_schedule_covers_every_probe_mode's idea on the device: over the schedule the length-bound repair ran (a ticket of the
    resident family behind a bound that does not hold: timing()["last_n_long"] > 0), the overflow repair ran (more associations handed
    out than the slot's first reservation holds), each of the two at least once with indels mode on, and every entry family ran"""
    facts = [run_case(oracle, bias, seed) for bias, seed0, count in SCHEDULE for seed in range(seed0, seed0 + count)]
    long_cases = [f for f in facts if f["expect_long"] and f["family"] == "submit_device"]
    assert long_cases and all(f["last_n_long"] > 0 for f in long_cases), [(f["family"], f["last_n_long"]) for f in long_cases]
    over = [f for f in facts if f["expect_overflow"]]
    assert over and all(f["n_assoc"] > fz.slot_reserve(f["n"]) for f in over)
    # and indels mode was on in an overflow case and behind a bound that did not hold: its table was compared after both repairs
    assert any(f["indels"] for f in over) and any(f["indels"] for f in long_cases)
    assert {f["family"] for f in facts} == set(fz.FAMILIES)
    print("fuzz records: %d cases, last kernels %s" % (len(facts), sorted({f["last_kernel"] for f in facts})))
